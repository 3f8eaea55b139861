"""Occupancy grids on human nets (neuman_hip/occupancy.py, csrc/occupancy.hip, csrc/render.hip), host side: the new
entry points are declared and bound, their refusals happen before any device work, grids attach to the canonical human net of every
head the reference's options build, and the canonical box helper -- no GPU needed."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from neuman_hip import _lib, occupancy, synthetic, vanilla

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("nm_occ_compact_points", "nm_mlp_forward_listed", "nm_render_rays_human_occ_workspace_floats", "nm_render_rays_human_occ")


def test_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "neuman_hip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"{name}(" in header, name


def test_refusals_before_device_work():
    L = _lib.lib()
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    one = ctypes.c_void_p(16)
    assert L.nm_occ_compact_points(one, 6, box, None, 0, None, one, one, None) == -1
    assert b"res" in L.nm_last_error()
    assert L.nm_occ_compact_points(None, 8, box, None, 0, None, one, one, None) == -1
    assert b"nm_occ_compact_points" in L.nm_last_error()
    bad = (ctypes.c_float * 6)(0, 0, 0, 1, 0, 1)
    assert L.nm_occ_compact_points(one, 8, bad, None, 0, None, one, one, None) == -1
    assert b"box" in L.nm_last_error()
    rc = L.nm_mlp_forward_listed(None, None, None, 0, None, None, 0, _lib.NM_PREC_FP32, 1.0, None, None)
    assert rc == -1 and b"exact-f32" in L.nm_last_error()
    rc = L.nm_mlp_forward_listed(None, None, None, 4, None, None, 8, _lib.NM_PREC_FP16X3, 1.0, None, None)
    assert rc == -1 and b"nm_mlp_forward_listed" in L.nm_last_error()              # more list entries than points
    assert L.nm_render_rays_human_occ(None, None, None, None, 8, box, None, None, None, None, 0, 8, None, 1, 1.0, _lib.NM_PREC_I8X3, None, None, None,
                                      None, None, None, None, None) == -1
    assert b"nm_render_rays_human_occ" in L.nm_last_error()
    # a posed mesh without its transforms
    assert L.nm_render_rays_human_occ(None, one, None, one, 8, box, None, None, None, None, 0, 8, None, 1, 1.0, _lib.NM_PREC_I8X3, None, None, None,
                                      one, None, None, None, None) == -1


def test_workspace_holds_the_human_layout_and_the_list():
    L = _lib.lib()
    for R, S, posed in ((1000, 128, 1), (1000, 128, 0), (7, 3, 1)):
        base = L.nm_render_rays_human_workspace_floats(R, S, posed)
        occ = L.nm_render_rays_human_occ_workspace_floats(R, S, posed)
        assert occ >= base + R * S + L.nm_occ_compact_workspace_ints(R * S)


def human_nets():
    """coarse_human_net as models/human_nerf.py:26-30 builds it, for both heads (specular_can) and both canonical encodings"""
    out = []
    for spec in (True, False):
        for pe in ('rotate', 'posenc'):
            opt = synthetic.default_opt(specular_can=spec, can_posenc=pe)
            t = copy.deepcopy(opt)
            t.pos_min_freq, t.use_viewdirs, t.posenc = 0, t.specular_can, t.can_posenc
            out.append(vanilla.build_nerf(t)[0])
    return out


def test_grids_attach_to_every_human_head():
    grid = occupancy.OccupancyGrid.from_mask(((-1, -1, -1), (1, 1, 1)), torch.ones(8, 8, 8, dtype=torch.bool))
    for net in human_nets():
        occupancy.attach(net, grid)
        assert occupancy.grid_of(net) is grid
        occupancy.detach(net)
        assert occupancy.grid_of(net) is None


def test_canonical_aabb():
    v, _ = synthetic.capsule_mesh(20, 24)
    box = occupancy.canonical_aabb(v, 0.05)
    assert box.dtype == torch.float32 and box.shape == (6,)
    assert np.array_equal(box.numpy(), np.concatenate([v.min(0) - np.float32(0.05), v.max(0) + np.float32(0.05)]).astype(np.float32))
    assert np.array_equal(occupancy.canonical_aabb(torch.from_numpy(v), 0.0).numpy(), np.concatenate([v.min(0), v.max(0)]))
    with pytest.raises(ValueError):
        occupancy.canonical_aabb(v, -0.1)
    with pytest.raises(ValueError):
        occupancy.canonical_aabb(np.zeros((4, 3), np.float32), 0.0)            # a point: no extent
    with pytest.raises(ValueError):
        occupancy.canonical_aabb(np.full((4, 3), np.nan, np.float32), 0.1)
