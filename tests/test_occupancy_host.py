"""Occupancy grids (neuman_hip/occupancy.py, csrc/occupancy.hip), host side: the probe lattice restated, masks and their persistence,
and the refusals that happen before any device work -- no GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from neuman_hip import _lib, occupancy, render_utils, synthetic


def restated_offsets(probes, seed):
    """The probe offsets as include/neuman_hip.h states them: slot (k % m, k / m % m, k / m^2) of an m^3 >= probes lattice plus a
    lowbias32 jitter of (seed * 0x9e3779b9 + 3 k + axis), top 24 bits, all in float32."""
    def h(x):
        x &= 0xffffffff
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xffffffff
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xffffffff
        x ^= x >> 16
        return x
    m = 1
    while m ** 3 < probes:
        m += 1
    out = np.zeros((probes, 3), np.float32)
    for k in range(probes):
        for a, sub in enumerate((k % m, (k // m) % m, k // (m * m))):
            jit = np.float32(h(seed * 0x9e3779b9 + 3 * k + a) >> 8) * np.float32(2.0 ** -24)
            out[k, a] = (np.float32(sub) + jit) / np.float32(m)
    return out


@pytest.mark.parametrize("probes,seed", [(1, 0), (8, 0), (8, 3), (27, 1), (64, 5)])
def test_probe_offsets_restated(probes, seed):
    got = occupancy.probe_offsets(probes, seed).numpy()
    want = restated_offsets(probes, seed)
    assert np.array_equal(got, want)
    assert (got >= 0).all() and (got < 1).all()
    if probes == 8:                                   # one probe per octant of the cell
        assert len({tuple((got[k] >= 0.5).tolist()) for k in range(8)}) == 8


def test_mask_round_trip_and_state_dict():
    g = torch.Generator().manual_seed(0)
    mask = torch.rand(16, 16, 16, generator=g) > 0.7
    grid = occupancy.OccupancyGrid.from_mask(((-1, -2, -3), (1, 2, 0)), mask)
    assert torch.equal(grid.to_mask(), mask)
    assert grid.occupied_fraction() == pytest.approx(mask.float().mean().item(), abs=0)
    # bit layout: cell (i, j, k) is bit (k res + j) res + i
    one = torch.zeros(16, 16, 16, dtype=torch.bool)
    one[3, 5, 7] = True
    b = occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 1, 1)), one).bits
    c = (7 * 16 + 5) * 16 + 3
    assert int(b[c >> 5]) == 1 << (c & 31) and int((b != 0).sum()) == 1
    sd = grid.state_dict()
    back = occupancy.OccupancyGrid.from_state_dict(sd)
    assert torch.equal(back.bits, grid.bits) and torch.equal(back.aabb, grid.aabb) and back.res == 16


def test_bad_grids_are_refused():
    with pytest.raises(ValueError):
        occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 1, 1)), torch.zeros(6, 6, 6, dtype=torch.bool))      # not a multiple of 4
    with pytest.raises(ValueError):
        occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 1, 1)), torch.zeros(8, 8, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 0, 1)), torch.zeros(8, 8, 8, dtype=torch.bool))      # empty box
    L = _lib.lib()
    box = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    assert L.nm_occ_compact_samples(ctypes.c_void_p(16), 6, box, None, None, None, 0, 4, None, ctypes.c_void_p(16), ctypes.c_void_p(16), None) == -1
    assert b"res" in L.nm_last_error()
    assert L.nm_occ_build(None, box, 128, 8, 1, 0.0, 0, _lib.NM_PREC_FP16X3, None, 0, None, None) == -1
    assert L.nm_occ_build_workspace_floats(128, 65) == -1
    assert L.nm_occ_build_workspace_floats(128, 8) >= 128 ** 3


def test_sample_list_launch_has_no_fp32_form():
    rc = _lib.lib().nm_mlp_forward_samples(None, None, None, None, 0, 4, None, None, 0, _lib.NM_PREC_FP32, 1.0, None, None)
    assert rc == -1 and b"exact-f32" in _lib.lib().nm_last_error()


def test_time_conditioned_net_is_refused():
    j4 = synthetic.make_variant_joiner(6, raw_pos_dim=4)
    grid = occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 1, 1)), torch.ones(8, 8, 8, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        occupancy.attach(j4, grid)
    with pytest.raises(NotImplementedError):
        occupancy.OccupancyGrid.from_net(j4, ((0, 0, 0), (1, 1, 1)), res=8)


def test_grid_with_early_termination_is_refused(monkeypatch):
    net = synthetic.make_joiner(1, preset='opaque')
    grid = occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 1, 1)), torch.ones(8, 8, 8, dtype=torch.bool))
    occupancy.attach(net, grid)
    assert occupancy.grid_of(net) is grid
    monkeypatch.setattr(render_utils, 'TERMINATION_EPS', 1e-3)
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    near, far = torch.zeros(4), torch.ones(4)
    with pytest.raises(NotImplementedError):
        render_utils.bkg_pass_rays(net, net, o, d, near, far, 8, 8, True)
    with pytest.raises(NotImplementedError):
        render_utils.bkg_shade(net, o, d, torch.zeros(4, 8))
    occupancy.detach(net)
    assert occupancy.grid_of(net) is None
