"""Early ray termination together with an occupancy grid in the background passes (render_utils.MARCH_WITH_GRID, march_pass_rays grid=,
nm_occ_compact_ray_chunk), host side: the entry is exported and bound, its argument errors are reported before any device work, the switch is
off unless asked for and the combination is then refused as before -- no GPU needed."""
import ctypes
import inspect
import os

import pytest
import torch

from neuman_hip import _lib, occupancy, render_utils, synthetic

ENTRY = "nm_occ_compact_ray_chunk"
P = ctypes.c_void_p(16)                                # a non-null pointer no refusal may dereference


def call(bits=P, res=8, box=(0, 0, 0, 1, 1, 1), o=P, d=P, z=P, R=4, S_total=8, ray_idx=None, n_dev=None, n_rays=4, s0=0, S=8, idx=P, counts=P, ws=P):
    box_c = (ctypes.c_float * 6)(*box) if box is not None else None
    return _lib.lib().nm_occ_compact_ray_chunk(bits, res, box_c, o, d, z, R, S_total, ray_idx, n_dev, n_rays, s0, S, idx, counts, ws, None)


def test_entry_is_exported_and_bound():
    assert ENTRY in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    assert len(argtypes) == 17
    fn = getattr(_lib.lib(), ENTRY)
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "neuman_hip.h")) as f:
        assert "int nm_occ_compact_ray_chunk(const uint32_t* bits, int res, const float* aabb," in f.read()


@pytest.mark.parametrize("what,kw", [
    ("null bits", dict(bits=None)),
    ("null box", dict(box=None)),
    ("null counts", dict(counts=None)),
    ("null workspace", dict(ws=None)),
    ("null origin", dict(o=None)),
    ("null direction", dict(d=None)),
    ("null z", dict(z=None)),
    ("null sample_idx", dict(idx=None)),
    ("res below 4", dict(res=0)),
    ("res above 256", dict(res=260)),
    ("res not a multiple of 4", dict(res=6)),
    ("empty box", dict(box=(0, 0, 0, 1, 0, 1))),
    ("box not finite", dict(box=(0, 0, 0, 1, float('inf'), 1))),
    ("box NaN", dict(box=(float('nan'), 0, 0, 1, 1, 1))),
    ("S < 1", dict(S=0)),
    ("s0 < 0", dict(s0=-1, S=4)),
    ("s0 + S > S_total", dict(s0=1, S=8)),
    ("s0 + S overflows an int", dict(s0=2 ** 31 - 1, S=8)),
    ("R * S_total >= 2^31", dict(R=1 << 20, S_total=1 << 11, S=8, ray_idx=P)),
    ("n_rays * S >= 2^31", dict(R=4, S_total=1 << 11, S=1 << 11, n_rays=1 << 20, ray_idx=P)),
    ("negative n_rays", dict(n_rays=-1)),
    ("more rays than given without ray_idx", dict(R=4, n_rays=5)),
])
def test_argument_errors_name_the_entry(what, kw):
    assert call(**kw) == -1, what
    assert ENTRY.encode() in _lib.lib().nm_last_error(), what


def test_switch_is_off_unless_asked_for():
    assert "NEUMAN_MARCH_WITH_GRID" not in os.environ                    # (the suite runs with the variable unset)
    assert render_utils.MARCH_WITH_GRID is False


def test_switch_off_still_refuses_and_names_the_switch(monkeypatch):
    assert render_utils.MARCH_WITH_GRID is False
    net = synthetic.make_joiner(1, preset='opaque')
    occupancy.attach(net, occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 1, 1)), torch.ones(8, 8, 8, dtype=torch.bool)))
    monkeypatch.setattr(render_utils, 'TERMINATION_EPS', 1e-3)
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    try:
        with pytest.raises(NotImplementedError, match="NEUMAN_MARCH_WITH_GRID"):
            render_utils.bkg_pass_rays(net, net, o, d, torch.zeros(4), torch.ones(4), 8, 8, True)
        with pytest.raises(NotImplementedError, match="NEUMAN_MARCH_WITH_GRID"):
            render_utils.bkg_shade(net, o, d, torch.zeros(4, 8))
    finally:
        occupancy.detach(net)


def test_switch_on_reports_the_grid_instead_of_refusing(monkeypatch):
    net = synthetic.make_joiner(1, preset='opaque')
    monkeypatch.setattr(render_utils, 'TERMINATION_EPS', 1e-3)
    monkeypatch.setattr(render_utils, 'MARCH_WITH_GRID', True)
    assert render_utils._occupancy_on(net) is False
    occupancy.attach(net, occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 1, 1)), torch.ones(8, 8, 8, dtype=torch.bool)))
    try:
        assert render_utils._occupancy_on(None, net) is True
    finally:
        occupancy.detach(net)


def test_march_takes_the_grid_as_its_last_keyword():
    params = list(inspect.signature(render_utils.march_pass_rays).parameters.values())
    assert params[-1].name == 'grid' and params[-1].default is None
    # ... behind the keywords it had: callers that pass those by position keep their meaning
    assert [p.name for p in params[:-1]] == ['net', 'o', 'd', 'z', 'eps', 'chunk', 'precision', 'role', 'stats', 'sigma_only', 'occluder', 'adaptive', 'dz']


def test_host_mirror_has_the_two_functions():
    assert list(inspect.signature(occupancy.OccupancyGrid.compact_ray_chunk).parameters) == ['self', 'o', 'd', 'z', 'ray_idx', 'n_rays_dev', 's0', 'c', 'n_rays']
    assert callable(occupancy.forward_listed_samples)
