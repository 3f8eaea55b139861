"""The marched background passes as one C call (nm_march_pass, nm_render_rays_bkg_march, render_utils.march_pass_rays_fused behind
render_utils.MARCH_FUSED), host side: the switch is off unless asked for, bkg_place_z and bkg_shade reach the fused pass exactly when the switch is
on, the net has no grid and the pass is not on the live-heads route, and csrc/march.hip keeps the fused passes' contract -- no GPU needed."""
import inspect
import os

import pytest
import torch

from neuman_hip import _lib, occupancy, ray_utils, render_utils, synthetic

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture
def recorders(monkeypatch):
    """both march functions, the sampling and the importance step replaced by recorders: what bkg_place_z / bkg_shade route to, without a device"""
    calls = []

    def fused(net, o, d, z, eps, **kw):
        calls.append(('fused', eps, kw))
        return torch.zeros(z.shape + (4,))

    def unfused(net, o, d, z, eps, **kw):
        calls.append(('march', eps, kw))
        return torch.zeros(z.shape + (4,))

    monkeypatch.setattr(render_utils, 'march_pass_rays_fused', fused)
    monkeypatch.setattr(render_utils, 'march_pass_rays', unfused)
    monkeypatch.setattr(ray_utils, 'sample_z', lambda o, d, near, far, S, *a, **k: (None, None, torch.zeros(o.shape[0], S)))
    monkeypatch.setattr(ray_utils, 'importance_z_from_raw', lambda raw, z, d, N, want_weights=False: (torch.zeros(z.shape[0], z.shape[1] + N), None))
    return calls


def rays(n=4):
    return torch.zeros(n, 3), torch.ones(n, 3), torch.zeros(n), torch.ones(n)


def full_grid():
    return occupancy.OccupancyGrid.from_mask(((0, 0, 0), (1, 1, 1)), torch.ones(8, 8, 8, dtype=torch.bool))


def test_switch_is_off_unless_asked_for():
    assert "NEUMAN_MARCH_FUSED" not in os.environ                        # (the suite runs with the variable unset)
    assert render_utils.MARCH_FUSED is False


def test_switch_off_never_reaches_the_fused_pass(recorders, monkeypatch):
    net = synthetic.make_joiner(1, preset='opaque')
    o, d, near, far = rays()
    monkeypatch.setattr(render_utils, 'TERMINATION_EPS', 1e-4)
    for live in (False, True):
        monkeypatch.setattr(render_utils, 'LIVE_HEADS', live)
        for composite_only in (False, True):
            render_utils.bkg_shade(net, o, d, torch.zeros(4, 8), composite_only=composite_only)
            render_utils.bkg_place_z(net, net, o, d, near, far, 8, 8, True, composite_only=composite_only)
            render_utils.bkg_pass_rays(net, None, o, d, near, far, 8, 0, True, composite_only=composite_only)
    assert len(recorders) == 12 and all(c[0] == 'march' for c in recorders)


def test_switch_on_without_termination_marches_nothing(recorders, monkeypatch):
    net = synthetic.make_joiner(1, preset='opaque')
    whole = []
    monkeypatch.setattr(net, 'forward_rays', lambda o, d, z, **kw: whole.append(kw) or torch.zeros(z.shape + (4,)))
    o, d, near, far = rays()
    monkeypatch.setattr(render_utils, 'MARCH_FUSED', True)
    monkeypatch.setattr(render_utils, 'TERMINATION_EPS', 0.0)
    render_utils.bkg_shade(net, o, d, torch.zeros(4, 8))
    render_utils.bkg_place_z(net, net, o, d, near, far, 8, 8, True)
    assert recorders == [] and len(whole) == 2


def test_switch_on_takes_the_fused_pass(recorders, monkeypatch):
    net = synthetic.make_joiner(1, preset='opaque')
    o, d, near, far = rays()
    monkeypatch.setattr(render_utils, 'MARCH_FUSED', True)
    monkeypatch.setattr(render_utils, 'TERMINATION_EPS', 1e-4)
    occl, dz = (torch.ones(4), torch.ones(4)), torch.ones(4, 8)
    render_utils.bkg_shade(net, o, d, torch.zeros(4, 8), precision='i8x3', occluder=occl, dz=dz)
    kind, eps, kw = recorders.pop()
    assert kind == 'fused' and eps == 1e-4 and kw['occluder'] is occl and kw['dz'] is dz and kw['role'] == 'shading' and kw['precision'] == 'i8x3'
    assert 'grid' not in kw and 'adaptive' not in kw
    # the coarse pass of a two-net render: density only, at TERMINATION_COARSE
    trace = {}
    render_utils.bkg_place_z(net, net, o, d, near, far, 8, 8, True, trace=trace)
    kind, eps, kw = recorders.pop()
    assert kind == 'fused' and eps == render_utils.TERMINATION_COARSE and kw['sigma_only'] is True and kw['role'] is None
    assert kw['stats'] is trace['march_coarse'][0]
    # composite_only without LIVE_HEADS is the whole-network launch: fused
    render_utils.bkg_shade(net, o, d, torch.zeros(4, 8), composite_only=True)
    assert recorders.pop()[0] == 'fused'
    # the single-net pass is left to bkg_shade
    trace = {}
    render_utils.bkg_pass_rays(net, None, o, d, near, far, 8, 0, True, trace=trace)
    assert [c[0] for c in recorders] == ['fused'] and recorders[0][2]['stats'] is trace['march'][0]


def test_switch_on_falls_through_on_the_live_heads_route(recorders, monkeypatch):
    net = synthetic.make_joiner(1, preset='opaque')
    o, d, near, far = rays()
    monkeypatch.setattr(render_utils, 'MARCH_FUSED', True)
    monkeypatch.setattr(render_utils, 'TERMINATION_EPS', 1e-4)
    monkeypatch.setattr(render_utils, 'LIVE_HEADS', True)
    render_utils.bkg_shade(net, o, d, torch.zeros(4, 8), composite_only=True)
    kind, _, kw = recorders.pop()
    assert kind == 'march' and kw['role'] == 'composite' and kw['grid'] is None
    render_utils.bkg_shade(net, o, d, torch.zeros(4, 8), composite_only=False)          # not a composite-only caller: 'shading', fused
    assert recorders.pop()[0] == 'fused'
    render_utils.bkg_place_z(net, net, o, d, near, far, 8, 8, True, composite_only=True)   # the coarse pass is never on the live route
    assert recorders.pop()[0] == 'fused'


def test_switch_on_falls_through_with_a_grid(recorders, monkeypatch):
    net, bare = synthetic.make_joiner(1, preset='opaque'), synthetic.make_joiner(0, preset='opaque')
    o, d, near, far = rays()
    monkeypatch.setattr(render_utils, 'MARCH_FUSED', True)
    monkeypatch.setattr(render_utils, 'MARCH_WITH_GRID', True)
    monkeypatch.setattr(render_utils, 'TERMINATION_EPS', 1e-4)
    grid = full_grid()
    occupancy.attach(net, grid)
    try:
        render_utils.bkg_shade(net, o, d, torch.zeros(4, 8))
        kind, _, kw = recorders.pop()
        assert kind == 'march' and kw['grid'] is grid
        render_utils.bkg_place_z(net, bare, o, d, near, far, 8, 8, True)
        kind, _, kw = recorders.pop()
        assert kind == 'march' and kw['grid'] is grid and kw['sigma_only'] is True
        # a grid on the other net of the pair does not keep this one off the fused pass
        render_utils.bkg_place_z(bare, net, o, d, near, far, 8, 8, True)
        assert recorders.pop()[0] == 'fused'
        render_utils.bkg_shade(bare, o, d, torch.zeros(4, 8))
        assert recorders.pop()[0] == 'fused'
    finally:
        occupancy.detach(net)


def test_fused_pass_takes_the_marchs_arguments_less_adaptive_and_grid():
    march = list(inspect.signature(render_utils.march_pass_rays).parameters.values())
    fused = list(inspect.signature(render_utils.march_pass_rays_fused).parameters.values())
    assert [(p.name, p.default) for p in fused] == [(p.name, p.default) for p in march if p.name not in ('adaptive', 'grid')]


def test_entries_are_bound_and_declared():
    with open(os.path.join(ROOT, "include", "neuman_hip.h")) as f:
        header = f.read()
    for name in ("nm_march_pass", "nm_march_pass_workspace_floats", "nm_render_rays_bkg_march", "nm_render_rays_bkg_march_workspace_floats"):
        assert name in _lib.SIGNATURES and name + "(" in header
        restype, argtypes = _lib.SIGNATURES[name]
        fn = getattr(_lib.lib(), name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert len(_lib.SIGNATURES["nm_march_pass"][1]) == 19 and len(_lib.SIGNATURES["nm_render_rays_bkg_march"][1]) == 26
    lib = _lib.lib()
    # an empty batch needs nothing; the sizes grow with R alone (one march) and hold the coarse pass's arrays (two nets)
    assert lib.nm_march_pass_workspace_floats(0) == 0 and lib.nm_render_rays_bkg_march_workspace_floats(0, 64, 64) == 0
    assert lib.nm_march_pass_workspace_floats(5) % 4 == 0 and lib.nm_march_pass_workspace_floats(5) >= 3 * 5
    one, two = lib.nm_render_rays_bkg_march_workspace_floats(100, 16, 0), lib.nm_render_rays_bkg_march_workspace_floats(100, 16, 16)
    assert one >= lib.nm_march_pass_workspace_floats(100) + 600 and two >= one + 100 * 16 * 5


def test_march_source_keeps_the_fused_passes_contract():
    """no allocation, no host synchronisation, no copy: the text of csrc/march.hip"""
    with open(os.path.join(ROOT, "ml-neuman_amd", "csrc", "march.hip")) as f:
        src = f.read()
    for word in ("hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy("):
        assert word not in src, word
    assert "nm_march_pass" in src and "nm_render_rays_bkg_march" in src
