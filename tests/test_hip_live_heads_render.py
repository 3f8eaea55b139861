"""-m gpu: the colour head on live samples only in every composited pass of the renderers (render_utils.LIVE_HEADS; the composite-only rule
there): each renderer's outputs with the switch on are torch.equal to its outputs with the switch off -- a sample whose stored density is <= 0
has weight exactly 0 in raw2outputs and in every merged composite -- and the route is really taken: a *_live entry of the library is called,
and the passes' raw carries a colour on fewer samples than it evaluated.  24 x 16 rays on the capsule scene of tests/test_hip_occupancy_human.py,
background 16 + 16 samples, human 16, 'mixed' precision (the composited passes run i8x3)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

S, N = 16, 16
LIVE_ENTRIES = ['nm_mlp_forward_rays_live', 'nm_mlp_forward_live', 'nm_mlp_forward_listed_live', 'nm_mlp_forward_samples_live', 'nm_mlp_forward_ray_chunk_live',
                'nm_render_rays_bkg_live', 'nm_render_rays_human_live', 'nm_render_rays_human_occ_live', 'nm_render_rays_hybrid_live']
NEW_ENTRIES = [e for e in LIVE_ENTRIES if e != 'nm_mlp_forward_rays_live']        # (render_vanilla's plain route predates the switch)


@pytest.fixture(scope="module")
def M():
    from neuman_hip import _lib, occupancy, ray_utils, render_utils, synthetic, vanilla
    dev = torch.device('cuda')
    verts_c, faces = synthetic.capsule_mesh(20, 24)
    posed, T = synthetic.twist_transforms(verts_c)
    cap = synthetic.SimpleCapture(24, 16, fx=1.6 * 24, c2w=synthetic.spherical_c2w(40., 0., 3.0))
    o, d = render_utils._pixel_rays(cap, dev)
    assert o.shape[0] == 24 * 16
    posed_t = torch.from_numpy(posed).to(dev)
    posed2 = (posed_t + torch.tensor([0.3, 0.0, 0.1], device=dev)).contiguous()
    # (the human net: seed 1 with the posenc encoding, whose sigma > 0 set covers about half of the canonical box -- the rotate-encoded seed-2 net of
    # tests/test_hip_occupancy_human.py is positive in every cell, which leaves the colour head nothing to skip)
    nets = types.SimpleNamespace(coarse=synthetic.make_joiner(0).to(dev), fine=synthetic.make_joiner(1).to(dev),
                                 human=synthetic.make_joiner(1, 'posenc', preset='opaque').to(dev), human2=synthetic.make_joiner(4, 'rotate', preset='opaque').to(dev))
    for n_ in vars(nets).values():
        n_.precision = 'mixed'
    return types.SimpleNamespace(lib=_lib, occ=occupancy, ray=ray_utils, render=render_utils, syn=synthetic, vanilla=vanilla, dev=dev, o=o, d=d, nets=nets,
                                 can=torch.from_numpy(verts_c).to(dev), posed=posed_t, posed2=posed2, mesh=ray_utils.mesh_to_device(posed, faces, T, dev),
                                 mesh2=ray_utils.mesh_to_device(posed2.cpu().numpy(), faces, T, dev), box=occupancy.canonical_aabb(verts_c, 0.1))


def mask_grid(M, seed, box=None, p=0.5, res=16):
    g = torch.Generator().manual_seed(seed)
    return M.occ.OccupancyGrid.from_mask(M.box if box is None else box, torch.rand(res, res, res, generator=g) < p, device=M.dev)


class Spy:
    """counts the calls of the library's *_live entries and, of every pass whose raw the renderers hold in Python, the samples it evaluated
    (a non-zero record) and the samples that carry a colour (where the colour head ran)"""

    def __init__(self, M, mp):
        self.calls, self.evaluated, self.coloured = {}, 0, 0
        L = M.lib.lib()
        for name in LIVE_ENTRIES:
            mp.setattr(L, name, self._count(name, getattr(L, name)))
        for name in ('human_pass_rays', 'human_march_rays', 'bkg_shade'):
            mp.setattr(M.render, name, self._watch(getattr(M.render, name)))

    def _count(self, name, fn):
        def wrapped(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return wrapped

    def _watch(self, fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            raw = out[0] if isinstance(out, tuple) else out
            self.evaluated += int((raw != 0).any(-1).sum())
            self.coloured += int((raw[..., :3] != 0).any(-1).sum())
            return out
        return wrapped

    def new_calls(self):
        return sum(self.calls.get(e, 0) for e in NEW_ENTRIES)


def ab(M, monkeypatch, render, fused=False):
    """render() with LIVE_HEADS off, then on under the spy: equal outputs, the route taken"""
    monkeypatch.setattr(M.vanilla, 'LIVE_MIN_SAMPLES', 0)                          # (the scene's passes are small)
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(M.render, 'LIVE_HEADS', False)
        off_spy = Spy(M, mp)
        off = render()
    assert off_spy.new_calls() == 0
    assert fused or (off_spy.evaluated > 0 and off_spy.coloured == off_spy.evaluated)
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(M.render, 'LIVE_HEADS', True)
        spy = Spy(M, mp)
        on = render()
    print(f"[live render] calls {spy.calls}; colour head on {spy.coloured} of {spy.evaluated} evaluated samples")
    assert spy.new_calls() >= 1
    if not fused:                                                                  # (the fused call keeps its raw to itself: see the stepwise test below)
        assert spy.evaluated == off_spy.evaluated and 0 < spy.coloured < spy.evaluated
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())
    return spy


def renderers(M):
    n = M.nets
    return {
        'smpl_posed': lambda: M.render.render_smpl_nerf_rays(n.human, M.o, M.d, M.posed, M.mesh, S, True, False, 0.2, 1.0),
        'smpl_canonical': lambda: M.render.render_smpl_nerf_rays(n.human, M.o, M.d, M.can, None, S, True, True, 0.2, 1.0),
        'hybrid_fused': lambda: M.render.render_hybrid_rays(n.coarse, n.fine, n.human, M.o, M.d, 0.0, 3.14, M.posed, M.mesh, S, N, True, 0.2),
        'hybrid_trace': lambda: M.render.render_hybrid_rays(n.coarse, n.fine, n.human, M.o, M.d, 0.0, 3.14, M.posed, M.mesh, S, N, True, 0.2, None, {}),
        'multi': lambda: M.render.render_multi_rays(n.coarse, n.fine, [n.human, n.human2], M.o, M.d, 0.0, 3.14, [M.posed, M.posed2], [M.mesh, M.mesh2], S, N, True,
                                                    0.2),
    }


CASES = ['smpl_posed', 'smpl_canonical', 'hybrid_fused', 'hybrid_trace', 'multi']


@pytest.mark.parametrize("case", CASES)
def test_plain(M, monkeypatch, case):
    ab(M, monkeypatch, renderers(M)[case], fused=case == 'hybrid_fused')


@pytest.mark.parametrize("case", CASES)
def test_with_a_grid_on_the_human_net(M, monkeypatch, case):
    M.occ.attach(M.nets.human, mask_grid(M, 1))
    M.occ.attach(M.nets.human2, mask_grid(M, 9, p=0.3))
    try:
        spy = ab(M, monkeypatch, renderers(M)[case])                               # (a human grid: the fused call gives way to the unfused passes)
        assert spy.calls.get('nm_render_rays_human_occ_live', 0) >= 1
    finally:
        M.occ.detach(M.nets.human)
        M.occ.detach(M.nets.human2)


@pytest.mark.parametrize("case", CASES)
def test_with_termination(M, monkeypatch, case):
    monkeypatch.setattr(M.render, 'TERMINATION_EPS', 1e-3)
    spy = ab(M, monkeypatch, renderers(M)[case])
    if case != 'smpl_canonical':                                                   # (the canonical render is never marched)
        assert spy.calls.get('nm_mlp_forward_live', 0) >= 1                        # human_march_rays' chunks
    if case.startswith('hybrid'):
        assert spy.calls.get('nm_mlp_forward_ray_chunk_live', 0) >= 1              # the marched background pass
    if case == 'multi':
        assert spy.calls.get('nm_mlp_forward_ray_chunk_live', 0) == 0              # the exclusion: its last sample's colours tell "never reached"


def test_render_vanilla_with_a_grid_on_both_nets(M, monkeypatch):
    n = M.nets
    box = M.occ.rays_aabb(M.o, M.d, 0.0, 3.14)
    M.occ.attach(n.coarse, mask_grid(M, 5, box))
    M.occ.attach(n.fine, mask_grid(M, 6, box))
    try:
        spy = ab(M, monkeypatch, lambda: M.render.render_vanilla_rays(n.coarse, n.fine, M.o, M.d, 0.0, 3.14, S, N, True))
        assert spy.calls.get('nm_mlp_forward_samples_live', 0) >= 1
    finally:
        M.occ.detach(n.coarse)
        M.occ.detach(n.fine)


def test_hybrid_live_call_equals_the_stepwise_passes(M, monkeypatch):
    """nm_render_rays_hybrid_live (render_hybrid_rays_fused) = render_hybrid_rays' per-batch sequence of calls (trace: the step-by-step path), bit
    for bit, with the switch on and off and against each other; hits and misses in one batch; and with one background net, no fine pass"""
    monkeypatch.setattr(M.vanilla, 'LIVE_MIN_SAMPLES', 0)
    n = M.nets
    for fine, n_imp in ((n.fine, N), (None, 0)):
        outs = {}
        for live in (False, True):
            monkeypatch.setattr(M.render, 'LIVE_HEADS', live)
            with monkeypatch.context() as mp, torch.no_grad():
                spy = Spy(M, mp)
                outs[live, 'steps'] = M.render.render_hybrid_rays(n.coarse, fine, n.human, M.o, M.d, 0.0, 3.14, M.posed, M.mesh, S, n_imp, True, 0.2, None, {})
                assert spy.calls.get('nm_render_rays_hybrid_live', 0) == 0
                outs[live, 'fused'] = M.render.render_hybrid_rays_fused(n.coarse, fine, n.human, M.o, M.d, 0.0, 3.14, M.posed, M.mesh, S, n_imp, True, 0.2)
                assert spy.calls.get('nm_render_rays_hybrid_live', 0) == (1 if live else 0)
        ref = outs[False, 'steps']
        assert float(ref[2].max()) > 0 and float((ref[2] == 0).float().mean()) > 0.1
        for key, got in outs.items():
            for x, y, what in zip(got, ref, ("rgb", "depth", "acc")):
                assert torch.equal(x, y), (key, what)


def test_direct_calls_keep_whole_network_records(M, monkeypatch):
    """human_pass_rays, human_march_rays and bkg_shade called outside a renderer's body return what they always did"""
    monkeypatch.setattr(M.vanilla, 'LIVE_MIN_SAMPLES', 0)
    with torch.no_grad():
        near, far = M.ray.geometry_guided_near_far(M.o, M.d, M.posed, 0.2)
        h = M.ray.compact_hits(near, far)[0].long()
        ho, hd, hn, hf = M.o[h].contiguous(), M.d[h].contiguous(), near[h].contiguous(), far[h].contiguous()
        with monkeypatch.context() as mp:
            spy = Spy(M, mp)
            raw, _ = M.render.human_pass_rays(M.nets.human, ho, hd, hn, hf, S, M.mesh, False, 1.0)
            raw_m, _ = M.render.human_march_rays(M.nets.human, ho, hd, hn, hf, S, M.mesh, 0.0)
            assert not spy.calls and spy.coloured == spy.evaluated
        assert torch.equal(raw, raw_m)
        monkeypatch.setattr(M.render, 'LIVE_HEADS', True)
        with M.render.raw_composited_only(raw[..., 0].numel(), M.dev):
            live, _ = M.render.human_pass_rays(M.nets.human, ho, hd, hn, hf, S, M.mesh, False, 1.0)
    dead = raw[..., 3] <= 0
    assert 0 < int(dead.sum()) < dead.numel()                                      # both classes of sample
    assert torch.equal(live[..., 3], raw[..., 3]) and torch.equal(live[..., :3][~dead], raw[..., :3][~dead]) and (live[..., :3][dead] == 0).all()


@pytest.mark.parametrize("n_imp", [N, 0])
def test_bkg_live_call_zeroes_the_colours_of_dead_samples(M, n_imp):
    """nm_render_rays_bkg_live against nm_render_rays_bkg (two passes, and one net alone): the body the fused hybrid call runs its background pass
    through, whose raw that call keeps to itself -- same z, same densities, the live samples' colours equal, the others exactly 0 (so the colour head
    did not run on them), rgb / depth / acc equal"""
    L, P, n = M.lib.lib(), M.lib.dev_ptr, M.nets
    fine = n.fine if n_imp else None
    R = M.o.shape[0]
    near, far = torch.zeros(R, device=M.dev), torch.full((R,), 3.14, device=M.dev)
    t_vals = torch.linspace(0., 1., steps=S, device=M.dev)
    u = torch.linspace(0., 1., steps=n_imp, device=M.dev) if n_imp else None
    pc, pf = n.coarse._prec(None, None if fine is not None else 'shading'), fine._prec(None, 'shading') if fine is not None else 0
    assert (pf if n_imp else pc) == M.lib.NM_PREC_I8X3
    outs = []
    for live in (False, True):
        ws = torch.empty(int(L.nm_render_rays_bkg_workspace_floats(R, S, n_imp)) + 4, device=M.dev)
        raw, z = torch.full((R, S + n_imp, 4), 7.0, device=M.dev), torch.empty((R, S + n_imp), device=M.dev)
        rgb, depth, acc = torch.empty((R, 3), device=M.dev), torch.empty(R, device=M.dev), torch.empty(R, device=M.dev)
        head = (n.coarse.handle(), fine.handle() if fine is not None else None, P(M.o), P(M.d), P(near), P(far), R, S, n_imp, P(t_vals), P(u), 1, pc, pf, P(ws), P(raw),
                P(z), P(rgb), P(depth), P(acc))
        if live:
            nbytes = L.nm_mlp_live_workspace_bytes(R * (S + n_imp), 0)
            lws = torch.empty(nbytes, device=M.dev, dtype=torch.uint8)
            M.lib.check(L.nm_render_rays_bkg_live(*head, P(lws, torch.uint8), nbytes, 0, M.lib.stream_ptr()), "nm_render_rays_bkg_live")
        else:
            M.lib.check(L.nm_render_rays_bkg(*head, M.lib.stream_ptr()), "nm_render_rays_bkg")
        outs.append((raw, z, rgb, depth, acc))
    (raw0, z0, *c0), (raw1, z1, *c1) = outs
    dead = raw0[..., 3] <= 0
    assert 0 < int(dead.sum()) < dead.numel() and bool((raw0[..., :3][dead] != 0).any())
    assert torch.equal(z0, z1) and torch.equal(raw0[..., 3], raw1[..., 3]) and torch.equal(raw0[..., :3][~dead], raw1[..., :3][~dead])
    assert (raw1[..., :3][dead] == 0).all()
    for a, b in zip(c0, c1):
        assert torch.equal(a, b)
