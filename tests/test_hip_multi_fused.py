"""-m gpu: the multi-person renderer's batch body as ONE C call (include/neuman_hip.h: nm_render_rays_multi / _live; render_utils.
render_multi_rays_fused) against the step-by-step body (render_multi_rays with a trace): the same kernels up to the merge, and a merge that is
bit-identical whatever the number of actors, so rgb and depth are torch.equal.  The 40 x 32 'multi' capture of tests/helpers/posed_scene.py,
actors shifted as tests/test_hip_sizes.py SHIFTS; 16 + 16 background and 16 human samples unless a case says otherwise."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import posed_scene as PS  # noqa: E402
from test_hip_sizes import SHIFTS, several_bodies  # noqa: E402

pytestmark = pytest.mark.gpu

OUT_OF_VIEW = (40.0, 0.0, 0.0)                                     # a body 40 units to the side: no ray of the capture comes near it


@pytest.fixture(scope="module")
def M():
    from neuman_hip import _lib, ray_utils, render_utils, synthetic, vanilla
    g = PS.load()
    c = PS.cap(g, 'multi')
    o, d = (torch.as_tensor(x).cuda().contiguous() for x in PS.frame_rays(c))
    assert o.shape[0] == PS.W * PS.H
    nets = types.SimpleNamespace(coarse=synthetic.make_joiner(0).cuda(), fine=synthetic.make_joiner(1).cuda(), human=synthetic.make_joiner(2, 'rotate').cuda(),
                                 human2=synthetic.make_joiner(1, 'posenc', preset='opaque').cuda())
    for n_ in vars(nets).values():
        assert n_.precision == 'mixed'                             # (the composited passes run i8x3, the last background sample is re-evaluated)
    return types.SimpleNamespace(lib=_lib, ray=ray_utils, R=render_utils, vanilla=vanilla, g=g, cap=c, o=o, d=d, nets=nets,
                                 faces=np.ascontiguousarray(g['faces'][:, :3], np.int32), cache={})


def actors(M, shifts):
    """-> (human nets, posed vertices on the device, meshes) of one actor per shift (the nets alternate)"""
    posed, T = M.g['posed_verts'], M.g['T']
    verts, meshes, humans = [], [], []
    for i, s in enumerate(shifts):
        v = (posed + np.array(s, np.float32)).astype(np.float32)
        t = T.copy()
        t[:, :3, 3] += np.array(s)
        verts.append(torch.as_tensor(v).cuda())
        meshes.append(M.ray.mesh_to_device(v, M.faces, t, 'cuda'))
        humans.append(M.nets.human if i % 2 == 0 else M.nets.human2)
    return humans, verts, meshes


def stepwise(M, shifts, S=16, N=16, fine=True, white=True, precision=None, o=None, d=None):
    """render_multi_rays with a trace: the step-by-step path -> ((rgb, depth), trace); computed once per case"""
    key = (tuple(shifts), S, N, fine, white, precision, None if o is None else o.shape[0])
    if key not in M.cache:
        humans, verts, meshes = actors(M, shifts)
        trace = {}
        out = M.R.render_multi_rays(M.nets.coarse, M.nets.fine if fine else None, humans, M.o if o is None else o, M.d if d is None else d, M.cap.near['bkg'],
                                    M.cap.far['bkg'], verts, meshes, S, N, white, 0.2, precision, trace=trace)
        M.cache[key] = (out, trace)
    return M.cache[key]


def fused(M, shifts, S=16, N=16, fine=True, white=True, precision=None, o=None, d=None, live=None):
    humans, verts, meshes = actors(M, shifts)
    return M.R.render_multi_rays_fused(M.nets.coarse, M.nets.fine if fine else None, humans, M.o if o is None else o, M.d if d is None else d, M.cap.near['bkg'],
                                       M.cap.far['bkg'], verts, meshes, S, N, white, 0.2, precision, live=live)


def equal(a, b):
    assert len(a) == len(b) == 2
    for x, y, what in zip(a, b, ("rgb", "depth")):
        assert x.shape == y.shape and torch.isfinite(x).all() and torch.equal(x, y), (what, float((x - y).abs().max()) if x.numel() else 0.0)


def entry_calls(M, mp):
    """counts the calls the host mirror makes of the library's merge and fused multi entries"""
    calls = {}
    L = M.lib.lib()
    for name in ('nm_render_rays_multi', 'nm_render_rays_multi_live', 'nm_merge_composite_lists', 'nm_merge_composite_lists_wide', 'nm_merge_sorted'):
        def wrapped(*a, _f=getattr(L, name), _n=name):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a)
        mp.setattr(L, name, wrapped)
    return calls


@pytest.mark.parametrize("S,N,A", [(16, 16, 1), (16, 16, 2), (16, 16, 3), (16, 16, 4), (16, 16, 5), (64, 64, 3), (64, 64, 5)])
def test_fused_batch_is_bit_identical_to_the_step_by_step_body(M, monkeypatch, S, N, A):
    ref, trace = stepwise(M, SHIFTS[:A], S, N)
    calls = entry_calls(M, monkeypatch)
    equal(fused(M, SHIFTS[:A], S, N), ref)
    # ONE call, and no host-side merge beside it (the call merges inside: nm_merge_composite_lists up to three actors, the wide kernel beyond)
    assert calls == {'nm_render_rays_multi': 1}
    hits = [int(h.numel()) for h in trace['hit']]
    assert len(hits) == A and all(0 < h < M.o.shape[0] for h in hits)
    if A >= 2:
        assert several_bodies(trace, M.o.shape[0], A) > 0


def test_scene_with_overlapping_bodies_missed_rays_and_an_actor_out_of_view(M):
    shifts = list(SHIFTS[:5])
    shifts[2] = OUT_OF_VIEW
    ref, trace = stepwise(M, shifts)
    R = M.o.shape[0]
    cnt = torch.zeros(R, dtype=torch.int64)
    for h in trace['hit']:
        cnt[h.long().cpu()] += 1
    assert int((cnt >= 2).sum()) > 0, "no ray goes through two bodies"
    assert int((cnt == 0).sum()) > 0, "no ray misses everybody"
    assert trace['hit'][2].numel() == 0 and all(trace['hit'][a].numel() > 0 for a in (0, 1, 3, 4)), "actor 2 is not the only one without hits"
    equal(fused(M, shifts), ref)


def test_all_actors_out_of_view_no_actor_and_no_ray(M):
    away = [(40.0 + 3 * i, 0.0, 0.0) for i in range(4)]
    ref, trace = stepwise(M, away)
    assert all(h.numel() == 0 for h in trace['hit'])
    equal(fused(M, away), ref)
    equal(fused(M, away[:2]), stepwise(M, away[:2])[0])
    equal(fused(M, []), stepwise(M, [])[0])                        # A = 0: the background alone
    e = torch.empty((0, 3), device='cuda')
    for shifts in ([], SHIFTS[:2], SHIFTS[:5]):                    # R = 0
        out = fused(M, shifts, o=e, d=e)
        assert out[0].shape == (0, 3) and out[1].shape == (0,)
        equal(out, stepwise(M, shifts, o=e, d=e)[0])


@pytest.mark.parametrize("A", [2, 5])
def test_coarse_only_background_black_background_and_float_precision(M, A):
    equal(fused(M, SHIFTS[:A], fine=False, N=0), stepwise(M, SHIFTS[:A], fine=False, N=0)[0])       # fine=None, N = 0
    equal(fused(M, SHIFTS[:A], white=False), stepwise(M, SHIFTS[:A], white=False)[0])
    a = stepwise(M, SHIFTS[:A], precision='fp16x3')[0]                                                # no last-sample re-evaluation ...
    equal(fused(M, SHIFTS[:A], precision='fp16x3'), a)
    b = stepwise(M, SHIFTS[:A])[0]                                                                    # ... and the default 'mixed', which has it
    equal(fused(M, SHIFTS[:A]), b)
    assert not torch.equal(a[0], b[0])


@pytest.mark.parametrize("A", [3, 5])
def test_several_batches_equal_one(M, monkeypatch, A):
    ref = stepwise(M, SHIFTS[:A])[0]
    monkeypatch.setattr(M.R, 'FUSED_MULTI_RAYS', 500)
    calls = entry_calls(M, monkeypatch)
    equal(fused(M, SHIFTS[:A]), ref)
    assert calls['nm_render_rays_multi'] == 3                      # 1280 rays in batches of 500


@pytest.mark.parametrize("A", [2, 5])
def test_workspace_is_used_within_its_stated_size(M, monkeypatch, A):
    """a sentinel behind the nm_render_rays_multi_workspace_floats floats of the workspace is untouched, whatever the workspace held before"""
    ref = stepwise(M, SHIFTS[:A])[0]
    made = []

    def guarded_ws(n_floats, device):
        n = max(int(n_floats), 4)
        t = torch.full((n + 4096,), 7.25, device=device, dtype=torch.float32)
        made.append((t, n))
        return t
    monkeypatch.setattr(M.R, '_ws', guarded_ws)
    out = fused(M, SHIFTS[:A])
    torch.cuda.synchronize()
    assert len(made) == 1
    t, n = made[0]
    assert n == int(M.lib.lib().nm_render_rays_multi_workspace_floats(M.o.shape[0], 16, 16, 16, A))
    assert bool((t[n:] == 7.25).all()), "the call wrote past the size it states"
    equal(out, ref)


@pytest.mark.parametrize("A", [2, 5])
def test_live_entry_equals_the_plain_one(M, monkeypatch, A):
    """LIVE_HEADS with vanilla.LIVE_MIN_SAMPLES patched to 0 (the scene's passes are small): nm_render_rays_multi_live -- the colour head on the live
    samples of the composited passes only -- gives the plain entry's rgb and depth bit for bit"""
    monkeypatch.setattr(M.vanilla, 'LIVE_MIN_SAMPLES', 0)
    plain = fused(M, SHIFTS[:A], live=False)
    monkeypatch.setattr(M.R, 'LIVE_HEADS', True)
    calls = entry_calls(M, monkeypatch)
    on = fused(M, SHIFTS[:A])
    assert calls.get('nm_render_rays_multi_live') == 1 and calls.get('nm_render_rays_multi', 0) == 0
    equal(on, plain)
    equal(plain, stepwise(M, SHIFTS[:A])[0])


@pytest.mark.parametrize("A", [3, 5])
def test_frame_renderer_with_the_switch_on_returns_the_same_frame(M, monkeypatch, A):
    """render_hybrid_nerf_multi_persons with MULTI_FUSED on = off, bit for bit; on, the frame is one nm_render_rays_multi call"""
    net = types.SimpleNamespace(coarse_bkg_net=M.nets.coarse, fine_bkg_net=M.nets.fine, coarse_human_net=M.nets.human, parameters=M.nets.coarse.parameters)
    posed, T = M.g['posed_verts'], M.g['T']
    posed_l = [(posed + np.array(s, np.float32)).astype(np.float32) for s in SHIFTS[:A]]
    T_l = []
    for s in SHIFTS[:A]:
        t = T.copy()
        t[:, :3, 3] += np.array(s)
        T_l.append(t)

    def frame():
        return M.R.render_hybrid_nerf_multi_persons(net, M.cap, [net] * A, posed_l, [M.faces] * A, T_l, samples_per_ray=16, importance_samples_per_ray=16,
                                                    geo_threshold=0.2, return_depth=True)
    monkeypatch.setattr(M.R, 'MULTI_FUSED', False)
    calls = entry_calls(M, monkeypatch)
    off = frame()
    assert calls.get('nm_render_rays_multi', 0) == 0
    monkeypatch.setattr(M.R, 'MULTI_FUSED', True)
    on = frame()
    assert calls.get('nm_render_rays_multi') == 1
    assert on[0].shape == (PS.H, PS.W, 3) and np.isfinite(on[0]).all()
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])


def test_fused_route_gives_way_to_every_hook_it_does_not_serve(M, monkeypatch):
    """with the switch on, a trace, a replay (`given`), early termination, an occupancy grid on a background or an actor's net, and actors whose
    nets run at different precisions still take the step-by-step body; the plain call takes the fused one"""
    from neuman_hip import occupancy, synthetic
    monkeypatch.setattr(M.R, 'MULTI_FUSED', True)
    calls = entry_calls(M, monkeypatch)
    humans, verts, meshes = actors(M, SHIFTS[:2])
    args = (M.nets.coarse, M.nets.fine, humans, M.o, M.d, M.cap.near['bkg'], M.cap.far['bkg'], verts, meshes, 16, 16, True, 0.2)

    def fused_calls():
        return calls.get('nm_render_rays_multi', 0) + calls.get('nm_render_rays_multi_live', 0)
    a = M.R.render_multi_rays(*args, None, {})                                     # a trace
    assert fused_calls() == 0
    b = M.R.render_multi_rays(*args)
    assert fused_calls() == 1
    equal(a, b)
    equal(M.R.render_multi_rays(*args, None, None, {}), a)                         # a replay dict (nothing recorded in it: everything is derived)
    assert fused_calls() == 1
    with monkeypatch.context() as mp:                                              # early termination
        mp.setattr(M.R, 'TERMINATION_EPS', 1e-4)
        t = M.R.render_multi_rays(*args)
        assert fused_calls() == 1 and torch.isfinite(t[0]).all() and float((t[0] - a[0]).abs().max()) < 3e-4     # (1 + actors) eps
    verts_c, _ = synthetic.capsule_mesh()
    full = torch.ones(16, 16, 16, dtype=torch.bool)
    for net, box in ((M.nets.coarse, occupancy.canonical_aabb(M.g['posed_verts'], 10.0)), (M.nets.human, occupancy.canonical_aabb(verts_c, 0.1))):
        occupancy.attach(net, occupancy.OccupancyGrid.from_mask(box, full, device='cuda'))
        try:
            g_ = M.R.render_multi_rays(*args)
        finally:
            occupancy.detach(net)
        assert fused_calls() == 1 and torch.isfinite(g_[0]).all()
    with monkeypatch.context() as mp:                                              # the actors' nets at two precisions
        mp.setattr(M.nets.human2, 'precision', 'fp16x3')
        p_ = M.R.render_multi_rays(*args)
        assert fused_calls() == 1
        equal(p_, M.R.render_multi_rays(*args, None, {}))
        with pytest.raises(M.lib.NeumanHipError, match="one precision"):
            M.R.render_multi_rays_fused(*args)
    equal(M.R.render_multi_rays(*args), a)                                         # and the plain call is the fused one again
    assert fused_calls() == 2
    with pytest.raises(M.lib.NeumanHipError, match="render_multi_rays_fused"):     # a shape the merge cannot stage, asked for directly
        fused(M, SHIFTS[:4], 2000, 2000)
