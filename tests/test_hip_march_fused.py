"""-m gpu: the marched background passes as one C call (nm_march_pass, nm_render_rays_bkg_march; render_utils.march_pass_rays_fused behind
render_utils.MARCH_FUSED).  The yardstick is the route that exists: march_pass_rays(adaptive=False, chunk=c) -- the same chunk launches with
nm_transmittance_chunk*, torch.where and nm_compact_hits over all R rays between them -- importance_z_from_raw and raw2outputs.  The MLP
arithmetic is per sample and the transmittance's is one shared device function, so every comparison is torch.equal."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

PRECISIONS = ["i8x3", "fp16x3"]
COMPACT_BLOCK = 256                                    # rays per block of the boundary's write launch (and of nm_compact_hits)
GRID_SWEEP = 8192 * 4                                  # live rays one sweep of the boundary's count launch covers: 8192 blocks of 4 waves
SENTINEL = -7.25


@pytest.fixture(scope="module")
def scene():
    from neuman_hip import _lib, ray_utils, render_utils, synthetic
    net = synthetic.make_joiner(1, preset='opaque').cuda()
    cap = synthetic.SimpleCapture(800, 800)
    o, d = ray_utils.shot_all_rays_dev(cap, torch.device('cuda'))
    sel = torch.arange(390 * 800, 390 * 800 + GRID_SWEEP + 5, device='cuda')
    return dict(net=net, o=o[sel].contiguous(), d=d[sel].contiguous(), render=render_utils, ray=ray_utils, syn=synthetic, lib=_lib, z={})


def rays(sc, R):
    return sc['o'][:R].contiguous(), sc['d'][:R].contiguous()


def near_far(R):
    return torch.zeros(R, device='cuda'), torch.full((R,), 3.14, device='cuda')


def fine_z(sc, R, S, NI):
    """the final sample positions of a two-pass render of the first R rays (NI = 0: the stratified samples); computed once per shape"""
    key = (R, S, NI)
    if key not in sc['z']:
        o, d = rays(sc, R)
        _, _, z = sc['ray'].sample_z(o, d, *near_far(R), S)
        if NI:
            z, _ = sc['ray'].importance_z_from_raw(sc['net'].forward_rays(o, d, z, sigma_only=True), z, d, NI)
        sc['z'][key] = z.contiguous()
    return sc['z'][key]


def yardstick(sc, R, z, eps, chunk, precision, **kw):
    o, d = rays(sc, R)
    stats = {}
    raw = sc['render'].march_pass_rays(sc['net'], o, d, z, eps, chunk=chunk, precision=precision, role=None, stats=stats, adaptive=False, **kw)
    return raw, stats


def fused(sc, R, z, eps, chunk, precision, **kw):
    o, d = rays(sc, R)
    stats = {}
    raw = sc['render'].march_pass_rays_fused(sc['net'], o, d, z, eps, chunk=chunk, precision=precision, role=None, stats=stats, **kw)
    return raw, stats


def assert_same(a, b):
    (raw_a, st_a), (raw_b, st_b) = a, b
    assert st_a == st_b, (st_a, st_b)
    assert torch.equal(raw_a, raw_b)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("R", [1, 3, 5, COMPACT_BLOCK + 1])
def test_ray_counts_that_leave_partial_waves_and_blocks(scene, R, precision):
    z = fine_z(scene, R, 32, 32)
    assert_same(fused(scene, R, z, 1e-4, 16, precision), yardstick(scene, R, z, 1e-4, 16, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("eps", [1e-4, 0.5])
def test_live_list_longer_than_one_grid_sweep(scene, eps, precision):
    """R = 32768 + 5, S_total = 24, chunk = 8: the boundary's waves walk more than one ray each; at eps = 0.5 a good share of the rays leaves
    the list (asserted on the yardstick's count), so the second boundary compacts a list that is no longer 0..R-1"""
    R = GRID_SWEEP + 5
    z = fine_z(scene, R, 24, 0)
    got, ref = fused(scene, R, z, eps, 8, precision), yardstick(scene, R, z, eps, 8, precision)
    print(f"[march fused] {R} rays, eps {eps:g}, {precision}: evaluated {ref[1]['evaluated']} of {ref[1]['total']}")
    assert ref[1]['launches'] == 3
    if eps == 0.5:
        assert R * 8 < ref[1]['evaluated'] < ref[1]['total']
    assert_same(got, ref)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("chunk", [100, 16, 32, 300])
def test_chunk_lengths(scene, chunk, precision):
    """S_total = 256: a short last chunk (100), 16 and 8 boundaries' worth (16, 32), and chunk > S_total (one launch, no boundary)"""
    R = 2048
    z = fine_z(scene, R, 128, 128)
    got, ref = fused(scene, R, z, 1e-4, chunk, precision), yardstick(scene, R, z, 1e-4, chunk, precision)
    assert_same(got, ref)
    assert got[1]['launches'] == -(-256 // chunk)
    if chunk > 256:
        assert got[1]['evaluated'] == got[1]['total'] == R * 256


@pytest.mark.parametrize("precision", PRECISIONS)
def test_without_termination_it_is_the_whole_launch(scene, precision):
    R = 1024
    o, d = rays(scene, R)
    z = fine_z(scene, R, 128, 128)
    raw, stats = fused(scene, R, z, 0.0, 100, precision)
    assert stats['evaluated'] == stats['total'] == z.numel()
    assert torch.equal(raw, scene['net'].forward_rays(o, d, z, precision=precision))


def test_density_only_without_termination_is_the_density_only_launch(scene):
    R = 1024
    o, d = rays(scene, R)
    z = fine_z(scene, R, 128, 0)
    raw, _ = fused(scene, R, z, 0.0, 48, 'fp16x3', sigma_only=True)
    assert torch.equal(raw, scene['net'].forward_rays(o, d, z, precision='fp16x3', sigma_only=True))
    assert_same(fused(scene, R, z, 4e-13, 48, 'fp16x3', sigma_only=True), yardstick(scene, R, z, 4e-13, 48, 'fp16x3', sigma_only=True))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mixed_survival(scene, precision):
    """eps = 1e-4 on the opaque preset: some rays are cut early, some never -- the premise is asserted, on the yardstick's own count"""
    R = 4096
    z = fine_z(scene, R, 128, 128)
    got, ref = fused(scene, R, z, 1e-4, 32, precision), yardstick(scene, R, z, 1e-4, 32, precision)
    print(f"[march fused] {precision}: evaluated {ref[1]['evaluated']} of {ref[1]['total']} (fused: {got[1]['evaluated']})")
    assert 0 < ref[1]['evaluated'] < 0.8 * ref[1]['total']
    assert_same(got, ref)


def c_march(sc, R, z, eps, chunk, precision, sigma_only=False, ws_short=0, guard=64, over=()):
    """nm_march_pass itself on buffers of the test's own: raw_out pre-filled with a sentinel and followed by a guard region, stats pre-filled
    -> (rc, raw [R,S,4], guard, stats int64[2])"""
    L = sc['lib']
    o, d = rays(sc, R)
    S = z.shape[1]
    buf = torch.full((R * S * 4 + guard,), SENTINEL, device='cuda', dtype=torch.float32)
    n_ws = int(L.lib().nm_march_pass_workspace_floats(R))
    ws = torch.zeros(n_ws, device='cuda', dtype=torch.float32)
    stats = torch.full((2,), -1, device='cuda', dtype=torch.int64)
    args = dict(mlp=sc['net'].handle(), o=L.dev_ptr(o), d=L.dev_ptr(d), z=L.dev_ptr(z), R=R, S=S, chunk=chunk, eps=eps, sigma_only=int(sigma_only),
                precision=L.PRECISIONS[precision], scale=1.0, dz=None, occ_z=None, occ_T=None, ws=L.dev_ptr(ws), n_ws=n_ws - ws_short, raw=L.dev_ptr(buf),
                stats=L.dev_ptr(stats, torch.int64), stream=L.stream_ptr())
    assert set(dict(over)) <= set(args)
    args.update(over)
    rc = L.lib().nm_march_pass(*args.values())
    torch.cuda.synchronize()
    return rc, buf[:R * S * 4].view(R, S, 4), buf[R * S * 4:], stats


def test_all_rays_cut_at_the_first_boundary(scene):
    """eps above every transmittance: the yardstick's list is empty after chunk 1 (asserted on its count), so every later launch of the fused
    pass runs over a count of 0: the records past the first chunk are exactly 0 and nothing behind raw_out is touched"""
    R, chunk = 1000, 32
    z = fine_z(scene, R, 128, 128)
    ref_raw, ref = yardstick(scene, R, z, 2.0, chunk, 'i8x3')
    assert ref['evaluated'] == R * chunk and ref['launches'] == 8           # the yardstick's live count after chunk 1 is 0
    rc, raw, guard, stats = c_march(scene, R, z, 2.0, chunk, 'i8x3')
    assert rc == 0
    assert torch.equal(raw, ref_raw)
    assert bool((raw[:, chunk:] == 0).all()) and bool((raw[:, :chunk, 3] != 0).any())
    assert bool((guard == SENTINEL).all())
    assert stats.tolist() == [R * chunk, 0]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_occluder_and_merged_intervals(scene, precision):
    """the list will be merged with a second one that ends mid-ray: cut on the merged list's intervals (dz) and, once behind the other list's
    last sample, on T x its transmittance"""
    R = 2048
    o, d = rays(scene, R)
    z = fine_z(scene, R, 64, 64)
    g = torch.Generator(device='cuda').manual_seed(5)
    near_b = 0.8 + 0.4 * torch.rand(R, device='cuda', generator=g)
    z_b = (near_b[:, None] + torch.linspace(0., 0.9, 24, device='cuda')[None, :]).contiguous()
    dz = scene['render'].merged_intervals([z, z_b])[0]
    z_far = z_b[:, -1].contiguous()
    T_occ = torch.rand(R, device='cuda', generator=g) ** 4                 # from nearly opaque to nearly clear
    assert bool((z[:, 0] < z_far).all()) and bool((z[:, -1] > z_far).any())    # z_far is mid-ray
    kw = dict(occluder=(z_far, T_occ), dz=dz)
    got, ref = fused(scene, R, z, 1e-4, 16, precision, **kw), yardstick(scene, R, z, 1e-4, 16, precision, **kw)
    assert 0 < ref[1]['evaluated'] < ref[1]['total']
    assert_same(got, ref)
    # the occluder matters: without it the cuts come later
    assert yardstick(scene, R, z, 1e-4, 16, precision, dz=dz)[1]['evaluated'] > ref[1]['evaluated']


def c_bkg_march(sc, R, S, N, eps, eps_coarse, chunk, p_coarse, p_fine, composite=True, ws_short=0, over=()):
    L = sc['lib']
    o, d = rays(sc, R)
    near, far = near_far(R)
    raw = torch.full((R, S + N, 4), SENTINEL, device='cuda', dtype=torch.float32)
    z = torch.full((R, S + N), SENTINEL, device='cuda', dtype=torch.float32)
    rgb, depth, acc = (torch.full(s, SENTINEL, device='cuda', dtype=torch.float32) for s in ((R, 3), (R,), (R,)))
    n_ws = int(L.lib().nm_render_rays_bkg_march_workspace_floats(R, S, N))
    ws = torch.zeros(n_ws, device='cuda', dtype=torch.float32)
    stats = torch.full((4,), -1, device='cuda', dtype=torch.int64)
    t_vals = torch.linspace(0., 1., steps=S, device='cuda')
    u = torch.linspace(0., 1., steps=N, device='cuda') if N else None
    args = dict(coarse=sc['net'].handle(), fine=sc['net'].handle() if N else None, o=L.dev_ptr(o), d=L.dev_ptr(d), near=L.dev_ptr(near), far=L.dev_ptr(far),
                R=R, S=S, N=N, t=L.dev_ptr(t_vals), u=L.dev_ptr(u), white=1, pc=L.PRECISIONS[p_coarse], pf=L.PRECISIONS[p_fine] if N else 0, eps=eps,
                eps_coarse=eps_coarse, chunk=chunk, ws=L.dev_ptr(ws), n_ws=n_ws - ws_short, raw=L.dev_ptr(raw), z=L.dev_ptr(z),
                rgb=L.dev_ptr(rgb) if composite else None, depth=L.dev_ptr(depth) if composite else None, acc=L.dev_ptr(acc) if composite else None,
                stats=L.dev_ptr(stats, torch.int64), stream=L.stream_ptr())
    assert set(dict(over)) <= set(args)
    args.update(over)
    rc = L.lib().nm_render_rays_bkg_march(*args.values())
    torch.cuda.synchronize()
    return rc, dict(raw=raw, z=z, rgb=rgb, depth=depth, acc=acc, stats=stats)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("S,N,chunk", [(16, 16, 8), (128, 128, 32)])
def test_two_net_call_vs_the_composed_pieces(scene, S, N, chunk, precision):
    """sample -> density-only march at TERMINATION_COARSE (fp16x3) -> importance samples -> march at eps -> composite, one call against the
    Python pieces: raw, z, rgb, depth, acc and both counters"""
    R, eps = 2048, 1e-4
    Rn, net = scene['render'], scene['net']
    o, d = rays(scene, R)
    _, _, zc = scene['ray'].sample_z(o, d, *near_far(R), S)
    st_c, st_f = {}, {}
    rawc = Rn.march_pass_rays(net, o, d, zc, Rn.TERMINATION_COARSE, chunk=chunk, precision='fp16x3', role=None, stats=st_c, sigma_only=True, adaptive=False)
    z, _ = scene['ray'].importance_z_from_raw(rawc, zc, d, N)
    raw = Rn.march_pass_rays(net, o, d, z, eps, chunk=chunk, precision=precision, role=None, stats=st_f, adaptive=False)
    rgb, _, acc, _, depth = Rn.raw2outputs(raw, z, d, white_bkg=True, want_weights=False)
    rc, got = c_bkg_march(scene, R, S, N, eps, Rn.TERMINATION_COARSE, chunk, 'fp16x3', precision)
    assert rc == 0, scene['lib'].lib().nm_last_error()
    assert got['stats'].tolist() == [st_f['evaluated'], 0, st_c['evaluated'], 0]
    if S == 128:
        assert st_f['evaluated'] < 0.8 * st_f['total']
    for name, ref in (('z', z), ('raw', raw), ('rgb', rgb), ('depth', depth), ('acc', acc)):
        assert torch.equal(got[name], ref), name
    # rgb == NULL: raw and z only (the hybrid renderers composite later)
    rc, bare = c_bkg_march(scene, R, S, N, eps, Rn.TERMINATION_COARSE, chunk, 'fp16x3', precision, composite=False)
    assert rc == 0 and torch.equal(bare['raw'], raw) and torch.equal(bare['z'], z) and bool((bare['rgb'] == SENTINEL).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_net_call_vs_the_composed_pieces(scene, precision):
    R, S, chunk, eps = 2048, 64, 16, 1e-4
    Rn = scene['render']
    o, d = rays(scene, R)
    z = fine_z(scene, R, S, 0)
    raw, st = yardstick(scene, R, z, eps, chunk, precision)
    rgb, _, acc, _, depth = Rn.raw2outputs(raw, z, d, white_bkg=True, want_weights=False)
    rc, got = c_bkg_march(scene, R, S, 0, eps, Rn.TERMINATION_COARSE, chunk, precision, precision)
    assert rc == 0, scene['lib'].lib().nm_last_error()
    assert got['stats'].tolist() == [st['evaluated'], 0, 0, 0]
    for name, ref in (('z', z), ('raw', raw), ('rgb', rgb), ('depth', depth), ('acc', acc)):
        assert torch.equal(got[name], ref), name


def test_renderer_switch(scene, monkeypatch):
    """render_vanilla_rays with MARCH_FUSED on = the same call with adaptive=False forced on march_pass_rays, trace included; off = today's frame"""
    Rn, net = scene['render'], scene['net']
    o, d = rays(scene, 2048)
    monkeypatch.setattr(Rn, 'TERMINATION_EPS', 1e-4)
    assert Rn.MARCH_FUSED is False
    tr_today = {}
    today = Rn.render_vanilla_rays(net, net, o, d, 0.0, 3.14, 128, 128, trace=tr_today)
    march = Rn.march_pass_rays
    monkeypatch.setattr(Rn, 'march_pass_rays', lambda *a, **kw: march(*a, **{**kw, 'adaptive': False}))
    tr_fixed = {}
    fixed = Rn.render_vanilla_rays(net, net, o, d, 0.0, 3.14, 128, 128, trace=tr_fixed)
    reached = []
    monkeypatch.setattr(Rn, 'march_pass_rays', lambda *a, **kw: reached.append(1))      # the fused route must not come back here
    monkeypatch.setattr(Rn, 'MARCH_FUSED', True)
    tr_fused = {}
    on = Rn.render_vanilla_rays(net, net, o, d, 0.0, 3.14, 128, 128, trace=tr_fused)
    assert not reached
    assert torch.equal(on[0], fixed[0]) and torch.equal(on[1], fixed[1])
    for key in ('march', 'march_coarse'):
        assert tr_fused[key] == tr_fixed[key] and set(tr_fused[key][0]) == {'evaluated', 'total', 'launches'}
    assert torch.equal(tr_fused['bkg_z'][0], tr_fixed['bkg_z'][0])
    assert tr_fused['march'][0]['evaluated'] < 0.8 * tr_fused['march'][0]['total']
    # off: the frame of the route as it is (adaptive chunks)
    monkeypatch.setattr(Rn, 'MARCH_FUSED', False)
    monkeypatch.setattr(Rn, 'march_pass_rays', march)
    tr_off = {}
    off = Rn.render_vanilla_rays(net, net, o, d, 0.0, 3.14, 128, 128, trace=tr_off)
    assert torch.equal(off[0], today[0]) and torch.equal(off[1], today[1]) and tr_off['march'] == tr_today['march']


P16 = ctypes.c_void_p(16)                              # a non-null pointer no refusal may dereference


@pytest.mark.parametrize("what,kw", [
    ("null handle", dict(mlp=None)),
    ("null origin", dict(o=None)),
    ("null direction", dict(d=None)),
    ("null z_vals", dict(z=None)),
    ("null workspace", dict(ws=None)),
    ("null raw_out", dict(raw=None)),
    ("occ_z_far without occ_T", dict(occ_z=P16)),
    ("chunk < 1", dict(chunk=0)),
    ("negative chunk", dict(chunk=-4)),
    ("S_total < 1", dict(S=0)),
    ("a workspace one float short", dict(ws_short=1)),
    ("NM_PREC_FP32", dict(precision=0)),
    ("no such precision", dict(precision=9)),
    ("raw_out not aligned", dict(raw=ctypes.c_void_p(20))),
])
def test_march_pass_argument_errors_name_the_entry_and_write_nothing(scene, what, kw):
    R = 64
    z = fine_z(scene, R, 32, 32)
    kw = dict(kw)
    short = kw.pop('ws_short', 0)
    rc, raw, guard, stats = c_march(scene, R, z, 1e-4, 16, 'i8x3', ws_short=short, over=kw)
    assert rc == -1, what
    assert b"nm_march_pass:" in scene['lib'].lib().nm_last_error(), (what, scene['lib'].lib().nm_last_error())
    assert bool((raw == SENTINEL).all()) and bool((guard == SENTINEL).all()) and stats.tolist() == [-1, -1], what


@pytest.mark.parametrize("what,kw", [
    ("null handle", dict(coarse=None)),
    ("null near", dict(near=None)),
    ("null t_vals", dict(t=None)),
    ("null u", dict(u=None)),
    ("null workspace", dict(ws=None)),
    ("null z_out", dict(z=None)),
    ("a fine net without importance samples", dict(N=0)),
    ("rgb without depth", dict(depth=None)),
    ("chunk < 1", dict(chunk=0)),
    ("a workspace one float short", dict(ws_short=1)),
    ("NM_PREC_FP32 coarse", dict(pc=0)),
    ("NM_PREC_FP32 fine", dict(pf=0)),
])
def test_bkg_march_argument_errors_name_the_entry_and_write_nothing(scene, what, kw):
    kw = dict(kw)
    short = kw.pop('ws_short', 0)
    rc, got = c_bkg_march(scene, 64, 16, 16, 1e-4, 4e-13, 8, 'fp16x3', 'i8x3', ws_short=short, over=kw)
    assert rc == -1, what
    assert b"nm_render_rays_bkg_march:" in scene['lib'].lib().nm_last_error(), (what, scene['lib'].lib().nm_last_error())
    for name in ('raw', 'z', 'rgb', 'depth', 'acc'):
        assert bool((got[name] == SENTINEL).all()), (what, name)
    assert got['stats'].tolist() == [-1] * 4, what
