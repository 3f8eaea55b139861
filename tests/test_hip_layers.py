"""-m gpu: the layered merge (csrc/merge_layers.hip: nm_merge_composite_layers; render_utils.merge_composite_layers) and what is built on it.

Kernel: rgb / depth / acc equal nm_merge_composite_lists_wide (and, up to four lists, nm_merge_composite_lists) BIT FOR BIT; with one list the
layer equals the totals bit for bit; every layer entry lies within the float32 summation bound of the float64 sum of the very weights
raw2outputs returns for the list merged by nm_merge_sorted (the same composite_ray body), attributed to their source list by a stable sort;
a list without density has an empty layer; exact ties go to the earlier list; compact lists behind `rows` equal the expanded arrays; two runs
give the same bits and nothing is written outside the outputs.  nm_layers_to_rgba8 equals frame_to_uint8 of the tensor torch builds by its rule.

Renderers (the 40 x 32 'multi' capture of tests/helpers/posed_scene.py, 16 + 16 background and 16 human samples): rgb and depth of
render_hybrid_layers_rays / render_multi_layers_rays equal the unlayered device cores bit for bit, with and without early termination; the layers
recompose the picture; missed actors and missed rays have empty layers.

THE BOUND (derived, not measured): a float32 sum of St non-negative terms, whatever its order, errs by at most St 2^-24 of the sum of the terms;
each term carries one product rounding and a sigmoid a few ulp from float64's: (St + 8) 2^-24 x the float64 sum of the terms' absolute values."""
import ctypes

import numpy as np
import pytest
import torch

from test_hip_fused import _lists
from test_hip_merge_wide import dirs, expand, list_by_list
from test_hip_multi_fused import M, OUT_OF_VIEW, actors  # noqa: F401  (M: the module-scoped scene fixture)
from test_hip_sizes import P, SHIFTS, check, guarded, guards_intact, lib, same, stream

pytestmark = pytest.mark.gpu

SIZES = {
    'one': (56,),
    'two': (40, 16),
    'four': (40, 16, 16, 16),
    'five_wide': (24, 8, 8, 8, 8),                                 # the wide regime, St = 56
    'ragged': (130, 1),                                            # St no multiple of 64, a one-sample list
    'nine': (8,) * 9,
}
RAYS = (1, 5, 257)
CASES = [(n, R) for n in SIZES for R in RAYS]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def R_():
    from neuman_hip import _lib, render_utils
    _lib.require_gpu()
    return render_utils


def bound_factor(St):
    return (St + 8) * U


def layer_sums64(R_, zs, raws, d):
    """-> (sums, abs sums), each a dict of float64 tensors acc [R,k], rgb [R,k,3], depth [R,k]: merge list by list with merge_sorted, the float32
    weights raw2outputs returns for the merged list (the composite_ray body the merge kernels use), every merged sample's source list from a
    stable sort of the concatenated z, the three per-list sums in float64"""
    z_all, raw_all = zs[0], raws[0]
    for z, raw in zip(zs[1:], raws[1:]):
        z_all, raw_all = R_.merge_sorted(z_all, raw_all, z, raw)
    w = R_.raw2outputs(raw_all, z_all, d, white_bkg=False, want_weights=True)[3]
    vals, idx = torch.sort(torch.cat(zs, 1), dim=1, stable=True)
    assert torch.equal(vals, z_all)
    assert torch.equal(torch.gather(torch.cat(raws, 1), 1, idx[..., None].expand(-1, -1, 4)), raw_all)      # (the stable order IS the merge's order)
    ends = torch.cumsum(torch.tensor([z.shape[1] for z in zs], device='cuda'), 0)
    src = torch.bucketize(idx, ends, right=True)                  # merged sample -> its list
    own = (src[:, None, :] == torch.arange(len(zs), device='cuda')[None, :, None]).double()               # [R,k,St]
    w64 = w.double()
    terms = dict(acc=w64[:, None, :, None], rgb=w64[:, None, :, None] * torch.sigmoid(raw_all[..., :3].double())[:, None], depth=(w64 * z_all.double())[:, None, :, None])
    sums = {k_: (t * own[..., None]).sum(2) for k_, t in terms.items()}
    sabs = {k_: (t.abs() * own[..., None]).sum(2) for k_, t in terms.items()}
    for k_ in ('acc', 'depth'):
        sums[k_], sabs[k_] = sums[k_][..., 0], sabs[k_][..., 0]
    return sums, sabs


def assert_layers_within_bound(R_, zs, raws, d, out, what):
    sums, sabs = layer_sums64(R_, zs, raws, d)
    St = sum(z.shape[1] for z in zs)
    worst = 0.0
    for name, dev in (('rgb', out[3]), ('depth', out[4]), ('acc', out[5])):
        assert dev.shape == sums[name].shape and torch.isfinite(dev).all(), (what, name)
        err, lim = (dev.double() - sums[name]).abs(), bound_factor(St) * sabs[name]
        ratio = float((err / lim.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= lim).all()), (what, name, ratio)
    print(f"layers {what}: St={St}, worst error / bound = {worst:.3f}")


_made = {}


def case(R_, name, R):
    """inputs and the layered outputs (both backgrounds) of a case, made once and shared by the tests that read them"""
    if (name, R) not in _made:
        zs, raws = _lists(R, SIZES[name], 21)
        assert float(torch.cat([r_[..., 3].reshape(-1) for r_ in raws]).min()) < 0 < float(torch.cat([r_[..., 3].reshape(-1) for r_ in raws]).max())
        d = dirs(R, 3)
        _made[(name, R)] = (zs, raws, d, {w: R_.merge_composite_layers(zs, raws, d, w) for w in (True, False)})
    return _made[(name, R)]


@pytest.mark.parametrize("name,R", CASES)
def test_rgb_depth_acc_equal_the_unlayered_kernels_bit_for_bit(R_, name, R):
    zs, raws, d, out = case(R_, name, R)
    for white in (True, False):
        refs = [R_.merge_composite_lists_wide(zs, raws, d, white)] + ([R_.merge_composite_lists(zs, raws, d, white)] if len(zs) <= 4 else [])
        for ref in refs:
            for x, y, what in zip(out[white][:3], ref, ("rgb", "depth", "acc")):
                assert torch.isfinite(x).all() and torch.equal(x, y), (name, R, white, what)
        assert all(torch.equal(x, y) for x, y in zip(out[True][3:], out[False][3:]))       # the layers never hold a background


@pytest.mark.parametrize("R", RAYS)
def test_one_list_the_layer_is_the_totals_bit_for_bit(R_, R):
    _, _, _, out = case(R_, 'one', R)
    rgb, depth, acc, l_rgb, l_depth, l_acc = out[False]
    assert l_rgb.shape == (R, 1, 3) and l_depth.shape == (R, 1) and l_acc.shape == (R, 1)
    assert torch.equal(l_rgb[:, 0], rgb) and torch.equal(l_depth[:, 0], depth) and torch.equal(l_acc[:, 0], acc)
    assert float(acc.max()) > 0


@pytest.mark.parametrize("name,R", CASES)
def test_layers_are_the_per_list_sums_of_the_merged_lists_weights(R_, name, R):
    zs, raws, d, out = case(R_, name, R)
    assert_layers_within_bound(R_, zs, raws, d, out[False], f"{name} R={R}")
    if len(zs) > 1 and R > 1:
        assert all(float(out[False][5][:, l].max()) > 0 for l in range(len(zs)) if SIZES[name][l] > 1)     # every list of the case shows


@pytest.mark.parametrize("R", RAYS)
def test_a_list_without_density_has_an_empty_layer(R_, R):
    zs, raws = _lists(R, SIZES['four'], 22)
    raws[2][..., 3] = -raws[2][..., 3].abs()                      # sigma <= 0 everywhere
    out = R_.merge_composite_layers(zs, raws, dirs(R, 4), True)
    assert all(bool((x[:, 2] == 0).all()) for x in out[3:])
    assert float(out[5][:, [0, 1, 3]].max()) > 0


@pytest.mark.parametrize("name", ['two', 'nine'])
@pytest.mark.parametrize("R", RAYS)
def test_exact_ties_go_to_the_earlier_list(R_, name, R):
    zs, raws = _lists(R, SIZES[name], 23, ties=False)
    h = min(zs[0].shape[1] // 2, zs[1].shape[1])
    zs[1][:, :h] = zs[0][:, :2 * h:2]                              # half of list 0's z, exactly, in list 1
    zs[1] = torch.sort(zs[1], dim=1)[0].contiguous()
    assert int((zs[1][:, :, None] == zs[0][:, None, :]).sum()) >= R * h
    d = dirs(R, 5)
    out = R_.merge_composite_layers(zs, raws, d, False)
    assert all(torch.equal(x, y) for x, y in zip(out[:3], list_by_list(R_, zs, raws, d, False)))
    assert_layers_within_bound(R_, zs, raws, d, out, f"ties {name} R={R}")


@pytest.mark.parametrize("R", RAYS)
def test_compact_lists_behind_rows_equal_the_expanded_arrays(R_, R):
    """the multi-person renderer's lists (actor_lists_compact): the background, an actor as a compact [n_hit + 1, S] array whose last row is the
    placeholder every missed ray points at, an actor nobody hits (the placeholder row alone)"""
    S = 16
    g = torch.Generator(device='cuda').manual_seed(6)
    d = dirs(R, 6)
    (zb, z1), (rawb, raw1) = _lists(R, (40, S), 24)
    pad_z, pad_raw = torch.linspace(8.0, 12.0, S, device='cuda')[None].contiguous(), torch.zeros((1, S, 4), device='cuda')
    hit = torch.nonzero(torch.rand(R, device='cuda', generator=g) < 0.6).reshape(-1)
    rows = torch.full((R,), hit.numel(), device='cuda', dtype=torch.int32)
    rows[hit] = torch.arange(hit.numel(), device='cuda', dtype=torch.int32)
    lists = [(zb, rawb, None), (torch.cat([z1[hit], pad_z]).contiguous(), torch.cat([raw1[hit], pad_raw]).contiguous(), rows),
             (pad_z, pad_raw, torch.zeros(R, device='cuda', dtype=torch.int32))]
    full = [expand(*l) for l in lists]
    for white in (True, False):
        a = R_.merge_composite_layers([l[0] for l in lists], [l[1] for l in lists], d, white, rows=[l[2] for l in lists])
        b = R_.merge_composite_layers([f[0] for f in full], [f[1] for f in full], d, white)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), white
        assert bool((a[5][:, 2] == 0).all()) and bool((a[5][rows.long() == hit.numel(), 1] == 0).all())


@pytest.mark.parametrize("name,R", CASES)
def test_two_runs_give_the_same_bits_and_nothing_is_written_outside_the_outputs(R_, name, R):
    zs, raws, d, out = case(R_, name, R)
    k = len(zs)
    arr = ctypes.c_void_p * k
    shapes = dict(rgb=(R, 3), depth=(R,), acc=(R,), layer_rgb=(R, k, 3), layer_depth=(R, k), layer_acc=(R, k))
    runs = []
    for _ in range(2):
        bufs = {n_: guarded(s) for n_, s in shapes.items()}
        O_ = {n_: v for n_, (b, v) in bufs.items()}
        check(lib().nm_merge_composite_layers(k, arr(*[z.data_ptr() for z in zs]), arr(*[r_.data_ptr() for r_ in raws]), None, (ctypes.c_int * k)(*SIZES[name]), R,
                                              P(d), 1, P(O_['rgb']), P(O_['depth']), P(O_['acc']), P(O_['layer_rgb']), P(O_['layer_depth']), P(O_['layer_acc']),
                                              stream()), "nm_merge_composite_layers")
        torch.cuda.synchronize()
        for n_, (b, _) in bufs.items():
            assert guards_intact(b), f"a write landed in the guard rows of {n_}"
        runs.append(O_)
    for (n_, x), y in zip(runs[0].items(), out[True]):
        assert same(x, runs[1][n_]) and same(x.contiguous(), y), n_
    # layer_depth is optional: without it the other outputs are the same bits
    bufs = {n_: guarded(s) for n_, s in shapes.items() if n_ != 'layer_depth'}
    O_ = {n_: v for n_, (b, v) in bufs.items()}
    check(lib().nm_merge_composite_layers(k, arr(*[z.data_ptr() for z in zs]), arr(*[r_.data_ptr() for r_ in raws]), None, (ctypes.c_int * k)(*SIZES[name]), R, P(d),
                                          1, P(O_['rgb']), P(O_['depth']), P(O_['acc']), P(O_['layer_rgb']), None, P(O_['layer_acc']), stream()),
          "nm_merge_composite_layers")
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b, _ in bufs.values()) and all(same(O_[n_], runs[0][n_]) for n_ in O_)


def test_more_than_the_staging_limit_is_refused_and_nothing_is_launched(R_):
    from neuman_hip import _lib
    R = 4
    limit = lib().nm_merge_composite_layers_max_samples(2)
    half = limit // 2 + 1
    zs, raws = _lists(R, (half, half), 25, ties=False)
    with pytest.raises(_lib.NeumanHipError, match=f"nm_merge_composite_layers.*{limit}"):
        R_.merge_composite_layers(zs, raws, dirs(R, 7))
    outs = [torch.full(s, 7.25, device='cuda') for s in ((R, 3), (R,), (R,), (R, 2, 3), (R, 2), (R, 2))]
    arr = ctypes.c_void_p * 2
    rc = lib().nm_merge_composite_layers(2, arr(*[z.data_ptr() for z in zs]), arr(*[r_.data_ptr() for r_ in raws]), None, (ctypes.c_int * 2)(half, half), R,
                                         P(dirs(R, 7)), 1, *[P(t) for t in outs], stream())
    torch.cuda.synchronize()
    assert rc == -1 and all(bool((t == 7.25).all()) for t in outs)


def test_rgba_bytes_are_frame_to_uint8_of_the_stated_rule(R_):
    g = torch.Generator(device='cuda').manual_seed(8)
    n = 4099
    acc = torch.rand(n, device='cuda', generator=g)
    acc[:64] = 0.0
    acc[64:128] = 1.0 + torch.rand(64, device='cuda', generator=g)            # acc > 1
    acc[128:192] = torch.rand(64, device='cuda', generator=g) * 1e-30 + 1e-38  # tiny
    acc[192:200] = -0.25
    acc[200] = -0.0
    rgb = torch.rand((n, 3), device='cuda', generator=g) * acc.abs()[:, None] * 1.1     # (a tenth of the colours beyond 1 after the division)
    rgb[:64] = torch.rand((64, 3), device='cuda', generator=g)               # colour without opacity: dropped
    acc[130], rgb[130] = 1e-38, 1e-30                                         # quotient far beyond 1
    want = torch.cat([torch.where((acc > 0)[:, None], (rgb / acc[:, None]).clamp(0, 1), torch.zeros_like(rgb)), acc.clamp(0, 1)[:, None]], 1)
    out = R_.layers_to_rgba_uint8(rgb, acc)
    assert out.dtype == torch.uint8 and out.shape == (n, 4)
    assert torch.equal(out, R_.frame_to_uint8(want))
    assert bool((out[:64] == 0).all()) and bool((out[64:128, 3] == 255).all()) and bool((out[192:201] == 0).all())
    img = R_.layers_to_rgba_uint8(rgb[:4096].reshape(64, 64, 3), acc[:4096].reshape(64, 64))       # any leading shape
    assert img.shape == (64, 64, 4) and torch.equal(img.reshape(-1, 4), out[:4096])


# ---- renderers ------------------------------------------------------------------------------------------------------------------
S_, N_ = 16, 16


def hybrid(M, layered, white=True, trace=None):
    humans, verts, meshes = actors(M, SHIFTS[:1])
    f = M.R.render_hybrid_layers_rays if layered else M.R.render_hybrid_rays
    return f(M.nets.coarse, M.nets.fine, humans[0], M.o, M.d, M.cap.near['bkg'], M.cap.far['bkg'], verts[0], meshes[0], S_, N_, white, 0.2, None, trace)


def multi(M, shifts, layered, white=True, trace=None):
    humans, verts, meshes = actors(M, shifts)
    f = M.R.render_multi_layers_rays if layered else M.R.render_multi_rays
    return f(M.nets.coarse, M.nets.fine, humans, M.o, M.d, M.cap.near['bkg'], M.cap.far['bkg'], verts, meshes, S_, N_, white, 0.2, None, trace)


SCENES = {'hybrid': 1, 'multi3': 3, 'multi4': 4}                   # (four actors: five lists, the regime of the wide merge)


def run(M, scene, layered, white=True, trace=None):
    return hybrid(M, layered, white, trace) if scene == 'hybrid' else multi(M, SHIFTS[:SCENES[scene]], layered, white, trace)


def recomposed_within_bound(out, rgb, white, A):
    """sum_l layer_rgb_l + white (1 - sum_l layer_acc_l) against rgb: both sides are float32 sums of the same St terms (twice the bound of a
    sum), the terms' magnitudes read from the layers themselves (non-negative terms: a sum is its absolute sum) plus, with a white background,
    the 1 and the opacity of 1 - acc"""
    St = S_ + N_ + A * S_
    l_rgb, l_acc = out['layer_rgb'].double(), out['layer_acc'].double()
    total = l_rgb.sum(1) + (1.0 - l_acc.sum(1))[:, None] * float(white)
    scale = l_rgb.abs().sum(1) + (1.0 + l_acc.sum(1))[:, None] * float(white)
    err, lim = (total - rgb.double()).abs(), 2 * bound_factor(St) * scale
    print(f"recomposition: St={St}, worst error / bound = {float((err / lim.clamp_min(1e-300)).max()):.3f}")
    return bool((err <= lim).all())


@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_layered_renderers_return_the_unlayered_picture_and_layers_that_recompose_it(M, monkeypatch, scene, eps):
    monkeypatch.setattr(M.R, 'TERMINATION_EPS', eps)
    A, R = SCENES[scene], M.o.shape[0]
    for white in (True, False):
        plain = run(M, scene, False, white)
        out = run(M, scene, True, white)
        assert sorted(out) == ['depth', 'layer_acc', 'layer_depth', 'layer_rgb', 'rgb']
        assert torch.equal(out['rgb'], plain[0]) and torch.equal(out['depth'], plain[1]), (scene, eps, white)
        assert out['layer_rgb'].shape == (R, 1 + A, 3) and out['layer_depth'].shape == (R, 1 + A) and out['layer_acc'].shape == (R, 1 + A)
        assert all(torch.isfinite(x).all() for x in out.values())
        assert recomposed_within_bound(out, out['rgb'], white, A), (scene, eps, white)
        assert float(out['layer_acc'].min()) >= 0 and float(out['layer_acc'].max()) <= 1 + 1e-6
        assert float(out['layer_acc'].sum(1).max()) <= 1 + 1e-6
        assert all(float(out['layer_acc'][:, l].max()) > 0 for l in range(1 + A)), "a layer of the scene is empty"
        if white:
            over_white = M.R.compose_over(out['layer_rgb'], out['layer_acc'], torch.ones(3, device='cuda'), layers=range(1 + A))
            scale = out['layer_rgb'].double().sum(1) + (1.0 + out['layer_acc'].double().sum(1))[:, None]
            assert bool(((over_white.double() - out['rgb'].double()).abs() <= 2 * bound_factor(S_ + N_ + A * S_) * scale).all())
        elif eps == 0:
            assert torch.equal(out['layer_rgb'], run(M, scene, True, True)['layer_rgb'])           # premultiplied: no background in a layer


def test_an_actor_no_ray_hits_has_an_empty_layer(M):
    shifts = [SHIFTS[0], OUT_OF_VIEW, SHIFTS[1], SHIFTS[2]]
    trace = {}
    out = multi(M, shifts, True, trace=trace)
    assert trace['hit'][1].numel() == 0 and all(trace['hit'][a].numel() > 0 for a in (0, 2, 3))
    assert all(bool((out[k_][:, 2] == 0).all()) for k_ in ('layer_rgb', 'layer_depth', 'layer_acc'))
    plain = multi(M, shifts, False)
    assert torch.equal(out['rgb'], plain[0]) and torch.equal(out['depth'], plain[1])
    for a in (0, 2, 3):                                            # an actor's layer lives on the rays that hit it
        missed = torch.ones(M.o.shape[0], dtype=torch.bool, device='cuda')
        missed[trace['hit'][a].long()] = False
        assert bool((out['layer_acc'][missed, 1 + a] == 0).all()) and float(out['layer_acc'][~missed, 1 + a].max()) > 0


def test_hybrid_rays_that_miss_the_body_hold_the_background_only_composite(M):
    trace = {}
    out = hybrid(M, True, trace=trace)
    R = M.o.shape[0]
    hit = torch.cat(trace['hit']).long()
    missed = torch.ones(R, dtype=torch.bool, device='cuda')
    missed[hit] = False
    assert 0 < hit.numel() < R
    assert all(bool((out[k_][missed, 1] == 0).all()) for k_ in ('layer_rgb', 'layer_depth', 'layer_acc'))
    n, f = (torch.full((R,), float(x), device='cuda') for x in (M.cap.near['bkg'], M.cap.far['bkg']))
    raw, z = M.R.bkg_pass_rays(M.nets.coarse, M.nets.fine, M.o, M.d, n, f, S_, N_, True, composite_only=M.R.LIVE_HEADS)
    rgb, _, acc, _, depth = M.R.raw2outputs(raw, z, M.d, white_bkg=False, want_weights=False)
    assert torch.equal(out['layer_acc'][missed, 0], acc[missed])
    assert torch.equal(out['layer_rgb'][missed, 0], rgb[missed]) and torch.equal(out['layer_depth'][missed, 0], depth[missed])
    assert float((out['layer_acc'][hit, 0] - acc[hit]).min()) < 0           # behind the body the background shows less than it would alone


def test_frame_level_functions_return_the_documented_shapes(M, tmp_path):
    import types
    net = types.SimpleNamespace(coarse_bkg_net=M.nets.coarse, fine_bkg_net=M.nets.fine, coarse_human_net=M.nets.human, parameters=M.nets.coarse.parameters)
    posed, T = M.g['posed_verts'], M.g['T']
    H, W = M.cap.shape

    def shifted(s):
        t = T.copy()
        t[:, :3, 3] += np.array(s)
        return (posed + np.array(s, np.float32)).astype(np.float32), t
    kw = dict(samples_per_ray=S_, importance_samples_per_ray=N_, geo_threshold=0.2)
    v, t = shifted(SHIFTS[0])
    one = M.R.render_hybrid_nerf_layers(net, M.cap, v, M.faces, t, **kw)
    A = 2
    vt = [shifted(s) for s in SHIFTS[:A]]
    two = M.R.render_hybrid_nerf_multi_persons_layers(net, M.cap, [net] * A, [x[0] for x in vt], [M.faces] * A, [x[1] for x in vt], **kw)
    for out, L in ((one, 2), (two, 1 + A)):
        assert sorted(out) == ['depth', 'layer_acc', 'layer_depth', 'layer_rgb', 'rgb'] and all(isinstance(x, np.ndarray) and x.dtype == np.float32 for x in out.values())
        assert out['rgb'].shape == (H, W, 3) and out['depth'].shape == (H, W)
        assert out['layer_rgb'].shape == (H, W, L, 3) and out['layer_depth'].shape == (H, W, L) and out['layer_acc'].shape == (H, W, L)
    ref = M.R.render_hybrid_nerf(net, M.cap, v, M.faces, t, return_depth=True, **kw)
    assert np.array_equal(one['rgb'], ref[0]) and np.array_equal(one['depth'], ref[1])
    # the recipe of INTEGRATION.md: the actors over a photograph, and an actor's matte as a 4-channel PNG
    photo = torch.rand((H, W, 3), device='cuda')
    comp = M.R.compose_over(torch.as_tensor(two['layer_rgb']).cuda(), torch.as_tensor(two['layer_acc']).cuda(), photo)
    nobody = two['layer_acc'][..., 1:].sum(-1) == 0
    assert comp.shape == (H, W, 3) and nobody.any() and torch.equal(comp[torch.as_tensor(nobody).cuda()], photo[torch.as_tensor(nobody).cuda()])
    rgba = M.R.layers_to_rgba_uint8(two['layer_rgb'][:, :, 1], two['layer_acc'][:, :, 1])
    M.R.save_png(str(tmp_path / "actor0.png"), rgba)
    assert rgba.shape == (H, W, 4) and (tmp_path / "actor0.png").stat().st_size > 100
