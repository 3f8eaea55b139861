"""-m gpu: the network kernels at the edges of the operand range -- the nets of tests/helpers/mlp_edges.py EDGE_NETS (a unit whose weights are small
against its bias, outlier rows and columns, dead layers, rescaled layers), large coordinates, non-finite samples and non-finite weights -- against a
float64 evaluation of the same net, within the bounds the suite states for ordinary nets (mlp_edges.BOUNDS; no tolerance of its own).

Kernels reached: nerf_mlp_kernel (fp32 / bf16x3 / bf16 / fp16x3, whole network, stage by stage, density only, the training forward's two storages),
nerf_mlp_i8s_kernel<false | true> (i8x3, view-dependent and plain head), nerf_mlp_i8w_kernel (i8x3 density only and stage by stage),
nerf_sigma_f16t_kernel (fp16x3 density only), the fused backward chain and the weight-gradient products, and nm_mlp_refresh_f16's pack kernels."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import mlp_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu

PARITY = ("fp32", "bf16x3", "fp16x3", "i8x3")
EMULATED = ("bf16x3", "fp16x3", "i8x3")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import types
    from neuman_hip import _lib, train
    return types.SimpleNamespace(L=_lib, train=train)


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to('cuda', torch.float32).contiguous()


def errs(got, rgb64, sig64):
    return float(np.abs(got[:, :3] - rgb64).max()), float(np.abs(got[:, 3] - sig64).max())


def as_rays(pts, dirs):
    """the points as one-sample rays: origin = the point, z = 0, so that o + d * 0 is the point itself"""
    return cu(pts), cu(dirs), torch.zeros((pts.shape[0], 1), device='cuda')


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# a. edge nets through every kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.FINITE_NETS, ids=lambda c: c.name)
def test_edge_nets_through_every_kernel(G, case):
    j, sd, spec, plain = E.build(case)
    jc = j.cuda()
    ora_err = None
    for n in (300, 128 * 3 + 5):
        pts, dirs = E.sample_points(n, seed=11 + n)
        rgb64, sig64 = E.f64_network(sd, spec, pts, dirs, plain=plain)
        emu = {}
        if n == 300:                                            # the emulation's and the float32 oracle's own error on the same points, for the printed line
            from oracle import nerf_mlp
            ora_err = errs(nerf_mlp.joiner_forward(sd, spec, pts, dirs), rgb64, sig64)
            for which in EMULATED:
                rc, img, msg = E.pack(j, spec, plain, which)
                assert rc == 0, msg
                with np.errstate(all='ignore'):
                    emu[which] = errs(E.emulation(which)(img, pts, dirs, spec, plain=plain), rgb64, sig64)
        for prec in (("fp16x3", "i8x3") if plain else PARITY):
            got = jc(cu(pts), cu(dirs), precision=prec).cpu().numpy()
            e_rgb, e_sig = errs(got, rgb64, sig64)
            b_rgb, b_sig = E.bounds(prec, sig64, spec.mapping)
            note = ""
            if prec in emu:
                loud = e_rgb > 2 * emu[prec][0] + ora_err[0] or e_sig > 2 * emu[prec][1] + ora_err[1]
                note = f"; emulation {emu[prec][0]:.2e} / {emu[prec][1]:.2e}, float32 oracle {ora_err[0]:.2e} / {ora_err[1]:.2e}" + (" <-- above twice the emulation's" if loud else "")
            print(f"[mlp edges] {case.name} n={n} {prec}: rgb {e_rgb:.2e} (bound {b_rgb:.1e}) sigma {e_sig:.2e} (bound {b_sig:.1e}){note}")
            assert np.isfinite(got).all()
            assert e_rgb < b_rgb and e_sig < b_sig, (case.name, n, prec)
        if not plain:
            fast = jc(cu(pts), cu(dirs), precision="bf16").cpu().numpy()                       # not parity grade: finite, nothing more
            assert np.isfinite(fast).all()
            o, d, z = as_rays(pts, dirs)
            for prec in ("fp16x3", "i8x3"):                                                     # the density-only launches
                full = jc.forward_rays(o, d, z, precision=prec)
                dens = jc.forward_rays(o, d, z, precision=prec, sigma_only=True)
                assert torch.equal(dens[..., 3], full[..., 3]), (case.name, n, prec)
                e_sig = float(np.abs(dens[:, 0, 3].cpu().numpy() - sig64).max())
                assert e_sig < E.bounds(prec, sig64, spec.mapping)[1], (case.name, n, prec, e_sig)


@pytest.mark.parametrize("prec", ["fp16x3", "i8x3"])
@pytest.mark.parametrize("case", [c for c in E.FINITE_NETS if c.kind in ("small_unit", "dead_part", "large_unit") and c.base != 'plain'], ids=lambda c: c.name)
def test_edge_nets_stage_by_stage(G, case, prec):
    """every intermediate the kernels can dump, so that a failure names its layer: the per-stage bounds of test_stage_by_stage / test_i8x3_stage_by_stage.
    For i8x3 the emulation's own error at the stage is printed beside the device's.

    The tightest cases are the i8x3 large_unit nets.  With units taken from the weights alone the stage behind a x1000 row missed its bound (stage 4: 1.11e-3
    on the device, 9.6e-4 in the emulation, against 4.3e-4): the row's unit is 1000 times its neighbours', so its column of the next layer's folded weights
    W[m][n] * u[n] is 1000 times the others and the int16 step of every row there left them 5 bits.  pack_image8 now balances such a column against the
    others (csrc/mlp_host.hip); what is left there is the x1000 row multiplying the 16-bit error of its own inputs (emulation: 0.83 of the bound)."""
    j, sd, spec, plain = E.build(case)
    jc = j.cuda()
    pts, dirs = E.sample_points(300, seed=311)
    _, _, hidden = E.f64_network(sd, spec, pts, dirs, hidden=True)
    emu = []
    if prec == "i8x3":
        rc, img, msg = E.pack(j, spec, plain, "i8x3")
        assert rc == 0, msg
        E.emulation("i8x3")(img, pts, dirs, spec, hidden=emu)
    scale = E.ROTATE_FACTOR if spec.mapping == 'rotate' else 1
    failed = []
    for st in range(10):
        got = jc.forward_debug(cu(pts), cu(dirs), st, precision=prec).cpu().numpy()
        ref = hidden[st]
        assert got.shape == ref.shape
        e, tol = float(np.abs(got - ref).max()), E.STAGE_BOUNDS[prec] * scale * max(1.0, float(np.abs(ref).max()))
        print(f"[mlp edges] {case.name} {prec} stage {st}: {e:.2e} (bound {tol:.1e}, |ref|max {np.abs(ref).max():.3g})" + (f"; emulation {np.abs(emu[st] - ref).max():.2e}" if emu else ""))
        if not e < tol:
            failed.append(f"stage {st}: {e:.2e} >= {tol:.2e}")
    assert not failed, (case.name, prec, failed)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# b. the training kernels on the same nets
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def unpack_signs(words):
    """the saved ReLU signs (csrc/mlp.hip save_bits / save_hvbits): [..., n, W] words of 32 features -> [..., n, 32 W] booleans; feature t of a word is
    register r = 4 (t >> 3) + (t & 3) of lane half g = (t >> 2) & 1: bit 16 g + 15 - r"""
    t = torch.arange(32, device=words.device)
    shift = 16 * ((t >> 2) & 1) + 15 - (4 * (t >> 3) + (t & 3))
    return (((words.to(torch.int64)[..., None] >> shift) & 1).reshape(*words.shape[:-1], -1).bool()).cpu()


def f64_autograd(sd, spec, pts, dirs, d_raw, masks, mask_hv):
    """float64 autograd of the torch network on the CPU, its ReLUs taking the signs the device saved (a pre-activation within rounding of zero may fall
    on either side; the backward pass under test differentiates the function its forward evaluated -- the pattern of test_backward_net16_against_float64)
    -> (raw [n,4], {parameter name: gradient}, {parameter name: per-entry bound factors (max |dZ|, sum_n |a|, |dZ|^T |a|)})"""
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    x_pe = torch.from_numpy(E.embed64(pts, spec.mapping, *spec.pos))
    d_pe = torch.from_numpy(E.embed64(dirs, spec.mapping, *spec.dir))
    pre, inp = {}, {}

    def lin(h, name):
        inp[name] = h.detach()
        z = h @ P[f'nerf.{name}.weight'].T + P[f'nerf.{name}.bias']
        z.retain_grad()
        pre[name] = z
        return z
    h = x_pe
    for i in range(8):
        h = lin(h, f'pts_linears.{i}') * masks[i]
        if i == 4:
            h = torch.cat([x_pe, h], -1)
    sigma = lin(h, 'alpha_linear')
    rgb = lin(lin(torch.cat([lin(h, 'feature_linear'), d_pe], -1), 'views_linears.0') * mask_hv, 'rgb_linear')
    raw = torch.cat([rgb, sigma], -1)
    raw.backward(torch.from_numpy(d_raw.astype(np.float64)))
    factors = {}
    for name, z in pre.items():
        dz, a = z.grad.abs(), inp[name].abs()
        factors[name] = (float(dz.max()), a.sum(0).numpy(), (dz.T @ a).numpy(), dz.sum(0).numpy())
    return raw.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}, factors, [bool((pre[f'pts_linears.{i}'].detach() > 0).ne(masks[i]).any()) for i in range(8)]


def train_step(G, monkeypatch, net, pts, dirs, d_raw, store16):
    monkeypatch.setattr(G.train, "GEMM_PRECISION", "mixed16")
    monkeypatch.setattr(G.train, "STORE16", store16)
    monkeypatch.setattr(G.train, "STORE16_MIN_ROWS", 1024)              # (the default sends batches this small to the float32 copies)
    for p in net.parameters():
        p.grad = None
    out = net(cu(pts), cu(dirs))
    node = out.grad_fn
    while node is not None and '_MLP' not in type(node).__name__:
        node = node.next_functions[0][0]
    assert (node.h16 is not None) == store16                            # the storage under test was taken
    masks = unpack_signs(node.bits)
    mask_hv = unpack_signs(node.hvbits) if store16 else (node.hv > 0).cpu()
    out.backward(cu(d_raw))
    return out.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in net.named_parameters()}, masks, mask_hv


# test_backward_net16_against_float64's bounds: a float32 dZ of the chain within CHAIN of its layer's largest entry ("the split-bf16 chain's 2e-5", gate 5e-5);
# an fp16 copy adds 2^-11 of the value; a bias gradient within CHAIN of the largest bias gradient of its layer.  The weight-gradient products: fp16 operands
# under fp16 storage (2^-11 each), split bf16 x3 under float32 storage (2^-17 each; neuman_hip/train.py).
CHAIN = 5e-5
PRODUCT = {True: 2.0 ** -10, False: 2.0 ** -16}
TRAIN_CASES = [(c, k) for c in E.FINITE_NETS if c.name in ("dead_layer", "dead_part", "scaled_layer-x400") for k in (("random", "zero", "eight_decades") if c.name == "dead_part" else ("random",))]


@pytest.mark.parametrize("store16", [True, False], ids=["fp16-storage", "float32-storage"])
@pytest.mark.parametrize("case,d_kind", TRAIN_CASES, ids=lambda x: x.name if hasattr(x, 'name') else x)
def test_training_step_on_edge_nets(G, monkeypatch, case, d_kind, store16):
    """one forward + backward of the background trainer's network call (nm_mlp_refresh_f16, nm_mlp_forward_save16 / _save_bits, the fused backward chain,
    the weight-gradient products) against float64 autograd of the torch network with the device's saved signs.  The raw output within the fp16x3 bound.
    A weight gradient is sum_n dZ[n][m] a[n][f] with dZ off by at most CHAIN max|dZ| and both operands rounded as PRODUCT says: entry (m, f) may be off by
    CHAIN max|dZ| sum_n |a[n][f]| + PRODUCT sum_n |dZ[n][m] a[n][f]|; a bias gradient by CHAIN of its layer's largest (+ 2^-11 sum_n |dZ[n][m]| under fp16
    storage, where a bias gradient is a sum of fp16 copies: nm_wgrad16's ones column).  A tensor whose
    float64 gradient is exactly zero (a dead layer and everything below it; an all-zero d_raw: nm_dz_scale(0)) is exactly zero."""
    j, sd, spec, plain = E.build(case)
    net = j.cuda().train()
    n = 1024
    pts, dirs = E.sample_points(n, seed=23, lim=1.0)
    rng = np.random.default_rng(5)
    d_raw = (rng.normal(size=(n, 4)) * 2e-5).astype(np.float32)
    if d_kind == "zero":
        d_raw[:] = 0
    elif d_kind == "eight_decades":
        d_raw *= (10.0 ** rng.uniform(-8, 0, size=(n, 1))).astype(np.float32)
    raw, g, masks, mask_hv = train_step(G, monkeypatch, net, pts, dirs, d_raw, store16)
    raw64, g64, factors, flipped = f64_autograd(sd, spec, pts, dirs, d_raw, masks, mask_hv)
    e_rgb, e_sig = errs(raw, raw64[:, :3], raw64[:, 3])
    b_rgb, b_sig = E.bounds("fp16x3", raw64[:, 3], spec.mapping)
    assert e_rgb < b_rgb and e_sig < b_sig
    worst = (0.0, None, 0.0)
    for name, ref in g64.items():
        got = g[name]
        assert np.isfinite(got).all(), name
        if not ref.any():
            assert not got.any(), f"{name}: the float64 gradient is exactly zero"
            continue
        dzmax, asum, prod, dzsum = factors[name[len('nerf.'):].rsplit('.', 1)[0]]
        if name.endswith('.weight'):
            tol = CHAIN * dzmax * asum[None, :] + PRODUCT[store16] * prod
        else:                                                  # (fp16 storage: the views layer's comes out of a product with the encoding's ones column, a sum of fp16 dZ)
            tol = CHAIN * float(np.abs(ref).max()) + 1e-12 + (2.0 ** -11 * dzsum if store16 else 0.0)
        ratio = float((np.abs(got - ref) / (tol + 1e-30)).max())
        worst = max(worst, (ratio, name, float(np.abs(got - ref).max() / np.abs(ref).max())))
        assert ratio < 1.0, (name, ratio)
    print(f"[mlp edges] {case.name} d_raw {d_kind} {'fp16' if store16 else 'float32'} storage: raw rgb {e_rgb:.2e} sigma {e_sig:.2e}; largest gradient error / its bound "
          f"{worst[0]:.2f} ({worst[1]}: {worst[2]:.1e} of the tensor's largest entry); layers with a sign on the other side of float64's: {sum(flipped)}")
    if case.name == "dead_layer":
        for i in range(3):
            assert not g[f'nerf.pts_linears.{i}.weight'].any() and not g[f'nerf.pts_linears.{i}.bias'].any()
    if d_kind == "zero":
        assert all(not v.any() for v in g.values())


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# c. large coordinates
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_large_coordinates(G):
    """points uniform in +-32 and eight at +-1000 through the unchanged posenc net.  The encoding: sin / cos within test_stage_by_stage's posenc bound of
    float64 sin / cos of the exact argument (the bands are powers of two); the raw coordinate within that bound times its magnitude (it is stored with the
    operand split's RELATIVE precision).  Outputs: BOUNDS times the largest hidden activation of the float64 net -- the raw coordinate is itself an input of
    layer 0, so every layer's magnitude grows with it (the scaling test_stage_by_stage applies per stage)."""
    case = E.EdgeNet('unchanged', 'unchanged', 'posenc', lambda m: None, True)
    j, sd, spec, plain = E.build(case)
    jc = j.cuda()
    pts, dirs = E.sample_points(512, seed=17, lim=32.0, far=8)
    x_pe = E.embed64(pts, 'posenc', *spec.pos)
    for prec in ("fp32", "bf16x3", "fp16x3"):
        pe = jc.forward_debug(cu(pts), cu(dirs), -1, precision=prec).cpu().numpy()
        tol = 2e-6 + (1.6e-5 if prec == "bf16x3" else 0)
        e_trig = float(np.abs(pe[:, 3:63] - x_pe[:, 3:]).max())
        e_raw = float((np.abs(pe[:, :3] - x_pe[:, :3]) / np.maximum(1.0, np.abs(x_pe[:, :3]))).max())
        print(f"[mlp edges] large coordinates {prec} encoding: sin / cos {e_trig:.2e}, raw coordinate (relative) {e_raw:.2e} (bound {tol:.1e})")
        assert e_trig < tol and e_raw < tol and np.abs(pe[:, 63]).max() == 0
    rgb64, sig64, hs = E.f64_network(sd, spec, pts, dirs, hidden=True)
    hmax = max(1.0, max(float(h.max()) for h in hs[:8]))
    o, d, z = as_rays(pts, dirs)
    for prec in PARITY:
        got = jc(cu(pts), cu(dirs), precision=prec).cpu().numpy()
        e_rgb, e_sig = errs(got, rgb64, sig64)
        b_rgb, b_sig = E.bounds(prec, sig64, 'posenc', scale=hmax)
        print(f"[mlp edges] large coordinates {prec}: largest hidden {hmax:.3g}, |sigma|max {np.abs(sig64).max():.3g}: rgb {e_rgb:.2e} (bound {b_rgb:.1e}) sigma {e_sig:.2e} (bound {b_sig:.1e})")
        assert np.isfinite(got).all() and e_rgb < b_rgb and e_sig < b_sig, prec
        if prec in ("fp16x3", "i8x3"):
            full = jc.forward_rays(o, d, z, precision=prec)
            dens = jc.forward_rays(o, d, z, precision=prec, sigma_only=True)
            assert torch.equal(dens[..., 3], full[..., 3])
            assert float(np.abs(dens[:, 0, 3].cpu().numpy() - sig64).max()) < b_sig


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# d. non-finite samples stay in their rows
# ---------------------------------------------------------------------------------------------------------------------------------------------------
N_POISON = 128 * 2 + 37
POISON_ROWS = [0, 31, 32, 63, 64, 127, 128, N_POISON - 1]
POISONS = {"nan_coordinate": ("pts", 0, float('nan')), "+inf_coordinate": ("pts", 1, float('inf')), "-inf_coordinate": ("pts", 2, float('-inf')),
           "nan_direction": ("dirs", 1, float('nan'))}
# Only launches whose addressing does not depend on a coordinate take such input: the network kernels index by row alone (csrc/mlp_device.h sample_input /
# sample_record; the encodings are arithmetic, csrc/mlp_device.h sincos_f64 / pe_feature).  The occupancy compaction and the sample lists it feeds, near / far
# and the closest-point search turn coordinates into indices and are not part of this test.
ENTRIES = ("points", "rays", "ray_chunk", "density_only")
PRECISIONS = ("fp32", "bf16x3", "bf16", "fp16x3", "i8x3")


def launch(jc, entry, prec, pts, dirs):
    p, d = cu(pts), cu(dirs)
    if entry == "points":
        return jc(p, d, precision=prec)
    z = torch.zeros((p.shape[0], 1), device='cuda')
    if entry == "rays":
        return jc.forward_rays(p, d, z, precision=prec)[:, 0]
    if entry == "density_only":
        return jc.forward_rays(p, d, z, precision=prec, sigma_only=True)[:, 0]
    idx = torch.arange(p.shape[0], device='cuda', dtype=torch.int32)
    live = torch.tensor([p.shape[0]], device='cuda', dtype=torch.int32)
    out = torch.full((p.shape[0], 1, 4), -7.0, device='cuda')
    jc.forward_ray_chunk(p, d, z, idx, live, 0, 1, out, precision=prec)
    return out[:, 0]


def poisoned(pts, dirs, poison):
    which, comp, value = POISONS[poison]
    p, d = pts.copy(), dirs.copy()
    (p if which == "pts" else d)[POISON_ROWS, comp] = value
    return p, d


def classify(x):
    """what the poisoned rows hold: 'nan' (every entry NaN), 'nonfinite' (none finite), 'finite' (all finite), 'mixed'"""
    if torch.isnan(x).all():
        return "nan"
    if not torch.isfinite(x).any():
        return "nonfinite"
    return "finite" if torch.isfinite(x).all() else "mixed"


def observe_poison(jc, entry, prec, poison, pts, dirs):
    clean = launch(jc, entry, prec, pts, dirs)
    got = launch(jc, entry, prec, *poisoned(pts, dirs, poison))
    keep = torch.ones(N_POISON, dtype=torch.bool, device='cuda')
    keep[POISON_ROWS] = False
    return torch.equal(got[keep], clean[keep]), classify(got[~keep][:, :3]), classify(got[~keep][:, 3])


# What the RENDER kernels return in a poisoned row, (colour, density) per (precision, poison); the same for the points, rays and ray-chunk entries;
# 'density_only' where that launch differs.  Their requantisation and clamps can swallow a NaN by design (inv_of(M) is 0 for a NaN row maximum,
# fmed3f returns a finite number for a NaN), and no instruction is spent on it: the table records the behaviour, the test pins it.
# Measured on an MI355X: every precision and entry returns FINITE values in a poisoned row, whatever the poison -- the ReLU is fmaxf / v_med3 / a clamp
# modifier, each of which answers a NaN with its other operand, so the first hidden layer already holds numbers again (an Inf coordinate becomes NaN in sin /
# cos and meets the same end).  A renderer fed non-finite samples therefore does NOT show them as NaN pixels; exceptions would be listed here per
# (precision, poison[, entry]).
POISON_TABLE = {}


def expected(entry, prec, poison):
    return POISON_TABLE.get((prec, poison, entry), POISON_TABLE.get((prec, poison), ("finite", "finite")))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_nonfinite_samples_stay_in_their_rows(G, entry, prec):
    if entry == "ray_chunk" and prec == "fp32":
        return                                                 # (the exact-f32 validation kernel has no chunked form)
    j, sd, spec, plain = E.build(E.EdgeNet('unchanged', 'unchanged', 'posenc', lambda m: None, True))
    jc = j.cuda()
    pts, dirs = E.sample_points(N_POISON, seed=41)
    for poison in POISONS:
        same, rgb, sigma = observe_poison(jc, entry, prec, poison, pts, dirs)
        print(f"[mlp edges] {entry} {prec} {poison}: other rows bit-identical {same}; poisoned rows: colour {rgb}, density {sigma}")
        assert same, (entry, prec, poison)
        assert (rgb, sigma) == expected(entry, prec, poison), (entry, prec, poison, rgb, sigma)


@pytest.mark.parametrize("store16", [True, False], ids=["fp16-storage", "float32-storage"])
def test_nonfinite_samples_in_the_training_forward(G, monkeypatch, store16):
    """a NaN batch has to reach the trainers' NaN check: all four outputs of a poisoned row are non-finite, as in the reference; every other row is
    bit-identical to the same launch on ordinary points"""
    monkeypatch.setattr(G.train, "GEMM_PRECISION", "mixed16")
    monkeypatch.setattr(G.train, "STORE16", store16)
    monkeypatch.setattr(G.train, "STORE16_MIN_ROWS", 256)
    j, sd, spec, plain = E.build(E.EdgeNet('unchanged', 'unchanged', 'posenc', lambda m: None, True))
    net = j.cuda().train()
    pts, dirs = E.sample_points(N_POISON, seed=41)
    clean = net(cu(pts), cu(dirs)).detach()
    assert torch.isfinite(clean).all()
    keep = torch.ones(N_POISON, dtype=torch.bool, device='cuda')
    keep[POISON_ROWS] = False
    for poison in POISONS:
        got = net(*[cu(x) for x in poisoned(pts, dirs, poison)]).detach()
        assert torch.equal(got[keep], clean[keep]), poison
        assert not torch.isfinite(got[~keep]).any(), (poison, got[~keep])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# e. non-finite weights on the device path
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _poison_parameter(nerf, what):
    with torch.no_grad():
        if what == "nan_trunk_weight":
            nerf.pts_linears[3].weight[1, 4] = float('nan')
        elif what == "inf_trunk_weight":
            nerf.pts_linears[6].weight[200, 17] = float('inf')
        elif what == "nan_trunk_bias":
            nerf.pts_linears[1].bias[77] = float('nan')
        elif what == "nan_views_bias":
            nerf.views_linears[0].bias[3] = float('nan')
        else:
            nerf.rgb_linear.weight[2, 100] = float('nan')


@pytest.mark.parametrize("store16", [True, False], ids=["fp16-storage", "float32-storage"])
@pytest.mark.parametrize("what", ["nan_trunk_weight", "inf_trunk_weight", "nan_trunk_bias", "nan_views_bias", "nan_rgb_weight"])
def test_nonfinite_weight_between_two_training_steps(G, monkeypatch, what, store16):
    """a parameter turns NaN / Inf between two training steps (a diverged optimiser step), so that only nm_mlp_refresh_f16 -- the device-side rebuild of
    the fp16 image, which asks the host nothing -- sees it: the next forward's raw output is NaN on every sample, as the reference's, and the trainers'
    math.isnan(total_loss) fires.  The rendering path, whose images the host packs, refuses the net."""
    monkeypatch.setattr(G.train, "GEMM_PRECISION", "mixed16")
    monkeypatch.setattr(G.train, "STORE16", store16)
    monkeypatch.setattr(G.train, "STORE16_MIN_ROWS", 256)
    j, sd, spec, plain = E.build(E.EdgeNet('unchanged', 'unchanged', 'posenc', lambda m: None, True))
    net = j.cuda().train()
    pts, dirs = E.sample_points(1000, seed=43)
    first = net(cu(pts), cu(dirs)).detach()
    assert torch.isfinite(first).all()
    _poison_parameter(net.nerf, what)
    second = net(cu(pts), cu(dirs)).detach()
    assert torch.isnan(second).all(), (what, int(torch.isfinite(second).sum()))
    net.eval()
    for prec in ("fp16x3", "i8x3", "bf16x3", "fp32"):
        with torch.no_grad(), pytest.raises(G.L.NeumanHipError, match="not finite"):
            net(cu(pts), cu(dirs), precision=prec)
