"""Host-side inputs and float64 references of tests/test_hip_train_edges.py (the training-step primitives of csrc/train.hip at their shape and
alignment edges).  Nothing here touches the device: every function is numpy / torch float64 on the host."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for _p in (ROOT, os.path.join(ROOT, "ml-neuman_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import train as OT  # noqa: E402

U = 2.0 ** -24                                                           # unit roundoff of float32
ACC, BIAS, RELU, MASK, COLSUM = 1, 2, 4, 8, 16                           # NM_GEMM_* (include/neuman_hip.h)


# ---- compositing adjoint ----------------------------------------------------------------------------------------------------------
# (S, R) of the one-wave-per-ray cases: every run-length regime of the kernel (c = ceil(S / 64) samples per lane: lanes without a sample, c = 2 with
# half the lanes empty, a ragged and a full last lane at c = 2 and c = 16) and every residue of R mod 4 (a workgroup holds four rays)
WAVE_CASES = [(1, 4), (2, 3), (63, 5), (64, 1), (65, 4), (127, 3), (129, 5), (1023, 1), (1024, 4)]
GRAD_SETS = {"all": (1, 1, 1, 1), "rgb": (1, 0, 0, 0), "depth": (0, 0, 1, 0), "weights": (0, 0, 0, 1)}     # which of g_rgb, g_acc, g_depth, g_weights is given


def mixed_rays(R, S, seed=11):
    """test_hip_train.saturated_rays, mixed: two rays in three run into an opaque region (alpha saturates to exactly 1, u = 1e-10, from sample `start` to
    the end of the ray), every third ray (r % 3 == 1) is ordinary; one sample in front has sigma <= 0.  The opaque density grows with S so that the
    shorter intervals of a long ray still saturate.  -> raw, z, d, [g_rgb, g_acc, g_depth, g_w], start (= S for an ordinary ray)"""
    assert S > 1 or R > 1
    rng = np.random.default_rng(seed + 1000 * S + R)
    raw = rng.normal(size=(R, S, 4)).astype(np.float32) * np.array([1, 1, 1, 3], np.float32)
    lo = min(4, S - 1)
    start = rng.integers(lo, max(lo + 1, min(S, max(20, S // 3))), size=R)
    start = np.where(np.arange(R) % 3 != 1, start, S)
    raw[..., 3] = np.where(np.arange(S)[None] >= start[:, None], np.float32(2000.0 * max(1.0, S / 64.0)), raw[..., 3])
    raw[1 if R > 1 else 0, 0, 3] = -0.5                                  # (R == 1: start >= 1 because S > 1)
    z = np.sort(rng.uniform(0.5, 4.0, size=(R, S)).astype(np.float32), -1)
    d = rng.normal(size=(R, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    g = [rng.normal(size=(R, 3)).astype(np.float32), rng.normal(size=R).astype(np.float32), rng.normal(size=R).astype(np.float32),
         (rng.normal(size=(R, S)) * 0.1).astype(np.float32)]
    return raw, z, d, g, start


@functools.lru_cache(maxsize=None)
def composite_case(R, S, white, grads="all"):
    """inputs + the float64 oracle's d_raw (read-only, shared by the tests that use the same case), with the two properties that keep a case from
    being vacuous checked on the oracle's own output"""
    raw, z, d, g, start = mixed_rays(R, S)
    use = GRAD_SETS[grads]
    full = [gi if u else np.zeros_like(gi) for gi, u in zip(g, use)]
    ora = OT.composite_backward(raw, z, d, white, *full)
    s = np.abs(ora).max()
    front = (np.arange(S)[None] <= start[:, None]) & (start[:, None] < S)         # up to the first sample of a saturated run (test_hip_train's `front`)
    assert front.any() and np.abs(ora[front]).max() > 1e-3 * s, (R, S, white, grads)
    dead = raw[..., 3] <= 0
    assert dead.any() and (ora[..., 3][dead] == 0).all()
    for a in (raw, z, d, ora, *g):
        a.setflags(write=False)
    return dict(raw=raw, z=z, d=d, g=[gi if u else None for gi, u in zip(g, use)], ora=ora, scale=s, dead=dead)


# ---- GEMM epilogues ---------------------------------------------------------------------------------------------------------------
PREC_FACTOR = {'f32': 1.0, 'fp16x3': 2.0, 'bf16x3': 10.0}


def gemm_gate(K, prec, terms=1):
    """test_hip_train.test_gemm's gate for a product of depth K"""
    return 3e-6 * np.sqrt(K) * PREC_FACTOR[prec] * 4 * terms


def gemm_inputs(M, N, K, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return dict(A=f(M, K), B=f(K, N), C0=f(M, N), bias=f(N), mask=f(M, N))


def gemm_reference(x, flags):
    """float64 relu?(A @ B + C0 + bias) * (mask > 0) of the float32 inputs"""
    r = x['A'].astype(np.float64) @ x['B'].astype(np.float64)
    if flags & ACC:
        r = r + x['C0'].astype(np.float64)
    if flags & BIAS:
        r = r + x['bias'].astype(np.float64)[None]
    if flags & RELU:
        r = np.maximum(r, 0.0)
    if flags & MASK:
        r = r * (x['mask'] > 0)
    return r


# ---- positional encoding ----------------------------------------------------------------------------------------------------------
def pe_table(kind, n_freqs):
    """posenc: the bands 2^linspace(0, n - 1, n) as float32 (models/vanilla.py:67-68); rotate: the caller passes the Embedder's table"""
    assert kind == 'posenc'
    return (2. ** torch.linspace(0, max(n_freqs - 1, 0), steps=n_freqs)).numpy().astype(np.float32)


def pe_width(kind, dims, n_freqs):
    return dims + 2 * dims * n_freqs if kind == 'posenc' else 3 + 6 * n_freqs


def pe_reference(kind, x, table, g=None):
    """models/vanilla.py:60-92 in float64 from the float32 inputs and table -> (features [n, width], |argument| bound per feature [n, width],
    and with g [n, >= width]: dx = the adjoint contracted with g[:, :width] through autograd, and its rounding scale per coordinate)"""
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    tab = torch.tensor(np.asarray(table), dtype=torch.float64)
    n, D = xt.shape
    if kind == 'posenc':
        out, arg = [xt], [torch.zeros_like(xt)]
        for f in tab:
            out += [torch.sin(xt * f), torch.cos(xt * f)]
            arg += [(xt * f).abs()] * 2                                  # (x * 2^b is exact in float32)
    else:
        proj = xt @ tab.T
        a = xt.abs() @ tab.abs().T                                       # sum_j |x_j B_mj|: what the three roundings of the float32 dot product scale with
        out, arg = [xt, torch.sin(proj), torch.cos(proj)], [torch.zeros_like(xt), a, a]
    feats, arg = torch.cat(out, -1), torch.cat(arg, -1).detach()
    if g is None:
        return feats.detach().numpy(), arg.numpy()
    w = feats.shape[1]
    gt = torch.tensor(np.asarray(g), dtype=torch.float64)[:, :w]
    (feats * gt).sum().backward()
    ga = gt.abs()
    if kind == 'posenc':
        nf = tab.shape[0]
        scale = ga[:, :D].clone()
        for b in range(nf):
            scale += tab[b] * (ga[:, D + 2 * D * b:D + 2 * D * b + D] + ga[:, D + 2 * D * b + D:D + 2 * D * b + 2 * D])
        lit = scale
    else:
        n3 = tab.shape[0]
        gsc = ga[:, 3:3 + n3] + ga[:, 3 + n3:3 + 2 * n3]                 # |g_sin| + |g_cos| per projection m
        lit = ga[:, :3] + gsc @ tab.abs()                                # the sum with |B| alone ...
        scale = ga[:, :3] + (gsc * (1.0 + a.detach())) @ tab.abs()       # ... and with the rounding of each argument, which moves its sin and cos by as much
    return feats.detach().numpy(), arg.numpy(), xt.grad.numpy(), scale.numpy(), lit.numpy()


def rotate_argument_float32(x, B):
    """x . B_m as the kernels form it: fmaf(x2, b2, fmaf(x1, b1, x0 * b0)) in float32 (a fused multiply-add = one rounding of the float64 value)"""
    f32, f64 = np.float32, np.float64
    a = (x[:, 0:1] * B[None, :, 0]).astype(f32)
    a = (x[:, 1:2].astype(f64) * B[None, :, 1] + a).astype(f32)
    return (x[:, 2:3].astype(f64) * B[None, :, 2] + a).astype(f32)


def pe_encode_float32(x, table):
    """the rotate encoding in float32 on the host, sin / cos correctly rounded"""
    x, B = np.asarray(x, np.float32), np.asarray(table, np.float32)
    a = rotate_argument_float32(x, B).astype(np.float64)
    return np.concatenate([x, np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)], 1)


def pe_backward_float32(x, table, g):
    """The rotate adjoint evaluated the way pe_backward_kernel does, in float32 on the host (the fused multiply-adds as one rounding of the float64
    value, sin / cos correctly rounded): what ANY float32 evaluation of that expression is good for"""
    f32, f64 = np.float32, np.float64
    x, B, g = np.asarray(x, f32), np.asarray(table, f32), np.asarray(g, f32)
    n3 = B.shape[0]
    d = g[:, :3].copy()
    arg = rotate_argument_float32(x, B)
    for m in range(n3):
        a = arg[:, m]
        sn, cs = np.sin(a.astype(f64)).astype(f32), np.cos(a.astype(f64)).astype(f32)
        t = ((g[:, 3 + m] * cs).astype(f32) - (g[:, 3 + n3 + m] * sn).astype(f32)).astype(f32)
        for k in range(3):
            d[:, k] = (d[:, k] + (B[m, k] * t).astype(f32)).astype(f32)
    return d


# ---- 16-bit weight gradients ------------------------------------------------------------------------------------------------------
def slot_perm():
    """perm[p] = the feature held by k-slot p = 8 c + e of a row (mlp_layout.h slot_feature)"""
    p = np.arange(256)
    c, e = p >> 3, p & 7
    return 32 * (c >> 2) + 8 * (2 * ((c >> 1) & 1) + (e >> 2)) + 4 * (c & 1) + (e & 3)


def dz_scale(amax):
    """nm_dz_scale: the power of two that puts amax into [2, 4)"""
    m, e = np.frexp(np.float32(amax))
    return float(2.0 ** (2 - e))
