"""-m gpu: the training-step primitives of csrc/train.hip at their shape and alignment edges -- both compositing-adjoint kernels in every run-length
regime, the narrow and the column-sum GEMM epilogues, nm_colsum, nm_pe_encode / nm_pe_encode16 / nm_pe_backward, and the band kernels of the 16-bit
weight gradients at fewer rows than row groups and around one full band.  Every reference is float64 on the host (tests/helpers/train_edges.py,
oracle.train.composite_backward); where a test says which kernel or epilogue ran, it evaluates the entry point's dispatch condition on its own
arguments."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import train_edges as E  # noqa: E402
from train_edges import ACC, BIAS, RELU, MASK, COLSUM, U  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 7.0                                                                # what every float a kernel must not write holds


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from neuman_hip import _lib, synthetic, train
    return types.SimpleNamespace(lib=_lib.lib(), L=_lib, syn=synthetic, train=train)


def cu(x):
    return torch.tensor(np.asarray(x, np.float32), device='cuda').contiguous()


def ptr(t, off=0):
    """device pointer `off` floats into a tensor"""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def carve(x, off, pad=8):
    """x as a view `off` floats into a larger buffer of sentinels -> (parent, view)"""
    x = np.asarray(x, np.float32)
    parent = torch.full((x.size + pad,), SENT, device='cuda')
    view = parent[off:off + x.size]
    view.copy_(torch.tensor(x.ravel()))
    return parent, view


# =====================================================================================================================================
# 1. compositing adjoint
# =====================================================================================================================================
def takes_wave_kernel(raw, d_raw, S):
    """nm_composite_backward's dispatch: S <= 64 * kCbMax and raw, d_raw 16-byte aligned"""
    return S <= 1024 and ((raw.data_ptr() | d_raw.data_ptr()) & 15) == 0


def composite_backward(G, c, R, S, white, offset=0):
    """the C entry point on case `c`; raw and d_raw `offset` floats into larger buffers -> (d_raw [R,S,4] numpy, parent of d_raw numpy, wave kernel?)"""
    _, raw = carve(c['raw'], offset)
    parent, d_raw = carve(np.full(c['raw'].shape, SENT, np.float32), offset)
    g = [None if gi is None else cu(gi) for gi in c['g']]
    z, d = cu(c['z']), cu(c['d'])
    wave = takes_wave_kernel(raw, d_raw, S)
    G.L.check(G.lib.nm_composite_backward(ptr(raw), ptr(z), ptr(d), R, S, int(white), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]),
                                          ptr(d_raw), G.L.stream_ptr()), "nm_composite_backward")
    return d_raw.cpu().numpy().reshape(R, S, 4), parent.cpu().numpy(), wave


def check_composite(c, got, parent, offset, what):
    err = np.abs(got - c['ora']).max()
    print(f"[train-edges] composite backward {what}: max |grad| {c['scale']:.3e}, device vs float64 {err / c['scale']:.2e} of it")
    assert np.isfinite(got).all() and err < 2e-5 * c['scale'], (what, err / c['scale'])      # test_composite_backward's gate
    assert (got[..., 3][c['dead']] == 0).all(), what                      # sigma <= 0: exactly no gradient
    outside = np.ones(parent.size, bool)
    outside[offset:offset + got.size] = False
    assert (parent[outside] == SENT).all(), what


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("S,R", E.WAVE_CASES)
def test_composite_backward_wave_kernel(G, S, R, white):
    """one wave per ray: lanes without a sample (S < 64), c = 2 with half the lanes empty (65), ragged and full last lanes (127, 129, 1023, 1024), workgroups
    with one to three idle waves (R mod 4)"""
    c = E.composite_case(R, S, white)
    got, parent, wave = composite_backward(G, c, R, S, white)
    assert wave
    check_composite(c, got, parent, 0, f"wave kernel R={R} S={S} white={white}")


@pytest.mark.parametrize("white", [True, False])
def test_composite_backward_serial_kernel_by_size(G, white):
    """S = 1025 > 64 * kCbMax: one lane per ray, T_i parked as a double in the d_raw records; ~700 saturated samples behind the visible ones"""
    R, S = 5, 1025
    c = E.composite_case(R, S, white)
    got, parent, wave = composite_backward(G, c, R, S, white)
    assert not wave
    check_composite(c, got, parent, 0, f"serial kernel R={R} S={S} white={white}")


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("S,R", [(1, 4), (2, 3), (64, 1), (65, 4)])
def test_composite_backward_serial_kernel_by_alignment(G, S, R, white):
    """raw and d_raw 8 bytes (not 16) into their buffers: the serial kernel on the wave kernel's inputs -- against float64, against the wave kernel (both
    accumulate in float64: only the association differs), and nothing written outside [R][S][4]"""
    c = E.composite_case(R, S, white)
    got, parent, wave = composite_backward(G, c, R, S, white, offset=2)
    assert not wave
    check_composite(c, got, parent, 2, f"serial kernel (8-byte aligned) R={R} S={S} white={white}")
    ref, _, wave = composite_backward(G, c, R, S, white)
    assert wave
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("grads", ["rgb", "weights", "depth", "all"])
@pytest.mark.parametrize("offset", [0, 2])
def test_composite_backward_optional_gradients(G, offset, grads, white):
    """each output gradient alone (the others null) and all four, on both kernels (offset 2: the serial one)"""
    R, S = 4, 65
    c = E.composite_case(R, S, white, grads)
    got, parent, wave = composite_backward(G, c, R, S, white, offset=offset)
    assert wave == (offset == 0)
    check_composite(c, got, parent, offset, f"{'wave' if wave else 'serial'} kernel, g_{grads} only, white={white}")


def test_composite_backward_refuses_a_4_byte_aligned_d_raw(G):
    """the serial kernel stores doubles into d_raw and is the one misaligned callers get: an odd float offset is an argument error, before any launch"""
    R, S = 3, 2
    c = E.composite_case(R, S, True)
    raw, z, d, g_rgb = cu(c['raw']), cu(c['z']), cu(c['d']), cu(c['g'][0])
    parent, d_raw = carve(np.full((R, S, 4), SENT, np.float32), 1)
    assert d_raw.data_ptr() % 8 == 4
    rc = G.lib.nm_composite_backward(ptr(raw), ptr(z), ptr(d), R, S, 1, ptr(g_rgb), None, None, None, ptr(d_raw), G.L.stream_ptr())
    assert rc != 0 and b"d_raw" in G.lib.nm_last_error()
    with pytest.raises(G.L.NeumanHipError):
        G.L.check(rc, "nm_composite_backward")
    assert bool((parent == SENT).all())


# =====================================================================================================================================
# 2. GEMM: the narrow epilogue (store_tile) and the column-sum epilogue
# =====================================================================================================================================
# name -> (C offset, ldc - N, ldmask - N, bias offset), offsets in floats
LAYOUTS = {"wide": (0, 4, 4, 0), "ldc+1": (0, 1, 4, 0), "C+1": (1, 4, 4, 0), "ldmask+3": (0, 4, 3, 0), "bias+1": (0, 4, 4, 1)}
EPILOGUES = [(0, ("ldc+1", "C+1")), (ACC, ("ldc+1", "C+1")), (BIAS | RELU, ("ldc+1", "C+1", "bias+1")), (MASK, ("ldc+1", "C+1", "ldmask+3")),
             (ACC | MASK, ("ldc+1", "C+1", "ldmask+3"))]


def wide_ok(c_ptr, ldc, flags, mask_ptr, ldmask, bias_ptr):
    """train.hip wide_ok(): which epilogue a (non split-K) product takes"""
    return ((c_ptr & 15) == 0 and (ldc & 3) == 0 and (not (flags & MASK) or ((mask_ptr & 15) == 0 and (ldmask & 3) == 0))
            and (not (flags & BIAS) or (bias_ptr & 15) == 0))


class Gemm:
    """one product's operands on the device; run() lays C / mask / bias out as asked and returns what the device left"""

    def __init__(self, G, M, N, K, akm, bkm, prec, seed=0):
        self.G, self.M, self.N, self.K, self.akm, self.bkm, self.prec = G, M, N, K, akm, bkm, prec
        self.x = x = E.gemm_inputs(M, N, K, seed + M * 7 + N * 3 + K + akm * 2 + bkm)
        a, b = (x['A'].T if akm else x['A']), (x['B'] if bkm else x['B'].T)
        pad = lambda m: np.pad(m, ((0, max(0, 4 - m.shape[0])), (0, max(0, 4 - m.shape[1]))))      # (K = 0: a real pointer and a legal leading dimension)
        self.a, self.b = cu(pad(a)), cu(pad(b))
        self.fn = {'f32': G.lib.nm_gemm_f32, 'bf16x3': G.lib.nm_gemm_bf16x3, 'fp16x3': G.lib.nm_gemm_fp16x3}[prec]

    def run(self, flags, layout="wide", ws_floats=None, ws_short=0):
        M, N, K, x = self.M, self.N, self.K, self.x
        c_off, dc, dm, b_off = LAYOUTS[layout]
        ldc, ldmask = N + dc, N + dm
        cbuf = torch.full((c_off + M * ldc + 8,), SENT, device='cuda')
        torch.as_strided(cbuf, (M, N), (ldc, 1), c_off).copy_(torch.from_numpy(x['C0']))        # (ignored unless ACCUMULATE)
        mbuf = torch.full((M * ldmask + 8,), SENT, device='cuda')
        torch.as_strided(mbuf, (M, N), (ldmask, 1), 0).copy_(torch.from_numpy(x['mask']))
        _, bias = carve(x['bias'], b_off)
        ws = None
        if flags & COLSUM:
            bands = (M + 63) // 64
            ws = torch.full((bands * N + 16,), SENT, device='cuda')
            ws_floats = bands * N - ws_short
        wide = wide_ok(cbuf.data_ptr() + 4 * c_off, ldc, flags, mbuf.data_ptr(), ldmask, bias.data_ptr())
        rc = self.fn(self.akm, self.bkm, M, N, K, ptr(self.a), self.a.shape[1], ptr(self.b), self.b.shape[1], ptr(cbuf, c_off), ldc,
                     ptr(bias) if flags & BIAS else None, ptr(mbuf) if flags & MASK else None, ldmask, flags, ptr(ws), ws_floats or 0, self.G.L.stream_ptr())
        full = cbuf.cpu().numpy()
        idx = c_off + np.arange(M)[:, None] * ldc + np.arange(N)[None]
        outside = np.ones(full.size, bool)
        outside[idx] = False
        return types.SimpleNamespace(rc=rc, wide=wide, C=full[idx], untouched=bool((full[outside] == SENT).all()), ws=None if ws is None else ws.cpu().numpy())


def flag_names(f):
    return "|".join(n for n, b in (("ACC", ACC), ("BIAS", BIAS), ("RELU", RELU), ("MASK", MASK), ("COLSUM", COLSUM)) if f & b) or "plain"


@pytest.mark.parametrize("M,N,K", [(4, 4, 4), (68, 36, 20), (260, 132, 36)])
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "fp16x3"])
def test_gemm_narrow_epilogue(G, M, N, K, prec):
    """odd ldc, C one float into its buffer, odd ldmask, bias one float into its buffer: store_tile, in every epilogue -- against float64, with the spare
    columns and the floats in front of C untouched, and bit-identical to the wide epilogue on the same inputs laid out aligned"""
    for akm, bkm in ([(0, 0), (0, 1), (1, 1), (1, 0)] if prec == "f32" else [(0, 1), (1, 1)]):
        g = Gemm(G, M, N, K, akm, bkm, prec)
        for flags, layouts in EPILOGUES:
            ref = E.gemm_reference(g.x, flags)
            w = g.run(flags)
            assert w.rc == 0 and w.wide and w.untouched
            for lay in layouts:
                r = g.run(flags, lay)
                what = (prec, (M, N, K), (akm, bkm), flag_names(flags), lay)
                assert r.rc == 0 and not r.wide, what                     # the narrow epilogue ran
                assert np.abs(r.C - ref).max() < E.gemm_gate(K, prec), (what, np.abs(r.C - ref).max())
                assert r.untouched, what
                assert np.array_equal(r.C.view(np.uint32), w.C.view(np.uint32)), what


@pytest.mark.parametrize("K", [0, 4])
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "fp16x3"])
def test_gemm_less_than_one_k_tile(G, K, prec):
    """K = 0 (no k-tile at all: C = the epilogue of zeros, exactly) and K = 4 (a quarter of the f32 kernel's tile, an eighth of the split kernels') on both
    epilogues"""
    M, N = 68, 36
    for akm, bkm in [(0, 0), (0, 1), (1, 1), (1, 0)]:
        g = Gemm(G, M, N, K, akm, bkm, prec)
        for flags in (0, ACC, BIAS | RELU, ACC | MASK):
            ref = E.gemm_reference(g.x, flags)
            for lay in ("wide", "ldc+1"):
                r = g.run(flags, lay)
                what = (prec, K, (akm, bkm), flag_names(flags), lay)
                assert r.rc == 0 and r.wide == (lay == "wide") and r.untouched, what
                if K == 0:
                    assert np.array_equal(r.C, ref.astype(np.float32)), what      # (0 + C0 + bias: at most one float32 value each, no rounding)
                else:
                    assert np.abs(r.C - ref).max() < E.gemm_gate(K, prec), (what, np.abs(r.C - ref).max())


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "fp16x3"])
def test_gemm_colsum_epilogue(G, prec):
    """NM_GEMM_COLSUM: workspace [ceil(M / 64)][N] = the column sums of the C the device stored (after mask / ReLU), per band of 64 rows.
    Tolerance 2^-23 * 24 * sum |C[:, col]|: a band value is a float32 sum of at most 64 terms, per lane a chain of 16 rows, then two butterfly steps over
    the four lanes that share a column -- depth 18 <= 24 roundings of at most 2^-24 of the running magnitude each."""
    K = 36
    worst = 0.0
    for M in (4, 60, 64, 68, 260):
        for N in (4, 28, 132, 256):
            g = Gemm(G, M, N, K, 0, 1, prec)
            bands = (M + 63) // 64
            for flags in (COLSUM, MASK | COLSUM, ACC | MASK | COLSUM, BIAS | RELU | COLSUM):
                r = g.run(flags)
                what = (prec, (M, N, K), flag_names(flags))
                assert r.rc == 0 and r.wide and r.untouched, what
                assert np.abs(r.C - E.gemm_reference(g.x, flags)).max() < E.gemm_gate(K, prec), what
                C = r.C.astype(np.float64)
                got = r.ws[:bands * N].astype(np.float64).reshape(bands, N)
                assert (r.ws[bands * N:] == SENT).all(), what
                tol = 2.0 ** -23 * 24 * np.abs(C).sum(0)
                err = np.abs(got.sum(0) - C.sum(0))
                worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
                assert (err <= tol).all(), (what, float((err - tol).max()))
                for b in range(bands):                                    # ... and every row went to its own band
                    Cb = C[64 * b:64 * b + 64]
                    assert (np.abs(got[b] - Cb.sum(0)) <= 2.0 ** -23 * 24 * np.abs(Cb).sum(0)).all(), (what, b)
    print(f"[train-edges] {prec} NM_GEMM_COLSUM: worst column-sum error {worst:.3f} of its tolerance")


def test_gemm_refusals(G):
    """argument errors, nothing launched: C keeps its contents"""
    big = Gemm(G, 256, 28, 8192, 0, 1, "bf16x3")
    assert int(G.lib.nm_gemm_workspace_floats(256, 28, 8192)) > 0          # a split-K shape
    small = Gemm(G, 68, 36, 20, 0, 1, "f32")
    ws = torch.empty(int(G.lib.nm_gemm_workspace_floats(256, 28, 8192)), device='cuda')
    for g, flags, lay, kw, word in ((big, COLSUM, "wide", {}, b"split-K"), (small, COLSUM, "C+1", {}, b"aligned"),
                                    (small, COLSUM, "ldc+1", {}, b"aligned"), (small, COLSUM, "wide", dict(ws_short=1), b"workspace")):
        r = g.run(flags, lay, **kw)
        assert r.rc != 0 and word in G.lib.nm_last_error(), (flag_names(flags), lay, G.lib.nm_last_error())
        with pytest.raises(G.L.NeumanHipError):
            G.L.check(r.rc, "nm_gemm")
        assert r.untouched and np.array_equal(r.C, g.x['C0'])
    # split-K with BIAS: the workspace is there, the epilogue is what is refused
    M, N, K = 256, 28, 8192
    C = torch.full((M, N), SENT, device='cuda')
    bias = cu(big.x['bias'])
    rc = big.fn(0, 1, M, N, K, ptr(big.a), big.a.shape[1], ptr(big.b), big.b.shape[1], ptr(C), N, ptr(bias), None, 0, BIAS, ptr(ws), ws.numel(), G.L.stream_ptr())
    assert rc != 0 and b"split-K" in G.lib.nm_last_error() and bool((C == SENT).all())


# =====================================================================================================================================
# 3. nm_colsum
# =====================================================================================================================================
def test_colsum(G):
    """out[W] = column sums of X [n, W] (row stride ld) against float64.  Tolerance 2^-23 * depth * sum |x|, depth = 35 + ceil(bands / 64) + 6: a band of
    256 rows is eight interleaved chains of at most 32 adds (31 + a tail of up to 7 on the first chain when the band is ragged: 38) and three levels of
    pairwise adds; the second stage adds ceil(bands / 64) band values per lane and six butterfly levels.  Each add rounds by at most 2^-24 of the
    running magnitude <= sum |x|, so the error is at most (38 + 3 + ceil(bands / 64) + 6) * 2^-24 * sum |x|, which the stated form (with 2^-23) covers."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for n in (0, 1, 7, 8, 9, 255, 256, 257, 64 * 256 + 257):                 # the last: 66 bands, the second stage's lane loop wraps
        for W in (1, 3, 4, 5, 256, 259):
            for ld in (W, W + 3):
                X = rng.normal(size=(n, ld)).astype(np.float32)
                x = cu(X) if n else None
                out = torch.full((W + 5,), SENT, device='cuda')
                need = int(G.lib.nm_colsum_workspace_floats(n, W))
                bands = (n + 255) // 256
                assert need == bands * W
                ws = torch.full((need + 4,), SENT, device='cuda')
                G.L.check(G.lib.nm_colsum(ptr(x), n, W, ld, ptr(out), ptr(ws), need, G.L.stream_ptr()), "nm_colsum")
                o = out.cpu().numpy()
                assert (o[W:] == SENT).all() and bool((ws[need:] == SENT).all()), (n, W, ld)
                if n == 0:
                    assert (o[:W] == 0).all(), (W, ld)
                    continue
                X64 = X[:, :W].astype(np.float64)
                depth = 35 + math.ceil(bands / 64) + 6
                tol = 2.0 ** -23 * depth * np.abs(X64).sum(0)
                err = np.abs(o[:W] - X64.sum(0))
                worst = max(worst, float((err / tol).max()))
                assert (err <= tol).all(), (n, W, ld, float((err / tol).max()))
    print(f"[train-edges] nm_colsum: worst error {worst:.3f} of its tolerance")
    x, out, ws = cu(rng.normal(size=(257, 5))), torch.full((5,), SENT, device='cuda'), torch.empty(16, device='cuda')
    rc = G.lib.nm_colsum(ptr(x), 257, 5, 5, ptr(out), ptr(ws), 2 * 5 - 1, G.L.stream_ptr())      # one float short
    assert rc != 0 and b"workspace" in G.lib.nm_last_error() and bool((out == SENT).all())


# =====================================================================================================================================
# 4. positional encoding and its adjoint
# =====================================================================================================================================
PE_NS = (0, 1, 127, 128, 129, 257)


def pe_mappings(G):
    """(name, kind, dims, n_freqs, table)"""
    rot = G.syn.make_variant_joiner(0, posenc='rotate').pos_pe
    assert rot.mapping == 'rotate'
    return [("posenc3x%d" % f, 'posenc', 3, f, E.pe_table('posenc', f)) for f in (0, 4, 10)] + [("posenc4x6", 'posenc', 4, 6, E.pe_table('posenc', 6)),
                                                                                             ("rotate", 'rotate', 3, rot.N_freqs, rot.table())]


def pe_lds(width):
    return sorted({width, (width + 63) // 64 * 64, 120})


def pe_inputs(n, dims, ld, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-2, 2, size=(n, dims)).astype(np.float32), rng.normal(size=(n, ld)).astype(np.float32))


def test_pe_encode(G):
    """nm_pe_encode against the float64 formula: |value - float64| <= 4 * 2^-24 * (1 + |argument|) (the rounding of the argument, which moves sin / cos by as
    much, and of sinf / cosf); posenc's argument x * 2^b is exact, rotate's is a three-term float32 dot product, whose roundings scale with
    sum_j |x_j B_mj| -- that sum stands for |argument| there.  The input columns are copied exactly, the padding columns are exactly 0."""
    worst = 0.0
    for name, kind, dims, nf, table in pe_mappings(G):
        width = E.pe_width(kind, dims, nf)
        tab = cu(table) if nf else None
        for n in PE_NS:
            for ld in pe_lds(width):
                X, _ = pe_inputs(n, dims, ld, 17 * n + ld)
                x = cu(X) if n else None
                out = torch.full((n + 2, ld), SENT, device='cuda')
                G.L.check(G.lib.nm_pe_encode(ptr(x), n, dims, G.L.NM_PE_ROTATE if kind == 'rotate' else G.L.NM_PE_POSENC, nf, ptr(tab), ptr(out), ld,
                                             G.L.stream_ptr()), "nm_pe_encode")
                o = out.cpu().numpy()
                assert (o[n:] == SENT).all(), (name, n, ld)
                if n == 0:
                    continue
                ref, arg = E.pe_reference(kind, X, table)
                assert np.array_equal(o[:n, :dims], X) and (o[:n, width:] == 0).all(), (name, n, ld)
                ratio = np.abs(o[:n, :width] - ref) / (4 * U * (1 + arg))
                worst = max(worst, float(ratio.max()))
                assert ratio.max() <= 1.0, (name, n, ld, float(ratio.max()))
                if kind == 'rotate' and n == 257 and ld == width:        # why |x . B_m| itself cannot stand for |argument|: float32 on the HOST misses that
                    lit = np.abs(ref) * 0
                    lit[:, dims:] = np.tile(np.abs(X.astype(np.float64) @ np.asarray(table, np.float64).T), (1, 2))
                    host = np.abs(E.pe_encode_float32(X, table) - ref) / (4 * U * (1 + lit))
                    print(f"[train-edges] rotate encoding, float32 on the HOST: {host.max():.1f} of 4 * 2^-24 * (1 + |x . B_m|)")
                    assert host.max() > 1.0
    print(f"[train-edges] nm_pe_encode: worst error {worst:.3f} of 4 * 2^-24 * (1 + |argument|)")


def test_pe_encode16_edges(G):
    """nm_pe_encode16 == fp16(32 x nm_pe_encode) bit for bit (test_pe_encode16's statement) for the 4-D encoding at the row counts around a 256-thread
    block's edge, the ones column at the first padding column and at ld - 1; a ones column inside the encoding or beyond the row is refused"""
    dims, nf = 4, 6
    width = E.pe_width('posenc', dims, nf)
    tab = cu(E.pe_table('posenc', nf))
    for n in PE_NS:
        for ld in (64, 120):
            X, _ = pe_inputs(n, dims, ld, 5 * n + ld)
            x = cu(X) if n else None
            a = torch.full((n + 1, ld), SENT, device='cuda')
            G.L.check(G.lib.nm_pe_encode(ptr(x), n, dims, 0, nf, ptr(tab), ptr(a), ld, G.L.stream_ptr()), "nm_pe_encode")
            for ones in (width, ld - 1):
                b = torch.full((n + 1, ld), SENT, device='cuda', dtype=torch.float16)
                G.L.check(G.lib.nm_pe_encode16(ptr(x), n, dims, 0, nf, ptr(tab), ptr(b), ld, ones, G.L.stream_ptr()), "nm_pe_encode16")
                want = (a * 32).half()
                want[:n, ones] = 32
                want[n:] = SENT
                assert torch.equal(b, want), (n, ld, ones)
    x, b = cu(pe_inputs(9, dims, 64, 1)[0]), torch.full((9, 64), SENT, device='cuda', dtype=torch.float16)
    for ones in (width - 1, 3, 64, 200):
        rc = G.lib.nm_pe_encode16(ptr(x), 9, dims, 0, nf, ptr(tab), ptr(b), 64, ones, G.L.stream_ptr())
        assert rc != 0 and b"ones_col" in G.lib.nm_last_error(), ones
    assert bool((b == SENT).all())


def test_pe_backward(G):
    """nm_pe_backward against autograd of the float64 encoding contracted with the same g; g is random in the padding columns too, which the adjoint must not
    read into dx.  Bound per coordinate k: 8 * 2^-24 * (|g_x| + sum_b f_b (|g_sin| + |g_cos|)) for posenc (x * 2^b is exact; what is left are the roundings of
    sincosf, of the products and of the running float32 sum).  rotate: 8 * 2^-24 * (|g_x| + sum_m |B_mk| (|g_sin,m| + |g_cos,m|) (1 + sum_j |x_j B_mj|)) --
    the float32 dot product x . B_m carries up to three roundings of 2^-24 sum_j |x_j B_mj|, and sin / cos move by as much as their argument; the same sum
    without that factor is below what a float32 evaluation of the expression in the kernel's order gives on the host (E.pe_backward_float32, asserted
    here on the host values so that the reason stays on record)."""
    worst = {}
    for name, kind, dims, nf, table in pe_mappings(G):
        width = E.pe_width(kind, dims, nf)
        tab = cu(table) if nf else None
        code = G.L.NM_PE_ROTATE if kind == 'rotate' else G.L.NM_PE_POSENC
        for n in PE_NS:
            for ld in pe_lds(width):
                X, g = pe_inputs(n, dims, ld, 31 * n + ld)
                x, gd = (cu(X), cu(g)) if n else (None, None)
                dx = torch.full((n + 3, dims), SENT, device='cuda')
                G.L.check(G.lib.nm_pe_backward(ptr(x), n, dims, code, nf, ptr(tab), ptr(gd), ld, ptr(dx), G.L.stream_ptr()), "nm_pe_backward")
                o = dx.cpu().numpy()
                assert (o[n:] == SENT).all(), (name, n, ld)
                if n == 0:
                    continue
                _, _, ref, scale, literal = E.pe_reference(kind, X, table, g)
                ratio = np.abs(o[:n] - ref) / (8 * U * scale)
                worst[name] = max(worst.get(name, 0.0), float(ratio.max()))
                assert ratio.max() <= 1.0, (name, n, ld, float(ratio.max()))
                if kind == 'rotate' and n == 257 and ld == width:
                    host = np.abs(E.pe_backward_float32(X, table, g) - ref) / (8 * U * literal)
                    print(f"[train-edges] rotate adjoint, float32 on the HOST in the kernel's order: {host.max():.1f} of the bound without the argument's rounding")
                    assert host.max() > 1.0
    print("[train-edges] nm_pe_backward: worst error as a fraction of its bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    x, g, dx = cu(pe_inputs(5, 3, 121, 1)[0]), cu(pe_inputs(5, 3, 121, 1)[1]), torch.full((5, 3), SENT, device='cuda')
    tab = cu(E.pe_table('posenc', 10))
    rc = G.lib.nm_pe_backward(ptr(x), 5, 3, 0, 10, ptr(tab), ptr(g), 121, ptr(dx), G.L.stream_ptr())
    assert rc != 0 and b"ld 121" in G.lib.nm_last_error() and bool((dx == SENT).all())


# =====================================================================================================================================
# 5. the 16-bit weight-gradient kernels at small and band-edge n
# =====================================================================================================================================
PERM = E.slot_perm()


def rel_err(got, ref):
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())


def h64(t16, scale):
    return t16.cpu().numpy().astype(np.float64) / scale


def wgrad16(G, p_cols, q_cols, dz16, act16, out, off, amax, n):
    P, Q = (ctypes.c_void_p * 1)(dz16.data_ptr()), (ctypes.c_void_p * 1)(act16.data_ptr())
    C, Ld = (ctypes.c_void_p * 1)(out.data_ptr() + 4 * off), (ctypes.c_int * 1)(out.shape[1])
    ws = torch.empty(int(G.lib.nm_wgrad16_workspace_floats(1, n, p_cols, q_cols)), device='cuda')
    G.L.check(G.lib.nm_wgrad16(1, p_cols, q_cols, P, Q, C, Ld, n, ptr(amax), ptr(ws), ws.numel(), G.L.stream_ptr()), "nm_wgrad16")


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 65, 511, 512, 513])
def test_wgrad16_kernels_at_small_and_band_edge_n(G, n):
    """fewer rows than row groups (the band kernels stride by 2, 8, 64), one row past a group, one band of 512 less a row, exactly, and one row more;
    reference and gate of test_wgrad16_against_float64: the float64 product of the fp16 operands, err / max |ref| < 2e-6"""
    g = torch.Generator(device='cuda').manual_seed(100 + n)
    perm = torch.from_numpy(PERM).cuda()
    amax = torch.tensor([3.7e-5], device='cuda')
    s = E.dz_scale(3.7e-5)
    dz16 = ((torch.randn((n, 256), device='cuda', generator=g) * 1e-5) * s).half()[:, perm].contiguous()
    dh16 = ((torch.randn((n, 128), device='cuda', generator=g) * 2e-5) * s).half()[:, perm[:128]].contiguous()
    act16 = (torch.relu(torch.randn((n, 256), device='cuda', generator=g)) * 32).half()[:, perm].contiguous()
    x0 = torch.randn((n, 64), device='cuda', generator=g)
    x0[:, 63] = 0
    x016 = (x0 * 32).half().contiguous()
    x0[:, 27:] = 0
    x0[:, 63] = 1
    x1_16 = (x0 * 32).half().contiguous()
    P256, P128, A, X63, X64 = h64(dz16, s), h64(dh16, s), h64(act16, 32), h64(x016, 32), h64(x1_16, 32)
    p128 = PERM[:128]
    # (256, 256) into a [256][319] gradient at column 63 (the skip layer's hidden columns)
    out = torch.full((256, 319), SENT, device='cuda')
    wgrad16(G, 256, 256, dz16, act16, out, 63, amax, n)
    ref = np.empty((256, 256))
    ref[PERM[:, None], PERM[None, :]] = P256.T @ A
    assert rel_err(out[:, 63:], ref) < 2e-6 and bool((out[:, :63] == SENT).all())
    # (256, 63): natural-order columns out of rows of 64
    out = torch.full((256, 70), SENT, device='cuda')
    wgrad16(G, 256, 63, dz16, x016, out, 0, amax, n)
    ref = np.empty((256, 64))
    ref[PERM] = P256.T @ X63
    assert rel_err(out[:, :63], ref[:, :63]) < 2e-6 and bool((out[:, 63:] == SENT).all())
    # (128, 256) and (128, 64)
    out = torch.full((128, 283), SENT, device='cuda')
    wgrad16(G, 128, 256, dh16, act16, out, 0, amax, n)
    ref = np.empty((128, 256))
    ref[p128[:, None], PERM[None, :]] = P128.T @ A
    assert rel_err(out[:, :256], ref) < 2e-6 and bool((out[:, 256:] == SENT).all())
    out = torch.full((128, 67), SENT, device='cuda')
    wgrad16(G, 128, 64, dh16, x1_16, out, 0, amax, n)
    ref = np.empty((128, 64))
    ref[p128] = P128.T @ X64
    assert rel_err(out[:, :64], ref) < 2e-6 and bool((out[:, 64:] == SENT).all())
    # alpha_linear's row, the 4-row heads, the plain head
    heads_and_out16(G, n, g, act16, A)


def heads_and_out16(G, n, g, act16, A):
    d_raw = torch.randn((n, 4), device='cuda', generator=g).contiguous()
    D = d_raw.cpu().numpy().astype(np.float64)
    colsum_tol = 2e-6 * float(np.abs(D).sum(0).max())
    out = torch.full((260,), SENT, device='cuda')
    ws = torch.empty(int(G.lib.nm_wgrad_alpha16_workspace_floats(n)), device='cuda')
    G.L.check(G.lib.nm_wgrad_alpha16(ptr(d_raw), ptr(act16), n, ptr(out), ptr(ws), ws.numel(), G.L.stream_ptr()), "nm_wgrad_alpha16")
    ref_a = np.empty(256)
    ref_a[PERM] = D[:, 3] @ A
    assert rel_err(out[:256], ref_a) < 2e-6 and bool((out[256:] == SENT).all())
    hv = torch.relu(torch.randn((n, 128), device='cuda', generator=g)).contiguous()
    heads, am = torch.full((648,), SENT, device='cuda'), torch.zeros(1, device='cuda')
    ws = torch.empty(int(G.lib.nm_wgrad_heads16_workspace_floats(n)), device='cuda')
    call_heads = lambda d, a: G.L.check(G.lib.nm_wgrad_heads16(ptr(d), ptr(act16), ptr(hv), n, ptr(heads), ptr(a), ptr(ws), ws.numel(), G.L.stream_ptr()), "nm_wgrad_heads16")
    call_heads(d_raw, am)
    ref_rgb = D[:, :3].T @ hv.cpu().numpy().astype(np.float64)
    assert rel_err(heads[:256], ref_a) < 2e-6
    assert rel_err(heads[256:640].view(3, 128), ref_rgb) < 2e-6
    assert float(np.abs(heads[640:644].cpu().numpy() - D.sum(0)).max()) <= colsum_tol and bool((heads[644:] == SENT).all())
    assert float(am) == float(d_raw.abs().max())
    # the plain head: out[k][f] = sum_n d_out[n][k] H7[n][f], the four column sums, max |d_out|
    o16, am2 = torch.full((1032,), SENT, device='cuda'), torch.zeros(1, device='cuda')
    ws2 = torch.empty(int(G.lib.nm_wgrad_out16_workspace_floats(n)), device='cuda')
    call_out = lambda d, a: G.L.check(G.lib.nm_wgrad_out16(ptr(d), ptr(act16), n, ptr(o16), ptr(a), ptr(ws2), ws2.numel(), G.L.stream_ptr()), "nm_wgrad_out16")
    call_out(d_raw, am2)
    ref_o = np.empty((4, 256))
    ref_o[:, PERM] = D.T @ A
    assert rel_err(o16[:1024].view(4, 256), ref_o) < 2e-6
    assert float(np.abs(o16[1024:1028].cpu().numpy() - D.sum(0)).max()) <= colsum_tol and bool((o16[1028:] == SENT).all())
    assert float(am2) == float(d_raw.abs().max())
    # amax only grows, and stays an exact zero on an all-zero gradient
    half, zero = (d_raw * 0.5).contiguous(), torch.zeros_like(d_raw)
    for call, a in ((call_heads, am), (call_out, am2)):
        call(half, a)
        assert float(a) == float(d_raw.abs().max())
        z = torch.zeros(1, device='cuda')
        call(zero, z)
        assert z.view(torch.int32).item() == 0
    return z


def test_wgrad_out16_past_several_bands(G):
    """n = 4100: nine bands of 512, the last with four rows"""
    n = 4100
    g = torch.Generator(device='cuda').manual_seed(4100)
    act16 = (torch.relu(torch.randn((n, 256), device='cuda', generator=g)) * 32).half()[:, torch.from_numpy(PERM).cuda()].contiguous()
    heads_and_out16(G, n, g, act16, h64(act16, 32))


def test_wgrad16_with_a_zero_amax_writes_zeros(G):
    """an all-zero d_raw leaves amax at zero (above); nm_dz_scale(0) = 1, so nm_wgrad16 on the all-zero dz16 of such a step writes exact zeros, not NaN"""
    n = 9
    g = torch.Generator(device='cuda').manual_seed(1)
    act16 = (torch.relu(torch.randn((n, 256), device='cuda', generator=g)) * 32).half().contiguous()
    amax = heads_and_out16(G, n, g, act16, h64(act16, 32))
    assert amax.view(torch.int32).item() == 0
    out = torch.full((256, 256), SENT, device='cuda')
    wgrad16(G, 256, 256, torch.zeros((n, 256), device='cuda', dtype=torch.float16), act16, out, 0, amax, n)
    assert bool((out == 0).all())


def test_absmax_small_counts(G):
    """count & 3 in {1, 2, 3} with and without a full float4 in front; count 0 leaves the scalar alone"""
    g = torch.Generator(device='cuda').manual_seed(2)
    for n in (0, 1, 2, 3, 5, 7):
        x = torch.randn(8, device='cuda', generator=g)
        x[n:] = 100.0                                                     # what lies beyond `count` must not be read into the maximum
        out = torch.zeros(1, device='cuda')
        G.L.check(G.lib.nm_absmax(ptr(x), n, ptr(out), G.L.stream_ptr()), "nm_absmax")
        assert float(out) == (float(x[:n].abs().max()) if n else 0.0), n
        if n:
            x[n - 1] = -50.0                                              # the last counted element is counted
            G.L.check(G.lib.nm_absmax(ptr(x), n, ptr(out), G.L.stream_ptr()), "nm_absmax")
            assert float(out) == 50.0, n
