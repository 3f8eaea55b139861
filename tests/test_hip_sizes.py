"""-m gpu: the per-ray and per-element kernels past the sizes at which they change behaviour (grid-stride sweeps, multi-chunk scans,
fewer waves per block, more lists than one merge kernel takes), each against a plain restatement of its operation.

Every launch size below is derived from TABLE, the constants the kernels' behaviour changes at; tests/test_kernel_size_table.py
checks on the CPU that each of them still reads so in its source line, so a change to one shows up as a stale table.

The sweep tests call the C entry points directly with every array placed inside a larger allocation whose guard rows before and after
hold a NaN-pattern sentinel: a stray access lands in memory the test owns, where it is visible and cannot fault.  Each launch is run
(1) whole, (2) whole again with finite junk in the input guards, (3) on consecutive row slices that each fit in one sweep; the output
guards must be untouched and (1), (2), (3) bit-identical.  A row subset drawn from every sweep, the last row included, is then held to a
restatement of the operation (float64, the oracle, or exact where the operation is a permutation or an index list)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import compositing, ray_ops as O
from test_hip_ray_ops import tie_aware

pytestmark = pytest.mark.gpu

# ---- the thresholds: name -> (value, source file, pattern whose integer groups multiply to the value) ----------------------------
TABLE = {
    # grid_for() caps every ray_ops grid at 256 * 16 blocks (ml-neuman_amd/csrc/ray_ops.hip, grid_for)
    'GRID_MAX_BLOCKS': (4096, 'ml-neuman_amd/csrc/ray_ops.hip', r'inline int grid_for\(int64_t work_items, int per_block, int max_blocks = (\d+) \* (\d+)\)'),
    # composite / sample_pdf<0,1,2> / merge_sorted: one wave per ray, 4 waves per block (ray_ops.hip, kRayWavesPerBlock)
    'RAY_WAVES_PER_BLOCK': (4, 'ml-neuman_amd/csrc/ray_ops.hip', r'constexpr int kRayWavesPerBlock = (\d+);'),
    # ray_to_samples / z_to_points / rows_kernel / merged_intervals: 256 elements per block (ray_ops.hip, nm_ray_to_samples' launch)
    'ELEMS_PER_BLOCK': (256, 'ml-neuman_amd/csrc/ray_ops.hip', r'ray_to_samples_kernel, dim3\(grid_for\(R \* S, (\d+)\)\)'),
    # merge_composite_kernel: 12 B of LDS per merged sample and wave, 64 KiB per block (ray_ops.hip, nm_merge_composite_lists)
    'MERGE_BYTES_PER_SAMPLE': (12, 'ml-neuman_amd/csrc/ray_ops.hip', r'per_wave = \(size_t\)L\.S_total \* (\d+);'),
    'MERGE_LDS_BYTES': (65536, 'ml-neuman_amd/csrc/ray_ops.hip', r'int wpb = \(int\)\(\((\d+) \* (\d+)\) / per_wave\);'),
    'MERGE_MAX_WAVES': (4, 'ml-neuman_amd/csrc/ray_ops.hip', r'if \(wpb > (\d+)\) wpb = \d+;'),
    # more lists than this: render_multi_rays merges list by list (ray_ops.hip, kMaxMergeLists; render_utils.py, `len(lists) <= 3`)
    'MAX_MERGE_LISTS': (4, 'ml-neuman_amd/csrc/ray_ops.hip', r'constexpr int kMaxMergeLists = (\d+);'),
    'MAX_INTERVAL_LISTS': (32, 'ml-neuman_amd/csrc/ray_ops.hip', r'constexpr int kMaxIntervalLists = (\d+);'),
    # transmittance_chunk: at most 8192 blocks of 4 waves (ml-neuman_amd/csrc/march.hip, nm_transmittance_chunk)
    'MARCH_MAX_BLOCKS': (8192, 'ml-neuman_amd/csrc/march.hip', r'if \(blocks > (\d+)\) blocks = \d+;'),
    'MARCH_WAVES_PER_BLOCK': (4, 'ml-neuman_amd/csrc/march.hip', r'int64_t blocks = \(n_rays \+ 3\) / (\d+);'),
    # nm_compact_hits: blocks of 256 rays, their counts scanned by ONE 1024-thread block (ml-neuman_amd/csrc/nearfar.hip)
    'COMPACT_BLOCK': (256, 'ml-neuman_amd/csrc/nearfar.hip', r'constexpr int kCompactBlock = (\d+);'),
    'SCAN_THREADS': (1024, 'ml-neuman_amd/csrc/nearfar.hip', r'scan_blocks_kernel, dim3\(1\), dim3\((\d+)\)'),
    # nm_occ_compact_points / _samples: blocks of 1024 points, the same one-block scan (ml-neuman_amd/csrc/occupancy.hip)
    'OCC_BLOCK': (1024, 'ml-neuman_amd/csrc/occupancy.hip', r'constexpr int kOccBlock = (\d+);'),
    'OCC_SCAN_THREADS': (1024, 'ml-neuman_amd/csrc/occupancy.hip', r'occ_scan_kernel, dim3\(1\), dim3\((\d+)\)'),
}
C = types.SimpleNamespace(**{k: v[0] for k, v in TABLE.items()})
RAY_SWEEP = C.GRID_MAX_BLOCKS * C.RAY_WAVES_PER_BLOCK             # 16 384 rays per grid-stride step of the per-ray kernels
ELEM_SWEEP = C.GRID_MAX_BLOCKS * C.ELEMS_PER_BLOCK                # 1 048 576 elements per step of the per-element kernels
MARCH_SWEEP = C.MARCH_MAX_BLOCKS * C.MARCH_WAVES_PER_BLOCK        # 32 768 rays per step of transmittance_chunk
COMPACT_CHUNK = C.COMPACT_BLOCK * C.SCAN_THREADS                  # 262 144 rays per pass of scan_blocks_kernel's carry loop
OCC_CHUNK = C.OCC_BLOCK * C.OCC_SCAN_THREADS                      # 1 048 576 points per pass of occ_scan_kernel's carry loop

R_RAY = 3 * RAY_SWEEP + 37                                        # three full sweeps, a fourth with a partial last block (idle waves)
S_SMALL = 16


def elem_rows(S):
    """rays of S samples for two full per-element sweeps and a partial third"""
    return 2 * ELEM_SWEEP // S + 17


def merge_wpb(S_total):
    return min(C.MERGE_MAX_WAVES, C.MERGE_LDS_BYTES // (C.MERGE_BYTES_PER_SAMPLE * S_total))


# ---- guarded buffers -----------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC5A5A5            # a quiet NaN with a payload (as int32: an index far out of range); no kernel produces it
GUARD = 67                       # guard rows before and after every array


def guarded(like, dtype=None, init=None):
    """-> (buf, view): `view` of shape `like` (a shape, or a tensor whose values are copied in) inside `buf`, GUARD sentinel rows each side"""
    shape = tuple(like.shape) if isinstance(like, torch.Tensor) else tuple(like)
    dtype = dtype or (like.dtype if isinstance(like, torch.Tensor) else torch.float32)
    buf = torch.empty((shape[0] + 2 * GUARD,) + shape[1:], device='cuda', dtype=dtype)
    buf.view(torch.int32).fill_(SENTINEL)
    view = buf[GUARD:GUARD + shape[0]]
    src = like if isinstance(like, torch.Tensor) else init
    if src is not None:
        view.copy_(src)
    return buf, view


def guards_intact(buf):
    b = buf.view(torch.int32).reshape(buf.shape[0], -1)
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())


def fill_guards(buf, value):
    buf[:GUARD] = value
    buf[-GUARD:] = value


def same(a, b):
    """bit for bit (NaN payloads included)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def lib():
    from neuman_hip import _lib
    return _lib.lib()


def check(rc, what):
    from neuman_hip import _lib
    _lib.check(rc, what)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sweep_checked(launch, ins, outs, R, step, int_guards=None):
    """ins {name: tensor} -> guarded copies; outs {name: shape | tensor (initial contents)} -> guarded, sentinel elsewhere.
    launch(I, O, i, j) runs the entry point on rows i..j-1 (it slices what is per row itself).  Runs (1) whole, (2) whole with finite junk
    in the input guards (int inputs: int_guards[1], a valid index, where (1) had int_guards[0]), (3) on slices of `step` rows; asserts that
    the output guards are intact and the three bit-identical -> (I, outputs of (1))"""
    bufs = {k: guarded(v) for k, v in ins.items()}
    for k, (b, v) in bufs.items():
        if v.dtype == torch.int32:
            fill_guards(b, int_guards[0])
    I = {k: v for k, (b, v) in bufs.items()}
    results = []
    for run in range(3):
        if run == 1:
            for b, v in bufs.values():
                fill_guards(b, int_guards[1] if v.dtype == torch.int32 else 7.25)
        ob = {k: guarded(v) for k, v in outs.items()}
        O_ = {k: v for k, (b, v) in ob.items()}
        if run < 2:
            launch(I, O_, 0, R)
        else:
            for i in range(0, R, step):
                launch(I, O_, i, min(R, i + step))
        torch.cuda.synchronize()
        for k, (b, _) in ob.items():
            assert guards_intact(b), f"run {run}: a write landed in the guard rows of {k}"
        results.append(O_)
    for run, tag in ((1, "junk in the input guards"), (2, f"slices of {step} rows")):
        for k in outs:
            assert same(results[0][k], results[run][k]), f"{k}: the whole launch differs from the one with {tag}"
    return I, results[0]


def subset_rows(R, step, per=60, seed=0):
    """a few rows from every sweep of `step` rows, the first and last row of each and the very last row included"""
    rng = np.random.default_rng(seed)
    rows = [np.array([0, R - 1])]
    for i in range(0, R, step):
        j = min(R, i + step)
        rows.append(np.array([i, j - 1]))
        rows.append(rng.integers(i, j, size=min(per, j - i)))
    return np.unique(np.concatenate(rows))


def gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def sorted_z(R, S, g, lo=0.0, hi=3.14):
    return torch.sort(lo + (hi - lo) * torch.rand((R, S), device='cuda', generator=g), dim=1).values.contiguous()


def raw_of(R, S, g):
    return (torch.randn((R, S, 4), device='cuda', generator=g) * torch.tensor([1., 1., 1., 5.], device='cuda')).contiguous()


def dirs_of(R, g):
    return torch.randn((R, 3), device='cuda', generator=g).contiguous()


def npy(t, rows=None):
    t = t if rows is None else t[torch.as_tensor(rows, device=t.device)]
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from neuman_hip import _lib, occupancy, ray_utils, render_utils
    _lib.require_gpu()
    return types.SimpleNamespace(ray=ray_utils, render=render_utils, occ=occupancy)


# ---- 1 + 2: per-ray kernels, sweeps of RAY_SWEEP rays ---------------------------------------------------------------------------
def raw2outputs_f64(raw, z, d, white=True):
    raw, z, d = (np.asarray(x, np.float64) for x in (raw, z, d))
    R = z.shape[0]
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((R, 1), 1e10)], 1) * np.linalg.norm(d, axis=1)[:, None]
    alpha = 1.0 - np.exp(-np.maximum(raw[..., 3], 0.0) * dist)
    T = np.cumprod(np.concatenate([np.ones((R, 1)), 1.0 - alpha + 1e-10], 1), 1)[:, :-1]
    w = alpha * T
    rgb = (w[..., None] / (1.0 + np.exp(-raw[..., :3]))).sum(1)
    depth, acc = (w * z).sum(1), w.sum(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        disp = 1.0 / np.maximum(1e-10, depth / acc)
    if white:
        rgb = rgb + (1.0 - acc[:, None])
    return rgb, disp, acc, w, depth


def composite_launch(S, white=1):
    def launch(I, O_, i, j):
        check(lib().nm_composite(P(I['raw'][i:j]), P(I['z'][i:j]), P(I['d'][i:j]), j - i, S, white, None, P(O_['rgb'][i:j]), P(O_['disp'][i:j]),
                                 P(O_['acc'][i:j]), P(O_['w'][i:j]), P(O_['depth'][i:j]), stream()), "nm_composite")
    return launch


def test_composite_past_one_sweep(H):
    """composite_kernel past grid_for's cap: R = 3 RAY_SWEEP + 37 rays, each wave on a ray of every sweep, the last sweep's block partly idle"""
    R, S = R_RAY, S_SMALL
    g = gen(1)
    ins = dict(raw=raw_of(R, S, g), z=sorted_z(R, S, g), d=dirs_of(R, g))
    outs = dict(rgb=(R, 3), disp=(R,), acc=(R,), w=(R, S), depth=(R,))
    I, out = sweep_checked(composite_launch(S), ins, outs, R, RAY_SWEEP)
    rows = subset_rows(R, RAY_SWEEP)
    rgb, disp, acc, w, depth = raw2outputs_f64(npy(I['raw'], rows), npy(I['z'], rows), npy(I['d'], rows))
    np.testing.assert_allclose(npy(out['w'], rows), w, atol=5e-7)                  # the tolerances of test_composite_vs_oracle
    np.testing.assert_allclose(npy(out['rgb'], rows), rgb, atol=3e-6)
    np.testing.assert_allclose(npy(out['acc'], rows), acc, atol=3e-6)
    np.testing.assert_allclose(npy(out['depth'], rows), depth, atol=1e-5)
    np.testing.assert_allclose(npy(out['disp'], rows), disp, rtol=2e-5)


def test_sample_pdf_past_one_sweep(H):
    """sample_pdf_kernel<0> past grid_for's cap: its LDS (bins, cdf) reused sweep after sweep, waves past the end idling on R - 1"""
    R, B, N = R_RAY, S_SMALL, 24
    g = gen(2)
    u = torch.linspace(0., 1., steps=N, device='cuda')
    ins = dict(bins=sorted_z(R, B, g), w=(torch.rand((R, B - 1), device='cuda', generator=g) ** 4).contiguous())

    def launch(I, O_, i, j):
        check(lib().nm_sample_pdf(P(I['bins'][i:j]), P(I['w'][i:j]), j - i, B, P(u), N, P(O_['s'][i:j]), stream()), "nm_sample_pdf")
    I, out = sweep_checked(launch, ins, dict(s=(R, N)), R, RAY_SWEEP)
    rows = subset_rows(R, RAY_SWEEP)
    bins = npy(I['bins'], rows)
    tie_aware(npy(out['s'], rows), O.sample_pdf(bins, npy(I['w'], rows), N), 2e-6, 0.01, np.diff(bins, axis=1).max())


@pytest.mark.parametrize("including_old", [True, False])
def test_importance_z_past_one_sweep(H, including_old):
    """sample_pdf_kernel<1> past grid_for's cap, with and without the sorted merge (its LDS: bins, cdf, samples and the ray's z)"""
    R, S, N = R_RAY, S_SMALL, 24
    g = gen(3)
    u = torch.linspace(0., 1., steps=N, device='cuda')
    w = torch.rand((R, S), device='cuda', generator=g) ** 6
    w[::5] = 0.0                                                                   # flat pdfs on every fifth ray
    ins = dict(z=sorted_z(R, S, g, 0.5, 4.0), w=w.contiguous())
    n_out = S + N if including_old else N

    def launch(I, O_, i, j):
        check(lib().nm_importance_z(P(I['z'][i:j]), P(I['w'][i:j]), j - i, S, P(u), N, int(including_old), P(O_['z'][i:j]), stream()), "nm_importance_z")
    I, out = sweep_checked(launch, ins, dict(z=(R, n_out)), R, RAY_SWEEP)
    rows = subset_rows(R, RAY_SWEEP)
    z = npy(I['z'], rows)
    zero = np.zeros((len(rows), 3), np.float32)
    oz = O.ray_to_importance_samples(zero, zero, z, npy(I['w'], rows), N, including_old=including_old)[2]
    hz = npy(out['z'], rows)
    if including_old:
        assert (np.diff(hz, axis=1) >= 0).all() and all(np.isin(z[k], hz[k]).all() for k in range(len(rows)))
    tie_aware(hz, oz, 3e-6, 0.01, np.diff(z, axis=1).max())


def test_importance_from_raw_past_one_sweep(H):
    """sample_pdf_kernel<2> past grid_for's cap (compositing weights in LDS as well); at this size it must equal nm_importance_z fed with
    nm_composite's weights bit for bit -- z and the weights it writes -- as its comment says"""
    R, S, N = R_RAY, S_SMALL, 24
    g = gen(4)
    u = torch.linspace(0., 1., steps=N, device='cuda')
    ins = dict(raw=raw_of(R, S, g), z=sorted_z(R, S, g, 0.5, 4.0), d=dirs_of(R, g))

    def launch(I, O_, i, j):
        check(lib().nm_importance_from_raw(P(I['raw'][i:j]), P(I['z'][i:j]), P(I['d'][i:j]), j - i, S, P(u), N, P(O_['z'][i:j]), P(O_['w'][i:j]), stream()),
              "nm_importance_from_raw")
    I, out = sweep_checked(launch, ins, dict(z=(R, S + N), w=(R, S)), R, RAY_SWEEP)
    w = H.render.raw2outputs(I['raw'], I['z'], I['d'])[3]
    assert same(out['w'], w)
    assert same(out['z'], H.ray.importance_z(I['z'], w, N, including_old=True))
    rows = subset_rows(R, RAY_SWEEP)
    z = npy(I['z'], rows)
    ow = compositing.raw2outputs(npy(I['raw'], rows), z, npy(I['d'], rows))[3]
    zero = np.zeros((len(rows), 3), np.float32)
    tie_aware(npy(out['z'], rows), O.ray_to_importance_samples(zero, zero, z, ow, N)[2], 3e-6, 0.01, np.diff(z, axis=1).max())


def test_merge_sorted_past_one_sweep(H):
    """merge_sorted_kernel past grid_for's cap (both lists staged in LDS per sweep), with exact cross-list ties on every ray"""
    R, Sa, Sb = R_RAY, 16, 9
    g = gen(5)
    za, zb = sorted_z(R, Sa, g), sorted_z(R, Sb, g, 1.0, 2.0)
    zb[:, 0] = za[:, 2]
    zb[::3, -1] = za[::3, -1]
    ins = dict(za=za, ra=raw_of(R, Sa, g), zb=torch.sort(zb, 1).values.contiguous(), rb=raw_of(R, Sb, g))

    def launch(I, O_, i, j):
        check(lib().nm_merge_sorted(P(I['za'][i:j]), P(I['ra'][i:j]), Sa, P(I['zb'][i:j]), P(I['rb'][i:j]), Sb, j - i, P(O_['z'][i:j]), P(O_['raw'][i:j]),
                                    stream()), "nm_merge_sorted")
    I, out = sweep_checked(launch, ins, dict(z=(R, Sa + Sb), raw=(R, Sa + Sb, 4)), R, RAY_SWEEP)
    rows = subset_rows(R, RAY_SWEEP)
    oz, oraw = compositing.merge_sorted([npy(I['za'], rows), npy(I['zb'], rows)], [npy(I['ra'], rows), npy(I['rb'], rows)])
    np.testing.assert_array_equal(npy(out['z'], rows), oz)
    np.testing.assert_array_equal(npy(out['raw'], rows), oraw)


# ---- 1 + 2: per-element kernels, sweeps of ELEM_SWEEP elements --------------------------------------------------------------------
@pytest.mark.parametrize("lindisp,perturb", [(0, True), (1, False)])
def test_ray_to_samples_past_one_sweep(H, lindisp, perturb):
    """ray_to_samples_kernel past grid_for's cap: 2 ELEM_SWEEP + 136 samples; exact against the oracle (same two-rounding lerp)"""
    S = 8
    R = elem_rows(S)
    g = gen(6 + lindisp)
    near = (0.1 + 0.9 * torch.rand(R, device='cuda', generator=g)).contiguous()
    ins = dict(o=torch.randn((R, 3), device='cuda', generator=g), d=dirs_of(R, g), near=near,
               far=(near + 0.5 + 2.5 * torch.rand(R, device='cuda', generator=g)).contiguous())
    if perturb:
        ins['t'] = torch.clip(torch.rand((R, S), device='cuda', generator=g), 0.01, 0.99).contiguous()
    t_vals = torch.linspace(0., 1., steps=S, device='cuda')

    def launch(I, O_, i, j):
        check(lib().nm_ray_to_samples(P(I['o'][i:j]), P(I['d'][i:j]), P(I['near'][i:j]), P(I['far'][i:j]), j - i, S, P(t_vals), lindisp,
                                      P(I['t'][i:j]) if perturb else None, P(O_['pts'][i:j]), P(O_['dirs'][i:j]), P(O_['z'][i:j]), stream()),
              "nm_ray_to_samples")
    I, out = sweep_checked(launch, ins, dict(pts=(R, S, 3), dirs=(R, S, 3), z=(R, S)), R, ELEM_SWEEP // S)
    rows = subset_rows(R, ELEM_SWEEP // S)
    op, od, oz = O.ray_to_samples(npy(I['o'], rows), npy(I['d'], rows), npy(I['near'], rows)[:, None], npy(I['far'], rows)[:, None], S,
                                  lindisp=bool(lindisp), t_rand=npy(I['t'], rows) if perturb else None, t_vals=t_vals.cpu().numpy())
    np.testing.assert_array_equal(npy(out['z'], rows), oz)
    np.testing.assert_array_equal(npy(out['pts'], rows), op)
    np.testing.assert_array_equal(npy(out['dirs'], rows), od)


def test_z_to_points_past_one_sweep(H):
    """z_to_points_kernel past grid_for's cap; exact (o + d z, two roundings)"""
    S = 8
    R = elem_rows(S)
    g = gen(8)
    ins = dict(o=torch.randn((R, 3), device='cuda', generator=g), d=dirs_of(R, g), z=sorted_z(R, S, g))

    def launch(I, O_, i, j):
        check(lib().nm_z_to_points(P(I['o'][i:j]), P(I['d'][i:j]), P(I['z'][i:j]), j - i, S, P(O_['pts'][i:j]), P(O_['dirs'][i:j]), stream()), "nm_z_to_points")
    I, out = sweep_checked(launch, ins, dict(pts=(R, S, 3), dirs=(R, S, 3)), R, ELEM_SWEEP // S)
    rows = subset_rows(R, ELEM_SWEEP // S)
    o, d, z = npy(I['o'], rows), npy(I['d'], rows), npy(I['z'], rows)
    np.testing.assert_array_equal(npy(out['pts'], rows), (o[:, None, :] + d[:, None, :] * z[..., None]).astype(np.float32))
    np.testing.assert_array_equal(npy(out['dirs'], rows), np.broadcast_to(d[:, None, :], (len(rows), S, 3)))


def test_gather_rows_past_one_sweep(H):
    """rows_kernel<gather> past grid_for's cap: 2 ELEM_SWEEP + 136 elements; then with a device count n_dev below n_max (the rows past it
    are not written).  Exact against torch indexing."""
    W = 8
    n = elem_rows(W)
    n_src = n + 999
    g = gen(9)
    src_buf, src = guarded(torch.randn((n_src, W), device='cuda', generator=g))
    ins = dict(idx=torch.randint(0, n_src, (n,), device='cuda', generator=g, dtype=torch.int32))

    def launch(I, O_, i, j):
        check(lib().nm_gather_rows(P(src), P(I['idx'][i:j]), None, j - i, W, P(O_['dst'][i:j]), stream()), "nm_gather_rows")
    I, out = sweep_checked(launch, ins, dict(dst=(n, W)), n, ELEM_SWEEP // W, int_guards=(0, n_src - 1))
    assert same(out['dst'], src[I['idx'].long()])
    fill_guards(src_buf, 7.25)                                                      # the source's own guards are never read
    n_dev = torch.tensor([n - 5], device='cuda', dtype=torch.int32)
    buf, dst = guarded((n, W))
    check(lib().nm_gather_rows(P(src), P(I['idx']), P(n_dev), n, W, P(dst), stream()), "nm_gather_rows")
    torch.cuda.synchronize()
    assert guards_intact(buf) and same(dst[:n - 5], out['dst'][:n - 5])
    assert bool((dst[n - 5:].view(torch.int32) == SENTINEL).all())


def test_scatter_rows_past_one_sweep(H):
    """rows_kernel<scatter> past grid_for's cap into a larger destination: exactly the listed rows are written"""
    W = 8
    n = elem_rows(W)
    n_dst = n + 999
    g = gen(10)
    perm = torch.randperm(n_dst, device='cuda', generator=g)[:n].to(torch.int32)
    ins = dict(src=torch.randn((n, W), device='cuda', generator=g), idx=perm.contiguous())
    dst_init = torch.full((n_dst, W), 0.0, device='cuda').view(torch.int32).fill_(SENTINEL).view(torch.float32)

    def launch(I, O_, i, j):
        check(lib().nm_scatter_rows(P(I['src'][i:j]), P(I['idx'][i:j]), None, j - i, W, P(O_['dst']), stream()), "nm_scatter_rows")
    I, out = sweep_checked(launch, ins, dict(dst=dst_init), n, ELEM_SWEEP // W, int_guards=(0, n_dst - 1))
    want = dst_init.clone()
    want[I['idx'].long()] = I['src']
    assert same(out['dst'], want)


def stable_intervals(lists):
    """the definition: stable argsort of cat(lists), differences of the sorted values, 1e10 at the end, scattered back"""
    z = np.concatenate(lists, 1)
    order = np.argsort(z, 1, kind='stable')
    zs = np.take_along_axis(z, order, 1)
    dz_s = np.concatenate([zs[:, 1:] - zs[:, :-1], np.full((z.shape[0], 1), 1e10, np.float32)], 1).astype(np.float32)
    want = np.empty_like(z)
    np.put_along_axis(want, order, dz_s, 1)
    return want


def test_merged_intervals_past_one_sweep(H):
    """merged_intervals_kernel past grid_for's cap: three lists (S_total = 16) on 2 ELEM_SWEEP / 16 + 17 rays, cross-list ties on every ray;
    exact against the stable-sort definition"""
    sizes = (7, 5, 4)
    St = sum(sizes)
    R = elem_rows(St)
    g = gen(11)
    z = [sorted_z(R, s, g, 0.5, 4.0) for s in sizes]
    z[1][:, 0] = z[0][:, 2]
    z[2][::3, -1] = z[0][::3, -1]
    ins = {f'z{l}': torch.sort(x, 1).values.contiguous() for l, x in enumerate(z)}
    k = len(sizes)

    def launch(I, O_, i, j):
        arr = ctypes.c_void_p * k
        check(lib().nm_merged_intervals(k, arr(*[I[f'z{l}'][i:j].data_ptr() for l in range(k)]), (ctypes.c_int * k)(*sizes), j - i,
                                        arr(*[O_[f'dz{l}'][i:j].data_ptr() for l in range(k)]), stream()), "nm_merged_intervals")
    I, out = sweep_checked(launch, ins, {f'dz{l}': (R, s) for l, s in enumerate(sizes)}, R, ELEM_SWEEP // St)
    rows = subset_rows(R, ELEM_SWEEP // St)
    want = stable_intervals([npy(I[f'z{l}'], rows) for l in range(k)])
    np.testing.assert_array_equal(np.concatenate([npy(out[f'dz{l}'], rows) for l in range(k)], 1), want)


# ---- transmittance_chunk: sweeps of MARCH_SWEEP rays --------------------------------------------------------------------------
@pytest.mark.parametrize("given_dz", [False, True])
@pytest.mark.parametrize("indexed", [False, True])
def test_transmittance_chunk_past_one_sweep(H, given_dz, indexed):
    """transmittance_chunk_kernel past its 8192-block cap: 3 MARCH_SWEEP + 5 rays; `indexed`: through a permuted ray list whose length is
    read on the device (n_rays_dev = n_rays - 3).  T of the listed rays against a float64 product; every other T untouched."""
    n, S_total, s0, S = 3 * MARCH_SWEEP + 5, 16, 3, 9
    g = gen(12 + 2 * given_dz + indexed)
    z = sorted_z(n, S_total, g)
    zin = (torch.rand((n, S_total), device='cuda', generator=g) * 0.3).contiguous() if given_dz else z
    raw, d = raw_of(n, S_total, g), dirs_of(n, g)
    T0 = (0.5 + 0.5 * torch.rand(n, device='cuda', generator=g)).contiguous()
    n_eff = n - 3 if indexed else n
    ins = dict(raw=raw, z=zin, d=d)
    if indexed:
        ins['idx'] = torch.randperm(n, device='cuda', generator=g).to(torch.int32).contiguous()
    fn = lib().nm_transmittance_chunk_dz if given_dz else lib().nm_transmittance_chunk

    def launch(I, O_, i, j):
        if indexed:
            cnt = torch.tensor([max(0, min(j, n_eff) - i)], device='cuda', dtype=torch.int32)
            check(fn(P(I['raw']), P(I['z']), P(I['d']), P(I['idx'][i:j]), P(cnt), j - i, s0, S, S_total, P(O_['T']), stream()), "nm_transmittance_chunk")
            torch.cuda.synchronize()                                                # (cnt lives until the launch is done)
        else:
            check(fn(P(I['raw'][i:j]), P(I['z'][i:j]), P(I['d'][i:j]), None, None, j - i, s0, S, S_total, P(O_['T'][i:j]), stream()), "nm_transmittance_chunk")
    I, out = sweep_checked(launch, ins, dict(T=T0), n, MARCH_SWEEP, int_guards=(0, n - 1))
    listed = I['idx'][:n_eff].long() if indexed else torch.arange(n, device='cuda')
    rest = torch.ones(n, dtype=torch.bool, device='cuda')
    rest[listed] = False
    assert int(rest.sum()) == n - n_eff and same(out['T'][rest], T0[rest])
    rows = subset_rows(n_eff, MARCH_SWEEP)
    r = npy(listed, rows)
    zz, rw, dd = npy(I['z'], r).astype(np.float64), npy(I['raw'], r).astype(np.float64), npy(I['d'], r).astype(np.float64)
    if given_dz:
        dist = zz
    else:
        dist = np.concatenate([zz[:, 1:] - zz[:, :-1], np.full((len(r), 1), 1e10)], 1)
    dist = dist * np.linalg.norm(dd, axis=1)[:, None]
    alpha = 1.0 - np.exp(-np.maximum(rw[..., 3], 0.0) * dist)
    want = npy(T0, r).astype(np.float64) * np.prod((1.0 - alpha + 1e-10)[:, s0:s0 + S], 1)
    np.testing.assert_allclose(npy(out['T'], r), want, rtol=0, atol=2e-6)


# ---- 3: scans past one chunk ---------------------------------------------------------------------------------------------------
def hit_patterns(R):
    i = torch.arange(R, device='cuda')
    g = gen(R)
    one_per_block = torch.zeros(R, dtype=torch.bool, device='cuda')
    blk = torch.arange(0, R, C.COMPACT_BLOCK, device='cuda')
    one_per_block[torch.clamp(blk + (blk // C.COMPACT_BLOCK * 97) % C.COMPACT_BLOCK, max=R - 1)] = True
    last = torch.zeros(R, dtype=torch.bool, device='cuda')
    last[-1] = True
    return {'random': torch.rand(R, device='cuda', generator=g) < 0.37, 'all': torch.ones(R, dtype=torch.bool, device='cuda'),
            'none': torch.zeros(R, dtype=torch.bool, device='cuda'), 'last only': last, 'one per block': one_per_block,
            'alternate blocks': (i // C.COMPACT_BLOCK) % 2 == 0}


@pytest.mark.parametrize("R", [COMPACT_CHUNK, COMPACT_CHUNK + 1, 640000, 4 * COMPACT_CHUNK])
def test_compact_hits_past_one_scan_chunk(H, R):
    """nm_compact_hits past scan_blocks_kernel's first 1024-block chunk (COMPACT_CHUNK rays): the hit and miss lists equal nonzero(),
    ascending, exactly; the counts are (hits, misses); nothing past either list's end and no guard is written"""
    L = lib()
    ws_n = int(L.nm_compact_workspace_ints(R))
    for name, m in hit_patterns(R).items():
        near = torch.where(m, 0.0, 1.0).to(torch.float32)
        res = []
        for junk in (None, (0.0, 1.0)):                                            # the second time, input guards that would count as hits
            nb, nv = guarded(near)
            fb, fv = guarded(torch.full((R,), 0.5, device='cuda'))
            if junk:
                fill_guards(nb, junk[0])
                fill_guards(fb, junk[1])
            hb, hit = guarded((R,), torch.int32)
            mb, miss = guarded((R,), torch.int32)
            cb, counts = guarded((2,), torch.int32)
            wb, ws = guarded((ws_n,), torch.int32)
            check(L.nm_compact_hits(P(nv), P(fv), R, P(hit), P(miss), P(counts), P(ws), stream()), "nm_compact_hits")
            torch.cuda.synchronize()
            assert all(guards_intact(b) for b in (hb, mb, cb, wb)), name
            res.append((hit, miss, counts))
        want_h, want_m = torch.nonzero(m).reshape(-1).to(torch.int32), torch.nonzero(~m).reshape(-1).to(torch.int32)
        nh = want_h.numel()
        for hit, miss, counts in res:
            assert counts.tolist() == [nh, R - nh], (name, counts.tolist())
            assert torch.equal(hit[:nh], want_h) and torch.equal(miss[:R - nh], want_m), name
            assert bool((hit[nh:] == SENTINEL).all()) and bool((miss[R - nh:] == SENTINEL).all()), name


OCC_RES = 16


@pytest.fixture(scope="module")
def grid(H):
    aabb = [-1.0, -0.5, -0.8, 1.2, 0.9, 0.7]
    mask = torch.rand((OCC_RES,) * 3, generator=torch.Generator().manual_seed(5)) < 0.4
    return H.occ.OccupancyGrid.from_mask(aabb, mask, device=torch.device('cuda'))


def occ_restatement(grid, pts):
    """test_hip_occupancy_human.py::test_compact_points_equals_a_torch_restatement: listed = outside the box, or in an occupied cell"""
    lo, hi = grid.aabb[:3].to('cuda'), grid.aabb[3:].to('cuda')
    inv = (torch.tensor(float(OCC_RES)) / (grid.aabb[3:] - grid.aabb[:3])).to('cuda')
    t = (pts - lo) * inv
    inside = ((t >= 0) & (t < OCC_RES)).all(1)
    c = torch.clamp(torch.nan_to_num(t, nan=0.0).long(), 0, OCC_RES - 1)
    occ = grid.to_mask().to('cuda')[c[:, 0], c[:, 1], c[:, 2]]
    assert 0 < int(inside.sum()) < pts.shape[0] and bool(occ[inside].any()) and not bool(occ[inside].all())
    return torch.nonzero(~inside | occ).reshape(-1).to(torch.int32)


def occ_checked(call, n, want):
    """call(idx, counts, ws) into guarded buffers -> idx equals `want` exactly, counts = (kept, skipped), nothing else written"""
    ib, idx = guarded((n,), torch.int32)
    cb, counts = guarded((2,), torch.int32)
    wb, ws = guarded((int(lib().nm_occ_compact_workspace_ints(n)),), torch.int32)
    call(idx, counts, ws)
    torch.cuda.synchronize()
    assert guards_intact(ib) and guards_intact(cb) and guards_intact(wb)
    k = want.numel()
    assert counts.tolist() == [k, n - k]
    assert torch.equal(idx[:k], want) and bool((idx[k:] == SENTINEL).all())


@pytest.mark.parametrize("n", [OCC_CHUNK, OCC_CHUNK + 1, 3 * OCC_CHUNK + 333])
def test_occ_compact_points_past_one_scan_chunk(H, grid, n):
    """nm_occ_compact_points past occ_scan_kernel's first 1024-block chunk (OCC_CHUNK points)"""
    g = gen(20)
    lo, hi = grid.aabb[:3].to('cuda'), grid.aabb[3:].to('cuda')
    pts = lo + (hi - lo) * (torch.rand((n, 3), device='cuda', generator=g) * 1.4 - 0.2)
    pts[::1001] = float('nan')
    pts = pts.contiguous()
    _, pv = guarded(pts)
    occ_checked(lambda idx, counts, ws: check(lib().nm_occ_compact_points(P(grid.bits), OCC_RES, grid.box_c(), P(pv), n, P(idx), P(counts), P(ws), stream()),
                                              "nm_occ_compact_points"), n, occ_restatement(grid, pts))


@pytest.mark.parametrize("R", [OCC_CHUNK // 16, OCC_CHUNK // 16 + 1, 3 * OCC_CHUNK // 16 + 21])
def test_occ_compact_samples_past_one_scan_chunk(H, grid, R):
    """nm_occ_compact_samples past occ_scan_kernel's first chunk: R x 16 samples, their points o + d z formed as the kernel does"""
    S = 16
    g = gen(21)
    lo, hi = grid.aabb[:3].to('cuda'), grid.aabb[3:].to('cuda')
    o = (lo + (hi - lo) * torch.rand((R, 3), device='cuda', generator=g)).contiguous()
    d = dirs_of(R, g)
    d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    z = (torch.rand((R, S), device='cuda', generator=g) * 2.0 - 0.5).contiguous()
    pts = o[:, None, :] + d[:, None, :] * z[..., None]                             # two roundings, as sample_input forms them
    _, ov = guarded(o)
    _, dv = guarded(d)
    _, zv = guarded(z)
    occ_checked(lambda idx, counts, ws: check(lib().nm_occ_compact_samples(P(grid.bits), OCC_RES, grid.box_c(), P(ov), P(dv), P(zv), R, S, P(idx), P(counts),
                                                                           P(ws), stream()), "nm_occ_compact_samples"),
                R * S, occ_restatement(grid, pts.reshape(-1, 3)))


# ---- 4: merge_composite_lists at every waves-per-block value -----------------------------------------------------------------
@pytest.mark.parametrize("sizes,with_rows,wpb", [((320, 192, 192, 192), (1, 2, 3), 4), ((1000, 500), (1,), 3), ((1200, 500, 300), (), 2),
                                                 ((5000,), (0,), 1), ((2461, 1500, 1000, 500), (1, 3), 1)])
def test_merge_composite_lists_at_every_block_shape(H, sizes, with_rows, wpb):
    """merge_composite_kernel runs min(4, 65536 / (12 S_total)) waves per block: here 4, 3, 2 and 1 (the last case at the limit, 5461 merged
    samples), on R = 2 x (GRID_MAX_BLOCKS wpb) + 37 rays (two sweeps of its own grid and a partial third), k = 1..4 lists, exact cross-list
    ties on every ray, lists read through `rows` (compacted lists with one shared placeholder row, as render_multi_rays passes them).
    Bit-identical to nm_composite on the lists merged by a stable numpy argsort."""
    St, k = sum(sizes), len(sizes)
    assert merge_wpb(St) == wpb
    sweep = C.GRID_MAX_BLOCKS * wpb
    R = 2 * sweep + 37
    g = gen(30 + St)
    full = [sorted_z(R, s, g, 0.5, 4.0) for s in sizes]
    if k > 1:
        full[1][:, 0] = full[0][:, 2]                                               # a cross-list tie on every ray
        full[-1][::3, -1] = full[0][::3, -1]                                        # ... and one at the end of the merged list
    full = [torch.sort(x, 1).values for x in full]
    ins, rows_of = {}, {}
    for l, s in enumerate(sizes):
        raw = raw_of(R, s, g)
        if l in with_rows:
            hit = torch.nonzero(torch.rand(R, device='cuda', generator=g) < 0.7).reshape(-1)
            perm = hit[torch.randperm(hit.numel(), device='cuda', generator=g)]
            rows = torch.full((R,), perm.numel(), device='cuda', dtype=torch.int32)
            rows[perm] = torch.arange(perm.numel(), device='cuda', dtype=torch.int32)
            pad_z = torch.linspace(8.0, 12.0, s, device='cuda')[None]
            ins[f'z{l}'] = torch.cat([full[l][perm], pad_z]).contiguous()
            ins[f'raw{l}'] = torch.cat([raw[perm], torch.zeros((1, s, 4), device='cuda')]).contiguous()
            ins[f'rows{l}'] = rows
            rows_of[l] = perm.numel()
        else:
            ins[f'z{l}'], ins[f'raw{l}'] = full[l].contiguous(), raw
    ins['d'] = dirs_of(R, g)
    del full
    arr = ctypes.c_void_p * k

    def launch(I, O_, i, j):
        def rows_view(l):
            return I[f'z{l}'] if l in rows_of else I[f'z{l}'][i:j]

        zp = arr(*[rows_view(l).data_ptr() for l in range(k)])
        rp = arr(*[(I[f'raw{l}'] if l in rows_of else I[f'raw{l}'][i:j]).data_ptr() for l in range(k)])
        xp = arr(*[I[f'rows{l}'][i:j].data_ptr() if l in rows_of else None for l in range(k)])
        check(lib().nm_merge_composite_lists(k, zp, rp, xp, (ctypes.c_int * k)(*sizes), j - i, P(I['d'][i:j]), 1, P(O_['rgb'][i:j]), P(O_['depth'][i:j]),
                                             P(O_['acc'][i:j]), stream()), "nm_merge_composite_lists")
    int_lo = min(rows_of.values()) if rows_of else 0
    I, out = sweep_checked(launch, ins, dict(rgb=(R, 3), depth=(R,), acc=(R,)), R, sweep, int_guards=(0, int_lo))
    rows = subset_rows(R, sweep, per=40)
    rt = torch.as_tensor(rows, device='cuda')
    zl, rl = [], []
    for l in range(k):
        at = I[f'rows{l}'][rt].long() if l in rows_of else rt
        zl.append(I[f'z{l}'][at].cpu().numpy())
        rl.append(I[f'raw{l}'][at].cpu().numpy())
    zm, rawm = compositing.merge_sorted(zl, rl)                                     # stable argsort of cat(lists)
    rgb, _, acc, _, depth = H.render.raw2outputs(torch.as_tensor(rawm).cuda(), torch.as_tensor(zm).cuda(), I['d'][rt].contiguous(), white_bkg=True)
    assert same(out['rgb'][rt], rgb) and same(out['depth'][rt], depth) and same(out['acc'][rt], acc)


# ---- 5: four and five actors -------------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import posed_scene as PS  # noqa: E402
from test_hip_march import body  # noqa: E402,F401  (the opaque body scene's fixture)
from test_hip_render import G, displacement_rank, small_scene  # noqa: E402,F401

# per-actor translations: the first three are the posed golden's multi_shifts; the others overlap them on screen, so that rays hit several bodies
SHIFTS = [(0.0, 0.0, 0.0), (0.35, 0.0, 0.2), (-0.3, 0.05, -0.15), (0.1, -0.05, 0.45), (-0.15, 0.1, 0.3)]


def actors(posed, T, n):
    posed_l, T_l = [], []
    for s in SHIFTS[:n]:
        posed_l.append((posed + np.array(s, np.float32)).astype(np.float32))
        t = T.copy()
        t[:, :3, 3] += np.array(s)
        T_l.append(t)
    return posed_l, T_l


def several_bodies(trace, R, n):
    cnt = torch.zeros(R, dtype=torch.int64)
    for h in trace['hit'][:n]:
        cnt[h.long().cpu()] += 1
    return int((cnt >= 2).sum())


@pytest.mark.parametrize("n_actors", [4, 5])
def test_multi_person_frames_with_more_actors_than_one_merge_takes(G, monkeypatch, n_actors):
    """More than MAX_MERGE_LISTS - 1 actors: render_multi_rays merges list by list.  The statements of test_hybrid_and_multi_person_frames:
    against the oracle's rendering with the rays beyond 1e-4 confined to the most displaced fifth, and within 1e-4 on every pixel of the
    oracle run on the device's samples and warped points; and MULTI_COMPACT must make no difference above three actors."""
    from test_hip_configs import conditional_hybrid
    from oracle import render as OR
    assert n_actors > C.MAX_MERGE_LISTS - 1
    cap, posed, faces, T = small_scene(G)
    posed_l, T_l = actors(posed, T, n_actors)
    coarse, fine, human = G.nets[0], G.nets[1], G.nets[2]
    net = types.SimpleNamespace(coarse_bkg_net=coarse[0], fine_bkg_net=fine[0], coarse_human_net=human[0], parameters=coarse[0].parameters)
    kw = dict(samples_per_ray=16, importance_samples_per_ray=16, geo_threshold=0.2, return_depth=True)
    o_t, d_t = G.render._pixel_rays(cap, torch.device('cuda'))
    o, d = o_t.cpu().numpy(), d_t.cpu().numpy()
    faces3 = np.ascontiguousarray(np.asarray(faces)[:, :3], np.int32)
    meshes = [G.ray.mesh_to_device(p, faces3, t, 'cuda') for p, t in zip(posed_l, T_l)]
    R = o.shape[0]
    pts, dd, z = O.ray_to_samples(o, d, np.full((R, 1), cap.near['bkg'], np.float32), np.full((R, 1), cap.far['bkg'], np.float32), 16)
    from oracle import nerf_mlp
    w = compositing.raw2outputs(nerf_mlp.joiner_forward(*coarse[1], pts, dd), z, d)[3]
    oz = O.ray_to_importance_samples(o, d, z, w, 16)[2]

    frames = {}
    for compact in (True, False):
        monkeypatch.setattr(G.render, 'MULTI_COMPACT', compact)
        rgb, _ = G.render.render_hybrid_nerf_multi_persons(net, cap, [net] * n_actors, posed_l, [faces] * n_actors, T_l, **kw)
        trace = {}
        rgb_t, _ = G.render.render_multi_rays(coarse[0], fine[0], [human[0]] * n_actors, o_t, d_t, cap.near['bkg'], cap.far['bkg'],
                                              [torch.as_tensor(p).cuda() for p in posed_l], meshes, 16, 16, trace=trace)
        assert np.array_equal(rgb_t.cpu().numpy(), rgb.reshape(-1, 3))
        frames[compact] = (rgb_t, trace)
    assert torch.equal(frames[True][0], frames[False][0]), "MULTI_COMPACT changed a frame of more than three actors"
    rgb_t, trace = frames[True]
    multi = several_bodies(trace, R, n_actors)
    assert multi > 0
    # the oracle on the device's bounds (its float64 discriminant, csrc/nearfar.hip), as test_posed_human_frame_with_warp gives them: the float32
    # evaluation's cancellation moves a grazing ray's far bound by 6e-5, and with it the body's samples -- a displacement displacement_rank,
    # which ranks the rays by their BACKGROUND samples, does not see
    nf64 = [tuple(x.astype(np.float32) for x in O.geometry_guided_near_far(o, d, p, 0.2, dtype=np.float64)) for p in posed_l]
    o_rgb, _ = OR.render_hybrid_nerf_multi_persons(coarse[1], fine[1], [human[1]] * n_actors, cap, posed_l, [faces] * n_actors, T_l,
                                                   given={'near_far': nf64}, **kw)
    err = np.abs(rgb_t.cpu().numpy() - o_rgb.reshape(-1, 3)).max(-1)
    displacement_rank(err, trace['bkg_z'][0].cpu().numpy(), oz, f"render: {n_actors} actors vs oracle")
    c_rgb, _ = conditional_hybrid(G, {'fine': fine[1], 'human': human[1]}, o, d, trace, n_actors, 16, far=cap.far['bkg'])
    e = np.abs(rgb_t.cpu().numpy() - c_rgb).max()
    print(f"[sizes] {n_actors} actors ({multi} rays through several bodies), oracle on the device's samples and warped points: Linf {e:.2e}")
    assert e < 1e-4


@pytest.mark.parametrize("n_actors", [4, 5])
def test_multi_person_termination_with_more_actors_than_one_merge_takes(body, monkeypatch, n_actors):
    """TERMINATION_EPS > 0 with more than MAX_MERGE_LISTS - 1 actors: the intervals of 1 + actors lists (nm_merged_intervals, up to
    MAX_INTERVAL_LISTS lists).  Opaque bodies in front of an opaque background: the frame renders, skips evaluations in the human and the
    background passes, and is within (1 + actors) eps of the eps = 0 frame; eps = 0 afterwards is the plain frame again."""
    from neuman_hip import render_utils as R
    c = PS.cap(body, 'multi')
    o, d = (torch.as_tensor(x).cuda().contiguous() for x in PS.frame_rays(c))
    posed_l, T_l = actors(body['posed_verts'], body['T'], n_actors)
    faces3 = np.ascontiguousarray(body['faces'][:, :3], np.int32)
    meshes = [body['ray'].mesh_to_device(v, faces3, t, 'cuda') for v, t in zip(posed_l, T_l)]
    verts = [torch.as_tensor(v).cuda() for v in posed_l]

    def run(trace=None):
        return R.render_multi_rays(body['bkg'], body['bkg'], [body['human']] * n_actors, o, d, c.near['bkg'], c.far['bkg'], verts, meshes, 192, 128,
                                   trace=trace)[0]
    monkeypatch.setattr(R, 'TERMINATION_EPS', 0.0)
    tr0 = {}
    a = run(tr0)
    monkeypatch.setattr(R, 'TERMINATION_EPS', 1e-4)
    tr = {}
    b = run(tr)
    monkeypatch.setattr(R, 'TERMINATION_EPS', 0.0)
    assert torch.equal(run(), a)
    multi = several_bodies(tr0, o.shape[0], n_actors)
    hs = tr['march_human']
    he, ht = sum(s_['human_evaluated'] for s_ in hs), sum(s_['human_total'] for s_ in hs)
    f_ = tr['march'][0]
    e = (a - b).abs().max().item()
    bound = (1 + n_actors) * 1e-4
    print(f"[sizes] {n_actors} actors, eps 1e-4 ({multi} rays through several bodies): body passes {he / ht:.3f} evaluated, background fine "
          f"{f_['evaluated'] / f_['total']:.3f}, colour Linf vs every sample {e:.2e} (bound {bound:g})")
    assert multi > 0 and he < ht and f_['evaluated'] < f_['total'] and e <= bound


def test_merged_intervals_refuses_more_lists_than_it_takes(H):
    """MAX_INTERVAL_LISTS lists are served (one background list and 31 actors); one more is refused, not run"""
    from neuman_hip import _lib
    z = [torch.linspace(0.0, 1.0, 4, device='cuda')[None].repeat(3, 1).contiguous() for _ in range(C.MAX_INTERVAL_LISTS + 1)]
    dz = H.render.merged_intervals(z[:C.MAX_INTERVAL_LISTS])
    assert len(dz) == C.MAX_INTERVAL_LISTS and float(dz[-1][0, -1]) == 1e10 and float(dz[0][0, 0]) == 0.0
    with pytest.raises(_lib.NeumanHipError, match="nm_merged_intervals"):
        H.render.merged_intervals(z)
