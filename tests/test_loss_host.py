"""CPU: what tests/test_hip_loss_edges.py and tests/test_hip_frame_edges.py rest on, checked without a device -- the size table against the sources,
every derived size past the threshold it claims, the float64 restatement against the existing test's own torch spelling, the ambiguity cap and the
planted table of every case, and the refusals the loss entries make before any device work."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import loss_ref as LR          # noqa: E402
import loss_sizes as LS        # noqa: E402

from neuman_hip import _lib    # noqa: E402

P = 0x10000                                                       # a non-null, 16-byte aligned address nothing dereferences: validation comes first


def err():
    return _lib.lib().nm_last_error().decode()


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LS.TABLE))
def test_the_size_table_reads_so_in_the_sources(name):
    value, path, pattern = LS.TABLE[name]
    found = re.findall(pattern, open(os.path.join(ROOT, path)).read())
    assert len(found) == 1, (name, found)
    groups = found[0] if isinstance(found[0], tuple) else (found[0],)
    assert int(np.prod([int(g) for g in groups])) == value, (name, groups)


def test_the_workspace_is_what_the_table_says():
    assert _lib.lib().nm_loss_workspace_doubles() == LS.WORKSPACE_DOUBLES == 6144


def test_every_derived_size_is_past_its_threshold():
    S, T = LS.SWEEP, LS.C.LOSS_THREADS
    assert S == 262144 and LS.loss_blocks(S) == LS.C.LOSS_MAX_BLOCKS and LS.sweeps(S) == 1
    assert [LS.sweeps(n) for n in LS.PAIR_SWEEP_SIZES] == [1, 2, 2, 3]
    assert LS.PAIR_SWEEP_SIZES[2] - S > T                        # the second sweep reaches a second workgroup
    assert LS.LARGEST == max(LS.PAIR_SWEEP_SIZES) == max(nh + nd for nh, nd in LS.SHAPE_SWEEP_SIZES) == 524291
    sums = [LS.sweeps(max(nh, nd)) for nh, nd in LS.SHAPE_SWEEP_SIZES]
    grad = [LS.sweeps(nh + nd) for nh, nd in LS.SHAPE_SWEEP_SIZES]
    assert sums == [2, 2, 1, 3, 1] and grad == [2, 2, 2, 3, 1]
    nh = LS.SHAPE_SWEEP_SIZES[2][0]
    assert nh % T != 0 and nh < S < 2 * nh                       # the switch falls inside a workgroup, and inside the gradient's first sweep
    assert [LS.loss_blocks(n) for n in LS.BLOCK_COUNT_SIZES] == [1, 2, 63, 64, 64, 65, 65, 66]
    assert LS.C.FINISH_LANES == 64 and set(LS.BLOCK_COUNTS) == {1, 63, 64, 65}
    assert LS.EDGE_SIZES[0] < S < LS.EDGE_SIZES[1] and LS.loss_blocks(LS.EDGE_SIZES[0]) > 1
    assert LS.planted_edges(LS.EDGE_SIZES[0]) == (0, T, LS.EDGE_SIZES[0]) and LS.planted_edges(LS.EDGE_SIZES[1]) == (0, T, S, LS.EDGE_SIZES[1])
    # frame
    assert LS.SSD_SWEEP == 16777216 and LS.SSD_PAST_THE_CAP == 16777216 + 257
    blocks = lambda n: min(LS.C.SSD_MAX_BLOCKS, (n + LS.C.SSD_PER_BLOCK - 1) // LS.C.SSD_PER_BLOCK)           # noqa: E731
    assert [blocks(n) for n in LS.SSD_SIZES_SMALL] == [1, 1, 1, 2]
    assert [blocks(n) for n in LS.SSD_SIZES_CAP + (LS.SSD_PAST_THE_CAP,)] == [4096] * 3 and blocks(LS.SSD_SWEEP - LS.C.SSD_PER_BLOCK) == 4095
    passes = lambda n: (n + LS.SSD_STRIDE - 1) // LS.SSD_STRIDE                                                # noqa: E731
    assert [passes(n) for n in LS.SSD_SIZES_CAP + (LS.SSD_PAST_THE_CAP,)] == [16, 17, 17]
    items = [LS.ssim_items(s) for s in LS.SSIM_SHAPES]
    assert LS.SSIM_SWEEP == 1048576 and items[0] == 1
    assert LS.SSIM_SWEEP < items[5] < 2 * LS.SSIM_SWEEP < items[6] < 3 * LS.SSIM_SWEEP                         # inside the second sweep; the third begins
    assert LS.ssim_items((800, 800, 3)) < 2 * LS.SSIM_SWEEP                                                    # (what the older test reaches)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_the_float64_run_is_the_existing_tests_own_spelling():
    """tests/test_hip_loss_ops.py's formulas on its own data: value and gradients, bit for bit or to rounding"""
    n = 1000
    a, b = LR.raw(n, 1), LR.raw(n, 2)
    ar, br = (torch.as_tensor(v).double().requires_grad_(True) for v in (a, b))
    want = 0.1 * F.mse_loss(torch.sigmoid(ar[:, :3]), torch.sigmoid(br[:, :3]))
    want.backward()
    got = LR.pair_mse(0, a, b, 0.1, torch.float64)
    assert got['value'] == pytest.approx(float(want.detach()), rel=1e-14)
    np.testing.assert_allclose(got['grads'][0], ar.grad.numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(got['grads'][1], br.grad.numpy(), rtol=1e-13, atol=0)
    ar.grad = br.grad = None
    squash = lambda raw: torch.tanh(torch.relu(raw[..., 3]))            # noqa: E731
    want = 0.25 * F.mse_loss(squash(ar), squash(br))
    want.backward()
    got = LR.pair_mse(1, a, b, 0.25, torch.float64)
    assert got['value'] == pytest.approx(float(want.detach()), rel=1e-14)
    np.testing.assert_allclose(got['grads'][0], ar.grad.numpy(), rtol=1e-13, atol=0)

    x = LR.unit(4099, 4099)
    for clamp in (True, False):
        xr = torch.as_tensor(x).double().requires_grad_(True)
        y = xr.clamp(0.0, 1.0) if clamp else xr
        want = torch.mean(-torch.log(torch.exp(-y.abs()) + torch.exp(-(1 - y).abs())) + LR.OFFSET)
        want.backward()
        got = LR.bimodal(x, clamp, LR.OFFSET, torch.float64)
        assert got['value'] == pytest.approx(float(want.detach()), rel=1e-14)
        np.testing.assert_allclose(got['grads'][0], xr.grad.numpy(), rtol=1e-13, atol=1e-300)

    def shape_ref(pred, dist_h, dummy, dist_d, w_smpl, w_dummy, factor, exponent):       # test_hip_loss_ops._shape_ref
        occ = lambda raw: 1 - torch.exp(-torch.relu(raw[..., 3]))       # noqa: E731

        def masked_mean(x, m):
            return x[m].mean() if bool(m.any()) else x.sum() * 0
        out = w_smpl * masked_mean((1 - occ(pred)) ** 2, dist_h < 0)
        out = out + w_dummy * masked_mean((1 - occ(dummy)) ** 2, dist_d < 0)
        return out + w_dummy * masked_mean((occ(dummy) * (dist_d.abs() * factor) ** exponent).abs(), dist_d > 0)

    pred, dummy, dh, dd = LR.raw(700, 5), LR.raw(300, 6), LR.dist(700, 7), LR.dist(300, 8, 0.4)
    dd[7] = 0.0
    pr, dr = (torch.as_tensor(v).double().requires_grad_(True) for v in (pred, dummy))
    want = shape_ref(pr, torch.as_tensor(dh).double(), dr, torch.as_tensor(dd).double(), 1.0, 0.7, 2.0, 2.0)
    want.backward()
    got = LR.shape(pred, dh, dummy, dd, 1.0, 0.7, 2.0, 2.0, torch.float64)
    assert got['value'] == pytest.approx(float(want.detach()), rel=1e-14)
    np.testing.assert_allclose(got['grads'][0], pr.grad.numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(got['grads'][1], dr.grad.numpy(), rtol=1e-12, atol=1e-300)


def test_the_edge_tables_hold_what_they_should():
    assert len(LR.RGB_EDGES) == 16 and len(LR.SIGMA_EDGES) == 13 and len(LR.DIST_EDGES) == 7
    assert not [s for s in LR.SIGMA_EDGES if 1e-12 < s < 1e-5]
    assert LR.TINY > 0 and np.float32(LR.TINY) / np.float32(2) == 0
    assert not any(np.isinf(d) for d in LR.DIST_EDGES) and sum(np.isnan(d) for d in LR.DIST_EDGES) == 1
    assert max(abs(x) for x in LR.BIMODAL_EDGES[False]) <= 60 and float('inf') in LR.BIMODAL_EDGES[True]
    for clamp in (True, False):
        E = np.asarray(LR.BIMODAL_EDGES[clamp], np.float32)
        for v in (0.0, 1.0, 0.5):
            assert {np.nextafter(np.float32(v), np.float32(-9)), np.float32(v), np.nextafter(np.float32(v), np.float32(9))} <= set(E)
        assert np.signbit(E[E == 0]).any() and not np.signbit(E[E == 0]).all()
    rows, d = LR.shape_rows()
    assert len(rows) == 13 * 7
    for n in LS.EDGE_SIZES:                                         # the planted copies straddle the edges: both neighbours of each are planted rows
        for T in (len(rows), 2 * len(LR.RGB_EDGES), len(LR.BIMODAL_EDGES[True])):
            starts = LR.plant_positions(n, T)
            assert len(starts) == len(LS.planted_edges(n))
            rows_planted = {r for s in starts for r in range(s, s + T)}
            want = {0, LS.C.LOSS_THREADS - 1, LS.C.LOSS_THREADS, n - 1} | ({LS.SWEEP - 1, LS.SWEEP} if n > LS.SWEEP else set())
            assert want <= rows_planted


# ---- every case of the device test -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LR.CASES))
def test_case_on_the_cpu(name):
    case = LR.CASES[name]()
    r64, r32 = LR.reference(case)
    total = sum(g.size for g in r64['grads'])
    masks = [LR.ambiguous(r64, r32, k) for k in range(len(r64['grads']))]
    n_amb = sum(int(m.sum()) for m in masks)
    assert n_amb <= 0.01 * total, (n_amb, total)
    # finite: every case asserts it on the device, so the float32 run must be (and the yardstick)
    for r in (r64, r32):
        assert np.isfinite(r['value']) and all(np.isfinite(g).all() for g in r['grads']), name
    if case['entry'] == 'shape' and 'planted' in case:
        sig, dd = case['dummy'][:, 3], case['dist_d']
        says = np.array([LR.table_is_ambiguous(float(sig[r]), float(dd[r])) for r in case['planted']])
        assert says.sum() == len(LR.plant_positions(len(sig), 13 * 7)) * (len(LR.AMBIGUOUS_SIGMA_AT_DIST_1) + 6)    # 6 sigma edges lie above float64's own zero
        assert np.array_equal(masks[1][case['planted'], 3], says)
        assert n_amb == says.sum() and not masks[0].any()         # and nothing else is
        assert np.all(r32['grads'][1][masks[1]] == 0.0) and np.all(r64["grads"][1][masks[1]] >= 0.0)
    else:
        assert n_amb == 0
    if 'expect' in case:
        assert tuple(c > 0 for c in r64['counts']) == case['expect'] and r64['counts'] == r32['counts']
        if case['expect'] == (True, False, False) or case['expect'][1]:
            assert 1 in r64['counts']                              # exactly one element in a selection
        if not (case['expect'][1] or case['expect'][2]):
            assert np.all(case['dist_d'] == 0) and np.signbit(case['dist_d']).any() and not np.signbit(case['dist_d']).all()
    if 'edge_items' in case:                                       # a live gradient on both sides of every switch and sweep edge
        for which, r in case['edge_items']:
            assert r64['grads'][0 if which == 'pred' else 1][r, 3] != 0.0, (which, r)
    if case['entry'] == 'pair':                                    # the columns a term does not read
        col = [3] if case['mode'] == 0 else [0, 1, 2]
        assert all(np.all(g[:, col] == 0) for g in r64['grads'])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_bimodal_refuses_bad_arguments_before_any_device_work():
    L = _lib.lib()
    for args in ((P, 0, 1, 0.0, P, P, P, None), (P, -1, 1, 0.0, P, P, P, None), (None, 4, 1, 0.0, P, P, P, None), (P, 4, 1, 0.0, None, P, P, None),
                 (P, 4, 1, 0.0, P, None, P, None), (P, 4, 1, 0.0, P, P, None, None)):
        assert L.nm_loss_bimodal(*args) == -1 and "nm_loss_bimodal" in err(), args


def test_pair_mse_refuses_bad_arguments_before_any_device_work():
    L = _lib.lib()
    good = [0, P, P, 4, 0.1, P, P, P, P, None]
    for i, v in ((3, 0), (3, -5), (1, None), (2, None), (5, None), (6, None), (7, None), (8, None), (0, 2), (0, -1)):
        args = list(good)
        args[i] = v
        assert L.nm_loss_pair_mse(*args) == -1 and "nm_loss_pair_mse" in err(), args
    for i in (1, 2, 6, 7):                                          # a row pointer off a 16-byte boundary
        for off in (4, 8):
            args = list(good)
            args[i] = P + off
            assert L.nm_loss_pair_mse(*args) == -1 and "nm_loss_pair_mse" in err() and "aligned" in err(), args


def test_shape_refuses_bad_arguments_before_any_device_work():
    L = _lib.lib()
    good = [P, P, 4, P, P, 4, 1.0, 0.7, 2.0, 2.0, P, P, P, P, P, None]
    for i, v in ((2, 0), (2, -1), (5, -1), (0, None), (1, None), (10, None), (11, None), (13, None), (14, None)):
        args = list(good)
        args[i] = v
        assert L.nm_loss_shape(*args) == -1 and "nm_loss_shape" in err(), args
    for i in (3, 4, 12):                                            # nd > 0 without one of its arrays
        args = list(good)
        args[i] = None
        assert L.nm_loss_shape(*args) == -1 and "nm_loss_shape" in err() and "dummy" in err(), args
    for i in (0, 3, 11, 12):
        args = list(good)
        args[i] = P + 8
        assert L.nm_loss_shape(*args) == -1 and "nm_loss_shape" in err() and "aligned" in err(), args


def test_the_wrapper_hands_the_kernels_aligned_dense_rows():
    """loss_ops._rows: a strided view and a dense view that starts 8 bytes off a 16-byte boundary both become aligned [n,4] rows of the same values;
    rows that already are stay where they are (no copy on the trainer's path)"""
    from neuman_hip import loss_ops
    n = 37
    flat = torch.arange(4 * n + 6, dtype=torch.float32)
    dense = flat[2:2 + 4 * n].view(n, 4)
    assert dense.is_contiguous() and dense.data_ptr() % 16 == 8
    wide = torch.arange(6 * n, dtype=torch.float32).view(n, 6)
    for view in (dense, wide[:, 1:5], dense.double(), dense.reshape(1, n, 4)):
        r = loss_ops._rows(view)
        assert r.dtype == torch.float32 and r.is_contiguous() and r.data_ptr() % 16 == 0 and r.shape == (n, 4)
        assert torch.equal(r, view.reshape(-1, 4).float())
    good = torch.zeros(n, 4)
    assert loss_ops._rows(good).data_ptr() == good.data_ptr() == loss_ops._rows(good.view(1, n, 4)).data_ptr()
