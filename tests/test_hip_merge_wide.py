"""-m gpu: nm_merge_composite_lists_wide (csrc/merge_wide.hip; render_utils.merge_composite_lists_wide) -- up to 32 sorted lists per ray merged
in the stable order and composited by ONE kernel -- against merge_sorted list by list + raw2outputs (existing entry points): rgb, depth and acc
equal BIT FOR BIT, white background or not, with exact z ties between lists, compact lists and placeholder rows reached through `rows`, past one
sweep of the grid inside guarded allocations; up to four lists it also equals merge_composite_lists; what it cannot stage is refused."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import compositing
from test_hip_fused import _lists
from test_hip_sizes import P, check, lib, same, stream, sweep_checked
from test_multi_fused_host import WIDE_GRID_MAX_BLOCKS, WIDE_MAX_WAVES

pytestmark = pytest.mark.gpu

CASES = {
    'five_tiny': (1, (3, 2, 1, 1, 2)),
    'six_ragged': (130, (64, 17, 5, 9, 33, 1)),
    'five_actors': (301, (320, 192, 192, 192, 192, 192)),
    'eight_actors': (257, (320,) + (192,) * 8),                    # 1856 merged samples: BASELINE config 5 with eight actors
    'thirty_two': (67, (4,) * 32),
}


@pytest.fixture(scope="module")
def R_():
    from neuman_hip import _lib, render_utils
    _lib.require_gpu()
    return render_utils


def dirs(R, seed=5):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((R, 3), device='cuda', generator=g) * 0.15 + torch.tensor([0., 0., 1.], device='cuda'), dim=-1).contiguous()


def list_by_list(R_, zs, raws, d, white):
    """the reference of every case: nm_merge_sorted list by list, then nm_composite -> (rgb, depth, acc)"""
    z_all, raw_all = zs[0], raws[0]
    for z, raw in zip(zs[1:], raws[1:]):
        z_all, raw_all = R_.merge_sorted(z_all, raw_all, z, raw)
    rgb, _, acc, _, depth = R_.raw2outputs(raw_all, z_all, d, white_bkg=white, want_weights=False)
    return rgb, depth, acc


_made = {}


def case(R_, name):
    """inputs and references of a case, made once and shared by the tests that read them"""
    if name not in _made:
        R, sizes = CASES[name]
        d = dirs(R)
        zs, raws = _lists(R, sizes, 11)
        assert any(bool((zs[l][:, :, None] == zs[0][:, None, :]).any()) for l in range(1, len(sizes)))      # exact cross-list ties
        _made[name] = (zs, raws, d, {w: list_by_list(R_, zs, raws, d, w) for w in (True, False)})
    return _made[name]


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_wide_merge_is_bit_identical_to_merging_list_by_list(R_, name, white):
    zs, raws, d, ref = case(R_, name)
    out = R_.merge_composite_lists_wide(zs, raws, d, white)
    for x, y, what in zip(out, ref[white], ("rgb", "depth", "acc")):
        assert torch.isfinite(x).all() and torch.equal(x, y), (name, white, what, float((x - y).abs().max()))


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_up_to_four_lists_equal_the_narrow_kernel(R_, k):
    R, sizes = 70, (7, 5, 3, 6)[:k]
    d = dirs(R, 6)
    zs, raws = _lists(R, sizes, 12)
    for white in (True, False):
        ref = list_by_list(R_, zs, raws, d, white)
        narrow = R_.merge_composite_lists(zs, raws, d, white)
        wide = R_.merge_composite_lists_wide(zs, raws, d, white)
        for x, y, r in zip(wide, narrow, ref):
            assert torch.equal(x, y) and torch.equal(x, r), (k, white)


def expand(z, raw, rows):
    return (z, raw) if rows is None else (z[rows.long()].contiguous(), raw[rows.long()].contiguous())


def test_placeholder_rows_shared_by_three_of_six_lists(R_):
    """the multi-person renderer's lists: the background, two actors as compact [n_hit + 1, S] arrays behind a row index, and three actors nobody
    hits -- the SAME one-row placeholder arrays, every ray pointing at row 0"""
    R, S = 203, 24
    g = torch.Generator(device='cuda').manual_seed(2)
    d = dirs(R, 7)
    (zb, z1, z2), (rawb, raw1, raw2) = _lists(R, (40, S, S), 13)
    pad_z, pad_raw = torch.linspace(8.0, 12.0, S, device='cuda')[None].contiguous(), torch.zeros((1, S, 4), device='cuda')
    lists = [(zb, rawb, None)]
    for z, raw in ((z1, raw1), (z2, raw2)):
        hit = torch.nonzero(torch.rand(R, device='cuda', generator=g) < 0.6).reshape(-1)
        rows = torch.full((R,), hit.numel(), device='cuda', dtype=torch.int32)
        rows[hit] = torch.arange(hit.numel(), device='cuda', dtype=torch.int32)
        lists.append((torch.cat([z[hit], pad_z]).contiguous(), torch.cat([raw[hit], pad_raw]).contiguous(), rows))
    zero = torch.zeros(R, device='cuda', dtype=torch.int32)
    lists = lists[:2] + [(pad_z, pad_raw, zero)] * 2 + lists[2:] + [(pad_z, pad_raw, zero)]
    full = [expand(*l) for l in lists]
    for white in (True, False):
        ref = list_by_list(R_, [f[0] for f in full], [f[1] for f in full], d, white)
        out = R_.merge_composite_lists_wide([l[0] for l in lists], [l[1] for l in lists], d, white, rows=[l[2] for l in lists])
        assert all(torch.equal(x, y) for x, y in zip(out, ref)), white


def test_background_list_read_in_place_through_a_hit_index(R_):
    R_all, R = 700, 211
    d_all = dirs(R_all, 8)
    (zb,), (rawb,) = _lists(R_all, (96,), 3, ties=False)
    hit = torch.sort(torch.randperm(R_all, device='cuda')[:R])[0].to(torch.int32)
    zh, rawh = _lists(R, (33, 20, 20, 20, 7), 4)
    zh, rawh = zh[1:], rawh[1:]                                   # (four actor lists)
    hd = d_all[hit.long()].contiguous()
    a = R_.merge_composite_lists_wide([zb] + zh, [rawb] + rawh, hd, True, rows=[hit, None, None, None, None])
    ref = list_by_list(R_, [zb[hit.long()].contiguous()] + zh, [rawb[hit.long()].contiguous()] + rawh, hd, True)
    assert all(torch.equal(x, y) for x, y in zip(a, ref))


def test_wide_merge_past_one_sweep_of_the_grid_in_guarded_arrays(R_):
    """R = 4096 blocks x waves per block + 37 rays (14 merged samples leave room for the most waves a block takes): rows beyond the grid are
    reached by the grid-stride loop.  Every array inside a larger allocation with sentinel guard rows: no write outside the outputs, finite
    junk in the input guards changes nothing, and the launch equals the same launch cut into row slices"""
    sizes = (4, 3, 2, 2, 3)
    k = len(sizes)
    sweep = WIDE_GRID_MAX_BLOCKS * WIDE_MAX_WAVES
    R = sweep + 37
    zs, raws = _lists(R, sizes, 14)
    ins = {'d': dirs(R, 9)}
    for l in range(k):
        ins[f'z{l}'], ins[f'raw{l}'] = zs[l], raws[l]
    arr = ctypes.c_void_p * k

    def launch(I, O_, i, j):
        check(lib().nm_merge_composite_lists_wide(k, arr(*[I[f'z{l}'][i:j].data_ptr() for l in range(k)]), arr(*[I[f'raw{l}'][i:j].data_ptr() for l in range(k)]),
                                                  None, (ctypes.c_int * k)(*sizes), j - i, P(I['d'][i:j]), 1, P(O_['rgb'][i:j]), P(O_['depth'][i:j]),
                                                  P(O_['acc'][i:j]), stream()), "nm_merge_composite_lists_wide")
    I, out = sweep_checked(launch, ins, dict(rgb=(R, 3), depth=(R,), acc=(R,)), R, 5000)
    ref = list_by_list(R_, zs, raws, ins['d'], True)
    assert same(out['rgb'], ref[0]) and same(out['depth'], ref[1]) and same(out['acc'], ref[2])


def test_wide_merge_against_the_oracle(R_):
    """sort(cat(lists)) + raw2outputs of the CPU oracle, within the 2e-5 tests/test_hip_fused.py holds the device composite to"""
    zs, raws, d, _ = case(R_, 'six_ragged')
    zm, rawm = compositing.merge_sorted([z.cpu().numpy() for z in zs], [r.cpu().numpy() for r in raws])
    o = compositing.raw2outputs(rawm, zm, d.cpu().numpy())
    rgb, depth, acc = R_.merge_composite_lists_wide(zs, raws, d, True)
    assert np.abs(rgb.cpu().numpy() - o[0]).max() < 2e-5 and np.abs(acc.cpu().numpy() - o[2]).max() < 2e-5


def test_shapes_the_kernel_cannot_stage_are_refused(R_):
    from neuman_hip import _lib
    R = 8
    d = dirs(R, 10)
    zs, raws = _lists(R, (2,) * 33, 15)
    with pytest.raises(_lib.NeumanHipError, match="nm_merge_composite_lists_wide|merge_composite_lists_wide"):
        R_.merge_composite_lists_wide(zs, raws, d)
    arr = ctypes.c_void_p * 33                                    # ... and by the library itself
    rgb, depth, acc = (torch.full(s, 7.25, device='cuda') for s in ((R, 3), (R,), (R,)))
    rc = lib().nm_merge_composite_lists_wide(33, arr(*[z.data_ptr() for z in zs]), arr(*[r.data_ptr() for r in raws]), None, (ctypes.c_int * 33)(*[2] * 33), R,
                                             P(d), 1, P(rgb), P(depth), P(acc), stream())
    assert rc == -1 and b"nm_merge_composite_lists_wide" in lib().nm_last_error()
    half = R_.WIDE_MERGE_MAX_SAMPLES // 2 + 1                     # two lists, one sample more than can be staged
    zs, raws = _lists(R, (half, half), 16, ties=False)
    with pytest.raises(_lib.NeumanHipError, match=f"nm_merge_composite_lists_wide.*{R_.WIDE_MERGE_MAX_SAMPLES}"):
        R_.merge_composite_lists_wide(zs, raws, d)
    arr = ctypes.c_void_p * 2
    rc = lib().nm_merge_composite_lists_wide(2, arr(*[z.data_ptr() for z in zs]), arr(*[r.data_ptr() for r in raws]), None, (ctypes.c_int * 2)(half, half), R, P(d), 1,
                                             P(rgb), P(depth), P(acc), stream())
    torch.cuda.synchronize()
    assert rc == -1 and all(bool((t == 7.25).all()) for t in (rgb, depth, acc))       # nothing was launched
