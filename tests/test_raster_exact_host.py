"""Without a device: the exact reference of the rasteriser's rules 1-3 and its quarter-pixel scenes (tests/helpers/raster_exact.py) against
the project's float64 restatement of the same contract (tests/helpers/raster_ref.py), at EVERY pixel -- the ones whose centre lies on an
edge or a vertex and the exact depth ties included, which every other parity test of the family has to leave out.  Also: that each scene
still exercises the case it exists for (its declared counts), that it can see the two classic mistakes (open edges, the higher id on a
tie), that the preconditions are verified and not assumed, and that the reference's rounding is float32's.
tests/test_hip_raster_exact.py holds the device to the same figures."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import raster_exact as RX  # noqa: E402
import raster_ref as RR  # noqa: E402

NAMES = list(RX.SCENES)


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_the_float64_helper_at_every_pixel(name):
    sc = RX.SCENES[name]
    ex = RX.exact_of(name)                                      # (raises LatticeError if a precondition fails)
    H, W = sc.H, sc.W
    assert ex['face_id'].shape == (H, W) and ex['face_id'].dtype == np.int32 and ex['zbuf'].dtype == np.float32 and ex['bary'].dtype == np.float32
    cov = ex['face_id'] >= 0
    assert np.array_equal(cov, ex['n_cover'] > 0) and np.all(np.isposinf(ex['zbuf'][~cov])) and np.all(ex['bary'][~cov] == 0)
    r32 = RR.rasterize(sc.verts, sc.faces, sc.camera, np.float32)
    for brute in (False, True):
        r64 = RR.rasterize(sc.verts, sc.faces, sc.camera, np.float64, brute=brute)
        assert np.array_equal(r64['face_id'], ex['face_id'])                     # every pixel: no ambiguity map
        # the float64 run carries the exact quotient to 2^-52; the exact reference is that quotient rounded to float32 once: half an ulp
        for k in ('zbuf', 'bary'):
            assert np.all(np.abs(r64[k][cov] - ex[k][cov].astype(np.float64)) <= 2.0 ** -24 * np.abs(r64[k][cov]) + 1e-300), k
    # the float32 run of the helper does the device's arithmetic: exact operands, one division -- the same bits
    assert np.array_equal(r32['face_id'], ex['face_id']) and np.array_equal(r32['zbuf'], ex['zbuf']) and np.array_equal(r32['bary'], ex['bary'])
    assert r64['face_id'].size == H * W                                          # all of them
    # the scene still exercises what it exists for, and can see the two mistakes
    n_open, n_tie = RX.wrong_rule_pixels(sc)
    print(f"[raster-exact] {name}: {H * W} px, {int(cov.sum())} covered by {ex['n_valid']} of {len(sc.faces)} faces, {ex['on_edge']} centres on an edge "
          f"(declared >= {sc.min_edge}), {ex['on_vertex']} on a vertex (>= {sc.min_vertex}); open edges change {n_open} px (>= {sc.min_open}), the higher id "
          f"on a tie {n_tie} (>= {sc.min_tie})")
    assert ex['on_edge'] >= sc.min_edge and ex['on_vertex'] >= sc.min_vertex
    assert n_open >= sc.min_open and n_tie >= sc.min_tie
    if not sc.id_dependent:
        assert n_tie == 0                                       # (what lets the device test permute the face list)


def test_the_families_pin_what_they_say():
    """figures the issue states, and the properties the device tests lean on"""
    S, ex = RX.SCENES, RX.exact_of
    assert S['diagonal-o0w0z22-32x24'].min_edge >= 12
    for o in (0, 1):
        for w in (0, 1):
            name = f'diagonal-o{o}w{w}z22-32x24'
            f = ex(name)['face_id']
            diag = np.array([f[3 + k, 2 + k] for k in range(16)])
            assert np.all(diag == 0) and np.all(ex(name)['n_cover'][3 + np.arange(16), 2 + np.arange(16)] == 2), name
    for name, winner in (('diagonal-o0w0z42-32x24', 1), ('diagonal-o1w1z24-32x24', 1), ('diagonal-o0w1z14-32x24', 0)):
        assert all(ex(name)['face_id'][3 + k, 2 + k] == winner for k in range(16)), name        # depth before id
    for hub in (15.5, 16.5):
        r, c = int(hub), int(hub)
        assert ex(f'fan-hub{hub}-flat')['face_id'][r, c] == 0 and ex(f'fan-hub{hub}-flat')['n_cover'][r, c] == 8
        for k in range(8):
            assert ex(f'fan-hub{hub}-near{k}')['face_id'][r, c] == k and ex(f'fan-hub{hub}-near{k}')['zbuf'][r, c] == 1
    # rejected: the six bad faces are dropped, and the result is the scene without them (ids shifted by their number)
    a, b = ex('rejected'), ex('rejected-without')
    assert a['n_valid'] == 2 and len(S['rejected'].faces) == 8 and np.array_equal(a['face_id'], b['face_id'] + 6) and np.array_equal(a['zbuf'], b['zbuf'])
    assert np.array_equal(a['n_cover'], b['n_cover']) and a['zbuf'].min() == 2
    # slivers: four faces win nowhere, the others exactly one pixel each
    f = ex('slivers')['face_id']
    assert [int((f == k).sum()) for k in range(1, 10)] == [0, 0, 0, 0, 1, 1, 1, 1, 1] and (f >= 0).all()
    # perspective: both faces win, depth and barycentrics are not short numbers
    for o in (0, 1):
        r = ex(f'perspective-o{o}')
        assert min(int((r['face_id'] == 0).sum()), int((r['face_id'] == 1).sum())) > 40 and int((r['n_cover'] == 2).sum()) > 60
        z = r['zbuf'][r['face_id'] >= 0]
        assert len(np.unique(z)) > 200 and np.mean(np.frexp(z)[0] * 2.0 ** 24 % 2.0 ** 12 != 0) > 0.5      # most depths use the low mantissa bits
    # stack: the list of tile (1, 0) straddles the batch of 256
    for N in (255, 256, 257, 512, 513):
        assert ex(f'stack-{N}-flat')['n_cover'].max() == N and set(np.unique(ex(f'stack-{N}-flat')['face_id'])) == {-1, 0}
        assert set(np.unique(ex(f'stack-{N}-near{N - 1}')['face_id'])) == {-1, N - 1}
    # seams: a leg on a column of centres covers them, one on a pixel border covers up to it
    f = ex('seams-xmax-40x48')['face_id']
    assert (f[:, 0] >= 0).sum() == 4 and f[:, 16].max() == 5 and (f[:, 39] >= 0).sum() == 4 + 4 + 3 and (f[:, 17:36] < 0).all()
    assert {(s.W, s.H) for n, s in S.items() if n.startswith(('diagonal', 'seams'))} >= set(RX.TINY)


def test_preconditions_are_verified_not_assumed():
    sc = RX.SCENES['perspective-o0']

    def variant(**kw):
        args = dict(name='bad', verts=sc.verts, faces=sc.faces, W=sc.W, H=sc.H, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, t=sc.w2c[:, 3])
        args.update(kw)
        return RX.Scene(**args)

    RX.check(variant())
    off = sc.verts.copy()
    off[0, 0] += np.float32(1 / 256)                            # an eighth of a pixel at z = 1
    bad = [variant(verts=off), variant(fx=sc.fx * 1.1), variant(cx=sc.cx + 0.125), variant(t=(1, -2, 1)), variant(W=65), variant(t=(1.5, -2, 0))]
    third = sc.verts.copy()
    third[1, 2] -= 1                                            # camera z = 3
    bad.append(variant(verts=third))
    for s in bad:
        with pytest.raises(RX.LatticeError):
            RX.check(s)
    # 24 significant bits: a triangle whose edge functions need 25
    big = 2.0 ** 13
    wide = RX.Scene('wide', np.array([[0.25, 0.25, 1], [big + 0.25, 0.5, 1], [0.5, big + 0.25, 1]], np.float32), [[0, 1, 2]], 8, 8, 1, 1, 0, 0)
    with pytest.raises(RX.LatticeError, match="24 bits"):
        RX.check(wide)
    # two depths that differ by less than 2^-20 relative: neither a tie nor a clear win.  Two faces of one projection at depths 4 and
    # 4 (1 + 2^-22) cannot be put on the lattice (z is 1, 2 or 4), which is the point; the gap test itself is shown on its inputs
    a = RX.Scene('tie', np.array([[0, 0, 2], [8, 0, 2], [0, 8, 2]] * 2, np.float32), [[0, 1, 2], [3, 4, 5]], 8, 8, 2, 2, 0, 0)
    RX.check(a)
    saved = RX.CLEAR_WIN
    try:
        RX.CLEAR_WIN = 2.0                                      # now depths 2 and 4 on one pixel count as too close
        near = RX.Scene('near', np.array([[0, 0, 2], [8, 0, 2], [0, 8, 2], [0, 0, 4], [16, 0, 4], [0, 16, 4]], np.float32), [[0, 1, 2], [3, 4, 5]], 8, 8, 2, 2, 0, 0)
        with pytest.raises(RX.LatticeError, match="closer than"):
            RX.check(near)
        RX.check(a)                                             # an exact tie stays acceptable
    finally:
        RX.CLEAR_WIN = saved


def test_rounding_is_float32s_own():
    """round_f32 works in integers; it equals np.float32(float(Fraction)) -- numpy's correctly rounded conversions -- on every value the scenes
    produce and on the cases a rounding routine gets wrong: ties to even, a carry into the next binade, one unit either side of a tie"""
    seen = 0
    for name in NAMES:
        RX.exact_of(name)
    assert len(RX._ROUND_CACHE) > 1000
    for (n, d), v in RX._ROUND_CACHE.items():
        assert isinstance(v, np.float32) and v == np.float32(float(Fraction(n, d))), (n, d)
        # float(Fraction) rounds to float64 first: harmless only if that lands on no float32 tie the exact value is off
        lo, hi = np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))
        x = Fraction(n, d)
        assert abs(x - Fraction(float(v))) <= abs(x - Fraction(float(lo))) and abs(x - Fraction(float(v))) <= abs(x - Fraction(float(hi))), (n, d)
        seen += 1
    m = 1 << 24
    cases = [(m + 1, m, 1.0), (m + 3, m, 1.0 + 2.0 ** -22), (2 * m + 1, 2 * m, 1.0), (2 * m + 3, 2 * m, 1.0 + 2.0 ** -23), (2 * m - 1, 2 * m, 1.0),
             (4 * m - 1, 4 * m, 1.0), (1, 3, np.float32(1) / np.float32(3)), (2, 3, np.float32(2) / np.float32(3)), (7, 1, 7.0), (1, 1 << 20, 2.0 ** -20),
             (3 * m + 2, 2 * m, 1.5), (3 * m + 6, 2 * m, 1.5 + 2.0 ** -22), ((1 << 30) + 64, 1 << 30, 1.0), ((1 << 30) + 65, 1 << 30, 1.0 + 2.0 ** -23), (0, 5, 0.0)]
    for n, d, want in cases:
        assert RX.round_f32(n, d) == np.float32(want) and RX.round_f32(n, d).dtype == np.float32, (n, d)
    rng = np.random.default_rng(0)
    for n, d in rng.integers(1, 1 << 26, (2000, 2)).tolist():
        x = Fraction(n, d)
        v = RX.round_f32(n, d)
        lo, hi = np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))
        assert abs(x - Fraction(float(v))) <= min(abs(x - Fraction(float(lo))), abs(x - Fraction(float(hi)))), (n, d)
        assert v == np.float32(n) / np.float32(d) or n >= m or d >= m             # float32's own division, where the operands are float32s
