"""The mesh rasteriser's rules 1-3 (include/neuman_hip.h 'mesh rasteriser') in integer and rational arithmetic, and the scenes on which that
arithmetic predicts the device's float32 bits at EVERY pixel: tests/test_raster_exact_host.py and tests/test_hip_raster_exact.py.

tests/helpers/raster_ref.py, the float64 restatement every other parity test of this family compares with, has to exclude the pixels whose
centre is within 1e-4 of an edge or whose two nearest depths are within 1e-4 of each other: on a capsule seen from an arbitrary camera float32
and float64 may disagree there.  Those are the pixels the closed-edge rule, the tie rule and the tile boxes' floors are about.  Here every
screen coordinate is an integer multiple of 1/4 pixel and every camera-space z is 1, 2 or 4 (or <= 0, which drops the face), so

  * a pixel centre (c + 0.5, r + 0.5) and every vertex are integers in quarter-pixel units, the translated vertices are integers, the edge
    functions are integers of a few thousand sixteenths: float32 products of differences compute them without rounding;
  * 1/z is a power of two, so w_i / z_i, q = w0/z0 + w1/z1 + w2/z2 and s = w0 + w1 + w2 are exact too;
  * depth = s / q and b_i' = (w_i / z_i) / q are then ONE float32 division of two exactly known numbers: the exact quotient rounded once.

`check` verifies all of that from the float32 inputs with fractions.Fraction (it assumes nothing about how a scene was built) and raises
LatticeError otherwise; `exact_rasterize` applies the rules, written from the header:

  rule 1  Xc = R Xw + t, u = fx Xc.x / Xc.z + cx, v = fy Xc.y / Xc.z + cy; pixel (r, c) is sampled at (c + 0.5, r + 0.5)
  rule 2  a face with a vertex at z <= 0 is dropped whole, so is a face of zero screen area; a face covers a centre whose three screen
          barycentrics are all >= 0 -- closed on all three edges, for either winding
  rule 3  depth = s / q, b_i' = (w_i / z_i) / q; the winner is the minimum of (float32 depth, face id); nothing covers: -1, +inf, 0

Every scene declares how many pixel centres lie exactly on an edge and exactly on a vertex of a valid face (min_edge, min_vertex) and on how
many pixels the two classic mistakes (open edges; the higher id on a depth tie) change the winner (min_open, min_tie); exact_rasterize
returns the first two, wrong_rule_pixels the last two, and the host test holds every scene to its figures."""
import collections
from fractions import Fraction

import numpy as np

SIG_BITS = 24                                                  # float32's significand
CLEAR_WIN = 2.0 ** -20                                         # two unequal exact depths on one pixel are at least this far apart, relative
TILE = 16                                                      # the device's tile side; its LDS batch is TILE * TILE faces


class LatticeError(ValueError):
    """a scene on which float32 would not be exact, or on which a depth comparison is neither a tie nor a clear win"""


class Scene:
    def __init__(self, name, verts, faces, W, H, fx, fy, cx, cy, t=(0, 0, 0), min_edge=0, min_vertex=0, min_open=0, min_tie=0, id_dependent=False,
                 pins=''):
        self.name, self.W, self.H = name, int(W), int(H)
        self.verts = np.ascontiguousarray(verts, np.float32)
        self.faces = np.ascontiguousarray(faces, np.int32)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.w2c = np.concatenate([np.eye(3), np.asarray(t, np.float64).reshape(3, 1)], 1)
        self.min_edge, self.min_vertex, self.min_open, self.min_tie = min_edge, min_vertex, min_open, min_tie
        self.id_dependent = id_dependent                       # the expected ids depend on the order of the face list (a depth tie somewhere)
        self.pins = pins
        for a in (self.verts, self.faces, self.w2c):
            a.setflags(write=False)

    @property
    def camera(self):
        """as raster_ref.rasterize and neuman_hip.raster.Rasterizer.rasterize take it"""
        return self.w2c, self.fx, self.fy, self.cx, self.cy, self.W, self.H

    def __repr__(self):
        return f"Scene({self.name}, {self.W} x {self.H}, F={len(self.faces)})"


# ---- the preconditions -------------------------------------------------------------------------------------------------------------------
def _sig_bits_ok(x):
    """every int64 of the arrays x has at most SIG_BITS significant bits (trailing zeros are the exponent's)"""
    x = np.abs(np.concatenate([np.asarray(a, np.int64).ravel() for a in x]))
    x = x[x != 0]
    return x.size == 0 or bool(np.all(x // (x & -x) < (1 << SIG_BITS)))


def _need(ok, scene, what):
    if not ok:
        raise LatticeError(f"{scene.name}: {what}")


def project(scene):
    """rule 1 on the float32 inputs in fractions.Fraction -> (U, V int64 [nv]: 4 u, 4 v, 0 for a vertex at z <= 0; Z int64 [nv]: camera z,
    0 standing for any z <= 0).  LatticeError unless w2c is the identity with an integer translation, z is 1, 2, 4 or <= 0, and u, v are
    multiples of 1/4"""
    R, t = scene.w2c[:, :3], scene.w2c[:, 3]
    _need(np.array_equal(R, np.eye(3)) and np.array_equal(t, np.round(t)), scene, "w2c must be the identity or an integer translation")
    _need(scene.W >= 1 and scene.H >= 1 and scene.W <= 64 and scene.H <= 48, scene, "at most 64 x 48")
    fx, fy, cx, cy = (Fraction(x) for x in (scene.fx, scene.fy, scene.cx, scene.cy))
    nv = len(scene.verts)
    U, V, Z = np.zeros(nv, np.int64), np.zeros(nv, np.int64), np.zeros(nv, np.int64)
    for i, (x, y, z) in enumerate(scene.verts.tolist()):        # float32 -> Python float -> Fraction: exact
        xc, yc, zc = Fraction(x) + int(t[0]), Fraction(y) + int(t[1]), Fraction(z) + int(t[2])
        if zc <= 0:
            continue
        _need(zc in (1, 2, 4), scene, f"vertex {i}: camera z = {zc} is none of 1, 2, 4 or <= 0")
        u4, v4 = 4 * (fx * xc / zc + cx), 4 * (fy * yc / zc + cy)
        _need(u4.denominator == 1 and v4.denominator == 1, scene, f"vertex {i}: (u, v) = ({u4 / 4}, {v4 / 4}) is off the quarter-pixel lattice")
        # the device forms fx * xc * (1 / zc) + cx in float64: exact when every factor and the result are short dyadic numbers
        for q in (fx * xc, fx * xc / zc, fy * yc, fy * yc / zc):
            _need(q.denominator & (q.denominator - 1) == 0 and abs(q.numerator).bit_length() <= 50, scene, f"vertex {i}: the float64 projection rounds")
        U[i], V[i], Z[i] = int(u4), int(v4), int(zc)
    return U, V, Z


def _evaluate(scene):
    """Everything the rules need, in integers: per valid face (ascending id) and pixel the edge functions, s and q in sixteenths of a squared
    pixel (q times 4).  Raises LatticeError where a float32 intermediate of the device would round."""
    U, V, Z = project(scene)
    f = scene.faces.astype(np.int64)
    _need(f.ndim == 2 and f.shape[1] == 3 and f.min() >= 0 and f.max() < len(U), scene, "faces must be [F,3] indices into verts")
    front = (Z[f] > 0).all(1)
    ax, ay, bx, by, cx, cy = U[f[:, 0]], V[f[:, 0]], U[f[:, 1]], V[f[:, 1]], U[f[:, 2]], V[f[:, 2]]
    d = [bx - ax, cy - ay, by - ay, cx - ax]
    area = d[0] * d[1] - d[2] * d[3]
    _need(_sig_bits_ok([x[front] for x in d + [d[0] * d[1], d[2] * d[3], area]]), scene, "the screen area needs more than 24 bits")
    valid = np.flatnonzero(front & (area != 0))
    f = f[valid]
    col, row = np.meshgrid(np.arange(scene.W, dtype=np.int64), np.arange(scene.H, dtype=np.int64))
    px, py = (4 * col + 2).reshape(1, -1), (4 * row + 2).reshape(1, -1)      # the pixel centres, in quarter pixels
    ax, ay = U[f[:, 0]][:, None] - px, V[f[:, 0]][:, None] - py
    bx, by = U[f[:, 1]][:, None] - px, V[f[:, 1]][:, None] - py
    cx, cy = U[f[:, 2]][:, None] - px, V[f[:, 2]][:, None] - py
    prod = [bx * cy, by * cx, cx * ay, cy * ax, ax * by, ay * bx]
    w = [prod[0] - prod[1], prod[2] - prod[3], prod[4] - prod[5]]            # w0 pairs (v1, v2), w1 (v2, v0), w2 (v0, v1)
    s01 = w[0] + w[1]
    s = s01 + w[2]
    qi = [w[k] * (4 // Z[f[:, k]])[:, None] for k in range(3)]                # 4 w_k / z_k: a power-of-two scaling
    q01 = qi[0] + qi[1]
    q = q01 + qi[2]
    _need(_sig_bits_ok([ax, ay, bx, by, cx, cy] + prod + w + [s01, s]), scene, "an intermediate of edge_functions or of s needs more than 24 bits")
    _need(_sig_bits_ok(qi + [q01, q]), scene, "an intermediate of q needs more than 24 bits")
    return valid, w, s, qi, q


_ROUND_CACHE = {}


def round_f32(n, d):
    """the rational n / d (Python ints, n >= 0, d > 0) rounded to float32 once, to nearest with ties to even, in integer arithmetic"""
    if n == 0:
        return np.float32(0)
    e = n.bit_length() - d.bit_length() - SIG_BITS             # n / d / 2^e lies in (2^23, 2^25)
    num, den = (n << -e, d) if e < 0 else (n, d << e)
    if num >= den << SIG_BITS:                                 # ... bring it into [2^23, 2^24)
        den <<= 1
        e += 1
    m, r = divmod(num, den)
    assert (1 << (SIG_BITS - 1)) <= m < (1 << SIG_BITS)
    if 2 * r > den or (2 * r == den and m & 1):
        m += 1
    return np.ldexp(np.float32(m), e)                          # m <= 2^24 is a float32; the scaling is exact (no subnormals here: asserted by the caller)


def _round_array(n, d):
    """round_f32 over int64 arrays of one shape, through the distinct reduced fractions"""
    n, d = np.asarray(n, np.int64), np.asarray(d, np.int64)
    g = np.gcd(n, d)
    pairs, inverse = np.unique(np.stack([(n // g).ravel(), (d // g).ravel()], 1), axis=0, return_inverse=True)
    out = np.empty(len(pairs), np.float32)
    for i, (a, b) in enumerate(pairs.tolist()):
        v = _ROUND_CACHE.get((a, b))
        if v is None:
            v = _ROUND_CACHE[(a, b)] = round_f32(a, b)
        out[i] = v
    return out[inverse.ravel()].reshape(n.shape)


def exact_rasterize(scene, closed=True, tie='lower'):
    """-> dict(face_id [H,W] int32, zbuf [H,W] f32, bary [H,W,3] f32, n_cover [H,W] int32: the valid faces whose closed triangle contains the
    centre; on_edge, on_vertex: the pixels whose centre lies exactly on an edge / on a vertex of a valid face; n_valid).
    closed=False and tie='higher' are the two deliberately WRONG variants of the rules (open edges; the higher id on a depth tie)."""
    valid, w, s, qi, q = _evaluate(scene)
    H, W = scene.H, scene.W
    pos = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)
    neg = (w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0)
    cover = ((s > 0) & pos) | ((s < 0) & neg)                   # rule 2, closed: (s == 0 with a non-zero area happens nowhere inside)
    zeros = (w[0] == 0).astype(np.int32) + (w[1] == 0) + (w[2] == 0)
    on_edge, on_vertex = (cover & (zeros >= 1)).any(0), (cover & (zeros >= 2)).any(0)
    n_cover = cover.sum(0).astype(np.int32)
    if not closed:
        cover = cover & (zeros == 0)
    out = dict(face_id=np.full(H * W, -1, np.int32), zbuf=np.full(H * W, np.inf, np.float32), bary=np.zeros((H * W, 3), np.float32))
    if cover.any():
        assert np.all(((s > 0) == (q > 0))[cover]) and np.all(q[cover] != 0)
        fi, pi = np.nonzero(cover)
        num, den = np.abs(4 * s[fi, pi]), np.abs(q[fi, pi])                  # depth = s / (q / 4)
        z32 = np.full(cover.shape, np.inf, np.float32)
        z32[fi, pi] = _round_array(num, den)
        # a depth comparison is an exact tie or a clear win: unequal rationals of such short integers are unequal float64s too
        z64 = np.full(cover.shape, np.inf)
        z64[fi, pi] = num / den
        zs = np.sort(z64, 0)
        with np.errstate(invalid='ignore'):
            gap = zs[1:] - zs[:-1]
            close = np.isfinite(zs[1:]) & (gap > 0) & (gap < CLEAR_WIN * zs[:-1])
        _need(not close.any(), scene, "two faces cover a pixel with unequal depths closer than 2^-20 relative")
        k = np.argmin(z32, 0) if tie == 'lower' else len(z32) - 1 - np.argmin(z32[::-1], 0)     # the first / the last of equal minima
        p = np.flatnonzero(cover.any(0))
        k = k[p]
        out['face_id'][p] = valid[k]
        out['zbuf'][p] = z32[k, p]
        for c in range(3):
            out['bary'][p, c] = _round_array(np.abs(qi[c][k, p]), np.abs(q[k, p]))
        assert np.all(np.isfinite(out['zbuf'][p])) and np.all(out['zbuf'][p] >= 2.0 ** -100)
    return dict(face_id=out['face_id'].reshape(H, W), zbuf=out['zbuf'].reshape(H, W), bary=out['bary'].reshape(H, W, 3), n_cover=n_cover.reshape(H, W),
                on_edge=int(on_edge.sum()), on_vertex=int(on_vertex.sum()), n_valid=int(len(valid)))


def check(scene):
    """the preconditions alone: LatticeError unless the scene is on the lattice, every float32 intermediate is exact and every depth
    comparison is a tie or a clear win"""
    exact_rasterize(scene)


def wrong_rule_pixels(scene):
    """(the pixels whose winner changes with open edges, with the higher id on a tie)"""
    right = exact_rasterize(scene)['face_id']
    return (int((exact_rasterize(scene, closed=False)['face_id'] != right).sum()), int((exact_rasterize(scene, tie='higher')['face_id'] != right).sum()))


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------
FX, FY = 32.0, 16.0                                            # unequal, so that a swapped axis shows


def _build(name, tris, W, H, t=(0, 0, 0), extra_verts=(), extra_faces=(), **kw):
    """tris: triangles as three (u, v, z) screen corners, each with vertices of its own (a shared edge is shared by coordinates, not by
    index, so every face has a depth of its own); extra_verts are camera-space (x, y, z), extra_faces index the final vertex list and come
    FIRST in the face list.  The world position of a corner is what projects to it: exact in float32, which `check` re-derives"""
    cx, cy = Fraction(W) / 2, Fraction(H) / 2
    verts, faces = [], []
    for tri in tris:
        faces.append([len(verts), len(verts) + 1, len(verts) + 2])
        for u, v, z in tri:
            verts.append([(Fraction(u) - cx) * z / Fraction(FX) - t[0], (Fraction(v) - cy) * z / Fraction(FY) - t[1], Fraction(z) - t[2]])
    n = len(verts)
    verts += [[Fraction(x) - t[0], Fraction(y) - t[1], Fraction(z) - t[2]] for x, y, z in extra_verts]
    faces = [[i if i >= 0 else n + ~i for i in f] for f in extra_faces] + faces          # ~k names extra vertex k
    v32 = np.array([[float(c) for c in v] for v in verts], np.float32)
    assert all(Fraction(float(a)) == b for row, frow in zip(v32, verts) for a, b in zip(row, frow)), name
    return Scene(name, v32, faces, W, H, FX, FY, float(cx), float(cy), t, **kw)


def _flip(tri, on):
    return (tri[0], tri[2], tri[1]) if on else tri


def diagonal(order, winding, depths, W=32, H=24, box=None):
    """a square with integer corners split along the diagonal that runs through pixel centres.  depths: (z of the upper-right half, z of the
    lower-left half); order 1 lists the lower-left half first; winding 1 reverses both faces"""
    x0, y0, x1, y1 = box or (2, 3, 18, 19)
    assert x1 - x0 == y1 - y0
    upper = ((x0, y0, depths[0]), (x1, y0, depths[0]), (x1, y1, depths[0]))
    lower = ((x0, y0, depths[1]), (x1, y1, depths[1]), (x0, y1, depths[1]))
    tris = [_flip(upper, winding), _flip(lower, winding)][::-1 if order else 1]
    on = sum(1 for k in range(x1 - x0) if 0 <= x0 + k < W and 0 <= y0 + k < H)           # the diagonal's centres inside the image
    tie = depths[0] == depths[1]
    return _build(f"diagonal-o{order}w{winding}z{depths[0]}{depths[1]}-{W}x{H}", tris, W, H, t=(0, 0, 3), min_edge=on, min_open=on, min_tie=on if tie else 0,
                  id_dependent=tie, pins='closed shared edge; lower id on the diagonal' if tie else 'closed shared edge; depth before id')


def fan(hub, near=None):
    """eight triangles around a hub that is a pixel centre, their outer corners pixel centres too, windings alternating; all at depth 2, or
    face `near` at depth 1"""
    ring = [(6, 0), (6, 6), (0, 6), (-6, 6), (-6, 0), (-6, -6), (0, -6), (6, -6)]
    tris = []
    for k in range(8):
        z = 1 if k == near else 2
        a, b = ring[k], ring[(k + 1) % 8]
        tris.append(_flip(((hub, hub, z), (hub + a[0], hub + a[1], z), (hub + b[0], hub + b[1], z)), k & 1))
    # on an edge: 8 spokes of 5 inner centres each, the hub, 8 outer corners, 8 outer edges of 5 inner centres each; ties: the spokes, the hub
    # and the outer corners (a nearer face takes its two spokes, its two corners and the hub out of them)
    return _build(f"fan-hub{hub}-" + ("flat" if near is None else f"near{near}"), tris, 32, 32, min_edge=89, min_vertex=9, min_open=89,
                  min_tie=49 if near is None else 36, id_dependent=True, pins='a vertex centre belongs to the whole fan; lower id on spokes and hub')


def seams(axis, side, W=40, H=48, pitch=5):
    """axis-aligned right triangles whose largest (side 'max') or smallest ('min') coordinate on `axis` is exactly each seam value; pitch 0
    stacks them on one another (tiny frames), at depths 1, 2, 4 in turn"""
    D = W if axis == 'x' else H
    values = list(collections.OrderedDict.fromkeys([-0.5, 0, 0.5, 15.5, 16, 16.5, D - 0.5, D, D + 0.5]))
    tris, E, other = [], 0, H if axis == 'x' else W
    for i, e in enumerate(values):
        o = 1 + pitch * i if pitch else -2                     # along the other axis
        if e % 1 == 0.5 and 0 < e < D:                         # the leg at e runs through the centres of an image column (row): count them
            E += sum(1 for r in range(other) if o <= r + 0.5 <= o + 4)
        z = (1, 2, 4)[i % 3] if not pitch else (4, 2, 1)[i % 3]
        far = e - 4 if side == 'max' else e + 4
        tri = ((far, o), (e, o), (e, o + 4))                   # the leg at e spans four centres of the other axis when e is a half
        tri = tuple((a, b, z) if axis == 'x' else (b, a, z) for a, b in tri)
        tris.append(_flip(tri, i & 1))
    return _build(f"seams-{axis}{side}-{W}x{H}", tris, W, H, t=(0, 0, -1), id_dependent=not pitch, min_edge=E, min_vertex=0,
                  min_open=E if pitch else 0,      # (stacked, another face may hold an edge pixel: n_cover carries the check there)
                  pins="tile_box's floors, clip and off-image rejection")


def slivers():
    """a face the size of the image behind triangles narrower than half a pixel: with no centre inside, and with exactly one (inside, on an
    edge, on a vertex)"""
    tris = [((-1, -1, 4), (80, -1, 4), (-1, 60, 4)),                                        # the backdrop
            ((4, 7.75, 2), (12, 8, 2), (4, 8.25, 2)),                                       # between rows 7 and 8, eight columns long: no centre
            ((15.75, 2, 1), (16.25, 2, 1), (16, 10, 1)),                                    # between columns 15 and 16, on the tile seam: none
            ((8, 12, 2), (8.25, 12, 2), (8, 12.25, 2)),                                     # a quarter-pixel corner: none
            ((20.25, 15.75, 1), (20.75, 15.75, 1), (20.5, 16.25, 1)),                       # straddles the seam between rows 15 and 16: none
            ((4.25, 10.25, 2), (4.75, 10.5, 2), (4.25, 10.75, 2)),                          # (4.5, 10.5) strictly inside
            ((6.25, 12.5, 1), (6.75, 12.5, 1), (6.5, 12.75, 1)),                            # (6.5, 12.5) on its edge
            ((4.5, 12.5, 2), (4.75, 12.75, 2), (4.25, 12.75, 2)),                           # (4.5, 12.5) is its vertex
            ((15.5, 15.5, 1), (15.75, 15.25, 1), (15.25, 15.25, 1)),                        # the last centre of tile 0 is its vertex
            ((16.25, 16.25, 2), (16.75, 16.5, 2), (16.25, 16.75, 2))]                       # the first centre of the diagonal neighbour, inside
    return _build("slivers", [_flip(t, i & 1) for i, t in enumerate(tris)], 32, 24, min_edge=3, min_vertex=2, min_open=3,
                  pins='sub-pixel faces: no centre, no pixel; one centre, one pixel')


def rejected(with_bad=True):
    """a backdrop at depth 4 and, listed before it and nearer, faces that rule 2 drops: collinear, a repeated index, a vertex at z == 0, a
    vertex at z < 0.  with_bad=False: the backdrop and a valid near triangle alone"""
    tris = [((-1, -1, 4), (80, -1, 4), (-1, 60, 4)), ((20.5, 3.5, 2), (28.5, 3.5, 2), (20.5, 11.5, 2))]
    if with_bad:
        tris = [((2, 2, 1), (10, 10, 1), (20, 20, 1)),                                       # collinear on the screen, at three different places
                ((3, 20, 1), (9, 20, 2), (15, 20, 4))] + tris                               # collinear, depths 1, 2, 4
        extra_verts = [(-0.25, -0.5, 1), (0.25, -0.5, 1), (0, 0.5, 1), (0, 0.5, 0), (0, 0.5, -1)]     # a near triangle's corners; its apex at z = 0 and behind
        extra_faces = [[~0, ~1, ~0], [~0, ~1, ~3], [~0, ~1, ~4], [~4, ~3, ~1]]
    else:
        extra_verts, extra_faces = [], []
    return _build("rejected" if with_bad else "rejected-without", tris, 32, 24, t=(0, 0, 0), extra_verts=extra_verts, extra_faces=extra_faces,
                  min_edge=24, min_vertex=3, min_open=24, pins='zero area and z <= 0 never appear, never count')


def perspective(order):
    """two interpenetrating triangles with corners at depths 1, 2 and 4: depth and barycentrics are non-trivial quotients, and the winner
    changes along the line where the two planes meet"""
    tris = [((2.25, 2.5, 1), (30.5, 4.25, 4), (6.5, 22.5, 2)), ((4.5, 3.25, 4), (28.25, 2.5, 1), (10.5, 21.75, 2))]
    return _build(f"perspective-o{order}", tris[::-1 if order else 1], 32, 24, t=(1, -2, 0), min_edge=2, min_vertex=1, min_open=1, pins='s / q and (w_i / z_i) / q rounded once')


def stack(N, near=None):
    """N triangles of one projection inside tile (1, 0) of a 32 x 16 image, corners on pixel centres: all at depth 2, or face `near` at depth 1"""
    tris = [_flip(((17.5, 1.5, 1 if k == near else 2), (30.5, 1.5, 1 if k == near else 2), (17.5, 14.5, 1 if k == near else 2)), k & 1) for k in range(N)]
    return _build(f"stack-{N}-" + ("flat" if near is None else f"near{near}"), tris, 32, 16, min_edge=39, min_vertex=3, min_open=39,
                  min_tie=105 if near is None else 0, id_dependent=True, pins='the (z, id) minimum across LDS batches of 256 faces')


TINY = ((1, 1), (16, 16), (17, 15), (33, 1))


def _scenes():
    out = []
    for order in (0, 1):
        for winding in (0, 1):
            out.append(diagonal(order, winding, (2, 2)))
    out += [diagonal(0, 0, (4, 2)), diagonal(1, 1, (2, 4)), diagonal(0, 1, (1, 4))]      # the far half first (twice), the near half first
    for hub in (15.5, 16.5):
        out.append(fan(hub))
        out += [fan(hub, k) for k in range(8)]
    out += [seams(axis, side, *((40, 48) if axis == 'x' else (48, 40))) for axis in 'xy' for side in ('max', 'min')]
    out += [slivers(), rejected(), rejected(False), perspective(0), perspective(1)]
    for N in (255, 256, 257, 512, 513):
        out.append(stack(N))
        out += [stack(N, k) for k in sorted({0, 255, 256, N - 1}) if k < N]
    for W, H in TINY:
        n = max(W, H)
        out.append(diagonal(0, 0, (2, 2), W, H, box=(-2, -2, n + 2, n + 2)))
        out.append(diagonal(1, 1, (4, 2), W, H, box=(-2, -2, n + 2, n + 2)))
        out += [seams(axis, side, W, H, pitch=0) for axis in 'xy' for side in ('max', 'min')]
    names = [s.name for s in out]
    assert len(set(names)) == len(names), names
    return collections.OrderedDict((s.name, s) for s in out)


SCENES = _scenes()
_EXACT = {}


def exact_of(name):
    """exact_rasterize of a scene of SCENES: computed once, shared, never written to"""
    if name not in _EXACT:
        r = exact_rasterize(SCENES[name])
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _EXACT[name] = r
    return _EXACT[name]
