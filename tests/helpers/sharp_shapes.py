"""Non-convex, sharp-edged meshes for the mesh kernels, their queries and the float64 truth of every query -- numpy only, no device.

synthetic.capsule_mesh, the only mesh the other suites feed to nm_signed_distance, is convex and smooth: whichever of the seven vectors of the
winning face (include/neuman_hip.h: face normal | three edge pseudonormals | three vertex pseudonormals) the kernel reads, (p - q) . n has the
same sign there, so a wrong slot, a wrong corner or an edge sum that missed a face cannot show.  The shapes below have acute convex tips, reflex
notches, sharp rims, a hole, an open boundary and an edge with three faces; tests/test_sharp_shapes_host.py proves on the CPU that on them every
wrong slot does flip signs, tests/test_hip_sharp_shapes.py holds the device to the truth computed here.

Shapes are of unit scale, closed (unless said otherwise) and outward oriented.  The star prism's coordinates are multiples of 2^-10, so the
midpoints of three rounds of subdivision are exact in float32: `star_prism_fine` is the same solid as `star_prism`, to the bit.

The truth of a query (`truth`): brute force over all faces in float64 -- distance, closest point, the faces within `FACE_TOL` of the minimum,
the winner (lowest face id among exact ties), the Voronoi region of the query in the winner (the region conditions of Ericson, RTCD 5.1.5, in
the priority of oracle/warp.py's closest_point_on_triangles: the `bary > 1e-9` feature test of oracle.warp.signed_distance is too coarse for a
slab 1e-3 thick), the pseudonormal of that region from oracle.warp.pseudonormals, and the sign by the header's rule: (p - q) . n < 0 negative,
a zero dot positive.  Independent of all mesh code: `inside` (point in the star polygon, |z| < h) where the solid has a formula; independent
of the closest-point code: oracle.warp.winding_number."""
import os
import sys

import numpy as np

_ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
for _p in (_ROOT, os.path.join(_ROOT, "ml-neuman_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import warp as OW  # noqa: E402

N_QUERY = 3000
SEED = 11
NEAR = 0.05                    # near-feature queries lie within this of a tip, a notch, a rim or a vertex
MIN_DIST = 1e-5                # tests/test_hip_render.py::test_signed_distance's rule: closer than this a point has no defined side
MIN_COS = 1e-3                 # |(p - q) . n| below this times |p - q| |n|: float32 may legitimately land on the other side
FACE_TOL = 2e-6                # test_signed_distance's distance tolerance: a face this close to the minimum is a valid answer
MAX_EXCLUDED = 0.01
MIN_FLIPS = 20
SLOTS = ("face normal", "edge v0v1", "edge v1v2", "edge v2v0", "vertex v0", "vertex v1", "vertex v2")

STAR_R_OUT, STAR_R_IN, STAR_H = 0.5, 0.2, 0.3125
PLATE_H = 5e-4
TORUS_R, TORUS_r = 0.45, 0.18

STAR_CAMERA = (30., -20., 2.6)                     # synthetic.spherical_c2w: oblique, through two arms of the star
TORUS_CAMERA = (40., 12., 1.8)                     # nearly in the ring's plane: the far side of the tube shows through the hole
TORUS_HOLE_CAMERAS = ((30., 55., 1.9), (-70., 40., 2.1))    # the hole open to the viewer (the silhouette's two views)

CLOSED = ("star_prism", "star_prism_fine", "star_prism_swapped", "torus", "thin_plate")
SHARP = ("star_prism", "star_prism_fine", "star_prism_swapped", "thin_plate")
UNSIGNED = ("star_prism_open", "star_prism_fin")   # no inside: the truth is the rule alone


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
def _star_ring(r_even, r_odd, n=5):
    ang = np.pi / 2 + np.arange(2 * n) * np.pi / n
    r = np.where(np.arange(2 * n) % 2 == 0, r_even, r_odd)
    return np.round(np.stack([r * np.cos(ang), r * np.sin(ang)], 1) * 1024.0) / 1024.0             # counter-clockwise seen from +z


def _prism(ring, h):
    """ring [n,2] counter-clockwise, star-shaped about the origin -> verts [2n+2,3] (bottom ring, top ring, bottom centre, top centre),
    faces [4n,3]: sides first, then the bottom fan, then the top fan"""
    n = len(ring)
    verts = np.concatenate([np.c_[ring, np.full(n, -h)], np.c_[ring, np.full(n, h)], [[0, 0, -h]], [[0, 0, h]]])
    faces = []
    for i in range(n):
        j = (i + 1) % n
        faces += [[i, j, n + j], [i, n + j, n + i]]
    faces += [[2 * n, (i + 1) % n, i] for i in range(n)]
    faces += [[2 * n + 1, n + i, n + (i + 1) % n] for i in range(n)]
    return verts.astype(np.float32), np.asarray(faces, np.int64)


def subdivide(verts, faces, rounds):
    """midpoint subdivision: every face into four, in place of its parent (children of face f are 4f .. 4f+3)"""
    v = [tuple(x) for x in np.asarray(verts, np.float64)]
    for _ in range(rounds):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(v)
                v.append(tuple((np.asarray(v[a]) + np.asarray(v[b])) / 2))
            return mid[key]
        for a, b, c in np.asarray(faces):
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
        faces = np.asarray(out, np.int64)
    v64 = np.asarray(v, np.float64)
    assert np.array_equal(v64.astype(np.float32).astype(np.float64), v64)                          # the midpoints are exact in float32
    return v64.astype(np.float32), faces


def _torus(n_major=32, n_minor=16, R=TORUS_R, r=TORUS_r):
    u = np.arange(n_major) * 2 * np.pi / n_major
    w = np.arange(n_minor) * 2 * np.pi / n_minor
    U, W = np.meshgrid(u, w, indexing='ij')
    verts = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % n_major) * n_minor + (j % n_minor)                                      # noqa: E731
    faces = []
    for i in range(n_major):
        for j in range(n_minor):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [[a, b, c], [a, c, d]]
    return verts.astype(np.float32), np.asarray(faces, np.int64)


_SHAPES = {}


def shape(name):
    """-> dict(verts float32 [V,3], faces int64 [F,3], closed, ring (the star's outline [10,2] float64, or None), h, features [K,3]: the points
    the near-feature queries gather around).  Built once, read-only."""
    if name in _SHAPES:
        return _SHAPES[name]
    ring, h = None, None
    if name in ("star_prism", "star_prism_fine", "star_prism_swapped", "star_prism_open", "star_prism_fin", "thin_plate"):
        swapped = name == "star_prism_swapped"
        ring = _star_ring(STAR_R_IN if swapped else STAR_R_OUT, STAR_R_OUT if swapped else STAR_R_IN)
        h = PLATE_H if name == "thin_plate" else STAR_H
        verts, faces = _prism(ring, h)
        h = float(verts[-1, 2])
        coarse = verts.astype(np.float64)
        if name in ("star_prism_fine", "star_prism_swapped", "star_prism_open"):
            verts, faces = subdivide(verts, faces, 3)
        if name == "star_prism_open":                                                               # the top cap removed: its rim is a boundary
            faces = faces[~(verts[faces][:, :, 2] == np.float32(h)).all(1)]
        if name == "star_prism_fin":                                                                # a third face on the vertical edge of notch 1,
            notch = coarse[1, :2]                                                                   # reaching out of the solid: feet from inside land there
            verts = np.concatenate([verts, [[notch[0] * 1.5, notch[1] * 1.5, 0.0]]]).astype(np.float32)
            faces = np.concatenate([faces, [[1, len(ring) + 1, len(verts) - 1]]])
        # tips and notches at both caps and mid-height, rim midpoints
        k = len(ring)
        rim_mid = (coarse[:k] + np.roll(coarse[:k], -1, 0)) / 2
        features = np.concatenate([coarse[:2 * k], (coarse[:k] + coarse[k:2 * k]) / 2, rim_mid, rim_mid * [1, 1, -1]])
        if name == "star_prism_fin":
            inward = np.stack([np.r_[coarse[1, :2] * 0.92, z] for z in np.linspace(-0.25, 0.25, 6)])        # inside, nearest to the notch's edge
            features = np.concatenate([features, verts[-1:].astype(np.float64), (verts[-1:] + coarse[1:2]) / 2, inward])
    elif name == "torus":
        verts, faces = _torus()
        features = verts.astype(np.float64)
    else:
        raise KeyError(name)
    # a seeded order of the faces and a seeded first corner of each (the orientation stays): the builders above put the same corner of every
    # face on the sharp features and the same face first at every tie, which would leave some of the seven slots unread
    rng = np.random.default_rng([SEED, 99])
    faces = np.asarray(faces)[rng.permutation(len(faces))]
    faces = faces[np.arange(len(faces))[:, None], (np.arange(3)[None] + rng.integers(0, 3, (len(faces), 1))) % 3]
    verts = np.ascontiguousarray(verts, np.float32)
    faces = np.ascontiguousarray(faces, np.int64)
    for a in (verts, faces, features):
        a.setflags(write=False)
    _SHAPES[name] = dict(name=name, verts=verts, faces=faces, closed=name not in UNSIGNED, ring=ring, h=h, features=features)
    return _SHAPES[name]


def reversed_faces(faces):
    """every face with the opposite orientation, in the same place of the list and from the same first corner"""
    return np.ascontiguousarray(np.asarray(faces)[:, [0, 2, 1]])


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    return float(np.einsum('ij,ij->i', v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---- queries -----------------------------------------------------------------------------------------------------------------------
def _ball(rng, n, radius):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3))


_QUERIES = {}


def queries(name, n=N_QUERY):
    """about n float32 points from a fixed seed: uniform in the box 1.3 times the shape's, a share within NEAR of the features (tips, notches,
    rims; mesh vertices), and for the thin plate a share within 2e-3 of the mid-plane.  The shares are chosen so that every wrong slot flips
    at least MIN_FLIPS signs on every sharp shape (tests/test_sharp_shapes_host.py asserts it)."""
    key = (name, n)
    if key in _QUERIES:
        return _QUERIES[key]
    s = shape(name)
    rng = np.random.default_rng([SEED, sorted(_ALL).index(name)])
    v = s['verts'].astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    c, e = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.05)
    n_feat = n // 2 if name != "torus" else n // 4
    n_vert = n // 8
    n_plane = n // 4 if name == "thin_plate" else 0
    n_uni = n - n_feat - n_vert - n_plane
    parts = [c + rng.uniform(-1.3, 1.3, (n_uni, 3)) * e]
    f = s['features']
    parts.append(f[rng.integers(0, len(f), n_feat)] + _ball(rng, n_feat, NEAR))
    parts.append(v[rng.integers(0, len(v), n_vert)] + _ball(rng, n_vert, NEAR))
    if n_plane:
        parts.append(np.c_[c[:2] + rng.uniform(-1.3, 1.3, (n_plane, 2)) * e[:2], rng.uniform(-2e-3, 2e-3, n_plane)])
    pts = np.ascontiguousarray(np.concatenate(parts).astype(np.float32))
    pts.setflags(write=False)
    _QUERIES[key] = pts
    return pts


_ALL = CLOSED + UNSIGNED


def capsule_queries(case):
    """the mesh and the first 400 queries of tests/test_hip_render.py::test_signed_distance (the ones it holds to the oracle), restated"""
    from neuman_hip import synthetic
    rng = np.random.default_rng(3)
    verts_c, faces = synthetic.capsule_mesh() if case == "smpl_size" else synthetic.capsule_mesh(n_rings=10, n_seg=12)
    posed, _ = synthetic.twist_transforms(np.asarray(verts_c, np.float32))
    faces = np.ascontiguousarray(np.asarray(faces)[:, :3], np.int64)
    n = 600 if case == "smpl_size" else 3000
    pts = (posed[rng.integers(0, len(posed), n)] + rng.normal(size=(n, 3)) * rng.choice([0.003, 0.03, 0.2], size=(n, 1))).astype(np.float32)
    return posed, faces, pts[:400]


# ---- truth -------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return np.sum(a * b, axis=-1)


def regions(p, a, b, c):
    """the Voronoi region of p in triangle (a, b, c): 0 face, 1 / 2 / 3 edge v0v1 / v1v2 / v2v0, 4 / 5 / 6 vertex v0 / v1 / v2 -- the conditions
    and the priority of oracle.warp.closest_point_on_triangles (vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, face)"""
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    return np.select(conds, [4, 5, 1, 6, 3, 2], default=0)


def slot_table(verts, faces):
    """the seven vectors per face in the kernel's layout [F,7,3], float64, from oracle.warp.pseudonormals (an edge sums the unit normals of
    EVERY face on it: one on a boundary, three on the fin's edge)"""
    fn, vn, en = OW.pseudonormals(verts, faces)
    return np.concatenate([fn[:, None], en, vn[np.asarray(faces)[:, :3]]], 1)


def point_in_polygon(xy, ring):
    """even-odd rule, float64"""
    x, y = xy[:, 0:1], xy[:, 1:2]
    x0, y0 = ring[:, 0][None], ring[:, 1][None]
    x1, y1 = np.roll(ring[:, 0], -1)[None], np.roll(ring[:, 1], -1)[None]
    with np.errstate(divide='ignore', invalid='ignore'):
        cross = ((y0 > y) != (y1 > y)) & (x < (x1 - x0) * (y - y0) / (y1 - y0) + x0)
    return (cross.sum(1) % 2) == 1


def closest_faces(verts, faces, pts, chunk=256):
    """float64 brute force -> (distance [N], winner [N] (lowest face id among exact ties), closest point [N,3], near [N,F] bool: the faces
    within FACE_TOL of the minimum)"""
    p = np.asarray(pts, np.float64)
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)[:, :3]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    N = p.shape[0]
    dist, win, closest, near = np.empty(N), np.empty(N, np.int64), np.empty((N, 3)), np.zeros((N, f.shape[0]), bool)
    # only the faces that can come within FACE_TOL of the minimum are evaluated: with d_ub the distance to the nearest mesh vertex (a point of
    # the surface) a face whose centroid is further than d_ub + FACE_TOL + (its radius about the centroid) cannot -- exact, not approximate
    cen = (a + b + c) / 3.0
    rad = np.sqrt(np.maximum(np.maximum(_dot(a - cen, a - cen), _dot(b - cen, b - cen)), _dot(c - cen, c - cen)))
    used = v[np.unique(f)]
    for s in range(0, N, chunk):
        ps = p[s:s + chunk]
        d_ub = np.sqrt(((ps[:, None] - used[None]) ** 2).sum(-1)).min(1)
        dc = np.sqrt(((ps[:, None] - cen[None]) ** 2).sum(-1))
        pi, fi = np.nonzero(dc <= (d_ub[:, None] + rad[None]) * (1 + 1e-9) + FACE_TOL + 1e-9)     # row-major: by point, then by face id
        q = OW.closest_point_on_triangles(ps[pi], a[fi], b[fi], c[fi])
        d = np.sqrt(_dot(q - ps[pi], q - ps[pi]))
        start = np.flatnonzero(np.r_[True, pi[1:] != pi[:-1]])
        assert len(start) == len(ps)
        dmin = np.minimum.reduceat(d, start)
        tie = d <= dmin[pi] + 1e-13                                                                 # exact ties: the lowest face id
        i = np.minimum.reduceat(np.where(tie, np.arange(len(d)), len(d)), start)
        dist[s:s + chunk], win[s:s + chunk], closest[s:s + chunk] = d[i], fi[i], q[i]
        ok = d <= dmin[pi] + FACE_TOL
        near[s + pi[ok], fi[ok]] = True
    return dist, win, closest, near


def truth(verts, faces, pts, ring=None, h=None, closed=True):
    """-> dict: dist, closest, face (the winner), near [N,F] bool (faces within FACE_TOL of the minimum), region, normal (the correct vector),
    sign (+1 / -1), excluded, slot_sign [7,N] (the sign with slot k of the winner in place of the correct vector), and for a closed shape
    winding [N] and, with a ring, inside [N]"""
    p = np.asarray(pts, np.float64)
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)[:, :3]
    N = p.shape[0]
    dist, win, closest, near = closest_faces(verts, faces, pts)
    tri = v[f[win]]
    region = regions(p, tri[:, 0], tri[:, 1], tri[:, 2])
    table = slot_table(verts, f)
    slots = table[win]                                                                              # [N,7,3]
    normal = slots[np.arange(N), region]
    d = p - closest

    def rule(n):
        return np.where(_dot(d, n) < 0, -1.0, 1.0)
    cos = np.abs(_dot(d, normal)) / np.maximum(np.linalg.norm(d, axis=1) * np.linalg.norm(normal, axis=1), 1e-300)
    out = dict(dist=dist, closest=closest, face=win, near=near, region=region, normal=normal, sign=rule(normal),
               excluded=(dist < MIN_DIST) | (cos < MIN_COS), slot_sign=np.stack([rule(slots[:, k]) for k in range(7)]), table=table)
    if closed:
        out['winding'] = OW.winding_number(p, verts, f)
        if ring is not None:
            out['inside'] = point_in_polygon(p[:, :2], np.asarray(ring, np.float64)) & (np.abs(p[:, 2]) < h)
    for x in out.values():
        x.setflags(write=False)
    return out


_TRUTH = {}


def shape_truth(name):
    """(shape, queries, truth) of one shape: computed once, shared, never written to"""
    if name not in _TRUTH:
        s = shape(name)
        q = queries(name)
        _TRUTH[name] = (s, q, truth(s['verts'], s['faces'], q, s['ring'], s['h'], s['closed']))
    return _TRUTH[name]


def flips(t):
    """per slot: the non-excluded queries whose sign changes when that slot of the winning face stands in for the correct vector"""
    ok = ~t['excluded']
    return [int(((t['slot_sign'][k] != t['sign']) & ok).sum()) for k in range(7)]


# ---- depth complexity ----------------------------------------------------------------------------------------------------------------
def capture(camera, W, H):
    from neuman_hip import synthetic
    return synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(*camera))


def coverage(verts, faces, camera):
    """how many faces cover each pixel centre, by the rasteriser's rules 1-2 in float64 (tests/helpers/raster_ref.py's projection and inside test,
    every face at every pixel) -> int [H,W]"""
    w2c, fx, fy, cx, cy, W, H = camera
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces)[:, :3]
    R, t = np.asarray(w2c)[:, :3], np.asarray(w2c)[:, 3]
    cam = v @ R.T + t
    sx, sy = fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy
    X, Y, Z = sx[f], sy[f], cam[:, 2][f]
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    valid = (Z > 0).all(1) & (area != 0)
    px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    px, py = px.reshape(-1, 1), py.reshape(-1, 1)
    count = np.zeros(H * W, np.int64)
    for s in range(0, len(f), 256):
        x, y = X[s:s + 256][None], Y[s:s + 256][None]
        ax, ay, bx, by, cx_, cy_ = x[..., 0] - px, y[..., 0] - py, x[..., 1] - px, y[..., 1] - py, x[..., 2] - px, y[..., 2] - py
        w0, w1, w2 = bx * cy_ - by * cx_, cx_ * ay - cy_ * ax, ax * by - ay * bx
        sm = (w0 + w1) + w2
        inside = ((sm > 0) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((sm < 0) & (w0 <= 0) & (w1 <= 0) & (w2 <= 0))
        count += (inside & valid[s:s + 256][None]).sum(1)
    return count.reshape(H, W)
