"""Numpy restatement of the 'mesh simplify' contract of include/neuman_hip.h (rules Q1-Q9): the cells, the clusters, the members' means, the
quadric placement and the surviving faces, in float64 elementwise operations in the stated association with one astype(np.float32) at the end.
numpy's float64 add, subtract, multiply, divide and floor are IEEE operations rounded one by one, which is what the device does with
contraction off.

Nothing here follows the kernels' method (flags, scans, an atomic cursor and a sort, a table of face indices): the clusters are np.unique of
the candidates' cells, the sums run through np.add.at, which applies its entries one after the other in the order given -- ascending vertex,
then list order, the left-to-right sums of rules Q5 and Q6 without a Python loop over clusters -- and the duplicates are np.unique over the
rotated triples, whose first occurrence is the lowest face."""
import math

import numpy as np

import mesh_smooth_ref as SR

PLACEMENTS = {'mean': 0, 'quadric': 1}


def grid(aabb, cell):
    """neuman_hip.mesh_simplify's grid over aabb = (lo xyz, hi xyz) with cell edge `cell` -> (lo float32 [3], h float32, dims): both rounded to
    float32 once, dims = max(1, ceil(extent / h)) per axis in float64"""
    box = np.asarray(aabb, np.float32).reshape(6)
    h = np.float32(cell)
    dims = tuple(max(1, int(math.ceil((float(box[3 + a]) - float(box[a])) / float(h)))) for a in range(3))
    return box[:3].copy(), h, dims


def cells(verts, lo, h, dims):
    """Q2 -> (linear cell index int64 [V], -1 for a vertex that is not finite; per-axis cell int64 [V,3])"""
    x = np.asarray(verts)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == 3
    finite = np.isfinite(x).all(1)
    with np.errstate(all='ignore'):
        t = np.floor((x.astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)[None]) / np.float64(np.float32(h)))
    t = np.where(finite[:, None], t, 0.0)
    c = np.clip(t, 0.0, np.asarray(dims, np.float64)[None] - 1.0).astype(np.int64)
    linear = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    return np.where(finite, linear, -1), c


def candidates(faces, vcell):
    """Q3 -> bool [F]: valid (checked by the caller), proper, three finite vertices in three pairwise distinct cells"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = vcell[f]
    return SR.proper(f) & (c >= 0).all(1) & (c[:, 0] != c[:, 1]) & (c[:, 0] != c[:, 2]) & (c[:, 1] != c[:, 2])


def clusters(verts, faces, lo, h, dims):
    """Q1-Q3 -> (vert_cluster int32 [V], used cells int64 [K] ascending, candidate mask [F]); ValueError on an invalid face"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = np.asarray(verts).shape[0]
    bad = SR.invalid_faces(f, V)
    if bad.size:
        raise ValueError(f"{bad.size} invalid faces, the first of them face {bad[0]}")
    vcell, _ = cells(verts, lo, h, dims)
    cand = candidates(f, vcell)
    used = np.unique(vcell[f[cand]].reshape(-1))
    vc = np.full(V, -1, np.int64)
    if used.size:
        at = np.searchsorted(used, vcell)
        at = np.minimum(at, used.size - 1)
        hit = (vcell >= 0) & (used[at] == vcell)
        vc[hit] = at[hit]
    return vc.astype(np.int32), used, cand


def average_rows(rows, vert_cluster, K):
    """Q5 -> (float32 [K,w], the unrounded float64 means [K,w], member counts [K])"""
    x = np.asarray(rows)
    assert x.dtype == np.float32 and x.ndim == 2
    vc = np.asarray(vert_cluster, np.int64)
    members = np.flatnonzero(vc >= 0)                          # ascending vertex index: so is every cluster's subsequence
    s = np.zeros((K, x.shape[1]), np.float64)
    with np.errstate(all='ignore'):
        np.add.at(s, vc[members], x[members].astype(np.float64))
        count = np.bincount(vc[members], minlength=K)
        m = s / count.astype(np.float64)[:, None]
        return m.astype(np.float32), m, count


def quadric_points(verts, faces, vert_cluster, used, lo, h, dims, mean64):
    """Q6 -> (float64 [K,3] the placed points before the one rounding, fallback bool [K]: the cluster took its mean)"""
    x = np.asarray(verts).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    vc = np.asarray(vert_cluster, np.int64)
    K = used.shape[0]
    v, face, _, _ = SR.entries(f, x.shape[0])                  # sorted by (vertex, face): member ascending, then list order
    keep = vc[v] >= 0
    v, face = v[keep], face[keep]
    k = vc[v]
    g = f[face]                                                # STORED corners
    with np.errstate(all='ignore'):
        a = x[g[:, 0]]
        u, w = x[g[:, 1]] - a, x[g[:, 2]] - a
        n0 = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        n1 = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        n2 = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        e = a - mean64[k]
        t = (n0 * e[:, 0] + n1 * e[:, 1]) + n2 * e[:, 2]
        A = np.zeros((K, 6), np.float64)                       # 00 01 02 11 12 22
        b = np.zeros((K, 3), np.float64)
        np.add.at(A, k, np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2], 1))
        np.add.at(b, k, np.stack([n0 * t, n1 * t, n2 * t], 1))
        A00, A01, A02, A11, A12, A22 = (A[:, i] for i in range(6))
        reg = ((A00 + A11) + A22) * np.float64(2.0 ** -10)
        A00, A11, A22 = A00 + reg, A11 + reg, A22 + reg
        c00, c01, c02 = A11 * A22 - A12 * A12, A02 * A12 - A01 * A22, A01 * A12 - A02 * A11
        c11, c12, c22 = A00 * A22 - A02 * A02, A01 * A02 - A00 * A12, A00 * A11 - A01 * A01
        det = (A00 * c00 + A01 * c01) + A02 * c02
        y = np.stack([((c00 * b[:, 0] + c01 * b[:, 1]) + c02 * b[:, 2]) / det,
                      ((c01 * b[:, 0] + c11 * b[:, 1]) + c12 * b[:, 2]) / det,
                      ((c02 * b[:, 0] + c12 * b[:, 1]) + c22 * b[:, 2]) / det], 1)
        p = mean64 + y
        c3 = np.stack([used % dims[0], (used // dims[0]) % dims[1], used // (dims[0] * dims[1])], 1).astype(np.float64)
        lo64, h64 = np.asarray(lo, np.float32).astype(np.float64)[None], np.float64(np.float32(h))
        box_lo, box_hi = lo64 + c3 * h64, lo64 + (c3 + 1.0) * h64
        ok = np.isfinite(det) & (det > 0) & np.isfinite(p).all(1) & ((box_lo <= p) & (p <= box_hi)).all(1)
    return np.where(ok[:, None], p, mean64), ~ok


def rotate(triples):
    """Q7: every row rotated cyclically so that its smallest entry (the rows' entries are pairwise distinct) comes first"""
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    first = t.argmin(1)
    return t[np.arange(t.shape[0])[:, None], (first[:, None] + np.arange(3)[None]) % 3]


def simplify(verts, faces, lo, h, dims, placement='quadric'):
    """Q1-Q8 -> dict: vert_cluster int32 [V], K, verts float32 [K,3], faces int32 [F',3], face_src int32 [F'], and for the tests members [K]
    (member counts), fallback bool [K] (quadric: the cluster took its mean), n_candidates, cells int64 [K] (the clusters' linear cell index)"""
    assert placement in PLACEMENTS
    verts = np.asarray(verts)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    vc, used, cand = clusters(verts, f, lo, h, dims)
    K = int(used.shape[0])
    rounded, mean64, count = average_rows(verts, vc, K)
    fallback = np.ones(K, bool)
    if placement == 'quadric':
        p, fallback = quadric_points(verts, f, vc, used, lo, h, dims, mean64)
        with np.errstate(all='ignore'):
            rounded = p.astype(np.float32)
    idx = np.flatnonzero(cand)
    triples = rotate(vc.astype(np.int64)[f[idx]])
    if idx.size:
        _, first = np.unique(triples, axis=0, return_index=True)
        first = np.sort(first)
    else:
        first = np.zeros(0, np.int64)
    return dict(vert_cluster=vc, K=K, verts=rounded, faces=triples[first].astype(np.int32).reshape(-1, 3), face_src=idx[first].astype(np.int32),
                members=count, fallback=fallback, n_candidates=int(idx.size), cells=used)


# ---- measures of the property tests ---------------------------------------------------------------------------------------------------------
def opposite_pairs(faces):
    """how many unordered pairs of output faces name the same three clusters with opposite orientation"""
    t = rotate(faces)
    flipped = rotate(t[:, [0, 2, 1]])
    have = {tuple(r) for r in t.tolist()}
    return sum(tuple(r) in have for r in flipped.tolist()) // 2


def cell_boxes(cells_, lo, h, dims):
    """-> (lo [K,3], hi [K,3]) float64 of the cells' closed boxes, Q6's expression"""
    c3 = np.stack([cells_ % dims[0], (cells_ // dims[0]) % dims[1], cells_ // (dims[0] * dims[1])], 1).astype(np.float64)
    lo64, h64 = np.asarray(lo, np.float32).astype(np.float64)[None], np.float64(np.float32(h))
    return lo64 + c3 * h64, lo64 + (c3 + 1.0) * h64
