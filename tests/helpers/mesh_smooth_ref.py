"""Numpy restatement of the 'mesh smooth' contract of include/neuman_hip.h (rules S1-S5): the vertex -> incident faces lists, the boundary
flags, Taubin steps and face-derived vertex normals, in float64 elementwise operations in the stated association with one astype(np.float32)
at the end.  numpy's float64 add, subtract, multiply, divide and sqrt are IEEE operations rounded one by one, which is what the device does
with contraction off.

Nothing here follows the kernels' method (count, scan, atomic fill, per-vertex sort): the lists are one stable sort of the (vertex, face)
entries, and the sums run through np.add.at, which applies its entries one after the other in the order given -- the left-to-right sum of
rule S3 without a Python loop over vertices."""
import numpy as np


def invalid_faces(faces, n_verts):
    """S1 -> the indices of the faces that name a vertex outside [0, n_verts), ascending"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.flatnonzero(((f < 0) | (f >= n_verts)).any(1))


def proper(faces):
    """S1 -> bool [F]: three pairwise distinct indices"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])


def entries(faces, n_verts):
    """the (vertex, face, p, q) entries of the adjacency sorted by (vertex, face): (v, p, q) is the face rotated so that v comes first"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bad = invalid_faces(f, n_verts)
    if bad.size:
        raise ValueError(f"{bad.size} invalid faces, the first of them face {bad[0]}")
    idx = np.flatnonzero(proper(f))
    g = f[idx]
    v = np.concatenate([g[:, 0], g[:, 1], g[:, 2]])
    p = np.concatenate([g[:, 1], g[:, 2], g[:, 0]])
    q = np.concatenate([g[:, 2], g[:, 0], g[:, 1]])
    face = np.concatenate([idx, idx, idx])
    order = np.lexsort((face, v))
    return v[order], face[order], p[order], q[order]


def adjacency(faces, n_verts):
    """S2 -> (inc_off [V+1] int32, inc [n_incident] int32, boundary [V] uint8)"""
    v, face, p, q = entries(faces, n_verts)
    inc_off = np.zeros(n_verts + 1, np.int64)
    np.cumsum(np.bincount(v, minlength=n_verts), out=inc_off[1:])
    # an undirected edge {v, u} once per proper face that names both: v's side of it is (v, p) and (v, q)
    a = np.concatenate([v, v])
    b = np.concatenate([p, q])
    boundary = np.zeros(n_verts, np.uint8)
    if a.size:
        key = a * max(n_verts, 1) + b
        uniq, counts = np.unique(key, return_counts=True)
        boundary[uniq[counts == 1] // max(n_verts, 1)] = 1
    return inc_off.astype(np.int32), face.astype(np.int32), boundary


def step(x, faces, t, hold=None):
    """S3: one step with factor t on rows x [V,w] float32 -> float32 [V,w]"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    V = x.shape[0]
    v, face, p, q = entries(faces, V)
    x64 = x.astype(np.float64)
    k = np.bincount(v, minlength=V)
    s = np.zeros(x64.shape, np.float64)
    both = np.stack([p, q], 1).reshape(-1)                     # per entry x[p] then x[q], the entries in (vertex, face) order
    with np.errstate(all='ignore'):
        np.add.at(s, np.repeat(v, 2), x64[both])               # s = (s + x[p]) + x[q], one entry after the other
        m = s / (2.0 * np.maximum(k, 1))[:, None]
        d = m - x64
        moved = (x64 + np.float64(np.float32(t)) * d).astype(np.float32)
    keep = k == 0
    if hold is not None:
        keep = keep | (np.asarray(hold) != 0)
    out = moved
    out[keep] = x[keep]                                        # the bits, a NaN's payload included
    return out


def smooth(x, faces, iterations, lam, mu, hold=None):
    """S4: `iterations` times a step with lam, then a step with mu if mu != 0"""
    x = np.array(x, np.float32, copy=True)
    for _ in range(iterations):
        x = step(x, faces, lam, hold)
        if np.float32(mu) != 0:
            x = step(x, faces, mu, hold)
    return x


def vertex_normals(verts, faces):
    """S5 on verts [V,3] or [B,V,3] float32 -> float32 of the same shape"""
    verts = np.asarray(verts)
    assert verts.dtype == np.float32 and verts.shape[-1] == 3
    if verts.ndim == 3:
        return np.stack([vertex_normals(frame, faces) for frame in verts])
    V = verts.shape[0]
    v, face, _, _ = entries(faces, V)
    f = np.asarray(faces, np.int64).reshape(-1, 3)[face]       # STORED vertex order
    x = verts.astype(np.float64)
    with np.errstate(all='ignore'):
        u, w = x[f[:, 1]] - x[f[:, 0]], x[f[:, 2]] - x[f[:, 0]]
        cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1],
                          u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                          u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)
        n = np.zeros((V, 3), np.float64)
        np.add.at(n, v, cross)
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        unit = n / np.sqrt(l2)[:, None]
    usable = np.isfinite(l2) & (l2 > 0)
    return np.where(usable[:, None], unit, 0.0).astype(np.float32)


# ---- measures of the property test ------------------------------------------------------------------------------------------------------
def radial(verts, centre):
    """-> (mean radius, RMS deviation of the radius from its mean) about `centre`, float64"""
    r = np.linalg.norm(np.asarray(verts, np.float64) - np.asarray(centre, np.float64), axis=1)
    return float(r.mean()), float(np.sqrt(((r - r.mean()) ** 2).mean()))
