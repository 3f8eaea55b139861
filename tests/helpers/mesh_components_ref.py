"""A numpy restatement of the mesh clean-up contract (include/neuman_hip.h 'mesh components', rules C1-C7): connected components of an
indexed triangle mesh, their statistics, and the mesh compacted to a subset of them.

Nothing here follows the kernels' method (a lock-free union-find): the components come from min-label propagation over the edges with
pointer jumping, vectorised, so that a mesh of a few hundred thousand faces takes the helper a second or so."""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def invalid_faces(faces, n_verts):
    """C1 -> the indices of the faces that name a vertex outside [0, n_verts), ascending"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.flatnonzero(((f < 0) | (f >= n_verts)).any(1))


def labels(faces, n_verts):
    """C2, C3 -> (vert_label [V] int32, face_label [F] int32, n_components); ValueError when a face is invalid"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bad = invalid_faces(f, n_verts)
    if bad.size:
        raise ValueError(f"{bad.size} invalid faces, the first of them face {bad[0]}")
    a = np.concatenate([f[:, 0], f[:, 0], f[:, 1]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 2]])
    low = np.arange(n_verts, dtype=np.int64)                  # low[v]: a vertex of v's component, never above v; at the end the smallest
    while True:
        new = low.copy()
        m = np.minimum(low[a], low[b])
        np.minimum.at(new, low[a], m)                          # after the jumping low[a] is the root of a's tree: whole trees merge,
        np.minimum.at(new, low[b], m)                          # so the rounds number about log V and not the mesh's diameter
        while True:                                            # pointer jumping to the fixed point
            hop = new[new]
            if np.array_equal(hop, new):
                break
            new = hop
        if np.array_equal(new, low):
            break
        low = new
    referenced = np.zeros(n_verts, bool)
    referenced[f.reshape(-1)] = True
    is_rep = referenced & (low == np.arange(n_verts))
    rank = np.cumsum(is_rep) - 1
    vert_label = np.where(referenced, rank[low], -1).astype(np.int32)
    face_label = vert_label[f[:, 0]] if f.shape[0] else np.zeros(0, np.int32)
    return vert_label, face_label.astype(np.int32), int(is_rep.sum())


def float_image(x):
    """the order-preserving integer image of float32: -inf < ... < -0 < +0 < ... < +inf as uint32"""
    b = np.asarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def image_float(u):
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(np.float32)


def stats(faces, vert_label, n, verts=None):
    """C4 -> (comp_verts [n] int32, comp_faces [n] int32, comp_box [n,6] float32 or None)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = np.asarray(vert_label, np.int64)
    comp_verts = np.bincount(lab[lab >= 0], minlength=n).astype(np.int32)
    first = lab[f[:, 0]] if f.shape[0] else np.zeros(0, np.int64)
    comp_faces = np.bincount(first[first >= 0], minlength=n).astype(np.int32)
    if verts is None:
        return comp_verts, comp_faces, None
    v = np.asarray(verts, np.float32)
    lo = np.full((n, 3), float_image(np.float32(np.inf)), np.uint32)
    hi = np.full((n, 3), float_image(np.float32(-np.inf)), np.uint32)
    for axis in range(3):
        use = (lab >= 0) & ~np.isnan(v[:, axis])
        img = float_image(v[use, axis])
        np.minimum.at(lo[:, axis], lab[use], img)
        np.maximum.at(hi[:, axis], lab[use], img)
    return comp_verts, comp_faces, np.concatenate([image_float(lo), image_float(hi)], 1)


def select(faces, vert_label, keep):
    """C5 -> (vert_src [Nv'] int32, faces_out [Nf',3] int32)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = np.asarray(vert_label, np.int64)
    keep = np.asarray(keep).astype(bool)
    kept = lab >= 0
    kept[kept] = keep[lab[kept]]
    vert_src = np.flatnonzero(kept).astype(np.int32)
    new = np.where(kept, np.cumsum(kept) - 1, -1)
    kept_face = kept[f[:, 0]] if f.shape[0] else np.zeros(0, bool)
    return vert_src, new[f[kept_face]].astype(np.int32).reshape(-1, 3)


def keep_largest(comp_faces, largest=1, min_faces=0):
    """clean_mesh's choice -> bool [n]: at least min_faces faces, and among those the `largest` biggest by face count, ties to the lower id"""
    nf = np.asarray(comp_faces, np.int64)
    enough = nf >= min_faces
    if largest is None:
        return enough
    order = sorted(np.flatnonzero(enough), key=lambda c: (-nf[c], c))[:largest]
    keep = np.zeros(nf.shape[0], bool)
    keep[order] = True
    return keep
