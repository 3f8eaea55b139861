"""A numpy restatement of the isosurface contract (include/neuman_hip.h 'isosurface', rules M1-M7): marching tetrahedra on the Kuhn split.

`extract(field, aabb, level)` follows the device's operation order in float32 (fmaf emulated through float64: the product of two float32 is
exact there, the sum rounds once in float64 and once more to float32); `extract(..., dtype=np.float64)` evaluates the same formulas in
float64 on the same float32 inputs -- the yardstick of the normals' tolerance.  Topology (which edges are crossed, the faces) does not
depend on dtype.  The tables are built here from rules M3 / M5, independently of the kernels' source."""
import itertools

import numpy as np

DIRS = [(m & 1, (m >> 1) & 1, m >> 2) for m in range(1, 8)]          # direction d = m - 1: (dx, dy, dz)


def _parity(perm):
    return sum(perm[i] > perm[j] for i in range(len(perm)) for j in range(i + 1, len(perm))) & 1


def tetrahedra():
    """-> [(corner masks c0..c3, odd)] for the six axis permutations in lexicographic order (M3)"""
    out = []
    for a, b, c in itertools.permutations(range(3)):
        out.append(((0, 1 << a, (1 << a) | (1 << b), 7), _parity((a, b, c))))
    return out


def tet_case(mask):
    """the triangles of one inside pattern (bit c = corner c inside) of an EVEN tetrahedron: a list of triangles, each three edges (p, q), p < q (M5)"""
    ins = [c for c in range(4) if (mask >> c) & 1]
    outs = [c for c in range(4) if not (mask >> c) & 1]
    if len(ins) in (0, 4):
        return []
    e = lambda p, q: (min(p, q), max(p, q))
    if len(ins) == 1:
        tris = [[e(ins[0], outs[0]), e(ins[0], outs[1]), e(ins[0], outs[2])]]
    elif len(ins) == 3:
        tris = [[e(ins[0], outs[0]), e(ins[1], outs[0]), e(ins[2], outs[0])]]
    else:
        A, B, C, D = ins[0], ins[1], outs[0], outs[1]
        tris = [[e(A, C), e(A, D), e(B, D)], [e(A, C), e(B, D), e(B, C)]]
    if _parity(ins + outs):
        tris = [[t[0], t[2], t[1]] for t in tris]
    return tris


def _fma(a, b, c, dtype):
    if dtype is np.float64:
        return a * b + c
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _gradient(f, h, dtype):
    """[3][nz,ny,nx]: central differences, one-sided at the box faces (M6); f indexed [z, y, x], h per axis (x, y, z)"""
    g = []
    for a in range(3):
        fa = np.moveaxis(f, 2 - a, 0)
        d = np.empty_like(fa)
        with np.errstate(all='ignore'):
            d[1:-1] = (fa[2:] - fa[:-2]) / (dtype(2) * h[a])
            d[0] = (fa[1] - fa[0]) / h[a]
            d[-1] = (fa[-1] - fa[-2]) / h[a]
        g.append(np.moveaxis(d, 0, 2 - a))
    return g


def extract(field, aabb, level, dtype=np.float32):
    """-> dict(verts [Nv,3], faces [Nf,3] int32, normals [Nv,3], n_verts, n_faces)"""
    f32 = np.asarray(field, np.float32)
    nz, ny, nx = f32.shape
    n = (nx, ny, nz)
    box = np.asarray(aabb, np.float32).reshape(6)
    level32 = np.float32(level)
    inside = f32 > level32                                            # M2 (a NaN compares false), the same in either dtype
    # ---- M4: crossed edges and their ranks ----
    N = nx * ny * nz
    crossed = np.zeros((nz, ny, nx, 7), bool)
    for d, (dx, dy, dz) in enumerate(DIRS):
        a = inside[:nz - dz, :ny - dy, :nx - dx]
        b = inside[dz:, dy:, dx:]
        crossed[:nz - dz, :ny - dy, :nx - dx, d] = a != b
    flat = crossed.reshape(-1)
    rank = np.cumsum(flat, dtype=np.int64) - 1
    edge_index = np.where(flat, rank, -1).reshape(N, 7)
    ev, ed = np.nonzero(crossed.reshape(N, 7))                        # ascending edge id 7 v + d
    n_verts = int(ev.size)
    # ---- positions and normals ----
    f = f32.astype(dtype)
    lo, hi = box[:3].astype(dtype), box[3:].astype(dtype)
    h = [(hi[a] - lo[a]) / dtype(n[a] - 1) for a in range(3)]
    lvl = dtype(level32)
    ia = np.stack([ev % nx, (ev // nx) % ny, ev // (nx * ny)], 1)
    ib = ia + np.array(DIRS, np.int64)[ed]
    fa, fb = f[ia[:, 2], ia[:, 1], ia[:, 0]], f[ib[:, 2], ib[:, 1], ib[:, 0]]
    with np.errstate(all='ignore'):
        t = (lvl - fa) / (fb - fa)
        t = np.where((t >= 0) & (t <= 1), t, dtype(0.5)).astype(dtype)
        verts = np.empty((n_verts, 3), dtype)
        for a in range(3):
            pa = _fma(ia[:, a].astype(dtype), h[a], lo[a], dtype)
            pb = _fma(ib[:, a].astype(dtype), h[a], lo[a], dtype)
            verts[:, a] = _fma(t, pb - pa, pa, dtype)
        grad = _gradient(f, h, dtype)
        g = np.empty((n_verts, 3), dtype)
        for a in range(3):
            ga, gb = grad[a][ia[:, 2], ia[:, 1], ia[:, 0]], grad[a][ib[:, 2], ib[:, 1], ib[:, 0]]
            g[:, a] = _fma(t, gb - ga, ga, dtype)
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = (length > 0) & np.isfinite(length)
        normals = np.where(ok[:, None], -g / np.where(ok, length, dtype(1))[:, None], dtype(0)).astype(dtype)
    # ---- M5: faces, cell-major (k, j, i), tetrahedron, triangle ----
    cz, cy, cx = nz - 1, ny - 1, nx - 1
    kk, jj, ii = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing='ij')
    v0 = ((kk * ny + jj) * nx + ii).reshape(-1)
    off = lambda m: (m & 1) + ((m >> 1) & 1) * nx + (m >> 2) * nx * ny
    ins_flat = inside.reshape(-1)
    tri = np.full((v0.size, 6, 2, 3), -1, np.int64)
    for ti, (corners, odd) in enumerate(tetrahedra()):
        in4 = sum(ins_flat[v0 + off(corners[c])].astype(np.int64) << c for c in range(4))
        for mask in range(1, 15):
            sel = np.nonzero(in4 == mask)[0]
            if sel.size == 0:
                continue
            for k, edges in enumerate(tet_case(mask)):
                if odd:
                    edges = [edges[0], edges[2], edges[1]]
                for e, (p, q) in enumerate(edges):
                    mp, mq = corners[p], corners[q]
                    tri[sel, ti, k, e] = edge_index[v0[sel] + off(mp), (mq ^ mp) - 1]
    tri = tri.reshape(-1, 3)
    faces = tri[tri[:, 0] >= 0]
    assert (faces >= 0).all() and (faces < max(n_verts, 1)).all()
    return dict(verts=verts, faces=faces.astype(np.int32), normals=normals, n_verts=n_verts, n_faces=int(faces.shape[0]))


# ---- properties of a mesh ---------------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def edge_census(faces):
    """-> (closed: every directed edge occurs once and its reverse once, boundary [n,2]: directed edges whose reverse is absent,
    repeated: directed edges occurring more than once)"""
    e = directed_edges(faces)
    if e.size == 0:
        return True, e, 0
    big = int(e.max()) + 1
    key, rev = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    repeated = int((counts > 1).sum())
    boundary = e[~np.isin(rev, uniq)]
    return repeated == 0 and boundary.shape[0] == 0, boundary, repeated


def euler_characteristic(n_verts, faces):
    e = np.sort(directed_edges(faces), 1)
    return int(n_verts) - int(np.unique(e, axis=0).shape[0]) + int(np.asarray(faces).shape[0])


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


# ---- fields -----------------------------------------------------------------------------------------------------------------------------
def grid_points(dims, aabb):
    """float64 positions [nz,ny,nx,3] of the grid vertices (for building analytic fields; the contract's own positions are extract's)"""
    nx, ny, nz = dims
    box = np.asarray(aabb, np.float64).reshape(6)
    ax = [np.linspace(box[a], box[3 + a], n) for a, n in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return np.stack([x, y, z], -1)


def sphere_field(dims, aabb, centre, r0):
    """r0 - |p - c| (positive inside): a signed distance"""
    p = grid_points(dims, aabb)
    return (r0 - np.linalg.norm(p - np.asarray(centre, np.float64), axis=-1)).astype(np.float32)


def torus_field(dims, aabb, centre, R, r):
    p = grid_points(dims, aabb) - np.asarray(centre, np.float64)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R
    return (r - np.sqrt(q * q + p[..., 2] ** 2)).astype(np.float32)


def gyroid_field(dims, aabb, freq):
    p = grid_points(dims, aabb) * freq
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return (np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x)).astype(np.float32)


def noise_field(dims, seed, waves=6):
    """a seeded sum of a few plane waves: smooth, with level sets of no particular symmetry"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing='ij')
    f = np.zeros((nz, ny, nx))
    for _ in range(waves):
        k = rng.normal(size=3) * 7.0
        f += rng.normal() * np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 6.28))
    return f.astype(np.float32)
