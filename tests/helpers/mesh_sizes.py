"""The sizes at which the mesh kernels change behaviour, and the shapes tests/test_hip_mesh_sizes.py crosses them with.

TABLE has the form of tests/test_hip_sizes.py's: name -> (value, source file, pattern whose integer groups multiply to the value);
tests/test_mesh_size_table.py checks on the CPU that every entry still reads so in its source line and that every shape derived below lies on
the far side of its threshold, so a change to one of the constants shows up as a stale table and not as a test that quietly stopped crossing.

Nothing here touches the device: the inputs of the GPU tests (meshes, fields, clouds, rays, query points) are built in numpy, so that their
properties (which tiles are covered, which spans own mesh vertices, that the oracle's float64 and float32 runs agree on every ray) can be
checked without one."""
import math
import types

import numpy as np

CSRC = 'ml-neuman_amd/csrc/'
TABLE = {
    # raster.hip / silhouette.hip: one 16 x 16-pixel tile per workgroup
    'TILE': (16, CSRC + 'raster_device.h', r'constexpr int kTile = (\d+);'),
    # raster_scan_kernel: ONE workgroup of 256 threads scans the T tile counts, ceil(T / 256) tiles per thread (raster_device.h); launched by
    # the rasteriser and by the one-frame silhouette
    'SCAN_THREADS': (256, CSRC + 'raster_device.h', r'const int per = \(T \+ 255\) / (\d+), lo = threadIdx\.x \* per'),
    'SCAN_THREADS_RASTER': (256, CSRC + 'raster.hip', r'raster_scan_kernel, dim3\(1\), dim3\((\d+)\)'),
    'SCAN_THREADS_SILHOUETTE': (256, CSRC + 'silhouette.hip', r'raster_scan_kernel, dim3\(1\), dim3\((\d+)\)'),
    # sil_scan_batch_kernel: ONE workgroup of 1024 threads scans the B T counts and looks at the B cameras, 1024 at a time
    'BATCH_SCAN_THREADS': (1024, CSRC + 'silhouette.hip', r'sil_scan_batch_kernel, dim3\(1\), dim3\((\d+)\)'),
    'BATCH_SCAN_PER': (1024, CSRC + 'silhouette.hip', r'const int64_t per = \(n \+ 1023\) / (\d+), lo = \(int64_t\)threadIdx\.x \* per'),
    'BATCH_CAMERA_STRIDE': (1024, CSRC + 'silhouette.hip', r'for \(int b = threadIdx\.x; b < B; b \+= (\d+)\)'),
    # iso_scan_kernel: ONE workgroup of kThreads scans the spans' sums, ceil(spans / kThreads) spans of kScanSpan grid vertices per thread
    'ISO_SPAN': (2048, CSRC + 'isosurface.hip', r'constexpr int kScanSpan = (\d+);'),
    'ISO_THREADS': (256, CSRC + 'isosurface.hip', r'constexpr int kThreads = (\d+);'),
    # near_far_kernel: bounding spheres for at most kMaxClusters clusters of 64 consecutive vertices; beyond, one sphere and every vertex
    'MAX_CLUSTERS': (512, CSRC + 'nearfar.hip', r'constexpr int kMaxClusters = (\d+);'),
    'CLUSTER': (64, CSRC + 'nearfar.hip', r'const bool use_cl = \(V \+ 63\) / (\d+) <= kMaxClusters;'),
    # the closest-point search: uint16 triangle ids up to this many faces (tests/test_hip_warp_edges.py::test_small_encoding_boundary)
    'SMALL_ENCODING_FACES': (65536, CSRC + 'warp.hip', r'const bool small = m->n_nodes <= \d+ && m->F <= (\d+) && !m->force_wide;'),
}
C = types.SimpleNamespace(**{k: v[0] for k, v in TABLE.items()})

CAMERA = (30., -20., 1.3)                # spherical_c2w of every case that does not say otherwise
FAR_CAMERA = (30., -20., 4.0)            # ... of the extracted meshes, which fill a box of side 2


def tiles(W, H):
    return ((W + C.TILE - 1) // C.TILE) * ((H + C.TILE - 1) // C.TILE)


def per_thread(n, threads):
    """what the one-workgroup scans give each thread: ceil(n / threads)"""
    return (n + threads - 1) // threads


# ---- a, b, c: images of more than SCAN_THREADS tiles: name -> (capsule_mesh arguments, W, H, principal-point shift in pixels) -------------
_ROW = (C.SCAN_THREADS + 1) * C.TILE                                  # 4112
_SIDE = (math.isqrt(C.SCAN_THREADS) + 1) * C.TILE                     # 272
RASTER_CASES = {
    # one row of SCAN_THREADS + 1 tiles: two tiles per thread, the last busy thread holds one, the upper half of the workgroup idles
    'one_tile_over_4112x16': ((12, 10), _ROW, C.TILE, (0, 0)),
    # SCAN_THREADS pixels high, 2 TILE + 1 tiles wide: more than 2 SCAN_THREADS tiles, three per thread
    'three_per_thread_528x256': ((12, 10), (2 * C.TILE + 1) * C.TILE, C.SCAN_THREADS, (0, 0)),
    # the smallest square past the threshold, with a mesh of many small faces
    'square_272x272': ((40, 38), _SIDE, _SIDE, (0, 0)),
    # In the first and the third image the body stays in tiles below SCAN_THREADS (it is centred): the same two with the principal point
    # moved, so that it reaches the LAST tiles -- the one tile of the last busy thread among them -- and partly leaves the frame there
    'one_tile_over_4112x16_at_the_right_end': ((12, 10), _ROW, C.TILE, (44 * C.TILE, 0)),
    'square_272x272_at_the_bottom': ((40, 38), _SIDE, _SIDE, (0, 3 * C.TILE)),
}
REACHES_PAST_THE_THREAD_COUNT = ('three_per_thread_528x256', 'one_tile_over_4112x16_at_the_right_end', 'square_272x272_at_the_bottom')
SILHOUETTE_CASES = ('one_tile_over_4112x16', 'three_per_thread_528x256')


def capture(W, H, shift=(0, 0), camera=CAMERA):
    """synthetic.SimpleCapture of W x H with its default intrinsics, the principal point moved by `shift` pixels"""
    from neuman_hip import synthetic
    return synthetic.SimpleCapture(W, H, cx=W / 2 + shift[0], cy=H / 2 + shift[1], c2w=synthetic.spherical_c2w(*camera))


def tile_census(mask, W, H):
    """-> (indices of the tiles holding a pixel of `mask` [H,W], the raster_scan_kernel threads that own those tiles)"""
    rows, cols = np.nonzero(mask)
    tx = (W + C.TILE - 1) // C.TILE
    t = np.unique((rows // C.TILE) * tx + cols // C.TILE)
    return t, np.unique(t // per_thread(tiles(W, H), C.SCAN_THREADS))
SILHOUETTE_SIGMA = 1e-2
SMALL_IMAGE = (6 * C.TILE, 4 * C.TILE)                                # 96 x 64, below the threshold: the size around which one handle regrows
BIG_IMAGE = RASTER_CASES['three_per_thread_528x256'][1:3]

# ---- d: batches of more than BATCH_SCAN_THREADS (frame, tile) entries ----------------------------------------------------------------------
BATCH_SIDE = (C.TILE - 1) * C.TILE                                    # 240 x 240: 225 tiles
BATCH_FRAMES = C.BATCH_SCAN_THREADS // tiles(BATCH_SIDE, BATCH_SIDE) + 1          # 5 frames: 1125 entries
MANY_FRAMES = C.BATCH_CAMERA_STRIDE + 6                               # 1030 frames of one tile: the camera check makes a second pass
MANY_CHECKED = (0, C.BATCH_CAMERA_STRIDE - 1, C.BATCH_CAMERA_STRIDE, MANY_FRAMES - 1)
MANY_BAD = C.BATCH_CAMERA_STRIDE + 3                                  # the frame whose w2c gets a NaN: seen only by the second pass

# ---- e: grids of more than ISO_THREADS spans (nx, ny, nz): name -> (dims, the gyroid's frequency, level) -----------------------------------
ISO_BOX = (-1.0, -0.8, -0.7, 1.1, 0.9, 0.75)                          # tests/test_hip_isosurface.py's SKEW
ISO_CASES = {
    'two_per_thread_131x67x63': ((131, 67, 63), 4.3, 0.1),
    'three_per_thread_97x81x135': ((97, 81, 135), 4.3, 0.1),
}
PRODUCTION_MESH = 'two_per_thread_131x67x63'                          # the mesh of section g


def spans(dims):
    n = dims[0] * dims[1] * dims[2]
    return (n + C.ISO_SPAN - 1) // C.ISO_SPAN


def owner_spans(field, level):
    """-> (the spans whose grid vertices own a mesh vertex -- a crossed edge toward a higher index, rule M4 --, the iso_scan_kernel threads
    that own those spans); field [nz,ny,nx]"""
    inside = np.asarray(field, np.float32) > np.float32(level)
    nz, ny, nx = inside.shape
    owns = np.zeros(inside.shape, bool)
    for m in range(1, 8):
        dx, dy, dz = m & 1, (m >> 1) & 1, m >> 2
        owns[:nz - dz, :ny - dy, :nx - dx] |= inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
    s = np.unique(np.flatnonzero(owns.reshape(-1)) // C.ISO_SPAN)
    return s, np.unique(s // per_thread(spans((nx, ny, nz)), C.ISO_THREADS))


# ---- f: near / far at the cluster table's end -------------------------------------------------------------------------------------------
V_TABLE_FULL = C.MAX_CLUSTERS * C.CLUSTER                             # 32 768: the last V with per-cluster spheres
N_RAYS = 5 * C.CLUSTER                                                # 320: five waves
CLOUD_SEED, CLOUD_RAY_SEED, MESH_RAY_SEED = 0, 0, 0                   # chosen on the CPU: see tests/test_mesh_size_table.py
NEAR_FAR_TAU = 0.05


def body_cloud(seed=CLOUD_SEED):
    """-> [V_TABLE_FULL, 3] float32: synthetic.human_vertex_cloud(0) tiled with seeded jitter, sorted along the body as
    test_near_far_cluster_skip_is_bit_identical sorts it (compact clusters), cut to the table's size"""
    from neuman_hip import synthetic
    base = synthetic.human_vertex_cloud(0).astype(np.float32)
    rng = np.random.default_rng(seed)
    copies = -(-V_TABLE_FULL // len(base))
    v = np.concatenate([base + rng.normal(size=base.shape).astype(np.float32) * np.float32(0.01) for _ in range(copies)]).astype(np.float32)
    v = v[np.argsort(v[:, 1] * 7 + v[:, 0], kind='stable')]
    return np.ascontiguousarray(v[:V_TABLE_FULL])


def rays_at(verts, seed, origin=(0.1, 0.2, -2.5), spread=0.3):
    """N_RAYS unit rays from one origin toward seeded points around seeded vertices -> o [N,3], d [N,3] float32"""
    rng = np.random.default_rng(seed)
    o = np.tile(np.asarray(origin, np.float32)[None], (N_RAYS, 1))
    tgt = verts[rng.integers(0, len(verts), N_RAYS)] + rng.normal(size=(N_RAYS, 3)).astype(np.float32) * np.float32(spread)
    d = tgt - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


# ---- g, h: query points of the closest-point search ---------------------------------------------------------------------------------------
N_QUERY, N_ORACLE = 4000, 256


def near_surface_points(verts, faces, n, seed):
    """[n,3] float32, finite: points of seeded faces' interiors moved along the face normal by 0, +-1e-4, +-0.01 or +-0.05, and every eighth a
    mesh vertex itself (ties among the faces around it).  A face of zero area has no normal: its points stay on it."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, len(faces), n)
    tri = verts[faces[f]].astype(np.float64)
    w = rng.dirichlet([1, 1, 1], n)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(length > 0, nrm / np.where(length > 0, length, 1.0), 0.0)
    off = rng.choice([0.0, 1e-4, 0.01, 0.05], n) * rng.choice([-1.0, 1.0], n)
    pts = (tri * w[..., None]).sum(1) + nrm * off[:, None]
    pts[::8] = verts[faces[f[::8], 0]]
    pts = pts.astype(np.float32)
    assert np.isfinite(pts).all()
    return pts


def zero_area(verts, faces):
    """the faces whose float32 vertices span no area: coincident or collinear corners (marching tetrahedra place a vertex ON a grid vertex whose
    sample equals the level, once for every crossed edge that ends there)"""
    tri = verts[faces].astype(np.float64)
    return np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) == 0


def _segment_distance(p, a, b):
    """[N,1,3] points against [1,M,3] segments a -> b (a == b: the point a) -> [N,M] distances, float64"""
    e = b - a
    ee = (e * e).sum(-1)
    t = np.clip(((p - a) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
    q = a + t[..., None] * e
    return np.sqrt(((p - q) ** 2).sum(-1))


def brute_distance(pts, verts, faces):
    """float64 distance from every point to the mesh as a set: every face of positive area by oracle.warp.closest_point_on_triangles, every
    face of zero area as its three edge segments -> [N]"""
    from oracle import warp as OW
    p = pts.astype(np.float64)[:, None, :]
    v = verts.astype(np.float64)
    flat = zero_area(verts, faces)
    best = np.full(len(pts), np.inf)
    tri = v[faces[~flat]]
    if len(tri):
        q = OW.closest_point_on_triangles(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        best = np.minimum(best, np.sqrt(((q - p) ** 2).sum(-1)).min(1))
    seg = v[faces[flat]]
    for i, j in ((0, 1), (1, 2), (2, 0)):
        if len(seg):
            best = np.minimum(best, _segment_distance(p, seg[None, :, i], seg[None, :, j]).min(1))
    return best
