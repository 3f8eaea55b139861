"""-m gpu: the mesh simplification kernels (ml-neuman_amd/csrc/mesh_simplify.hip) through the C ABI against the numpy restatement
(tests/helpers/mesh_simplify_ref.py), and the Python surface over them (mesh_simplify.simplify_mesh, mesh_extract.extract_net_mesh's simplify
argument).

Every output lies inside a larger allocation with sentinel guard rows before and after, as in tests/test_hip_mesh_smooth.py.  vert_cluster, the
counts, the placed vertices under both placements, the faces, face_src and the averaged rows are compared with the restatement bit for bit: every
operation of rules Q5 and Q6 is a float64 add, subtract, multiply or divide in a stated order, which numpy and the device (contraction off) both
round one by one.  The sizes come from tests/helpers/simplify_sizes.py (checked against the source by tests/test_mesh_simplify_host.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mesh_simplify_ref as QR  # noqa: E402
import sharp_shapes as SH  # noqa: E402
import simplify_sizes as QS  # noqa: E402
import smooth_sizes as SS  # noqa: E402

from neuman_hip import _lib, mesh_extract, mesh_simplify, mesh_smooth, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5            # a quiet NaN with a payload (as int32: an index far out of range); no kernel produces it
GUARD = 67                       # guard rows before and after every array
I32, U8, F32 = torch.int32, torch.uint8, torch.float32
WIDTHS = (1, 3, 64)


def guarded(shape, dtype):
    """-> (buf, view): `view` of `shape` inside `buf`, GUARD rows of the sentinel's bytes each side (and in the view, until it is written)"""
    shape = tuple(shape)
    buf = torch.empty((shape[0] + 2 * GUARD,) + shape[1:], device='cuda', dtype=dtype)
    buf.view(-1).view(I32).fill_(SENTINEL)
    return buf, buf[GUARD:GUARD + shape[0]]


def guards_intact(buf):
    b = buf.view(I32).reshape(buf.shape[0], -1)
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())


def P(t):
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def attribute_rows(V, width, seed=QS.SEED):
    return np.random.default_rng(seed + width).normal(size=(V, width)).astype(np.float32)


class Device:
    """one mesh and grid on the device and the raw entry points on them, every output guarded; results come back as numpy"""

    def __init__(self, verts, faces, lo, h, dims):
        self.lib = _lib.lib()
        self.V, self.F = int(verts.shape[0]), int(faces.shape[0])
        self.verts = torch.from_numpy(np.array(verts, np.float32)).cuda().reshape(self.V, 3)                 # (a copy: the shapes are read-only)
        self.faces = torch.from_numpy(np.array(faces, np.int32)).cuda().reshape(self.F, 3)
        self.lo, self.h, self.dims = (ctypes.c_float * 3)(*(float(x) for x in lo)), float(h), tuple(int(n) for n in dims)
        self.nbytes = int(self.lib.nm_mesh_simplify_workspace_bytes(self.V, self.F, *self.dims))
        assert self.nbytes > 0
        self.ws_buf = torch.empty((self.nbytes + 2 * GUARD * 16,), device='cuda', dtype=U8).fill_(0xA5)     # 16-byte rows: the view stays aligned
        self.ws = self.ws_buf[GUARD * 16:GUARD * 16 + self.nbytes]
        assert self.ws.data_ptr() % 16 == 0
        self.bufs = []
        self.adj = None

    def out(self, shape, dtype):
        buf, view = guarded(shape, dtype)
        self.bufs.append(buf)
        return view

    def intact(self):
        torch.cuda.synchronize()
        edge = GUARD * 16
        return all(guards_intact(b) for b in self.bufs) and bool((self.ws_buf[:edge] == 0xA5).all()) and bool((self.ws_buf[-edge:] == 0xA5).all())

    def mesh(self):
        return (P(self.verts), self.V, P(self.faces), self.F, self.lo, self.h, *self.dims)

    def count(self):
        """-> (rc, vert_cluster, K, F')"""
        self.vc = self.out((self.V,), I32)
        k, nf = ctypes.c_int64(-7), ctypes.c_int64(-7)
        rc = self.lib.nm_mesh_simplify_count(*self.mesh(), P(self.vc), P(self.ws), self.nbytes, ctypes.byref(k), ctypes.byref(nf), stream())
        assert self.intact()
        self.K, self.Fo = int(k.value), int(nf.value)
        return rc, self.vc.cpu().numpy(), self.K, self.Fo

    def fill(self, placement, face_src=True, K=None, Fo=None):
        """-> (rc, verts_out, faces_out, face_src)"""
        K, Fo = self.K if K is None else K, self.Fo if Fo is None else Fo
        vo, fo = self.out((K, 3), F32), self.out((Fo, 3), I32)
        src = self.out((Fo,), I32) if face_src else None
        off = inc = None
        if placement == 'quadric':
            if self.adj is None:
                self.adj = mesh_smooth.adjacency(self.faces, self.V)
            off, inc = ctypes.c_void_p(self.adj.inc_off.data_ptr()), mesh_smooth._inc_ptr(self.adj)
        rc = self.lib.nm_mesh_simplify_fill(*self.mesh(), QR.PLACEMENTS[placement], off, inc, P(self.ws), self.nbytes, P(vo), P(fo), P(src), K, Fo, stream())
        assert self.intact()
        return rc, vo.cpu().numpy(), fo.cpu().numpy(), None if src is None else src.cpu().numpy()

    def rows(self, rows, K=None):
        K = self.K if K is None else K
        x = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
        out = self.out((K, x.shape[1]), F32)
        rc = self.lib.nm_mesh_simplify_rows(P(x), int(x.shape[1]), self.V, self.F, *self.dims, P(self.ws), self.nbytes, P(out), K, stream())
        assert self.intact()
        return rc, out.cpu().numpy()


def check(verts, faces, lo, h, dims, widths=WIDTHS, placements=('mean', 'quadric')):
    """every output of the three entry points against the restatement, bit for bit -> (device, the restatement's results by placement)"""
    d = Device(verts, faces, lo, h, dims)
    want = {p: QR.simplify(verts, faces, lo, h, dims, p) for p in placements}
    first = want[placements[0]]
    rc, vc, K, Fo = d.count()
    assert rc == 0, d.lib.nm_last_error()
    assert (K, Fo) == (first['K'], first['faces'].shape[0]) and same(vc, first['vert_cluster'])
    for p in placements:
        rc, vo, fo, src = d.fill(p)
        assert rc == 0, d.lib.nm_last_error()
        assert same(vo, want[p]['verts']), (p, int((bits(vo) != bits(want[p]['verts'])).any(1).sum()), K)
        assert same(fo, want[p]['faces']) and same(src, want[p]['face_src']), p
    rc, vo, fo, none = d.fill(placements[0], face_src=False)                          # face_src is nullable
    assert rc == 0 and none is None and same(vo, first['verts']) and same(fo, first['faces'])
    for w in widths:
        x = attribute_rows(d.V, w)
        rc, got = d.rows(x)
        assert rc == 0, d.lib.nm_last_error()
        assert same(got, QR.average_rows(x, first['vert_cluster'], K)[0]), w
    assert same(d.verts.cpu().numpy(), np.ascontiguousarray(verts, np.float32)) and same(d.faces.cpu().numpy(), np.ascontiguousarray(faces, np.int32))
    return d, want


# ---- 1: the octahedron --------------------------------------------------------------------------------------------------------------------
def test_octahedron_one_cell_per_vertex_and_one_cell_for_all():
    _lib.require_gpu()
    d, want = check(QS.OCTA_VERTS, QS.OCTA_FACES, *QS.OCTA_FINE)
    assert d.K == 6 and d.Fo == 8
    d, want = check(QS.OCTA_VERTS, QS.OCTA_FACES, *QS.OCTA_COARSE)                    # K = 0: every output has capacity 0 and a null pointer
    assert d.K == 0 and d.Fo == 0 and (want['mean']['vert_cluster'] == -1).all()
    none = np.zeros((0, 3), np.int32)
    d, want = check(QS.OCTA_VERTS, none, *QS.OCTA_FINE)                               # no face: no cluster
    assert d.K == 0 and d.Fo == 0
    d, want = check(np.zeros((0, 3), np.float32), none, *QS.OCTA_FINE, placements=('mean',))      # no vertex
    assert d.K == 0 and d.Fo == 0


# ---- 2: the sharp shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cell", [("torus", 0.11)] + [("star_prism_fine", c) for c in QS.STAR_CELLS] + [("star_prism_open", 0.11)])
def test_sharp_shapes(name, cell):
    s = SH.shape(name)
    lo, h, dims = QR.grid(QS.UNIT_BOX, cell)
    d, want = check(s['verts'], s['faces'], lo, h, dims)
    q, m = want['quadric'], want['mean']
    assert 0 < d.K < s['verts'].shape[0] and 0 < d.Fo < s['faces'].shape[0]
    assert not q['fallback'].all() and not same(q['verts'], m['verts'])
    if (name, cell) == ("star_prism_fine", 0.3):
        assert q['members'].max() == QS.STAR_LARGEST_CLUSTER and q['fallback'].any()
    if (name, cell) == ("star_prism_fine", 0.11):
        assert q['n_candidates'] > d.Fo and QR.opposite_pairs(q['faces']) >= 1       # duplicates dropped, opposite pairs kept


# ---- 3: an extracted sphere, the grid not aligned to the extraction's --------------------------------------------------------------------
def test_extracted_sphere_on_an_unaligned_grid():
    verts, faces, lo, h, dims = QS.sphere_mesh()
    assert verts.shape[0] > 2 * QS.C.SPAN
    d, want = check(verts, faces, lo, h, dims)
    assert 100 < d.K < verts.shape[0] // 4
    r = np.linalg.norm(want['quadric']['verts'].astype(np.float64) - np.asarray(SS.SPHERE_CENTRE), axis=1)
    assert np.abs(r - SS.SPHERE_RADIUS).max() < 0.25 * QS.SPHERE_CELL                 # the placed vertices stay at the surface


# ---- 4: the robustness cases --------------------------------------------------------------------------------------------------------------
def test_hand_written_mesh():
    verts, faces, lo, h, dims = QS.hand_mesh()
    d, want = check(verts, faces, lo, h, dims, widths=(3,))
    vc = want['mean']['vert_cluster']
    assert d.K == 17 and d.Fo == 13 and vc[6] == -1 and vc[18] == vc[0] and vc[19] == vc[20] == -1
    rc, got = d.rows(SS.hand_rows(3))                                                 # the NaN row belongs to no cluster
    assert rc == 0 and np.isfinite(got).all() and same(got, QR.average_rows(SS.hand_rows(3), vc, 17)[0])


@pytest.mark.parametrize("bad", [-1, 'V', 2 ** 31 - 1, -2 ** 31])
def test_invalid_faces_are_counted_and_never_followed(bad):
    verts, faces = SS.grid_mesh(*QS.GRID_SMALL)
    V = verts.shape[0]
    lo, h, dims = QS.grid_of_mesh(verts, QS.GRID_SMALL_CELL)
    broken = faces.copy()
    for f, k in ((1234, 2), (77, 0), (2000, 1)):                                      # not in index order: the LOWEST face is reported
        broken[f, k] = V if bad == 'V' else bad
    d = Device(verts, broken, lo, h, dims)
    rc, vc, K, Fo = d.count()                                                         # (asserts the guards, the workspace's included)
    msg = d.lib.nm_last_error().decode()
    assert rc == -1 and (K, Fo) == (-7, -7) and "nm_mesh_simplify_count" in msg and "3 invalid faces" in msg and "face 77" in msg, msg
    rc, vo, fo, src = d.fill('mean', K=5, Fo=5)                                       # no count stands for this workspace: refused, nothing written
    assert rc == -1 and b"nm_mesh_simplify_fill" in d.lib.nm_last_error() and (bits(vo) == SENTINEL).all() and (fo == SENTINEL).all()
    d.faces.copy_(torch.from_numpy(faces))                                            # the next valid call on the same workspace
    want = QR.simplify(verts, faces, lo, h, dims, 'mean')
    rc, vc, K, Fo = d.count()
    assert rc == 0 and same(vc, want['vert_cluster']) and (K, Fo) == (want['K'], want['faces'].shape[0])
    rc, vo, fo, src = d.fill('mean')
    assert rc == 0 and same(vo, want['verts']) and same(fo, want['faces']) and same(src, want['face_src'])


# ---- 5: past the scans, the in-thread sort and a quiet table ------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,cell", [("GRID_SMALL", QS.GRID_SMALL_CELL), ("GRID_PAST_THE_SCAN", QS.GRID_PAST_CELL)])
def test_grids_past_the_vertex_and_face_scans(grid, cell):
    rows, cols = getattr(QS, grid)
    verts, faces = SS.grid_mesh(rows, cols)
    lo, h, dims = QS.grid_of_mesh(verts, cell)
    d, want = check(verts, faces, lo, h, dims, widths=(3,))
    assert d.K > 100 and d.Fo > 100


def test_cells_past_the_cell_scan():
    t = SH.shape('torus')
    d, want = check(t['verts'], t['faces'], QS.CELLS_PAST_LO, QS.CELLS_PAST_H, QS.CELLS_PAST_THE_SCAN, widths=(3,))
    assert 500 < d.K < 512 and d.Fo == 1024                                           # nearly a cell per vertex (the clamped rows of y merge a few): every face stays


@pytest.mark.parametrize("extra", [QS.CROWD_JUST_PAST, QS.CROWD_FAR_PAST])
def test_clusters_past_the_in_thread_sort(extra):
    verts, faces = QS.crowded_octahedron(extra)
    d, want = check(verts, faces, *QS.OCTA_FINE)
    assert d.K == 6 and d.Fo == 8 and want['mean']['members'].max() == extra + 1


def test_many_faces_of_one_triple():
    f = QS.repeated_octahedron()
    d, want = check(QS.OCTA_VERTS, f, *QS.OCTA_FINE, widths=(1,))
    assert d.K == 6 and d.Fo == 16 and want['mean']['n_candidates'] == 8 * QS.REPEATS


# ---- 6: determinism, the order of the faces' rows, a stale workspace ----------------------------------------------------------------------
def run_all(verts, faces, lo, h, dims):
    d = Device(verts, faces, lo, h, dims)
    rc, vc, K, Fo = d.count()
    assert rc == 0
    out = [vc, np.array([K, Fo])]
    for p in ('mean', 'quadric'):
        rc, vo, fo, src = d.fill(p)
        assert rc == 0
        out += [vo, fo, src]
    out.append(d.rows(attribute_rows(d.V, 3))[1])
    return out


def test_determinism_and_face_order():
    s = SH.shape('star_prism_fine')
    verts, faces = s['verts'], s['faces'].astype(np.int32)
    lo, h, dims = QR.grid(QS.UNIT_BOX, 0.11)
    crowd = QS.crowded_octahedron(QS.CROWD_FAR_PAST)
    for args in ((verts, faces, lo, h, dims), crowd + QS.OCTA_FINE, (QS.OCTA_VERTS, QS.repeated_octahedron()) + QS.OCTA_FINE):
        a, b = run_all(*args), run_all(*args)
        assert all(same(x, y) for x, y in zip(a, b))
    base = run_all(verts, faces, lo, h, dims)
    perm = np.random.default_rng(QS.SEED + 2).permutation(faces.shape[0])
    p = run_all(verts, faces[perm], lo, h, dims)
    assert same(p[0], base[0]) and same(p[1], base[1]) and same(p[2], base[2]) and same(p[-1], base[-1])      # vert_cluster, the counts, the means, the rows
    assert {tuple(t) for t in p[3].tolist()} == {tuple(t) for t in base[3].tolist()}                           # the set of kept rotated triples
    assert np.abs(p[5].astype(np.float64) - base[5]).max() < 1e-5                     # quadric sums follow face order: the last bits may move


def test_fill_refuses_sizes_the_count_did_not_leave():
    d = Device(QS.OCTA_VERTS, QS.OCTA_FACES, *QS.OCTA_FINE)
    assert d.count()[0] == 0 and (d.K, d.Fo) == (6, 8)
    for K, Fo in ((5, 8), (6, 7), (7, 8), (0, 0)):
        rc, vo, fo, src = d.fill('mean', K=K, Fo=Fo)
        assert rc == -1 and b"nm_mesh_simplify_fill" in d.lib.nm_last_error() and (bits(vo) == SENTINEL).all() and (fo == SENTINEL).all(), (K, Fo)
    rc, got = d.rows(attribute_rows(6, 3), K=5)
    assert rc == -1 and b"nm_mesh_simplify_rows" in d.lib.nm_last_error() and (bits(got) == SENTINEL).all()
    other = Device(QS.OCTA_VERTS, QS.OCTA_FACES[:7], *QS.OCTA_FINE)                    # the same workspace address counted for another mesh
    other.ws, other.ws_buf, other.nbytes = d.ws, d.ws_buf, d.nbytes
    assert other.count()[0] == 0 and other.Fo == 7
    rc, vo, fo, src = d.fill('mean')
    assert rc == -1 and (bits(vo) == SENTINEL).all()
    assert d.count()[0] == 0 and d.fill('mean')[0] == 0


# ---- 7: the Python surface ----------------------------------------------------------------------------------------------------------------
def test_simplify_mesh_and_what_takes_its_output():
    from neuman_hip import mesh_pose, render_utils
    body_v, body_f = synthetic.capsule_mesh(12, 10)
    fine_v, fine_f = synthetic.capsule_mesh(40, 38)
    fine_f = np.ascontiguousarray(np.asarray(fine_f)[:, :3], np.int32)
    verts = torch.from_numpy(np.asarray(fine_v, np.float32) * np.float32(1.15)).cuda()
    faces = torch.from_numpy(fine_f).cuda()
    V = verts.shape[0]
    colours = torch.from_numpy(attribute_rows(V, 3)).cuda()
    wide = torch.from_numpy(attribute_rows(V, 64)).cuda()
    lo_hi = torch.cat([verts.amin(0), verts.amax(0)]).cpu().tolist()
    cell = 0.3 * float(min(lo_hi[3 + a] - lo_hi[a] for a in range(3)))
    v2, f2, c2, w2, vc, src = mesh_simplify.simplify_mesh(verts, faces, cell, colours, wide, return_map=True)      # aabb=None, quadric, adj built
    K = v2.shape[0]
    assert 8 < K < V // 4 and f2.dtype == I32 and v2.dtype == F32 and c2.shape == (K, 3) and w2.shape == (K, 64) and vc.shape == (V,) and src.shape == (f2.shape[0],)
    box = tuple(lo_hi)
    again = mesh_simplify.simplify_mesh(verts, faces, cell, colours, aabb=box, adj=mesh_smooth.adjacency(faces, V))
    assert len(again) == 3 and torch.equal(again[0], v2) and torch.equal(again[1], f2) and torch.equal(again[2], c2)
    lo, h, dims = QR.grid(box, cell)
    want = QR.simplify(verts.cpu().numpy(), faces.cpu().numpy(), lo, h, dims, 'quadric')
    assert same(v2.cpu().numpy(), want['verts']) and same(f2.cpu().numpy(), want['faces']) and same(vc.cpu().numpy(), want['vert_cluster'])
    assert same(src.cpu().numpy(), want['face_src'])
    assert same(c2.cpu().numpy(), QR.average_rows(colours.cpu().numpy(), want['vert_cluster'], K)[0])            # the attributes are the averaged rows
    assert same(w2.cpu().numpy(), QR.average_rows(wide.cpu().numpy(), want['vert_cluster'], K)[0])
    mean = mesh_simplify.simplify_mesh(verts, faces, cell, aabb=box, placement='mean')
    assert torch.equal(mean[1], f2) and same(mean[0].cpu().numpy(), QR.simplify(verts.cpu().numpy(), faces.cpu().numpy(), lo, h, dims, 'mean')['verts'])
    # the output is a mesh like any other
    comps = mesh_extract.components(f2, K, v2)
    assert comps.n == 1 and int(comps.n_verts[0]) == K and int(comps.n_faces[0]) == f2.shape[0]
    adj = mesh_smooth.adjacency(f2, K)
    assert adj.inc.shape[0] == 3 * f2.shape[0] and not bool(adj.boundary.any())      # still closed
    normals = mesh_smooth.vertex_normals(v2, f2, adj=adj)
    binding = mesh_pose.bind_mesh(v2, body_v, body_f)
    T = torch.from_numpy(np.stack([synthetic.twist_transforms(body_v, twist)[1] for twist in (0.8, -0.5)])).cuda()
    posed, posed_n = mesh_pose.pose_mesh(v2, binding, T, normals=normals, check=True)
    caps = [synthetic.SimpleCapture(48, 48, c2w=synthetic.spherical_c2w(a, -20, 4.0), far=8.0) for a in (30, 120)]
    frames = render_utils.render_mesh_frames(posed, f2, caps, colours=torch.sigmoid(c2), normals=posed_n)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 48, 48, 3) and bool((frames != 255).any())
    # refusals
    with pytest.raises(_lib.NeumanHipError):
        mesh_simplify.simplify_mesh(verts, faces, cell, colours[:-1].contiguous())
    with pytest.raises(_lib.NeumanHipError):
        mesh_simplify.simplify_mesh(verts, faces, cell, adj=adj)                      # an adjacency of another mesh
    with pytest.raises(_lib.NeumanHipError):
        mesh_simplify.simplify_mesh(verts, torch.cat([faces, torch.tensor([[0, 1, V]], device='cuda', dtype=I32)]), cell, placement='mean')
    empty = mesh_simplify.simplify_mesh(verts, faces, 100.0, colours)                 # one cell for everything
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0, 3)


# ---- 8: extract_net_mesh ------------------------------------------------------------------------------------------------------------------
def test_extract_net_mesh_simplifies_after_the_smoothing():
    net = synthetic.make_joiner(0).cuda()
    box, res = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), 24
    field = mesh_extract.density_grid(net, box, res)
    level = float(field.reshape(-1).quantile(0.9))
    plain = mesh_extract.extract_net_mesh(net, box, res, level, largest=1, smooth=2)
    for kw in (dict(simplify=0), dict(simplify=0.0)):                                 # simplify = 0: the path as it was, tensor for tensor
        assert all(torch.equal(a, b) for a, b in zip(mesh_extract.extract_net_mesh(net, box, res, level, largest=1, smooth=2, **kw), plain)), kw
    h = 2.5 * 2.0 / (res - 1)
    v, f, nrm, col = mesh_extract.extract_net_mesh(net, box, res, level, largest=1, smooth=2, simplify=h)
    sv, sf = mesh_simplify.simplify_mesh(plain[0], plain[1], h, aabb=box)             # the chain by hand
    sn = mesh_smooth.vertex_normals(sv, sf)
    with torch.no_grad():
        want = torch.sigmoid(net(sv, -sn if net.nerf.use_viewdirs else None)[..., :3])
    assert torch.equal(v, sv) and torch.equal(f, sf) and torch.equal(nrm, sn) and torch.equal(col, want)
    assert 0 < v.shape[0] < plain[0].shape[0] // 2 and col.shape == (v.shape[0], 3)
