"""-m gpu: the mesh smoothing kernels (ml-neuman_amd/csrc/mesh_smooth.hip) through the C ABI against the numpy restatement
(tests/helpers/mesh_smooth_ref.py), and the Python surface over them (mesh_smooth.adjacency / smooth_mesh / vertex_normals,
mesh_extract.extract_net_mesh's smooth argument).

Every output lies inside a larger allocation with sentinel guard rows before and after, as in tests/test_hip_mesh_components.py.  The
adjacency, the boundary flags and smoothed rows are compared with the restatement bit for bit (a NaN by position); normals within one float32
step per component: a float64 quotient or root a few float64 steps off moves the float32 result by at most one (the rule of
tests/test_hip_mesh_pose.py).  The sizes come from tests/helpers/smooth_sizes.py (checked against the source by tests/test_mesh_smooth_host.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mesh_pose_ref as PR  # noqa: E402
import mesh_smooth_ref as SR  # noqa: E402
import smooth_sizes as SS  # noqa: E402

from neuman_hip import _lib, mesh_extract, mesh_smooth, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5            # a quiet NaN with a payload (as int32: an index far out of range); no kernel produces it
GUARD = 67                       # guard rows before and after every array
I32, U8, F32 = torch.int32, torch.uint8, torch.float32
TAUBIN = (0.5, -0.53)


def guarded(shape, dtype):
    """-> (buf, view): `view` of `shape` inside `buf`, GUARD rows of the sentinel's bytes each side (and in the view, until it is written)"""
    shape = tuple(shape)
    buf = torch.empty((shape[0] + 2 * GUARD,) + shape[1:], device='cuda', dtype=dtype)
    flat = buf.view(-1)
    if dtype == U8:
        flat.fill_(0xA5)
    else:
        flat.view(I32).fill_(SENTINEL)
    return buf, buf[GUARD:GUARD + shape[0]]


def guards_intact(buf):
    if buf.dtype == U8:
        return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())
    b = buf.view(I32).reshape(buf.shape[0], -1)
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_rows(a, b):
    """float32 rows bit for bit, a NaN by position"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def within_one_step(a, b):
    return a.shape == b.shape and int(PR.ulp_distance(a, b).max(initial=0)) <= 1


class Device:
    """one mesh on the device and the raw entry points on it, every output guarded; results come back as numpy"""

    def __init__(self, faces, n_verts):
        self.lib = _lib.lib()
        self.F, self.V = int(faces.shape[0]), int(n_verts)
        self.faces = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).cuda().reshape(self.F, 3)
        self.nbytes = int(self.lib.nm_mesh_adjacency_workspace_bytes(self.V, self.F))
        assert self.nbytes > 0
        self.ws_buf = torch.empty((self.nbytes + 2 * GUARD * 16,), device='cuda', dtype=U8).fill_(0xA5)     # 16-byte rows: the view stays aligned
        self.ws = self.ws_buf[GUARD * 16:GUARD * 16 + self.nbytes]
        assert self.ws.data_ptr() % 16 == 0
        self.bufs = []

    def out(self, shape, dtype):
        buf, view = guarded(shape, dtype)
        self.bufs.append(buf)
        return view

    def intact(self):
        torch.cuda.synchronize()
        edge = GUARD * 16
        return all(guards_intact(b) for b in self.bufs) and bool((self.ws_buf[:edge] == 0xA5).all()) and bool((self.ws_buf[-edge:] == 0xA5).all())

    def adjacency(self, boundary=True):
        """-> (rc, inc_off, inc trimmed to n_incident, boundary, n_incident); the part of inc past n_incident must be untouched"""
        self.inc_off, self.inc = self.out((self.V + 1,), I32), self.out((3 * self.F,), I32)
        b = self.out((self.V,), U8) if boundary else None
        n = ctypes.c_int64(-7)
        rc = self.lib.nm_mesh_adjacency(P(self.faces), self.F, self.V, P(self.inc_off), P(self.inc), P(b), P(self.ws), self.nbytes, ctypes.byref(n), stream())
        assert self.intact()
        k = int(n.value)
        if rc == 0:
            assert 0 <= k <= 3 * self.F and bool((self.inc[k:] == SENTINEL).all())
        return rc, self.inc_off.cpu().numpy(), self.inc[:max(k, 0)].cpu().numpy(), None if b is None else b.cpu().numpy(), k

    def smooth(self, rows, iterations, lam, mu, hold=None):
        x = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
        h = None if hold is None else torch.from_numpy(np.ascontiguousarray(hold, np.uint8)).cuda()
        out, scratch = self.out(x.shape, F32), self.out(x.shape, F32)
        rc = self.lib.nm_mesh_smooth(P(x), int(x.shape[1]), self.V, P(self.faces), self.F, P(self.inc_off), P(self.inc), P(h), lam, mu, iterations, P(out),
                                     P(scratch), stream())
        assert rc == 0, self.lib.nm_last_error()
        assert self.intact() and same(x.cpu().numpy(), np.ascontiguousarray(rows, np.float32))               # the input is not written
        return out.cpu().numpy()

    def normals(self, verts):
        x = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).cuda()
        B = int(x.shape[0]) if x.dim() == 3 else 1
        out = self.out((B * self.V, 3), F32)
        rc = self.lib.nm_mesh_vertex_normals(P(x), B, self.V, P(self.faces), self.F, P(self.inc_off), P(self.inc), P(out), stream())
        assert rc == 0, self.lib.nm_last_error()
        assert self.intact()
        return out.cpu().numpy().reshape(tuple(x.shape))


def check_adjacency(faces, n_verts, want=None):
    want = want or SR.adjacency(faces, n_verts)
    d = Device(faces, n_verts)
    rc, off, inc, boundary, n = d.adjacency()
    assert rc == 0, d.lib.nm_last_error()
    assert n == want[1].shape[0] and same(off, want[0]) and same(inc, want[1]) and same(boundary, want[2])
    return d, want


# ---- 1: the hand-written mesh -------------------------------------------------------------------------------------------------------------
def test_hand_written_mesh():
    _lib.require_gpu()
    d, (off, inc, boundary) = check_adjacency(SS.HAND_FACES, SS.HAND_VERTS)
    assert same(off, SS.HAND_INC_OFF) and same(boundary, SS.HAND_BOUNDARY) and inc.shape[0] == SS.HAND_N_INCIDENT
    rc, off2, inc2, none, n = d.adjacency(boundary=False)                             # boundary is nullable
    assert rc == 0 and none is None and same(off2, off) and same(inc2, inc)
    hold = np.zeros(SS.HAND_VERTS, np.uint8)
    hold[[1, 9, 14]] = (1, 255, 2)
    for width in (1, 3, 4):
        x = SS.hand_rows(width)
        assert np.isnan(x).sum() == 1
        for iterations in (0, 1, 3):
            for lam, mu in (TAUBIN, (0.5, 0.0)):
                for h in (None, hold):
                    got = d.smooth(x, iterations, lam, mu, h)
                    assert same_rows(got, SR.smooth(x, SS.HAND_FACES, iterations, lam, mu, h)), (width, iterations, mu, h is not None)
                    if iterations == 0:
                        assert same(got, x)                                           # byte for byte, the NaN's payload included
                    if h is not None:
                        assert same(got[[1, 9, 14]], x[[1, 9, 14]])
    x = SS.hand_rows(3)
    assert within_one_step(d.normals(x), SR.vertex_normals(x, SS.HAND_FACES))
    clean = np.nan_to_num(x, nan=0.25)
    got = d.normals(clean)
    assert within_one_step(got, SR.vertex_normals(clean, SS.HAND_FACES)) and not got[18:].any() and got[:18].any(1).all()
    # no face at all, and no vertex
    none = np.zeros((0, 3), np.int32)
    e = Device(none, 5)
    rc, off, inc, boundary, n = e.adjacency()
    assert rc == 0 and n == 0 and off.tolist() == [0] * 6 and inc.shape == (0,) and boundary.tolist() == [0] * 5
    e = Device(none, 0)
    rc, off, inc, boundary, n = e.adjacency()
    assert rc == 0 and n == 0 and off.tolist() == [0]


# ---- 2: invalid indices: the defined refusal ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1, 'V', 2 ** 31 - 1, -2 ** 31])
def test_invalid_faces_are_counted_and_never_followed(bad):
    verts, faces = SS.grid_mesh(*SS.GRID_SMALL)
    V = verts.shape[0]
    broken = faces.copy()
    for f, k in ((1234, 2), (77, 0), (2000, 1)):                                      # not in index order: the LOWEST face is reported
        broken[f, k] = V if bad == 'V' else bad
    assert SR.invalid_faces(broken, V).tolist() == [77, 1234, 2000]
    d = Device(broken, V)
    rc, off, inc, boundary, n = d.adjacency()                                         # (asserts the guards, the workspace's included)
    msg = d.lib.nm_last_error().decode()
    assert rc == -1 and n == -7 and "nm_mesh_adjacency" in msg and "3 invalid faces" in msg and "face 77" in msg, msg
    d.faces.copy_(torch.from_numpy(faces))                                            # the next valid call on the same workspace
    rc, off, inc, boundary, n = d.adjacency()
    want = SR.adjacency(faces, V)
    assert rc == 0 and same(off, want[0]) and same(inc, want[1]) and same(boundary, want[2])
    # the entries that take lists follow no index that is out of range: lists of the valid mesh, faces with the bad indices
    d.faces.copy_(torch.from_numpy(broken))
    got = d.smooth(verts, 1, 0.5, 0.0)
    touched = np.unique(faces[[77, 1234, 2000]])                                      # the vertices whose lists name a broken face
    rest = np.setdiff1d(np.arange(V), touched)
    assert same_rows(got[rest], SR.smooth(verts, faces, 1, 0.5, 0.0)[rest]) and np.isfinite(got).all()
    normals = d.normals(verts)
    assert within_one_step(normals[rest], SR.vertex_normals(verts, faces)[rest]) and np.isfinite(normals).all()


# ---- 3: the scans past their sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["GRID_SMALL", "GRID_PAST_THE_SCAN"])
def test_grids_past_the_scans(grid):
    rows, cols = getattr(SS, grid)
    verts, faces = SS.grid_mesh(rows, cols)
    d, (off, inc, boundary) = check_adjacency(faces, rows * cols)
    assert np.array_equal(boundary.astype(bool), SS.grid_rim(rows, cols))
    assert same_rows(d.smooth(verts, 2, *TAUBIN, boundary), SR.smooth(verts, faces, 2, *TAUBIN, boundary))
    assert within_one_step(d.normals(verts), SR.vertex_normals(verts, faces))


# ---- 4: long lists ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valence", [SS.CONE_NEIGHBOURS_PAST, SS.CONE_JUST_PAST, SS.CONE_FAR_PAST])
@pytest.mark.parametrize("apex_last", [False, True])
def test_cones_past_the_in_thread_sort(valence, apex_last):
    verts, faces, apex = SS.cone(valence, apex_last)
    d, (off, inc, boundary) = check_adjacency(faces, valence + 1)
    assert all((np.diff(inc[off[v]:off[v + 1]]) > 0).all() for v in range(valence + 1))
    assert off[apex + 1] - off[apex] == valence and boundary[apex] == 0 and np.delete(boundary, apex).all()      # the rim only
    assert same_rows(d.smooth(verts, 1, 0.5, 0.0), SR.smooth(verts, faces, 1, 0.5, 0.0))
    assert within_one_step(d.normals(verts), SR.vertex_normals(verts, faces))


# ---- 5: determinism and the order of the faces' rows --------------------------------------------------------------------------------------
def test_determinism_and_face_order():
    verts, faces = SS.grid_mesh(*SS.GRID_SMALL)
    cone_verts, cone_faces, _ = SS.cone(SS.CONE_FAR_PAST, True)
    for x, f in ((verts, faces), (cone_verts, cone_faces), (SS.hand_rows(3), SS.HAND_FACES)):
        V = x.shape[0]
        runs = []
        for _ in range(2):
            d = Device(f, V)
            rc, off, inc, boundary, n = d.adjacency()
            assert rc == 0
            runs.append((off, inc, boundary, d.smooth(x, 3, *TAUBIN), d.normals(x)))
        assert all(same(a, b) for a, b in zip(*runs))
        perm = np.random.default_rng(SS.SEED + 5).permutation(f.shape[0])
        p = Device(f[perm], V)
        rc, off, inc, boundary, n = p.adjacency()
        assert rc == 0 and same(boundary, runs[0][2]) and same(off, runs[0][0])
        assert np.array_equal(np.sort(perm[inc[off[0]:off[1]]]), runs[0][1][off[0]:off[1]])      # the same faces under their new numbers


# ---- 6: frames ----------------------------------------------------------------------------------------------------------------------------
def test_normals_of_three_frames_are_three_single_calls():
    verts, faces = SS.grid_mesh(*SS.GRID_SMALL)
    rng = np.random.default_rng(SS.SEED + 6)
    frames = np.stack([verts, verts * np.float32(1.7) + rng.normal(size=verts.shape).astype(np.float32) * np.float32(0.1), verts[:, [2, 0, 1]].copy()])
    d = Device(faces, verts.shape[0])
    assert d.adjacency()[0] == 0
    batch = d.normals(frames)
    assert batch.shape == frames.shape and not same(batch[0], batch[1]) and not same(batch[0], batch[2])
    for b in range(3):
        assert same(batch[b], d.normals(frames[b])), b
    assert within_one_step(batch, SR.vertex_normals(frames, faces))


# ---- 7: what smoothing is for -------------------------------------------------------------------------------------------------------------
def test_taubin_takes_the_ripple_off_a_noisy_sphere_and_keeps_its_size():
    field = torch.from_numpy(SS.noisy_sphere_field()).cuda()
    verts, faces, grad_normals = mesh_extract.extract_mesh(field, SS.SPHERE_BOX, 0.0)
    before = faces.clone()
    adj = mesh_smooth.adjacency(faces, verts.shape[0])
    assert isinstance(adj, mesh_smooth.Adjacency) and (adj.n_verts, adj.n_faces) == (verts.shape[0], faces.shape[0]) and not bool(adj.boundary.any())
    assert adj.inc.shape[0] == 3 * faces.shape[0]
    taubin = mesh_smooth.smooth_mesh(verts, faces, 10, adj=adj)
    laplace = mesh_smooth.smooth_mesh(verts, faces, 10, mu=0.0, adj=adj)
    assert torch.equal(faces, before) and torch.equal(taubin, mesh_smooth.smooth_mesh(verts, faces))     # the defaults; adj built inside
    r0, dev0 = SR.radial(verts.cpu().numpy(), SS.SPHERE_CENTRE)
    r1, dev1 = SR.radial(taubin.cpu().numpy(), SS.SPHERE_CENTRE)
    r2, dev2 = SR.radial(laplace.cpu().numpy(), SS.SPHERE_CENTRE)
    assert dev1 < dev0                                                                # smoother ...
    assert abs(r1 - r0) < abs(r2 - r0)                                                # ... and it shrinks less than plain Laplacian steps do
    normals = mesh_smooth.vertex_normals(taubin, faces, adj=adj)
    assert bool(((normals.double() * grad_normals.double()).sum(1) > 0).all())
    assert same_rows(taubin.cpu().numpy(), SR.smooth(verts.cpu().numpy(), faces.cpu().numpy(), 10, *TAUBIN))
    # the Python surface: [B,V,3], fixed and pin_boundary, an adj of another mesh
    both = mesh_smooth.vertex_normals(torch.stack([taubin, verts]), faces, adj=adj)
    assert both.shape == (2,) + tuple(verts.shape) and torch.equal(both[0], normals) and torch.equal(both[1], mesh_smooth.vertex_normals(verts, faces))
    fixed = torch.zeros(verts.shape[0], dtype=torch.bool, device='cuda')
    fixed[::3] = True
    held = mesh_smooth.smooth_mesh(verts, faces, 2, fixed=fixed, adj=adj)
    assert torch.equal(held[::3], verts[::3]) and bool((held[1::3] != verts[1::3]).any(1).all())
    with pytest.raises(_lib.NeumanHipError):
        mesh_smooth.smooth_mesh(verts[:-1].contiguous(), faces, adj=adj)
    open_verts, open_faces = (torch.from_numpy(a).cuda() for a in SS.grid_mesh(5, 4))
    rim = torch.from_numpy(SS.grid_rim(5, 4)).cuda()
    pinned = mesh_smooth.smooth_mesh(open_verts, open_faces, 2)
    free = mesh_smooth.smooth_mesh(open_verts, open_faces, 2, pin_boundary=False)
    assert torch.equal(pinned[rim], open_verts[rim]) and bool((free[rim] != open_verts[rim]).any(1).all())
    with pytest.raises(_lib.NeumanHipError):
        mesh_smooth.adjacency(torch.cat([open_faces, torch.tensor([[0, 1, 20]], device='cuda', dtype=I32)]), 20)


# ---- 8: extract_net_mesh ------------------------------------------------------------------------------------------------------------------
def test_extract_net_mesh_smooths_after_the_clean_up():
    net = synthetic.make_joiner(0).cuda()
    box, res = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), 24
    field = mesh_extract.density_grid(net, box, res)
    level = float(field.reshape(-1).quantile(0.9))
    plain = mesh_extract.extract_mesh(field, box, level)
    assert plain[0].shape[0] > 0
    with torch.no_grad():
        colours = torch.sigmoid(net(plain[0], -plain[2] if net.nerf.use_viewdirs else None)[..., :3])
    # smooth omitted or 0: today's four outputs, tensor for tensor
    for kw in ({}, dict(smooth=0)):
        assert all(torch.equal(a, b) for a, b in zip(mesh_extract.extract_net_mesh(net, box, res, level, **kw), plain + (colours,))), kw
    # smooth = 3: the chain by hand
    v, f, nrm, col = mesh_extract.extract_net_mesh(net, box, res, level, largest=1, smooth=3)
    cv, cf, cn = mesh_extract.clean_mesh(*plain[:2], plain[2])
    sv = mesh_smooth.smooth_mesh(cv, cf, 3)
    sn = mesh_smooth.vertex_normals(sv, cf)
    with torch.no_grad():
        want = torch.sigmoid(net(sv, -sn if net.nerf.use_viewdirs else None)[..., :3])
    assert torch.equal(f, cf) and torch.equal(v, sv) and torch.equal(nrm, sn) and torch.equal(col, want)
    assert not torch.equal(sv, cv) and not torch.equal(sn, cn) and col.shape == (v.shape[0], 3)
