"""-m gpu: the mesh pose kernel (ml-neuman_amd/csrc/mesh_pose.hip) through the C ABI against the numpy restatement of the header's rules
P2-P5 (tests/helpers/mesh_pose_ref.py), and the Python surface over it (neuman_hip/mesh_pose.py: bind_mesh, pose_mesh, pose_mesh_frames).

The comparison rule of every case: POINTS equal the restatement bit for bit -- on the device the point path is IEEE float64 multiply and add
without contraction and one rounding conversion, and numpy does the same.  NORMALS are within 1 float32 ulp per component: whether the
device's float64 square root and divide are correctly rounded is not something this project has established, and an error of a few float64
ulps moves the float32 result by at most one step.  Every output of a raw call lies inside a larger allocation with sentinel guard rows
before and after."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import isosurface_ref as IR  # noqa: E402
import mesh_pose_ref as PR  # noqa: E402

from neuman_hip import _lib, mesh_extract, mesh_pose, raster, ray_utils, smpl, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC5A5A5            # a quiet NaN with a payload; the kernel's own NaN is 0x7FC00000
GUARD = 67                       # guard rows before and after every output
SLACK = 7.0                      # what the slack rows around a transform table hold (case 4)
ROWS, BODY = 55, 50              # case 1's table: 55 rows over 50 "vertices", as nm_smpl_frames' V + J over V


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))


def guarded(rows):
    buf = torch.empty((rows + 2 * GUARD, 3), device='cuda', dtype=torch.float32)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf):
    b = buf.view(torch.int32)
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())


def dev(a):
    return None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda())


def run(T, tri, bary, pts, normals=None, count=True):
    """one raw nm_mesh_pose_batch call -> (out_pts [B,N,3], out_normals or None, n_invalid or None) as numpy; T a device tensor or numpy"""
    T, tri, bary, pts, normals = dev(T), dev(tri), dev(bary), dev(pts), dev(normals)
    B, rows, N = int(T.shape[0]), int(T.shape[1]), int(pts.shape[0])
    assert T.is_contiguous() and T.dtype in (torch.float64, torch.float32)
    op_buf, op = guarded(B * N)
    on_buf, on = guarded(B * N) if normals is not None else (None, None)
    counter = torch.zeros((1,), device='cuda', dtype=torch.int32) if count else None
    rc = _lib.lib().nm_mesh_pose_batch(P(T), 1 if T.dtype == torch.float64 else 0, rows, B, P(tri), P(bary), 1 if tri.dim() == 3 else 0, P(pts), P(normals), N,
                                       P(op), P(on), P(counter), stream())
    assert rc == 0, _lib.lib().nm_last_error()
    torch.cuda.synchronize()
    assert guards_intact(op_buf) and (on_buf is None or guards_intact(on_buf))
    return (op.cpu().numpy().reshape(B, N, 3), None if on is None else on.cpu().numpy().reshape(B, N, 3), None if counter is None else int(counter.item()))


def check(got, want, what=""):
    """the comparison rule: points bit for bit, normals within 1 ulp, the same count of invalid rows"""
    assert same_bits(got[0], want[0]), (what, int((bits(got[0]) != bits(want[0])).sum()), float(np.nanmax(np.abs(got[0] - want[0]))))
    assert (got[1] is None) == (want[1] is None), what
    if want[1] is not None:
        d = PR.ulp_distance(got[1], want[1])
        assert d.max() <= 1, (what, int(d.max()), int((d > 1).sum()))
    assert got[2] is None or got[2] == want[2], (what, got[2], want[2])


def edge_inputs(N, B, seed, per_frame=False, rows=ROWS, body=BODY):
    """random general affine transforms (not only rigid) with entries of mixed magnitude; barycentrics with exact (1,0,0), negative entries
    and sums != 1; points up to 1e3; indices that name the last "vertex" row and the rows beyond it"""
    rng = np.random.default_rng(seed)
    T = rng.normal(size=(B, rows, 4, 4)) * 10.0 ** rng.integers(-2, 3, size=(B, rows, 4, 4))
    lead = (B, N) if per_frame else (N,)
    tri = rng.integers(0, body, size=lead + (3,)).astype(np.int32)
    bary = rng.normal(size=lead + (3,)).astype(np.float32)
    flat_t, flat_b = tri.reshape(-1, 3), bary.reshape(-1, 3)
    n = flat_t.shape[0]
    flat_b[::5] = (1.0, 0.0, 0.0)
    flat_b[1::7] = np.abs(flat_b[1::7]) / np.abs(flat_b[1::7]).sum(1, keepdims=True)          # a proper convex combination (to float32)
    flat_t[rng.integers(0, n, max(1, n // 6)), rng.integers(0, 3, max(1, n // 6))] = body - 1
    flat_t[rng.integers(0, n, max(1, n // 6)), rng.integers(0, 3, max(1, n // 6))] = rng.integers(body, rows, max(1, n // 6))
    flat_t[-1] = (rows - 1, body - 1, 0)
    pts = (rng.normal(size=(N, 3)) * 10.0 ** rng.integers(-2, 3, size=(N, 1))).astype(np.float32)
    pts[0] = (1e3, -1e3, 999.5)
    normals = rng.normal(size=(N, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    if N > 2:
        normals[2] = 0                                                                         # rule P4: s = 0 -> (0, 0, 0)
    return T, tri, bary, pts, normals


# ---- 1: block edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_block_edges(N, B):
    T, tri, bary, pts, normals = edge_inputs(N, B, seed=N * 10 + B)
    assert (tri == BODY - 1).any() and (tri >= BODY).any() and tri.max() == ROWS - 1
    for table in (T, T.astype(np.float32)):
        for nrm in (None, normals):
            want = PR.pose(table, tri, bary, pts, nrm)
            assert want[2] == 0 and np.isfinite(want[0]).all()
            check(run(table, tri, bary, pts, nrm), want, (table.dtype, nrm is not None))
    if N > 2:
        assert (PR.pose(T, tri, bary, pts, normals)[1][:, 2] == 0).all()
    check(run(T, tri, bary, pts, normals, count=False), PR.pose(T, tri, bary, pts, normals), "n_invalid is nullable")


# ---- 2: a binding per frame ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [True, False])
def test_per_frame_bindings(f64):
    T, tri, bary, pts, normals = edge_inputs(300, 3, seed=21, per_frame=True)
    assert tri.shape == (3, 300, 3) and not np.array_equal(tri[0], tri[1])
    table = T if f64 else T.astype(np.float32)
    check(run(table, tri, bary, pts, normals), PR.pose(table, tri, bary, pts, normals))
    check(run(table, tri, bary, pts), PR.pose(table, tri, bary, pts))


# ---- 3: frame independence ----------------------------------------------------------------------------------------------------------------
def test_a_frame_is_its_own_slice():
    T, tri, bary, pts, normals = edge_inputs(700, 3, seed=31)
    for table in (T, T.astype(np.float32)):
        whole = run(table, tri, bary, pts, normals)
        alone = run(np.ascontiguousarray(table[2:3]), tri, bary, pts, normals)
        assert same_bits(whole[0][2:3], alone[0]) and same_bits(whole[1][2:3], alone[1])
    Tp, trip, baryp, ptsp, nrmp = edge_inputs(700, 3, seed=32, per_frame=True)
    whole = run(Tp, trip, baryp, ptsp, nrmp)
    alone = run(np.ascontiguousarray(Tp[2:3]), np.ascontiguousarray(trip[2]), np.ascontiguousarray(baryp[2]), ptsp, nrmp)
    assert same_bits(whole[0][2:3], alone[0]) and same_bits(whole[1][2:3], alone[1])


# ---- 4: rule P5, without risking a fault ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [True, False])
def test_invalid_rows_are_counted_and_never_followed(f64):
    """The rows just outside a frame's table are allocated memory holding SLACK: a broken guard would show up as a finite value where NaN is
    due, not as an illegal access.  The entry takes the frames back to back, so in the B-frame call the slack of an inner frame is its
    neighbour's first or last row (allocated too) and only the two ends hold SLACK; the one-frame calls below put SLACK on both sides of
    every frame's table."""
    B, N = 3, 1000
    T, tri, bary, pts, normals = edge_inputs(N, B, seed=41)
    dtype = torch.float64 if f64 else torch.float32
    flat = torch.full((1 + B * ROWS + 1, 4, 4), SLACK, device='cuda', dtype=dtype)
    inner = flat[1:-1].view(B, ROWS, 4, 4)
    inner.copy_(torch.from_numpy(T))
    assert inner.is_contiguous() and inner.data_ptr() % 16 == 0
    table = inner.cpu().numpy()
    valid = run(inner, tri, bary, pts, normals)
    check(valid, PR.pose(table, tri, bary, pts, normals))
    assert valid[2] == 0
    where = [(3, 0, -1), (100, 2, ROWS), (255, 1, -1), (256, 0, ROWS), (999, 2, -1), (999, 0, ROWS)]      # (vertex, corner, index): 5 vertices
    bad_tri = tri.copy()
    for v, k, index in where:
        bad_tri[v, k] = index
    rows_bad = sorted({v for v, _, _ in where})
    got = run(inner, bad_tri, bary, pts, normals)
    assert got[2] == len(rows_bad) * B
    check(got, PR.pose(table, bad_tri, bary, pts, normals))
    keep = np.ones(N, bool)
    keep[rows_bad] = False
    for g, v in ((got[0], valid[0]), (got[1], valid[1])):
        assert (bits(g[:, rows_bad]) == 0x7FC00000).all()
        assert same_bits(np.ascontiguousarray(g[:, keep]), np.ascontiguousarray(v[:, keep]))
    # every frame with SLACK on both sides of its own table: one-frame calls, one counter
    padded = torch.full((B, ROWS + 2, 4, 4), SLACK, device='cuda', dtype=dtype)
    padded[:, 1:-1].copy_(inner)
    total = 0
    for b in range(B):
        one = run(padded[b, 1:-1][None], bad_tri, bary, pts, normals)
        assert same_bits(one[0][0], got[0][b]) and same_bits(one[1][0], got[1][b])
        total += one[2]
    assert total == len(rows_bad) * B
    # the Python surface: the same outputs, and check=True names the count
    binding = mesh_pose.Binding(dev(bad_tri), dev(bary))
    posed, posed_n = mesh_pose.pose_mesh(dev(pts), binding, inner, normals=dev(normals))
    assert same_bits(posed.cpu().numpy(), got[0]) and same_bits(posed_n.cpu().numpy(), got[1])
    with pytest.raises(_lib.NeumanHipError, match=str(len(rows_bad) * B)):
        mesh_pose.pose_mesh(dev(pts), binding, inner, check=True)
    fine = mesh_pose.pose_mesh(dev(pts), mesh_pose.Binding(dev(tri), dev(bary)), inner, check=True)
    assert same_bits(fine.cpu().numpy(), valid[0])
    assert bool((flat[0] == SLACK).all()) and bool((flat[-1] == SLACK).all())


# ---- 5: T straight from the body model ----------------------------------------------------------------------------------------------------
def test_transforms_straight_from_the_body_model():
    body = smpl.SMPL(synthetic.smpl_like_model(), device='cuda')
    poses, betas, align = synthetic.smpl_like_frames(3)
    aligns = np.tile(np.eye(4), (3, 1, 1))
    for i, name in enumerate(sorted(align)):
        aligns[i][:, :3] = align[name]
    scale = 1.25
    T, world, static = body.frames(poses, betas, aligns, scale, True)
    V = body.V
    assert T.dtype == torch.float64 and tuple(T.shape) == (3, V + body.J, 4, 4)
    pts = static[0, :V].contiguous()
    ids = torch.arange(V, device='cuda', dtype=torch.int32)
    binding = mesh_pose.Binding(ids[:, None].expand(V, 3).contiguous(), torch.tensor([1.0, 0.0, 0.0], device='cuda').expand(V, 3).contiguous())
    posed = mesh_pose.pose_mesh(pts, binding, T)
    want = PR.pose(T.cpu().numpy(), binding.tri.cpu().numpy(), binding.bary.cpu().numpy(), pts.cpu().numpy())      # M is T_i exactly under rule P2
    assert same_bits(posed.cpu().numpy(), want[0])
    # the map means what the header says: frame 0's canonical vertices land on frame 0's world vertices (computed by another kernel in
    # another order: a few float32 steps of coordinates of order one)
    assert float((posed[0] - world[0, :V]).abs().max()) < 1e-4
    chunked = mesh_pose.pose_mesh_frames(body, poses, betas, aligns, scale, pts, binding, frames_per_call=2)       # chunks of 2 + 1
    assert torch.equal(chunked.view(torch.int32), posed.view(torch.int32))
    nrm = torch.nn.functional.normalize(pts, dim=1).contiguous()
    both = mesh_pose.pose_mesh_frames(body, poses, betas, aligns, scale, pts, binding, normals=nrm, frames_per_call=1)
    whole = mesh_pose.pose_mesh(pts, binding, T, normals=nrm)
    assert torch.equal(both[0].view(torch.int32), posed.view(torch.int32)) and torch.equal(both[1].view(torch.int32), whole[1].view(torch.int32))
    check((whole[0].cpu().numpy(), whole[1].cpu().numpy(), None), PR.pose(T.cpu().numpy(), binding.tri.cpu().numpy(), binding.bary.cpu().numpy(),
                                                                         pts.cpu().numpy(), nrm.cpu().numpy()))


# ---- 6, 7: end to end at the smallest useful size, twice ------------------------------------------------------------------------------------
BOX = (-0.4, -0.75, -0.3, 0.4, 0.75, 0.3)
OFFSET = 0.05


def end_to_end():
    """extract -> clean -> bind -> pose -> rasterise on the surface OFFSET outside synthetic.capsule_mesh(12, 10) -> every result as numpy"""
    body_v, body_f = synthetic.capsule_mesh(12, 10)
    body = ray_utils.Mesh(body_v, body_f, None, torch.device('cuda'))
    grid = torch.from_numpy(IR.grid_points((24, 24, 24), BOX).astype(np.float32)).cuda()
    sdist = ray_utils.signed_distance_dev(grid.reshape(-1, 3), body)[0]
    field = (OFFSET - sdist).reshape(24, 24, 24).contiguous()                         # positive inside the offset surface
    verts, faces, normals = mesh_extract.clean_mesh(*mesh_extract.extract_mesh(field, BOX, 0.0))
    faces_before = faces.clone()
    binding = mesh_pose.bind_mesh(verts, body_v, body_f)
    T = torch.from_numpy(np.stack([synthetic.twist_transforms(body_v, twist)[1] for twist in (0.8, -0.5)])).cuda()
    posed, posed_n = mesh_pose.pose_mesh(verts, binding, T, normals=normals, check=True)
    cap = synthetic.SimpleCapture(32, 32, c2w=synthetic.spherical_c2w(30, -20, 4.0), far=8.0)
    face_id = raster.Rasterizer(faces, verts.shape[0]).rasterize(posed[0], raster.camera_of(cap), want_bary=False)[0]
    out = dict(verts=verts, faces=faces, normals=normals, faces_before=faces_before, tri=binding.tri, bary=binding.bary, face=binding.face,
               sdist=binding.sdist, T=T, posed=posed, posed_n=posed_n, face_id=face_id)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    # binding.bary is what a direct nm_bary_forward call gives for the device's own closest points
    s, f, closest = ray_utils.signed_distance_dev(verts, body)
    bary = torch.empty_like(verts)
    _lib.check(_lib.lib().nm_bary_forward(P(body.verts), P(binding.tri), P(closest), verts.shape[0], P(bary), stream()), "nm_bary_forward")
    out.update(direct_bary=bary.cpu().numpy(), direct_face=f.cpu().numpy(), direct_sdist=s.cpu().numpy(), body_f=np.asarray(body_f, np.int32))
    return out


@pytest.fixture(scope="module")
def first_run():
    return end_to_end()


def test_end_to_end(first_run):
    r = first_run
    N = r['verts'].shape[0]
    assert N > 100 and r['faces'].shape[0] > 200 and r['T'].shape == (2, 122, 4, 4)
    assert np.array_equal(r['tri'], r['body_f'][r['face']]) and r['tri'].dtype == np.int32 and r['tri'].shape == (N, 3)
    assert same_bits(r['bary'], r['direct_bary']) and np.array_equal(r['face'], r['direct_face']) and same_bits(r['sdist'], r['direct_sdist'])
    assert np.abs(r['sdist'] - OFFSET).max() < 0.02                                   # the mesh is the offset surface, to within the grid's resolution
    want = PR.pose(r['T'], r['tri'], r['bary'], r['verts'], r['normals'])
    assert want[2] == 0
    check((r['posed'], r['posed_n'], None), want)
    assert np.array_equal(r['faces'], r['faces_before'])
    assert np.isfinite(r['posed']).all() and np.abs(np.linalg.norm(r['posed_n'], axis=-1) - 1).max() < 1e-6
    assert r['face_id'].shape == (32, 32) and (r['face_id'] >= 0).any() and r['face_id'].max() < r['faces'].shape[0]      # plumbing only


def test_determinism(first_run):
    again = end_to_end()
    assert sorted(again) == sorted(first_run)
    for k, a in again.items():
        assert a.dtype == first_run[k].dtype and a.tobytes() == first_run[k].tobytes(), k
