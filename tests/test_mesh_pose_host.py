"""Without a device: nm_mesh_pose_batch is exported and refuses bad arguments before any device work, the Python surface over it
(neuman_hip/mesh_pose.py) refuses CPU tensors, and the numpy restatement of the contract (tests/helpers/mesh_pose_ref.py) -- the yardstick of
tests/test_hip_mesh_pose.py -- gives what the rules say on inputs whose answer is known."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mesh_pose_ref as PR  # noqa: E402

from neuman_hip import _lib, mesh_pose  # noqa: E402

TOO_MANY = 1 << 31


def _host_block(nbytes):
    block = (ctypes.c_char * (nbytes + 64))()
    return block, ctypes.c_void_p((ctypes.addressof(block) + 15) // 16 * 16)


def _call(lib, a):
    return lib.nm_mesh_pose_batch(a['T'], a['t_f64'], a['t_rows'], a['B'], a['tri'], a['bary'], a['per_frame'], a['pts'], a['normals'], a['N'],
                                  a['out_pts'], a['out_normals'], a['n_invalid'], None)


def test_the_library_exports_the_entry():
    assert hasattr(_lib.lib(), "nm_mesh_pose_batch") and "nm_mesh_pose_batch" in _lib.SIGNATURES


def test_entry_refuses_bad_arguments_before_any_device_work():
    lib = _lib.lib()
    # the checks run before any pointer is followed: a block of host memory stands in for the device arrays
    block, d = _host_block(4096)
    good = dict(T=d, t_f64=1, t_rows=55, B=3, tri=d, bary=d, per_frame=0, pts=d, normals=d, N=7, out_pts=d, out_normals=d, n_invalid=None)
    bad = [dict(T=None), dict(tri=None), dict(bary=None), dict(pts=None), dict(out_pts=None),                       # a null required pointer, N > 0
           dict(normals=None), dict(out_normals=None),                                                              # one of the pair without the other
           dict(B=0), dict(B=-1), dict(B=65536), dict(N=-1), dict(N=TOO_MANY), dict(t_rows=0), dict(t_rows=-1), dict(t_rows=TOO_MANY),
           dict(t_f64=2), dict(t_f64=-1), dict(per_frame=2), dict(per_frame=-1),
           dict(T=ctypes.c_void_p(d.value + 8))]                                                                    # the 16-byte loads need an aligned table
    for over in bad:
        for base in (good, dict(good, normals=None, out_normals=None), dict(good, t_f64=0), dict(good, per_frame=1)):
            if ('normals' in over or 'out_normals' in over) and base['normals'] is None:
                continue
            rc = _call(lib, dict(base, **over))
            assert rc == -1 and b"nm_mesh_pose_batch" in lib.nm_last_error(), (over, rc, lib.nm_last_error())
    del block


def test_no_vertices_need_no_device():
    lib = _lib.lib()
    block, d = _host_block(256)
    none = dict(T=None, t_f64=1, t_rows=1, B=1, tri=None, bary=None, per_frame=0, pts=None, normals=None, N=0, out_pts=None, out_normals=None, n_invalid=None)
    assert _call(lib, none) == 0
    assert _call(lib, dict(none, T=d, tri=d, bary=d, pts=d, normals=d, out_pts=d, out_normals=d, n_invalid=d, B=65535, t_rows=TOO_MANY - 1, t_f64=0, per_frame=1)) == 0
    # ... but the sizes and switches are still checked
    for over in (dict(B=0), dict(t_rows=0), dict(t_f64=3), dict(per_frame=3)):
        assert _call(lib, dict(none, **over)) == -1 and b"nm_mesh_pose_batch" in lib.nm_last_error(), over
    del block


def test_cpu_tensors_are_refused():
    """(with or without a device in the machine: the tensors are what is refused)"""
    verts = torch.zeros(5, 3)
    body = torch.eye(3)
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(_lib.NeumanHipError):
        mesh_pose.bind_mesh(verts, body, faces)
    with pytest.raises(_lib.NeumanHipError):
        mesh_pose.bind_mesh(verts.numpy(), body.numpy(), faces.numpy())
    binding = mesh_pose.Binding(torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5, 3))
    T = torch.eye(4, dtype=torch.float64).expand(2, 3, 4, 4).contiguous()
    with pytest.raises(_lib.NeumanHipError):
        mesh_pose.pose_mesh(verts, binding, T)
    with pytest.raises(_lib.NeumanHipError):
        mesh_pose.pose_mesh(verts, binding, T, normals=verts, check=True)
    with pytest.raises(_lib.NeumanHipError):
        mesh_pose.pose_mesh_frames(None, np.zeros((2, 72), np.float32), np.zeros((2, 10), np.float32), np.zeros((2, 4, 4)), 1.0, verts, binding)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def test_identity_returns_the_points_bit_for_bit():
    rng = np.random.default_rng(5)
    pts = (rng.normal(size=(40, 3)) * 10.0 ** rng.integers(-3, 4, size=(40, 1))).astype(np.float32)
    pts[0] = (0.0, 1e-30, 1e3)                                                     # (a -0 would come out +0: the sum with the zero products)
    tri = rng.integers(0, 6, size=(40, 3)).astype(np.int32)
    bary = np.tile(np.array([1, 0, 0], np.float32), (40, 1))
    for dtype in (np.float64, np.float32):
        T = np.tile(np.eye(4, dtype=dtype), (2, 6, 1, 1))
        out, nrm, bad = PR.pose(T, tri, bary, pts)
        assert nrm is None and bad == 0 and out.dtype == np.float32 and out.shape == (2, 40, 3)
        assert np.array_equal(out.view(np.uint32), np.broadcast_to(pts, (2, 40, 3)).copy().view(np.uint32))
        out, nrm, bad = PR.pose(T, tri, bary, pts, pts)                            # the identity's cofactor matrix is the identity: n / |n|
        unit = (pts.astype(np.float64) / np.linalg.norm(pts.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        assert PR.ulp_distance(nrm, np.broadcast_to(unit, nrm.shape)).max() <= 1


def test_one_rotation_in_every_row_rotates_unit_normals():
    rng = np.random.default_rng(6)
    R = _rotation((0.3, -1.0, 0.5), 0.9)
    T = np.tile(np.eye(4), (1, 9, 1, 1))
    T[..., :3, :3] = R
    T[..., :3, 3] = (0.5, -2.0, 4.0)
    n = rng.normal(size=(64, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    bary = rng.uniform(0.05, 1, size=(64, 3))
    bary = (bary / bary.sum(1, keepdims=True)).astype(np.float32)
    tri = rng.integers(0, 9, size=(64, 3)).astype(np.int32)
    pts = rng.normal(size=(64, 3)).astype(np.float32)
    out, nrm, bad = PR.pose(T, tri, bary, pts, n)
    assert bad == 0
    want = (n.astype(np.float64) @ R.T).astype(np.float32)                         # R n: a rotation is its own cofactor matrix
    assert PR.ulp_distance(nrm[0], want).max() <= 1
    assert np.abs(out[0] - (pts.astype(np.float64) @ R.T + T[0, 0, :3, 3])).max() < 1e-5      # (the weights sum to one only to float32)


def test_restatement_follows_the_other_rules():
    rng = np.random.default_rng(7)
    T = rng.normal(size=(2, 5, 4, 4))
    pts = rng.normal(size=(6, 3)).astype(np.float32)
    nrm = rng.normal(size=(6, 3)).astype(np.float32)
    tri = rng.integers(0, 5, size=(6, 3)).astype(np.int32)
    bary = rng.normal(size=(6, 3)).astype(np.float32)
    tri[1, 2], tri[4, 0] = 5, -1                                                   # rule P5
    nrm[2] = 0                                                                     # rule P4: s = 0
    out, on, bad = PR.pose(T, tri, bary, pts, nrm)
    assert bad == 4 and np.isnan(out[:, [1, 4]]).all() and np.isnan(on[:, [1, 4]]).all()
    assert np.isfinite(out[:, [0, 2, 3, 5]]).all() and (on[:, 2] == 0).all() and np.isfinite(on[:, [0, 3, 5]]).all()
    # the stated association, spelled out for one vertex and frame
    w = bary[3].astype(np.float64)
    M = (w[0] * T[1, tri[3, 0]] + w[1] * T[1, tri[3, 1]]) + w[2] * T[1, tri[3, 2]]
    x, y, z = pts[3].astype(np.float64)
    want = [np.float32(((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]) for r in range(3)]
    assert out[1, 3].tolist() == want
    # a reflection flips the normal the linear map alone would give: the cofactor matrix of diag(-1, 1, 1) is diag(1, -1, -1)
    F = np.tile(np.diag([-1.0, 1.0, 1.0, 1.0]), (1, 5, 1, 1))
    one = np.tile(np.array([1, 0, 0], np.float32), (6, 1))
    _, on, _ = PR.pose(F, np.clip(tri, 0, 4), one, pts, np.tile(np.array([0.6, 0.8, 0.0], np.float32), (6, 1)))
    assert PR.ulp_distance(on[0], np.tile(np.array([0.6, -0.8, 0.0], np.float32), (6, 1))).max() <= 1
    # a binding per frame, and a frame is its own slice
    tri_b = rng.integers(0, 5, size=(2, 6, 3)).astype(np.int32)
    bary_b = rng.normal(size=(2, 6, 3)).astype(np.float32)
    both = PR.pose(T, tri_b, bary_b, pts, nrm)
    for b in range(2):
        alone = PR.pose(T[b:b + 1], tri_b[b], bary_b[b], pts, nrm)
        assert np.array_equal(both[0][b].view(np.uint32), alone[0][0].view(np.uint32)) and np.array_equal(both[1][b].view(np.uint32), alone[1][0].view(np.uint32))
