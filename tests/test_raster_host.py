"""Without a device: the float64 restatement of the rasteriser's contract (tests/helpers/raster_ref.py) against a triangle whose coverage and
depth are known in closed form, the new entry points' argument checks, and the Python surface (install(), the CPU refusal)."""
import ctypes
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import raster_ref as RR  # noqa: E402

from neuman_hip import _lib  # noqa: E402

EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_helper_on_a_triangle_with_analytic_coverage_and_depth(dtype):
    """(0,0,2), (4,0,4), (0,2,2) through fx = fy = 8, cx = cy = 0 land on (0,0), (8,0), (0,8) of an 8 x 8 image: the centre of pixel (r, c) is
    covered iff c + r <= 7 (the hypotenuse passes through the centres with c + r = 7, which rule 2's >= 0 keeps), 1/z is linear on the screen:
    z = 1 / (1/2 - u/32), and b' follows from b = (1 - u/8 - v/8, u/8, v/8)."""
    verts = np.array([[0, 0, 2], [4, 0, 4], [0, 2, 2]], np.float32)
    faces = np.array([[0, 1, 2]])
    for brute in (False, True):
        r = RR.rasterize(verts, faces, (EYE, 8.0, 8.0, 0.0, 0.0, 8, 8), dtype, brute=brute, analyse=True)
        rr, cc = np.mgrid[0:8, 0:8]
        want = cc + rr <= 7
        assert np.array_equal(r['face_id'] >= 0, want) and np.array_equal(r['face_id'][want], np.zeros(int(want.sum()), np.int32))
        u, v = cc + 0.5, rr + 0.5
        z = 1.0 / (0.5 - u / 32)
        assert np.all(np.isinf(r['zbuf'][~want])) and np.abs(r['zbuf'][want] - z[want]).max() < (1e-12 if dtype is np.float64 else 1e-5)
        b = np.stack([1 - u / 8 - v / 8, u / 8, v / 8], -1) / np.array([2.0, 4.0, 2.0])
        b = b / b.sum(-1, keepdims=True)
        assert np.abs(r['bary'][want] - b[want]).max() < (1e-12 if dtype is np.float64 else 1e-5)
        assert np.all(r['rgba'][~want] == np.array([1, 1, 1, 0])) and np.all(r['rgba'][want][:, 3] == 1)
        col = r['rgba'][want][:, 0]
        assert np.all((col >= 0.5) & (col <= 1.0 + 1e-6)) and np.all(r['rgba'][want][:, 1] == col)
        assert np.array_equal(r['ambiguous'], cc + rr == 7)                      # exactly the pixels whose centre is on an edge
    img = np.arange(8 * 8 * 3, dtype=np.uint8).reshape(8, 8, 3)
    o = RR.overlay(r['rgba'], img)
    assert np.array_equal(o[~want], img[~want]) and np.array_equal(o[want][:, 0], np.uint8(r['rgba'][want][:, 0] * dtype(255)))


def test_helper_rules_on_small_cases():
    cam = (EYE, 8.0, 8.0, 4.0, 4.0, 8, 8)
    tri = np.array([[-1, -1, 2], [1, -1, 2], [0, 1, 2]], np.float32)
    # a vertex at z <= 0 drops the face whole; zero screen area is skipped; back faces are kept
    for z0 in (0.0, -1.0):
        behind = tri.copy()
        behind[0, 2] = z0
        assert (RR.rasterize(behind, [[0, 1, 2]], cam)['face_id'] == -1).all()
    assert (RR.rasterize(np.array([[0, 0, 2], [1, 1, 2], [2, 2, 2]], np.float32), [[0, 1, 2]], cam)['face_id'] == -1).all()
    a, b = RR.rasterize(tri, [[0, 1, 2]], cam), RR.rasterize(tri, [[0, 2, 1]], cam)
    assert (a['face_id'] >= 0).sum() > 4 and np.array_equal(a['face_id'], b['face_id']) and np.array_equal(a['zbuf'], b['zbuf'])
    # nearest wins; on an exact tie the lower index
    two = np.concatenate([tri, tri * np.array([1, 1, 0.5], np.float32)])
    assert set(np.unique(RR.rasterize(two, [[0, 1, 2], [3, 4, 5]], cam)['face_id'])) == {-1, 1}
    tie = RR.rasterize(np.concatenate([tri, tri]), [[3, 4, 5], [0, 1, 2]], cam, analyse=True)
    assert set(np.unique(tie['face_id'])) == {-1, 0} and tie['ambiguous'][tie['face_id'] == 0].all()
    # the area-weighted vertex normal of a flat fan is its plane's normal
    n = RR.vertex_normals(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-3, 0, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]]))
    assert np.allclose(n, [[0, 0, 1]] * 4)


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    lib = _lib.lib()
    faces = np.array([[0, 1, 2]], np.int32)
    fp = faces.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    for args in ((None, 1, 3, ctypes.byref(h)), (fp, 1, 3, None), (fp, 0, 3, ctypes.byref(h)), (fp, 1, 0, ctypes.byref(h)), (fp, 1, 2, ctypes.byref(h))):
        assert lib.nm_raster_create(*args) == -1 and b"nm_raster_create" in lib.nm_last_error() and not h.value, args
    assert lib.nm_raster_destroy(None) == 0
    # the checks run before the handle or any pointer is looked at: a block of host memory stands in for them
    dummy = (ctypes.c_char * 256)()
    d = ctypes.cast(dummy, ctypes.c_void_p)
    w2c = (ctypes.c_double * 12)(*EYE.reshape(-1))
    light = (ctypes.c_double * 3)(2, 2, -2)
    bad_mesh = [(None, d, w2c, 8, 8, d, d), (d, None, w2c, 8, 8, d, d), (d, d, None, 8, 8, d, d), (d, d, w2c, 0, 8, d, d), (d, d, w2c, 8, 0, d, d),
                (d, d, w2c, -4, 8, d, d), (d, d, w2c, 8, 8, None, d), (d, d, w2c, 8, 8, d, None)]
    for hh, v, m, W, H, fid, zb in bad_mesh:
        assert lib.nm_raster_mesh(hh, v, m, 8.0, 8.0, 4.0, 4.0, W, H, fid, zb, None, None) == -1 and b"nm_raster_mesh" in lib.nm_last_error(), (W, H)
    bad_phong = [(None, d, w2c, 8, 8, light, d), (d, d, w2c, 8, 0, light, d), (d, d, w2c, 8, 8, None, d), (d, d, w2c, 8, 8, light, None),
                 (d, d, w2c, 8, 8, light, ctypes.c_void_p(d.value + 4))]
    for hh, v, m, W, H, li, out in bad_phong:
        assert lib.nm_raster_phong(hh, v, m, 8.0, 8.0, 4.0, 4.0, W, H, None, None, None, li, out, None) == -1 and b"nm_raster_phong" in lib.nm_last_error()
    assert lib.nm_raster_mesh(d, d, w2c, float('nan'), 8.0, 4.0, 4.0, 8, 8, d, d, None, None) == -1
    for args in ((None, d, d, 4), (d, None, d, 4), (d, d, None, 4), (d, d, d, 0), (d, d, d, -1)):
        assert lib.nm_overlay_rgba8(*args, None) == -1 and b"nm_overlay_rgba8" in lib.nm_last_error(), args


def test_install_rebinds_overlay_smpl_with_the_references_parameters():
    import neuman_hip
    from neuman_hip import render_utils
    mods = [types.ModuleType(n) for n in ("utils.ray_utils", "utils.render_utils", "models.vanilla")]
    assert not hasattr(mods[1], 'overlay_smpl')
    neuman_hip.install(*mods)
    assert mods[1].overlay_smpl is render_utils.overlay_smpl
    assert list(inspect.signature(mods[1].overlay_smpl).parameters) == ['img', 'verts', 'faces', 'cap']       # render_utils.py:485
    assert 'overlay_smpl' in neuman_hip._RENDER_FNS and not hasattr(mods[1], 'phong_renderer_from_pinhole_cam')  # (a pytorch3d object: not served)


def test_cpu_tensors_are_refused():
    from neuman_hip import raster, render_utils, synthetic
    cap = synthetic.SimpleCapture(16, 16, c2w=synthetic.spherical_c2w(30, -20, 1.3))
    verts, faces = synthetic.capsule_mesh(4, 5)
    img = np.zeros((16, 16, 3), np.uint8)
    for call in (lambda: render_utils.overlay_smpl(img, torch.from_numpy(verts), torch.from_numpy(faces), cap),
                 lambda: render_utils.rasterize_mesh(torch.from_numpy(verts), faces, cap),
                 lambda: render_utils.body_mask(torch.from_numpy(verts), faces, cap),
                 lambda: render_utils.overlay_smpl(img, verts, faces, cap)):
        with pytest.raises(_lib.NeumanHipError):
            call()
    # the camera of a capture: SimpleCapture's intrinsic matrix and inverse pose, or the reference's pinhole_cam + world-to-camera pose
    w2c, fx, fy, cx, cy, W, H = raster.camera_of(cap)
    assert (W, H) == (16, 16) and (fx, fy, cx, cy) == (20.0, 20.0, 8.0, 8.0) and np.allclose(w2c, np.linalg.inv(cap.cam_pose.camera_to_world)[:3])
    ref_cap = types.SimpleNamespace(pinhole_cam=types.SimpleNamespace(fx=30., fy=31., cx=7., cy=9., width=20, height=12),
                                    cam_pose=types.SimpleNamespace(rotation_matrix=np.eye(4), translation_vector=np.array([1., 2., 3.])), shape=(12, 20))
    w2c, fx, fy, cx, cy, W, H = raster.camera_of(ref_cap)
    assert (fx, fy, cx, cy, W, H) == (30., 31., 7., 9., 20, 12) and np.array_equal(w2c, np.concatenate([np.eye(3), [[1.], [2.], [3.]]], 1))
