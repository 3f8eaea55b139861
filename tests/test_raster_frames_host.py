"""Without a device: nm_raster_frames (csrc/raster_frames.hip; the header's 'mesh frames') in the header, in `_lib.SIGNATURES` and in the library,
its refusals and the Python layer's; tests/helpers/raster_frames_ref.py (rules F2-F5 in numpy) on scenes with closed-form answers;
`render_utils.depth_to_camera_z`; and the ambiguity cap of tests/test_hip_raster_frames.py on every image that test renders, so that the GPU
test cannot hide behind it."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import raster_frames_ref as FR  # noqa: E402
import raster_ref as RR  # noqa: E402

from neuman_hip import _lib  # noqa: E402

NAME = "nm_raster_frames"


def test_the_entry_is_declared_bound_and_exported_with_matching_arity():
    src = open(os.path.join(HERE, "..", "include", "neuman_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + NAME + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{NAME} is not declared in neuman_hip.h"
    assert NAME in _lib.SIGNATURES and hasattr(_lib.lib(), NAME)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[NAME][1]) == 17


def test_every_refusal_comes_before_any_device_work():
    lib = _lib.lib()
    dummy = (ctypes.c_char * 256)()                                     # stands in for every device pointer: the checks run before any is read
    d = ctypes.cast(dummy, ctypes.c_void_p)
    nan, inf = float('nan'), float('inf')
    as_d = lambda *x: (ctypes.c_double * 3)(*x)                         # noqa: E731
    good = dict(h=d, verts=d, w2c=d, intr=d, B=2, W=8, H=8, colours=d, normals=d, light=as_d(2, 2, -2), bg=d, bg_z=d, out=d, face_id=d, zbuf=d, bary=d)
    bad = [dict(h=None), dict(verts=None), dict(w2c=None), dict(intr=None), dict(out=None), dict(B=0), dict(B=-3), dict(B=1 << 16), dict(W=0), dict(H=0),
           dict(W=-1), dict(W=1 << 16, H=1 << 16), dict(light=None), dict(normals=None), dict(light=as_d(nan, 0, 0)), dict(light=as_d(0, inf, 0)),
           dict(light=as_d(0, 0, -inf))]
    for over in bad:
        k = dict(good, **over)
        rc = lib.nm_raster_frames(k['h'], k['verts'], k['w2c'], k['intr'], k['B'], k['W'], k['H'], k['colours'], k['normals'], k['light'], k['bg'], k['bg_z'],
                                  k['out'], k['face_id'], k['zbuf'], k['bary'], None)
        assert rc == -1 and b"nm_raster_frames:" in lib.nm_last_error(), over


def _caps(sizes):
    from neuman_hip import synthetic
    return [synthetic.SimpleCapture(w, h, c2w=synthetic.spherical_c2w(30., -20., 1.3)) for w, h in sizes]


def test_the_python_layer_refuses_cpu_tensors_mismatched_shapes_and_mixed_image_sizes():
    from neuman_hip import render_utils
    faces = np.array([[0, 1, 2]])
    caps = _caps([(8, 6), (8, 6)])
    with pytest.raises(_lib.NeumanHipError, match="no CPU path"):
        render_utils.render_mesh_frames(torch.zeros(2, 3, 3), faces, caps)
    with pytest.raises(_lib.NeumanHipError, match="no CPU path"):
        render_utils.render_mesh_frames(np.zeros((2, 3, 3), np.float32), faces, caps)
    if not torch.cuda.is_available():
        return                                                          # (what follows needs tensors that pass as device tensors)
    v = torch.zeros(2, 3, 3, device='cuda')
    with pytest.raises(ValueError, match="one image size"):
        render_utils.render_mesh_frames(v, faces, _caps([(8, 6), (10, 6)]))
    for kw in (dict(colours=torch.zeros(4, 3, device='cuda')), dict(normals=torch.zeros(2, 4, 3, device='cuda')), dict(normals=torch.zeros(2, 3, 3)),
               dict(colours=torch.zeros(3, 3, device='cuda', dtype=torch.float64)), dict(background=torch.zeros(6, 8, 3, device='cuda')),
               dict(background=torch.zeros(2, 6, 9, 3, device='cuda', dtype=torch.uint8)), dict(background_depth=torch.zeros(6, 8, device='cuda')),
               dict(frames_per_call=0)):
        with pytest.raises(_lib.NeumanHipError):
            render_utils.render_mesh_frames(v, faces, caps, **kw)
    with pytest.raises(_lib.NeumanHipError):
        render_utils.render_mesh_frames(torch.zeros(3, 3, 3, device='cuda'), faces, caps)           # three frames, two captures


class _Fake(torch.Tensor):
    """a CPU tensor that says it lives on the device: the layer's checks of shapes, dtypes and devices run, on a box without one, up to the
    first call that needs it"""
    is_cuda = True


def test_the_python_layers_checks_without_a_device():
    from neuman_hip import render_utils
    if torch.cuda.is_available():
        pytest.skip("GPU box: the same refusals run on real device tensors in the test above")
    fake = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype).as_subclass(_Fake)      # noqa: E731
    faces = np.array([[0, 1, 2]])
    caps = _caps([(8, 6), (8, 6)])
    with pytest.raises(ValueError, match="one image size"):
        render_utils.render_mesh_frames(fake(2, 3, 3), faces, _caps([(8, 6), (10, 6)]))
    for kw in (dict(colours=fake(4, 3)), dict(normals=fake(2, 4, 3)), dict(normals=torch.zeros(2, 3, 3)), dict(colours=fake(3, 3, dtype=torch.float64)),
               dict(background=fake(6, 8, 3)), dict(background=fake(2, 6, 9, 3, dtype=torch.uint8)), dict(background_depth=fake(6, 8))):
        with pytest.raises(_lib.NeumanHipError, match="render_mesh_frames: (colours|normals|background|background_depth) must be"):
            render_utils.render_mesh_frames(fake(2, 3, 3), faces, caps, **kw)
    with pytest.raises(_lib.NeumanHipError, match="2 cameras for 3 frames"):
        render_utils.render_mesh_frames(fake(3, 3, 3), faces, caps)
    with pytest.raises(_lib.NeumanHipError, match="no HIP device"):                                 # every check passed: only the device is missing
        render_utils.render_mesh_frames(fake(2, 3, 3), faces, caps, colours=fake(3, 3), normals=fake(2, 3, 3))


def test_the_default_chunk_follows_the_documented_scratch():
    from neuman_hip import render_utils
    V, F, W, H = 150_000, 300_000, 512, 512
    n = render_utils.mesh_frames_per_call(V, F, W, H)
    per_frame = 16 * V + 12 * 32 * 32 + 8 * F                           # the header's per-frame scratch and two 4-byte list entries per face
    assert n * per_frame <= render_utils.MESH_FRAMES_SCRATCH < (n + 1) * per_frame and n > 1
    assert render_utils.mesh_frames_per_call(10 ** 9, 1, 16, 16) == 1 and render_utils.mesh_frames_per_call(1, 1, 16, 16) == 65535


# ---- the helper on closed-form scenes ------------------------------------------------------------------------------------------------------
TRI = np.array([[-0.5, -0.35, 2.0], [0.55, -0.3, 2.6], [0.0, 0.4, 1.7]], np.float32)
RGB = np.eye(3, dtype=np.float32)


def _tri_camera(W=48, H=40):
    from neuman_hip import synthetic
    return RR.camera_of(synthetic.SimpleCapture(W, H))


def test_a_triangle_with_red_green_and_blue_corners():
    cam = _tri_camera()
    r = FR.render(TRI, [[0, 1, 2]], cam, colours=RGB)
    cov = r['face_id'] >= 0
    assert cov.sum() > 100 and np.array_equal(r['show'], cov)
    # the colour IS the perspective-correct barycentric triple, and it sums to one
    assert np.abs(r['colour'][cov] - r['bary'][cov]).max() < 1e-15 and np.abs(r['colour'][cov].sum(-1) - 1).max() < 1e-12
    # the closed form, with no screen space in it: the pixel's ray (the camera is the identity) meets the triangle's plane at X, and the
    # colour is X's barycentric triple in 3D -- (1/3, 1/3, 1/3) on the ray through the centroid, whatever the corners' depths
    w2c, fx, fy, cx, cy, W, H = cam
    assert np.array_equal(w2c, np.eye(4)[:3])
    tri = TRI.astype(np.float64)
    normal = np.cross(tri[1] - tri[0], tri[2] - tri[0])

    def on_ray(u, v):
        ray = np.array([(u - cx) / fx, (v - cy) / fy, 1.0])
        return np.linalg.solve(tri.T, ray * (normal @ tri[0]) / (normal @ ray))

    rows, cols = np.nonzero(cov)
    want = np.array([on_ray(c + 0.5, r_ + 0.5) for r_, c in zip(rows, cols)])
    assert np.abs(r['colour'][cov] - want).max() < 1e-12
    centroid = tri.mean(0)
    u, v = fx * centroid[0] / centroid[2] + cx, fy * centroid[1] / centroid[2] + cy
    assert np.abs(on_ray(u, v) - 1 / 3).max() < 1e-14
    assert np.abs(r['colour'][int(np.floor(v)), int(np.floor(u))] - 1 / 3).max() < 0.05            # the centroid's pixel: within half a pixel of it
    assert np.array_equal(r['out'][cov], np.clip(r['colour'][cov] * 255, 0, 255).astype(np.uint8)) and (r['out'][~cov] == 255).all()
    # unlit white without colours, and the light darkens nothing below one half
    white = FR.render(TRI, [[0, 1, 2]], cam)
    assert (white['out'] == 255).all()
    n = np.tile(np.array([[0, 0, -1]], np.float32), (3, 1))
    lit = FR.render(TRI, [[0, 1, 2]], cam, normals=n)
    assert (lit['colour'][cov] >= 0.5).all() and (lit['colour'][cov] <= 1.0).all() and lit['colour'][cov].min() < 0.99
    away = FR.render(TRI, [[0, 1, 2]], cam, normals=-n)
    assert (away['colour'][cov] == 0.5).all() and (away['out'][cov] == 127).all()


def test_a_background_plane_in_front_and_behind_and_at_the_mesh():
    cam = _tri_camera()
    bg = np.random.default_rng(0).integers(0, 100, (40, 48, 3), dtype=np.uint8)
    free = FR.render(TRI, [[0, 1, 2]], cam, colours=RGB, bg=bg)
    cov = free['face_id'] >= 0
    assert np.array_equal(free['out'][~cov], bg[~cov]) and (free['out'][cov] != bg[cov]).any(-1).all()
    near, far = np.float32(free['zbuf'][cov].min() - 1e-3), np.float32(free['zbuf'][cov].max() + 1e-3)
    front = FR.render(TRI, [[0, 1, 2]], cam, colours=RGB, bg=bg, bg_z=np.full((40, 48), near, np.float32))
    behind = FR.render(TRI, [[0, 1, 2]], cam, colours=RGB, bg=bg, bg_z=np.full((40, 48), far, np.float32))
    assert not front['show'].any() and np.array_equal(front['out'], bg)                             # every covered pixel flips ...
    assert np.array_equal(behind['show'], cov) and np.array_equal(behind['out'], free['out'])       # ... and flips back
    for r in (front, behind):                                                                       # F1: the geometry reports the mesh alone
        assert np.array_equal(r['face_id'], free['face_id']) and np.array_equal(r['zbuf'], free['zbuf'])
    for dtype in (np.float64, np.float32):
        r = FR.render(TRI, [[0, 1, 2]], cam, dtype, colours=RGB, bg=bg)
        same = FR.render(TRI, [[0, 1, 2]], cam, dtype, colours=RGB, bg=bg, bg_z=r['zbuf'])
        assert np.array_equal(same['out'], bg) and not same['show'].any()                           # bg_z == zbuf hides the mesh everywhere
    z = np.where(cov, np.nan, np.inf).astype(np.float32)
    assert np.array_equal(FR.render(TRI, [[0, 1, 2]], cam, colours=RGB, bg=bg, bg_z=z)['out'], bg)  # NaN hides
    assert np.array_equal(FR.render(TRI, [[0, 1, 2]], cam, colours=RGB, bg=bg, bg_z=np.full((40, 48), np.inf, np.float32))['out'], free['out'])
    nan_colour = RGB.copy()
    nan_colour[0, 0] = np.nan
    assert (FR.render(TRI, [[0, 1, 2]], cam, colours=nan_colour)['out'][cov][:, 0] == 0).all()      # F5: a NaN gives 0


def test_byte_range_brackets_the_truncation():
    c = np.array([0.5, 127.999999 / 255, 128 / 255, 1.0, 1.2, -0.1, np.nan])
    lo, hi = FR.byte_range(c, 1e-6)
    assert lo.tolist() == [127, 127, 127, 254, 255, 0, 0] and hi.tolist() == [127, 128, 128, 255, 255, 0, 0]


def test_depth_to_camera_z_on_a_fronto_parallel_plane(monkeypatch):
    """a plane at camera depth 2.5: the renderers' depth is the distance along each pixel's ray, and the helper gives 2.5 back everywhere"""
    from neuman_hip import ray_utils, render_utils, synthetic
    monkeypatch.setattr(render_utils, "HOST_RAYS", True)               # the renderer's rays from their host mirror: no device here
    cap = synthetic.SimpleCapture(20, 14, c2w=synthetic.spherical_c2w(25., -15., 3.0))
    o, d = ray_utils.shot_all_rays(cap)
    axis = np.asarray(cap.cam_pose.camera_to_world, np.float64)[:3, 2]
    depth = (2.5 / (d @ axis)).reshape(14, 20)                          # where each ray meets the plane
    assert depth.max() > depth.min() * 1.02                            # (the distances themselves are far from constant)
    z = render_utils.depth_to_camera_z(torch.from_numpy(depth.astype(np.float32)), cap)
    assert tuple(z.shape) == (14, 20) and z.dtype == torch.float32 and float((z - 2.5).abs().max()) < 1e-5
    with pytest.raises(_lib.NeumanHipError):
        render_utils.depth_to_camera_z(torch.zeros(14, 21), cap)


@pytest.mark.parametrize("name", list(FR.SCENES))
def test_the_float64_helper_calls_at_most_one_percent_of_the_gpu_tests_pixels_ambiguous(name):
    s = FR.scene(name)
    for b, cap in enumerate(s['caps']):
        r = RR.rasterize(s['verts'][b], s['faces'], RR.camera_of(cap), analyse=True)
        cov, amb = int((r['face_id'] >= 0).sum()), int(r['ambiguous'].sum())
        assert cov > 50 and amb <= 0.01 * cov, (name, b, amb, cov)
