"""-m gpu: the mesh rasteriser (csrc/raster.hip: nm_raster_mesh / nm_raster_phong / nm_overlay_rgba8, render_utils.rasterize_mesh / body_mask /
overlay_smpl, HumanNeRFTrainer.validation_images) against the float64 restatement of its contract, tests/helpers/raster_ref.py -- pytorch3d,
which the reference's overlay_smpl sits on, is absent, so no golden of the reference's own exists.

Tolerances on values are calibrated at run time: the helper also runs in float32, and the device is allowed 4 x that run's own worst deviation
from the float64 run on the same input (floor: 1e-6 relative) -- four is the margin for a different but equally valid float32 evaluation order.
Face ids are compared exactly, except on the pixels the float64 run itself calls ambiguous (a pixel centre within 1e-4, in barycentrics, of an
edge of a face that is not more than 0.1 % behind the winner, or two covering depths within 1e-4 relative); those are at most 1 % of the covered
pixels.  The measured deviations are printed ([raster] lines; profiles/raster.md keeps a copy).

The ambiguous pixels left out here -- centres on an edge or a vertex, exact depth ties -- are what tests/test_hip_raster_exact.py is about: on
the quarter-pixel scenes of tests/helpers/raster_exact.py every float32 operand is exact, and ids, depth and barycentrics are compared at every
pixel with no tolerance and no exclusions."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import raster_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

CAMERA = (30., -20., 1.3)
CASES = {                                                    # mesh (rings, segments), W, H
    'whole_tiles_96x64': ((84, 82), 96, 64),
    'ragged_tiles_37x29': ((84, 82), 37, 29),
    'one_tile_16x16': ((84, 82), 16, 16),                    # all 13 776 faces in one tile's list: 54 LDS batches, sub-pixel triangles
    'wide_faces_160x120': ((12, 10), 160, 120),              # faces spanning several tiles
}
_REF = {}


def _mesh(shape):
    from neuman_hip import synthetic
    return synthetic.capsule_mesh(*shape)


def _reference(verts, faces, cap, key):
    """float64 run (with its ambiguity map), float32 run and the calibrated tolerances of one input: computed once, shared, never written to"""
    if key not in _REF:
        cam = RR.camera_of(cap)
        r64, r32 = RR.rasterize(verts, faces, cam, np.float64, analyse=True), RR.rasterize(verts, faces, cam, np.float32)
        tol, dev = RR.tolerances(r64, r32, ~r64['ambiguous'])
        for r in (r64, r32):
            for a in r.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _REF[key] = (r64, tol, dev)
    return _REF[key]


def _device(verts, faces, cap, image=None):
    from neuman_hip import raster, render_utils
    v = torch.as_tensor(verts).cuda()
    face_id, zbuf, bary, rgba = raster.rasterizer_for(faces, v.shape[0]).rasterize(v, raster.camera_of(cap), shade=True)
    out = dict(face_id=face_id.cpu().numpy(), zbuf=zbuf.cpu().numpy(), bary=bary.cpu().numpy(), rgba=rgba.cpu().numpy())
    if image is not None:
        out['overlay'] = render_utils.overlay_smpl(image, v, torch.as_tensor(faces).cuda(), cap)
    return out


def _image(H, W, seed=0, high=100):
    return np.random.default_rng(seed).integers(0, high, (H, W, 3), dtype=np.uint8)


def _compare(name, dev, r64, tol, f32dev, image):
    """the parity statement of every case: exact face ids and calibrated values off the ambiguous pixels, untouched pixels where nothing covers"""
    amb, cov = r64['ambiguous'], r64['face_id'] >= 0
    ok = ~amb
    n_amb, n_cov = int(amb.sum()), int(cov.sum())
    both = ok & cov
    err = {k: float(np.abs(dev[k][both].astype(np.float64) - r64[k][both]).max()) if both.any() else 0.0 for k in ('zbuf', 'bary', 'rgba')}
    want_bytes = RR.overlay(r64['rgba'], image)
    byte_err = int(np.abs(dev['overlay'][both].astype(np.int32) - want_bytes[both]).max()) if both.any() else 0
    print(f"[raster] {name}: covered {n_cov} px, ambiguous {n_amb} ({100.0 * n_amb / max(n_cov, 1):.2f} %), face-id mismatches off them "
          f"{int((dev['face_id'] != r64['face_id'])[ok].sum())}; device vs float64 | float32 helper vs float64 | allowed: "
          + ", ".join(f"{k} {err[k]:.2e} | {f32dev[k]:.2e} | {tol[k]:.2e}" for k in err) + f"; overlay bytes off by at most {byte_err}")
    assert n_amb <= 0.01 * n_cov, (n_amb, n_cov)
    assert np.array_equal(dev['face_id'][ok], r64['face_id'][ok])
    for k in err:
        assert err[k] <= tol[k], (k, err[k], tol[k])
    assert byte_err <= 1
    none = dev['face_id'] < 0
    assert np.all(np.isposinf(dev['zbuf'][none])) and np.all(np.isfinite(dev['zbuf'][~none])) and np.all(dev['zbuf'][~none] > 0)
    assert np.array_equal(dev['overlay'][none], image[none])                                 # bit for bit
    assert np.all(dev['rgba'][none] == np.array([1, 1, 1, 0], np.float32)) and np.all(dev['rgba'][~none][:, 3] == 1) and np.all(dev['bary'][none] == 0)
    assert np.abs(dev['bary'][~none].sum(-1) - 1).max() < 1e-5 if (~none).any() else True


@pytest.mark.parametrize("case", list(CASES))
def test_parity_at_the_edges_of_the_kernels_structure(case):
    from neuman_hip import render_utils, synthetic
    shape, W, H = CASES[case]
    verts, faces = _mesh(shape)
    cap = synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(*CAMERA))
    r64, tol, f32dev = _reference(verts, faces, cap, case)
    image = _image(H, W)
    dev = _device(verts, faces, cap, image)
    assert int((r64['face_id'] >= 0).sum()) > 50
    _compare(case, dev, r64, tol, f32dev, image)
    # the pass without shading is the same pass
    face_id, zbuf, bary = render_utils.rasterize_mesh(torch.as_tensor(verts).cuda(), faces, cap)
    assert face_id.dtype == torch.int32 and tuple(face_id.shape) == (H, W) and tuple(bary.shape) == (H, W, 3)
    assert np.array_equal(face_id.cpu().numpy(), dev['face_id']) and np.array_equal(zbuf.cpu().numpy(), dev['zbuf']) and np.array_equal(bary.cpu().numpy(), dev['bary'])
    mask = render_utils.body_mask(torch.as_tensor(verts).cuda(), faces, cap)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), dev['face_id'] >= 0)


def test_a_face_larger_than_the_image():
    """two triangles forming a quad that overfills a 40 x 24 frame (its diagonal off the pixel centres), a small triangle in front"""
    from neuman_hip import synthetic
    verts = np.array([[-3, -3.2, 2], [3.1, -3, 2], [3, 3.3, 2], [-3.3, 3, 2], [-0.1, -0.1, 1], [0.15, -0.05, 1], [0, 0.12, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]])
    cap = synthetic.SimpleCapture(40, 24)
    r64, tol, f32dev = _reference(verts, faces, cap, 'large_face')
    image = _image(24, 40, 1)
    dev = _device(verts, faces, cap, image)
    assert (r64['face_id'] >= 0).all() and (dev['face_id'] >= 0).all()                       # every pixel is covered
    assert 20 < int((r64['face_id'] == 2).sum()) < 200
    _compare('large_face', dev, r64, tol, f32dev, image)
    ok = ~r64['ambiguous']
    assert np.array_equal((dev['face_id'] == 2)[ok], (r64['face_id'] == 2)[ok])          # the small triangle wins exactly where the helper says


def test_rejection_and_exactly_sized_outputs():
    """the camera close enough that part of the capsule is behind it and part off the frame: rule 2 drops those faces whole; the outputs are
    sized exactly, between guard words that stay as they were"""
    from neuman_hip import _lib, raster, synthetic
    verts, faces = _mesh((84, 82))
    W, H = 48, 40
    cap = synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(30., -20., 0.5))
    cam = RR.camera_of(cap)
    zc = verts.astype(np.float64) @ cam[0][2, :3] + cam[0][2, 3]
    r64, tol, f32dev = _reference(verts, faces, cap, 'rejection')
    assert (zc <= 0).sum() > 20 and (zc[faces] <= 0).any(1).sum() > 20                       # faces behind the camera plane ...
    assert 0 < r64['n_valid_faces'] < len(faces) and (r64['face_id'] < 0).any()
    border = np.concatenate([r64['face_id'][0], r64['face_id'][-1], r64['face_id'][:, 0], r64['face_id'][:, -1]])
    assert (border >= 0).any()                                                               # ... and the body leaves the frame
    v = torch.as_tensor(verts).cuda()
    R = raster.rasterizer_for(faces, v.shape[0])
    G, n = 64, H * W
    bufs = {'face_id': (torch.int32, 1, -77), 'zbuf': (torch.float32, 1, 123.0), 'bary': (torch.float32, 3, 123.0), 'rgba': (torch.float32, 4, 123.0)}
    mem = {k: torch.full((G + n * c + G,), fill, device='cuda', dtype=dt) for k, (dt, c, fill) in bufs.items()}
    ptr = {k: ctypes.c_void_p(mem[k].data_ptr() + G * 4) for k in mem}
    w2c = np.ascontiguousarray(cam[0])
    light = np.array(raster.LIGHT, np.float64)
    as_d = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))                      # noqa: E731
    _lib.check(_lib.lib().nm_raster_phong(R._h, _lib.dev_ptr(v), as_d(w2c), *[float(x) for x in cam[1:5]], W, H, ptr['face_id'], ptr['zbuf'], ptr['bary'],
                                          as_d(light), ptr['rgba'], _lib.stream_ptr()), "nm_raster_phong")
    torch.cuda.synchronize()
    dev = {}
    for k, (dt, c, fill) in bufs.items():
        a = mem[k].cpu().numpy()
        assert np.all(a[:G] == fill) and np.all(a[G + n * c:] == fill), k                    # the guard words
        dev[k] = a[G:G + n * c].reshape((H, W) if c == 1 else (H, W, c))
    image = _image(H, W, 2)
    from neuman_hip import render_utils
    dev['overlay'] = render_utils.overlay_smpl(image, v, faces, cap)
    _compare('rejection', dev, r64, tol, f32dev, image)
    # looking away: nothing is in front of the camera, and the overlay is the photograph
    away = synthetic.SimpleCapture(W, H, c2w=cap.cam_pose.camera_to_world @ np.diag([1., -1., -1., 1.]))
    back = _device(verts, faces, away, image)
    assert (back['face_id'] == -1).all() and np.all(np.isposinf(back['zbuf'])) and np.array_equal(back['overlay'], image)


def test_order_independence_and_determinism():
    from neuman_hip import synthetic
    verts, faces = _mesh((84, 82))
    cap = synthetic.SimpleCapture(96, 64, c2w=synthetic.spherical_c2w(*CAMERA))
    r64, _, _ = _reference(verts, faces, cap, 'whole_tiles_96x64')
    a, b = _device(verts, faces, cap), _device(verts, faces, cap)
    for k in a:
        assert np.array_equal(a[k], b[k]), k                                                 # two runs: the same bits in every output
    perm = np.random.default_rng(5).permutation(len(faces))
    p = _device(verts, faces[perm], cap)
    assert np.array_equal(p['zbuf'], a['zbuf'])                                              # bit-identical
    ok = ~r64['ambiguous'] & (a['face_id'] >= 0)
    assert np.array_equal(p['face_id'] >= 0, a['face_id'] >= 0) and np.array_equal(perm[p['face_id'][ok]], a['face_id'][ok])
    # one tile with every face in its list: the order the atomics left the list in does not show
    cap1 = synthetic.SimpleCapture(16, 16, c2w=synthetic.spherical_c2w(*CAMERA))
    a1, b1, p1 = _device(verts, faces, cap1), _device(verts, faces, cap1), _device(verts, faces[perm], cap1)
    assert all(np.array_equal(a1[k], b1[k]) for k in a1) and np.array_equal(p1['zbuf'], a1['zbuf'])


def test_exact_tie_goes_to_the_lower_face_index():
    """two coincident triangles (the same coordinates in the same corner order: the same float32 depth at every pixel), alone and with a third
    triangle of the same projection twice as far away, listed first, between and last"""
    from neuman_hip import synthetic
    tri = np.array([[-0.5, -0.3, 2], [0.45, -0.25, 2.5], [0.05, 0.33, 1.8]], np.float32)
    verts = np.concatenate([tri, tri, tri * np.float32(2)])
    cap = synthetic.SimpleCapture(40, 24)
    for faces, winner in (([[3, 4, 5], [0, 1, 2]], 0), ([[6, 7, 8], [0, 1, 2], [3, 4, 5]], 1), ([[3, 4, 5], [6, 7, 8], [0, 1, 2]], 0)):
        faces = np.array(faces)
        r64 = RR.rasterize(verts, faces, RR.camera_of(cap))
        dev = _device(verts, faces, cap)
        assert (r64['face_id'] >= 0).sum() > 100 and (r64['face_id'][r64['face_id'] >= 0] == winner).all()
        covered = dev['face_id'] >= 0
        assert covered.sum() > 100 and (dev['face_id'][covered] == winner).all(), faces.tolist()


def test_watertight_along_shared_edges():
    """rule 2 keeps a pixel on both sides of an edge, so a closed mesh has no cracks: every pixel of the float64 silhouette's interior (the mask
    eroded by one pixel) is covered, and no row of the (convex) silhouette has a hole"""
    from neuman_hip import render_utils, synthetic
    for case in ('whole_tiles_96x64', 'one_tile_16x16', 'wide_faces_160x120'):
        shape, W, H = CASES[case]
        verts, faces = _mesh(shape)
        cap = synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(*CAMERA))
        r64, _, _ = _reference(verts, faces, cap, case)
        mask = render_utils.body_mask(torch.as_tensor(verts).cuda(), faces, cap).cpu().numpy()
        m = np.pad(r64['face_id'] >= 0, 1)
        interior = np.ones((H, W), bool)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                interior &= m[dy:dy + H, dx:dx + W]
        assert interior.sum() > 10 and mask[interior].all(), case
        for r in np.flatnonzero(mask.any(1)):
            c = np.flatnonzero(mask[r])
            assert mask[r, c[0]:c[-1] + 1].all(), (case, r)


def test_validation_images_of_the_human_trainer():
    """reference trainers/human_nerf_trainer.py:475-513 on the synthetic body model at 48 x 32"""
    from neuman_hip import human_trainer, render_utils, synthetic
    from test_hip_human_trainer import TinyHumanNeRF
    dev = torch.device('cuda')
    net = TinyHumanNeRF(dev)
    for m in (net.coarse_bkg_net, net.fine_bkg_net, net.coarse_human_net):
        m.eval()
    faces = synthetic.smpl_like_model(0)['f'].astype(np.int32)
    can_verts = synthetic.smpl_like_model(0)['v_template'].astype(np.float32)
    opt = types.SimpleNamespace(samples_per_ray=16, importance_samples_per_ray=16, perturb=0.0, white_bkg=True, penalize_smpl_alpha=1.0,
                                penalize_symmetric_alpha=0.1, penalize_dummy=1.0, penalize_hard_surface=0.1, penalize_color_range=0.1, penalize_mask=0.01,
                                penalize_lpips=0.0, penalize_sharp_edge=0.1, penalize_outside_factor=2.0, dist_exponent=2.0)
    can_caps = [synthetic.SimpleCapture(48, 32, fx=40., c2w=synthetic.spherical_c2w(a, 0., 3.0)) for a in (0., 90.)]
    tr = human_trainer.HumanNeRFTrainer(opt, net, None, faces, (can_verts, faces), can_caps, interval_comp=0.8, seed=4)
    cap = synthetic.SimpleCapture(48, 32, fx=60., c2w=synthetic.spherical_c2w(15., -5., 3.0), near=0.5, far=5.0)
    image = _image(32, 48, 3)                                                                # bytes < 100: a shaded byte (>= 127) always changes the pixel
    imgs = tr.validation_images(cap, image, 1, can_caps[1])
    assert len(imgs) == 4 and all(isinstance(a, np.ndarray) and a.shape == (32, 48, 3) for a in imgs)
    rgb, depth, acc, overlay = imgs
    assert overlay.dtype == np.uint8 and np.isfinite(rgb).all() and np.isfinite(depth).all() and acc.min() >= 0 and acc.max() <= 1 + 1e-5
    assert np.array_equal(depth[..., 0], depth[..., 2]) and np.array_equal(acc[..., 0], acc[..., 1])
    with torch.no_grad():
        verts = net.vertex_forward(1)[0][0]
    assert np.array_equal(overlay, render_utils.overlay_smpl(image, verts, faces, cap))      # bit for bit
    mask = render_utils.body_mask(verts, faces, cap).cpu().numpy()
    assert 40 < mask.sum() < 32 * 48 and np.array_equal((overlay != image).any(-1), mask)
    assert len(tr.validation_images(cap, image, 1)) == 4                                     # the default canonical camera
