"""-m gpu: the soft silhouette (csrc/silhouette.hip: nm_raster_silhouette / nm_raster_silhouette_backward, raster.Rasterizer.silhouette,
render_utils.soft_silhouette, neuman_hip/optimize_smpl.py) against the float64 restatement of its contract, tests/helpers/silhouette_ref.py --
pytorch3d, which the reference's silhouette sits on, is absent, so no golden of the reference's own exists.

Tolerances are calibrated at run time, by the rasteriser tests' rule: the helper also runs in float32, and the device is allowed 4 x that
run's own worst deviation from the float64 run on the same input (floor: 1e-6, for gradients relative to the largest component).  alpha, keep
and n_cand are compared off the pixels the float64 run itself calls ambiguous (a non-inside face within 1e-5, relative, of the candidate cut; a
weighted inside candidate whose two smallest edge distances are within 1e-5, relative); those are at most 1 % of the pixels with alpha > 0,
and the upstream gradient of every gradient comparison is zero on them.  The measured figures are printed ([silhouette] lines;
profiles/silhouette.md keeps a copy)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import silhouette_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

CAMERA = (30., -20., 1.3)
CASES = {                                                    # mesh (rings, segments), W, H, sigma: what it crosses
    'whole_tiles': ((40, 38), 96, 64, 1e-2),                 # R_px 9.7: boxes reach neighbouring tiles
    'far_reach': ((40, 38), 96, 64, 4e-2),                   # R_px 19.4: beyond the adjacent tile
    'ragged_tiles': ((84, 82), 37, 29, 1e-2),                # partial tiles, 13 776 sub-pixel faces, thousands of candidates in one pixel
    'one_tile': ((84, 82), 16, 16, 1e-3),                    # every face in one list: 54 LDS batches
    'wide_faces': ((12, 10), 160, 120, 1e-3),                # faces spanning tiles; nearly every covered pixel soft
    'reference_sigma': ((40, 38), 96, 64, 1e-4),             # the defaults
}
_REF = {}


def _mesh(shape):
    from neuman_hip import synthetic
    return synthetic.capsule_mesh(*shape)


def _cap(W, H, camera=CAMERA):
    from neuman_hip import synthetic
    return synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(*camera))


def _helper(verts, faces, cam, sigma, blur, dtype, g_alpha=None, analyse=False):
    v = torch.as_tensor(verts).clone().requires_grad_(True)
    r = SR.silhouette(v, faces, cam, sigma, blur, dtype, analyse=analyse)
    if g_alpha is None:                                      # the upstream gradient: seeded noise, zero on the ambiguous pixels
        g_alpha = (np.random.default_rng(7).standard_normal(r['alpha'].shape) * ~r['ambiguous']).astype(np.float32)
    (r['alpha'] * torch.as_tensor(g_alpha).to(dtype)).sum().backward()
    out = dict(alpha=r['alpha'].detach().double().numpy(), keep=r['keep'].detach().double().numpy(), n_cand=r['n_cand'], g_verts=v.grad.double().numpy(),
               g_alpha=g_alpha)
    if analyse:
        out['ambiguous'] = r['ambiguous']
    return out


def _reference(key, verts, faces, cap, sigma, blur=None):
    """float64 run (with its ambiguity map and gradient), float32 run and the calibrated tolerances of one input: computed once, shared,
    never written to"""
    if key not in _REF:
        cam = SR.camera_of(cap)
        blur = SR.default_blur_radius(sigma) if blur is None else blur
        r64 = _helper(verts, faces, cam, sigma, blur, torch.float64, analyse=True)
        r32 = _helper(verts, faces, cam, sigma, blur, torch.float32, g_alpha=r64['g_alpha'])
        ok = ~r64['ambiguous']
        tol, dev = {}, {}
        for k in ('alpha', 'keep'):
            tol[k], dev[k] = SR.tolerance(r64[k], r32[k], ok)
        tol['g_verts'], dev['g_verts'] = SR.tolerance(r64['g_verts'], r32['g_verts'], relative=True)
        for a in r64.values():
            a.setflags(write=False)
        _REF[key] = (r64, tol, dev)
    return _REF[key]


def _device(verts, faces, cap, sigma, blur=None, g_alpha=None, rast=None):
    from neuman_hip import raster
    v = torch.as_tensor(verts).cuda()
    R = raster.rasterizer_for(faces, v.shape[0]) if rast is None else rast
    cam = raster.camera_of(cap)
    blur = raster.default_blur_radius(sigma) if blur is None else blur
    alpha, keep, n_cand = R.silhouette(v, cam, sigma, blur, want_count=True)
    out = dict(alpha=alpha.cpu().numpy(), keep=keep.cpu().numpy(), n_cand=n_cand.cpu().numpy())
    if g_alpha is not None:
        out['g_verts'] = R.silhouette_backward(v, cam, sigma, blur, keep, torch.tensor(g_alpha).cuda()).cpu().numpy()
    return out


def _compare(name, dev, r64, tol, f32dev):
    """the parity statement of every case"""
    amb = r64['ambiguous']
    ok = ~amb
    n_amb, n_cov = int(amb.sum()), int((r64['alpha'] > 0).sum())
    err = {k: float(np.abs(dev[k][ok].astype(np.float64) - r64[k][ok]).max()) for k in ('alpha', 'keep')}
    err['g_verts'] = float(np.abs(dev['g_verts'].astype(np.float64) - r64['g_verts']).max())
    gmax = float(np.abs(r64['g_verts']).max())
    print(f"[silhouette] {name}: alpha > 0 on {n_cov} px, ambiguous {n_amb} ({100.0 * n_amb / max(n_cov, 1):.2f} %), most candidates in a pixel "
          f"{int(r64['n_cand'].max())}, n_cand mismatches off the ambiguous {int((dev['n_cand'] != r64['n_cand'])[ok].sum())}, largest gradient component "
          f"{gmax:.3e}; device vs float64 | float32 helper vs float64 | allowed: " + ", ".join(f"{k} {err[k]:.2e} | {f32dev[k]:.2e} | {tol[k]:.2e}" for k in err))
    assert n_amb <= 0.01 * n_cov, (n_amb, n_cov)
    assert np.array_equal(dev['n_cand'][ok], r64['n_cand'][ok])
    for k in err:
        assert err[k] <= tol[k], (k, err[k], tol[k])
    assert np.array_equal(dev['alpha'], np.float32(1) - dev['keep'])                             # alpha is 1 - keep, keep the product itself
    none = dev['n_cand'] == 0
    assert np.all(dev['alpha'][none] == 0) and np.all(dev['keep'][none] == 1)
    assert np.all((dev['keep'] >= 0) & (dev['keep'] <= 1)) and np.isfinite(dev['g_verts']).all()


@pytest.mark.parametrize("case", list(CASES))
def test_parity_at_the_edges_of_the_kernels_structure(case):
    shape, W, H, sigma = CASES[case]
    verts, faces = _mesh(shape)
    cap = _cap(W, H)
    r64, tol, f32dev = _reference(case, verts, faces, cap, sigma)
    dev = _device(verts, faces, cap, sigma, g_alpha=r64['g_alpha'])
    assert int((r64['alpha'] > 0).sum()) > 50 and np.abs(r64['g_verts']).max() > 0
    _compare(case, dev, r64, tol, f32dev)


def test_a_face_larger_than_the_image():
    """two triangles forming a quad that overfills a 40 x 24 frame (its diagonal off the pixel centres), a small triangle in front: depth
    plays no role, all three count wherever they reach"""
    from neuman_hip import synthetic
    verts = np.array([[-3, -3.2, 2], [3.1, -3, 2], [3, 3.3, 2], [-3.3, 3, 2], [-0.1, -0.1, 1], [0.15, -0.05, 1], [0, 0.12, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]])
    cap = synthetic.SimpleCapture(40, 24)
    for sigma in (1e-4, 1e-2):
        r64, tol, f32dev = _reference(f'large_face_{sigma}', verts, faces, cap, sigma)
        dev = _device(verts, faces, cap, sigma, g_alpha=r64['g_alpha'])
        assert (r64['n_cand'] >= 1).all() and r64['n_cand'].max() == 3
        _compare(f'large_face_{sigma}', dev, r64, tol, f32dev)


def test_a_face_with_a_vertex_behind_the_camera_is_dropped_whole():
    from neuman_hip import synthetic
    front = np.array([[-0.5, -0.3, 2], [0.45, -0.25, 2.5], [0.05, 0.33, 1.8]], np.float32)
    verts = np.concatenate([front, [[-0.4, 0.2, 1.5], [0.4, 0.25, 1.2], [0.0, -0.2, -0.5]]]).astype(np.float32)      # the last vertex is behind
    faces = np.array([[0, 1, 2], [3, 4, 5]])
    cap = synthetic.SimpleCapture(40, 24)
    sigma = 1e-2
    r64, tol, f32dev = _reference('behind', verts, faces, cap, sigma)
    dev = _device(verts, faces, cap, sigma, g_alpha=r64['g_alpha'])
    _compare('behind', dev, r64, tol, f32dev)
    alone = _device(front, faces[:1], cap, sigma, g_alpha=r64['g_alpha'])
    assert (alone['alpha'] > 0).sum() > 100
    for k in ('alpha', 'keep', 'n_cand'):
        assert np.array_equal(dev[k], alone[k]), k                                               # it contributes nothing ...
    assert np.all(dev['g_verts'][3:] == 0) and np.array_equal(dev['g_verts'][:3], alone['g_verts'])      # ... and receives nothing


def test_an_empty_view():
    from neuman_hip import synthetic
    verts, faces = _mesh((12, 10))
    cap = _cap(48, 40)
    away = synthetic.SimpleCapture(48, 40, c2w=cap.cam_pose.camera_to_world @ np.diag([1., -1., -1., 1.]))
    g = np.random.default_rng(3).standard_normal((40, 48)).astype(np.float32)
    dev = _device(verts, faces, away, 1e-2, g_alpha=g)
    assert np.all(dev['alpha'] == 0) and np.all(dev['keep'] == 1) and np.all(dev['n_cand'] == 0) and np.all(dev['g_verts'] == 0)
    # in view but wholly off the frame's reach: a principal point far outside
    off = synthetic.SimpleCapture(48, 40, cx=4000., c2w=cap.cam_pose.camera_to_world)
    dev = _device(verts, faces, off, 1e-2, g_alpha=g)
    assert np.all(dev['alpha'] == 0) and np.all(dev['keep'] == 1) and np.all(dev['g_verts'] == 0)


def test_blur_radius_zero_keeps_only_inside_faces():
    from neuman_hip import render_utils
    verts, faces = _mesh((12, 10))
    cap = _cap(40, 32)
    r64, tol, f32dev = _reference('blur0', verts, faces, cap, 1e-3, blur=0.0)
    dev = _device(verts, faces, cap, 1e-3, blur=0.0, g_alpha=r64['g_alpha'])
    _compare('blur0', dev, r64, tol, f32dev)
    mask = render_utils.body_mask(torch.as_tensor(verts).cuda(), faces, cap).cpu().numpy()
    assert mask.sum() > 100 and np.array_equal(dev['n_cand'] > 0, mask)                          # inside is the rasteriser's own coverage
    assert dev['n_cand'].max() >= 2                                                              # front and back of the closed mesh


def test_reproducibility():
    """S6: the same bits on every run, and through a fresh handle"""
    from neuman_hip import raster
    shape, W, H, sigma = CASES['ragged_tiles']
    verts, faces = _mesh(shape)
    cap = _cap(W, H)
    g = np.random.default_rng(11).standard_normal((H, W)).astype(np.float32)
    a, b = _device(verts, faces, cap, sigma, g_alpha=g), _device(verts, faces, cap, sigma, g_alpha=g)
    fresh = raster.Rasterizer(faces, verts.shape[0])
    c = _device(verts, faces, cap, sigma, g_alpha=g, rast=fresh)
    fresh.close()
    assert np.abs(a['g_verts']).max() > 0 and a['n_cand'].max() > 256
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


def test_autograd_plumbing():
    from neuman_hip import raster, render_utils
    verts, faces = _mesh((12, 10))
    cap = _cap(48, 40)
    v = torch.as_tensor(verts).cuda().requires_grad_(True)
    alpha = render_utils.soft_silhouette(v, faces, cap, sigma=1e-2)
    assert alpha.shape == (40, 48) and alpha.dtype == torch.float32 and alpha.is_cuda and alpha.requires_grad
    alpha.square().mean().backward()
    # the same upstream gradient, made by torch from the same alpha, through a direct call
    R = raster.rasterizer_for(faces, verts.shape[0])
    cam = raster.camera_of(cap)
    blur = raster.default_blur_radius(1e-2)
    a2, keep, _ = R.silhouette(v.detach(), cam, 1e-2, blur)
    leaf = a2.clone().requires_grad_(True)
    leaf.square().mean().backward()
    g = R.silhouette_backward(v.detach(), cam, 1e-2, blur, keep, leaf.grad)
    assert torch.equal(alpha.detach(), a2) and v.grad is not None and v.grad.abs().max() > 0 and torch.equal(v.grad, g)
    # the default blur radius is the reference's log(1/1e-4 - 1) sigma
    d = render_utils.soft_silhouette(v.detach(), faces, cap)
    e = R.silhouette(v.detach(), cam, 1e-4, np.log(1. / 1e-4 - 1.) * 1e-4)[0]
    assert torch.equal(d, e) and not d.requires_grad


# ---- the fit -------------------------------------------------------------------------------------------------------------------------
def _fit_setup(W, H):
    """the synthetic body at rest, seen from the front; the target is the same body with joints 16 and 17 (upper arms) turned by 0.15 rad
    on their free axes: its body_mask is the detected mask, its projected joints are the keypoints (confidence 1), every DensePose label is seen"""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import render_utils, smpl, synthetic
    model = synthetic.smpl_like_model(0)
    body = smpl.SMPLDiff(model, 'cuda')
    faces = model['f'].astype(np.int32)
    cap = synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(20., -10., 3.0))
    start = dict(pose=np.zeros(72, np.float32), betas=np.zeros(10, np.float32))
    align = np.eye(4)[:, :3]
    target = np.zeros(72, np.float32)
    target[[16 * 3 + 1, 16 * 3 + 2, 17 * 3 + 1, 17 * 3 + 2]] = 0.15
    obj = O.Objective(types.SimpleNamespace(binary_mask=np.zeros((H, W)), keypoints=np.zeros((17, 3)), intrinsic_matrix=cap.intrinsic_matrix, shape=cap.shape,
                                            cam_pose=cap.cam_pose), start, faces, body, align, 1.0)
    with torch.no_grad():
        wv, wj = O.vertext_forward(torch.as_tensor(target).cuda(), obj.betas, obj.align, body, 1.0)
        mask = render_utils.body_mask(wv[0], faces, cap).cpu().numpy()
        proj = O.project_joints(wj[0], obj.K, obj.w2c, obj.shape).cpu().numpy()
    keypoints = np.zeros((17, 3))
    keypoints[:, 2] = 1.0
    for s, c in O._SMPL_FROM_COCO.items():
        keypoints[c, :2] = proj[s]
    cap.binary_mask, cap.keypoints, cap.densepose = mask.astype(np.float32), keypoints, np.arange(25).reshape(5, 5)
    return cap, start, faces, body, model, align


def test_the_fit_descends_keeps_masked_entries_and_repeats():
    from neuman_hip import optimize_smpl as O
    cap, start, faces, body, _, align = _fit_setup(96, 64)
    assert 100 < cap.binary_mask.sum() < 96 * 64 / 2 and (cap.keypoints[5:, :2] > 0).all(1).sum() >= 10     # (a joint with a zero coordinate is masked)
    a = O.optimize_smpl(cap, start, faces, body, align, 1.0, num_iters=20)
    b = O.optimize_smpl(cap, start, faces, body, align, 1.0, num_iters=20)
    assert isinstance(a, np.ndarray) and a.shape == (72,) and a.dtype == np.float32
    obj = O.Objective(cap, start, faces, body, align, 1.0)
    with torch.no_grad():
        before = float(obj.terms(torch.as_tensor(start['pose']).cuda())[1])
        after = float(obj.terms(torch.as_tensor(a).cuda())[1])
    print(f"[silhouette] fit 96x64: silhouette mse {before:.6e} at iteration 0, {after:.6e} after 20 iterations")
    assert after < before                                                                        # (a)
    free = O.turn_smpl_gradient_on(cap.densepose) != 0
    assert free.sum() == 18 and np.array_equal(a[~free].view(np.int32), start['pose'][~free].view(np.int32))      # (b) the same bits
    assert (a[free] != start['pose'][free]).any()
    assert np.array_equal(a.view(np.int32), b.view(np.int32))                                    # (c)


def test_the_fits_pose_gradient_against_float64():
    """(d) pose.grad after one loss.backward() at 40 x 32 against SMPLDiff on the CPU in float64 through the helper; the allowance is 4 x what
    the same evaluation in float32 deviates by"""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import smpl
    cap, start, faces, body, model, align = _fit_setup(40, 32)
    pose0 = (np.random.default_rng(5).standard_normal(72) * 0.05).astype(np.float32)
    cam = SR.camera_of(cap)
    grads = {}
    for name, dtype in (('f64', torch.float64), ('f32', torch.float32)):
        cpu = smpl.SMPLDiff(model, 'cpu').to(dtype)
        obj = O.Objective(cap, start, faces, cpu, align, 1.0, silhouette=lambda v, dtype=dtype: SR.silhouette(v, faces, cam, 1e-4, dtype=dtype)['alpha'])
        pose = torch.as_tensor(pose0).to(dtype).requires_grad_(True)
        obj.loss(pose).backward()
        grads[name] = pose.grad.double().numpy()
    pose = torch.as_tensor(pose0).cuda().requires_grad_(True)
    O.Objective(cap, start, faces, body, align, 1.0).loss(pose).backward()
    got = pose.grad.double().cpu().numpy()
    tol, f32dev = SR.tolerance(grads['f64'], grads['f32'], relative=True)
    err = float(np.abs(got - grads['f64']).max())
    print(f"[silhouette] fit 40x32 pose.grad: largest component {np.abs(grads['f64']).max():.3e}; device vs float64 | float32 helper vs float64 | allowed: "
          f"{err:.2e} | {f32dev:.2e} | {tol:.2e}")
    assert np.abs(grads['f64']).max() > 0 and err <= tol, (err, tol)
