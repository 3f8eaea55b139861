"""Without a device: the float64 restatement of the soft silhouette's contract (tests/helpers/silhouette_ref.py) against closed forms on one
triangle, its autograd gradient against central finite differences, brute force against bounding-box candidates; the small pure functions of
neuman_hip/optimize_smpl.py against what the reference's own return (tests/golden/optimize_smpl.npz); the two entry points' argument checks."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import silhouette_ref as SR  # noqa: E402

from neuman_hip import _lib  # noqa: E402

EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
CAM64 = (EYE, 1.0, 1.0, 0.0, 0.0, 64, 64)                            # z = 1, unit focal length: world x, y are screen x, y; 1 pixel = 1/32 NDC


def _triangle(x_edge):
    """a triangle with a vertical edge at screen x = x_edge, as float64: pixel (row 30, column 3), centre (3.5, 30.5), faces that edge"""
    return torch.tensor([[x_edge, 4., 1.], [60., 32., 1.], [x_edge, 60., 1.]], dtype=torch.float64)


def test_helper_on_a_triangle_with_closed_forms():
    sigma, blur = SR.SIGMA, SR.default_blur_radius()
    assert blur == math.log(1.0 / 1e-4 - 1.0) * 1e-4
    faces = np.array([[0, 1, 2]])
    r_px = math.sqrt(blur) * 32                                          # the reach of the face beyond its edge, in pixels: 0.971
    for brute in (False, True):
        # the pixel centre on the edge: d = 0, alpha = 1/2; far inside alpha -> 1; one pixel further out than the reach: nothing
        r = SR.silhouette(_triangle(3.5), faces, CAM64, brute=brute, analyse=True)
        a = r['alpha'].numpy()
        assert a[30, 3] == 0.5 and r['n_cand'][30, 3] == 1
        assert 1 - a[32, 30] < 1e-300 and r['keep'].numpy()[32, 30] == 1 - a[32, 30]
        assert a[30, 2] == 0 and r['n_cand'][30, 2] == 0 and r['keep'].numpy()[30, 2] == 1
        assert a[2, 2] == 0 and r['alpha'].shape == (64, 64) and r['n_cand'].dtype == np.int32
        assert not r['ambiguous'][30, 3] and not r['ambiguous'][32, 30]
        # half a pixel outside: m = (0.5 / 32)^2, alpha = 1 / (1 + exp(m / sigma))
        a = SR.silhouette(_triangle(4.0), faces, CAM64, brute=brute)['alpha'].numpy()
        assert abs(a[30, 3] - 1 / (1 + math.exp((0.5 / 32) ** 2 / sigma))) < 1e-15
        # at distance sqrt(blur_radius): just inside the cut alpha = 1e-4 (that is what blur_radius is made from), just outside exactly 0
        near = SR.silhouette(_triangle(3.5 + r_px * (1 - 1e-7)), faces, CAM64, brute=brute, analyse=True)
        far = SR.silhouette(_triangle(3.5 + r_px * (1 + 1e-7)), faces, CAM64, brute=brute, analyse=True)
        assert abs(near['alpha'].numpy()[30, 3] - 1e-4) < 1e-4 * 1e-5 and near['n_cand'][30, 3] == 1
        assert far['alpha'].numpy()[30, 3] == 0 and far['n_cand'][30, 3] == 0
        assert near['ambiguous'][30, 3] and far['ambiguous'][30, 3]     # within 1e-5 of the cut, relative: both are called ambiguous
    # blur_radius = 0: only inside faces contribute
    r = SR.silhouette(_triangle(4.0), faces, CAM64, blur_radius=0.0)
    assert r['alpha'].numpy()[30, 3] == 0 and r['alpha'].numpy()[30, 4] > 0.5 and (r['n_cand'] <= 1).all()
    # a vertex at z <= 0 drops the face whole; zero screen area is skipped
    behind = _triangle(3.5)
    behind[1, 2] = 0.0
    assert (SR.silhouette(behind, faces, CAM64)['alpha'] == 0).all()
    assert (SR.silhouette(torch.tensor([[1., 1., 1.], [2., 2., 1.], [3., 3., 1.]], dtype=torch.float64), faces, CAM64)['alpha'] == 0).all()


def _three_faces():
    verts = np.array([[-0.5, -0.4, 2.0], [0.45, -0.35, 2.3], [0.05, 0.4, 1.9], [0.6, 0.45, 2.2], [-0.55, 0.5, 2.1]], np.float64)
    return verts, np.array([[0, 1, 2], [1, 3, 2], [0, 2, 4]])


def test_helper_gradient_against_central_differences():
    verts, faces = _three_faces()
    cam = (EYE, 14.0, 13.0, 6.2, 5.1, 12, 10)
    sigma, blur = 1e-2, SR.default_blur_radius(1e-2)
    r = SR.silhouette(verts, faces, cam, sigma, blur, analyse=True)
    a = r['alpha'].numpy()
    assert ((a > 1e-3) & (a < 1 - 1e-3)).sum() > 20 and r['n_cand'].max() >= 2 and r['ambiguous'].sum() <= 2
    g_alpha = np.random.default_rng(1).standard_normal((10, 12)) * ~r['ambiguous']
    g = SR.gradient(verts, faces, cam, g_alpha, sigma, blur)
    h = 1e-6
    fd = np.zeros_like(verts)
    for i in range(verts.shape[0]):
        for j in range(3):
            up, dn = verts.copy(), verts.copy()
            up[i, j] += h
            dn[i, j] -= h
            lu = (SR.silhouette(up, faces, cam, sigma, blur)['alpha'].numpy() * g_alpha).sum()
            ld = (SR.silhouette(dn, faces, cam, sigma, blur)['alpha'].numpy() * g_alpha).sum()
            fd[i, j] = (lu - ld) / (2 * h)
    assert np.abs(g).max() > 0.1
    assert np.abs(g - fd).max() < 1e-6 * np.abs(g).max(), (np.abs(g - fd).max(), np.abs(g).max())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_brute_force_agrees_with_bounding_box_candidates(dtype):
    from neuman_hip import synthetic
    verts, faces = synthetic.capsule_mesh(6, 7)
    cap = synthetic.SimpleCapture(20, 14, c2w=synthetic.spherical_c2w(30., -20., 1.3))
    cam = SR.camera_of(cap)
    for sigma in (1e-2, 1e-3):
        a, b = (SR.silhouette(verts, faces, cam, sigma, dtype=dtype, brute=br, analyse=True) for br in (False, True))
        assert b['n_pairs'] == len(faces) * 20 * 14 and a['n_pairs'] < b['n_pairs']
        assert np.array_equal(a['n_cand'], b['n_cand']) and a['n_cand'].max() > 2
        assert np.array_equal(a['alpha'].numpy(), b['alpha'].numpy()) and np.array_equal(a['keep'].numpy(), b['keep'].numpy())
        assert np.array_equal(a['ambiguous'], b['ambiguous'])
        assert a['alpha'].dtype == dtype and 0 < (a['alpha'] > 0).sum() < 20 * 14
    g = np.random.default_rng(2).standard_normal((14, 20))
    ga, gb = (SR.gradient(verts, faces, cam, g, 1e-2, dtype=dtype, brute=br) for br in (False, True))
    assert np.abs(ga).max() > 0 and np.array_equal(ga, gb)


def test_pure_functions_against_the_references_recorded_values():
    from neuman_hip import optimize_smpl as O
    G = np.load(os.path.join(HERE, "golden", "optimize_smpl.npz"))
    for coco, want in zip(G['coco'], G['smpl2d']):
        got = O.coco_to_smpl(coco)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    with pytest.raises(AssertionError):
        O.coco_to_smpl(np.zeros((17, 3)))
    assert O.densepose_name_to_idx() == json.loads(str(G['name_to_idx']))
    assert list(O.densepose_name_to_idx()) == list(json.loads(str(G['name_to_idx'])))             # the order of the parts too
    for dp, want in zip(G['maps'], G['masks']):
        got = O.turn_smpl_gradient_on(dp)
        assert got.shape == (72,) and got.dtype == want.dtype and np.array_equal(got, want)
    lim = O.clip_smpl_vals()
    assert lim.shape == (72, 2) and lim.dtype == G['limits'].dtype and np.array_equal(lim, G['limits'])


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    lib = _lib.lib()
    # the checks run before the handle or any pointer is looked at: a block of host memory stands in for them
    dummy = (ctypes.c_char * 256)()
    d = ctypes.cast(dummy, ctypes.c_void_p)
    w2c = (ctypes.c_double * 12)(*EYE.reshape(-1))
    nan, inf = float('nan'), float('inf')
    good = dict(h=d, verts=d, w2c=w2c, fx=8.0, fy=8.0, cx=4.0, cy=4.0, W=8, H=8, sigma=1e-4, blur=1e-3, a=d, b=d, c=d)
    bad = [dict(h=None), dict(verts=None), dict(w2c=None), dict(a=None), dict(b=None), dict(W=0), dict(H=0), dict(W=-4), dict(W=1 << 16, H=1 << 16),
           dict(fx=nan), dict(fy=nan), dict(cx=nan), dict(cy=nan), dict(sigma=0.0), dict(sigma=-1e-4), dict(sigma=nan), dict(sigma=inf), dict(sigma=1e-60),
           dict(blur=-1e-9), dict(blur=nan), dict(blur=inf)]
    for over in bad:
        k = dict(good, **over)
        args = (k['h'], k['verts'], k['w2c'], k['fx'], k['fy'], k['cx'], k['cy'], k['W'], k['H'], k['sigma'], k['blur'], k['a'], k['b'])
        assert lib.nm_raster_silhouette(*args, None, None) == -1 and b"nm_raster_silhouette:" in lib.nm_last_error(), over
        assert lib.nm_raster_silhouette_backward(*args, k['c'], None) == -1 and b"nm_raster_silhouette_backward:" in lib.nm_last_error(), over
    k = good
    args = (k['h'], k['verts'], k['w2c'], k['fx'], k['fy'], k['cx'], k['cy'], k['W'], k['H'], k['sigma'], k['blur'], k['a'], k['b'])
    assert lib.nm_raster_silhouette_backward(*args, None, None) == -1 and b"nm_raster_silhouette_backward:" in lib.nm_last_error()    # null g_verts


def test_cpu_tensors_are_refused():
    from neuman_hip import render_utils, synthetic
    cap = synthetic.SimpleCapture(16, 16, c2w=synthetic.spherical_c2w(30, -20, 1.3))
    verts, faces = synthetic.capsule_mesh(4, 5)
    for v in (torch.from_numpy(verts), verts, torch.from_numpy(verts).requires_grad_(True)):
        with pytest.raises(_lib.NeumanHipError):
            render_utils.soft_silhouette(v, faces, cap)


def test_vertext_forward_on_the_cpu_is_the_skinning_chain_from_the_t_pose():
    """reference :105-130 in float64: world = scale * align^T * T(pose) applied to the T-pose vertices; the joints are the chain's own, and at
    rest both are the shaped template under the alignment"""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import smpl, synthetic
    model = smpl.SMPLDiff(synthetic.smpl_like_model(0), 'cpu').double()
    poses, betas, aligns = synthetic.smpl_like_frames(1)
    align = np.eye(4)
    align[:, :3] = aligns["00000.png"]
    align = torch.as_tensor(align)
    beta = torch.as_tensor(betas[0]).double()
    v0, j0 = O.vertext_forward(torch.zeros(72, dtype=torch.float64), beta, align, model, 1.7)
    assert v0.shape == (1, 6890, 3) and j0.shape == (1, 24, 3)
    _, joints, v_shaped = model.joint_transformations(torch.zeros(1, 72, dtype=torch.float64), beta[None])
    M = torch.diag(torch.tensor([1.7, 1.7, 1.7, 1.0], dtype=torch.float64)) @ align.T
    hom = lambda x: torch.cat([x, torch.ones_like(x[:, :1])], 1)                                   # noqa: E731
    assert torch.allclose(v0[0], (hom(v_shaped) @ M.T)[:, :3], atol=1e-12) and torch.allclose(j0[0], (hom(joints) @ M.T)[:, :3], atol=1e-12)
    # posed: the vertices agree with HumanNeRF.vertex_forward's chain when its canonical pose is at rest, and the gradient reaches the pose
    pose = torch.as_tensor(poses[0]).double().requires_grad_(True)
    v, j = O.vertext_forward(pose, beta, align, model, 1.7)
    want, _ = model.vertex_forward_torch(pose[None], beta[None], align, 1.7, da_pose=torch.zeros(1, 72, dtype=torch.float64))
    assert torch.allclose(v, want, atol=1e-10)
    (v.sum() + j.sum()).backward()
    assert pose.grad.abs().min() > 0
