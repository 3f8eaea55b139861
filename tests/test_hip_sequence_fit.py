"""-m gpu: the batched fit of a sequence's SMPL poses -- nm_raster_silhouette_batch / _backward_batch (csrc/silhouette.hip),
nm_smpl_vertex_forward_batch / _backward_batch (csrc/smpl.hip), SMPLDiff.vertex_forward_batch, render_utils.soft_silhouette_batch,
optimize_smpl.optimize_smpl_sequence / optimize_scene.

What a batch owes: frame b's outputs are the one-frame entries' BITS on frame b's inputs (torch.equal throughout), whatever B is and wherever
b sits.  What is new arithmetic (the world joints and their gradient, the per-frame objective) is held to float64 by the rule of
tests/test_hip_silhouette.py: the same computation in float32 torch is run beside the float64 one, and the device is allowed 4 x that run's own
worst deviation (floor 1e-6), relative to the largest component (tests/helpers/silhouette_ref.tolerance).  The measured figures are printed
([sequence-fit] lines; profiles/sequence_fit.md keeps a copy)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import silhouette_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

VIEWS = ((30., -20., 1.3), (75., 10., 1.6), (-40., -35., 1.15))      # spherical_c2w: angles and radii of the three cameras
TWISTS = (0.8, -0.5, 1.4)


# ---- 1: the silhouette batch ---------------------------------------------------------------------------------------------------------
def _frames(shape, W, H, views=VIEWS, twists=TWISTS):
    """-> faces, V, verts [B,V,3] (device), caps: one mesh under B twists, seen by B cameras"""
    from neuman_hip import synthetic
    verts, faces = synthetic.capsule_mesh(*shape)
    posed = np.stack([synthetic.twist_transforms(verts, twist=t)[0] for t in twists])
    caps = [synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(*v)) for v in views]
    return faces, verts.shape[0], torch.as_tensor(posed).cuda(), caps


def _g_alpha(B, H, W, seed=7):
    return torch.as_tensor(np.random.default_rng(seed).standard_normal((B, H, W)).astype(np.float32)).cuda()


def _one_by_one(R, verts, caps, sigma, g_alpha):
    from neuman_hip import raster
    blur = raster.default_blur_radius(sigma)
    out = []
    for b, cap in enumerate(caps):
        cam = raster.camera_of(cap)
        alpha, keep, n_cand = R.silhouette(verts[b], cam, sigma, blur, want_count=True)
        out.append((alpha, keep, n_cand, R.silhouette_backward(verts[b], cam, sigma, blur, keep, g_alpha[b])))
    return [torch.stack(x) for x in zip(*out)]


def _batched(R, verts, caps, sigma, g_alpha):
    from neuman_hip import raster
    blur = raster.default_blur_radius(sigma)
    cams = raster.batch_cameras(caps, verts.device)
    alpha, keep, n_cand = R.silhouette_batch(verts, cams, sigma, blur, want_count=True)
    return [alpha, keep, n_cand, R.silhouette_backward_batch(verts, cams, sigma, blur, keep, g_alpha)]


NAMES = ('alpha', 'keep', 'n_cand', 'g_verts')


def _same(a, b, what=''):
    for k, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (what, k)


@pytest.mark.parametrize("case", ["whole_tiles", "ragged_tiles"])
def test_silhouette_batch_is_the_one_frame_entry_bit_for_bit(case):
    from neuman_hip import raster
    shape, W, H, sigma = {'whole_tiles': ((40, 38), 96, 64, 1e-2), 'ragged_tiles': ((84, 82), 37, 29, 1e-2)}[case]
    faces, V, verts, caps = _frames(shape, W, H)
    R = raster.Rasterizer(faces, V)
    g = _g_alpha(3, H, W)
    one = _one_by_one(R, verts, caps, sigma, g)
    bat = _batched(R, verts, caps, sigma, g)
    for b in range(3):                                                   # the frames differ, each is seen, each has a gradient
        assert int((one[0][b] > 0).sum()) > 50 and float(one[3][b].abs().max()) > 0 and int(one[2][b].max()) >= 2
    assert not torch.equal(one[0][0], one[0][1]) and not torch.equal(one[0][1], one[0][2])
    if case == 'ragged_tiles':
        assert int(one[2].max()) > 256                                   # more than one LDS batch in a pixel's list
    _same(bat, one, case)
    _same(_batched(R, verts, caps, sigma, g), bat, 'second run')         # the same bits on every run
    R.close()


def test_silhouette_batch_positions_sizes_and_scratch_reuse():
    """B = 1; the same frame at positions 0 and 2; a smaller batch after a larger one on the same handle; a batch through a fresh handle"""
    from neuman_hip import raster
    W, H, sigma = 96, 64, 1e-2
    faces, V, verts, caps = _frames((40, 38), W, H)
    R = raster.Rasterizer(faces, V)
    g = _g_alpha(3, H, W)
    one = _one_by_one(R, verts, caps, sigma, g)
    # frame 1 alone, as a batch of one
    b1 = _batched(R, verts[1:2], caps[1:2], sigma, g[1:2])
    _same(b1, [x[1:2] for x in one], 'B = 1')
    # frame 0 at positions 0 and 2 of a batch of three
    order = [0, 1, 0]
    rep = _batched(R, verts[order].contiguous(), [caps[i] for i in order], sigma, g[order].contiguous())
    _same(rep, [x[order] for x in one], 'positions 0 and 2')
    # five frames (the scratch grows), then two (it is reused), on the same handle
    order = [2, 0, 1, 1, 2]
    five = _batched(R, verts[order].contiguous(), [caps[i] for i in order], sigma, g[order].contiguous())
    _same(five, [x[order] for x in one], 'B = 5')
    two = _batched(R, verts[1:3].contiguous(), caps[1:3], sigma, g[1:3].contiguous())
    _same(two, [x[1:3] for x in one], 'B = 2 after B = 5')
    fresh = raster.Rasterizer(faces, V)
    _same(_batched(fresh, verts, caps, sigma, g), one, 'fresh handle')
    fresh.close()
    R.close()


def test_silhouette_batch_with_an_empty_frame_between_two_seen_ones():
    from neuman_hip import raster, synthetic
    W, H, sigma = 96, 64, 1e-2
    faces, V, verts, caps = _frames((40, 38), W, H)
    caps[1] = synthetic.SimpleCapture(W, H, c2w=caps[1].cam_pose.camera_to_world @ np.diag([1., -1., -1., 1.]))      # turned away
    R = raster.Rasterizer(faces, V)
    g = _g_alpha(3, H, W)
    one = _one_by_one(R, verts, caps, sigma, g)
    bat = _batched(R, verts, caps, sigma, g)
    assert bool((bat[0][1] == 0).all()) and bool((bat[1][1] == 1).all()) and bool((bat[2][1] == 0).all()) and bool((bat[3][1] == 0).all())
    assert int((bat[0][0] > 0).sum()) > 50 and int((bat[0][2] > 0).sum()) > 50
    _same(bat, one, 'empty middle frame')
    R.close()


# ---- 2: argument checks -----------------------------------------------------------------------------------------------------------------
def test_silhouette_batch_argument_checks_leave_the_device_usable():
    from neuman_hip import _lib, raster
    W, H, sigma = 96, 64, 1e-2
    faces, V, verts, caps = _frames((40, 38), W, H)
    R = raster.Rasterizer(faces, V)
    lib = _lib.lib()
    blur = raster.default_blur_radius(sigma)
    w2c, intr, _, _ = raster.batch_cameras(caps, verts.device)
    alpha, keep = torch.full((3, H, W), 7., device='cuda'), torch.full((3, H, W), 7., device='cuda')
    p = _lib.dev_ptr

    def call(B=3, keep_=keep, sigma_=sigma, w2c_=w2c):
        rc = lib.nm_raster_silhouette_batch(R._h, p(verts), p(w2c_, torch.float64), p(intr, torch.float64), B, W, H, sigma_, blur, p(alpha), p(keep_), None,
                                            _lib.stream_ptr())
        return rc, lib.nm_last_error()

    for over in (dict(B=0), dict(keep_=None), dict(sigma_=0.0), dict(sigma_=-1e-2)):
        rc, msg = call(**over)
        assert rc == -1 and b"nm_raster_silhouette_batch:" in msg, (over, rc, msg)
    torch.cuda.synchronize()
    assert bool((alpha == 7).all()) and bool((keep == 7).all())          # refused before any device work
    bad = w2c.clone()
    bad[1, 1, 2] = float('nan')
    rc, msg = call(w2c_=bad)
    torch.cuda.synchronize()
    assert rc == -1 and b"nm_raster_silhouette_batch:" in msg and b"frame 1" in msg, (rc, msg)
    one = _one_by_one(R, verts, caps, sigma, _g_alpha(3, H, W))
    assert bool((alpha[1] == 0).all()) and bool((keep[1] == 1).all())    # the frame's outputs are defined
    for b in (0, 2):
        assert torch.equal(alpha[b], one[0][b]) and torch.equal(keep[b], one[1][b])
    with pytest.raises(_lib.NeumanHipError, match="nm_raster_silhouette_batch"):
        R.silhouette_batch(verts, (bad, intr, W, H), sigma, blur)
    g = R.silhouette_backward_batch(verts, (bad, intr, W, H), sigma, blur, one[1], _g_alpha(3, H, W))
    assert bool((g[1] == 0).all()) and torch.equal(g[0], one[3][0]) and torch.equal(g[2], one[3][2])
    # the device stays usable: a valid call passes
    _same(_batched(R, verts, caps, sigma, _g_alpha(3, H, W)), one, 'after the refusals')
    R.close()


# ---- 3: the skinning batch -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body():
    from neuman_hip import smpl, synthetic
    model = synthetic.smpl_like_model(0)
    return smpl.SMPLDiff(model, 'cuda'), model


def _leaf(x, dtype=torch.float32, device='cuda'):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=device, requires_grad=True)


def _skin_inputs(B):
    from neuman_hip import synthetic
    pose, betas, align = synthetic.smpl_like_frames(B, 0)
    al = np.stack([np.concatenate([align[f'{f:05d}.png'], np.array([[0.], [0.], [0.], [1.]])], 1) for f in range(B)])
    return pose * 0.7, betas * 0.5, al


@pytest.mark.parametrize("B", [1, 3, 5])
def test_skinning_batch_is_the_one_frame_entries_bit_for_bit(body, B):
    """g_joints null (nothing reads the joints): world, g_pose, g_beta and g_align of every frame against SMPLDiff.vertex_forward"""
    b, _ = body
    pose, betas, al = _skin_inputs(B)
    V = b.v_template.shape[0]
    gw = torch.randn((B, V, 3), device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
    P, Be, Al = _leaf(pose), _leaf(betas), _leaf(al)
    world, joints = b.vertex_forward_batch(P, Be, Al, 1.3)
    assert world.shape == (B, V, 3) and joints.shape == (B, 24, 3)
    (world * gw).sum().backward()
    for f in range(B):
        p, be, a = _leaf(pose[f][None]), _leaf(betas[f][None]), _leaf(al[f])
        w1, _ = b.vertex_forward(p, be, a, 1.3)
        (w1[0] * gw[f]).sum().backward()
        assert torch.equal(world[f], w1[0].detach()), f
        assert float(p.grad.abs().max()) > 0 and torch.equal(P.grad[f], p.grad[0]) and torch.equal(Be.grad[f], be.grad[0]) and torch.equal(Al.grad[f], a.grad), f
    # the same bits on a second run
    P2, Be2, Al2 = _leaf(pose), _leaf(betas), _leaf(al)
    world2, joints2 = b.vertex_forward_batch(P2, Be2, Al2, 1.3)
    (world2 * gw).sum().backward()
    assert torch.equal(world2, world) and torch.equal(joints2, joints) and torch.equal(P2.grad, P.grad) and torch.equal(Be2.grad, Be.grad) and torch.equal(Al2.grad, Al.grad)


@pytest.mark.parametrize("B", [1, 3, 5])
def test_skinning_batch_joints_and_their_gradients_against_float64(body, B):
    """joints_out against the float64 joint_transformations route (optimize_smpl.vertext_forward on the CPU); with g_joints given, g_pose,
    g_beta and g_align against float64 autograd; the allowance is 4 x what the same computation in float32 torch deviates by"""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import smpl
    b, model = body
    pose, betas, al = _skin_inputs(B)
    V = b.v_template.shape[0]
    rng = np.random.default_rng(6)
    gw, gj = rng.standard_normal((B, V, 3)).astype(np.float32), (rng.standard_normal((B, 24, 3)) * 40).astype(np.float32)
    res = {}
    for name, dtype in (('f64', torch.float64), ('f32', torch.float32)):
        cpu = smpl.SMPLDiff(model, 'cpu').to(dtype)
        P, Be, Al = (_leaf(x, dtype, 'cpu') for x in (pose, betas, al))
        out = [O.vertext_forward(P[f], Be[f], Al[f], cpu, 1.3) for f in range(B)]
        world, joints = torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
        ((world * torch.as_tensor(gw).to(dtype)).sum() + (joints * torch.as_tensor(gj).to(dtype)).sum()).backward()
        res[name] = [x.detach().double().numpy() for x in (world, joints, P.grad, Be.grad, Al.grad)]
    P, Be, Al = _leaf(pose), _leaf(betas), _leaf(al)
    world, joints = b.vertex_forward_batch(P, Be, Al, 1.3, da_pose=torch.zeros((1, 72), device='cuda'))
    ((world * torch.as_tensor(gw).cuda()).sum() + (joints * torch.as_tensor(gj).cuda()).sum()).backward()
    got = [x.detach().double().cpu().numpy() for x in (world, joints, P.grad, Be.grad, Al.grad)]
    # the joints' share of the gradient is not lost in the vertices': without it the result differs
    P0, Be0, Al0 = _leaf(pose), _leaf(betas), _leaf(al)
    w0, _ = b.vertex_forward_batch(P0, Be0, Al0, 1.3, da_pose=torch.zeros((1, 72), device='cuda'))
    (w0 * torch.as_tensor(gw).cuda()).sum().backward()
    assert float((P0.grad - P.grad).abs().max()) > 1e-3 * float(P.grad.abs().max())
    for what, x, r64, r32 in zip(("world", "joints", "g_pose", "g_beta", "g_align"), got, res['f64'], res['f32']):
        for f in range(B):
            tol, f32dev = SR.tolerance(r64[f], r32[f], relative=True)
            err = float(np.abs(x[f] - r64[f]).max())
            print(f"[sequence-fit] skinning B = {B}, frame {f}, {what}: largest component {np.abs(r64[f]).max():.3e}; device vs float64 | float32 torch vs float64 | "
                  f"allowed: {err:.2e} | {f32dev:.2e} | {tol:.2e}")
            assert np.abs(r64[f]).max() > 0 and err <= tol, (what, f, err, tol)


# ---- 4, 5: the sequence fit ---------------------------------------------------------------------------------------------------------------
ANGLES = (0.15, 0.10, -0.12)                                             # joints 16 and 17 on their free axes, per frame
FIT_VIEWS = ((20., -10., 3.0), (28., -6., 3.2), (12., -14., 2.9))


def _fit_setup(W, H):
    """tests/test_hip_silhouette.py's fit, three frames of it: the synthetic body at rest; frame i's target is the body with joints 16 and
    17 (upper arms) turned by ANGLES[i] on their free axes, seen by camera i: its body_mask is the detected mask, its projected joints are
    the keypoints (confidence 1).  Frames 0 and 1 see every DensePose label, frame 2 only the arms'."""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import render_utils, smpl, synthetic
    model = synthetic.smpl_like_model(0)
    body = smpl.SMPLDiff(model, 'cuda')
    faces = model['f'].astype(np.int32)
    aligns = {f"{i:05d}.png": np.eye(4)[:, :3] for i in range(3)}
    caps, smpls = [], []
    eye = torch.eye(4, device='cuda')
    for i in range(3):
        cap = synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(*FIT_VIEWS[i]))
        cap.image_path = f"/scene/images/{i:05d}.png"
        target = np.zeros(72, np.float32)
        target[[16 * 3 + 1, 16 * 3 + 2, 17 * 3 + 1, 17 * 3 + 2]] = ANGLES[i]
        w2c, fx, fy, cx, cy, _, _ = O.raster.camera_of(cap)
        K0 = torch.tensor([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]], device='cuda')
        with torch.no_grad():
            wv, wj = O.vertext_forward(torch.as_tensor(target).cuda(), torch.zeros(10, device='cuda'), eye, body, 1.0)
            mask = render_utils.body_mask(wv[0], faces, cap).cpu().numpy()
            proj = O.project_joints(wj[0], K0, torch.as_tensor(w2c).cuda().float(), (H, W)).cpu().numpy()
        keypoints = np.zeros((17, 3))
        keypoints[:, 2] = 1.0
        for s, c in O._SMPL_FROM_COCO.items():
            keypoints[c, :2] = proj[s]
        cap.binary_mask, cap.keypoints = mask.astype(np.float32), keypoints
        cap.densepose = np.arange(25).reshape(5, 5) if i < 2 else np.array([[0, 15, 16, 17, 18, 19, 20, 21, 22]])
        caps.append(cap)
        smpls.append(dict(pose=np.zeros(72, np.float32), betas=np.zeros(10, np.float32)))
    return caps, smpls, faces, body, model, aligns


@pytest.fixture(scope="module")
def fit():
    """the scene at 96 x 64 and its 20-iteration fit, made once and never written to"""
    from neuman_hip import optimize_smpl as O
    caps, smpls, faces, body, model, aligns = _fit_setup(96, 64)
    poses = O.optimize_smpl_sequence(caps, smpls, faces, body, aligns, 1.0, num_iters=20)
    poses.setflags(write=False)
    return dict(caps=caps, smpls=smpls, faces=faces, body=body, model=model, aligns=aligns, poses=poses)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_the_sequence_fit_descends_keeps_masked_entries_and_repeats(fit):
    from neuman_hip import optimize_smpl as O
    caps, smpls, faces, body, aligns, a = (fit[k] for k in ('caps', 'smpls', 'faces', 'body', 'aligns', 'poses'))
    assert isinstance(a, np.ndarray) and a.shape == (3, 72) and a.dtype == np.float32
    start = np.stack([s['pose'] for s in smpls])
    obj = O.SequenceObjective(caps, smpls, faces, body, aligns, 1.0)
    with torch.no_grad():
        before = obj.terms(torch.as_tensor(start).cuda())[1].cpu().numpy()
        after = obj.terms(torch.as_tensor(a.copy()).cuda())[1].cpu().numpy()
    n_free = []
    for b in range(3):
        assert 100 < caps[b].binary_mask.sum() < 96 * 64 / 2 and (caps[b].keypoints[5:, :2] > 0).all(1).sum() >= 10
        print(f"[sequence-fit] fit 96x64 frame {b}: silhouette mse {before[b]:.6e} at iteration 0, {after[b]:.6e} after 20 iterations")
        assert after[b] < before[b], b                                                              # (a)
        free = O.turn_smpl_gradient_on(caps[b].densepose) != 0
        n_free.append(int(free.sum()))
        assert np.array_equal(_bits(a[b][~free]), _bits(start[b][~free])) and (a[b][free] != start[b][free]).any(), b      # (b) the same bits
    assert n_free == [18, 18, 6]
    again = O.optimize_smpl_sequence(caps, smpls, faces, body, aligns, 1.0, num_iters=20)
    assert np.array_equal(_bits(a), _bits(again))                                                   # (c)


def test_a_frames_fit_does_not_depend_on_its_batch(fit):
    """(d) alone, in the batch of three, in chunks of 2 + 1: the same bits"""
    from neuman_hip import optimize_smpl as O
    caps, smpls, faces, body, aligns, a = (fit[k] for k in ('caps', 'smpls', 'faces', 'body', 'aligns', 'poses'))
    chunks = O.optimize_smpl_sequence(caps, smpls, faces, body, aligns, 1.0, num_iters=20, frames_per_batch=2)
    assert np.array_equal(_bits(chunks), _bits(a))
    for b in range(3):
        alone = O.optimize_smpl_sequence([caps[b]], [smpls[b]], faces, body, aligns, 1.0, num_iters=20)
        assert alone.shape == (1, 72) and np.array_equal(_bits(alone[0]), _bits(a[b])), b


def test_optimize_scene_is_the_sequence_fit_in_mains_dict(fit):
    from neuman_hip import optimize_smpl as O
    caps, smpls, faces, body, aligns, a = (fit[k] for k in ('caps', 'smpls', 'faces', 'body', 'aligns', 'poses'))
    betas = [s['betas'].copy() for s in smpls]
    out = O.optimize_scene(caps, smpls, faces, body, aligns, 1.0, num_iters=20)
    assert list(out) == [1] and list(out[1]) == ['pose', 'betas'] and len(out[1]['pose']) == len(out[1]['betas']) == 3
    for b in range(3):
        assert np.array_equal(_bits(out[1]['pose'][b]), _bits(a[b]))
        assert out[1]['betas'][b] is smpls[b]['betas'] and np.array_equal(out[1]['betas'][b], betas[b])


def _float64_hook(caps, faces, dtype):
    cams = [SR.camera_of(c) for c in caps]
    return lambda v: torch.stack([SR.silhouette(v[b], faces, cams[b], 1e-4, dtype=dtype)['alpha'] for b in range(len(cams))])


def test_the_sequence_fits_pose_gradient_against_float64():
    """(e) pose.grad [B,72] after one backward at 40 x 32 against SequenceObjective on the CPU in float64 through the helper"""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import smpl
    caps, smpls, faces, body, model, aligns = _fit_setup(40, 32)
    pose0 = (np.random.default_rng(5).standard_normal((3, 72)) * 0.05).astype(np.float32)
    grads = {}
    for name, dtype in (('f64', torch.float64), ('f32', torch.float32)):
        cpu = smpl.SMPLDiff(model, 'cpu').to(dtype)
        obj = O.SequenceObjective(caps, smpls, faces, cpu, aligns, 1.0, silhouette=_float64_hook(caps, faces, dtype))
        poses = torch.as_tensor(pose0).to(dtype).requires_grad_(True)
        obj.loss(poses).backward()
        grads[name] = poses.grad.double().numpy()
    poses = torch.as_tensor(pose0).cuda().requires_grad_(True)
    O.SequenceObjective(caps, smpls, faces, body, aligns, 1.0).loss(poses).backward()
    got = poses.grad.double().cpu().numpy()
    assert got.shape == (3, 72)
    for b in range(3):
        tol, f32dev = SR.tolerance(grads['f64'][b], grads['f32'][b], relative=True)
        err = float(np.abs(got[b] - grads['f64'][b]).max())
        print(f"[sequence-fit] fit 40x32 frame {b} pose.grad: largest component {np.abs(grads['f64'][b]).max():.3e}; device vs float64 | float32 torch vs float64 | "
              f"allowed: {err:.2e} | {f32dev:.2e} | {tol:.2e}")
        assert np.abs(grads['f64'][b]).max() > 0 and err <= tol, (b, err, tol)


def test_the_sequence_fit_is_as_close_to_float64_as_the_one_frame_fit(fit):
    """(f) 20 steps: the sequence fit and the one-frame optimize_smpl, each against a float64 run of the same 20 steps (SequenceObjective on
    the CPU with the float64 helper behind the silhouette hook); the sequence fit's largest pose deviation may be 4 x the one-frame fit's own"""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import smpl
    caps, smpls, faces, body, model, aligns, seq = (fit[k] for k in ('caps', 'smpls', 'faces', 'body', 'model', 'aligns', 'poses'))
    cpu = smpl.SMPLDiff(model, 'cpu').double()
    obj = O.SequenceObjective(caps, smpls, faces, cpu, aligns, 1.0, silhouette=_float64_hook(caps, faces, torch.float64))
    poses = torch.nn.Parameter(torch.as_tensor(np.stack([s['pose'] for s in smpls])).double())
    optim = torch.optim.Adam([{"params": poses, "lr": 5e-3}])
    grad_mask = torch.as_tensor(np.stack([O.turn_smpl_gradient_on(c.densepose) for c in caps]))
    limits = torch.as_tensor(O.clip_smpl_vals())
    for _ in range(20):
        optim.zero_grad()
        obj.loss(poses).backward()
        valid = ((poses < limits[..., 1]) * (poses > limits[..., 0])).double()
        poses.grad = poses.grad * grad_mask * valid
        optim.step()
    ref = poses.detach().numpy()
    single = np.stack([O.optimize_smpl(caps[b], smpls[b], faces, body, aligns[os.path.basename(caps[b].image_path)], 1.0, num_iters=20) for b in range(3)])
    d_seq, d_one = float(np.abs(seq - ref).max()), float(np.abs(single - ref).max())
    print(f"[sequence-fit] 20 steps at 96x64, largest pose deviation from the float64 run: sequence fit {d_seq:.3e}, one-frame fit {d_one:.3e} "
          f"(largest pose entry {np.abs(ref).max():.3e})")
    assert np.abs(ref).max() > 1e-2 and d_seq <= 4 * d_one, (d_seq, d_one)
