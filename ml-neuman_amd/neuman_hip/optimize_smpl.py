"""Per-frame refinement of the SMPL pose against the detected mask and 2-D joints -- reference preprocess/optimize_smpl.py.

    coco_to_smpl, densepose_name_to_idx, densepose_idx_to_name      :33-81
    vertext_forward                                                 :105-130
    turn_smpl_gradient_on, clip_smpl_vals                           :133-193
    optimize_smpl                                                   :196-256

The reference renders the body's soft silhouette with pytorch3d (:84-102); here it is `render_utils.soft_silhouette` (csrc/silhouette.hip,
include/neuman_hip.h 'soft silhouette': every face within the blur radius counts, not the 100 nearest).  The body is skinned by the
hand-written kernels of `SMPLDiff.vertex_forward`; the 24 joints, which are tiny, go through SMPLDiff's tensor algebra.  The file handling of the
reference's main() / dump_visualizations() is not here: `data_io.py` reads what they read.

    main's loop over the captures                                   :277-293    optimize_scene, over optimize_smpl_sequence

A video's frames are independent problems of one topology and one image size: `optimize_smpl_sequence` fits `frames_per_batch` of them at a
time on the batched kernels (`SMPLDiff.vertex_forward_batch`, `render_utils.soft_silhouette_batch`), a handful of launches and one host read per
iteration whatever the number of frames, and every frame takes exactly the steps it would take alone.
"""
import os

import numpy as np
import torch

from . import raster, render_utils

# SMPL joint <- COCO keypoint: hips, knees, ankles, shoulders, elbows, wrists (:41-52); the other SMPL joints have no COCO partner and stay 0
_SMPL_FROM_COCO = {1: 11, 2: 12, 4: 13, 5: 14, 7: 15, 8: 16, 16: 5, 17: 6, 18: 7, 19: 8, 20: 9, 21: 10}

_DENSEPOSE_PARTS = (('Torso', (1, 2)), ('Right Hand', (3,)), ('Left Hand', (4,)), ('Left Foot', (5,)), ('Right Foot', (6,)),
                    ('Upper Leg Right', (7, 9)), ('Upper Leg Left', (8, 10)), ('Lower Leg Right', (11, 13)), ('Lower Leg Left', (12, 14)),
                    ('Upper Arm Left', (15, 17)), ('Upper Arm Right', (16, 18)), ('Lower Arm Left', (19, 21)), ('Lower Arm Right', (20, 22)),
                    ('Head', (23, 24)))

# the pose entries (joint, axes) that a visible DensePose part frees (:141-164): limbs only
_FREED_BY = {'Upper Leg Left': (1, (0, 2)), 'Upper Leg Right': (2, (0, 2)), 'Lower Leg Left': (4, (0,)), 'Lower Leg Right': (5, (0,)),
             'Left Foot': (7, (0, 1, 2)), 'Right Foot': (8, (0, 1, 2)), 'Upper Arm Left': (16, (1, 2)), 'Upper Arm Right': (17, (1, 2)),
             'Lower Arm Left': (18, (1,)), 'Lower Arm Right': (19, (1,))}

# joint-angle ranges in degrees, (joint, axis): (low, high); every other entry is (-360, 360) (:173-192)
_LIMITS_DEG = {(4, 0): (0, 160), (4, 1): (0, 0), (4, 2): (0, 0), (5, 0): (0, 160), (5, 1): (0, 0), (5, 2): (0, 0),                   # knees
               (7, 0): (-45, 90), (7, 1): (-60, 60), (7, 2): (-10, 10), (8, 0): (-45, 90), (8, 1): (-60, 60), (8, 2): (-10, 10),     # feet
               (18, 1): (-160, 0), (19, 2): (0, 160)}                                                                                # elbows


def coco_to_smpl(coco2d):
    """2-D joints in COCO order [17,2] -> SMPL order [24,2]; joints COCO does not have are zeros."""
    coco2d = np.asarray(coco2d)
    assert coco2d.shape == (17, 2)
    smpl2d = np.zeros((24, 2))
    for s, c in _SMPL_FROM_COCO.items():
        smpl2d[s] = coco2d[c]
    return smpl2d


def densepose_name_to_idx():
    return {name: list(labels) for name, labels in _DENSEPOSE_PARTS}


def densepose_idx_to_name():
    return {label: name for name, labels in _DENSEPOSE_PARTS for label in labels}


def turn_smpl_gradient_on(dp_mask):
    """[72] of 0 / 1: the pose entries that may move, given the DensePose labels present in dp_mask -- the limbs that are seen."""
    present = set(np.unique(dp_mask).tolist())
    names = densepose_idx_to_name()
    visible = {names[i] for i in range(1, 25) if i in present}
    grad_mask = np.zeros([24, 3])
    for name, (joint, axes) in _FREED_BY.items():
        if name in visible:
            grad_mask[joint, list(axes)] = 1
    return grad_mask.reshape(-1)


def clip_smpl_vals():
    """[72,2] (low, high) in radians: a pose entry outside its open range no longer moves (a knee has one degree of freedom)."""
    limits = np.ones([24, 3, 2])
    limits[..., 0] *= -360
    limits[..., 1] *= 360
    for (joint, axis), lim in _LIMITS_DEG.items():
        limits[joint, axis] = lim
    return limits.reshape(-1, 2) / 180 * np.pi


def vertext_forward(pose, betas, align, body_model, scale):
    """pose [72], betas [10], align [4,4] (its TRANSPOSE is applied), body_model an `smpl.SMPLDiff`, scale -> world_verts [1,V,3],
    world_joints [1,24,3]: scale * align^T * (the skinning transform from the T pose) applied to the T-pose vertices and joints (:105-130),
    differentiable with respect to pose.  (The name is the reference's.)"""
    pose2, beta2 = pose.reshape(1, -1), betas.reshape(1, -1)
    A, joints, v_shaped = body_model.joint_transformations(pose2, beta2)
    s = torch.eye(4, dtype=A.dtype, device=A.device)
    s[:3, :3] *= scale
    M = s @ align.to(A.dtype).T
    hom = lambda x: torch.cat([x, torch.ones_like(x[:, :1])], 1)                                   # noqa: E731
    world_joints = torch.einsum('ab,jbc,jc->ja', M, A, hom(joints))[:, :3]
    if pose.is_cuda and pose.dtype == torch.float32 and isinstance(scale, (int, float)):
        # csrc/smpl.hip's kernels, forward and backward: with the canonical pose at rest its transform is the identity, and what is left of
        # HumanNeRF.vertex_forward is this function
        world_verts = body_model.vertex_forward(pose2, beta2, align, float(scale), da_pose=torch.zeros_like(pose2))[0]
    else:
        T = torch.einsum('vj,jab->vab', body_model.lbs_weights, A)
        world_verts = torch.einsum('ab,vbc,vc->va', M, T, hom(v_shaped))[None, :, :3]
    return world_verts, world_joints[None]


def project_joints(world_joints, K, w2c, shape):
    """pcd_projector.pcd_3d_to_pcd_2d_torch as :236-243 calls it (crop and filter_neg on, pixel coordinates, no depth): [N,3] -> [N,2];
    a joint with a zero coordinate, at z <= 0 or off the frame is (0, 0) and carries no gradient.  (The crop has no lower bound on y.)"""
    H, W = shape
    cam = torch.einsum('ab,nb->na', (K @ w2c), torch.cat([world_joints, torch.ones_like(world_joints[:, :1])], 1))
    valid = (world_joints != 0).all(1) & (cam[:, 2] > 0)
    # (a masked joint divides by 1, not by its own depth: 0 / 0 would put a NaN into every gradient, masked or not)
    uv = cam[:, :2] * valid[:, None].to(cam.dtype) / torch.where(valid, cam[:, 2], torch.ones_like(cam[:, 2]))[:, None]
    valid = valid & (uv[:, 0] >= 0) & (uv[:, 0] < W - 1) & (uv[:, 1] < H - 1)
    return uv * valid[:, None].to(uv.dtype)


class Objective:
    """The loss of :245-251 for one capture: mse over the confident joints + mse(soft silhouette, mask).  `silhouette(world_verts [V,3])`
    -> alpha [H,W] is `render_utils.soft_silhouette` unless given (the tests put a float64 restatement there)."""

    def __init__(self, cap, smpl, faces, body_model, align, scale, sigma=1e-4, silhouette=None):
        self.body_model, self.scale = body_model, scale
        ref = body_model.v_template
        dev, dt = ref.device, ref.dtype
        self.betas = torch.as_tensor(np.asarray(smpl['betas']), dtype=dt, device=dev).reshape(-1)
        temp = np.eye(4)
        temp[..., :3] = np.asarray(align)
        self.align = torch.as_tensor(temp, dtype=dt, device=dev)
        self.mask_target = torch.as_tensor(np.asarray(cap.binary_mask)).to(dev, dt)
        keypoints = np.array(cap.keypoints, dtype=np.float64)                                      # (a copy: the reference edits cap.keypoints)
        joints_target = keypoints[:, :2]
        joints_target[keypoints[:, 2] < 0.3] = 0                                                   # low-confidence detections are dropped
        self.joints_target = torch.as_tensor(coco_to_smpl(joints_target)).to(dev, dt)
        self.joints_mask = self.joints_target.sum(dim=1) != 0
        w2c, fx, fy, cx, cy, W, H = raster.camera_of(cap)
        self.K = torch.tensor([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]], dtype=dt, device=dev)
        self.w2c = torch.as_tensor(w2c).to(dev, dt)
        self.shape = (H, W)
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()                                                   # (once, not every step)
        self.silhouette = silhouette if silhouette is not None else (lambda v: render_utils.soft_silhouette(v, faces, cap, sigma))

    def terms(self, pose):
        """-> (joint term, silhouette term); the joint term is 0 when no joint is confident (an mse over nothing is NaN)"""
        world_verts, world_joints = vertext_forward(pose, self.betas, self.align, self.body_model, self.scale)
        proj = project_joints(world_joints[0], self.K, self.w2c, self.shape)
        if bool(self.joints_mask.any()):
            joint_term = torch.nn.functional.mse_loss(proj[self.joints_mask], self.joints_target[self.joints_mask])
        else:
            joint_term = proj.sum() * 0
        return joint_term, torch.nn.functional.mse_loss(self.silhouette(world_verts[0]), self.mask_target)

    def loss(self, pose):
        joint_term, silhouette_term = self.terms(pose)
        return joint_term + silhouette_term


def optimize_smpl(cap, smpl, faces, body_model, align, scale, num_iters=100, sigma=1e-4):
    """:196-256 with the reference's names: Adam (lr 5e-3) on smpl['pose'] for num_iters steps of Objective.loss, the gradient masked by
    turn_smpl_gradient_on(cap.densepose) and by clip_smpl_vals() -> the refined pose, numpy [72].  `cap` carries pinhole_cam or
    intrinsic_matrix, cam_pose, binary_mask [H,W], keypoints [17,3] (COCO: x, y, confidence) and densepose [H,W]; `body_model` is an
    `smpl.SMPLDiff` on the device; `align` the frame's [4,3] alignment."""
    device = body_model.v_template.device
    objective = Objective(cap, smpl, faces, body_model, align, scale, sigma)
    pose = torch.nn.Parameter(torch.tensor(np.asarray(smpl['pose']), device=device).float().reshape(-1), requires_grad=True)
    optim = torch.optim.Adam([{"params": pose, "lr": 5e-3}])
    grad_mask = torch.from_numpy(turn_smpl_gradient_on(cap.densepose)).float().to(device)
    limits = torch.from_numpy(clip_smpl_vals()).float().to(device)
    for _ in range(num_iters):
        optim.zero_grad()
        objective.loss(pose).backward()
        valid_mask = ((pose < limits[..., 1]) * (pose > limits[..., 0])).float()
        pose.grad = pose.grad * grad_mask * valid_mask
        optim.step()
    return pose.detach().cpu().numpy()


def _alignment_of(alignments, cap, i):
    """the frame's [4,3] alignment: `alignments` is main()'s dict keyed by the image's file name (:269, :289), or one per capture in order"""
    if isinstance(alignments, dict):
        return alignments[os.path.basename(cap.image_path)]
    return alignments[i]


class SequenceObjective:
    """The sum over the captures of `Objective.loss`, every frame with its own normalisers (the mean over ITS confident joints, the mean over
    ITS pixels): only the sum is across frames, so row b of the gradient with respect to poses [B,72] is the gradient of frame b's own loss.
    On float32 CUDA poses the skinning and the silhouette are the batched kernels and everything between them is elementwise in the frame
    (no reduction or matrix product whose order could depend on B); elsewhere (the float64 restatement the tests check against) the
    skinning is `vertext_forward` frame by frame.  `silhouette(world_verts [B,V,3]) -> alpha [B,H,W]` is `render_utils.soft_silhouette_batch`
    unless given.  Every per-frame input is stacked on the host and uploaded once, here."""

    def __init__(self, caps, smpls, faces, body_model, alignments, scale, sigma=1e-4, silhouette=None):
        self.body_model, self.scale, self.B = body_model, scale, len(caps)
        ref = body_model.v_template
        dev, dt = ref.device, ref.dtype
        npdt = np.float32 if dt == torch.float32 else np.float64
        cams = [raster.camera_of(cap) for cap in caps]
        sizes = sorted({(c[5], c[6]) for c in cams})
        if len(sizes) != 1:
            raise ValueError(f"the captures of a sequence fit must share one image size, got (W, H) = {sizes}: group them by size")
        W, H = sizes[0]
        self.shape = (H, W)
        aligns, targets, P = [], [], []
        for i, (cap, cam) in enumerate(zip(caps, cams)):
            temp = np.eye(4)
            temp[..., :3] = np.asarray(_alignment_of(alignments, cap, i))
            aligns.append(temp)
            keypoints = np.array(cap.keypoints, dtype=np.float64)
            joints_target = keypoints[:, :2]
            joints_target[keypoints[:, 2] < 0.3] = 0
            targets.append(coco_to_smpl(joints_target))
            K = np.array([[cam[1], 0., cam[3]], [0., cam[2], cam[4]], [0., 0., 1.]])
            P.append(K.astype(npdt) @ cam[0].astype(npdt))                                         # K w2c, [3,4], in the objective's precision
        up = lambda a: torch.as_tensor(np.stack(a)).to(dev, dt)                                    # noqa: E731
        self.betas = up([np.asarray(s['betas']).reshape(-1) for s in smpls])
        self.align = up(aligns)
        self.mask_target = up([np.asarray(cap.binary_mask) for cap in caps])
        self.joints_target = up(targets)
        self.joints_mask = (self.joints_target.sum(dim=2) != 0).to(dt)                             # [B,24]
        self.joints_count = self.joints_mask.sum(dim=1).clamp(min=1) * 2                           # (x and y; a frame without a confident joint divides 0 by 2)
        self.P = up(P)
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        if silhouette is None:
            cameras = raster.batch_cameras(caps, dev)
            silhouette = lambda v: render_utils.soft_silhouette_batch(v, faces, cameras, sigma)     # noqa: E731
        self.silhouette = silhouette

    def forward_bodies(self, poses):
        """-> world_verts [B,V,3], world_joints [B,24,3]"""
        if poses.is_cuda and poses.dtype == torch.float32 and isinstance(self.scale, (int, float)):
            return self.body_model.vertex_forward_batch(poses, self.betas, self.align, float(self.scale), da_pose=torch.zeros_like(poses[:1]))
        out = [vertext_forward(poses[b], self.betas[b], self.align[b], self.body_model, self.scale) for b in range(self.B)]
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

    def project(self, world_joints):
        """`project_joints` for every frame, written elementwise: [B,24,3] -> [B,24,2]"""
        H, W = self.shape
        x, y, z = world_joints[..., 0], world_joints[..., 1], world_joints[..., 2]
        P = self.P[:, None]                                                                        # [B,1,3,4]
        cam = [((P[..., k, 0] * x + P[..., k, 1] * y) + P[..., k, 2] * z) + P[..., k, 3] for k in range(3)]
        valid = (world_joints != 0).all(2) & (cam[2] > 0)
        vf = valid.to(world_joints.dtype)
        depth = torch.where(valid, cam[2], torch.ones_like(cam[2]))
        u, v = cam[0] * vf / depth, cam[1] * vf / depth
        valid = valid & (u >= 0) & (u < W - 1) & (v < H - 1)
        return torch.stack([u, v], 2) * valid[..., None].to(u.dtype)

    def terms(self, poses):
        """-> (joint terms [B], silhouette terms [B]): frame b's are `Objective.terms` of frame b"""
        world_verts, world_joints = self.forward_bodies(poses)
        d = (self.project(world_joints) - self.joints_target) * self.joints_mask[..., None]
        joint_terms = (d * d).sum(dim=(1, 2)) / self.joints_count
        e = self.silhouette(world_verts) - self.mask_target
        return joint_terms, (e * e).sum(dim=(1, 2)) / float(self.shape[0] * self.shape[1])

    def loss(self, poses):
        joint_terms, silhouette_terms = self.terms(poses)
        return (joint_terms + silhouette_terms).sum()


def optimize_smpl_sequence(caps, smpls, faces, body_model, alignments, scale, num_iters=100, sigma=1e-4, frames_per_batch=32):
    """`optimize_smpl` for every capture of a sequence -> the refined poses, numpy [N,72] float32.  The N frames are fitted `frames_per_batch` at
    a time: one Adam (lr 5e-3) on a [B,72] parameter per chunk under `SequenceObjective.loss`, the gradient masked per frame by
    turn_smpl_gradient_on(cap.densepose) and clip_smpl_vals().  Adam is elementwise and every frame's gradient is its own, so a frame's result
    is the same bits whatever the chunking (alone, or anywhere in a chunk of any size).  `alignments`: main()'s dict keyed by
    os.path.basename(cap.image_path), or one [4,3] per capture.  All captures must share one image size (ValueError otherwise: group them).
    Masks, keypoints, cameras and gradient masks are uploaded once per chunk; inside the loop the only host read is the silhouette's list
    total, once per iteration."""
    N = len(caps)
    if len(smpls) != N:
        raise ValueError(f"{N} captures but {len(smpls)} smpls")
    if frames_per_batch < 1:
        raise ValueError(f"frames_per_batch must be >= 1, got {frames_per_batch}")
    sizes = sorted({raster.camera_of(cap)[5:] for cap in caps})
    if len(sizes) > 1:
        raise ValueError(f"the captures of a sequence fit must share one image size, got (W, H) = {sizes}: group them by size")
    device = body_model.v_template.device
    limits = torch.from_numpy(clip_smpl_vals()).float().to(device)
    out = np.zeros((N, 72), np.float32)
    for lo in range(0, N, frames_per_batch):
        idx = range(lo, min(lo + frames_per_batch, N))
        chunk = [caps[i] for i in idx]
        aligns = [_alignment_of(alignments, caps[i], i) for i in idx]
        objective = SequenceObjective(chunk, [smpls[i] for i in idx], faces, body_model, aligns, scale, sigma)
        start = np.stack([np.asarray(smpls[i]['pose'], np.float32).reshape(-1) for i in idx])
        poses = torch.nn.Parameter(torch.from_numpy(start).to(device), requires_grad=True)
        optim = torch.optim.Adam([{"params": poses, "lr": 5e-3}])
        grad_mask = torch.from_numpy(np.stack([turn_smpl_gradient_on(cap.densepose) for cap in chunk])).float().to(device)
        for _ in range(num_iters):
            optim.zero_grad()
            objective.loss(poses).backward()
            valid_mask = ((poses < limits[..., 1]) * (poses > limits[..., 0])).float()
            poses.grad = poses.grad * grad_mask * valid_mask
            optim.step()
        out[lo:lo + len(chunk)] = poses.detach().cpu().numpy()
    return out


def optimize_scene(caps, smpls, faces, body_model, alignments, scale, **kw):
    """The loop of main() (:277-293) over a scene's captures on the batched fit -> {1: {'pose': [N x [72] f32], 'betas': [N x the input
    betas, untouched]}}, the dict main() dumps as smpl_output_optimized.pkl.  `alignments` is alignments.npy's dict, keyed by
    os.path.basename(cap.image_path) as there; **kw go to `optimize_smpl_sequence` (num_iters, sigma, frames_per_batch).  Reading the scene
    and WRITING THE .pkl stay with the caller: the reference dumps with joblib, which is not a dependency of this package --
    `joblib.dump(result, path)` on the returned dict is the whole of it."""
    poses = optimize_smpl_sequence(caps, smpls, faces, body_model, alignments, scale, **kw)
    results = {1: {'pose': [], 'betas': []}}
    for i in range(len(caps)):
        results[1]['pose'].append(poses[i])
        results[1]['betas'].append(smpls[i]['betas'])
    return results
