"""Host-side inputs and references of tests/test_body_edges_host.py and tests/test_hip_smpl_edges.py: tiny body models away from SMPL's one shape
(V = 6890, J = 24, NB = 10), poses at the edges of Rodrigues' formula, and the skinning chain of neuman_hip.smpl.SMPLDiff evaluated on the host in
float32 and float64.  Nothing here touches the device."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for _p in (ROOT, os.path.join(ROOT, "ml-neuman_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# the project's own tolerances at V = 6890, as a fraction of the largest entry: tests/test_hip_smpl.py `close` for outputs,
# tests/test_hip_smpl_diff.py for the gradients to pose, shape and alignment
TOL_OUT, TOL_GRAD = 2e-5, 2e-4
SCALE = 1.3

# (V, J, NB): one vertex; one short of / exactly / one past a wave; one short of / exactly / one past a workgroup (256 lanes, four waves); two and
# four workgroups with a ragged last one; the ABI's limits J = 64 (2 J = every lane of smpl_chain_kernel's workgroup) and NB = 32 (the workspace
# strides blocks * 32 against blocks * NB coincide only there); J = 3 is the smallest the wrappers take (da_pose() writes joints 1 and 2)
SHAPE_CASES = [(1, 3, 1), (63, 3, 1), (64, 24, 10), (65, 24, 10), (255, 24, 32), (256, 64, 10), (257, 64, 32), (513, 5, 3), (1025, 24, 10)]
POSE_KINDS = ["random", "zero", "tiny", "pi", "mixed"]
THROUGH = ["world", "T", "both"]
CASES = [(V, J, NB, kind) for (V, J, NB) in SHAPE_CASES for kind in POSE_KINDS]


def case_id(c):
    return "V{}-J{}-NB{}-{}".format(*c)


def small_body_model(V, J, NB, seed=0):
    """A body model with the keys SMPL / SMPLDiff / oracle.smpl.Model read, at any size: a random kinematic tree (parents[j] in [max(0, j-3), j)),
    joint anchors N(0,1) * (0.2, 0.5, 0.1), every vertex an anchor + N(0, 0.05); skinning weights exp(-d^2 / 0.02) with the 4 largest per vertex kept
    and the rest EXACTLY zero (as real SMPL has; the kernels skip zero weights), joint regressor exp(-d^2 / 0.005) with the 8 largest per joint kept;
    both normalised to sum to one.  (The exponent is taken relative to the row's smallest d^2 -- the same numbers after normalisation -- so that a
    joint far from every vertex does not underflow to 0 / 0.)"""
    rng = np.random.default_rng(seed)
    parents = np.zeros(J, np.int64)
    for j in range(1, J):
        parents[j] = rng.integers(max(0, j - 3), j)
    anchors = rng.normal(size=(J, 3)) * np.array([0.2, 0.5, 0.1])
    verts = anchors[rng.integers(0, J, V)] + rng.normal(size=(V, 3)) * 0.05
    d2 = ((verts[:, None, :] - anchors[None]) ** 2).sum(-1)                                        # [V,J]

    def keep_largest(x, k):                                                                        # per row
        if x.shape[1] > k:
            cut = np.sort(x, 1)[:, -k][:, None]
            x = np.where(x >= cut, x, 0.0)
        return x / x.sum(1, keepdims=True)

    w = keep_largest(np.exp(-(d2 - d2.min(1, keepdims=True)) / 0.02), 4)
    jr = keep_largest(np.exp(-(d2.T - d2.T.min(1, keepdims=True)) / 0.005), 8)
    kintree = np.stack([parents, np.arange(J)], 0).astype(np.int64)
    kintree[0, 0] = 2 ** 32 - 1                                                                    # as in the SMPL files
    return {
        'f': rng.integers(0, V, (max(1, 2 * V - 4), 3)).astype(np.uint32),
        'v_template': verts.astype(np.float64),
        'shapedirs': (rng.normal(size=(V, 3, NB)) * 0.004).astype(np.float64),
        'J_regressor': jr.astype(np.float64),
        'posedirs': np.zeros((V, 3, (J - 1) * 9), np.float64),
        'kintree_table': kintree,
        'weights': w.astype(np.float64),
    }


def edge_pose(J, kind, rng):
    """[J*3] float32.  random: N(0, 0.35); zero: every joint at rest (Rodrigues at |0 + 1e-8|, its adjoint divides by that angle and its square);
    tiny: N(0, 1e-6); pi: a random pose with joint 0 = (pi, 0, 0) (1 - cos = 2, sin ~ 0), the last joint = (0, 2 pi + 0.3, 0) (an angle past one
    turn) and joint 1 = (0, 0, 1) (the da pose's own joint 1); mixed: a random pose with every second joint exactly zero."""
    p = (rng.normal(size=(J, 3)) * 0.35).astype(np.float32)
    if kind == "zero":
        p[:] = 0
    elif kind == "tiny":
        p = (rng.normal(size=(J, 3)) * 1e-6).astype(np.float32)
    elif kind == "pi":
        p[0] = (np.pi, 0, 0)
        p[J - 1] = (0, 2 * np.pi + 0.3, 0)
        p[1] = (0, 0, 1)
    elif kind == "mixed":
        p[::2] = 0
    elif kind != "random":
        raise ValueError(kind)
    return p.reshape(-1)


def alignment(rng):
    """[4,4] float32, the matrix whose TRANSPOSE is applied (models/human_nerf.py:110): a scaled rotation in the upper 3x3, a translation ROW"""
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    ang = rng.uniform(0.2, 1.2)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K) * rng.uniform(0.8, 1.3)
    M[:3, 3] = rng.normal(size=3) * 0.5
    return np.ascontiguousarray(M.T).astype(np.float32)


@functools.lru_cache(maxsize=None)
def model(V, J, NB):
    return small_body_model(V, J, NB, seed=1000 * V + 10 * J + NB)


@functools.lru_cache(maxsize=None)
def inputs(V, J, NB, kind):
    """-> dict of float32 arrays: pose [1,J*3], beta [1,NB], align [4,4], upstream gradients gw [1,V,3] and gT [1,V,4,4]"""
    rng = np.random.default_rng(7 + 1000 * V + 10 * J + NB + 100000 * POSE_KINDS.index(kind))
    return dict(pose=edge_pose(J, kind, rng)[None], beta=(rng.normal(size=(1, NB)) * 0.8).astype(np.float32), align=alignment(rng),
                gw=rng.normal(size=(1, V, 3)).astype(np.float32), gT=rng.normal(size=(1, V, 4, 4)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def body(V, J, NB, double):
    from neuman_hip import smpl
    b = smpl.SMPLDiff(model(V, J, NB), 'cpu')
    return b.double() if double else b


@functools.lru_cache(maxsize=None)
def reference(V, J, NB, kind, through="both", double=True):
    """SMPLDiff.vertex_forward_torch on the host in float64 (or float32) -> dict of float64 arrays world, T, g_pose, g_beta, g_align for the loss
    (world * gw).sum() [through world / both] + (T * gT).sum() [through T / both].  Computed once per case and shared: treat as read-only."""
    x = inputs(V, J, NB, kind)
    dt = torch.float64 if double else torch.float32
    leaf = lambda a: torch.tensor(a, dtype=dt, requires_grad=True)                 # noqa: E731
    p, be, al = leaf(x['pose']), leaf(x['beta']), leaf(x['align'])
    world, T = body(V, J, NB, double).vertex_forward_torch(p, be, al, SCALE)
    loss = 0
    if through != "T":
        loss = loss + (world * torch.tensor(x['gw'], dtype=dt)).sum()
    if through != "world":
        loss = loss + (T * torch.tensor(x['gT'], dtype=dt)).sum()
    loss.backward()
    out = {k: v.detach().double().numpy() for k, v in (("world", world), ("T", T), ("g_pose", p.grad), ("g_beta", be.grad), ("g_align", al.grad))}
    for v in out.values():
        v.setflags(write=False)
    return out


def rel_err(got, want, scale=None):
    """largest |got - want| as a fraction of the largest |want| (the measure of tests/test_hip_smpl_diff.py), or of `scale` where given"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / ((np.abs(want).max() if scale is None else scale) + 1e-30))


def grad_scale(V, J, NB, kind, through, name):
    """The entry that a gradient's error is a fraction of: its own largest (None), with ONE exception, the model of a single vertex.  It regresses
    every joint to that vertex, and a rotation about a point does not move the point: the vertex does not depend on the pose at all, so the pose
    gradient that arrives through `world` alone is exactly zero (1e-16 in float64, the leftovers of cancelling terms in any float32 evaluation), and
    at rest the transform does not depend on where the joints are, so the shape gradient through `T` alone vanishes likewise.  A gradient that is
    zero has no largest entry to be a fraction of: the float32 host evaluation misses the measure there as well (tests/test_body_edges_host.py is
    what found it).  For V = 1 the two partial gradients are therefore held to the tolerance as a fraction of the gradient they add up to, the one
    through both outputs (or of their own largest entry where that is larger); through both outputs V = 1 is measured like every other case."""
    if V == 1 and through != "both" and name.startswith("g_"):
        return float(max(np.abs(reference(V, J, NB, kind, through)[name]).max(), np.abs(reference(V, J, NB, kind, "both")[name]).max()))
    return None


def tol(name):
    return TOL_OUT if name in ("world", "T", "static") else TOL_GRAD


def with_joint_rows(m):
    """The model with its J joints appended as vertices V .. V+J-1: vertex V+j has the one-hot weight of joint j and sits at the regressed joint
    (template and shape directions pushed through the regressor, which gets zero columns for the new vertices and so regresses the same joints).
    Its vertex rows V.. are what `SMPL.frames` returns as joint rows (concat_joints=True, models/smpl.py:347-349): T = A_j, point = J_j."""
    jr = np.asarray(m['J_regressor'], np.float64)
    J, V = jr.shape
    out = dict(m)
    out['v_template'] = np.concatenate([m['v_template'], jr @ m['v_template']], 0)
    out['shapedirs'] = np.concatenate([m['shapedirs'], np.einsum('jv,vkl->jkl', jr, m['shapedirs'])], 0)
    out['J_regressor'] = np.concatenate([jr, np.zeros((J, J))], 1)
    out['weights'] = np.concatenate([m['weights'], np.eye(J)], 0)
    out['posedirs'] = np.zeros((V + J, 3, (J - 1) * 9), np.float64)
    return out


@functools.lru_cache(maxsize=None)
def frames_reference(V, J, NB, kind):
    """the float64 chain on all V + J rows of `SMPL.frames`: -> world [V+J,3], T [V+J,4,4], static [V+J,3] (the body in the da pose), read-only"""
    x = inputs(V, J, NB, kind)
    b = _body_joint_rows(V, J, NB)
    t = lambda a: torch.tensor(a, dtype=torch.float64)                             # noqa: E731
    with torch.no_grad():
        world, T = b.vertex_forward_torch(t(x['pose']), t(x['beta']), t(x['align']), SCALE)
        T_da, v_shaped = b.transformations(b.da_smpl, t(x['beta']))
        static = torch.einsum('vab,vb->va', T_da, torch.cat([v_shaped, torch.ones_like(v_shaped[:, :1])], 1))[:, :3]
    out = dict(world=world[0].numpy(), T=T[0].numpy(), static=static.numpy())
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _body_joint_rows(V, J, NB):
    from neuman_hip import smpl
    return smpl.SMPLDiff(with_joint_rows(model(V, J, NB)), 'cpu').double()
