"""-m gpu: every entry of csrc/smpl.hip away from SMPL's one shape (V = 6890, J = 24, NB = 10): the body models and poses of
tests/helpers/body_edges.py -- V from one vertex to four ragged workgroups, J and NB up to the ABI's limits 64 and 32, sparse weights and regressor,
poses at rest, at 1e-6, at pi and past one turn -- against the skinning chain in float64 on the host (SMPLDiff.vertex_forward_torch, pinned to the
reference by tests/golden/smpl_grad.npz) at the project's tolerances for V = 6890: 2e-5 of the largest entry for outputs (tests/test_hip_smpl.py),
2e-4 for the gradients (tests/test_hip_smpl_diff.py).  tests/test_body_edges_host.py holds the float32 host evaluations of the same inputs to a
quarter of these.  Every measured error is printed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import body_edges as BE  # noqa: E402
from oracle import smpl as OS  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["V{}-J{}-NB{}".format(*s) for s in BE.SHAPE_CASES]


def leaf(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device='cuda', requires_grad=True)


def cu(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device='cuda')


_BODIES = {}


def diff_body(V, J, NB):
    from neuman_hip import smpl
    if (V, J, NB) not in _BODIES:
        _BODIES[(V, J, NB)] = smpl.SMPLDiff(BE.model(V, J, NB), 'cuda')
    return _BODIES[(V, J, NB)]


def hip_vertex(V, J, NB, kind, through, da_pose=None):
    """SMPLDiff.vertex_forward on the device and its gradients -> dict like BE.reference"""
    x = BE.inputs(V, J, NB, kind)
    p, be, al = leaf(x['pose']), leaf(x['beta']), leaf(x['align'])
    world, T = diff_body(V, J, NB).vertex_forward(p, be, al, BE.SCALE, da_pose)
    assert world.shape == (1, V, 3) and T.shape == (1, V, 4, 4) and world.is_cuda and T.dtype == torch.float32
    loss = 0
    if through != "T":
        loss = loss + (world * cu(x['gw'])).sum()
    if through != "world":
        loss = loss + (T * cu(x['gT'])).sum()
    loss.backward()
    return {k: v.detach().clone() for k, v in (("world", world), ("T", T), ("g_pose", p.grad), ("g_beta", be.grad), ("g_align", al.grad))}


def check(tag, got, want, names, scales={}):
    """print every error, then assert them all"""
    errs = {n: BE.rel_err(got[n].cpu().numpy() if isinstance(got[n], torch.Tensor) else got[n], want[n], scales.get(n)) for n in names}
    print(f"[smpl-edges] {tag}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        g = got[n]
        assert bool(torch.isfinite(g).all()) if isinstance(g, torch.Tensor) else np.isfinite(g).all(), (tag, n, "not finite")
        assert e <= BE.tol(n), (tag, n, e, BE.tol(n))


# ---- SMPLDiff.vertex_forward: nm_smpl_vertex_forward / _backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("through", BE.THROUGH)
@pytest.mark.parametrize("shape", BE.SHAPE_CASES, ids=SHAPE_IDS)
def test_vertex_forward_and_gradients_against_float64(shape, through):
    """outputs and the gradients to pose, shape and alignment for every pose kind; gradients arriving through the vertices only (g_T null in the
    kernel), through the transforms only (g_world null) and through both"""
    V, J, NB = shape
    for kind in BE.POSE_KINDS:
        got = hip_vertex(V, J, NB, kind, through)
        names = ("world", "T", "g_pose", "g_beta", "g_align")
        check(f"V={V} J={J} NB={NB} {kind}, gradient through {through}", got, BE.reference(V, J, NB, kind, through), names,
              {n: BE.grad_scale(V, J, NB, kind, through, n) for n in names})


def test_caller_supplied_da_pose():
    """the canonical pose handed in by the caller (HumanNeRF keeps it as a parameter) instead of the handle's: another pose than the built-in one"""
    from neuman_hip import smpl
    V, J, NB, kind = 257, 64, 32, "random"
    da = smpl.da_pose(J).reshape(J, 3).copy()
    da[1], da[2], da[J - 1] = (0.1, 0, 0.8), (0, -0.2, -0.9), (0.3, 0.3, 0)
    x = BE.inputs(V, J, NB, kind)
    got = hip_vertex(V, J, NB, kind, "both", cu(da.reshape(1, -1)))
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)         # noqa: E731
    p, be, al = t(x['pose']), t(x['beta']), t(x['align'])
    world, T = BE.body(V, J, NB, True).vertex_forward_torch(p, be, al, BE.SCALE, torch.tensor(da.reshape(1, -1), dtype=torch.float64))
    ((world * torch.tensor(x['gw']).double()).sum() + (T * torch.tensor(x['gT']).double()).sum()).backward()
    want = {k: v.detach().numpy() for k, v in (("world", world), ("T", T), ("g_pose", p.grad), ("g_beta", be.grad), ("g_align", al.grad))}
    check("caller's da pose, V=257 J=64 NB=32", got, want, tuple(want))
    builtin = BE.reference(V, J, NB, kind, "both")
    assert BE.rel_err(want["T"], builtin["T"]) > 1e-2                               # (the supplied pose is not the built-in one in disguise)


def test_vertex_forward_is_bit_identical_with_another_model_in_between():
    """nothing of a call survives in the handle or the workspace: the same call twice, another model's forward and backward in between"""
    a, b = (1025, 24, 10), (257, 64, 32)
    first = hip_vertex(*a, "random", "both")
    hip_vertex(*b, "pi", "both")
    second = hip_vertex(*a, "random", "both")
    for k in first:
        assert torch.equal(first[k], second[k]), k


# ---- SMPL.frames: nm_smpl_frames ---------------------------------------------------------------------------------------------------------------------
def frame_args(V, J, NB, kinds):
    xs = [BE.inputs(V, J, NB, k) for k in kinds]
    return (np.stack([x['pose'][0] for x in xs]).reshape(len(xs), J * 3), np.stack([x['beta'][0] for x in xs]).reshape(len(xs), NB),
            np.stack([x['align'] for x in xs]).astype(np.float64).reshape(len(xs), 4, 4))


@pytest.mark.parametrize("shape", BE.SHAPE_CASES, ids=SHAPE_IDS)
def test_frames_against_the_oracle_and_float64(shape):
    """all five poses as one batch.  precise=True: the render scripts' chain against oracle.smpl.read_smpl_frame and against the float64 chain on ALL
    V + J rows (the joint rows through a model with the joints appended as vertices); precise=False: against oracle.smpl.vertex_forward, and against
    SMPLDiff.vertex_forward on the same input, which regresses the joints and walks the chains in other kernels (smpl_jreg_kernel + smpl_chain_kernel
    against smpl_joints_kernel)"""
    from neuman_hip import smpl
    V, J, NB = shape
    m = BE.model(V, J, NB)
    body, om = smpl.SMPL(m), OS.Model(m)
    po, be, al = frame_args(V, J, NB, BE.POSE_KINDS)
    T, world, static = body.frames(po, be, al, BE.SCALE, True)
    assert T.shape == (5, V + J, 4, 4) and T.dtype == torch.float64 and world.shape == (5, V + J, 3) and static.shape == (5, V + J, 3)
    Tl, wl, _ = body.frames(po, be, al, BE.SCALE, False)
    for i, kind in enumerate(BE.POSE_KINDS):
        tag = f"V={V} J={J} NB={NB} {kind}"
        got = dict(T=T[i], world=world[i], static=static[i])
        wv, wj, sv, sj, Ts = OS.read_smpl_frame(om, po[i], be[i], al[i][:, :3], BE.SCALE)
        check(tag + ", frames(precise) vs oracle", got, dict(T=Ts, world=np.concatenate([wv, wj]), static=np.concatenate([sv, sj])), ("T", "world", "static"))
        check(tag + ", frames(precise) vs float64", got, BE.frames_reference(V, J, NB, kind), ("T", "world", "static"))
        ow, oT = OS.vertex_forward(om, po[i], be[i], al[i].astype(np.float32), BE.SCALE)
        loose = dict(T=Tl[i, :V], world=wl[i, :V])
        check(tag + ", frames(float32) vs oracle", loose, dict(T=oT, world=ow), ("T", "world"))
        dv = hip_vertex(V, J, NB, kind, "world")
        check(tag + ", frames(float32) vs SMPLDiff.vertex_forward", loose, dict(T=dv["T"][0].cpu().numpy(), world=dv["world"][0].cpu().numpy()), ("T", "world"))


@pytest.mark.parametrize("precise", [True, False])
def test_frames_batch_edges_on_one_handle(precise):
    """B = 1, 4, 2, 0 in this order on one handle: the workspace grows once (at 4) and is reused by the smaller batches; every frame of a batch is
    bit-identical to the same frame computed alone; an empty batch returns empty tensors"""
    from neuman_hip import smpl
    V, J, NB = 257, 64, 32
    kinds = ["random", "pi", "zero", "mixed"]
    body, solo = smpl.SMPL(BE.model(V, J, NB)), smpl.SMPL(BE.model(V, J, NB))
    po, be, al = frame_args(V, J, NB, kinds)
    alone = [[t.clone() for t in solo.frames(po[i:i + 1], be[i:i + 1], al[i:i + 1], BE.SCALE, precise)] for i in range(4)]
    for sel in ([0], [0, 1, 2, 3], [3, 1], []):
        out = body.frames(po[sel].reshape(len(sel), J * 3), be[sel].reshape(len(sel), NB), al[sel].reshape(len(sel), 4, 4), BE.SCALE, precise)
        assert out[0].shape == (len(sel), V + J, 4, 4) and out[1].shape == (len(sel), V + J, 3) and out[2].shape == (len(sel), V + J, 3)
        for k, i in enumerate(sel):
            for got, want, what in zip(out, alone[i], ("T", "world", "static")):
                assert torch.equal(got[k], want[0]), (sel, i, what)
    torch.cuda.synchronize()


# ---- limits ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,NB,ok", [(64, 32, True), (65, 10, False), (24, 33, False), (24, 0, False)], ids=["J64-NB32", "J65", "NB33", "NB0"])
def test_create_limits(J, NB, ok):
    """J <= 64 and 1 <= NB <= 32: nm_smpl_create takes the limits and refuses one past them, and a model without shape directions (whose empty betas
    array every entry would then refuse as a null pointer), naming the sizes"""
    from neuman_hip import _lib
    V = 8
    rng = np.random.default_rng(0)
    f = lambda *s: np.ascontiguousarray(rng.random(s), np.float32)                  # noqa: E731
    vt, sd, jr, w, da = f(V, 3), f(V, 3, max(NB, 1)), f(J, V), f(V, J), np.zeros(J * 3, np.float32)
    par = np.ascontiguousarray(np.maximum(np.arange(J) - 1, 0), np.int32)
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                 # noqa: E731
    rc = _lib.lib().nm_smpl_create(p(vt), p(sd), p(jr), p(par), p(w), p(da), V, J, NB, ctypes.byref(h))
    if ok:
        assert rc == 0 and h.value
        _lib.lib().nm_smpl_destroy(h)
        return
    msg = _lib.lib().nm_last_error().decode()
    assert rc != 0 and not h.value
    assert "nm_smpl_create: bad sizes" in msg and f"J={J}" in msg and f"NB={NB}" in msg and "J <= 64" in msg and "1 <= NB <= 32" in msg, msg
    if NB == 0:
        from neuman_hip import smpl
        m = dict(BE.model(64, 24, 10))
        m['shapedirs'] = np.zeros((64, 3, 0))
        with pytest.raises(_lib.NeumanHipError, match="NB=0"):
            smpl.SMPL(m)
