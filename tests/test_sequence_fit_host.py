"""Without a device: the batched entries of the sequence fit (nm_raster_silhouette_batch / _backward_batch, nm_smpl_vertex_forward_batch /
_backward_batch, nm_smpl_vertex_batch_workspace_floats) in the header, in `_lib.SIGNATURES` and in the library, and their argument checks;
`optimize_smpl.SequenceObjective` in float64 on the CPU (the torch restatement of the sequence objective, with the float64 silhouette of
tests/helpers/silhouette_ref.py behind the `silhouette=` hook) against `Objective` frame by frame; `optimize_scene`'s dict; mixed image sizes."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import silhouette_ref as SR  # noqa: E402

from neuman_hip import _lib  # noqa: E402

NEW = ("nm_raster_silhouette_batch", "nm_raster_silhouette_backward_batch", "nm_smpl_vertex_forward_batch", "nm_smpl_vertex_backward_batch",
       "nm_smpl_vertex_batch_workspace_floats")


def test_the_five_entries_are_declared_bound_and_exported_with_matching_arity():
    src = open(os.path.join(HERE, "..", "include", "neuman_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in neuman_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_the_batched_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.lib()
    dummy = (ctypes.c_char * 256)()                                     # stands in for every pointer: the checks run before any is read
    d = ctypes.cast(dummy, ctypes.c_void_p)
    nan, inf = float('nan'), float('inf')
    good = dict(h=d, verts=d, w2c=d, intr=d, B=2, W=8, H=8, sigma=1e-4, blur=1e-3, a=d, b=d, c=d)
    bad = [dict(h=None), dict(verts=None), dict(w2c=None), dict(intr=None), dict(a=None), dict(b=None), dict(B=0), dict(B=-3), dict(B=1 << 16), dict(W=0),
           dict(H=0), dict(W=1 << 16, H=1 << 16), dict(sigma=0.0), dict(sigma=-1e-4), dict(sigma=nan), dict(sigma=inf), dict(sigma=1e-60), dict(blur=-1e-9),
           dict(blur=nan), dict(blur=inf)]
    for over in bad:
        k = dict(good, **over)
        args = (k['h'], k['verts'], k['w2c'], k['intr'], k['B'], k['W'], k['H'], k['sigma'], k['blur'], k['a'], k['b'])
        assert lib.nm_raster_silhouette_batch(*args, None, None) == -1 and b"nm_raster_silhouette_batch:" in lib.nm_last_error(), over
        assert lib.nm_raster_silhouette_backward_batch(*args, k['c'], None) == -1 and b"nm_raster_silhouette_backward_batch:" in lib.nm_last_error(), over
    k = good
    args = (k['h'], k['verts'], k['w2c'], k['intr'], k['B'], k['W'], k['H'], k['sigma'], k['blur'], k['a'], k['b'])
    assert lib.nm_raster_silhouette_backward_batch(*args, None, None) == -1 and b"nm_raster_silhouette_backward_batch:" in lib.nm_last_error()
    # the skinning batch: a null pointer, B < 1, no upstream gradient
    assert lib.nm_smpl_vertex_batch_workspace_floats(None, 3) == 0 and lib.nm_smpl_vertex_batch_workspace_floats(d, 0) == 0
    assert lib.nm_smpl_vertex_forward_batch(d, d, d, d, 1.0, None, 0, d, d, d, None, None) == -1 and b"nm_smpl_vertex_forward_batch:" in lib.nm_last_error()
    assert lib.nm_smpl_vertex_forward_batch(d, d, d, d, 1.0, None, 2, d, d, None, None, None) == -1 and b"nm_smpl_vertex_forward_batch:" in lib.nm_last_error()
    assert lib.nm_smpl_vertex_forward_batch(None, d, d, d, 1.0, None, 2, d, d, d, None, None) == -1
    assert lib.nm_smpl_vertex_backward_batch(d, d, d, d, 1.0, None, 0, d, d, None, d, d, d, d, None) == -1 and b"nm_smpl_vertex_backward_batch:" in lib.nm_last_error()
    assert lib.nm_smpl_vertex_backward_batch(d, d, d, d, 1.0, None, 2, None, None, None, d, d, d, d, None) == -1 and b"no upstream gradient" in lib.nm_last_error()
    assert lib.nm_smpl_vertex_backward_batch(d, d, d, d, 1.0, None, 2, d, d, None, d, None, d, d, None) == -1


# ---- the objective ---------------------------------------------------------------------------------------------------------------------
W, H = 20, 14


def _scene(sizes=((W, H),) * 3):
    """three frames of the synthetic body on the CPU in float64: their own poses, shapes, alignments, cameras, masks and keypoints; the middle
    frame has no confident joint"""
    from neuman_hip import smpl, synthetic
    model = synthetic.smpl_like_model(0)
    body = smpl.SMPLDiff(model, 'cpu').double()
    faces = model['f'].astype(np.int32)
    poses, betas, aligns = synthetic.smpl_like_frames(3)
    rng = np.random.default_rng(4)
    caps, smpls = [], []
    for i, (w, h) in enumerate(sizes):
        cap = synthetic.SimpleCapture(w, h, c2w=synthetic.spherical_c2w(20. + 25. * i, -10. - 5. * i, 4.0 + 0.5 * i))
        cap.image_path = f"/somewhere/images/{i:05d}.png"
        cap.binary_mask = (rng.random((h, w)) < 0.3).astype(np.float32)
        kp = np.concatenate([rng.random((17, 2)) * [w - 2, h - 2] + 0.5, rng.random((17, 1)) * 0.7 + 0.3], 1)
        kp[::4, 2] = 0.1                                                # some below the confidence cut
        if i == 1:
            kp[:, 2] = 0.0
        cap.keypoints = kp
        cap.densepose = np.arange(25).reshape(5, 5) if i != 2 else np.array([[0, 7, 9, 15, 17]])
        caps.append(cap)
        smpls.append(dict(pose=(poses[i] * 0.2).astype(np.float32), betas=betas[i]))
    return caps, smpls, faces, body, aligns


def _hooks(caps, faces):
    cams = [SR.camera_of(c) for c in caps]
    one = [lambda v, cam=cam: SR.silhouette(v, faces, cam, 1e-2, dtype=torch.float64)['alpha'] for cam in cams]
    return one, (lambda v: torch.stack([one[b](v[b]) for b in range(len(caps))]))


def test_the_sequence_objective_is_the_sum_of_the_frames_objectives_and_every_gradient_row_is_its_frames_own():
    from neuman_hip import optimize_smpl as O
    caps, smpls, faces, body, aligns = _scene()
    one, batch = _hooks(caps, faces)
    start = torch.as_tensor(np.stack([s['pose'] for s in smpls])).double()
    seq = O.SequenceObjective(caps, smpls, faces, body, aligns, 1.3, silhouette=batch)
    poses = start.clone().requires_grad_(True)
    jt, st = seq.terms(poses)
    total = seq.loss(poses)
    total.backward()
    assert jt.shape == (3,) and st.shape == (3,) and poses.grad.shape == (3, 72)
    assert float(jt[1]) == 0.0 and torch.isfinite(poses.grad).all()                              # no confident joint: 0, not NaN
    want = 0.0
    for b in range(3):
        name = os.path.basename(caps[b].image_path)
        obj = O.Objective(caps[b], smpls[b], faces, body, aligns[name], 1.3, silhouette=one[b])
        p = start[b].clone().requires_grad_(True)
        j1, s1 = obj.terms(p)
        (j1 + s1).backward()
        want = want + float(j1 + s1)
        assert abs(float(jt[b]) - float(j1)) <= 1e-12 * max(1.0, abs(float(j1))) and abs(float(st[b]) - float(s1)) <= 1e-12
        assert float(p.grad.abs().max()) > 0
        assert float((poses.grad[b] - p.grad).abs().max()) <= 1e-11 * float(p.grad.abs().max()), b
    assert float(jt[0]) > 0 and float(jt[2]) > 0 and abs(float(total) - want) <= 1e-12 * abs(want)
    # a list of alignments in capture order is the dict's equal
    as_list = [aligns[os.path.basename(c.image_path)] for c in caps]
    again = O.SequenceObjective(caps, smpls, faces, body, as_list, 1.3, silhouette=batch)
    assert float(again.loss(start)) == float(total)


def test_mixed_image_sizes_are_refused():
    from neuman_hip import optimize_smpl as O
    from neuman_hip import raster
    caps, smpls, faces, body, aligns = _scene(sizes=((W, H), (W, H), (W + 4, H)))
    with pytest.raises(ValueError, match="one image size"):
        O.SequenceObjective(caps, smpls, faces, body, aligns, 1.0, silhouette=lambda v: v)
    with pytest.raises(ValueError, match="one image size"):
        O.optimize_smpl_sequence(caps, smpls, faces, body, aligns, 1.0, num_iters=1)
    with pytest.raises(ValueError, match="one image size"):
        O.optimize_scene(caps, smpls, faces, body, aligns, 1.0, num_iters=1)
    with pytest.raises(ValueError, match="one image size"):
        raster.batch_cameras(caps, 'cpu')
    w2c, intr, w, h = raster.batch_cameras(caps[:2], 'cpu')
    assert w2c.shape == (2, 4, 4) and w2c.dtype == torch.float64 and intr.shape == (2, 4) and (w, h) == (W, H)
    assert np.array_equal(w2c[1, :3].numpy(), raster.camera_of(caps[1])[0]) and np.array_equal(w2c[1, 3].numpy(), [0, 0, 0, 1])
    assert intr[1].tolist() == list(raster.camera_of(caps[1])[1:5])


def test_optimize_scenes_dict_layout_and_key_order(monkeypatch):
    """the dict main() dumps (:277-295): {1: {'pose': [...], 'betas': [...]}}, one entry per capture in capture order, the betas the very
    objects that came in; the fit itself is stood in for (it needs the device)"""
    from neuman_hip import optimize_smpl as O
    caps = [types.SimpleNamespace(image_path=f"/x/{i:05d}.png") for i in range(4)]
    smpls = [dict(pose=np.full(72, i, np.float32), betas=np.full(10, 10 + i, np.float32)) for i in range(4)]
    seen = {}

    def fit(caps_, smpls_, faces, body_model, alignments, scale, **kw):
        seen.update(kw, n=len(caps_), alignments=alignments, scale=scale)
        return np.stack([s['pose'] + 0.5 for s in smpls_])

    monkeypatch.setattr(O, "optimize_smpl_sequence", fit)
    aligns = {f"{i:05d}.png": np.eye(4)[:, :3] for i in range(4)}
    out = O.optimize_scene(caps, smpls, None, None, aligns, 2.0, num_iters=7, frames_per_batch=3)
    assert list(out) == [1] and list(out[1]) == ['pose', 'betas']
    assert isinstance(out[1]['pose'], list) and isinstance(out[1]['betas'], list) and len(out[1]['pose']) == len(out[1]['betas']) == 4
    for i in range(4):
        assert out[1]['pose'][i].shape == (72,) and out[1]['pose'][i].dtype == np.float32 and np.all(out[1]['pose'][i] == i + 0.5)
        assert out[1]['betas'][i] is smpls[i]['betas']
    assert seen.pop('alignments') is aligns and seen == dict(num_iters=7, frames_per_batch=3, n=4, scale=2.0)
