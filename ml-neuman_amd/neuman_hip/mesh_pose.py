"""An extracted mesh animated by the body (csrc/mesh_pose.hip; include/neuman_hip.h 'mesh pose', rules P1-P6).

mesh_extract gives the learned human as a mesh frozen in the canonical "da" pose.  This binds its vertices to the canonical body once and
poses them for every frame of a sequence: the observation -> canonical warp of the renderers (ray_utils.warp_samples_to_canonical; reference
utils/ray_utils.py:48-66) run forwards -- closest body triangle, barycentric blend of its three per-vertex transforms, applied as it is.

    verts, faces, normals = clean_mesh(*extract_mesh(field, box, level))                # canonical space
    binding = bind_mesh(verts, static_verts, body.faces)                                 # once: closest triangle + barycentrics
    posed, posed_normals = pose_mesh_frames(body, poses, betas, alignments, scale, verts, binding, normals)      # [B,N,3] each
    frames = render_utils.render_mesh_frames(posed, faces, caps, colours, posed_normals) # uint8 [B,H,W,3]; the faces do not change

The forward map takes the closest point on the CANONICAL body, the renderers' inverse map the closest point on the POSED body: the two agree
to first order near the surface (`Binding.sdist` says how far from it a vertex sits).  Every tensor is a CUDA tensor; there is no CPU path."""
import ctypes

import torch

from . import _lib
from .ray_utils import Mesh, signed_distance_dev

FRAMES_PER_CALL = 64                                               # pose_mesh_frames' default chunk: 57 MB of transforms for SMPL's V + J rows


class Binding:
    """What `bind_mesh` returns, every tensor on the mesh's device: tri [N,3] int32 (rows of a frame's transform table: the closest body
    triangle's vertex ids), bary [N,3] float32 (nm_bary_forward's, not renormalised or clamped), face [N] int32 (the closest body face),
    sdist [N] float32 (signed distance to the body, negative inside: vertices far from it animate least reliably).  tri and bary may also
    be [B,N,3]: a binding of its own per frame (`pose_mesh` then takes frame b's rows for frame b)."""
    __slots__ = ('tri', 'bary', 'face', 'sdist')

    def __init__(self, tri, bary, face=None, sdist=None):
        self.tri, self.bary, self.face, self.sdist = tri, bary, face, sdist


def _cuda_rows(a, who, name, dtype=torch.float32):
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise _lib.NeumanHipError(f"{who}: {name} must be a CUDA (HIP) tensor: there is no CPU path")
    if a.dim() != 2 or a.shape[1] != 3 or a.dtype != dtype:
        raise _lib.NeumanHipError(f"{who}: {name} must be {dtype} [N, 3], got {a.dtype} {tuple(a.shape)}")
    return a.detach().contiguous()


def bind_mesh(verts, body_verts, body_faces, mesh=None):
    """Bind canonical mesh vertices verts [N,3] (CUDA float32) to the canonical body (body_verts [V,3], body_faces [F,3]: SMPL.frames'
    static rows or the trainer's static vertices, tensors or numpy) -> Binding.  The closest face and point come from
    ray_utils.signed_distance_dev on ray_utils.Mesh(body_verts, body_faces, None, device) -- or on the caller's `mesh`, whose own vertices
    and faces are then the body -- tri = faces[face], bary = nm_bary_forward of the closest point in that triangle."""
    verts = _cuda_rows(verts, "bind_mesh", "verts")
    dev = verts.device
    with torch.cuda.device(dev):
        if mesh is None:
            mesh = Mesh(body_verts, body_faces, None, dev)
        elif mesh.verts.device != dev:
            raise _lib.NeumanHipError(f"bind_mesh: the mesh lives on {mesh.verts.device}, verts on {dev}")
        N = int(verts.shape[0])
        if N == 0:
            return Binding(torch.empty((0, 3), device=dev, dtype=torch.int32), torch.empty((0, 3), device=dev, dtype=torch.float32),
                           torch.empty((0,), device=dev, dtype=torch.int32), torch.empty((0,), device=dev, dtype=torch.float32))
        sdist, face, closest = signed_distance_dev(verts, mesh)
        tri = mesh.faces[face.long()].contiguous()
        bary = torch.empty((N, 3), device=dev, dtype=torch.float32)
        _lib.check(_lib.lib().nm_bary_forward(_lib.dev_ptr(mesh.verts), _lib.dev_ptr(tri, torch.int32), _lib.dev_ptr(closest), N, _lib.dev_ptr(bary),
                                              _lib.stream_ptr()), "nm_bary_forward")
    return Binding(tri, bary, face, sdist)


def _check_pose_inputs(who, verts, binding, T, normals):
    """-> (verts, normals, T [B,rows,4,4], tri, bary, per_frame) checked against each other; nothing is converted"""
    verts = _cuda_rows(verts, who, "verts")
    dev, N = verts.device, int(verts.shape[0])
    if normals is not None:
        normals = _cuda_rows(normals, who, "normals")
        if normals.shape[0] != N or normals.device != dev:
            raise _lib.NeumanHipError(f"{who}: {normals.shape[0]} normals on {normals.device} for {N} vertices on {dev}")
    if not isinstance(T, torch.Tensor) or not T.is_cuda:
        raise _lib.NeumanHipError(f"{who}: T must be a CUDA (HIP) tensor: there is no CPU path")
    if T.dim() == 3:
        T = T[None]
    if T.dim() != 4 or tuple(T.shape[2:]) != (4, 4) or T.shape[0] < 1 or T.shape[1] < 1 or T.dtype not in (torch.float64, torch.float32):
        raise _lib.NeumanHipError(f"{who}: T must be float64 or float32 [B, rows, 4, 4] or [rows, 4, 4], got {T.dtype} {tuple(T.shape)}")
    if not T.is_contiguous() or T.device != dev:
        raise _lib.NeumanHipError(f"{who}: T must be contiguous and on {dev} (it is passed as it is, not converted)")
    tri, bary = binding.tri, binding.bary
    for a, name, dtype in ((tri, "binding.tri", torch.int32), (bary, "binding.bary", torch.float32)):
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise _lib.NeumanHipError(f"{who}: {name} must be a CUDA (HIP) tensor: there is no CPU path")
        if a.dtype != dtype or a.device != dev or not a.is_contiguous():
            raise _lib.NeumanHipError(f"{who}: {name} must be contiguous {dtype} on {dev}, got {a.dtype} on {a.device}")
    B = int(T.shape[0])
    per_frame = tri.dim() == 3
    want = (B, N, 3) if per_frame else (N, 3)
    if tuple(tri.shape) != want or tuple(bary.shape) != want:
        raise _lib.NeumanHipError(f"{who}: binding of {tuple(tri.shape)} / {tuple(bary.shape)} for {N} vertices and {B} frames "
                                  f"(expected [N, 3], or [B, N, 3] for a binding per frame)")
    return verts, normals, T, tri, bary, per_frame


def _launch(verts, normals, T, tri, bary, per_frame, out_pts, out_normals, counter):
    B, rows, N = int(T.shape[0]), int(T.shape[1]), int(verts.shape[0])
    _lib.check(_lib.lib().nm_mesh_pose_batch(ctypes.c_void_p(T.data_ptr()), 1 if T.dtype == torch.float64 else 0, rows, B, _lib.dev_ptr(tri, torch.int32),
                                             _lib.dev_ptr(bary), 1 if per_frame else 0, _lib.dev_ptr(verts), _lib.dev_ptr(normals), N, _lib.dev_ptr(out_pts),
                                             _lib.dev_ptr(out_normals), _lib.dev_ptr(counter, torch.int32), _lib.stream_ptr()), "nm_mesh_pose_batch")


def pose_mesh(verts, binding, T, normals=None, check=False):
    """The canonical mesh vertices verts [N,3] (and normals [N,3]) under the transforms T [B,rows,4,4] or [rows,4,4] (CUDA float64 or
    float32, canonical -> scene: SMPL.frames' T, or nm_smpl_vertex_forward_batch's T_out; passed as it is) blended by `binding` (rules
    P2-P4) -> posed [B,N,3] float32, or (posed, posed_normals) when normals is given.  A binding whose tensors are [B,N,3] is per frame.
    A vertex bound to a row outside [0, rows) comes out NaN (rule P5); check=True counts those on the device, reads the count back once
    and raises NeumanHipError naming it."""
    verts, normals, T, tri, bary, per_frame = _check_pose_inputs("pose_mesh", verts, binding, T, normals)
    dev, B, N = verts.device, int(T.shape[0]), int(verts.shape[0])
    with torch.cuda.device(dev):
        out_pts = torch.empty((B, N, 3), device=dev, dtype=torch.float32)
        out_normals = None if normals is None else torch.empty((B, N, 3), device=dev, dtype=torch.float32)
        counter = torch.zeros((1,), device=dev, dtype=torch.int32) if check else None
        _launch(verts, normals, T, tri, bary, per_frame, out_pts, out_normals, counter)
        if check:
            bad = int(counter.item())
            if bad:
                raise _lib.NeumanHipError(f"pose_mesh: {bad} (frame, vertex) pairs are bound to a row outside [0, {int(T.shape[1])}) of the transform table")
    return out_pts if normals is None else (out_pts, out_normals)


def pose_mesh_frames(body_model, poses, betas, alignments, scale, verts, binding, normals=None, frames_per_call=None):
    """`pose_mesh` under a sequence's own body transforms: poses [B,J*3], betas [B,NB], alignments [B,4,4] (the matrices whose transpose is
    applied) and scale as smpl.SMPL.frames takes them; `body_model` an smpl.SMPL.  The transforms come from its batched skinning in the
    precise arithmetic (nm_smpl_frames: float64, V + J rows) frames_per_call frames at a time (default 64), so that they never exist for
    the whole sequence at once; every chunk's output goes straight into the result -> posed [B,N,3], or (posed, posed_normals)."""
    n_frames = int(len(poses))
    if n_frames < 1 or len(betas) != n_frames or len(alignments) != n_frames:
        raise _lib.NeumanHipError(f"pose_mesh_frames: {n_frames} poses, {len(betas)} betas, {len(alignments)} alignments")
    step = FRAMES_PER_CALL if frames_per_call is None else int(frames_per_call)
    if step < 1:
        raise ValueError(f"frames_per_call must be >= 1, got {frames_per_call!r}")
    verts = _cuda_rows(verts, "pose_mesh_frames", "verts")
    dev, N = verts.device, int(verts.shape[0])
    per_frame = isinstance(binding.tri, torch.Tensor) and binding.tri.dim() == 3
    if per_frame and binding.tri.shape[0] != n_frames:
        raise _lib.NeumanHipError(f"pose_mesh_frames: a per-frame binding of {binding.tri.shape[0]} frames for {n_frames} frames")
    with torch.cuda.device(dev):
        out_pts = torch.empty((n_frames, N, 3), device=dev, dtype=torch.float32)
        out_normals = None if normals is None else torch.empty((n_frames, N, 3), device=dev, dtype=torch.float32)
        for b0 in range(0, n_frames, step):
            b1 = min(n_frames, b0 + step)
            T, _, _ = body_model.frames(poses[b0:b1], betas[b0:b1], alignments[b0:b1], scale, True)
            chunk = Binding(binding.tri[b0:b1], binding.bary[b0:b1]) if per_frame else binding
            v, n, T, tri, bary, _ = _check_pose_inputs("pose_mesh_frames", verts, chunk, T, normals)
            _launch(v, n, T, tri, bary, per_frame, out_pts[b0:b1], None if n is None else out_normals[b0:b1], None)
    return out_pts if normals is None else (out_pts, out_normals)
