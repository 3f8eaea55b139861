"""Smooth a triangle mesh without touching its faces, and derive normals from the faces themselves (csrc/mesh_smooth.hip;
include/neuman_hip.h 'mesh smooth', rules S1-S6).

What mesh_extract.extract_mesh takes from a learned density is rippled at the scale of a grid cell.  `smooth_mesh` runs Taubin's lambda|mu
pass over it: every vertex moves towards the average of its neighbours by lambda, then away from it by mu, which removes the ripple and does
not shrink the body.  Only vertices move: `faces` stays byte for byte, the mesh stays watertight, and components, binding, posing and the
rasteriser take the result as they take any mesh.  `vertex_normals` gives the area-weighted normals of the faces around every vertex -- the
normals of a smoothed mesh (the field gradient of extract_mesh no longer fits it) and of every posed frame of mesh_pose.pose_mesh_frames:

    verts, faces, normals = clean_mesh(*extract_mesh(field, box, level))
    adj = adjacency(faces, verts.shape[0])                                  # once per mesh; both calls below build it if it is not given
    verts = smooth_mesh(verts, faces, iterations=10, adj=adj)
    normals = vertex_normals(verts, faces, adj=adj)
    frame_normals = vertex_normals(pose_mesh_frames(binding, frames)[0], faces, adj=adj)      # [B,V,3] in one launch

Every tensor is a CUDA tensor; there is no CPU path."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .mesh_extract import _mesh_faces, _vertex_rows


class Adjacency:
    """What `adjacency` returns, every tensor on the mesh's device: inc_off [V+1] int32 and inc [n_incident] int32 -- inc[inc_off[v] :
    inc_off[v+1]] are the proper faces (three distinct vertices) that name v, in ascending face index; boundary [V] uint8 -- 1 where the vertex
    lies on an edge with exactly one face; n_verts, n_faces: the mesh it was built for."""
    __slots__ = ('inc_off', 'inc', 'boundary', 'n_verts', 'n_faces')

    def __init__(self, inc_off, inc, boundary, n_verts, n_faces):
        self.inc_off, self.inc, self.boundary, self.n_verts, self.n_faces = inc_off, inc, boundary, n_verts, n_faces


def adjacency(faces, n_verts):
    """The vertex -> incident faces lists of faces [F,3] (CUDA int32) over n_verts vertices and the boundary flags (rules S1, S2) ->
    Adjacency.  One read-back, for the lists' total length; a face that names a vertex outside [0, n_verts) raises NeumanHipError."""
    faces = _mesh_faces(faces, "adjacency")
    n_verts, n_faces = int(n_verts), int(faces.shape[0])
    dev = faces.device
    L = _lib.lib()
    I32, U8 = torch.int32, torch.uint8
    with torch.cuda.device(dev):
        nbytes = int(L.nm_mesh_adjacency_workspace_bytes(n_verts, n_faces))
        if nbytes < 0:
            _lib.check(nbytes, "nm_mesh_adjacency_workspace_bytes")
        ws = torch.empty((nbytes,), device=dev, dtype=U8)
        inc_off = torch.empty((n_verts + 1,), device=dev, dtype=I32)
        inc = torch.empty((3 * n_faces,), device=dev, dtype=I32)
        boundary = torch.empty((n_verts,), device=dev, dtype=U8)
        n = ctypes.c_int64(0)
        _lib.check(L.nm_mesh_adjacency(_lib.dev_ptr(faces, I32), n_faces, n_verts, _lib.dev_ptr(inc_off, I32), _lib.dev_ptr(inc, I32),
                                       _lib.dev_ptr(boundary, U8), _lib.dev_ptr(ws, U8), nbytes, ctypes.byref(n), _lib.stream_ptr()),
                   "nm_mesh_adjacency")
    return Adjacency(inc_off, inc[:int(n.value)], boundary, n_verts, n_faces)


def _adjacency_of(adj, faces, n_verts, who):
    if adj is None:
        return adjacency(faces, n_verts)
    if not isinstance(adj, Adjacency) or adj.n_verts != n_verts or adj.n_faces != int(faces.shape[0]) or adj.inc_off.device != faces.device:
        raise _lib.NeumanHipError(f"{who}: adj was not built by adjacency() for this mesh ({n_verts} vertices, {int(faces.shape[0])} faces on {faces.device})")
    return adj


def _inc_ptr(adj):
    """the lists' pointer; a mesh without a proper face has an empty `inc`, whose pointer is null: one unread entry stands in"""
    inc = adj.inc if adj.inc.numel() else torch.zeros((1,), device=adj.inc_off.device, dtype=torch.int32)
    return _lib.dev_ptr(inc.contiguous(), torch.int32)


def smooth_mesh(rows, faces, iterations=10, lam=0.5, mu=-0.53, fixed=None, pin_boundary=True, adj=None):
    """`iterations` Taubin iterations on rows [V,w] (CUDA float32, 1 <= w <= 64: positions, or any per-vertex attribute) over the mesh
    faces [F,3] -> rows' [V,w] (rules S3, S4): a step with lam, then a step with mu; mu = 0 is plain Laplacian smoothing.  The defaults are
    Taubin's pair, pass-band 1/lam + 1/mu ~ 0.11.  fixed [V] (bool or uint8 CUDA tensor): vertices that keep their bits; pin_boundary:
    so do the vertices of open edges (the rim of an open mesh would otherwise shrink).  adj: the mesh's Adjacency, built here if None.
    All steps are one call on the current stream; nothing is read back (building adj reads one count)."""
    faces = _mesh_faces(faces, "smooth_mesh")
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda:
        raise _lib.NeumanHipError("smooth_mesh: rows must be a CUDA (HIP) tensor: there is no CPU path")
    n_verts, n_faces = int(rows.shape[0]), int(faces.shape[0])
    dev = faces.device
    rows = _vertex_rows(rows, n_verts, dev, "smooth_mesh", "rows")
    width = int(rows.shape[1])
    if width > 64:
        raise _lib.NeumanHipError(f"smooth_mesh: rows must be [V, w] with w <= 64, got {tuple(rows.shape)}")
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError(f"smooth_mesh: iterations must be an int >= 0, got {iterations!r}")
    lam, mu = float(lam), float(mu)
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError(f"smooth_mesh: lam and mu must be finite, got {lam}, {mu}")
    if fixed is not None and (not isinstance(fixed, torch.Tensor) or not fixed.is_cuda or fixed.dtype not in (torch.bool, torch.uint8)
                              or tuple(fixed.shape) != (n_verts,) or fixed.device != dev):
        raise _lib.NeumanHipError(f"smooth_mesh: fixed must be a bool or uint8 CUDA tensor [{n_verts}] on {dev}")
    adj = _adjacency_of(adj, faces, n_verts, "smooth_mesh")
    L = _lib.lib()
    I32, U8 = torch.int32, torch.uint8
    with torch.cuda.device(dev):
        hold = None                                                # composed on the device: no read-back
        if fixed is not None:
            hold = (fixed != 0).to(U8)
        if pin_boundary:
            hold = adj.boundary if hold is None else (hold | adj.boundary)
        out, scratch = torch.empty_like(rows), torch.empty_like(rows)
        _lib.check(L.nm_mesh_smooth(_lib.dev_ptr(rows), width, n_verts, _lib.dev_ptr(faces, I32), n_faces, _lib.dev_ptr(adj.inc_off, I32),
                                    _inc_ptr(adj), _lib.dev_ptr(None if hold is None else hold.contiguous(), U8), lam, mu,
                                    int(iterations), _lib.dev_ptr(out), _lib.dev_ptr(scratch), _lib.stream_ptr()), "nm_mesh_smooth")
    return out


def vertex_normals(verts, faces, adj=None):
    """Area-weighted unit normals of verts [V,3] or [B,V,3] (CUDA float32; B frames of one mesh, e.g. pose_mesh_frames' points) from the
    faces around every vertex (rule S5) -> the same shape; outward for extract_mesh's counter-clockwise faces, (0, 0, 0) at a vertex no
    proper face names.  All frames in one launch, nothing read back (building adj reads one count)."""
    faces = _mesh_faces(faces, "vertex_normals")
    dev = faces.device
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise _lib.NeumanHipError("vertex_normals: verts must be a CUDA (HIP) tensor: there is no CPU path")
    if verts.dim() not in (2, 3) or verts.shape[-1] != 3 or verts.dtype != torch.float32 or verts.device != dev or (verts.dim() == 3 and verts.shape[0] < 1):
        raise _lib.NeumanHipError(f"vertex_normals: verts must be float32 [V, 3] or [B, V, 3] (B >= 1) on {dev}, got {verts.dtype} {tuple(verts.shape)} "
                                  f"on {verts.device}")
    verts = verts.detach().contiguous()
    frames = int(verts.shape[0]) if verts.dim() == 3 else 1
    n_verts, n_faces = int(verts.shape[-2]), int(faces.shape[0])
    adj = _adjacency_of(adj, faces, n_verts, "vertex_normals")
    L = _lib.lib()
    I32 = torch.int32
    with torch.cuda.device(dev):
        normals = torch.empty_like(verts)
        _lib.check(L.nm_mesh_vertex_normals(_lib.dev_ptr(verts), frames, n_verts, _lib.dev_ptr(faces, I32), n_faces, _lib.dev_ptr(adj.inc_off, I32),
                                            _inc_ptr(adj), _lib.dev_ptr(normals), _lib.stream_ptr()), "nm_mesh_vertex_normals")
    return normals
