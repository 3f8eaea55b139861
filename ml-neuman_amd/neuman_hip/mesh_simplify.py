"""Thin a triangle mesh by clustering its vertices on a uniform grid (csrc/mesh_simplify.hip; include/neuman_hip.h 'mesh simplify', rules
Q1-Q9).

What mesh_extract.extract_mesh emits has the size its grid dictates: a 128^3 extraction is some 80 000 vertices and twice as many faces,
and binding, posing, drawing and saving it all pay for every one.  `simplify_mesh` merges the vertices of every cell of edge `cell` into
one and keeps the faces whose corners fall into three different cells.  With placement='quadric' (the default) a cell's vertex goes to the
point that minimises its squared distance, weighted by area^2, to the planes of the faces around the cell's vertices, which keeps edges and
corners sharp; placement='mean' puts it at the vertices' mean, which rounds them off.  Attributes (colours, any float32 [V,w]) are averaged
per cell:

    verts, faces, normals = clean_mesh(*extract_mesh(field, box, level))
    verts = smooth_mesh(verts, faces, iterations=10)
    verts, faces, colours = simplify_mesh(verts, faces, 0.02, colours, aabb=box)        # cells of 2 cm
    normals = vertex_normals(verts, faces)                                              # the old normals fit no longer
    binding = bind_mesh(verts, ...)

The output has no unreferenced vertex and no degenerate face, and components, adjacency, bind_mesh and the rasteriser take it as they take
any mesh.  Every tensor is a CUDA tensor; there is no CPU path."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .mesh_extract import _mesh_faces, _vertex_rows
from .mesh_smooth import _adjacency_of, _inc_ptr
from .occupancy import _check_box

PLACEMENTS = {'mean': 0, 'quadric': 1}


def grid_of(aabb, cell):
    """The grid of rule Q2 over aabb = (lo xyz, hi xyz) with cells of edge `cell` -> (lo: three floats, h, (nx, ny, nz)): lo and h rounded to
    float32 once, dims = max(1, ceil(extent / h)) per axis, so the grid covers the box; ValueError for a cell that is not finite and > 0 or a
    grid of 2^31 cells or more."""
    box = _check_box(aabb).numpy()
    h = float(np.float32(cell))
    if not (math.isfinite(h) and h > 0):
        raise ValueError(f"simplify_mesh: cell must be finite and > 0, got {cell!r}")
    dims = tuple(max(1, int(math.ceil((float(box[3 + a]) - float(box[a])) / h))) for a in range(3))
    if dims[0] * dims[1] * dims[2] >= 1 << 31:
        raise ValueError(f"simplify_mesh: cell = {cell} gives a grid of {dims[0]} x {dims[1]} x {dims[2]}: 2^31 cells or more")
    return tuple(float(x) for x in box[:3]), h, dims


def _check_cell(cell):
    if isinstance(cell, bool) or not isinstance(cell, (int, float, np.integer, np.floating)) or not math.isfinite(float(cell)) or float(cell) <= 0:
        raise ValueError(f"simplify_mesh: cell must be a finite number > 0, got {cell!r}")
    return float(cell)


def simplify_mesh(verts, faces, cell, *attrs, aabb=None, placement='quadric', adj=None, return_map=False):
    """The mesh (verts [V,3] CUDA float32, faces [F,3] CUDA int32) clustered on a grid of cell edge `cell` -> (verts' [K,3], faces' [F',3],
    *attrs'), and with return_map also (vert_cluster [V] int32: old vertex -> new, -1 for a vertex that is dropped; face_src [F'] int32: new
    face -> old).  attrs: float32 [V,w], 1 <= w <= 64, averaged over each cell's vertices.  aabb: the six floats extract_mesh takes; the grid
    starts at its lower corner with dims = ceil(extent / cell), and a vertex outside it belongs to the nearest border cell.  aabb=None takes
    the box of the finite vertices.  placement: 'quadric' or 'mean'; 'quadric' needs the mesh's Adjacency (mesh_smooth.adjacency), built
    here if adj is None.  Kept faces stay in their old order, each rotated so that its smallest new index comes first; of the faces that
    collapse onto the same three cells with the same orientation the first is kept.

    Read-backs: one (the output's sizes), plus one if aabb is None (the box), plus one if the placement is 'quadric' and adj is None (the
    lists' length).  A face that names a vertex outside [0, V) raises NeumanHipError."""
    cell = _check_cell(cell)
    if placement not in PLACEMENTS:
        raise ValueError(f"simplify_mesh: placement must be 'quadric' or 'mean', got {placement!r}")
    faces = _mesh_faces(faces, "simplify_mesh")
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise _lib.NeumanHipError("simplify_mesh: verts must be a CUDA (HIP) tensor: there is no CPU path")
    n_verts, n_faces = int(verts.shape[0]), int(faces.shape[0])
    dev = faces.device
    rows = [_vertex_rows(a, n_verts, dev, "simplify_mesh", "verts" if i == 0 else f"attribute {i - 1}") for i, a in enumerate((verts,) + attrs)]
    if rows[0].shape[1] != 3:
        raise _lib.NeumanHipError(f"simplify_mesh: verts must be [V, 3], got {tuple(verts.shape)}")
    if any(a.shape[1] > 64 for a in rows[1:]):
        raise _lib.NeumanHipError("simplify_mesh: an attribute must be [V, w] with w <= 64")
    verts = rows[0]
    if adj is not None or placement == 'quadric':
        adj = _adjacency_of(adj, faces, n_verts, "simplify_mesh")
    if aabb is None:
        with torch.cuda.device(dev):
            finite = torch.isfinite(verts).all(1, keepdim=True)
            lo = torch.where(finite, verts, torch.full_like(verts, math.inf)).amin(0) if n_verts else torch.zeros(3, device=dev)
            hi = torch.where(finite, verts, torch.full_like(verts, -math.inf)).amax(0) if n_verts else torch.zeros(3, device=dev)
            box = torch.cat([lo, hi]).cpu()                        # the one extra read-back
        if not bool(torch.isfinite(box).all()):                    # no finite vertex: any grid serves, nothing survives
            box = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
        box = torch.cat([box[:3], torch.maximum(box[3:], torch.nextafter(box[:3], torch.full((3,), math.inf)))])     # a flat axis: one cell
        aabb = box.tolist()
    lo, h, dims = grid_of(aabb, cell)
    L = _lib.lib()
    I32, U8, F32 = torch.int32, torch.uint8, torch.float32
    lo_c = (ctypes.c_float * 3)(*lo)
    with torch.cuda.device(dev):
        nbytes = int(L.nm_mesh_simplify_workspace_bytes(n_verts, n_faces, *dims))
        if nbytes < 0:
            _lib.check(nbytes, "nm_mesh_simplify_workspace_bytes")
        ws = torch.empty((nbytes,), device=dev, dtype=U8)
        vert_cluster = torch.empty((n_verts,), device=dev, dtype=I32)
        k, nf = ctypes.c_int64(0), ctypes.c_int64(0)
        mesh = (_lib.dev_ptr(verts), n_verts, _lib.dev_ptr(faces, I32), n_faces, lo_c, h, *dims)
        _lib.check(L.nm_mesh_simplify_count(*mesh, _lib.dev_ptr(vert_cluster, I32), _lib.dev_ptr(ws, U8), nbytes, ctypes.byref(k), ctypes.byref(nf),
                                            _lib.stream_ptr()), "nm_mesh_simplify_count")
        k, nf = int(k.value), int(nf.value)
        verts_out = torch.empty((k, 3), device=dev, dtype=F32)
        faces_out = torch.empty((nf, 3), device=dev, dtype=I32)
        face_src = torch.empty((nf,), device=dev, dtype=I32)
        quadric = placement == 'quadric'
        _lib.check(L.nm_mesh_simplify_fill(*mesh, PLACEMENTS[placement], _lib.dev_ptr(adj.inc_off, I32) if quadric else None,
                                           _inc_ptr(adj) if quadric else None, _lib.dev_ptr(ws, U8), nbytes, _lib.dev_ptr(verts_out),
                                           _lib.dev_ptr(faces_out, I32), _lib.dev_ptr(face_src, I32), k, nf, _lib.stream_ptr()), "nm_mesh_simplify_fill")
        out = []
        for a in rows[1:]:
            w = int(a.shape[1])
            g = torch.empty((k, w), device=dev, dtype=F32)
            _lib.check(L.nm_mesh_simplify_rows(_lib.dev_ptr(a), w, n_verts, n_faces, *dims, _lib.dev_ptr(ws, U8), nbytes, _lib.dev_ptr(g), k,
                                               _lib.stream_ptr()), "nm_mesh_simplify_rows")
            out.append(g)
    result = (verts_out, faces_out, *out)
    return result + (vert_cluster, face_src) if return_map else result
