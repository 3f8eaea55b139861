"""A trained density as a triangle mesh (csrc/isosurface.hip; include/neuman_hip.h 'isosurface', rules M1-M7).

The reference stops at images; this turns a net's learned field into geometry that the rest of the package takes as it takes any mesh:
render_utils.rasterize_mesh / overlay_smpl to look at it, ray_utils.Mesh (nm_mesh_create, nm_signed_distance) to compare it with the
SMPL surface, save_ply to hand it on.

    box = occupancy.canonical_aabb(static_verts, 0.1)                       # a human net lives in canonical space
    verts, faces, normals, colours = extract_net_mesh(human.coarse_human_net, box, 128, level=10.0)
    save_ply('body.ply', verts, faces, normals, colours)

`density_grid` samples the raw (pre-ReLU) density sigma, which is smooth through zero, on the grid of rule M1 with the density-only launch
(nm_mlp_sigma_rays) at the precision of the net's coarse pass; `extract_mesh` runs marching tetrahedra on any such grid.  `level` has no
default: a sensible density threshold depends on the scene's scale.  Every tensor is a CUDA tensor; there is no CPU path."""
import ctypes
import struct

import numpy as np
import torch

from . import _lib
from .occupancy import _check_box, _refuse_time_net

SLAB_BYTES = 256 << 20                                             # density_grid's default budget for one slab's raw output


def _check_dims(res):
    dims = (int(res),) * 3 if isinstance(res, (int, np.integer)) else tuple(int(r) for r in res)
    if len(dims) != 3 or min(dims) < 2 or dims[0] * dims[1] * dims[2] >= 1 << 31:
        raise ValueError(f"res must be an int or (nx, ny, nz), every entry >= 2 and fewer than 2^31 vertices in all, got {res}")
    return dims


def grid_axes(aabb, dims):
    """The vertex coordinates of rule M1 per axis, float32 numpy: fmaf(i, h, lo) with h = (hi - lo) / (n - 1) in float32 (the fused
    multiply-add through float64: the product is exact there)."""
    box = _check_box(aabb).numpy()
    out = []
    for a, n in enumerate(dims):
        h = np.float32(box[3 + a] - box[a]) / np.float32(n - 1)
        out.append((np.arange(n, dtype=np.float64) * np.float64(h) + np.float64(box[a])).astype(np.float32))
    return out


def density_grid(net, aabb, res, precision=None, slab_bytes=SLAB_BYTES):
    """[nz, ny, nx] float32 on the net's device: the raw density (the pre-ReLU sigma the kernels return) at the grid vertices of rule M1
    over `aabb` (lo xyz, hi xyz); res = n or (nx, ny, nz) vertices.  A grid row along x is a ray -- origin (lo_x, y_j, z_k), direction
    (1, 0, 0), z_i = i h_x -- so no point tensor is made: nm_mlp_sigma_rays builds the points (they are rule M1's to within one rounding of
    x) and returns sigma bit-identical to the net's own forward at those points.  The rows go in slabs of whole z-layers whose raw output
    [rows, nx, 4] stays within `slab_bytes`."""
    _refuse_time_net(net)
    nx, ny, nz = _check_dims(res)
    box = _check_box(aabb)
    net._guard()
    dev = next(net.parameters()).device
    if dev.type != 'cuda':
        raise _lib.NeumanHipError("density_grid: the net must live on a CUDA (HIP) device: there is no CPU path")
    xs, ys, zs = grid_axes(box, (nx, ny, nz))
    with torch.no_grad(), torch.cuda.device(dev):
        b = box.numpy()
        h_x = np.float32(b[3] - b[0]) / np.float32(nx - 1)
        z_row = (torch.arange(nx, device=dev, dtype=torch.float32) * float(h_x))
        y_t, z_t = torch.from_numpy(ys).to(dev), torch.from_numpy(zs).to(dev)
        direction = torch.tensor([1.0, 0.0, 0.0], device=dev)
        grid = torch.empty((nz, ny, nx), device=dev, dtype=torch.float32)
        layers = max(1, int(slab_bytes) // (ny * nx * 16))
        for k0 in range(0, nz, layers):
            k1 = min(nz, k0 + layers)
            rows = (k1 - k0) * ny
            o = torch.empty((k1 - k0, ny, 3), device=dev, dtype=torch.float32)
            o[..., 0] = float(box[0])
            o[..., 1] = y_t[None, :]
            o[..., 2] = z_t[k0:k1, None]
            raw = net.forward_rays(o.reshape(rows, 3), direction.expand(rows, 3).contiguous(), z_row.expand(rows, nx).contiguous(),
                                   precision=precision, sigma_only=True)
            grid[k0:k1] = raw[..., 3].reshape(k1 - k0, ny, nx)
    return grid


def extract_mesh(field, aabb, level):
    """Marching tetrahedra on field [nz, ny, nx] (CUDA float32, values at the grid vertices over aabb = (lo xyz, hi xyz)): the surface
    field = level, inside where field > level -> (verts [Nv,3] f32, faces [Nf,3] int32, normals [Nv,3] f32 = -grad / |grad|) on the
    field's device, counter-clockwise faces seen from outside.  Two launches' worth of work: nm_isosurface_count (one 16-byte read-back
    sizes the outputs exactly), then nm_isosurface_fill; an empty surface returns empty tensors without the second."""
    if not isinstance(field, torch.Tensor) or not field.is_cuda:
        raise _lib.NeumanHipError("extract_mesh: field must be a CUDA (HIP) tensor: there is no CPU path")
    if field.dim() != 3 or field.dtype != torch.float32:
        raise _lib.NeumanHipError(f"extract_mesh: field must be float32 [nz, ny, nx], got {field.dtype} {tuple(field.shape)}")
    level = float(level)
    if not np.isfinite(level):
        raise ValueError(f"extract_mesh: level must be finite, got {level}")
    box = _check_box(aabb)
    field = field.detach().contiguous()
    nz, ny, nx = (int(s) for s in field.shape)
    _check_dims((nx, ny, nz))
    dev = field.device
    L = _lib.lib()
    box_c = (ctypes.c_float * 6)(*box.tolist())
    with torch.cuda.device(dev):
        nbytes = int(L.nm_isosurface_workspace_bytes(nx, ny, nz))
        if nbytes < 0:
            _lib.check(nbytes, "nm_isosurface_workspace_bytes")
        ws = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
        n_verts, n_faces = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(L.nm_isosurface_count(_lib.dev_ptr(field, name='field'), nx, ny, nz, box_c, level, _lib.dev_ptr(ws, torch.uint8), nbytes,
                                         ctypes.byref(n_verts), ctypes.byref(n_faces), _lib.stream_ptr()), "nm_isosurface_count")
        nv, nf = int(n_verts.value), int(n_faces.value)
        verts = torch.empty((nv, 3), device=dev, dtype=torch.float32)
        normals = torch.empty((nv, 3), device=dev, dtype=torch.float32)
        faces = torch.empty((nf, 3), device=dev, dtype=torch.int32)
        if nv > 0:
            _lib.check(L.nm_isosurface_fill(_lib.dev_ptr(field, name='field'), nx, ny, nz, box_c, level, _lib.dev_ptr(ws, torch.uint8), nbytes,
                                            _lib.dev_ptr(verts), _lib.dev_ptr(normals), _lib.dev_ptr(faces, torch.int32), nv, nf, _lib.stream_ptr()),
                       "nm_isosurface_fill")
    return verts, faces, normals


def extract_net_mesh(net, aabb, res, level, colour=True, precision=None, slab_bytes=SLAB_BYTES):
    """density_grid + extract_mesh on a static net (a background Joiner, or HumanNeRF.coarse_human_net with the box of
    occupancy.canonical_aabb) -> (verts, faces, normals, colours).  colour: per-vertex RGB [Nv,3] in [0, 1], the sigmoid of the net's own
    forward at the vertices seen along -normal (from outside, head on); the plain head takes no view.  Otherwise colours is None."""
    field = density_grid(net, aabb, res, precision=precision, slab_bytes=slab_bytes)
    verts, faces, normals = extract_mesh(field, aabb, level)
    colours = None
    if colour:
        with torch.no_grad():
            if verts.shape[0] == 0:
                colours = torch.empty((0, 3), device=verts.device, dtype=torch.float32)
            else:
                raw = net(verts, -normals if net.nerf.use_viewdirs else None, precision=precision)
                colours = torch.sigmoid(raw[..., :3])
    return verts, faces, normals, colours


def _rows(a, width, name):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().tolist()
    elif hasattr(a, 'tolist'):
        a = a.tolist()
    rows = [tuple(r) for r in a]
    if any(len(r) != width for r in rows):
        raise ValueError(f"save_ply: {name} must be [n, {width}]")
    return rows


def save_ply(path, verts, faces, normals=None, colours=None):
    """Binary little-endian PLY: vertex x y z (float), then nx ny nz (float) if normals, then red green blue (uchar, colours in [0, 1]
    scaled by 255 and rounded) if colours; faces as `list uchar int vertex_indices`.  Tensors (of any device), arrays or nested lists."""
    v, f = _rows(verts, 3, 'verts'), _rows(faces, 3, 'faces')
    n, c = _rows(normals, 3, 'normals'), _rows(colours, 3, 'colours')
    for extra, name in ((n, 'normals'), (c, 'colours')):
        if extra is not None and len(extra) != len(v):
            raise ValueError(f"save_ply: {len(extra)} {name} for {len(v)} vertices")
    if any(not 0 <= int(i) < len(v) for r in f for i in r):
        raise ValueError(f"save_ply: a face names a vertex outside [0, {len(v)})")
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    fmt = "<3f"
    if n is not None:
        head += ["property float nx", "property float ny", "property float nz"]
        fmt += "3f"
    if c is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        fmt += "3B"
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    rec, face = struct.Struct(fmt), struct.Struct("<B3i")
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        for i, p in enumerate(v):
            row = [float(x) for x in p]
            if n is not None:
                row += [float(x) for x in n[i]]
            if c is not None:
                row += [int(min(max(float(x), 0.0), 1.0) * 255.0 + 0.5) for x in c[i]]
            out.write(rec.pack(*row))
        for r in f:
            out.write(face.pack(3, *(int(i) for i in r)))
