"""Export a lattice-coloured mesh as OBJ + MTL + PNG (csrc/mesh_atlas.hip; include/neuman_hip.h 'mesh atlas', rules A1-A5).

`mesh_texture.bake_face_colours` gives a thinned mesh a colour lattice [F,S,3] that only this project's frame renderer reads.  Here the
lattices are packed into one image: two faces share a block of (R+4) x (R+1) texels, a face's nodes are texels, and the gutter between the
two faces is filled so that a viewer's bilinear filter shows the lattice's own blend in the cells on the hypotenuse (elsewhere it differs
from it by at most a quarter of the cell's second difference).  Every face has its own three texture coordinates, the centres of its corner
nodes' texels.

    face_colours = bake_face_colours(net, verts, faces, normals, R)         # [F,S,3]
    obj, mtl, png = export_mesh("body.obj", verts, faces, face_colours, normals)      # opens in Blender, MeshLab, ...
    # or step by step, and a textured view without leaving the device:
    atlas = pack_atlas(face_colours)                                        # [H,W,3] float32
    _, face_id, _, bary = rasterizer.render_frames(world, cams, want_geometry=True)
    rgb = sample_atlas(atlas, F, R, face_id, bary)                          # [B,H',W',3]: what a bilinear viewer shows

Not here: a textured colour source inside the frame rasteriser, padding for mip-mapped viewers, glTF.  The packing and the sampling run on
CUDA tensors only; the files are written on the host."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .mesh_texture import _check_r

MATERIAL = "atlas"


def atlas_size(F, R):
    """nm_mesh_atlas_size (rule A1): the atlas of F faces at resolution R -> (W, H, nbx), Python ints.  Host only.  ValueError for an F
    that is no int >= 1 or an R outside 1..64, NeumanHipError for an atlas wider or higher than 16384 texels."""
    R = _check_r(R, "atlas_size")
    if isinstance(F, bool) or not isinstance(F, (int, np.integer)) or F < 1:
        raise ValueError(f"atlas_size: F must be an int >= 1, got {F!r}")
    W, H, nbx = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().nm_mesh_atlas_size(int(F), R, ctypes.byref(W), ctypes.byref(H), ctypes.byref(nbx)), "nm_mesh_atlas_size")
    return W.value, H.value, nbx.value


def atlas_uvs(F, R):
    """Rule A4: the texture coordinates of every face's three corners -> numpy float64 [F,3,2] (u, v), the centres of the texels of the
    nodes (0, 0), (R, 0) and (0, R); v = 1 is the image's top edge.  Needs no device."""
    W, H, nbx = atlas_size(F, R)
    f = np.arange(int(F), dtype=np.int64)
    p, odd = f >> 1, (f & 1).astype(bool)
    x = np.array([0, R, 0], np.int64)[None, :].repeat(len(f), 0)                    # the corners' local texels, lower face
    y = np.array([0, 0, R], np.int64)[None, :].repeat(len(f), 0)
    x[odd], y[odd] = R + 3 - x[odd], R - y[odd]                                     # A2: the upper face is the point reflection
    X = (p % nbx * (R + 4))[:, None] + x
    Y = (p // nbx * (R + 1))[:, None] + y
    return np.stack([(X + 0.5) / W, 1.0 - (Y + 0.5) / H], -1)


def _lattice_of(face_colours, who):
    """-> (face_colours dense, F, R) or NeumanHipError"""
    from .raster import lattice_resolution_of
    if not isinstance(face_colours, torch.Tensor) or not face_colours.is_cuda:
        raise _lib.NeumanHipError(f"{who}: face_colours must be a CUDA (HIP) tensor: there is no CPU path")
    if face_colours.dim() != 3 or face_colours.shape[0] < 1 or face_colours.dtype != torch.float32:
        raise _lib.NeumanHipError(f"{who}: face_colours must be float32 [F >= 1, S, 3], got {face_colours.dtype} {list(face_colours.shape)}")
    F = int(face_colours.shape[0])
    return face_colours.detach().contiguous(), F, lattice_resolution_of(face_colours, F, who)


def pack_atlas(face_colours):
    """nm_mesh_atlas_pack (rules A2, A3): the colour lattices [F,S,3] (CUDA float32) of a mesh -> its atlas [H,W,3] (CUDA float32), with
    (W, H) = atlas_size(F, R)[:2] and R recovered from S.  Not clamped: `frame_to_uint8` clamps.  No read-back."""
    face_colours, F, R = _lattice_of(face_colours, "pack_atlas")
    W, H, _ = atlas_size(F, R)
    _lib.require_gpu()
    with torch.cuda.device(face_colours.device):
        atlas = torch.empty((H, W, 3), device=face_colours.device, dtype=torch.float32)
        _lib.check(_lib.lib().nm_mesh_atlas_pack(_lib.dev_ptr(face_colours), F, R, _lib.dev_ptr(atlas), _lib.stream_ptr()), "nm_mesh_atlas_pack")
    return atlas


def sample_atlas(atlas, F, R, face_id, bary):
    """nm_mesh_atlas_sample (rule A5): what a viewer with bilinear filtering shows at the points (face_id [...] int32, bary [..., 3]
    float32) of a mesh whose atlas is `atlas` [H,W,3] = pack_atlas of F faces at resolution R -> float32 [..., 3]; (0, 0, 0) where
    face_id is outside [0, F).  Takes what `Rasterizer.render_frames(..., want_geometry=True)` returns.  No read-back."""
    W, H, _ = atlas_size(F, R)
    for name, a in (("atlas", atlas), ("face_id", face_id), ("bary", bary)):
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise _lib.NeumanHipError(f"sample_atlas: {name} must be a CUDA (HIP) tensor: there is no CPU path")
    dev = atlas.device
    if tuple(atlas.shape) != (H, W, 3) or atlas.dtype != torch.float32:
        raise _lib.NeumanHipError(f"sample_atlas: the atlas of {F} faces at R = {R} is float32 [{H}, {W}, 3], got {atlas.dtype} {list(atlas.shape)}")
    if face_id.dtype != torch.int32 or face_id.device != dev:
        raise _lib.NeumanHipError(f"sample_atlas: face_id must be int32 on {dev}, got {face_id.dtype} on {face_id.device}")
    if bary.dtype != torch.float32 or bary.device != dev or tuple(bary.shape) != tuple(face_id.shape) + (3,):
        raise _lib.NeumanHipError(f"sample_atlas: bary must be float32 {list(face_id.shape) + [3]} on {dev}, got {bary.dtype} {list(bary.shape)} "
                                  f"on {bary.device}")
    atlas, face_id, bary = atlas.detach().contiguous(), face_id.contiguous(), bary.detach().contiguous()
    _lib.require_gpu()
    with torch.cuda.device(dev):
        out = torch.empty(tuple(bary.shape), device=dev, dtype=torch.float32)
        if face_id.numel() > 0:
            _lib.check(_lib.lib().nm_mesh_atlas_sample(_lib.dev_ptr(atlas), int(F), int(R), _lib.dev_ptr(face_id, torch.int32), _lib.dev_ptr(bary),
                                                       face_id.numel(), _lib.dev_ptr(out), _lib.stream_ptr()), "nm_mesh_atlas_sample")
    return out


def _host(a, dtype, tail, name):
    """a tensor of any device, an array or nested lists -> numpy [n, *tail] of `dtype`, or ValueError"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    try:
        a = np.asarray(a)
    except ValueError:
        a = None
    if a is None or a.dtype == object or a.ndim != 1 + len(tail) or tuple(a.shape[1:]) != tuple(tail):
        raise ValueError(f"write_obj: {name} must be [n, {', '.join(str(t) for t in tail)}]")
    if np.issubdtype(dtype, np.integer):
        if not (np.issubdtype(a.dtype, np.integer) or np.array_equal(a, np.floor(a))):
            raise ValueError(f"write_obj: {name} must be whole numbers")
        return a.astype(dtype)
    a = a.astype(dtype)
    if not np.isfinite(a).all():
        raise ValueError(f"write_obj: {name} has a value that is not finite")
    return a


def write_obj(path, verts, faces, uvs, atlas_u8, normals=None):
    """Write `stem`.obj, .mtl and .png for path = `stem` or `stem`.obj -> the three paths.  Host only; tensors (of any device), arrays or
    nested lists.  verts [V,3], faces [F,3], uvs [F,3,2] (`atlas_uvs`), atlas_u8 uint8 [H,W,3] with (W, H) the atlas size of F faces at some
    R, normals [V,3] or None.
      .obj  mtllib and usemtl; `v` at %.9g; `vn` if normals are given; 3 F `vt` at %.10f, no two faces sharing one; 1-based `f a/t ...` or
            `f a/t/n ...` with t = 3 f + k + 1 and n = a
      .mtl  newmtl, a white Kd, map_Kd; both files name their neighbour by its basename
      .png  `render_utils.save_png`
    ValueError for a face index outside [0, V), a vertex that is not finite, counts that do not match, an atlas of another shape."""
    from .render_utils import save_png
    v, f = _host(verts, np.float64, (3,), 'verts'), _host(faces, np.int64, (3,), 'faces')
    t = _host(uvs, np.float64, (3, 2), 'uvs')
    n = None if normals is None else _host(normals, np.float64, (3,), 'normals')
    if isinstance(atlas_u8, torch.Tensor):
        atlas_u8 = atlas_u8.detach().cpu().numpy()
    image = np.asarray(atlas_u8)
    if len(f) < 1 or len(t) != len(f):
        raise ValueError(f"write_obj: {len(t)} faces' uvs for {len(f)} faces (at least one)")
    if n is not None and len(n) != len(v):
        raise ValueError(f"write_obj: {len(n)} normals for {len(v)} vertices")
    if f.min() < 0 or f.max() >= len(v):
        raise ValueError(f"write_obj: a face names a vertex outside [0, {len(v)})")
    sizes = set()
    for R in range(1, 65):
        try:
            sizes.add(atlas_size(len(f), R)[:2])
        except _lib.NeumanHipError:
            break
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3 or (image.shape[1], image.shape[0]) not in sizes:
        raise ValueError(f"write_obj: atlas_u8 must be uint8 [H, W, 3] with (W, H) = atlas_size({len(f)}, R)[:2] for some R, got {image.dtype} "
                         f"{list(image.shape)}")
    path = os.fspath(path)
    stem = path[:-4] if path.lower().endswith(".obj") else path
    base = os.path.basename(stem)
    lines = [f"mtllib {base}.mtl", f"usemtl {MATERIAL}"]
    lines += ["v %.9g %.9g %.9g" % tuple(r) for r in v.tolist()]
    if n is not None:
        lines += ["vn %.9g %.9g %.9g" % tuple(r) for r in n.tolist()]
    lines += ["vt %.10f %.10f" % tuple(r) for r in t.reshape(-1, 2).tolist()]
    corner = "%d/%d" if n is None else "%d/%d/%d"
    for i, r in enumerate(f.tolist()):
        lines.append("f " + " ".join(corner % ((a + 1, 3 * i + k + 1) if n is None else (a + 1, 3 * i + k + 1, a + 1)) for k, a in enumerate(r)))
    with open(stem + ".obj", "w", newline="\n") as out:
        out.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w", newline="\n") as out:
        out.write(f"newmtl {MATERIAL}\nKd 1 1 1\nmap_Kd {base}.png\n")
    save_png(stem + ".png", np.ascontiguousarray(image))
    return stem + ".obj", stem + ".mtl", stem + ".png"


def export_mesh(path, verts, faces, face_colours, normals=None):
    """A lattice-coloured mesh as OBJ + MTL + PNG -> the three paths: `pack_atlas`, `frame_to_uint8` (clip to [0, 1], round), ONE
    device-to-host copy of the byte atlas, `atlas_uvs`, `write_obj`.  verts [V,3], faces [F,3] and normals [V,3] as `write_obj` takes
    them; face_colours [F,S,3] CUDA float32 as `bake_face_colours` returns it."""
    from .render_utils import frame_to_uint8
    face_colours, F, R = _lattice_of(face_colours, "export_mesh")
    atlas_u8 = frame_to_uint8(pack_atlas(face_colours)).cpu().numpy()
    return write_obj(path, verts, faces, atlas_uvs(F, R), atlas_u8, normals)
