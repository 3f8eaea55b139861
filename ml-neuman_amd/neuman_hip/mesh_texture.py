"""Colour a mesh per face instead of per vertex (csrc/mesh_lattice.hip, csrc/raster_frames.hip; include/neuman_hip.h 'mesh lattice', rules
L1-L3 and F2', and 'mesh mip', rules M1-M3 and F2'').

A mesh from mesh_extract.extract_net_mesh carries its look as one RGB per vertex.  Thinning it (mesh_simplify.simplify_mesh) keeps the shape
and makes binding, posing and drawing cheap, but leaves a fraction of the vertices, so the look is sampled that much more sparsely and blended
across faces several pixels wide.  A colour lattice ("mesh colours") keeps more colour samples than the mesh has vertices: every face gets
the nodes of a regular barycentric grid of resolution R -- (R+1)(R+2)/2 of them, no UV atlas, no seams, no packing -- and the frame rasteriser
blends the three nodes around a pixel's point.  The lattice belongs to the canonical mesh: baked once, it serves every frame of every posed
sequence.

    verts, faces, normals, _ = extract_net_mesh(net, box, 128, level=10.0, largest=1, smooth=10, simplify=4 * h)      # thinned
    R = lattice_resolution(verts, faces, texel=h)                           # nodes about one grid step apart on the longest edge
    face_colours = bake_face_colours(net, verts, faces, normals, R)         # [F,S,3]: the net asked at every node
    frames = render_mesh_frames(posed, faces, caps, normals=posed_normals, face_colours=face_colours)

A lattice is point-sampled at the pixel centre, so a face drawn two or three pixels wide -- a far camera, or a face much shorter than the
mesh's longest edge -- shows moire and shimmers from frame to frame.  `lattice_pyramid` filters the lattice once into coarser levels, and
the frame renderer picks a level per frame and face from the face's size on the screen and blends two of them:

    R = lattice_resolution(verts, faces, texel=h, pow2=True)                # a power of two: every halving is a level, down to R = 2
    pyramid = lattice_pyramid(bake_face_colours(net, verts, faces, normals, R))
    frames = render_mesh_frames(posed, faces, caps, normals=posed_normals, face_colours=pyramid)       # lod_scale=1.0

Not here (mesh_export.py writes the OBJ): a resolution that varies from face to face; a level that varies inside a face, anisotropic
filtering; filtering the corner nodes across the faces around a vertex; atlas padding for mip-mapping viewers.  Every tensor is a CUDA
tensor; there is no CPU path."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .mesh_extract import _mesh_faces
from .occupancy import _refuse_time_net

MAX_R = 64


def _check_r(R, who):
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= MAX_R:
        raise ValueError(f"{who}: R must be an int in 1..{MAX_R}, got {R!r}")
    return int(R)


def lattice_size(R):
    """S = (R+1)(R+2)/2, the nodes of one face at resolution R (rule L1)."""
    R = _check_r(R, "lattice_size")
    return (R + 1) * (R + 2) // 2


def lattice_rows(rows, faces, R):
    """nm_mesh_lattice_rows (rule L2): per-vertex rows [V,w] (CUDA float32) blended to the lattice nodes of faces [F,3] (CUDA int32) ->
    [F,S,w].  With the vertices it gives the nodes' positions, with the vertex normals their (unnormalised) normals, with per-vertex colours
    a lattice that renders as those colours do.  One read-back (the face check); a face that names a vertex outside [0, V) raises
    NeumanHipError."""
    R = _check_r(R, "lattice_rows")
    faces = _mesh_faces(faces, "lattice_rows")
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda:
        raise _lib.NeumanHipError("lattice_rows: rows must be a CUDA (HIP) tensor: there is no CPU path")
    dev = faces.device
    if rows.dim() != 2 or rows.shape[0] < 1 or rows.shape[1] < 1 or rows.dtype != torch.float32 or rows.device != dev:
        raise _lib.NeumanHipError(f"lattice_rows: rows must be float32 [V >= 1, w >= 1] on {dev}, got {rows.dtype} {tuple(rows.shape)} on {rows.device}")
    if faces.shape[0] < 1:
        raise _lib.NeumanHipError("lattice_rows: a mesh without faces has no lattice")
    rows = rows.detach().contiguous()
    n_faces, n_verts, w = int(faces.shape[0]), int(rows.shape[0]), int(rows.shape[1])
    _lib.require_gpu()
    with torch.cuda.device(dev):
        out = torch.empty((n_faces, lattice_size(R), w), device=dev, dtype=torch.float32)
        _lib.check(_lib.lib().nm_mesh_lattice_rows(_lib.dev_ptr(faces, torch.int32), n_faces, n_verts, _lib.dev_ptr(rows), w, R, _lib.dev_ptr(out),
                                                   _lib.stream_ptr()), "nm_mesh_lattice_rows")
    return out


def bake_face_colours(source, verts, faces, normals, R, precision=None, chunk=1 << 20):
    """The colour lattice of a mesh -> [F,S,3] float32 in [0, 1], what `render_mesh_frames(face_colours=)` takes.  verts [V,3], normals
    [V,3] (CUDA float32) and faces [F,3] (CUDA int32) as extract_net_mesh returns them, in the space `source` lives in (canonical for a human
    net).  source: a static net (a background Joiner, or HumanNeRF.coarse_human_net), evaluated exactly as extract_net_mesh colours vertices
    -- the net's own forward at the node positions seen along -normalize(node normal), then a sigmoid; the plain head takes no view; a
    time-conditioned net is refused as it is there -- or any callable (points [n,3], dirs [n,3]) -> rgb [n,3], whose values are clamped to
    [0, 1].  The node positions and normals are rule L2's blends of the vertices' (`lattice_rows`); the nodes go through `source` in chunks
    of `chunk`."""
    R = _check_r(R, "bake_face_colours")
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1:
        raise ValueError(f"bake_face_colours: chunk must be an int >= 1, got {chunk!r}")
    is_net = hasattr(source, 'nerf')
    if is_net:
        _refuse_time_net(source)
    elif not callable(source):
        raise TypeError("bake_face_colours: source must be a static net or a callable (points [n,3], dirs [n,3]) -> rgb [n,3]")
    for name, a in (("verts", verts), ("normals", normals)):
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise _lib.NeumanHipError(f"bake_face_colours: {name} must be a CUDA (HIP) tensor: there is no CPU path")
        if a.dim() != 2 or a.shape[1] != 3 or a.shape != verts.shape:
            raise _lib.NeumanHipError(f"bake_face_colours: verts and normals must both be [V, 3], got {name} {tuple(a.shape)}")
    with torch.no_grad():
        points = lattice_rows(verts, faces, R)
        shape = tuple(points.shape)
        points = points.reshape(-1, 3)
        node_normals = lattice_rows(normals, faces, R).reshape(-1, 3)
        out = torch.empty_like(points)
        for n0 in range(0, points.shape[0], int(chunk)):
            p, n = points[n0:n0 + chunk], node_normals[n0:n0 + chunk]
            dirs = -torch.nn.functional.normalize(n, dim=-1)
            if is_net:
                raw = source(p, dirs if source.nerf.use_viewdirs else None, precision=precision)
                rgb = torch.sigmoid(raw[..., :3])
            else:
                rgb = source(p, dirs)
                if not isinstance(rgb, torch.Tensor) or tuple(rgb.shape) != tuple(p.shape) or rgb.device != p.device:
                    raise _lib.NeumanHipError(f"bake_face_colours: source must return rgb {list(p.shape)} on {p.device}, got "
                                              f"{list(getattr(rgb, 'shape', ()))}")
                rgb = rgb.to(torch.float32).clamp(0.0, 1.0)
            out[n0:n0 + chunk] = rgb
    return out.reshape(shape)


def lattice_resolution(verts, faces, texel, pow2=False):
    """The resolution at which the nodes of the mesh's longest edge lie about `texel` apart: clamp(ceil(longest edge / texel), 1, 64), a
    Python int.  The edge lengths are computed on the device; one read-back (the longest).  pow2: round that up to a power of two (still at
    most 64), so that every halving down to R = 1 is a level `lattice_pyramid` can make."""
    if isinstance(texel, bool) or not isinstance(texel, (int, float, np.integer, np.floating)) or not math.isfinite(float(texel)) or float(texel) <= 0:
        raise ValueError(f"lattice_resolution: texel must be a finite length > 0, got {texel!r}")
    faces = _mesh_faces(faces, "lattice_resolution")
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise _lib.NeumanHipError("lattice_resolution: verts must be a CUDA (HIP) tensor: there is no CPU path")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.device != faces.device:
        raise _lib.NeumanHipError(f"lattice_resolution: verts must be [V, 3] on {faces.device}, got {tuple(verts.shape)} on {verts.device}")
    if faces.shape[0] < 1 or verts.shape[0] < 1:
        return 1
    pow2 = bool(pow2)
    with torch.no_grad():
        # (an index outside [0, V) is clamped, not followed: lattice_rows is what refuses such a mesh)
        corners = verts.detach().to(torch.float32)[faces.long().clamp(0, verts.shape[0] - 1)]      # [F,3,3]
        longest = float((corners - corners.roll(1, 1)).norm(dim=-1).max())                         # the one read-back
    if not math.isfinite(longest):
        raise _lib.NeumanHipError("lattice_resolution: the mesh has a vertex that is not finite")
    R = int(min(max(math.ceil(longest / float(texel)), 1), MAX_R))
    return 1 << (R - 1).bit_length() if pow2 else R


def lattice_levels(R):
    """The levels a lattice of resolution R has ('mesh mip', rule M1): level l has resolution R >> l while 2^l divides R, so 1 + the trailing
    zero bits of R -- 4 for R = 8, 1 for an odd R, 7 for R = 64."""
    R = _check_r(R, "lattice_levels")
    return (R & -R).bit_length()


def filtered_levels(R):
    """The levels `lattice_pyramid` makes by default: `lattice_levels(R)` without a coarsest level of resolution 1 (at least one level).
    Rule M1 copies corner nodes, so a level of resolution 1 -- three corners and nothing else -- is the lattice point-sampled at the vertices:
    it filters nothing, and a face small enough to reach it would show the aliasing the pyramid is there to remove.  Every other level has
    edge or interior nodes, which are averages.  3 levels for R = 8 (8, 4, 2), 6 for R = 64, 3 for R = 12 (12, 6, 3), 1 for R <= 2 or odd."""
    most = lattice_levels(R)
    return max(most - 1, 1) if R >> (most - 1) == 1 else most


class LatticePyramid:
    """A colour lattice and its coarser levels as `lattice_pyramid` makes them.  data: the flat float32 buffer, level-major (level k is a
    contiguous [F,S(R >> k),w] block after the finer levels' blocks); R: level 0's resolution; levels; F faces; w columns."""

    def __init__(self, data, R, levels, F, w):
        self.data, self.R, self.levels, self.F, self.w = data, int(R), int(levels), int(F), int(w)

    def level(self, k):
        """the [F,S(R >> k),w] view of level k: a lattice like any other (level 0 is the input's bytes)"""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < self.levels:
            raise ValueError(f"LatticePyramid.level: k must be an int in 0..{self.levels - 1}, got {k!r}")
        before = sum(lattice_size(self.R >> j) for j in range(k))
        S = lattice_size(self.R >> k)
        return self.data[self.F * before * self.w:self.F * (before + S) * self.w].view(self.F, S, self.w)


def lattice_pyramid(face_colours, levels=None):
    """nm_mesh_lattice_pyramid (rule M1): a lattice [F,S(R),w] (CUDA float32, w <= 64) -> its LatticePyramid of `levels` levels, at most
    `lattice_levels(R)` (more is a ValueError).  levels=None: `filtered_levels(R)`, every level that has a filtered node -- the R = 1 level
    of a power-of-two R is left out, `levels=lattice_levels(R)` asks for it.  levels - 1 launches, no read-back.  What
    `render_mesh_frames(face_colours=)` filters with; every `.level(k)` is a lattice that `pack_atlas`, `export_mesh` and the renderer take."""
    who = "lattice_pyramid"
    if not isinstance(face_colours, torch.Tensor) or not face_colours.is_cuda:
        raise _lib.NeumanHipError(f"{who}: face_colours must be a CUDA (HIP) tensor: there is no CPU path")
    shape = tuple(face_colours.shape)
    R = (math.isqrt(8 * int(shape[1]) + 1) - 3) // 2 if len(shape) == 3 else 0
    if len(shape) != 3 or shape[0] < 1 or not 1 <= shape[2] <= 64 or not 1 <= R <= MAX_R or (R + 1) * (R + 2) // 2 != shape[1] or face_colours.dtype != torch.float32:
        raise _lib.NeumanHipError(f"{who}: face_colours must be float32 [F >= 1, S, 1 <= w <= 64] with S = (R+1)(R+2)/2 nodes for a resolution 1 <= R <= {MAX_R}, "
                                  f"got {face_colours.dtype} {list(shape)}")
    most = lattice_levels(R)
    if levels is None:
        levels = filtered_levels(R)
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= levels <= most:
        raise ValueError(f"{who}: levels must be an int in 1..{most} for R = {R}, got {levels!r}")
    levels = int(levels)
    face_colours = face_colours.detach().contiguous()
    F, w = int(shape[0]), int(shape[2])
    _lib.require_gpu()
    total = ctypes.c_int64(0)
    _lib.check(_lib.lib().nm_mesh_lattice_pyramid_size(R, levels, ctypes.byref(total)), "nm_mesh_lattice_pyramid_size")
    with torch.cuda.device(face_colours.device):
        data = torch.empty((F * int(total.value) * w,), device=face_colours.device, dtype=torch.float32)
        _lib.check(_lib.lib().nm_mesh_lattice_pyramid(_lib.dev_ptr(face_colours), F, R, levels, w, _lib.dev_ptr(data), _lib.stream_ptr()),
                   "nm_mesh_lattice_pyramid")
    return LatticePyramid(data, R, levels, F, w)
