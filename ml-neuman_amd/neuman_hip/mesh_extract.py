"""A trained density as a triangle mesh (csrc/isosurface.hip; include/neuman_hip.h 'isosurface', rules M1-M7).

The reference stops at images; this turns a net's learned field into geometry that the rest of the package takes as it takes any mesh:
render_utils.rasterize_mesh / overlay_smpl to look at it, ray_utils.Mesh (nm_mesh_create, nm_signed_distance) to compare it with the
SMPL surface, save_ply to hand it on.

    box = occupancy.canonical_aabb(static_verts, 0.1)                       # a human net lives in canonical space
    verts, faces, normals, colours = extract_net_mesh(human.coarse_human_net, box, 128, level=10.0)
    save_ply('body.ply', verts, faces, normals, colours)

`density_grid` samples the raw (pre-ReLU) density sigma, which is smooth through zero, on the grid of rule M1 with the density-only launch
(nm_mlp_sigma_rays) at the precision of the net's coarse pass; `extract_mesh` runs marching tetrahedra on any such grid.  `level` has no
default: a sensible density threshold depends on the scene's scale.  Every tensor is a CUDA tensor; there is no CPU path.

A learned density crosses any level in empty space too: the mesh is the body plus small closed blobs.  `components` labels the connected
components of a mesh, `select_components` compacts it to some of them and `clean_mesh` does both (csrc/mesh_components.hip; the header's
'mesh components', rules C1-C7); `extract_net_mesh(..., largest=, min_faces=)` cleans before it evaluates colours:

    verts, faces, normals, colours = extract_net_mesh(human.coarse_human_net, box, 128, level=10.0, largest=1)      # the body alone
    verts, faces, normals = clean_mesh(verts, faces, normals, largest=None, min_faces=200)                             # or: drop the small ones
    verts, faces, normals, colours = extract_net_mesh(human.coarse_human_net, box, 128, level=10.0, largest=1, smooth=10)  # ... and smoothed

`smooth=` runs neuman_hip.mesh_smooth (smooth_mesh, vertex_normals; csrc/mesh_smooth.hip, the header's 'mesh smooth', rules S1-S6) after the
clean-up: Taubin iterations that take the grid-scale ripple off the surface and leave `faces` as they are.  `simplify=` then runs
neuman_hip.mesh_simplify (simplify_mesh; csrc/mesh_simplify.hip, the header's 'mesh simplify', rules Q1-Q9): the vertices of every grid cell
of that edge become one, placed by the quadrics of the faces around them, so that binding, posing and drawing pay for the detail one wants.

The step after `clean_mesh` is neuman_hip.mesh_pose: `bind_mesh` binds the canonical mesh to the body, `pose_mesh` / `pose_mesh_frames` pose it
for the frames of a sequence (csrc/mesh_pose.hip; the header's 'mesh pose', rules P1-P6)."""
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


class Components:
    """What `components` returns, every tensor on the mesh's device: vert_label [V] int32 (-1: no face names the vertex), face_label [F]
    int32, n (the number of components, a Python int), n_verts [n] and n_faces [n] int32, box [n,6] float32 (lo xyz, hi xyz) or None."""
    __slots__ = ('vert_label', 'face_label', 'n', 'n_verts', 'n_faces', 'box')

    def __init__(self, vert_label, face_label, n, n_verts, n_faces, box):
        self.vert_label, self.face_label, self.n, self.n_verts, self.n_faces, self.box = vert_label, face_label, n, n_verts, n_faces, box


def _mesh_faces(faces, who):
    if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
        raise _lib.NeumanHipError(f"{who}: faces must be a CUDA (HIP) tensor: there is no CPU path")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise _lib.NeumanHipError(f"{who}: faces must be int32 [F, 3], got {faces.dtype} {tuple(faces.shape)}")
    return faces.detach().contiguous()


def _vertex_rows(a, n_verts, dev, who, name):
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise _lib.NeumanHipError(f"{who}: {name} must be a CUDA (HIP) tensor: there is no CPU path")
    if a.dim() != 2 or a.shape[0] != n_verts or a.shape[1] < 1 or a.dtype != torch.float32 or a.device != dev:
        raise _lib.NeumanHipError(f"{who}: {name} must be float32 [{n_verts}, w] on {dev}, got {a.dtype} {tuple(a.shape)} on {a.device}")
    return a.detach().contiguous()


def _workspace(L, n_verts, n_faces, dev):
    nbytes = int(L.nm_mesh_components_workspace_bytes(n_verts, n_faces))
    if nbytes < 0:
        _lib.check(nbytes, "nm_mesh_components_workspace_bytes")
    return torch.empty((nbytes,), device=dev, dtype=torch.uint8), nbytes


def components(faces, n_verts, verts=None):
    """The connected components of the mesh faces [F,3] (CUDA int32) over n_verts vertices (rules C1-C4: two vertices are connected if a
    face names both; ids in ascending order of the components' smallest vertex) -> Components.  verts [n_verts,3] (CUDA float32) adds the
    components' boxes.  One read-back, for n; a face that names a vertex outside [0, n_verts) raises NeumanHipError."""
    faces = _mesh_faces(faces, "components")
    n_verts, n_faces = int(n_verts), int(faces.shape[0])
    dev = faces.device
    if verts is not None:
        verts = _vertex_rows(verts, n_verts, dev, "components", "verts")
        if verts.shape[1] != 3:
            raise _lib.NeumanHipError(f"components: verts must be [V, 3], got {tuple(verts.shape)}")
    L = _lib.lib()
    I32 = torch.int32
    with torch.cuda.device(dev):
        ws, nbytes = _workspace(L, n_verts, n_faces, dev)
        vert_label = torch.empty((n_verts,), device=dev, dtype=I32)
        face_label = torch.empty((n_faces,), device=dev, dtype=I32)
        n = ctypes.c_int64(0)
        _lib.check(L.nm_mesh_components(_lib.dev_ptr(faces, I32), n_faces, n_verts, _lib.dev_ptr(vert_label, I32), _lib.dev_ptr(face_label, I32),
                                        _lib.dev_ptr(ws, torch.uint8), nbytes, ctypes.byref(n), _lib.stream_ptr()), "nm_mesh_components")
        C = int(n.value)
        comp_verts = torch.empty((C,), device=dev, dtype=I32)
        comp_faces = torch.empty((C,), device=dev, dtype=I32)
        box = None if verts is None else torch.empty((C, 6), device=dev, dtype=torch.float32)
        _lib.check(L.nm_mesh_component_stats(_lib.dev_ptr(faces, I32), n_faces, n_verts, _lib.dev_ptr(vert_label, I32), _lib.dev_ptr(verts), C,
                                             _lib.dev_ptr(comp_verts, I32), _lib.dev_ptr(comp_faces, I32), _lib.dev_ptr(box), _lib.stream_ptr()),
                   "nm_mesh_component_stats")
    return Components(vert_label, face_label, C, comp_verts, comp_faces, box)


def select_components(verts, faces, comps, keep, *attrs):
    """The mesh (verts [V,3], faces [F,3]) compacted to the components of `comps` (what `components` returned for it) with keep[c] set
    (rule C5; keep: bool or uint8 CUDA tensor [comps.n]) -> (verts', faces', *attrs'): kept vertices and faces in their old order, face
    indices remapped; verts and every attribute (float32 [V, w], any width) gathered by nm_gather_rows.  One read-back, for the sizes."""
    faces = _mesh_faces(faces, "select_components")
    dev = faces.device
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise _lib.NeumanHipError("select_components: verts must be a CUDA (HIP) tensor: there is no CPU path")
    n_verts, n_faces = int(verts.shape[0]), int(faces.shape[0])
    rows = [_vertex_rows(a, n_verts, dev, "select_components", "verts" if i == 0 else f"attribute {i - 1}") for i, a in enumerate((verts,) + attrs)]
    if not isinstance(keep, torch.Tensor) or not keep.is_cuda or keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (comps.n,):
        raise _lib.NeumanHipError(f"select_components: keep must be a bool or uint8 CUDA tensor [{comps.n}]")
    if tuple(comps.vert_label.shape) != (n_verts,):
        raise _lib.NeumanHipError(f"select_components: comps labels {comps.vert_label.shape[0]} vertices, the mesh has {n_verts}")
    keep = keep.to(torch.uint8).contiguous()
    label = comps.vert_label.contiguous()
    L = _lib.lib()
    I32, U8 = torch.int32, torch.uint8
    with torch.cuda.device(dev):
        ws, nbytes = _workspace(L, n_verts, n_faces, dev)
        nv, nf = ctypes.c_int64(0), ctypes.c_int64(0)
        mesh = (_lib.dev_ptr(faces, I32), n_faces, n_verts, _lib.dev_ptr(label, I32), _lib.dev_ptr(keep, U8), comps.n, _lib.dev_ptr(ws, U8), nbytes)
        _lib.check(L.nm_mesh_select_count(*mesh, ctypes.byref(nv), ctypes.byref(nf), _lib.stream_ptr()), "nm_mesh_select_count")
        nv, nf = int(nv.value), int(nf.value)
        vert_src = torch.empty((nv,), device=dev, dtype=I32)
        faces_out = torch.empty((nf, 3), device=dev, dtype=I32)
        _lib.check(L.nm_mesh_select_fill(*mesh, _lib.dev_ptr(vert_src, I32), _lib.dev_ptr(faces_out, I32), nv, nf, _lib.stream_ptr()),
                   "nm_mesh_select_fill")
        out = []
        for a in rows:
            g = torch.empty((nv, a.shape[1]), device=dev, dtype=torch.float32)
            _lib.check(L.nm_gather_rows(_lib.dev_ptr(a), _lib.dev_ptr(vert_src, I32), None, nv, int(a.shape[1]), _lib.dev_ptr(g), _lib.stream_ptr()),
                       "nm_gather_rows")
            out.append(g)
    return (out[0], faces_out, *out[1:])


def _check_clean(largest, min_faces):
    if largest is not None and (isinstance(largest, bool) or not isinstance(largest, (int, np.integer)) or largest < 1):
        raise ValueError(f"largest must be None (no limit) or an int >= 1, got {largest!r}")
    if isinstance(min_faces, bool) or not isinstance(min_faces, (int, np.integer)) or min_faces < 0:
        raise ValueError(f"min_faces must be an int >= 0, got {min_faces!r}")


def keep_mask(n_faces, largest=1, min_faces=0):
    """clean_mesh's choice as a uint8 mask [C] from the components' face counts n_faces [C] (CUDA int32), computed on the device: the
    components of at least min_faces faces, and among those the `largest` biggest by face count (None: all), ties to the lower id."""
    _check_clean(largest, min_faces)
    enough = n_faces >= int(min_faces)
    if largest is None:
        return enough.to(torch.uint8)
    order = torch.sort(torch.where(enough, n_faces, torch.full_like(n_faces, -1)), descending=True, stable=True).indices
    keep = torch.zeros_like(enough)
    keep[order[:int(largest)]] = True
    return (keep & enough).to(torch.uint8)


def clean_mesh(verts, faces, *attrs, largest=1, min_faces=0):
    """Drop the floaters: keep the components with at least min_faces faces, and among those the `largest` biggest by face count (ties to
    the lower id; None: all of them) -> (verts', faces', *attrs') as select_components.  The default keeps the one largest component;
    largest=None, min_faces=0 returns the input mesh as it is.  Two read-backs: the number of components and the output's sizes."""
    _check_clean(largest, min_faces)
    if largest is None and min_faces == 0:
        return (verts, faces, *attrs)
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise _lib.NeumanHipError("clean_mesh: verts must be a CUDA (HIP) tensor: there is no CPU path")
    comps = components(faces, verts.shape[0])
    return select_components(verts, faces, comps, keep_mask(comps.n_faces, largest, min_faces), *attrs)


def extract_net_mesh(net, aabb, res, level, colour=True, precision=None, slab_bytes=SLAB_BYTES, largest=None, min_faces=0, smooth=0, simplify=0.0):
    """density_grid + extract_mesh on a static net (a background Joiner, or HumanNeRF.coarse_human_net with the box of
    occupancy.canonical_aabb) -> (verts, faces, normals, colours).  colour: per-vertex RGB [Nv,3] in [0, 1], the sigmoid of the net's own
    forward at the vertices seen along -normal (from outside, head on); the plain head takes no view.  Otherwise colours is None.
    largest / min_faces: clean_mesh's, run on (verts, faces, normals) before the colours, which are then evaluated at kept vertices only;
    the defaults keep everything.  smooth = n > 0: after the clean-up, n Taubin iterations of mesh_smooth.smooth_mesh on the vertices (faces
    unchanged) and the normals replaced by mesh_smooth.vertex_normals of the smoothed mesh; the colours are then evaluated at the smoothed
    vertices along the new normals.  smooth = 0 changes nothing.  simplify = h > 0: after the smoothing, mesh_simplify.simplify_mesh with
    cells of edge h on the grid of `aabb` (quadric placement) and the normals replaced by mesh_smooth.vertex_normals of the simplified mesh;
    the colours are then evaluated at the new vertices along them.  simplify = 0 changes nothing."""
    _check_clean(largest, min_faces)
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or smooth < 0:
        raise ValueError(f"smooth must be an int >= 0 (Taubin iterations), got {smooth!r}")
    if isinstance(simplify, bool) or not isinstance(simplify, (int, float, np.integer, np.floating)) or not np.isfinite(simplify) or simplify < 0:
        raise ValueError(f"simplify must be a finite cell edge >= 0 (0: no simplification), got {simplify!r}")
    field = density_grid(net, aabb, res, precision=precision, slab_bytes=slab_bytes)
    verts, faces, normals = extract_mesh(field, aabb, level)
    if largest is not None or min_faces != 0:
        verts, faces, normals = clean_mesh(verts, faces, normals, largest=largest, min_faces=min_faces)
    if smooth > 0:
        from . import mesh_smooth                                  # (it imports this module)
        adj = mesh_smooth.adjacency(faces, verts.shape[0])
        verts = mesh_smooth.smooth_mesh(verts, faces, int(smooth), adj=adj)
        normals = mesh_smooth.vertex_normals(verts, faces, adj=adj)
    if simplify > 0:
        from . import mesh_simplify, mesh_smooth                   # (they import this module)
        verts, faces = mesh_simplify.simplify_mesh(verts, faces, float(simplify), aabb=aabb)
        normals = mesh_smooth.vertex_normals(verts, faces)
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
