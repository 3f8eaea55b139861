"""The mesh rasteriser's handle (csrc/raster.hip, include/neuman_hip.h 'mesh rasteriser'): one `Rasterizer` per topology holds the
faces, the vertex -> face table of the normals and the passes' scratch on the device; `rasterizer_for(faces, V)` keeps the last few.

The camera of a capture is read here too: intrinsics from `cap.pinhole_cam` (the reference's captures) or `cap.intrinsic_matrix`
(synthetic.SimpleCapture), the world-to-camera matrix from `cap.cam_pose` in float64.

The soft silhouette (csrc/silhouette.hip, the header's 'soft silhouette') works on the same handle: `Rasterizer.silhouette` and
`silhouette_backward` are the two entries, `soft_silhouette` joins them under torch's autograd.

`Rasterizer.render_frames` (csrc/raster_frames.hip, the header's 'mesh frames') renders B frames of the mesh as uint8 images in one call:
the rasteriser's geometry per frame, per-vertex colours, a diffuse light on supplied normals, a depth test against a background."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib

LIGHT = (2.0, 2.0, -2.0)                                           # PointLights(location=...) of render_utils.py:469
SIGMA = 1e-4                                                       # BlendParams(sigma=1e-4) of preprocess/optimize_smpl.py:89


def default_blur_radius(sigma=SIGMA):
    """preprocess/optimize_smpl.py:92: the squared NDC distance at which a face's probability has fallen to 1e-4"""
    return math.log(1.0 / 1e-4 - 1.0) * sigma


def camera_of(cap):
    """(w2c f64 [3,4], fx, fy, cx, cy, W, H) of a capture."""
    cam = getattr(cap, 'pinhole_cam', None)
    if cam is not None:
        fx, fy, cx, cy, W, H = cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height
    else:
        K = np.asarray(cap.intrinsic_matrix, np.float64)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        H, W = cap.shape
    pose = cap.cam_pose
    if hasattr(pose, 'rotation_matrix') and hasattr(pose, 'translation_vector'):
        w2c = np.concatenate([np.asarray(pose.rotation_matrix, np.float64)[:3, :3], np.asarray(pose.translation_vector, np.float64).reshape(3, 1)], 1)
    else:
        w2c = np.linalg.inv(np.asarray(pose.camera_to_world, np.float64))[:3, :4]
    return np.ascontiguousarray(w2c), float(fx), float(fy), float(cx), float(cy), int(W), int(H)


def _f64(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class Rasterizer:
    """nm_raster_create over faces [F,3] (numpy or tensor, any integer type) of a mesh with V vertices."""

    def __init__(self, faces, V):
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        self.faces = np.ascontiguousarray(np.asarray(faces)[:, :3], np.int32)
        self.F, self.V = int(self.faces.shape[0]), int(V)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().nm_raster_create(self.faces.ctypes.data_as(ctypes.c_void_p), self.F, self.V, ctypes.byref(h)), "nm_raster_create")
        self._h = h

    def close(self):
        if getattr(self, '_h', None):
            _lib.lib().nm_raster_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _verts(self, verts):
        if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
            raise _lib.NeumanHipError("verts must be a CUDA (HIP) tensor: the rasteriser has no CPU path")
        verts = verts.detach().to(torch.float32).contiguous()
        if verts.shape != (self.V, 3):
            raise _lib.NeumanHipError(f"verts {tuple(verts.shape)} is not [{self.V}, 3]")
        return verts

    def rasterize(self, verts, camera, want_bary=True, shade=False, light=LIGHT):
        """-> (face_id [H,W] int32, zbuf [H,W] f32, bary [H,W,3] f32 or None, rgba [H,W,4] f32 or None) on verts' device."""
        verts = self._verts(verts)
        w2c, fx, fy, cx, cy, W, H = camera
        if W < 1 or H < 1:
            raise _lib.NeumanHipError(f"rasterize: empty image {W} x {H}")
        dev = verts.device
        with torch.cuda.device(dev):
            face_id = torch.empty((H, W), device=dev, dtype=torch.int32)
            zbuf = torch.empty((H, W), device=dev, dtype=torch.float32)
            bary = torch.empty((H, W, 3), device=dev, dtype=torch.float32) if want_bary else None
            w2c, w2c_p = _f64(w2c)
            if shade:
                rgba = torch.empty((H, W, 4), device=dev, dtype=torch.float32)
                light, light_p = _f64(light)
                _lib.check(_lib.lib().nm_raster_phong(self._h, _lib.dev_ptr(verts), w2c_p, fx, fy, cx, cy, W, H, _lib.dev_ptr(face_id, torch.int32),
                                                      _lib.dev_ptr(zbuf), _lib.dev_ptr(bary), light_p, _lib.dev_ptr(rgba), _lib.stream_ptr()), "nm_raster_phong")
            else:
                rgba = None
                _lib.check(_lib.lib().nm_raster_mesh(self._h, _lib.dev_ptr(verts), w2c_p, fx, fy, cx, cy, W, H, _lib.dev_ptr(face_id, torch.int32),
                                                     _lib.dev_ptr(zbuf), _lib.dev_ptr(bary), _lib.stream_ptr()), "nm_raster_mesh")
        return face_id, zbuf, bary, rgba

    def silhouette(self, verts, camera, sigma=SIGMA, blur_radius=None, want_count=False):
        """nm_raster_silhouette -> (alpha [H,W] f32, keep [H,W] f32 = 1 - alpha as the product left it, n_cand [H,W] int32 or None) on verts'
        device; no graph is recorded (`soft_silhouette` is the differentiable form)."""
        verts = self._verts(verts)
        w2c, fx, fy, cx, cy, W, H = camera
        if W < 1 or H < 1:
            raise _lib.NeumanHipError(f"silhouette: empty image {W} x {H}")
        blur_radius = default_blur_radius(sigma) if blur_radius is None else blur_radius
        dev = verts.device
        with torch.cuda.device(dev):
            alpha = torch.empty((H, W), device=dev, dtype=torch.float32)
            keep = torch.empty((H, W), device=dev, dtype=torch.float32)
            n_cand = torch.empty((H, W), device=dev, dtype=torch.int32) if want_count else None
            w2c, w2c_p = _f64(w2c)
            _lib.check(_lib.lib().nm_raster_silhouette(self._h, _lib.dev_ptr(verts), w2c_p, fx, fy, cx, cy, W, H, float(sigma), float(blur_radius), _lib.dev_ptr(alpha),
                                                       _lib.dev_ptr(keep), _lib.dev_ptr(n_cand, torch.int32), _lib.stream_ptr()), "nm_raster_silhouette")
        return alpha, keep, n_cand

    def silhouette_backward(self, verts, camera, sigma, blur_radius, keep, g_alpha):
        """nm_raster_silhouette_backward: keep [H,W] of `silhouette` on the same arguments, g_alpha [H,W] = d loss / d alpha -> g_verts [V,3] f32"""
        verts = self._verts(verts)
        w2c, fx, fy, cx, cy, W, H = camera
        keep, g_alpha = keep.detach().to(torch.float32).contiguous(), g_alpha.detach().to(torch.float32).contiguous()
        if tuple(keep.shape) != (H, W) or tuple(g_alpha.shape) != (H, W) or keep.device != verts.device or g_alpha.device != verts.device:
            raise _lib.NeumanHipError(f"silhouette_backward: keep {tuple(keep.shape)} and g_alpha {tuple(g_alpha.shape)} must be [{H}, {W}] on {verts.device}")
        with torch.cuda.device(verts.device):
            g_verts = torch.empty((self.V, 3), device=verts.device, dtype=torch.float32)
            w2c, w2c_p = _f64(w2c)
            _lib.check(_lib.lib().nm_raster_silhouette_backward(self._h, _lib.dev_ptr(verts), w2c_p, fx, fy, cx, cy, W, H, float(sigma), float(blur_radius),
                                                                _lib.dev_ptr(keep), _lib.dev_ptr(g_alpha), _lib.dev_ptr(g_verts), _lib.stream_ptr()),
                       "nm_raster_silhouette_backward")
        return g_verts


    def _batch(self, verts, cameras, who):
        """verts [B,V,3] on the device, cameras = (w2c [B,4,4] f64, intr [B,4] f64 (fx, fy, cx, cy), W, H), both on verts' device"""
        if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
            raise _lib.NeumanHipError("verts must be a CUDA (HIP) tensor: the rasteriser has no CPU path")
        verts = verts.detach().to(torch.float32).contiguous()
        w2c, intr, W, H = cameras
        B = verts.shape[0] if verts.dim() == 3 else -1
        if B < 1 or tuple(verts.shape) != (B, self.V, 3) or tuple(w2c.shape) != (B, 4, 4) or tuple(intr.shape) != (B, 4):
            raise _lib.NeumanHipError(f"{who}: verts {tuple(verts.shape)} must be [B >= 1, {self.V}, 3], w2c {tuple(w2c.shape)} [B, 4, 4], intr {tuple(intr.shape)} [B, 4]")
        if W < 1 or H < 1:
            raise _lib.NeumanHipError(f"{who}: empty image {W} x {H}")
        return verts, w2c.contiguous(), intr.contiguous(), B, int(W), int(H)

    def silhouette_batch(self, verts, cameras, sigma=SIGMA, blur_radius=None, want_count=False):
        """nm_raster_silhouette_batch: B frames as one call -> (alpha [B,H,W], keep [B,H,W], n_cand [B,H,W] int32 or None); frame b's are the
        bits `silhouette` gives on frame b.  `cameras` as `batch_cameras` makes them.  One host read per call."""
        verts, w2c, intr, B, W, H = self._batch(verts, cameras, "silhouette_batch")
        blur_radius = default_blur_radius(sigma) if blur_radius is None else blur_radius
        dev = verts.device
        with torch.cuda.device(dev):
            alpha = torch.empty((B, H, W), device=dev, dtype=torch.float32)
            keep = torch.empty((B, H, W), device=dev, dtype=torch.float32)
            n_cand = torch.empty((B, H, W), device=dev, dtype=torch.int32) if want_count else None
            _lib.check(_lib.lib().nm_raster_silhouette_batch(self._h, _lib.dev_ptr(verts), _lib.dev_ptr(w2c, torch.float64), _lib.dev_ptr(intr, torch.float64), B,
                                                             W, H, float(sigma), float(blur_radius), _lib.dev_ptr(alpha), _lib.dev_ptr(keep),
                                                             _lib.dev_ptr(n_cand, torch.int32), _lib.stream_ptr()), "nm_raster_silhouette_batch")
        return alpha, keep, n_cand

    def silhouette_backward_batch(self, verts, cameras, sigma, blur_radius, keep, g_alpha):
        """nm_raster_silhouette_backward_batch: keep [B,H,W] of `silhouette_batch`, g_alpha [B,H,W] -> g_verts [B,V,3] f32; no host read"""
        verts, w2c, intr, B, W, H = self._batch(verts, cameras, "silhouette_backward_batch")
        keep, g_alpha = keep.detach().to(torch.float32).contiguous(), g_alpha.detach().to(torch.float32).contiguous()
        if tuple(keep.shape) != (B, H, W) or tuple(g_alpha.shape) != (B, H, W) or keep.device != verts.device or g_alpha.device != verts.device:
            raise _lib.NeumanHipError(f"silhouette_backward_batch: keep {tuple(keep.shape)} and g_alpha {tuple(g_alpha.shape)} must be [{B}, {H}, {W}] on {verts.device}")
        with torch.cuda.device(verts.device):
            g_verts = torch.empty((B, self.V, 3), device=verts.device, dtype=torch.float32)
            _lib.check(_lib.lib().nm_raster_silhouette_backward_batch(self._h, _lib.dev_ptr(verts), _lib.dev_ptr(w2c, torch.float64),
                                                                      _lib.dev_ptr(intr, torch.float64), B, W, H, float(sigma), float(blur_radius),
                                                                      _lib.dev_ptr(keep), _lib.dev_ptr(g_alpha), _lib.dev_ptr(g_verts), _lib.stream_ptr()),
                       "nm_raster_silhouette_backward_batch")
        return g_verts

    def render_frames(self, verts, cameras, colours=None, normals=None, light=LIGHT, background=None, background_z=None, want_geometry=False, out=None, *,
                      face_colours=None, lod_scale=None):
        """nm_raster_frames (the header's 'mesh frames', rules F1-F7): B frames of the mesh as images, one call and one host read -> out uint8
        [B,H,W,3], or (out, face_id [B,H,W] int32, zbuf [B,H,W] f32, bary [B,H,W,3] f32) with want_geometry; frame b's geometry is the bits
        `rasterize` gives on frame b.  verts [B,V,3]; `cameras` as `batch_cameras` makes them; colours [V,3] f32 (None: white); normals
        [B,V,3] f32 switch the diffuse light at `light` on; background uint8 [B,H,W,3] (None: white); background_z f32 [B,H,W], camera-space
        depth the mesh must be nearer than.  `out`: a dense uint8 [B,H,W,3] tensor on verts' device to write into instead of a new one.
        face_colours [F,S,3] f32, a colour lattice as `mesh_texture.bake_face_colours` makes it, in place of `colours` (ValueError for both):
        nm_raster_frames_lattice (the header's 'mesh lattice', rule F2'), the resolution recovered from S; the geometry is the same bits.
        face_colours a `mesh_texture.LatticePyramid`: nm_raster_frames_lattice_mip (the header's 'mesh mip', rule F2''), which filters under
        minification: a level per frame and face from the face's size on the screen, two levels blended.  lod_scale (default 1.0; finite,
        >= 0) scales the nodes-per-pixel figure the level comes from: 0 is the plain lattice, larger is blurrier.  lod_scale without a
        pyramid is a ValueError."""
        who = "render_frames"
        if colours is not None and face_colours is not None:
            raise ValueError(f"{who}: give colours (one per vertex) or face_colours (a lattice per face), not both")
        pyramid, face_colours = pyramid_of(face_colours, lod_scale, self.F, who)
        verts, w2c, intr, B, W, H = self._batch(verts, cameras, who)
        dev = verts.device
        R = None if face_colours is None else pyramid.R if pyramid is not None else lattice_resolution_of(face_colours, self.F, who)

        def dense(t, name, dtype, shape):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise _lib.NeumanHipError(f"{who}: {name} must be a CUDA (HIP) tensor: there is no CPU path")
            if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev:
                raise _lib.NeumanHipError(f"{who}: {name} must be {dtype} {list(shape)} on {dev}, got {t.dtype} {list(t.shape)} on {t.device}")
            return t.detach().contiguous()

        colours = dense(colours, "colours", torch.float32, (self.V, 3))
        face_colours = dense(face_colours, "face_colours", torch.float32, tuple(getattr(face_colours, 'shape', ())))
        normals = dense(normals, "normals", torch.float32, (B, self.V, 3))
        background = dense(background, "background", torch.uint8, (B, H, W, 3))
        background_z = dense(background_z, "background_z", torch.float32, (B, H, W))
        if out is not None:
            dense(out, "out", torch.uint8, (B, H, W, 3))
            if not out.is_contiguous():
                raise _lib.NeumanHipError(f"{who}: out must be contiguous")
        light_p = _f64(light)[1] if normals is not None else None
        with torch.cuda.device(dev):
            if out is None:
                out = torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8)
            face_id = torch.empty((B, H, W), device=dev, dtype=torch.int32) if want_geometry else None
            zbuf = torch.empty((B, H, W), device=dev, dtype=torch.float32) if want_geometry else None
            bary = torch.empty((B, H, W, 3), device=dev, dtype=torch.float32) if want_geometry else None
            head = (self._h, _lib.dev_ptr(verts), _lib.dev_ptr(w2c, torch.float64), _lib.dev_ptr(intr, torch.float64), B, W, H)
            tail = (_lib.dev_ptr(normals), light_p, _lib.dev_ptr(background, torch.uint8), _lib.dev_ptr(background_z), _lib.dev_ptr(out, torch.uint8),
                    _lib.dev_ptr(face_id, torch.int32), _lib.dev_ptr(zbuf), _lib.dev_ptr(bary), _lib.stream_ptr())
            if face_colours is None:
                _lib.check(_lib.lib().nm_raster_frames(*head, _lib.dev_ptr(colours), *tail), "nm_raster_frames")
            elif pyramid is not None:
                _lib.check(_lib.lib().nm_raster_frames_lattice_mip(*head, _lib.dev_ptr(face_colours), R, pyramid.levels, 1.0 if lod_scale is None else lod_scale,
                                                                   *tail), "nm_raster_frames_lattice_mip")
            else:
                _lib.check(_lib.lib().nm_raster_frames_lattice(*head, _lib.dev_ptr(face_colours), R, *tail), "nm_raster_frames_lattice")
        return (out, face_id, zbuf, bary) if want_geometry else out


def pyramid_of(face_colours, lod_scale, n_faces, who):
    """-> (the `mesh_texture.LatticePyramid` or None, the tensor the entry reads: the pyramid's flat buffer, or face_colours as it came).
    ValueError for a lod_scale without a pyramid or one that is no number; NeumanHipError for a pyramid of another mesh or not of colours"""
    from .mesh_texture import LatticePyramid
    if not isinstance(face_colours, LatticePyramid):
        if lod_scale is not None:
            raise ValueError(f"{who}: lod_scale goes with a LatticePyramid (mesh_texture.lattice_pyramid), not with "
                             f"{'a plain lattice' if face_colours is not None else 'no face_colours'}")
        return None, face_colours
    if lod_scale is not None and (isinstance(lod_scale, bool) or not isinstance(lod_scale, (int, float, np.integer, np.floating))):
        raise ValueError(f"{who}: lod_scale must be a number, got {lod_scale!r}")
    if face_colours.F != n_faces or face_colours.w != 3:
        raise _lib.NeumanHipError(f"{who}: face_colours must be the pyramid of a [{n_faces}, S, 3] lattice, got one of a [{face_colours.F}, S, {face_colours.w}] lattice")
    return face_colours, face_colours.data


def lattice_resolution_of(face_colours, n_faces, who):
    """R of a colour lattice [F,S,3] with S = (R+1)(R+2)/2 nodes per face (the header's 'mesh lattice', rule L1), 1 <= R <= 64; NeumanHipError
    for any other shape"""
    shape = tuple(getattr(face_colours, 'shape', ()))
    if len(shape) == 3 and shape[0] == n_faces and shape[2] == 3:
        R = (math.isqrt(8 * int(shape[1]) + 1) - 3) // 2
        if 1 <= R <= 64 and (R + 1) * (R + 2) // 2 == shape[1]:
            return R
    raise _lib.NeumanHipError(f"{who}: face_colours must be [{n_faces}, S, 3] with S = (R+1)(R+2)/2 nodes for a resolution 1 <= R <= 64, got {list(shape)}")


def batch_cameras(caps, device):
    """The cameras of captures of ONE image size as the batched entries read them: (w2c [B,4,4] f64, intr [B,4] f64 (fx, fy, cx, cy), W, H),
    the two arrays on `device` (one upload each).  Captures of differing (W, H) raise ValueError: the caller groups them."""
    cams = [camera_of(c) for c in caps]
    if not cams:
        raise ValueError("batch_cameras: no captures")
    sizes = sorted({(c[5], c[6]) for c in cams})
    if len(sizes) != 1:
        raise ValueError(f"the captures of a batch must share one image size, got (W, H) = {sizes}: group them by size")
    w2c = np.tile(np.eye(4), (len(cams), 1, 1))
    w2c[:, :3] = np.stack([c[0] for c in cams])
    intr = np.array([c[1:5] for c in cams], np.float64)
    return torch.from_numpy(w2c).to(device), torch.from_numpy(intr).to(device), sizes[0][0], sizes[0][1]


class _SilhouetteBatchFn(torch.autograd.Function):
    """alpha [B,H,W] as a function of verts [B,V,3]: the two batched entries of csrc/silhouette.hip; keep is what the forward saved"""

    @staticmethod
    def forward(ctx, verts, rast, cameras, sigma, blur_radius):
        alpha, keep, _ = rast.silhouette_batch(verts, cameras, sigma, blur_radius)
        ctx.rast, ctx.cameras, ctx.sigma, ctx.blur_radius = rast, cameras, sigma, blur_radius
        ctx.save_for_backward(verts.detach(), keep)
        return alpha

    @staticmethod
    def backward(ctx, g_alpha):
        verts, keep = ctx.saved_tensors
        g = ctx.rast.silhouette_backward_batch(verts, ctx.cameras, ctx.sigma, ctx.blur_radius, keep, g_alpha)
        return g.to(verts.dtype), None, None, None, None


def soft_silhouette_batch(rast, verts, cameras, sigma=SIGMA, blur_radius=None):
    """alpha [B,H,W] f32, differentiable with respect to verts [B,V,3] (a CUDA tensor); `cameras` from `batch_cameras`"""
    rast._batch(verts, cameras, "soft_silhouette_batch")           # (refuses a CPU tensor or a wrong shape before autograd sees it)
    return _SilhouetteBatchFn.apply(verts, rast, cameras, float(sigma), float(default_blur_radius(sigma) if blur_radius is None else blur_radius))


class _SilhouetteFn(torch.autograd.Function):
    """alpha [H,W] of the soft silhouette as a function of verts [V,3]: the two entries of csrc/silhouette.hip.  The backward recomputes the
    candidates from verts; keep is what the forward saved (rule S5)."""

    @staticmethod
    def forward(ctx, verts, rast, camera, sigma, blur_radius):
        alpha, keep, _ = rast.silhouette(verts, camera, sigma, blur_radius)
        ctx.rast, ctx.camera, ctx.sigma, ctx.blur_radius = rast, camera, sigma, blur_radius
        ctx.save_for_backward(verts.detach(), keep)
        return alpha

    @staticmethod
    def backward(ctx, g_alpha):
        verts, keep = ctx.saved_tensors
        g = ctx.rast.silhouette_backward(verts, ctx.camera, ctx.sigma, ctx.blur_radius, keep, g_alpha)
        return g.to(verts.dtype), None, None, None, None


def soft_silhouette(rast, verts, camera, sigma=SIGMA, blur_radius=None):
    """alpha [H,W] f32, differentiable with respect to verts [V,3] (a CUDA tensor)"""
    rast._verts(verts)                                             # (refuses a CPU tensor or a wrong shape before autograd sees it)
    return _SilhouetteFn.apply(verts, rast, camera, float(sigma), float(default_blur_radius(sigma) if blur_radius is None else blur_radius))


_CACHE = collections.OrderedDict()
_CACHE_SIZE = 4


def rasterizer_for(faces, V):
    """The handle of this topology, built on first use (a trainer overlays the same body every validation)."""
    if isinstance(faces, torch.Tensor):
        faces = faces.detach().cpu().numpy()
    faces = np.ascontiguousarray(np.asarray(faces)[:, :3], np.int32)
    key = (int(V), faces.shape[0], hash(faces.tobytes()))
    r = _CACHE.get(key)
    if r is None or not np.array_equal(r.faces, faces):
        r = _CACHE[key] = Rasterizer(faces, V)
        while len(_CACHE) > _CACHE_SIZE:
            _CACHE.popitem(last=False)[1].close()
    _CACHE.move_to_end(key)
    return r


def overlay_rgba(rgba, image):
    """Rule 5: rgba [H,W,4] f32 (device) over image [H,W,3] uint8 (device) -> uint8 [H,W,3] (device)."""
    if image.dtype != torch.uint8 or image.shape != (*rgba.shape[:2], 3):
        raise _lib.NeumanHipError(f"overlay: the image must be uint8 [{rgba.shape[0]}, {rgba.shape[1]}, 3], got {image.dtype} {tuple(image.shape)}")
    image = image.contiguous()
    out = torch.empty_like(image)
    with torch.cuda.device(rgba.device):
        _lib.check(_lib.lib().nm_overlay_rgba8(_lib.dev_ptr(rgba), _lib.dev_ptr(image, torch.uint8), _lib.dev_ptr(out, torch.uint8), rgba.shape[0] * rgba.shape[1],
                                               _lib.stream_ptr()), "nm_overlay_rgba8")
    return out
