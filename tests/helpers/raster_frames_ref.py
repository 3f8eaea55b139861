"""Rules F2-F5 of include/neuman_hip.h 'mesh frames' in numpy on top of raster_ref.rasterize (rules 1-3), parametrised by dtype as raster_ref
is: the float64 run is the yardstick of tests/test_hip_raster_frames.py, the float32 run calibrates its tolerances.  One frame at a time: the
batch is a loop here.

Below the rules, the scenes the GPU test renders (`SCENES`, `scene()`), built in numpy alone so that tests/test_raster_frames_host.py can check
on the CPU that the float64 run calls at most 1 % of their covered pixels ambiguous."""
import numpy as np

import raster_ref as RR

LIGHT = RR.LIGHT


def _blend(b, a, fw):
    """(b0' a0 + b1' a1) + b2' a2 for per-vertex rows a [V,3], winning faces fw [n,3], barycentrics b [n,3]"""
    return (b[:, 0:1] * a[fw[:, 0]] + b[:, 1:2] * a[fw[:, 1]]) + b[:, 2:3] * a[fw[:, 2]]


def render(verts, faces, camera, dtype=np.float64, colours=None, normals=None, light=LIGHT, bg=None, bg_z=None, analyse=False):
    """One frame -> raster_ref.rasterize's dict plus colour [H,W,3] (F2, F3; ones where nothing covers), show [H,W] bool (F4) and out [H,W,3]
    uint8 (F5).  verts, normals [V,3] float32, colours [V,3] float32, bg [H,W,3] uint8, bg_z [H,W] float32."""
    T = np.dtype(dtype).type
    r = RR.rasterize(verts, faces, camera, dtype, analyse=analyse)
    faces = np.asarray(faces)[:, :3].astype(np.int64)
    H, W = r['face_id'].shape
    cov = r['face_id'] >= 0
    fw, b = faces[r['face_id'][cov]], r['bary'][cov].astype(T)
    c = np.ones((int(cov.sum()), 3), T)
    with np.errstate(all='ignore'):
        if colours is not None:
            c = _blend(b, np.asarray(colours).astype(T), fw)                                         # F2
        if normals is not None:                                                                      # F3
            n = RR._normalize(_blend(b, np.asarray(normals).astype(T), fw), T)
            p = _blend(b, np.asarray(verts).astype(T), fw)
            l = RR._normalize(np.asarray(light, np.float64).astype(T)[None] - p, T)
            nl = (n[:, 0] * l[:, 0] + n[:, 1] * l[:, 1]) + n[:, 2] * l[:, 2]
            c = c * (T(0.5) + T(0.5) * np.maximum(nl, T(0)))[:, None]
        colour = np.ones((H, W, 3), T)
        colour[cov] = c
        show = cov.copy()
        if bg_z is not None:
            show &= r['zbuf'] < np.asarray(bg_z).astype(T)                                           # F4: strict, false for a NaN
        x = colour * T(255)
        byte = np.clip(np.where(np.isnan(x), T(0), x), 0, 255).astype(np.uint8)                      # F5: truncation, a NaN gives 0
    back = np.full((H, W, 3), 255, np.uint8) if bg is None else np.asarray(bg)
    r.update(colour=colour, show=show, out=np.where(show[..., None], byte, back))
    return r


def colour_tolerance(r64, r32, ok):
    """The device's allowance on the colour before it becomes a byte, as raster_ref.tolerances has it: 4 x the float32 run's worst deviation from
    the float64 run over the pixels `ok` where both picked the same face, with a floor of 1e-6 of the largest colour there -> (tol, deviation)"""
    same = ok & (r64['face_id'] == r32['face_id']) & (r64['face_id'] >= 0)
    a, b = r64['colour'][same].astype(np.float64), r32['colour'][same].astype(np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    dev = float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
    return max(4.0 * dev, 1e-6 * (float(np.abs(a[fin]).max()) if fin.any() else 1.0)), dev


def byte_range(colour, tol):
    """the bytes F5 makes of any colour within tol of `colour` (float64): lowest and highest, [..] uint8 each; a NaN gives 0"""
    nan = np.isnan(colour)
    c = np.where(nan, 0.0, colour)
    lo = np.clip(np.floor((c - tol) * 255.0), 0, 255)
    hi = np.clip(np.floor((c + tol) * 255.0), 0, 255)
    return np.where(nan, 0, lo).astype(np.uint8), np.where(nan, 0, hi).astype(np.uint8)


# ---- the scenes of tests/test_hip_raster_frames.py ---------------------------------------------------------------------------------------
CAMERAS = ((30., -20., 1.3), (75., 10., 1.6), (-40., 35., 1.45))          # spherical_c2w arguments: three different views of the capsule
SCENES = {                                                                 # capsule_mesh arguments, W, H, cameras (indices into CAMERAS)
    'three_frames_96x64': ((40, 38), 96, 64, (0, 1, 2)),                   # 3040 faces
    'ragged_50x37': ((40, 38), 50, 37, (0, 1)),                            # neither side a multiple of the tile
    'past_the_scan_240x240': ((20, 18), 240, 240, (0, 1, 2, 0, 1)),        # 5 x 225 (frame, tile) pairs: more than the scan's 1024 threads
    'one_tile_16x16': ((40, 38), 16, 16, (0, 2)),                          # every face in one tile's list: 12 LDS batches
}


def scene(name):
    """-> dict(verts [B,V,3] float32 (frame b the capsule moved and turned a little, so no two frames share vertices), faces [F,3], normals
    [B,V,3] float32 unit, colours [V,3] float32 in [0, 1], caps (synthetic.SimpleCapture per frame), W, H)"""
    from neuman_hip import synthetic
    shape, W, H, cams = SCENES[name]
    base, faces = synthetic.capsule_mesh(*shape)
    rng = np.random.default_rng(len(name))
    colours = rng.random((len(base), 3)).astype(np.float32)
    verts, normals, caps = [], [], []
    for b, ci in enumerate(cams):
        ang = 0.15 * b
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.]])
        v = (base.astype(np.float64) @ R.T + [0.02 * b, -0.01 * b, 0.015 * b]).astype(np.float32)
        verts.append(v)
        normals.append(RR.vertex_normals(v, faces).astype(np.float32))
        caps.append(synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(*CAMERAS[ci])))
    return dict(verts=np.stack(verts), faces=faces, normals=np.stack(normals), colours=colours, caps=caps, W=W, H=H)
