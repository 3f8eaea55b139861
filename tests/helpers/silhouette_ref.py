"""The soft silhouette's contract (include/neuman_hip.h 'soft silhouette', rules S1-S5 on the rasteriser's rules 1-2) in torch on the CPU,
parametrised by dtype: the float64 run is the yardstick of tests/test_hip_silhouette.py, the float32 run calibrates its tolerances.
pytorch3d, which the reference's silhouette (preprocess/optimize_smpl.py:84-102) sits on, is absent, so no golden of the reference's own
exists; this file states what the device must compute.

Brute force over faces, in chunks: every face is evaluated at every pixel of its screen bounding box grown by the blur radius plus a margin
(`brute=True`: at every pixel of the image; tests/test_silhouette_host.py checks that the two agree).  Nothing here bins, tiles or orders
the faces.  The values are torch expressions of `verts`, so gradients come from torch's autograd and not from a formula written here: a
first pass without a graph finds the candidate (face, pixel) pairs of rule S2, which rule S5 treats as constants, and a second pass evaluates
S1 and S3 on those pairs under autograd."""
import math

import numpy as np
import torch

from raster_ref import camera_of  # noqa: F401  (the camera of a synthetic.SimpleCapture, as the rasteriser's helper reads it)

SIGMA = 1e-4
AMBIGUOUS_CUT = 1e-5           # a non-inside face whose m is this close, relative, to blur_radius: the candidate cut
AMBIGUOUS_KINK = 1e-5          # an inside candidate whose two smallest edge distances are this close, relative: the kink of the min ...
AMBIGUOUS_WEIGHT = 1e-12       # ... if its p (1 - p) is above this (elsewhere the kink carries no weight)
PAIRS_PER_CHUNK = 1 << 22


def default_blur_radius(sigma=SIGMA):
    return math.log(1.0 / 1e-4 - 1.0) * sigma


def _segment(ax, ay, bx, by):
    """S1 for one edge a -> b, both relative to the pixel centre: the squared distance from the centre to the segment"""
    ex, ey = bx - ax, by - ay
    t = torch.clamp(-(ax * ex + ay * ey) / (ex * ex + ey * ey), 0, 1)
    qx, qy = ax + t * ex, ay + t * ey
    return qx * qx + qy * qy


def _pairs(sx, sy, faces, pf, col, row, s2):
    """S1 on (face, pixel) pairs: inside [n] bool, the three edges' squared distances [3,n] in NDC units"""
    T = sx.dtype
    px, py = col.to(T) + 0.5, row.to(T) + 0.5
    i0, i1, i2 = faces[pf, 0], faces[pf, 1], faces[pf, 2]
    ax, ay, bx, by, cx, cy = sx[i0] - px, sy[i0] - py, sx[i1] - px, sy[i1] - py, sx[i2] - px, sy[i2] - py
    w0 = bx * cy - by * cx                                                                          # the rasteriser's edge functions
    w1 = cx * ay - cy * ax
    w2 = ax * by - ay * bx
    s = (w0 + w1) + w2
    inside = ((s > 0) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((s < 0) & (w0 <= 0) & (w1 <= 0) & (w2 <= 0))
    m = torch.stack([_segment(ax, ay, bx, by), _segment(bx, by, cx, cy), _segment(cx, cy, ax, ay)]) * s2
    return inside, m


def _project(verts, camera, T):
    """rule 1 in dtype T -> screen x, y [V] and the camera depth [V]; a vertex at z <= 0 gets a harmless position (its faces are dropped)"""
    w2c = torch.as_tensor(np.asarray(camera[0], np.float64)).to(T)
    fx, fy, cx, cy = (torch.tensor(float(a), dtype=T) for a in camera[1:5])
    v = verts.to(T)
    xc = ((w2c[0, 0] * v[:, 0] + w2c[0, 1] * v[:, 1]) + w2c[0, 2] * v[:, 2]) + w2c[0, 3]
    yc = ((w2c[1, 0] * v[:, 0] + w2c[1, 1] * v[:, 1]) + w2c[1, 2] * v[:, 2]) + w2c[1, 3]
    zc = ((w2c[2, 0] * v[:, 0] + w2c[2, 1] * v[:, 1]) + w2c[2, 2] * v[:, 2]) + w2c[2, 3]
    zs = torch.where(zc > 0, zc, torch.ones_like(zc))
    return fx * xc / zs + cx, fy * yc / zs + cy, zc


def silhouette(verts, faces, camera, sigma=SIGMA, blur_radius=None, dtype=torch.float64, brute=False, analyse=False, margin=1.0):
    """-> dict(alpha [H,W], keep [H,W]: torch tensors of `dtype`, functions of `verts` under autograd when it requires a gradient;
    n_cand [H,W] int32 numpy; n_pairs; and with analyse=True ambiguous [H,W] bool numpy).
    verts [V,3] numpy float32 or a torch tensor, faces [F,3] int, camera as camera_of()."""
    T = dtype
    W, H = int(camera[5]), int(camera[6])
    blur_radius = default_blur_radius(sigma) if blur_radius is None else blur_radius
    verts = torch.as_tensor(verts)
    faces = torch.as_tensor(np.asarray(faces)[:, :3].astype(np.int64))
    F = faces.shape[0]
    ndc = 2.0 / min(W, H)
    s2, blur, sig = torch.tensor(ndc * ndc, dtype=T), torch.tensor(float(blur_radius), dtype=T), torch.tensor(float(sigma), dtype=T)
    reach = math.sqrt(blur_radius) / ndc + margin                                                   # R_px and the margin, in pixels
    sx, sy, zc = _project(verts, camera, T)
    keep_pf, keep_pix, keep_in = [], [], []
    amb = np.zeros(H * W, bool)
    n_pairs = 0
    with torch.no_grad():
        X, Y, Z = sx[faces].numpy().astype(np.float64), sy[faces].numpy().astype(np.float64), zc[faces].numpy()
        area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        valid = (Z > 0).all(1) & (area != 0) & np.isfinite(X).all(1) & np.isfinite(Y).all(1)       # rule 2: dropped whole / zero area
        if brute:
            c0, c1 = np.zeros(F, np.int64), np.full(F, W - 1, np.int64)
            r0, r1 = np.zeros(F, np.int64), np.full(F, H - 1, np.int64)
        else:
            lim = 1 << 40
            c0 = np.clip(np.floor(np.where(valid, X.min(1), 0) - 0.5 - reach), 0, lim).astype(np.int64)
            c1 = np.clip(np.ceil(np.where(valid, X.max(1), -1) - 0.5 + reach), -1, W - 1).astype(np.int64)
            r0 = np.clip(np.floor(np.where(valid, Y.min(1), 0) - 0.5 - reach), 0, lim).astype(np.int64)
            r1 = np.clip(np.ceil(np.where(valid, Y.max(1), -1) - 0.5 + reach), -1, H - 1).astype(np.int64)
        nx, ny = np.maximum(c1 - c0 + 1, 0), np.maximum(r1 - r0 + 1, 0)
        n = np.where(valid, nx * ny, 0)
        ends = np.cumsum(n)
        lo = 0
        while lo < F:                                                                               # chunks of whole faces
            hi = max(int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + PAIRS_PER_CHUNK, side='right')), lo + 1)
            nc = n[lo:hi]
            pf = np.repeat(np.arange(lo, hi), nc)
            if pf.size:
                local = np.arange(pf.size) - np.repeat(np.cumsum(nc) - nc, nc)
                col, row = c0[pf] + local % np.maximum(nx[pf], 1), r0[pf] + local // np.maximum(nx[pf], 1)
                pft, colt, rowt = torch.from_numpy(pf), torch.from_numpy(col), torch.from_numpy(row)
                inside, m3 = _pairs(sx, sy, faces, pft, colt, rowt, s2)
                m = m3.min(0).values
                cand = inside | (m < blur)                                                          # S2
                pix = row * W + col
                keep_pf.append(pft[cand])
                keep_pix.append(torch.from_numpy(pix)[cand])
                keep_in.append(inside[cand])
                n_pairs += int(pf.size)
                if analyse:
                    near_cut = (~inside & ((m - blur).abs() <= AMBIGUOUS_CUT * blur)).numpy()
                    q = torch.sigmoid(torch.where(inside, -m, m) / sig)
                    two = m3.sort(0).values
                    kink = (inside & (q * (1 - q) > AMBIGUOUS_WEIGHT) & ((two[1] - two[0]) <= AMBIGUOUS_KINK * two[1])).numpy()
                    amb[pix[near_cut | kink]] = True
            lo = hi
    pf = torch.cat(keep_pf) if keep_pf else torch.zeros(0, dtype=torch.int64)
    pix = torch.cat(keep_pix) if keep_pix else torch.zeros(0, dtype=torch.int64)
    inside = torch.cat(keep_in) if keep_in else torch.zeros(0, dtype=torch.bool)
    # the differentiable pass, on the candidates alone
    _, m3 = _pairs(sx, sy, faces, pf, pix % W, pix // W, s2)
    m = torch.minimum(torch.minimum(m3[0], m3[1]), m3[2])
    q = torch.sigmoid(torch.where(inside, -m, m) / sig)                                             # S3: 1 / (1 + exp(-d / sigma))
    keep = torch.ones(H * W, dtype=T).scatter_reduce(0, pix, q, 'prod', include_self=True)
    out = dict(alpha=(1 - keep).reshape(H, W), keep=keep.reshape(H, W), n_pairs=n_pairs,
               n_cand=np.bincount(pix.numpy(), minlength=H * W).astype(np.int32).reshape(H, W))
    if analyse:
        out['ambiguous'] = amb.reshape(H, W)
    return out


def gradient(verts, faces, camera, g_alpha, sigma=SIGMA, blur_radius=None, dtype=torch.float64, brute=False):
    """d sum(g_alpha * alpha) / d verts by autograd -> numpy [V,3] float64"""
    v = torch.as_tensor(verts).detach().clone().requires_grad_(True)
    out = silhouette(v, faces, camera, sigma, blur_radius, dtype, brute=brute)
    (out['alpha'] * torch.as_tensor(np.asarray(g_alpha)).to(dtype)).sum().backward()
    return v.grad.double().numpy()


def tolerance(ref64, ref32, ok=None, relative=False):
    """The device's allowance for one quantity: 4 x the float32 run's own worst deviation from the float64 run (over `ok`, if given), with
    a floor of 1e-6 -- of the quantity's largest magnitude when `relative` (gradients).  -> (tol, the float32 run's deviation)"""
    a, b = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    if ok is not None:
        a, b = a[ok], b[ok]
    dev = float(np.abs(a - b).max()) if a.size else 0.0
    scale = (float(np.abs(a).max()) if a.size else 1.0) if relative else 1.0
    return max(4.0 * dev, 1e-6 * scale), dev
