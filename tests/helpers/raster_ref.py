"""The mesh rasteriser's contract (include/neuman_hip.h 'mesh rasteriser', rules 1-5) in numpy, parametrised by dtype: the float64 run is
the yardstick of tests/test_hip_raster.py, the float32 run calibrates its tolerances.  pytorch3d, which the reference's overlay_smpl
(utils/render_utils.py:464-501) sits on, is absent, so no golden of the reference's own exists; this file states what the device must compute.

Brute force over faces: every face is evaluated at every pixel of its screen bounding box grown by a margin (`brute=True`: at every pixel
of the image; tests/test_raster_host.py checks that the two agree).  Nothing here bins, tiles or orders the faces."""
import numpy as np

LIGHT = (2.0, 2.0, -2.0)
NORM_EPS = 1e-6
AMBIGUOUS_BARY = 1e-4          # a face whose smallest screen barycentric is this close to zero ...
AMBIGUOUS_BEHIND = 1e-3        # ... and whose depth is not more than 0.1 % behind the winner's
AMBIGUOUS_DEPTH = 1e-4         # the two nearest covering depths closer than this, relative


def camera_of(cap):
    """(w2c f64 [3,4], fx, fy, cx, cy, W, H) of a synthetic.SimpleCapture"""
    K = np.asarray(cap.intrinsic_matrix, np.float64)
    H, W = cap.shape
    return np.linalg.inv(np.asarray(cap.cam_pose.camera_to_world, np.float64))[:3, :4], K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H


def _normalize(x, T):
    n = np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])
    return x / np.maximum(n, T(NORM_EPS))[..., None]


def vertex_normals(verts, faces, T=np.float64):
    """rule 4: normalize(sum over incident faces of cross(v1 - v0, v2 - v0)), summed in face order"""
    v = verts.astype(T)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]).astype(T)
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    return _normalize(n, T)


def rasterize(verts, faces, camera, dtype=np.float64, light=LIGHT, brute=False, analyse=False, margin=1.0):
    """-> dict(face_id [H,W] int32 (-1), zbuf [H,W] (+inf), bary [H,W,3] (0), rgba [H,W,4] ((1,1,1,0)), and with analyse=True
    ambiguous [H,W] bool plus counts).  verts [V,3] float32, faces [F,3] int, camera as camera_of()."""
    T = np.dtype(dtype).type
    w2c, fx, fy, cx, cy, W, H = camera
    faces = np.asarray(faces)[:, :3].astype(np.int64)
    F = faces.shape[0]
    v = np.asarray(verts).astype(T)
    R, t = np.asarray(w2c)[:, :3].astype(T), np.asarray(w2c)[:, 3].astype(T)
    with np.errstate(all='ignore'):
        xc = ((R[0, 0] * v[:, 0] + R[0, 1] * v[:, 1]) + R[0, 2] * v[:, 2]) + t[0]                   # rule 1
        yc = ((R[1, 0] * v[:, 0] + R[1, 1] * v[:, 1]) + R[1, 2] * v[:, 2]) + t[1]
        zc = ((R[2, 0] * v[:, 0] + R[2, 1] * v[:, 1]) + R[2, 2] * v[:, 2]) + t[2]
        sx = T(fx) * xc / zc + T(cx)
        sy = T(fy) * yc / zc + T(cy)
        iz = T(1) / zc
        X, Y, Z, IZ = sx[faces], sy[faces], zc[faces], iz[faces]                                    # [F,3]
        area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
        valid = (Z > 0).all(1) & (area != 0) & np.isfinite(X).all(1) & np.isfinite(Y).all(1)        # rule 2: dropped whole / zero area
        # candidate (face, pixel) pairs
        if brute:
            c0, c1 = np.zeros(F, np.int64), np.full(F, W - 1, np.int64)
            r0, r1 = np.zeros(F, np.int64), np.full(F, H - 1, np.int64)
        else:
            lim = 1 << 40
            c0 = np.clip(np.floor(np.where(valid, X.min(1), 0) - 0.5 - margin), 0, lim).astype(np.int64)
            c1 = np.clip(np.ceil(np.where(valid, X.max(1), -1) - 0.5 + margin), -1, W - 1).astype(np.int64)
            r0 = np.clip(np.floor(np.where(valid, Y.min(1), 0) - 0.5 - margin), 0, lim).astype(np.int64)
            r1 = np.clip(np.ceil(np.where(valid, Y.max(1), -1) - 0.5 + margin), -1, H - 1).astype(np.int64)
        nx, ny = np.maximum(c1 - c0 + 1, 0), np.maximum(r1 - r0 + 1, 0)
        n = np.where(valid, nx * ny, 0)
        pf = np.repeat(np.arange(F), n)                                                             # the pair's face
        local = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
        col, row = c0[pf] + local % np.maximum(nx[pf], 1), r0[pf] + local // np.maximum(nx[pf], 1)
        px, py = (col.astype(T) + T(0.5)), (row.astype(T) + T(0.5))
        ax, ay, bx, by, cx_, cy_ = X[pf, 0] - px, Y[pf, 0] - py, X[pf, 1] - px, Y[pf, 1] - py, X[pf, 2] - px, Y[pf, 2] - py
        w0 = bx * cy_ - by * cx_                                                                    # the edge functions on translated vertices
        w1 = cx_ * ay - cy_ * ax
        w2 = ax * by - ay * bx
        s = (w0 + w1) + w2
        inside = ((s > 0) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((s < 0) & (w0 <= 0) & (w1 <= 0) & (w2 <= 0))
        q0, q1, q2 = w0 * IZ[pf, 0], w1 * IZ[pf, 1], w2 * IZ[pf, 2]
        q = (q0 + q1) + q2
        z = s / q                                                                                   # rule 3
        pix = row * W + col
        # the winner: nearest z, lower face index on a tie
        k = np.flatnonzero(inside)
        order = k[np.lexsort((pf[k], z[k], pix[k]))]
        first = np.ones(order.size, bool)
        first[1:] = pix[order][1:] != pix[order][:-1]
        win = order[first]
        face_id = np.full(H * W, -1, np.int32)
        zbuf = np.full(H * W, np.inf, T)
        bary = np.zeros((H * W, 3), T)
        face_id[pix[win]] = pf[win]
        zbuf[pix[win]] = z[win]
        bary[pix[win]] = np.stack([q0[win] / q[win], q1[win] / q[win], q2[win] / q[win]], 1)
        # rule 4
        rgba = np.tile(np.array([1, 1, 1, 0], T), (H * W, 1))
        cov = pix[win]
        if cov.size:
            vn = vertex_normals(verts, faces, T)
            fw, b = faces[pf[win]], bary[cov]
            nrm = (b[:, 0:1] * vn[fw[:, 0]] + b[:, 1:2] * vn[fw[:, 1]]) + b[:, 2:3] * vn[fw[:, 2]]
            pos = (b[:, 0:1] * v[fw[:, 0]] + b[:, 1:2] * v[fw[:, 1]]) + b[:, 2:3] * v[fw[:, 2]]
            nrm = _normalize(nrm, T)
            centre = -(np.asarray(w2c, np.float64)[:, :3].T @ np.asarray(w2c, np.float64)[:, 3])
            l = _normalize(np.asarray(light, np.float64).astype(T)[None] - pos, T)
            wv = _normalize(centre.astype(T)[None] - pos, T)
            nl = (nrm[:, 0] * l[:, 0] + nrm[:, 1] * l[:, 1]) + nrm[:, 2] * l[:, 2]
            refl = (T(2) * nl)[:, None] * nrm - l
            a = np.maximum((refl[:, 0] * wv[:, 0] + refl[:, 1] * wv[:, 1]) + refl[:, 2] * wv[:, 2], T(0))
            for _ in range(6):
                a = a * a                                                                           # ^64
            colour = (T(0.5) + T(0.3) * np.maximum(nl, T(0))) + np.where(nl > 0, T(0.2) * a, T(0))
            rgba[cov] = np.stack([colour, colour, colour, np.ones_like(colour)], 1)
        out = dict(face_id=face_id.reshape(H, W), zbuf=zbuf.reshape(H, W), bary=bary.reshape(H, W, 3), rgba=rgba.reshape(H, W, 4))
        if analyse:
            bmin = np.minimum(np.minimum(w0 / s, w1 / s), w2 / s)                                   # the smallest screen-space barycentric
            zwin = zbuf[pix]
            near_edge = (np.abs(bmin) < AMBIGUOUS_BARY) & ~(z > zwin * (1 + AMBIGUOUS_BEHIND))
            amb = np.zeros(H * W, bool)
            amb[pix[near_edge]] = True
            second = order[1:][~first[1:]]                                                          # pairs that are not their pixel's nearest ...
            prev = order[:-1][~first[1:]]
            is_second = first[:-1][~first[1:]]                                                      # ... and directly follow it
            close = is_second & ((z[second] - z[prev]) < AMBIGUOUS_DEPTH * z[prev])
            amb[pix[second[close]]] = True
            out.update(ambiguous=amb.reshape(H, W), n_pairs=int(pf.size), n_valid_faces=int(valid.sum()))
    return out


def overlay(rgba, image):
    """rule 5: covered pixels take uint8(colour * 255), truncated; the others keep the image's byte"""
    byte = np.clip(rgba[..., :3] * rgba.dtype.type(255), 0, 255).astype(np.uint8)
    return np.where(rgba[..., 3:4] > 0, byte, image)


def tolerances(ref64, ref32, ok):
    """The device's allowance per quantity: 4 x the float32 run's own worst deviation from the float64 run over the pixels `ok` (where the
    two runs picked the same face), with a floor of 1e-6 of the quantity's largest magnitude there.  -> ({name: tol}, {name: float32 deviation})"""
    same = ok & (ref64['face_id'] == ref32['face_id']) & (ref64['face_id'] >= 0)
    tol, dev = {}, {}
    for name in ('zbuf', 'bary', 'rgba'):
        a, b = ref64[name][same].astype(np.float64), ref32[name][same].astype(np.float64)
        dev[name] = float(np.abs(a - b).max()) if a.size else 0.0
        tol[name] = max(4.0 * dev[name], 1e-6 * (float(np.abs(a).max()) if a.size else 1.0))
    return tol, dev
