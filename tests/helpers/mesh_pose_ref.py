"""Numpy restatement of the 'mesh pose' contract of include/neuman_hip.h (rules P2-P5): float64 elementwise operations in the stated
association, one astype(np.float32) at the end.  numpy's float64 multiply, add, subtract, divide and sqrt are IEEE operations rounded one
by one (nothing here is a dot product or a sum() that numpy could reorder or fuse), which is what the device does with contraction off.

    pose(T, tri, bary, pts, normals=None) -> (out_pts [B,N,3] f32, out_normals [B,N,3] f32 or None, n_invalid)

T [B,rows,4,4] float64 or float32; tri / bary [N,3] or [B,N,3] (a binding per frame); pts / normals [N,3] float32."""
import numpy as np


def _cross(a, b):
    """rule P4's cross(a, b) on [..., 3] float64: each component two products and one subtraction"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def pose(T, tri, bary, pts, normals=None):
    T = np.asarray(T)
    assert T.ndim == 4 and T.shape[2:] == (4, 4) and T.dtype in (np.float64, np.float32)
    B, rows = T.shape[:2]
    tri, bary = np.asarray(tri), np.asarray(bary)
    pts = np.asarray(pts)
    assert tri.dtype == np.int32 and bary.dtype == np.float32 and pts.dtype == np.float32
    N = pts.shape[0]
    if tri.ndim == 2:
        tri, bary = np.broadcast_to(tri, (B, N, 3)), np.broadcast_to(bary, (B, N, 3))
    assert tri.shape == bary.shape == (B, N, 3)
    bad = ((tri < 0) | (tri >= rows)).any(-1)                                      # rule P5: [B,N]
    safe = np.where(bad[..., None], 0, tri).astype(np.int64)                       # never dereferenced: row 0 stands in, overwritten below
    T64 = T.astype(np.float64)                                                     # exact
    frame = np.arange(B)[:, None]
    w = bary.astype(np.float64)
    t0, t1, t2 = (T64[frame, safe[..., k]] for k in range(3))                      # [B,N,4,4]
    w0, w1, w2 = (w[..., k, None, None] for k in range(3))
    M = (w0 * t0 + w1 * t1) + w2 * t2                                              # rule P2
    p = pts.astype(np.float64)
    x, y, z = p[None, :, 0, None], p[None, :, 1, None], p[None, :, 2, None]        # [1,N,1] against M[..., :3, c] [B,N,3]
    out = ((M[..., :3, 0] * x + M[..., :3, 1] * y) + M[..., :3, 2] * z) + M[..., :3, 3]      # rule P3
    out_pts = out.astype(np.float32)
    out_pts[bad] = np.nan
    out_normals = None
    if normals is not None:
        normals = np.asarray(normals)
        assert normals.dtype == np.float32 and normals.shape == (N, 3)
        n = normals.astype(np.float64)
        n0, n1, n2 = n[None, :, 0, None], n[None, :, 1, None], n[None, :, 2, None]
        A = M[..., :3, :3]
        C = np.stack([_cross(A[..., 1, :], A[..., 2, :]), _cross(A[..., 2, :], A[..., 0, :]), _cross(A[..., 0, :], A[..., 1, :])], -2)      # rule P4
        q = (C[..., 0] * n0 + C[..., 1] * n1) + C[..., 2] * n2
        s = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        with np.errstate(all='ignore'):
            unit = q / np.sqrt(s)[..., None]
        usable = (s != 0) & np.isfinite(s)
        out_normals = np.where(usable[..., None], unit, 0.0).astype(np.float32)
        out_normals[bad] = np.nan
    return out_pts, out_normals, int(bad.sum())


def ulp_distance(a, b):
    """per element, how many float32 steps apart a and b are (0 for equal bits and for two NaNs; a NaN against a number: a huge count)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)                               # -0 and +0 coincide
    d = np.abs(ordered(a) - ordered(b))
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, 1 << 40, d))
