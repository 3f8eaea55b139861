"""Rules M1-M3 and F2'' of include/neuman_hip.h 'mesh mip' in numpy, on top of mesh_lattice_ref (rules L1-L3), which stays as it is.  The pyramid
is float32 alone: nm_mesh_lattice_pyramid must give its bits.  `shade` is parametrised by dtype as mesh_lattice_ref.shade is: the float64 run is
the yardstick of the rendered bytes in tests/test_hip_mesh_mip.py, the float32 run calibrates their tolerance and is the device's arithmetic
for the level (screen vertices projected in float64 and rounded to float32, as the device's vertex pass makes them, then float32 throughout).

Below the rules, the scene of the quality test: mesh_lattice_ref's thinned striped capsule with a wavelength of half a mean edge, drawn from so far
that a wavelength is 1.25 pixels, and the box-filtered truth of a 4 x supersampled frame."""
import numpy as np

import mesh_lattice_ref as LR
import raster_frames_ref as FR


# ---- M1 --------------------------------------------------------------------------------------------------------------------------------------
def lattice_levels(R0):
    """1 + the trailing zero bits of R0"""
    n = 1
    while R0 % 2 == 0:
        R0, n = R0 // 2, n + 1
    return n


def nodes_before(R0, l):
    """S(R0 >> k) summed over the levels k < l: where level l's block starts, in nodes per face"""
    return sum(LR.lattice_size(R0 >> k) for k in range(l))


def reduce(fine):
    """one level: fine [F,S(2R),w] float32 -> coarse [F,S(R),w] float32"""
    fine = np.asarray(fine)
    assert fine.dtype == np.float32
    Rf = next(R for R in range(2, 65, 2) if LR.lattice_size(R) == fine.shape[1])
    R = Rf // 2
    i1, i2 = LR.nodes(R)
    i0 = R - i1 - i2
    j1, j2 = 2 * i1, 2 * i2
    at = lambda a1, a2: fine[:, LR.node_index(Rf, np.clip(a1, 0, Rf), np.clip(a2, 0, Rf - np.clip(a1, 0, Rf)))]      # noqa: E731  (clipped: unused where out of range)
    h, q, e = np.float32(0.5), np.float32(0.25), np.float32(0.125)
    zeros = (i0 == 0).astype(int) + (i1 == 0) + (i2 == 0)
    c = at(j1, j2)
    with np.errstate(all='ignore'):
        # an edge node's two fine neighbours along its edge: the smaller i1 first, on the edge i1 = 0 the smaller i2
        a = np.where((i1 == 0)[None, :, None], at(0 * j1, j2 - 1), np.where((i2 == 0)[None, :, None], at(j1 - 1, 0 * j2), at(j1 - 1, j2 + 1)))
        b = np.where((i1 == 0)[None, :, None], at(0 * j1, j2 + 1), np.where((i2 == 0)[None, :, None], at(j1 + 1, 0 * j2), at(j1 + 1, j2 - 1)))
        edge = h * c + q * (a + b)
        n = [at(j1 + d1, j2 + d2) for d1, d2 in ((1, 0), (0, 1), (-1, 1), (-1, 0), (0, -1), (1, -1))]
        inner = q * c + e * (((((n[0] + n[1]) + n[2]) + n[3]) + n[4]) + n[5])
    out = np.where((zeros >= 2)[None, :, None], c, np.where((zeros == 1)[None, :, None], edge, inner))
    return np.ascontiguousarray(out, np.float32)


def pyramid(lattice, levels=None):
    """-> the list of the levels' arrays [F,S(R0 >> l),w] float32; level 0 is the input"""
    lat = np.asarray(lattice)
    R0 = next(R for R in range(1, 65) if LR.lattice_size(R) == lat.shape[1])
    levels = lattice_levels(R0) if levels is None else levels
    assert 1 <= levels <= lattice_levels(R0)
    out = [lat]
    for _ in range(levels - 1):
        out.append(reduce(out[-1]))
    return out


def flat(levels):
    """the pyramid as the device lays it out: one float32 vector, level-major"""
    return np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in levels])


# ---- M2 --------------------------------------------------------------------------------------------------------------------------------------
def screen_vertices(verts, camera, dtype=np.float32):
    """rule 1's (u, v) per vertex [V,2]: float64 arithmetic, rounded to `dtype` at the end as the device's vertex pass rounds to float32"""
    w2c, fx, fy, cx, cy, _, _ = camera
    v = np.asarray(verts).astype(np.float64)
    M = np.asarray(w2c, np.float64)
    xc = ((M[0, 0] * v[:, 0] + M[0, 1] * v[:, 1]) + M[0, 2] * v[:, 2]) + M[0, 3]
    yc = ((M[1, 0] * v[:, 0] + M[1, 1] * v[:, 1]) + M[1, 2] * v[:, 2]) + M[1, 3]
    zc = ((M[2, 0] * v[:, 0] + M[2, 1] * v[:, 1]) + M[2, 2] * v[:, 2]) + M[2, 3]
    with np.errstate(all='ignore'):
        iz = 1.0 / zc
        return np.stack([fx * xc * iz + cx, fy * yc * iz + cy], 1).astype(dtype)


def level_of(sv, faces, face, R0, levels, lod_scale, dtype=np.float32):
    """rule M2 for the winning faces `face` [n] -> (l [n] int, t [n] `dtype`, rho [n] `dtype` BEFORE the halvings)"""
    T = np.dtype(dtype).type
    f = np.asarray(faces, np.int64)[np.asarray(face, np.int64)]
    p0, p1, p2 = (np.asarray(sv).astype(T)[f[:, k]] for k in range(3))
    with np.errstate(all='ignore'):
        d01, d02, d12 = p1 - p0, p2 - p0, p2 - p1
        sq = lambda d: d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]                                      # noqa: E731
        e2 = np.fmax(np.fmax(sq(d01), sq(d02)), sq(d12))
        cr = np.abs(d01[:, 0] * d02[:, 1] - d01[:, 1] * d02[:, 0])
        rho0 = ((T(lod_scale) * T(R0)) * np.sqrt(e2)) / cr
        rho = rho0.copy()
        l = np.zeros(rho.shape, np.int64)
        for _ in range(levels - 1):
            go = (rho >= T(2)) & (l < levels - 1)                                                # false for a NaN
            rho = np.where(go, rho * T(0.5), rho)
            l = l + go
        t = np.where(l < levels - 1, np.fmin(np.fmax(rho - T(1), T(0)), T(1)), T(0))            # fmax, fmin: a NaN gives the other operand
    return l, t.astype(T), rho0.astype(T)


def near_power_of_two(rho, rel=1e-5):
    """rho within `rel` relative of a power of two (>= 2): where sqrtf and the division's last bit can move the level"""
    r = np.asarray(rho).astype(np.float64)
    with np.errstate(all='ignore'):
        k = np.round(np.log2(np.where(np.isfinite(r) & (r > 0), r, 1.0)))
        return np.isfinite(r) & (r > 0) & (k >= 1) & (np.abs(r - 2.0 ** k) <= rel * 2.0 ** k)


# ---- M3, F2'' ----------------------------------------------------------------------------------------------------------------------------------
def shade(fr, levels_list, R0, lod_scale, sv, faces, dtype=np.float64, lit=True, bg=None):
    """mesh_lattice_ref.shade with rule F2'': `fr` is mesh_lattice_ref.frame's dict (made with `dtype` and the same bg), levels_list what
    `pyramid` returns, sv `screen_vertices` -> a new dict with 'colour', 'out', and per pixel 'level' (-1 where nothing covers), 't', 'rho'"""
    T = np.dtype(dtype).type
    cov = fr['face_id'] >= 0
    H, W = cov.shape
    face = fr['face_id'][cov]
    b = fr['bary'][cov].astype(T)
    l, t, rho = level_of(sv, faces, face, R0, len(levels_list), lod_scale, dtype)
    c = np.zeros((face.size, 3), T)
    with np.errstate(all='ignore'):
        for k in range(len(levels_list)):
            at = l == k
            if at.any():
                c[at] = LR.lookup(levels_list[k], face[at], R0 >> k, b[at, 1], b[at, 2], dtype)[0]
            two = at & (t > 0)
            if two.any():
                d = LR.lookup(levels_list[k + 1], face[two], R0 >> (k + 1), b[two, 1], b[two, 2], dtype)[0]
                c[two] = c[two] + t[two][:, None] * (d - c[two])
        if lit:
            c = c * fr['colour'][cov][:, :1].astype(T)
        colour = np.ones((H, W, 3), T)
        colour[cov] = c
        x = colour * T(255)
        byte = np.clip(np.where(np.isnan(x), T(0), x), 0, 255).astype(np.uint8)                  # F5
    back = np.full((H, W, 3), 255, np.uint8) if bg is None else np.asarray(bg)
    level = np.full((H, W), -1, np.int64)
    level[cov] = l
    tt, rr = np.zeros((H, W), T), np.zeros((H, W), T)
    tt[cov], rr[cov] = t, rho
    out = dict(fr)
    out.update(colour=colour, out=np.where(fr['show'][..., None], byte, back), level=level, t=tt, rho=rr)
    return out


# ---- the quality test's scene ------------------------------------------------------------------------------------------------------------------
STRIPE_PIXELS = 1.25                                                       # a wavelength on the screen, at the image centre's depth
SUPER = 4                                                                  # the truth's sub-samples per pixel side


def stripe_wavelength(verts, faces):
    """four node spacings of an R = 8 lattice: half a mean edge"""
    return 0.5 * LR.mean_edge(verts, faces)


def far_cameras(wavelength, scale=1):
    """mesh_lattice_ref's three views from so far that `wavelength` is STRIPE_PIXELS pixels at the origin's depth; scale = SUPER: the same
    views at SUPER times the image size, whose pixel (SUPER x + i, SUPER y + j) is sub-sample (i, j) of pixel (x, y)"""
    from neuman_hip import synthetic
    W, H = LR.STRIPE_IMAGE
    fx = 1.25 * W
    dist = fx * wavelength / STRIPE_PIXELS
    assert 1.0 <= wavelength * fx / dist <= 1.5
    return [synthetic.SimpleCapture(scale * W, scale * H, c2w=synthetic.spherical_c2w(c[0], c[1], dist)) for c in FR.CAMERAS]


def box_truth(face_id, bary, verts, faces, wavelength):
    """face_id [SUPER H, SUPER W] and bary [.., 3] of a supersampled frame -> (truth [H,W,3] float64: the source at every sub-sample's surface
    point, averaged per pixel; full [H,W] bool: all SUPER^2 sub-samples of the pixel are covered)"""
    fr = dict(face_id=np.asarray(face_id), bary=np.asarray(bary))
    cov = fr['face_id'] >= 0
    value = np.zeros(cov.shape + (3,))
    value[cov] = LR.stripes(LR.surface_points(fr, verts, faces), wavelength)
    Hs, Ws = cov.shape
    blocks = lambda a: a.reshape(Hs // SUPER, SUPER, Ws // SUPER, SUPER, *a.shape[2:])            # noqa: E731
    return blocks(value).mean(axis=(1, 3)), blocks(cov).all(axis=(1, 3))


def mean_abs_error(out, truth, full):
    """-> (sum of |byte / 255 - truth| over the pixels `full`, number of values)"""
    got = np.asarray(out)[full].astype(np.float64) / 255.0
    return float(np.abs(got - truth[full]).sum()), int(got.size)
