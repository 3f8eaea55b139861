"""Rules L1-L3 and F2' of include/neuman_hip.h 'mesh lattice' in numpy, parametrised by dtype as raster_frames_ref.render is: the float32 run
is what nm_mesh_lattice_rows must give bit for bit, the float64 run is the yardstick of the rendered bytes in tests/test_hip_mesh_lattice.py and
the float32 run calibrates their tolerance.  Built on raster_ref and raster_frames_ref, which stay as they are: `render` takes their frame
(geometry, F3's shade, F4, the background) and replaces the colour by L3's.

Below the rules, the scene of the quality test (`stripe_scene`): a thinned capsule, a striped colour source and three cameras, built in numpy
alone so that tests/test_mesh_lattice_host.py can state the test's condition on the CPU."""
import numpy as np

import raster_frames_ref as FR
import raster_ref as RR


# ---- L1 --------------------------------------------------------------------------------------------------------------------------------------
def lattice_size(R):
    return (R + 1) * (R + 2) // 2


def node_index(R, i1, i2):
    """where node (i1, i2) is stored: rows by i2, row i2 has R + 1 - i2 entries"""
    return i2 * (R + 1) - i2 * (i2 - 1) // 2 + i1


def nodes(R):
    """-> (i1 [S], i2 [S]) int64 in storage order"""
    i2 = np.repeat(np.arange(R + 1), R + 1 - np.arange(R + 1))
    i1 = np.arange(lattice_size(R)) - node_index(R, 0, i2)
    return i1, i2


# ---- L2 --------------------------------------------------------------------------------------------------------------------------------------
def rows(values, faces, R, dtype=np.float32):
    """out[f,s,:] = (w0 r0 + w1 r1) + w2 r2, w_k = i_k / R, for values [V,w] and faces [F,3] -> [F,S,w] in `dtype`"""
    T = np.dtype(dtype).type
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    x = np.asarray(values).astype(T)
    i1, i2 = nodes(R)
    w0, w1, w2 = ((i.astype(T) / T(R))[None, :, None] for i in (R - i1 - i2, i1, i2))
    r0, r1, r2 = (x[f[:, k]][:, None, :] for k in range(3))
    with np.errstate(all='ignore'):
        return ((w0 * r0 + w1 * r1) + w2 * r2).astype(T)


# ---- L3 --------------------------------------------------------------------------------------------------------------------------------------
def lookup(lattice, face, R, b1, b2, dtype=np.float64):
    """The colours [n,C] of lattice [F,S,C] at the points (face [n], barycentrics b1 [n], b2 [n]) -> (colour [n,C] in `dtype`, the three node
    indices read [n,3], upper [n] bool)"""
    T = np.dtype(dtype).type
    lat = np.asarray(lattice)
    face = np.asarray(face, np.int64)
    with np.errstate(all='ignore'):
        u1, u2 = np.asarray(b1).astype(T) * T(R), np.asarray(b2).astype(T) * T(R)
        i1 = np.clip(np.where(np.isnan(u1), 0, np.floor(u1)), 0, R - 1).astype(np.int64)
        i2 = np.clip(np.where(np.isnan(u2), 0, np.floor(u2)), 0, R - 1 - i1).astype(np.int64)
        f1, f2 = u1 - i1.astype(T), u2 - i2.astype(T)
        upper = (f1 + f2 > T(1)) & (i1 + i2 < R - 1)
        wa = np.where(upper, (f1 + f2) - T(1), (T(1) - f1) - f2)
        wb = np.where(upper, T(1) - f1, f1)
        wc = np.where(upper, T(1) - f2, f2)
        sa = node_index(R, np.where(upper, i1 + 1, i1), np.where(upper, i2 + 1, i2))
        sb = node_index(R, np.where(upper, i1, i1 + 1), np.where(upper, i2 + 1, i2))
        sc = node_index(R, np.where(upper, i1 + 1, i1), np.where(upper, i2, i2 + 1))
        ca, cb, cc = (lat[face, s].astype(T) for s in (sa, sb, sc))
        colour = (wa[:, None] * ca + wb[:, None] * cb) + wc[:, None] * cc
    return colour.astype(T), np.stack([sa, sb, sc], 1), upper


# ---- F2' -------------------------------------------------------------------------------------------------------------------------------------
def frame(verts, faces, camera, dtype=np.float64, normals=None, light=FR.LIGHT, bg=None, bg_z=None, analyse=False):
    """raster_frames_ref.render without colours: the geometry, F4's `show`, and in 'colour' F3's shade of a white mesh (1 without normals).
    What `shade` turns into a lattice-coloured frame; one such frame serves every lattice."""
    return FR.render(verts, faces, camera, dtype, colours=None, normals=normals, light=light, bg=bg, bg_z=bg_z, analyse=analyse)


def shade(fr, face_colours, R, dtype=np.float64, lit=True, bg=None):
    """`frame`'s dict with 'colour' = L3's colour (times the frame's shade if lit) and 'out' its bytes (F5) -> a new dict, plus 'nodes'
    [H,W,3] (the node indices read, -1 where nothing covers).  The frame must have been made with `dtype` and the same bg."""
    T = np.dtype(dtype).type
    cov = fr['face_id'] >= 0
    H, W = cov.shape
    b = fr['bary'][cov].astype(T)
    c, idx, _ = lookup(face_colours, fr['face_id'][cov], R, b[:, 1], b[:, 2], dtype)
    with np.errstate(all='ignore'):
        if lit:
            c = c * fr['colour'][cov][:, :1].astype(T)                                           # a white mesh's colour IS the shade, per channel
        colour = np.ones((H, W, 3), T)
        colour[cov] = c
        x = colour * T(255)
        byte = np.clip(np.where(np.isnan(x), T(0), x), 0, 255).astype(np.uint8)                  # F5
    back = np.full((H, W, 3), 255, np.uint8) if bg is None else np.asarray(bg)
    node_map = np.full((H, W, 3), -1, np.int64)
    node_map[cov] = idx
    out = dict(fr)
    out.update(colour=colour, out=np.where(fr['show'][..., None], byte, back), nodes=node_map)
    return out


def render(verts, faces, camera, face_colours, R, dtype=np.float64, normals=None, light=FR.LIGHT, bg=None, bg_z=None, analyse=False):
    """One frame of nm_raster_frames_lattice: `frame` then `shade`"""
    fr = frame(verts, faces, camera, dtype, normals, light, bg, bg_z, analyse)
    return shade(fr, face_colours, R, dtype, lit=normals is not None, bg=bg)


def surface_points(fr, verts, faces):
    """float64 [n,3]: the points of the mesh the covered pixels of a frame show, (b0 v0 + b1 v1) + b2 v2 with the frame's barycentrics, in the
    order of np.nonzero(face_id >= 0)"""
    cov = fr['face_id'] >= 0
    fw = np.asarray(faces, np.int64)[fr['face_id'][cov]]
    b = fr['bary'][cov].astype(np.float64)
    v = np.asarray(verts).astype(np.float64)
    return (b[:, 0:1] * v[fw[:, 0]] + b[:, 1:2] * v[fw[:, 1]]) + b[:, 2:3] * v[fw[:, 2]]


# ---- the quality test's scene ------------------------------------------------------------------------------------------------------------------
STRIPE_SHAPE = (40, 38)                                                    # synthetic.capsule_mesh arguments: 1522 vertices, 3040 faces
STRIPE_CELL = 0.09                                                         # two of the capsule's edges: faces some 8 pixels wide in STRIPE_IMAGE
STRIPE_R = 8
STRIPE_IMAGE = (96, 64)                                                    # W, H
STRIPE_BOX = (-0.3, -0.65, -0.2, 0.3, 0.65, 0.2)                           # the capsule's radii (0.25, 0.6, 0.15) with room around them


def mean_edge(verts, faces):
    v, f = np.asarray(verts).astype(np.float64), np.asarray(faces, np.int64)
    return float(np.mean([np.linalg.norm(v[f[:, k]] - v[f[:, (k + 1) % 3]], axis=1).mean() for k in range(3)]))


def stripes(points, wavelength):
    """0.5 + 0.5 sin(2 pi x / wavelength) in float64, the same in the three channels -> [n,3]"""
    x = np.asarray(points).astype(np.float64)[:, 0]
    return np.repeat((0.5 + 0.5 * np.sin(2.0 * np.pi * x / wavelength))[:, None], 3, 1)


def stripe_cameras():
    from neuman_hip import synthetic
    W, H = STRIPE_IMAGE
    return [synthetic.SimpleCapture(W, H, c2w=synthetic.spherical_c2w(*c)) for c in FR.CAMERAS]


def colour_errors(out, fr, verts, faces, wavelength):
    """mean |byte / 255 - stripes(surface point)| over the covered pixels of one frame -> (sum of the errors, number of values)"""
    cov = fr['face_id'] >= 0
    want = stripes(surface_points(fr, verts, faces), wavelength)
    got = np.asarray(out)[cov].astype(np.float64) / 255.0
    return float(np.abs(got - want).sum()), int(want.size)
