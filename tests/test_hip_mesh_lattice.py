"""-m gpu: nm_mesh_lattice_rows and nm_raster_frames_lattice (csrc/mesh_lattice.hip, csrc/raster_frames.hip; include/neuman_hip.h 'mesh
lattice', rules L1-L3 and F2'), neuman_hip.mesh_texture and the face_colours keyword of Rasterizer.render_frames / render_mesh_frames.

L2 is checked as bits against the float32 run of tests/helpers/mesh_lattice_ref.py.  The renderer's geometry is checked as bits against
nm_raster_frames; its bytes against the float64 helper as tests/test_hip_raster_frames.py checks F2: the helper also runs in float32, the
device is allowed 4 x that run's own worst deviation from the float64 run (floor: 1e-6 relative), the allowance is applied through
raster_frames_ref.byte_range and is never more than 1 byte, all of it away from the pixels the float64 run calls ambiguous
(tests/test_raster_frames_host.py holds them to 1 % on these scenes).  Unlit, L3 is float32 arithmetic on the device's own barycentrics, so
there the bytes are also compared exactly.  Every output of every raw call sits inside a larger allocation whose guard elements must stay as
they were.  The measured figures are printed ([mesh lattice] lines)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mesh_lattice_ref as LR  # noqa: E402
import raster_frames_ref as FR  # noqa: E402
import raster_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64                                                       # guard elements before and after every output
BUFS = {'out': (torch.uint8, 3, 77), 'face_id': (torch.int32, 1, -77), 'zbuf': (torch.float32, 1, 123.0), 'bary': (torch.float32, 3, 123.0)}
GEOMETRY = ('face_id', 'zbuf', 'bary')
_SCENE, _FRAME, _LATTICE = {}, {}, {}


def _scene(name):
    """the scene's numpy arrays (read-only), its device tensors, its batched cameras and its handle: built once, shared, never written to"""
    if name not in _SCENE:
        from neuman_hip import raster
        s = FR.scene(name)
        rng = np.random.default_rng(7)
        s['bg'] = rng.integers(0, 256, (len(s['caps']), s['H'], s['W'], 3), dtype=np.uint8)
        for a in s.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        s['d'] = {k: torch.from_numpy(np.array(s[k])).cuda() for k in ('verts', 'normals', 'colours', 'bg')}
        s['cams'] = raster.batch_cameras(s['caps'], 'cuda')
        s['rast'] = raster.Rasterizer(s['faces'], s['verts'].shape[1])
        _SCENE[name] = s
    return _SCENE[name]


def _lattice(name, R):
    """random node colours [F,S,3] in [0, 1] for a scene's mesh -> (numpy, device tensor): made once, shared, never written to"""
    if (name, R) not in _LATTICE:
        lat = np.random.default_rng(100 + R).random((len(_scene(name)['faces']), LR.lattice_size(R), 3)).astype(np.float32)
        lat.setflags(write=False)
        _LATTICE[name, R] = (lat, torch.from_numpy(np.array(lat)).cuda())
    return _LATTICE[name, R]


def _frame(name, b, dtype):
    """the helper's lit frame of a white mesh (geometry, shade, background; the float64 one with its ambiguity map): one per scene, frame and
    dtype serves every lattice, lit and unlit"""
    key = (name, b, np.dtype(dtype).name)
    if key not in _FRAME:
        s = _scene(name)
        fr = LR.frame(s['verts'][b], s['faces'], RR.camera_of(s['caps'][b]), dtype, normals=s['normals'][b], bg=s['bg'][b], analyse=dtype is np.float64)
        for a in fr.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _FRAME[key] = fr
    return _FRAME[key]


def _raw(entry, rast, verts, cams, colours, R=None, normals=None, light=RR.LIGHT, bg=None, bg_z=None, want_rc=0):
    """one raw call of nm_raster_frames (R None: `colours` [V,3] or None) or nm_raster_frames_lattice (`colours` the lattice) with every output
    between guard elements -> dict of numpy arrays [B,...] (and 'error': nm_last_error())"""
    from neuman_hip import _lib
    w2c, intr, W, H = cams
    B = int(verts.shape[0])
    n = B * H * W
    mem = {k: torch.full((G + n * c + G,), fill, device='cuda', dtype=dt) for k, (dt, c, fill) in BUFS.items()}
    ptr = {k: ctypes.c_void_p(mem[k].data_ptr() + G * mem[k].element_size()) for k in mem}
    light_p = None if normals is None else (ctypes.c_double * 3)(*light)
    P = _lib.dev_ptr
    head = (rast._h, P(verts), P(w2c, torch.float64), P(intr, torch.float64), B, W, H)
    tail = (P(normals), light_p, P(bg, torch.uint8), P(bg_z), ptr['out'], ptr['face_id'], ptr['zbuf'], ptr['bary'], _lib.stream_ptr())
    assert (entry == "nm_raster_frames") == (R is None)
    rc = getattr(_lib.lib(), entry)(*head, P(colours), *(() if R is None else (R,)), *tail)
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _lib.lib().nm_last_error())
    res = dict(error=_lib.lib().nm_last_error().decode())
    for k, (dt, c, fill) in BUFS.items():
        a = mem[k].cpu().numpy()
        assert np.all(a[:G] == fill) and np.all(a[G + n * c:] == fill), k                    # the guard elements
        res[k] = a[G:G + n * c].reshape((B, H, W) if c == 1 else (B, H, W, c))
    return res


def _lat(rast, verts, cams, face_colours, R, **kw):
    return _raw("nm_raster_frames_lattice", rast, verts, cams, face_colours, R, **kw)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _unlit_bytes(res, lattice, R, bg):
    """what rule L3 makes, in float32, of the device's own face_id and bary, as bytes [B,H,W,3]: unlit and without bg_z the device's `out`
    bit for bit"""
    out = np.array(bg)
    for b in range(out.shape[0]):
        cov = res['face_id'][b] >= 0
        c, _, _ = LR.lookup(lattice, res['face_id'][b][cov], R, res['bary'][b][cov][:, 1], res['bary'][b][cov][:, 2], np.float32)
        with np.errstate(all='ignore'):
            x = c * np.float32(255)
            out[b][cov] = np.clip(np.where(np.isnan(x), np.float32(0), x), 0, 255).astype(np.uint8)
    return out


# ---- L2 ------------------------------------------------------------------------------------------------------------------------------------
def _rows_call(faces, V, rows, R, want_rc=0):
    """one raw nm_mesh_lattice_rows call, out between guard elements -> ([F,S,w] float32, nm_last_error())"""
    from neuman_hip import _lib
    F, w, S = int(faces.shape[0]), int(rows.shape[1]), LR.lattice_size(R)
    n = F * S * w
    mem = torch.full((G + n + G,), 123.0, device='cuda', dtype=torch.float32)
    rc = _lib.lib().nm_mesh_lattice_rows(_lib.dev_ptr(faces, torch.int32), F, V, _lib.dev_ptr(rows), w, R, ctypes.c_void_p(mem.data_ptr() + 4 * G),
                                         _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _lib.lib().nm_last_error())
    a = mem.cpu().numpy()
    assert np.all(a[:G] == 123.0) and np.all(a[G + n:] == 123.0)
    return a[G:G + n].reshape(F, S, w), _lib.lib().nm_last_error().decode()


@pytest.mark.parametrize("w", [1, 3, 4])
@pytest.mark.parametrize("R", [1, 2, 3, 7, 64])
def test_node_rows_are_the_float32_helpers_bits(R, w):
    """one face; one face short of a workgroup's 256 threads' worth at R = 1 ... and past it; the largest lattice"""
    V = 97
    rng = np.random.default_rng(1000 * R + w)
    rows = (rng.standard_normal((V, w)) * 3).astype(np.float32)
    d_rows = torch.from_numpy(rows).cuda()
    for F in (1, 255, 256, 257):
        faces = rng.integers(0, V, (F, 3)).astype(np.int32)
        got, _ = _rows_call(torch.from_numpy(faces).cuda(), V, d_rows, R)
        assert _same_bits(got, LR.rows(rows, faces, R, np.float32)), (R, w, F)


def test_a_face_index_out_of_range_is_found_on_the_device_and_reported():
    from neuman_hip import _lib, mesh_texture
    V, F, R = 50, 257, 3
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    faces[200, 1], faces[30, 2], faces[256, 0] = V, -1, 1 << 30
    got, error = _rows_call(torch.from_numpy(faces).cuda(), V, torch.from_numpy(rows).cuda(), R, want_rc=-1)
    assert "nm_mesh_lattice_rows:" in error and "3 invalid faces" in error and "face 30" in error, error
    bad = np.zeros(F, bool)
    bad[[30, 200, 256]] = True
    assert (got[bad] == 123.0).all()                                                         # never dereferenced, never written
    assert _same_bits(got[~bad], LR.rows(rows, faces[~bad], R, np.float32))                  # the other faces' nodes are as they would be
    with pytest.raises(_lib.NeumanHipError, match="invalid faces"):
        mesh_texture.lattice_rows(torch.from_numpy(rows).cuda(), torch.from_numpy(faces).cuda(), R)


# ---- F2' -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lit", [True, False], ids=["lit", "unlit"])
@pytest.mark.parametrize("R", [1, 2, 5, 16])
@pytest.mark.parametrize("name", list(FR.SCENES))
def test_random_node_colours_against_nm_raster_frames_geometry_and_the_float64_helper(name, R, lit):
    s = _scene(name)
    d = s['d']
    lat, d_lat = _lattice(name, R)
    normals = d['normals'] if lit else None
    dev = _lat(s['rast'], d['verts'], s['cams'], d_lat, R, normals=normals, bg=d['bg'])
    old = _raw("nm_raster_frames", s['rast'], d['verts'], s['cams'], d['colours'], normals=normals, bg=d['bg'])
    for k in GEOMETRY:
        assert _same_bits(dev[k], old[k]), (name, R, k)                                      # F1: the same bits as nm_raster_frames gives
    if not lit:
        assert np.array_equal(dev['out'], _unlit_bytes(dev, lat, R, s['bg']))                # L3 is float32 arithmetic on the device's own b'
    for b in range(len(s['caps'])):
        f64, f32 = _frame(name, b, np.float64), _frame(name, b, np.float32)
        r64 = LR.shade(f64, lat, R, np.float64, lit=lit, bg=s['bg'][b])
        r32 = LR.shade(f32, lat, R, np.float32, lit=lit, bg=s['bg'][b])
        amb, cov = f64['ambiguous'], f64['face_id'] >= 0
        ok, both = ~amb, ~amb & cov
        tol, f32dev = FR.colour_tolerance(r64, r32, ok)
        lo, hi = FR.byte_range(r64['colour'], tol)
        got = dev['out'][b]
        outside = int(((got < lo) | (got > hi))[both].sum())
        byte_err = int(np.abs(got[both].astype(np.int32) - r64['out'][both]).max())
        print(f"[mesh lattice] {name} frame {b} R = {R} {'lit' if lit else 'unlit'}: covered {int(cov.sum())} px, ambiguous {int(amb.sum())}; colour: "
              f"float32 helper vs float64 {f32dev:.2e}, allowed {tol:.2e}, bytes outside what it allows {outside}, bytes off by at most {byte_err}")
        assert int(cov.sum()) > 50 and int(amb.sum()) <= 0.01 * int(cov.sum())
        assert np.array_equal(dev['face_id'][b][ok], f64['face_id'][ok])
        assert outside == 0 and byte_err <= 1
        none = dev['face_id'][b] < 0
        assert np.array_equal(got[none], s['bg'][b][none])                                   # F5: every other pixel takes bg's bytes


@pytest.mark.parametrize("R", [1, 4])
def test_a_lattice_made_from_vertex_colours_renders_as_the_vertex_colours_do(R):
    from neuman_hip import mesh_texture
    s = _scene('three_frames_96x64')
    d = s['d']
    d_faces = torch.from_numpy(s['faces'].astype(np.int32)).cuda()
    d_lat = mesh_texture.lattice_rows(d['colours'], d_faces, R)
    assert tuple(d_lat.shape) == (len(s['faces']), mesh_texture.lattice_size(R), 3) and d_lat.dtype == torch.float32
    assert _same_bits(d_lat.cpu().numpy(), LR.rows(s['colours'], s['faces'], R, np.float32))
    for normals in (d['normals'], None):
        a = _lat(s['rast'], d['verts'], s['cams'], d_lat, R, normals=normals, bg=d['bg'])
        b = _raw("nm_raster_frames", s['rast'], d['verts'], s['cams'], d['colours'], normals=normals, bg=d['bg'])
        cov = a['face_id'] >= 0
        diff = np.abs(a['out'].astype(np.int32) - b['out'])
        print(f"[mesh lattice] vertex colours as an R = {R} lattice, {'lit' if normals is not None else 'unlit'}: {int((diff > 0).sum())} of "
              f"{3 * int(cov.sum())} bytes differ, by at most {int(diff.max())}")
        assert cov.sum() > 1000 and diff.max() <= 1 and (diff > 0).mean() < 0.05


def test_a_nan_node_gives_byte_zero_exactly_at_the_pixels_whose_three_nodes_include_it():
    name, R = 'three_frames_96x64', 5
    s = _scene(name)
    d = s['d']
    lat, d_lat = _lattice(name, R)
    poisoned = np.array(lat)
    bad_node = LR.node_index(R, 2, 1)                                                        # an interior node: six sub-triangles share it
    poisoned[::3, bad_node, 1] = np.nan                                                      # the green of that node on every third face
    clean = _lat(s['rast'], d['verts'], s['cams'], d_lat, R, bg=d['bg'])
    dev = _lat(s['rast'], d['verts'], s['cams'], torch.from_numpy(poisoned).cuda(), R, bg=d['bg'])
    cov = dev['face_id'] >= 0
    # "per the helper": rule L3's float32 arithmetic on the device's own face_id and bary, which is what picks the three nodes
    _, idx, _ = LR.lookup(lat, dev['face_id'][cov], R, dev['bary'][cov][:, 1], dev['bary'][cov][:, 2], np.float32)
    hit = np.zeros(cov.shape, bool)
    hit[cov] = (idx == bad_node).any(1) & (dev['face_id'][cov] % 3 == 0)
    assert hit.sum() > 100 and (cov & ~hit).sum() > 1000
    assert (dev['out'][hit][:, 1] == 0).all()                                                # a weight of zero does not hide a NaN either
    assert np.array_equal(dev['out'][..., [0, 2]], clean['out'][..., [0, 2]]) and np.array_equal(dev['out'][~hit], clean['out'][~hit])
    assert np.array_equal(dev['out'], _unlit_bytes(dev, poisoned, R, s['bg']))
    # ... and the float64 helper's frame says the same away from its ambiguous pixels and from the cells' borders (where a rounding moves a
    # pixel into the neighbouring sub-triangle)
    for b in range(len(s['caps'])):
        f64 = _frame(name, b, np.float64)
        r64 = LR.shade(f64, poisoned, R, np.float64, lit=False, bg=s['bg'][b])
        r32 = LR.shade(_frame(name, b, np.float32), poisoned, R, np.float32, lit=False, bg=s['bg'][b])
        agree = ~f64['ambiguous'] & (f64['face_id'] >= 0) & (r64['nodes'] == r32['nodes']).all(-1) & (f64['face_id'] == dev['face_id'][b])
        assert agree.sum() > 0.9 * (f64['face_id'] >= 0).sum() and np.array_equal(np.isnan(r64['colour'][..., 1])[agree], hit[b][agree])


def test_bg_and_bg_z_byte_for_byte():
    name, R = 'three_frames_96x64', 5
    s = _scene(name)
    d = s['d']
    args = (s['rast'], d['verts'], s['cams'], _lattice(name, R)[1], R)
    free = _lat(*args, normals=d['normals'], bg=d['bg'])
    cov = free['face_id'] >= 0
    assert np.array_equal(free['out'][~cov], s['bg'][~cov]) and (free['out'][cov] != s['bg'][cov]).any(-1).mean() > 0.9
    z = torch.from_numpy(free['zbuf']).cuda()
    at = _lat(*args, normals=d['normals'], bg=d['bg'], bg_z=z)
    assert np.array_equal(at['out'], s['bg'])                                                # bg_z = zbuf: out == bg byte for byte
    behind = _lat(*args, normals=d['normals'], bg=d['bg'], bg_z=torch.nextafter(z, torch.full_like(z, float('inf'))))
    assert np.array_equal(behind['out'], free['out'])                                        # one step behind: the unoccluded result
    checker = (np.indices(cov.shape).sum(0) % 2).astype(bool)
    mixed = _lat(*args, normals=d['normals'], bg=d['bg'], bg_z=torch.from_numpy(np.where(checker, np.nan, np.inf).astype(np.float32)).cuda())
    assert np.array_equal(mixed['out'], np.where(checker[..., None], s['bg'], free['out']))  # a NaN hides the mesh, +inf never does
    assert (cov & checker).sum() > 100 and (cov & ~checker).sum() > 100
    for r in (at, behind, mixed):                                                            # the geometry reports the mesh alone
        for k in GEOMETRY:
            assert _same_bits(r[k], free[k]), k
    white = _lat(*args, normals=d['normals'])
    assert (white['out'][~cov] == 255).all() and np.array_equal(white['out'][cov], free['out'][cov])      # bg = None gives white
    assert (_lat(*args, normals=d['normals'], bg_z=z)['out'] == 255).all()


def test_frame_b_of_a_batch_is_the_one_frame_call_on_it_and_two_runs_give_the_same_bytes():
    name, R = 'three_frames_96x64', 16
    s = _scene(name)
    d = s['d']
    d_lat = _lattice(name, R)[1]
    whole, again = (_lat(s['rast'], d['verts'], s['cams'], d_lat, R, normals=d['normals'], bg=d['bg']) for _ in range(2))
    for k in BUFS:
        assert _same_bits(whole[k], again[k]), k                                             # F7
    w2c, intr, W, H = s['cams']
    for b in range(3):
        one = _lat(s['rast'], d['verts'][b:b + 1], (w2c[b:b + 1].contiguous(), intr[b:b + 1].contiguous(), W, H), d_lat, R, normals=d['normals'][b:b + 1],
                   bg=d['bg'][b:b + 1])
        for k in BUFS:
            assert _same_bits(one[k][0], whole[k][b]), (b, k)


def test_a_frame_with_a_nan_camera_between_ordinary_frames():
    name, R = 'three_frames_96x64', 2
    s = _scene(name)
    d = s['d']
    d_lat = _lattice(name, R)[1]
    good = _lat(s['rast'], d['verts'], s['cams'], d_lat, R, normals=d['normals'], bg=d['bg'])
    w2c, intr, W, H = s['cams']
    w2c = w2c.clone()
    w2c[1, 2, 1] = float('nan')
    bad = _lat(s['rast'], d['verts'], (w2c, intr, W, H), d_lat, R, normals=d['normals'], bg=d['bg'], want_rc=-1)
    assert "nm_raster_frames_lattice:" in bad['error'] and "frame 1" in bad['error'], bad['error']
    assert (bad['face_id'][1] == -1).all() and np.isposinf(bad['zbuf'][1]).all() and (bad['bary'][1] == 0).all() and np.array_equal(bad['out'][1], s['bg'][1])
    for k in BUFS:                                                                           # F6: reported AFTER every frame's outputs are written
        assert _same_bits(bad[k][0], good[k][0]) and _same_bits(bad[k][2], good[k][2]), k


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_the_lattice_shows_a_stripe_pattern_that_per_vertex_colours_blur():
    """The test that states the feature.  The capsule thinned on the device; colour = 0.5 + 0.5 sin(2 pi x / wavelength), four thinned edge
    lengths per period: the vertices sample it four times per period, an R = 8 lattice 32 times.  Linear interpolation's error goes with
    the spacing squared, so eight times finer nodes predict a factor of about 64; the mean absolute error against the float64 value of the
    source at each covered pixel's surface point must fall below a quarter, which leaves 16 for faces of uneven size and the bytes' step of
    1/255.  tests/test_mesh_lattice_host.py shows the same for the numpy helper alone (ratio 0.061 there)."""
    from neuman_hip import mesh_simplify, mesh_texture, raster, render_utils, synthetic
    full, full_faces = synthetic.capsule_mesh(*LR.STRIPE_SHAPE)
    verts, faces = mesh_simplify.simplify_mesh(torch.from_numpy(full).cuda(), torch.from_numpy(full_faces.astype(np.int32)).cuda(), LR.STRIPE_CELL,
                                               aabb=LR.STRIPE_BOX)
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    assert 4 * len(v) < len(full) and len(f) > 200
    wavelength = 4.0 * LR.mean_edge(v, f)

    def source(points, dirs):
        assert points.shape == dirs.shape and points.is_cuda and bool((dirs.norm(dim=-1) - 1).abs().max() < 1e-5)
        return (0.5 + 0.5 * torch.sin(2.0 * np.pi * points[:, :1].double() / wavelength)).float().expand(-1, 3)

    normals = torch.from_numpy(RR.vertex_normals(v, f).astype(np.float32)).cuda()
    colours = source(verts, torch.nn.functional.normalize(normals, dim=-1)).contiguous()
    face_colours = mesh_texture.bake_face_colours(source, verts, faces, normals, LR.STRIPE_R)
    assert tuple(face_colours.shape) == (len(f), mesh_texture.lattice_size(LR.STRIPE_R), 3) and face_colours.dtype == torch.float32
    assert float(face_colours.min()) >= 0 and float(face_colours.max()) <= 1
    assert torch.equal(face_colours, mesh_texture.bake_face_colours(source, verts, faces, normals, LR.STRIPE_R, chunk=1000))
    caps = LR.stripe_cameras()
    world = verts[None].expand(len(caps), -1, -1).contiguous()
    by_vertex = render_utils.render_mesh_frames(world, f, caps, colours=colours).cpu().numpy()
    by_lattice = render_utils.render_mesh_frames(world, f, caps, face_colours=face_colours).cpu().numpy()
    _, face_id, _, bary = raster.rasterizer_for(f, len(v)).render_frames(world, raster.batch_cameras(caps, 'cuda'), want_geometry=True)
    err_v = err_l = n = 0
    for b in range(len(caps)):
        fr = dict(face_id=face_id[b].cpu().numpy(), bary=bary[b].cpu().numpy())
        assert int((fr['face_id'] >= 0).sum()) > 500
        e_v, k = LR.colour_errors(by_vertex[b], fr, v, f, wavelength)
        e_l, _ = LR.colour_errors(by_lattice[b], fr, v, f, wavelength)
        err_v, err_l, n = err_v + e_v, err_l + e_l, n + k
    print(f"[mesh lattice] device: {len(v)} vertices, {len(f)} faces, wavelength {wavelength:.4f}; mean |colour error| per vertex {err_v / n:.5f}, "
          f"R = {LR.STRIPE_R} lattice {err_l / n:.5f}, ratio {err_l / err_v:.4f}")
    assert err_l < 0.25 * err_v


def test_render_mesh_frames_with_face_colours_does_not_depend_on_the_chunking():
    from neuman_hip import render_utils
    name, R = 'past_the_scan_240x240', 5
    s = _scene(name)
    d, B = s['d'], 5
    d_lat = _lattice(name, R)[1]
    kw = dict(normals=d['normals'], background=d['bg'], face_colours=d_lat)
    whole = render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], frames_per_call=B, **kw)
    assert whole.dtype == torch.uint8 and tuple(whole.shape) == (B, 240, 240, 3) and whole.is_cuda
    raw = _lat(s['rast'], d['verts'], s['cams'], d_lat, R, normals=d['normals'], bg=d['bg'])
    assert np.array_equal(whole.cpu().numpy(), raw['out'])
    for step in (2, 1, None):                                                                # 2 + 2 + 1; one by one; the default
        assert torch.equal(render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], frames_per_call=step, **kw), whole), step
    out, face_id, zbuf, bary = s['rast'].render_frames(d['verts'], s['cams'], normals=d['normals'], background=d['bg'], want_geometry=True, face_colours=d_lat)
    assert torch.equal(out, whole) and all(_same_bits(t.cpu().numpy(), raw[k]) for t, k in ((face_id, 'face_id'), (zbuf, 'zbuf'), (bary, 'bary')))
    # without face_colours nothing changes: the old call, byte for byte
    old = render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], colours=d['colours'], normals=d['normals'], background=d['bg'])
    assert np.array_equal(old.cpu().numpy(), _raw("nm_raster_frames", s['rast'], d['verts'], s['cams'], d['colours'], normals=d['normals'], bg=d['bg'])['out'])
    with pytest.raises(ValueError, match="not both"):
        s['rast'].render_frames(d['verts'], s['cams'], d['colours'], face_colours=d_lat)


def test_lattice_resolution_and_a_static_nets_bake():
    from neuman_hip import _lib, mesh_texture, synthetic
    v, f = synthetic.capsule_mesh(12, 10)
    verts, faces = torch.from_numpy(v).cuda(), torch.from_numpy(f.astype(np.int32)).cuda()
    longest = max(float(np.linalg.norm(v[f[:, k]].astype(np.float64) - v[f[:, (k + 1) % 3]], axis=1).max()) for k in range(3))
    for texel, want in ((longest * 10, 1), (longest / 2.5, 3), (longest / 7.99, 8), (longest / 1000, 64)):
        R = mesh_texture.lattice_resolution(verts, faces, texel)
        assert type(R) is int and R == want, (texel, R, want)
    normals = torch.from_numpy(RR.vertex_normals(v, f).astype(np.float32)).cuda()
    for net in (synthetic.make_joiner(0).cuda(), synthetic.make_variant_joiner(3, use_viewdirs=False).cuda()):
        with torch.no_grad():
            raw = net(verts, -normals if net.nerf.use_viewdirs else None, precision='fp32')  # extract_net_mesh's per-vertex colours
        per_vertex = torch.sigmoid(raw[..., :3])
        lat = mesh_texture.bake_face_colours(net, verts, faces, normals, 1, precision='fp32')
        assert tuple(lat.shape) == (len(f), 3, 3) and float(lat.min()) >= 0 and float(lat.max()) <= 1
        assert float((lat - per_vertex[faces.long()]).abs().max()) < 1e-5                   # R = 1: the nodes are the corners
        fine = mesh_texture.bake_face_colours(net, verts, faces, normals, 4, precision='fp32')
        corners = [LR.node_index(4, 0, 0), LR.node_index(4, 4, 0), LR.node_index(4, 0, 4)]
        assert tuple(fine.shape) == (len(f), 15, 3) and float((fine[:, corners] - lat).abs().max()) < 1e-5
        assert float((mesh_texture.bake_face_colours(net, verts, faces, normals, 4, precision='fp32', chunk=777) - fine).abs().max()) < 1e-5
    with pytest.raises(NotImplementedError):
        mesh_texture.bake_face_colours(synthetic.make_variant_joiner(6, raw_pos_dim=4).cuda(), verts, faces, normals, 2)
    with pytest.raises(_lib.NeumanHipError):
        mesh_texture.bake_face_colours(net, verts.cpu(), faces, normals, 2)
