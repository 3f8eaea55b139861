"""-m gpu: nm_mesh_atlas_pack and nm_mesh_atlas_sample (csrc/mesh_atlas.hip; include/neuman_hip.h 'mesh atlas', rules A1-A5) and
neuman_hip.mesh_export.

Both kernels are float32 arithmetic with no freedom in its order, so they are checked as bits against the float32 run of
tests/helpers/mesh_atlas_ref.py (a NaN for a NaN: its sign and payload are not the rules').  What the header derives -- the node at a node,
rule L3 in the cells on the hypotenuse, a quarter of the cell's second difference elsewhere -- is checked on the geometry the frame
rasteriser returns, against mesh_lattice_ref.lookup in float64, with the project's usual allowance: 4 x the float32 helper's own worst
deviation from its float64 run, floor 1e-6 relative.  Every output of every raw call sits inside a larger allocation whose guard elements
must stay as they were.  The measured figures are printed ([mesh atlas] lines)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mesh_atlas_ref as AR  # noqa: E402
import mesh_lattice_ref as LR  # noqa: E402
import raster_frames_ref as FR  # noqa: E402
import raster_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64                                                       # guard elements before and after every output
FILL = 123.0
_LATTICE = {}


def _lattice(F, R):
    """random node colours [F,S,3], some of them outside [0, 1] (the packing does not clamp): made once per (F, R), shared, never written to"""
    if (F, R) not in _LATTICE:
        lat = (np.random.default_rng(1000 * R + F).standard_normal((F, LR.lattice_size(R), 3)) * 2).astype(np.float32)
        lat.setflags(write=False)
        _LATTICE[F, R] = lat
    return _LATTICE[F, R]


def _guarded(n):
    mem = torch.full((G + n + G,), FILL, device='cuda', dtype=torch.float32)
    return mem, ctypes.c_void_p(mem.data_ptr() + 4 * G)


def _unguard(mem, n):
    a = mem.cpu().numpy()
    assert np.all(a[:G] == FILL) and np.all(a[G + n:] == FILL)                                 # the guard elements
    return a[G:G + n]


def _pack_call(lat, R):
    """one raw nm_mesh_atlas_pack call, the atlas between guard elements -> [H,W,3] float32"""
    from neuman_hip import _lib
    F = int(lat.shape[0])
    W, H, _ = AR.atlas_size(F, R)
    mem, ptr = _guarded(H * W * 3)
    d_lat = torch.from_numpy(np.array(lat)).cuda()
    rc = _lib.lib().nm_mesh_atlas_pack(_lib.dev_ptr(d_lat), F, R, ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (rc, _lib.lib().nm_last_error())
    return _unguard(mem, H * W * 3).reshape(H, W, 3)


def _sample_call(atlas, F, R, face_id, bary):
    """one raw nm_mesh_atlas_sample call, out between guard elements -> [n,3] float32"""
    from neuman_hip import _lib
    n = int(face_id.shape[0])
    mem, ptr = _guarded(3 * n)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (atlas, face_id.astype(np.int32), bary.astype(np.float32))]
    rc = _lib.lib().nm_mesh_atlas_sample(_lib.dev_ptr(d[0]), F, R, _lib.dev_ptr(d[1], torch.int32), _lib.dev_ptr(d[2]), n, ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (rc, _lib.lib().nm_last_error())
    return _unguard(mem, 3 * n).reshape(n, 3)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- A3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 3, 10, 257])
@pytest.mark.parametrize("R", [1, 2, 3, 7, 64])
def test_the_atlas_is_the_float32_helpers_bits(R, F):
    """a lone lower face; one full block; an odd count; a last row with empty blocks; more texels than one workgroup's 256"""
    lat = np.array(_lattice(F, R))
    lat[0, 0, 0], lat[F - 1, -1, 2] = -0.0, 1e30                                               # a copy keeps a zero's sign; nothing is clamped
    want, writes = AR.pack(lat, R, np.float32)
    got = _pack_call(lat, R)
    W, H, nbx = AR.atlas_size(F, R)
    unused = int((writes == 0).sum())
    print(f"[mesh atlas] pack F = {F} R = {R}: {W} x {H}, {nbx} blocks a row, {unused} of {W * H} texels belong to no face")
    assert not np.isnan(want).any() and _same_bits(got, want)
    assert not np.signbit(got[writes == 0]).any() and (got[writes == 0] == 0).all()            # +0.0 where no face owns the texel
    assert unused == W * H - F * (LR.lattice_size(R) + R + 1)
    assert _same_bits(_pack_call(lat, R), got)                                                 # two runs, the same bits


def test_a_nan_node_shows_in_its_texel_and_in_the_gutter_texels_computed_from_it_and_nowhere_else():
    F, R = 5, 5
    lat = _lattice(F, R)
    poisoned = np.array(lat)
    # (face, node, channel) -> the face's own local texels that must turn NaN in that channel
    cases = {(1, (2, 1), 1): [(2, 1)],                                                         # interior: its texel alone
             (3, (3, 2), 0): [(3, 2), (3, 3), (4, 2)],                                         # on the hypotenuse: c(x, y-1) of one gutter texel, c(x-1, y) of the next
             (3, (2, 2), 2): [(2, 2), (3, 3)],                                                 # one row below it: c(x-1, y-1) of one gutter texel
             (1, (R, 0), 2): [(R, 0), (R, 1), (R + 1, 0)]}                                     # corner 1: a gutter texel and the corner gutter's copy
    W, H, nbx = AR.atlas_size(F, R)
    want_nan = np.zeros((H, W, 3), bool)
    for (f, (i1, i2), ch), texels in cases.items():
        poisoned[f, LR.node_index(R, i1, i2), ch] = np.nan
        for x, y in texels:
            X, Y = AR.place(f, x, y, R, nbx)
            want_nan[Y, X, ch] = True
    clean, dev = _pack_call(lat, R), _pack_call(poisoned, R)
    assert int(want_nan.sum()) == 9 and np.array_equal(np.isnan(dev), want_nan) and not np.isnan(clean).any()
    assert np.array_equal(dev[~want_nan].view(np.uint8), clean[~want_nan].view(np.uint8))      # nothing else changes
    assert AR.same_values(dev, AR.pack(poisoned, R, np.float32)[0])


# ---- A5 ------------------------------------------------------------------------------------------------------------------------------------
def _probe_points(F, R, seed):
    """(face_id [n] int64, bary [n,3] float32): random points of every face, points on and a rounding beside the cells' borders, barycentrics
    that are no barycentrics, and face ids outside [0, F)"""
    rng = np.random.default_rng(seed)
    b = rng.dirichlet((1, 1, 1), 1500).astype(np.float32)
    grid = (np.arange(R + 1, dtype=np.float32) / np.float32(R))
    on = np.array([(1 - p - q, p, q) for p in grid for q in grid], np.float32)                 # the whole square of nodes: half of it outside
    beside = [np.nextafter(on, np.float32(s)).astype(np.float32) for s in (-1, 2)]
    edge = np.stack([np.zeros(40, np.float32), rng.random(40, dtype=np.float32), rng.integers(0, R + 1, 40).astype(np.float32) / np.float32(R)], 1)
    wild = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.3, -0.5, 2.0], np.float32)
    odd = np.array([(0, p, q) for p in wild for q in wild], np.float32)
    bary = np.concatenate([b, on] + beside + [edge, edge[:, [0, 2, 1]], odd])
    face = rng.integers(0, F, len(bary))
    face[::97] = -1
    face[5::101] = F
    face[7::103] = 1 << 30
    return face, bary


@pytest.mark.parametrize("R", [1, 2, 5, 16])
def test_the_sample_is_the_float32_helpers_bits(R):
    F = 7                                                                                      # even and odd faces, a lone lower face last
    atlas, _ = AR.pack(_lattice(F, R), R, np.float32)
    face, bary = _probe_points(F, R, R)
    want, info = AR.sample(atlas, F, R, face, bary[:, 1], bary[:, 2], np.float32)
    got = _sample_call(atlas, F, R, face, bary)
    outside = ~info['valid']
    print(f"[mesh atlas] sample R = {R}: {len(face)} points, {int(outside.sum())} with a face_id outside [0, {F}), {int(np.isnan(want).any(1).sum())} NaN, "
          f"{int((info['i1'] + info['i2'] == R - 1).sum())} in hypotenuse cells, odd faces {int((face[~outside] % 2 == 1).sum())}")
    assert outside.sum() >= 30 and {int(f) for f in face[outside]} == {-1, F, 1 << 30}
    assert (got[outside] == 0).all() and not np.signbit(got[outside]).any()
    assert np.isnan(want).any() and np.isfinite(want).all(1).sum() > 1000 and len(face) > 256
    assert AR.same_values(got, want)
    # whatever the barycentrics, the texels the rule reads are the face's own (and the device gave the rule's values)
    owner, _ = AR.owners(F, R)
    assert (owner[info['Y'], info['X']][~outside] == face[~outside, None]).all()


@pytest.mark.parametrize("R", [1, 2, 4, 8, 16, 64])
def test_the_sample_at_a_nodes_barycentrics_is_the_node_bit_for_bit(R):
    """i / R and (i / R) R are exact for these R: the weights are 1, 0, 0, 0"""
    F = 3
    lat = _lattice(F, R)
    i1, i2 = LR.nodes(R)
    S = len(i1)
    b1, b2 = (i1 / R).astype(np.float32), (i2 / R).astype(np.float32)
    bary = np.tile(np.stack([1 - b1 - b2, b1, b2], 1), (F, 1))
    face = np.repeat(np.arange(F), S)
    got = _sample_call(_pack_call(lat, R), F, R, face, bary)                                   # the device's own atlas
    assert _same_bits(got.reshape(F, S, 3), lat)


@pytest.mark.parametrize("R", [2, 5])
def test_a_textured_view_stays_within_the_derived_bound_of_the_lattice_renderers_rule(R):
    """Rasterizer.render_frames(want_geometry=True), then sample_atlas: the per-pixel difference from rule L3 (mesh_lattice_ref.lookup, float64,
    on the same face_id and bary) is at most |D| / 4 of the pixel's cell and 0 in a cell on the hypotenuse, plus the rounding allowance"""
    from neuman_hip import mesh_export, raster
    s = FR.scene('three_frames_96x64')
    F = len(s['faces'])
    lat = np.random.default_rng(100 + R).random((F, LR.lattice_size(R), 3)).astype(np.float32)
    d_lat = torch.from_numpy(lat).cuda()
    rast = raster.Rasterizer(s['faces'], s['verts'].shape[1])
    _, face_id, _, bary = rast.render_frames(torch.from_numpy(s['verts']).cuda(), raster.batch_cameras(s['caps'], 'cuda'), want_geometry=True)
    atlas = mesh_export.pack_atlas(d_lat)
    W, H, _ = mesh_export.atlas_size(F, R)
    assert tuple(atlas.shape) == (H, W, 3) and atlas.dtype == torch.float32 and atlas.is_cuda
    a32, a64 = AR.pack(lat, R, np.float32)[0], AR.pack(lat, R, np.float64)[0]
    assert _same_bits(atlas.cpu().numpy(), a32)
    view = mesh_export.sample_atlas(atlas, F, R, face_id, bary)
    assert tuple(view.shape) == tuple(bary.shape) and view.dtype == torch.float32
    fid, b, got = face_id.cpu().numpy().reshape(-1), bary.cpu().numpy().reshape(-1, 3), view.cpu().numpy().reshape(-1, 3)
    cov = fid >= 0
    assert cov.sum() > 3000 and (got[~cov] == 0).all()
    s32, _ = AR.sample(a32, F, R, fid, b[:, 1], b[:, 2], np.float32)
    s64, info = AR.sample(a64, F, R, fid, b[:, 1], b[:, 2], np.float64)
    assert AR.same_values(got, s32)
    l3, _, _ = LR.lookup(lat, fid[cov], R, b[cov, 1], b[cov, 2], np.float64)
    f32dev = float(np.abs(s32[cov].astype(np.float64) - s64[cov]).max())
    tol = max(4.0 * f32dev, 1e-6 * float(np.abs(s64[cov]).max()))
    hyp = (info['i1'] + info['i2'] == R - 1)[cov]
    D = np.abs(info['D'][cov])
    assert np.abs(D[hyp]).max() < 1e-14
    diff = np.abs(got[cov].astype(np.float64) - l3)
    print(f"[mesh atlas] textured view R = {R}: {int(cov.sum())} covered px, {int(hyp.sum())} in hypotenuse cells; float32 helper vs float64 {f32dev:.2e}, "
          f"allowed {tol:.2e}; |sample - L3| at most {diff[hyp].max():.2e} in hypotenuse cells, {diff[~hyp].max():.3f} elsewhere (largest |D| / 4 "
          f"{D.max() / 4:.3f}), largest excess over |D| / 4 {float((diff - D / 4).max()):.2e}")
    assert hyp.sum() > 500 and (~hyp).sum() > 500
    assert (diff[hyp] <= tol).all() and (diff <= D / 4 + tol).all()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_an_exported_stripe_capsule_opened_by_a_plain_viewer_keeps_what_per_vertex_colours_blur(tmp_path):
    """The test that states the feature.  The stripe capsule of tests/test_hip_mesh_lattice.py -- thinned on the device, a sine of four
    thinned edge lengths per period, baked at R = 8 -- exported, the three files parsed back, and every covered pixel of the test's cameras
    coloured as an OBJ viewer would: the face's three `vt` blended with the device's barycentrics, the decoded PNG filtered bilinearly in
    float64.  The mean absolute error against the analytic source must be below a quarter of the per-vertex colouring's, the lattice test's
    own threshold for the same reason (eight times finer samples predict 1/64; the rest is for uneven faces and the bytes' step)."""
    from neuman_hip import mesh_export, mesh_simplify, mesh_texture, raster, render_utils, synthetic
    full, full_faces = synthetic.capsule_mesh(*LR.STRIPE_SHAPE)
    verts, faces = mesh_simplify.simplify_mesh(torch.from_numpy(full).cuda(), torch.from_numpy(full_faces.astype(np.int32)).cuda(), LR.STRIPE_CELL,
                                               aabb=LR.STRIPE_BOX)
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    assert 4 * len(v) < len(full) and len(f) > 200
    wavelength = 4.0 * LR.mean_edge(v, f)

    def source(points, dirs):
        return (0.5 + 0.5 * torch.sin(2.0 * np.pi * points[:, :1].double() / wavelength)).float().expand(-1, 3)

    normals = torch.from_numpy(RR.vertex_normals(v, f).astype(np.float32)).cuda()
    colours = source(verts, None).contiguous()
    R = LR.STRIPE_R
    face_colours = mesh_texture.bake_face_colours(source, verts, faces, normals, R)
    paths = mesh_export.export_mesh(str(tmp_path / "capsule.obj"), verts, faces, face_colours, normals)
    assert [os.path.basename(p) for p in paths] == ["capsule.obj", "capsule.mtl", "capsule.png"] and all(os.path.getsize(p) > 0 for p in paths)
    obj, image = AR.read_export(paths[0])
    W, H, _ = mesh_export.atlas_size(len(f), R)
    assert image.shape == (H, W, 3) and np.array_equal(image, render_utils.frame_to_uint8(mesh_export.pack_atlas(face_colours)).cpu().numpy())
    assert np.array_equal(obj['v'].astype(np.float32), v) and np.array_equal(obj['f_v'], f) and np.array_equal(obj['f_n'], f)
    assert np.array_equal(obj['vn'].astype(np.float32), normals.cpu().numpy()) and np.abs(obj['vt'].reshape(-1, 3, 2) - AR.uvs(len(f), R)).max() < 1e-10
    caps = LR.stripe_cameras()
    world = verts[None].expand(len(caps), -1, -1).contiguous()
    by_vertex = render_utils.render_mesh_frames(world, f, caps, colours=colours).cpu().numpy()
    by_lattice = render_utils.render_mesh_frames(world, f, caps, face_colours=face_colours).cpu().numpy()
    _, face_id, _, bary = raster.rasterizer_for(f, len(v)).render_frames(world, raster.batch_cameras(caps, 'cuda'), want_geometry=True)
    err_v = err_l = err_a = n = 0
    for b in range(len(caps)):
        fr = dict(face_id=face_id[b].cpu().numpy(), bary=bary[b].cpu().numpy())
        cov = fr['face_id'] >= 0
        assert int(cov.sum()) > 500
        vt = obj['vt'][obj['f_t'][fr['face_id'][cov]]]                                         # [n,3,2]: the face's three texture coordinates
        seen = np.zeros(cov.shape + (3,))
        seen[cov] = AR.viewer_sample(image, (fr['bary'][cov].astype(np.float64)[:, :, None] * vt).sum(1))     # bytes, as float64
        e_v, k = LR.colour_errors(by_vertex[b], fr, v, f, wavelength)
        e_l, _ = LR.colour_errors(by_lattice[b], fr, v, f, wavelength)
        e_a, _ = LR.colour_errors(seen, fr, v, f, wavelength)
        err_v, err_l, err_a, n = err_v + e_v, err_l + e_l, err_a + e_a, n + k
    print(f"[mesh atlas] exported capsule: {len(v)} vertices, {len(f)} faces, atlas {W} x {H}, wavelength {wavelength:.4f}; mean |colour error| per vertex "
          f"{err_v / n:.5f}, R = {R} lattice renderer {err_l / n:.5f} (ratio {err_l / err_v:.4f}), the exported files in a bilinear viewer {err_a / n:.5f} "
          f"(ratio {err_a / err_v:.4f})")
    assert err_a < 0.25 * err_v
