"""-m gpu: the mesh kernels past the sizes at which they change behaviour -- what tests/test_hip_sizes.py does for the ray-list kernels.
  a, b  raster_scan_kernel (csrc/raster_device.h: ONE workgroup of 256 threads, ceil(T / 256) tiles each) on images of more than 256 tiles,
        through the rasteriser and through the soft silhouette with its gradient;
  c     one handle from a small image to a large one and back: the tile scratch and the lists regrow under it;
  d     sil_scan_batch_kernel (csrc/silhouette.hip: 1024 threads over B T entries, the cameras checked 1024 at a time) past 1024 entries and
        past 1024 frames;
  e     iso_scan_kernel (csrc/isosurface.hip: 256 threads, ceil(spans / 256) spans of 2048 grid vertices each) on grids of more than 256 spans;
  f     near_far_kernel (csrc/nearfar.hip) with its cluster table full, V = 32 768, and one vertex past it, where it falls back to one sphere;
  g, h  an extracted mesh of production size (222 050 faces), and one with faces of zero area, through the rasteriser, near / far and the
        closest-point search.
Every shape comes from tests/helpers/mesh_sizes.py, whose table tests/test_mesh_size_table.py holds to the kernels' source on the CPU; that
file also shows, from the float64 helpers alone, that the covered tiles and the owning spans straddle many scan threads -- a wrong partial sum
moves every later list, so it must show here.  No tolerance is new: every comparison is made by the suite it extends (_compare of
test_hip_raster.py / test_hip_silhouette.py, check_against_restatement of test_hip_isosurface.py, atol 1e-6 of test_near_far_and_compaction,
the closest-point tolerance of test_hip_warp_edges.py).  Each test prints a [mesh-sizes] line; profiles/mesh_sizes.md keeps a copy."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import isosurface_ref as IR  # noqa: E402
import mesh_sizes as MS  # noqa: E402
import raster_ref as RR  # noqa: E402
import test_hip_raster as TR  # noqa: E402
import test_hip_sequence_fit as TQ  # noqa: E402
import test_hip_silhouette as TS  # noqa: E402
from oracle import ray_ops as O  # noqa: E402
from oracle import warp as OW  # noqa: E402
from test_hip_isosurface import M, check_against_restatement, run_c_abi  # noqa: E402,F401  (M: the extractor's fixture)
from test_hip_warp_edges import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


def cu(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to('cuda', dtype).contiguous()


def _capsule(shape):
    from neuman_hip import synthetic
    return synthetic.capsule_mesh(*shape)


# ---- a: the rasteriser past SCAN_THREADS tiles --------------------------------------------------------------------------------------------
def _raster_errors(dev, r64):
    both = ~r64['ambiguous'] & (r64['face_id'] >= 0)
    return {k: float(np.abs(dev[k][both].astype(np.float64) - r64[k][both]).max()) for k in ('zbuf', 'bary', 'rgba')}


def _rasterised(tag, verts, faces, cap, seed=0):
    """the statements of tests/test_hip_raster.py::test_parity_at_the_edges_of_the_kernels_structure on one input, and two runs with the same bits
    -> (the float64 run, the device's outputs)"""
    from neuman_hip import render_utils
    H, W = cap.shape
    r64, tol, f32dev = TR._reference(verts, faces, cap, 'mesh-sizes: ' + tag)
    image = TR._image(H, W, seed)
    dev = TR._device(verts, faces, cap, image)
    TR._compare(tag, dev, r64, tol, f32dev, image)
    v = torch.as_tensor(verts).cuda()
    face_id, zbuf, bary = render_utils.rasterize_mesh(v, faces, cap)                      # the pass without shading is the same pass
    assert np.array_equal(face_id.cpu().numpy(), dev['face_id']) and np.array_equal(zbuf.cpu().numpy(), dev['zbuf']) and np.array_equal(bary.cpu().numpy(), dev['bary'])
    mask = render_utils.body_mask(v, faces, cap)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), dev['face_id'] >= 0)
    again = TR._device(verts, faces, cap, image)
    for k in dev:
        assert np.array_equal(dev[k], again[k]), (tag, k)                                 # two runs: the same bits in every output
    err = _raster_errors(dev, r64)
    return r64, dev, ", ".join(f"{k} {err[k]:.2e} (allowed {tol[k]:.2e})" for k in err)


@pytest.mark.parametrize("case", list(MS.RASTER_CASES))
def test_rasteriser_past_one_tile_per_scan_thread(case):
    shape, W, H, shift = MS.RASTER_CASES[case]
    T = MS.tiles(W, H)
    assert T > MS.C.SCAN_THREADS
    verts, faces = _capsule(shape)
    r64, dev, figures = _rasterised(case, verts, faces, MS.capture(W, H, shift))
    t, threads = MS.tile_census(r64['face_id'] >= 0, W, H)
    assert len(threads) >= 3                                                               # a wrong partial sum moves every later tile's list
    if case in MS.REACHES_PAST_THE_THREAD_COUNT:
        assert t.max() >= MS.C.SCAN_THREADS
    print(f"[mesh-sizes] raster {case}: {T} tiles, {MS.per_thread(T, MS.C.SCAN_THREADS)} per scan thread; covered tiles {t.min()}-{t.max()}, owned by "
          f"{len(threads)} scan threads; {int((r64['face_id'] >= 0).sum())} px covered, {int(r64['ambiguous'].sum())} ambiguous; device vs float64: {figures}")


# ---- b: the silhouette and its gradient past SCAN_THREADS tiles -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(MS.SILHOUETTE_CASES))
def test_silhouette_and_gradient_past_one_tile_per_scan_thread(case):
    shape, W, H, shift = MS.RASTER_CASES[case]
    sigma = MS.SILHOUETTE_SIGMA
    verts, faces = _capsule(shape)
    cap = MS.capture(W, H, shift)
    r64, tol, f32dev = TS._reference('mesh-sizes: ' + case, verts, faces, cap, sigma)
    dev = TS._device(verts, faces, cap, sigma, g_alpha=r64['g_alpha'])                    # (the upstream gradient is zero on the ambiguous pixels)
    assert np.abs(r64['g_verts']).max() > 0
    TS._compare(case, dev, r64, tol, f32dev)
    t, threads = MS.tile_census(r64['alpha'] > 0, W, H)
    assert len(threads) >= 3
    ok = ~r64['ambiguous']
    err = {k: float(np.abs(dev[k][ok].astype(np.float64) - r64[k][ok]).max()) for k in ('alpha', 'keep')}
    err['g_verts'] = float(np.abs(dev['g_verts'].astype(np.float64) - r64['g_verts']).max())
    print(f"[mesh-sizes] silhouette {case}, sigma {sigma:g}: {MS.tiles(W, H)} tiles; alpha > 0 in tiles {t.min()}-{t.max()}, owned by {len(threads)} scan threads; "
          f"{int((r64['alpha'] > 0).sum())} px, {int(r64['ambiguous'].sum())} ambiguous; device vs float64: "
          + ", ".join(f"{k} {err[k]:.2e} (allowed {tol[k]:.2e})" for k in err))


# ---- c: one handle across the threshold ----------------------------------------------------------------------------------------------------
def _all_passes(R, verts, cap, g_alpha):
    from neuman_hip import raster
    cam = raster.camera_of(cap)
    sigma, blur = MS.SILHOUETTE_SIGMA, raster.default_blur_radius(MS.SILHOUETTE_SIGMA)
    out = list(R.rasterize(verts, cam, shade=True))
    alpha, keep, n_cand = R.silhouette(verts, cam, sigma, blur, want_count=True)
    return out + [alpha, keep, n_cand, R.silhouette_backward(verts, cam, sigma, blur, keep, g_alpha)]


def test_one_handle_from_a_small_image_to_a_large_one_and_back():
    """count / offset / cursor are carved from ONE allocation sized by the largest image seen, the lists from another: after the regrowth, and
    back at the small size inside the large scratch, every output is the output of a fresh handle, bit for bit"""
    from neuman_hip import raster
    verts, faces = _capsule((12, 10))
    v = torch.as_tensor(verts).cuda()
    R = raster.Rasterizer(faces, verts.shape[0])
    names = ('face_id', 'zbuf', 'bary', 'rgba', 'alpha', 'keep', 'n_cand', 'g_verts')
    covered = []
    for step, (W, H) in enumerate((MS.SMALL_IMAGE, MS.BIG_IMAGE, MS.SMALL_IMAGE)):
        cap = MS.capture(W, H)
        g = torch.as_tensor(np.random.default_rng(W).standard_normal((H, W)).astype(np.float32)).cuda()
        got = _all_passes(R, v, cap, g)
        fresh = raster.Rasterizer(faces, verts.shape[0])
        want = _all_passes(fresh, v, cap, g)
        fresh.close()
        for k, a, b in zip(names, got, want):
            assert a.shape == b.shape and same_bits(a, b), (step, W, H, k)
        covered.append(int((got[0] >= 0).sum()))
        assert covered[-1] > 50 and float(got[-1].abs().max()) > 0
    R.close()
    print(f"[mesh-sizes] one handle at {MS.SMALL_IMAGE}, {MS.BIG_IMAGE}, {MS.SMALL_IMAGE} ({MS.tiles(*MS.SMALL_IMAGE)}, {MS.tiles(*MS.BIG_IMAGE)}, "
          f"{MS.tiles(*MS.SMALL_IMAGE)} tiles): 8 outputs each equal to a fresh handle's, bit for bit; covered px {covered}")


# ---- d: the batched silhouette past BATCH_SCAN_THREADS entries -----------------------------------------------------------------------------
def test_silhouette_batch_past_one_entry_per_scan_thread():
    """B = 5 frames of 225 tiles: 1125 entries, two per thread of sil_scan_batch_kernel; every frame's forward and backward are the one-frame
    entries' bits"""
    from neuman_hip import raster
    B, side, sigma = MS.BATCH_FRAMES, MS.BATCH_SIDE, MS.SILHOUETTE_SIGMA
    n = B * MS.tiles(side, side)
    assert n > MS.C.BATCH_SCAN_THREADS
    views = (TQ.VIEWS + ((120., 25., 1.45), (-100., -5., 1.25)))[:B]
    twists = (TQ.TWISTS + (-1.1, 0.3))[:B]
    faces, V, verts, caps = TQ._frames((40, 38), side, side, views, twists)
    R = raster.Rasterizer(faces, V)
    g = TQ._g_alpha(B, side, side)
    one = TQ._one_by_one(R, verts, caps, sigma, g)
    bat = TQ._batched(R, verts, caps, sigma, g)
    for b in range(B):
        assert int((one[0][b] > 0).sum()) > 50 and float(one[3][b].abs().max()) > 0
    TQ._same(bat, one, 'B T = 1125')
    TQ._same(TQ._batched(R, verts, caps, sigma, g), bat, 'second run')
    R.close()
    print(f"[mesh-sizes] silhouette batch {B} x {side} x {side}: {n} (frame, tile) entries, {MS.per_thread(n, MS.C.BATCH_SCAN_THREADS)} per scan thread; alpha, keep, "
          f"n_cand, g_verts of every frame equal to the one-frame entries', bit for bit; alpha > 0 on {[int((one[0][b] > 0).sum()) for b in range(B)]} px")


def test_silhouette_batch_past_one_pass_of_the_camera_check():
    """B = 1030 frames of one tile: the camera check makes a second pass, and a NaN in frame 1027's w2c is seen only by it"""
    from neuman_hip import _lib, raster, synthetic
    B, side, sigma = MS.MANY_FRAMES, MS.C.TILE, MS.SILHOUETTE_SIGMA
    blur = raster.default_blur_radius(sigma)
    verts1, faces = _capsule((12, 10))
    V = verts1.shape[0]
    rng = np.random.default_rng(1030)
    views = np.stack([rng.uniform(-180, 180, B), rng.uniform(-40, 40, B), rng.uniform(1.2, 1.8, B)], 1)      # a seeded set: no two frames alike
    caps = [synthetic.SimpleCapture(side, side, c2w=synthetic.spherical_c2w(*v)) for v in views]
    verts = torch.as_tensor(verts1).cuda()[None].expand(B, V, 3).contiguous()
    R = raster.Rasterizer(faces, V)
    cams = raster.batch_cameras(caps, verts.device)
    g = TQ._g_alpha(B, side, side)
    alpha, keep, n_cand = R.silhouette_batch(verts, cams, sigma, blur, want_count=True)
    g_verts = R.silhouette_backward_batch(verts, cams, sigma, blur, keep, g)
    pick = list(MS.MANY_CHECKED)
    one = TQ._one_by_one(R, verts[pick], [caps[b] for b in pick], sigma, g[pick])
    TQ._same([alpha[pick], keep[pick], n_cand[pick], g_verts[pick]], one, f'frames {pick} of {B}')
    seen = (alpha > 0).flatten(1).any(1)
    assert bool(seen[pick].all()) and not torch.equal(alpha[pick[1]], alpha[pick[2]])
    # the same call with a NaN in the camera of frame MANY_BAD, through the C entry (its outputs are defined although it fails)
    bad_b, last = MS.MANY_BAD, B - 1
    assert bool(seen[bad_b]) and bool(seen[last])
    w2c, intr, W, H = cams
    bad = w2c.clone()
    bad[bad_b, 1, 2] = float('nan')
    a2, k2 = torch.full_like(alpha, 7.), torch.full_like(keep, 7.)
    p = _lib.dev_ptr
    rc = _lib.lib().nm_raster_silhouette_batch(R._h, p(verts), p(bad, torch.float64), p(intr, torch.float64), B, W, H, float(sigma), float(blur), p(a2), p(k2), None,
                                               _lib.stream_ptr())
    msg = _lib.lib().nm_last_error()
    torch.cuda.synchronize()
    assert rc == -1 and b"nm_raster_silhouette_batch:" in msg and f"frame {bad_b}".encode() in msg, (rc, msg)
    assert bool((a2[bad_b] == 0).all()) and bool((k2[bad_b] == 1).all())
    assert same_bits(a2[last], alpha[last]) and same_bits(k2[last], keep[last])
    others = [b for b in range(B) if b != bad_b]
    assert same_bits(a2[others], alpha[others]) and same_bits(k2[others], keep[others])
    with pytest.raises(_lib.NeumanHipError, match=f"frame {bad_b}"):
        R.silhouette_batch(verts, (bad, intr, W, H), sigma, blur)
    g2 = R.silhouette_backward_batch(verts, (bad, intr, W, H), sigma, blur, keep, g)
    assert bool((g2[bad_b] == 0).all()) and float(g_verts[bad_b].abs().max()) > 0 and same_bits(g2[others], g_verts[others])
    TQ._same([alpha[pick], keep[pick], n_cand[pick], g_verts[pick]], TQ._one_by_one(R, verts[pick], [caps[b] for b in pick], sigma, g[pick]), 'after the refusal')
    R.close()
    print(f"[mesh-sizes] silhouette batch {B} x {side} x {side}: frames {pick} equal to the one-frame entries', bit for bit; with a NaN in frame {bad_b}'s w2c the "
          f"call fails with '{msg.decode()}', frame {bad_b} is alpha 0 / keep 1 / zero gradient and the other {len(others)} frames keep their bits; "
          f"alpha > 0 in {int(seen.sum())} of {B} frames")


# ---- e: the isosurface past ISO_THREADS spans ----------------------------------------------------------------------------------------------
_ISO = {}


def _iso(M, case):
    """check_against_restatement on one grid, once: (field, level, the restatement, the device's verts, faces, normals)"""
    if case not in _ISO:
        dims, freq, level = MS.ISO_CASES[case]
        field = IR.gyroid_field(dims, MS.ISO_BOX, freq)
        field.setflags(write=False)
        _ISO[case] = (field, level) + tuple(check_against_restatement(M, field, MS.ISO_BOX, level, f"mesh-sizes: gyroid {dims[0]}x{dims[1]}x{dims[2]}"))
    return _ISO[case]


@pytest.mark.parametrize("case", list(MS.ISO_CASES))
def test_isosurface_past_one_span_per_scan_thread(M, case):
    dims = MS.ISO_CASES[case][0]
    n_spans = MS.spans(dims)
    assert n_spans > MS.C.ISO_THREADS
    field, level, ref, verts, faces, normals = _iso(M, case)                               # exact counts and face indices, positions, normals
    owners, threads = MS.owner_spans(field, level)
    assert owners.max() >= MS.C.ISO_THREADS and len(threads) >= 3                          # mesh vertices ranked through span offsets past the thread count
    dv = float(np.abs(verts.cpu().numpy() - ref['verts']).max())
    line = (f"[mesh-sizes] isosurface {case}: {n_spans} spans, {MS.per_thread(n_spans, MS.C.ISO_THREADS)} per scan thread; {ref['n_verts']} verts, {ref['n_faces']} faces, "
            f"every face index equal to the restatement's; verts vs the restatement {dv:.2e} (allowed {4 * 2.0 ** -23 * float(np.abs(np.asarray(MS.ISO_BOX)).max()):.2e}); "
            f"mesh vertices owned by spans {owners.min()}-{owners.max()}, of {len(threads)} scan threads")
    if case == MS.PRODUCTION_MESH:                                                         # the C entries between guard rows, twice
        rc, v1, n1, f1, intact = run_c_abi(M, field, MS.ISO_BOX, level)
        assert rc == 0 and intact and torch.equal(f1.cpu(), torch.from_numpy(ref['faces'])) and v1.shape[0] == ref['n_verts']
        assert torch.equal(v1, verts) and torch.equal(n1, normals)
        rc2, v2, n2, f2, intact2 = run_c_abi(M, field, MS.ISO_BOX, level)
        assert rc2 == 0 and intact2 and torch.equal(v1, v2) and torch.equal(n1, n2) and torch.equal(f1, f2)
        line += "; through the C entries twice: guard rows intact, the same bits"
    print(line)


# ---- f: near / far at the cluster table's end ----------------------------------------------------------------------------------------------
def _near_far(o, d, verts, tau=MS.NEAR_FAR_TAU):
    from neuman_hip import ray_utils
    n, f = ray_utils.geometry_guided_near_far(cu(o), cu(d), cu(verts), tau)
    return n.cpu().numpy(), f.cpu().numpy()


def _held_to_the_float64_oracle(n, f, o, d, verts):
    """test_near_far_and_compaction's statement: no hit decision flipped, atol 1e-6 on both bounds -> (hit fraction, worst deviation)"""
    on, of = O.geometry_guided_near_far(o, d, verts, MS.NEAR_FAR_TAU, chunk=32, dtype=np.float64)
    assert ((n < f) != (on < of)).sum() == 0
    hit = on < of
    assert 0 < hit.sum() < len(hit) and np.isposinf(n[~hit]).all() and np.isneginf(f[~hit]).all()
    np.testing.assert_allclose(n[hit], on[hit], atol=1e-6)
    np.testing.assert_allclose(f[hit], of[hit], atol=1e-6)
    return float(hit.mean()), float(max(np.abs(n[hit] - on[hit]).max(), np.abs(f[hit] - of[hit]).max()))


def test_near_far_with_the_cluster_table_full_and_one_vertex_past_it():
    """(measured: the worst bound is 1.02e-6 from the float64 oracle's, inside assert_allclose's atol 1e-6 + rtol 1e-7 |x| and 2 % over a
    bare 1e-6: the kernel rounds v - o to float32 before its float64 discriminant -- profiles/mesh_sizes.md)"""
    V = MS.V_TABLE_FULL
    cloud = MS.body_cloud()
    assert cloud.shape[0] == V == MS.C.MAX_CLUSTERS * MS.C.CLUSTER
    o, d = MS.rays_at(cloud, MS.CLOUD_RAY_SEED)
    n0, f0 = _near_far(o, d, cloud)                                                        # 512 compact clusters: most are skipped
    shuffled = cloud[np.random.default_rng(9).permutation(V)]
    n1, f1 = _near_far(o, d, shuffled)                                                     # 512 body-sized clusters: none is skipped
    n2, f2 = _near_far(o, d, np.concatenate([cloud, cloud[-1:]]))                          # V + 1: one sphere, every vertex; a duplicate changes no min / max
    n3, f3 = _near_far(o, d, np.concatenate([shuffled, shuffled[-1:]]))
    for tag, n, f in (("a permutation", n1, f1), ("V + 1, the fallback", n2, f2), ("V + 1 of the permutation", n3, f3)):
        assert np.array_equal(n0.view(np.int32), n.view(np.int32)) and np.array_equal(f0.view(np.int32), f.view(np.int32)), tag
    hit, err = _held_to_the_float64_oracle(n0, f0, o, d, cloud)
    print(f"[mesh-sizes] near / far, V = {V} (the table's last) and {V + 1} (the fallback), {len(o)} rays, tau {MS.NEAR_FAR_TAU}: sorted, permuted and V + 1 the same "
          f"bits; {100 * hit:.1f} % hit; device vs the float64 oracle {err:.2e} (assert_allclose at atol 1e-6), no decision flipped")


# ---- g: a production-size extracted mesh through its consumers -----------------------------------------------------------------------------
def _search_agrees(verts, faces, pts):
    """'tree' and 'all' bit for bit on distance, face and closest point -> (the tree mesh's info, |signed distance|, face, closest as numpy)"""
    from neuman_hip import ray_utils
    q = cu(pts)
    tree, brute = ray_utils.Mesh(verts, faces, None, 'cuda', search='tree'), ray_utils.Mesh(verts, faces, None, 'cuda', search='all')
    a, b = ray_utils.signed_distance_dev(q, tree), ray_utils.signed_distance_dev(q, brute)
    assert same_bits(a[0].abs(), b[0].abs()) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])
    dist, face, closest = a[0].abs().cpu().numpy(), a[1].cpu().numpy(), a[2].cpu().numpy()
    assert np.isfinite(dist).all() and np.isfinite(closest).all() and face.min() >= 0 and face.max() < len(faces)
    return tree.info(), dist, face, closest


def test_production_size_mesh_through_the_rasteriser(M):
    _, _, ref, verts, faces, _ = _iso(M, MS.PRODUCTION_MESH)
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    cap = MS.capture(64, 48, camera=MS.FAR_CAMERA)
    r64, dev, figures = _rasterised('extracted mesh 64x48', v, f, cap, seed=4)
    assert int((r64['face_id'] >= 0).sum()) > 1000 and len(np.unique(dev['face_id'])) > 200
    print(f"[mesh-sizes] raster of the extracted mesh ({len(f)} faces) at 64 x 48: {int((r64['face_id'] >= 0).sum())} px covered, {int(r64['ambiguous'].sum())} "
          f"ambiguous, {len(np.unique(dev['face_id'])) - 1} faces visible; device vs float64: {figures}")


def test_production_size_mesh_through_near_far(M):
    _, _, ref, verts, _, _ = _iso(M, MS.PRODUCTION_MESH)
    v = verts.cpu().numpy()
    assert (len(v) + MS.C.CLUSTER - 1) // MS.C.CLUSTER > MS.C.MAX_CLUSTERS                 # the fallback by itself
    o, d = MS.rays_at(v, MS.MESH_RAY_SEED, spread=0.8)
    n, f = _near_far(o, d, v)
    hit, err = _held_to_the_float64_oracle(n, f, o, d, v)
    print(f"[mesh-sizes] near / far of the extracted mesh, V = {len(v)}, {len(o)} rays, tau {MS.NEAR_FAR_TAU}: {100 * hit:.1f} % hit; device vs the float64 oracle "
          f"{err:.2e} (assert_allclose at atol 1e-6), no decision flipped")


def test_production_size_mesh_through_the_closest_point_search(M):
    _, _, ref, verts, faces, _ = _iso(M, MS.PRODUCTION_MESH)
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    assert len(f) > MS.C.SMALL_ENCODING_FACES                                              # the wide encoding by itself
    pts = MS.near_surface_points(v, f, MS.N_QUERY, seed=3)
    info, dist, face, closest = _search_agrees(v, f, pts)                                  # (the surface is open: nothing is said about the sign)
    assert info["levels"] >= 9 and face.max() > MS.C.SMALL_ENCODING_FACES
    k = MS.N_ORACLE
    sq, _, _ = OW.closest_point_on_mesh(pts[:k], v, f, culled=True)
    od = np.sqrt(sq)
    print(f"[mesh-sizes] closest point on the extracted mesh ({len(f)} faces, {info['levels']} levels): tree and all-triangles loop the same bits on {len(pts)} "
          f"points; distance vs the float64 oracle on {k}: Linf {np.abs(dist[:k] - od).max():.2e}")
    np.testing.assert_allclose(dist[:k], od, atol=2e-5 * (1 + np.abs(v).max()), rtol=1e-5)      # test_search_below_and_around_one_wave's


# ---- h: faces of zero area -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat_mesh(M):
    """the field of test_values_equal_to_the_level_and_non_finite_values: a sphere with |f| < 0.08 set to the level"""
    from test_hip_isosurface import BOX
    f = IR.sphere_field((13, 12, 11), BOX, (0.0, 0.0, 0.0), 0.5)
    f[np.abs(f) < 0.08] = 0.0
    verts, faces, _ = M.me.extract_mesh(torch.from_numpy(f).cuda(), BOX, 0.0)
    v, fc = verts.cpu().numpy(), faces.cpu().numpy()
    flat = MS.zero_area(v, fc)
    assert 0 < flat.sum() < len(fc)
    return v, fc, flat


def test_zero_area_faces_through_the_rasteriser(flat_mesh):
    v, f, flat = flat_mesh
    cap = MS.capture(64, 48, camera=(30., -20., 2.0))
    r64, dev, figures = _rasterised('zero-area faces 64x48', v, f, cap, seed=5)
    assert r64['n_valid_faces'] <= len(f) - int(flat.sum())                                # rule 2 drops them
    seen = np.unique(dev['face_id'][dev['face_id'] >= 0])
    assert len(seen) > 20 and not flat[seen].any()
    print(f"[mesh-sizes] raster of a mesh with {int(flat.sum())} zero-area faces of {len(f)} at 64 x 48: {r64['n_valid_faces']} faces kept, "
          f"{int((r64['face_id'] >= 0).sum())} px covered, {int(r64['ambiguous'].sum())} ambiguous; device vs float64: {figures}")


def test_zero_area_faces_through_the_closest_point_search(flat_mesh):
    v, f, flat = flat_mesh
    pts = MS.near_surface_points(v, f, MS.N_QUERY, seed=4)
    info, dist, face, closest = _search_agrees(v, f, pts)                                  # finite, tree and all-triangles loop the same bits
    k = MS.N_ORACLE
    od = MS.brute_distance(pts[:k], v, f)                                                  # a zero-area face counts as its three edge segments
    print(f"[mesh-sizes] closest point on a mesh with {int(flat.sum())} zero-area faces of {len(f)}: tree and all-triangles loop the same bits on {len(pts)} points, "
          f"all finite, {int(flat[face].sum())} answers on a zero-area face; distance vs the float64 brute force on {k}: Linf {np.abs(dist[:k] - od).max():.2e}")
    np.testing.assert_allclose(dist[:k], od, atol=2e-5 * (1 + np.abs(v).max()), rtol=1e-5)
