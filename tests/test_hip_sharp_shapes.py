"""-m gpu: the mesh kernels on non-convex, sharp-edged meshes (tests/helpers/sharp_shapes.py): a star prism with acute tips and reflex
notches (40 faces, and 2560 after three rounds of subdivision), the same topology with inner and outer radius exchanged, a torus, a star-shaped
slab 1e-3 thick, the fine prism without its top cap and the prism with a third face on one edge.

Every other suite feeds these kernels synthetic.capsule_mesh, on which the sign of nm_signed_distance does not depend on which of the seven
vectors of the winning face is read (tests/test_sharp_shapes_host.py shows it, and shows that here every wrong slot flips at least 20 of the
signs asserted below).  The truth is float64 brute force with the header's rule restated, the analytic inside test of the solid and the winding
number.  No tolerance is new: atol 2e-6 on distances and barycentrics > -1e-4 are tests/test_hip_render.py::test_signed_distance's, the warp's
are test_tree_search_is_bit_identical_to_all_triangles' and test_warp_vs_oracle's, the rasteriser's and the silhouette's are the calibrated
ones of _compare in tests/test_hip_raster.py and tests/test_hip_silhouette.py.  Each test prints [sharp] lines; profiles/sharp_shapes.md keeps a
copy."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import raster_ref as RR  # noqa: E402
import sharp_shapes as SS  # noqa: E402
import test_hip_raster as TR  # noqa: E402
import test_hip_sequence_fit as TQ  # noqa: E402
import test_hip_silhouette as TS  # noqa: E402
from oracle import warp as OW  # noqa: E402
from test_hip_warp_edges import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SEARCHES = ('tree', 'all', 'tree_wide')


def cu(x, dtype=torch.float32):
    return torch.as_tensor(np.array(x)).to('cuda', dtype).contiguous()


def _np(xs):
    return [x.cpu().numpy() for x in xs]


def _three_searches(verts, faces, pts, T=None):
    """nm_signed_distance through the tree, the all-triangles loop and the wide stack: the same bits -> the tree's (sdist, face, closest)"""
    from neuman_hip import ray_utils
    q = cu(pts)
    out = [ray_utils.signed_distance_dev(q, ray_utils.Mesh(np.array(verts), np.array(faces), T, 'cuda', search=s)) for s in SEARCHES]
    for other, what in zip(out[1:], SEARCHES[1:]):
        for x, y, name in zip(out[0], other, ('sdist', 'face', 'closest')):
            assert same_bits(x, y), f"{name}: '{what}' differs from 'tree' at {int((x != y).sum())} of {x.numel()} values"
    return out[0]


def _held_to_the_truth(tag, answers, s, q, t):
    """the statements of the signed-distance tests on one set of answers (numpy): distance, foot, face, sign; prints the figures first"""
    S, I, C = answers
    verts, faces = s['verts'].astype(np.float64), s['faces']
    n = len(q)
    assert S.shape == (n,) and I.shape == (n,) and C.shape == (n, 3) and I.min() >= 0 and I.max() < len(faces)
    ok = ~t['excluded']
    e_dist = float(np.abs(np.abs(S) - t['dist']).max())
    e_foot = float(np.abs(np.linalg.norm(C.astype(np.float64) - q, axis=1) - t['dist']).max())
    bad_face = int((~t['near'][np.arange(n), I]).sum())
    tri = verts[faces[I]]
    bary = OW.barycentric_coordinates_tri(C.astype(np.float64), tri[:, 0], tri[:, 1], tri[:, 2])
    neg = S < 0
    bad_sign = int(((neg != (t['sign'] < 0)) & ok).sum())
    line = (f"[sharp] {tag}: F {len(faces)}, {n} queries, {neg.mean():.2f} inside, {int((~ok).sum())} excluded; |sdist| vs float64 {e_dist:.2e}, |closest - p| vs float64 "
            f"{e_foot:.2e} (allowed 2e-6); faces not among the float64 minima {bad_face}, same face as the float64 winner {int((I == t['face']).sum())}; smallest "
            f"barycentric of the foot {bary.min():.1e}; signs differing from the float64 rule {bad_sign}")
    if s['closed']:
        bad_wn = int(((neg != (t['winding'] > 0.5)) & ok).sum())
        line += f", from the winding number {bad_wn}"
        if 'inside' in t:
            bad_in = int(((neg != t['inside']) & ok).sum())
            line += f", from the analytic inside test {bad_in}"
    fl = SS.flips(t)
    print(line + f"; of these signs a wrong slot would flip {min(fl)} to {max(fl)}")
    np.testing.assert_allclose(np.abs(S), t['dist'], atol=2e-6)
    np.testing.assert_allclose(np.linalg.norm(C.astype(np.float64) - q, axis=1), t['dist'], atol=2e-6)
    assert bad_sign == 0
    if s['closed']:
        assert bad_wn == 0
        if 'inside' in t:
            assert bad_in == 0
    assert bad_face == 0
    assert (bary > -1e-4).all()


# ---- signed distance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SS.CLOSED + SS.UNSIGNED)
def test_signed_distance_on_sharp_shapes(name):
    """closed shapes: distance, foot, face and the sign against the float64 rule, the analytic inside test and the winding number; the open
    prism and the fin: the same without the inside tests -- a boundary edge sums one normal, the fin's edge three"""
    s, q, t = SS.shape_truth(name)
    _held_to_the_truth(name, _np(_three_searches(s['verts'], s['faces'], q)), s, q, t)


def _both_orientations(name):
    from neuman_hip import ray_utils
    s, q, t = SS.shape_truth(name)
    a = ray_utils.signed_distance_dev(cu(q), ray_utils.Mesh(np.array(s['verts']), np.array(s['faces']), None, 'cuda'))
    b = ray_utils.signed_distance_dev(cu(q), ray_utils.Mesh(np.array(s['verts']), SS.reversed_faces(s['faces']), None, 'cuda'))
    return t, a, b


@pytest.mark.parametrize("name", SS.CLOSED)
def test_reversed_orientation_gives_the_opposite_sign(name):
    """every face reversed (v1 and v2 exchanged, the list in the same order): the sign is the opposite on every query off the surface, and the
    answers meet the float64 truth as before -- the corner pick and the angle weights of the vertex pseudonormals, and the edge sums, read
    the other way round"""
    t, (S, I, C), (Sr, Ir, Cr) = _both_orientations(name)
    n = len(t['dist'])
    ok = ~t['excluded']
    Sr_, Ir_, Cr_ = _np((Sr, Ir, Cr))
    same_side = int(((Sr < 0) == (S < 0))[S != 0].sum())
    bad_sign = int((((Sr_ < 0) == (t['sign'] < 0)) & ok).sum())
    bad_face = int((~t['near'][np.arange(n), Ir_]).sum())
    print(f"[sharp] {name} reversed: sign not the opposite of the forward answer at {same_side} of {int((S != 0).sum())} queries off the surface, not the opposite of "
          f"the float64 rule's at {bad_sign}; |sdist| vs float64 {np.abs(np.abs(Sr_) - t['dist']).max():.2e} (allowed 2e-6); faces not among the float64 minima {bad_face}")
    assert same_side == 0 and bad_sign == 0 and bad_face == 0
    np.testing.assert_allclose(np.abs(Sr_), t['dist'], atol=2e-6)
    np.testing.assert_allclose(np.linalg.norm(Cr_.astype(np.float64) - SS.queries(name), axis=1), t['dist'], atol=2e-6)


@pytest.mark.parametrize("name", SS.CLOSED)
def test_reversed_orientation_keeps_every_other_bit(name):
    """with every face reversed sdist is the exact negative wherever the distance is not zero, and face and closest are unchanged, bit for bit.

    (This did not hold at first.  exact_tri builds the foot as fmaf(ac, w, fmaf(ab, v, a)) and the foot on edge v1v2 as (1 - t_bc, t_bc); a
    reversed face exchanges (ab, v) with (ac, w), neither expression is symmetric under that in floating point, so feet moved by an ulp and
    near-ties went to the other face: of 3000 queries sdist was not the exact negative at 57 on star_prism_fine and 164 on thin_plate, the
    face differed at 24 and 165, closest at 332 and 730 -- on the slab by 6.56e-05, the other sheet at the same distance.  tri_prep_kernel now
    writes a face and its reverse as ONE record, the corners after the first in the order of their vertex ids; profiles/sharp_shapes.md.)"""
    t, (S, I, C), (Sr, Ir, Cr) = _both_orientations(name)
    off = S != 0
    print(f"[sharp] {name} reversed, bit for bit: of {int(off.sum())} queries off the surface sdist is not the exact negative at {int((Sr != -S)[off].sum())} (largest "
          f"difference of |sdist| {float((Sr.abs() - S.abs()).abs().max()):.2e}); face differs at {int((Ir != I).sum())}, closest at "
          f"{int((Cr != C).any(1).sum())} (largest {float((Cr - C).abs().max()):.2e})")
    assert same_bits(Sr[off], -S[off])
    assert torch.equal(Ir, I) and same_bits(Cr, C)


def test_update_to_the_swapped_prism_and_back():
    """nm_mesh_update from star_prism_fine to star_prism_swapped -- every convex side edge becomes reflex and the reverse -- on a handle whose
    pseudonormal table exists: the pn_stale branch rebuilds it on the adjacency of the first build.  Equal to a fresh build bit for bit, held
    to the swapped truth; then back, equal to the first answers bit for bit"""
    from neuman_hip import ray_utils
    s0, q0, t0 = SS.shape_truth('star_prism_fine')
    s1, q1, t1 = SS.shape_truth('star_prism_swapped')
    assert np.array_equal(s0['faces'], s1['faces'])
    for search in SEARCHES:
        m = ray_utils.Mesh(np.array(s0['verts']), np.array(s0['faces']), None, 'cuda', search=search)
        first = ray_utils.signed_distance_dev(cu(q0), m)                                         # the table exists from here on
        m.update(cu(s1['verts']))
        moved = ray_utils.signed_distance_dev(cu(q1), m)
        fresh = ray_utils.signed_distance_dev(cu(q1), ray_utils.Mesh(np.array(s1['verts']), np.array(s1['faces']), None, 'cuda', search=search))
        for x, y, k in zip(moved, fresh, ('sdist', 'face', 'closest')):
            assert same_bits(x, y), (search, k, int((x != y).sum()))
        if search == 'tree':
            _held_to_the_truth('star_prism_fine updated to star_prism_swapped', _np(moved), s1, q1, t1)
            changed = int(((moved[0] < 0) != (ray_utils.signed_distance_dev(cu(q1), ray_utils.Mesh(np.array(s0['verts']), np.array(s0['faces']), None, 'cuda'))[0] < 0)).sum())
            assert changed > 100                                                                 # (the two solids do differ on these queries)
        m.update(cu(s0['verts']))
        back = ray_utils.signed_distance_dev(cu(q0), m)
        for x, y, k in zip(back, first, ('sdist', 'face', 'closest')):
            assert same_bits(x, y), (search, 'back', k, int((x != y).sum()))
        if search == 'tree':
            _held_to_the_truth('star_prism_fine after the update back', _np(back), s0, q0, t0)
    print(f"[sharp] update: star_prism_fine -> star_prism_swapped -> star_prism_fine through {SEARCHES}: the updated handle equals a fresh build, and the "
          f"first answers after the way back, bit for bit; {changed} of {len(q1)} queries are on the other side of the swapped solid")


# ---- warp --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["star_prism_fine", "thin_plate"])
@pytest.mark.parametrize("pose", ["identity", "twist"])
def test_warp_on_sharp_shapes(name, pose):
    """nm_warp_to_canonical: tree, all-triangles loop and wide stack the same bits; the foot's distance against the float64 minimum; with the
    identity the canonical point is the query -- the thin plate's mid-plane queries are where winner and runner-up are within rounding"""
    from neuman_hip import ray_utils, synthetic
    s, q, t = SS.shape_truth(name)
    if pose == "identity":
        posed, T, want = np.array(s['verts']), np.tile(np.eye(4), (len(s['verts']), 1, 1)), t['dist']
    else:
        posed, T = synthetic.twist_transforms(np.array(s['verts']))
        want = SS.closest_faces(posed, s['faces'], q)[0]
    pts = q.reshape(100, -1, 3)
    out = [ray_utils.warp_to_canonical_dev(cu(pts), ray_utils.Mesh(posed, np.array(s['faces']), T, 'cuda', search=k), want_closest=True) for k in SEARCHES]
    for other, what in zip(out[1:], SEARCHES[1:]):
        for x, y, k in zip(out[0], other, ("can_pts", "can_dirs", "closest")):
            assert same_bits(x, y), f"{name} {pose}: {k} of '{what}' differs from 'tree' at {int((x != y).sum())} of {x.numel()} values"
    cp, cd, cl = [x.reshape(-1, 3) for x in _np(out[0])]
    dist = np.linalg.norm(cl.astype(np.float64) - q, axis=1)
    line = f"[sharp] warp {name} {pose}: {len(q)} samples, three searches the same bits; |closest - p| vs the float64 minimum {np.abs(dist - want).max():.2e}"
    if pose == "identity":
        line += f"; canonical point vs the query {np.abs(cp - q).max():.2e} (allowed 1e-6)"
    print(line)
    assert np.isfinite(cp).all() and np.isfinite(cd).all()
    np.testing.assert_allclose(dist, want, atol=2e-5 * (1 + np.abs(posed).max()), rtol=1e-5)
    if pose == "identity":
        np.testing.assert_allclose(cp, q, atol=1e-6)


# ---- binding -----------------------------------------------------------------------------------------------------------------------------
def test_binding_to_the_fine_prism():
    """mesh_pose.bind_mesh of the queries to star_prism_fine: sdist, face and bary are the direct nm_signed_distance / nm_bary_forward answers
    bit for bit (tests/test_hip_mesh_pose.py's statement for the capsule), and the barycentrics reproduce the closest point to 1e-5"""
    from neuman_hip import _lib, mesh_pose, ray_utils
    s, q, t = SS.shape_truth('star_prism_fine')
    pts = cu(q)
    binding = mesh_pose.bind_mesh(pts, np.array(s['verts']), np.array(s['faces']))
    body = ray_utils.Mesh(np.array(s['verts']), np.array(s['faces']), None, torch.device('cuda'))
    S, I, C = ray_utils.signed_distance_dev(pts, body)
    bary = torch.empty_like(pts)
    P = _lib.dev_ptr
    _lib.check(_lib.lib().nm_bary_forward(P(body.verts), P(binding.tri, torch.int32), P(C), pts.shape[0], P(bary), _lib.stream_ptr()), "nm_bary_forward")
    assert same_bits(binding.sdist, S) and torch.equal(binding.face, I) and same_bits(binding.bary, bary)
    assert torch.equal(binding.tri, body.faces[I.long()])
    b, tri = binding.bary.cpu().numpy().astype(np.float64), binding.tri.cpu().numpy()
    foot = (b[:, :, None] * s['verts'].astype(np.float64)[tri]).sum(1)
    err = float(np.abs(foot - C.cpu().numpy()).max())
    print(f"[sharp] binding to star_prism_fine: {len(q)} points, sdist, face and bary the direct calls' bits; barycentrics reproduce the closest point to {err:.2e} "
          f"(allowed 1e-5), smallest {b.min():.1e}, rows summing to 1 within {np.abs(b.sum(1) - 1).max():.1e}")
    assert err <= 1e-5
    _held_to_the_truth('binding: star_prism_fine', (binding.sdist.cpu().numpy(), binding.face.cpu().numpy(), C.cpu().numpy()), s, q, t)


# ---- rasteriser --------------------------------------------------------------------------------------------------------------------------
RASTER = {'star_prism_fine': (SS.STAR_CAMERA, 'star_prism_swapped', SS.STAR_CAMERA), 'torus': (SS.TORUS_CAMERA, 'torus', SS.TORUS_HOLE_CAMERAS[0])}


@pytest.mark.parametrize("size", [(96, 64), (50, 37)])
@pytest.mark.parametrize("name", list(RASTER))
def test_rasteriser_where_four_faces_cover_a_pixel(name, size):
    """the parity statement of tests/test_hip_raster.py; in addition the winner is exact on the pixels that four or more faces cover"""
    W, H = size
    s = SS.shape(name)
    verts, faces = np.array(s['verts']), np.array(s['faces'])
    cap = SS.capture(RASTER[name][0], W, H)
    tag = f"{name} {W}x{H}"
    r64, tol, f32dev = TR._reference(verts, faces, cap, 'sharp: ' + tag)
    image = TR._image(H, W, 3)
    dev = TR._device(verts, faces, cap, image)
    TR._compare(tag, dev, r64, tol, f32dev, image)
    count = SS.coverage(verts, faces, RR.camera_of(cap))
    deep = count >= 4
    wrong = int((dev['face_id'] != r64['face_id'])[deep].sum())
    print(f"[sharp] raster {tag}: pixels under 0, 1, 2, ... faces {np.bincount(count.ravel()).tolist()}; under four or more {int(deep.sum())}, of them ambiguous "
          f"{int((deep & r64['ambiguous']).sum())}, winner differing from float64's {wrong}")
    assert deep.sum() >= (100 if size == (96, 64) else 30)
    assert wrong == 0


@pytest.mark.parametrize("size", [(96, 64), (50, 37)])
@pytest.mark.parametrize("name", list(RASTER))
def test_frames_entry_gives_the_one_frame_bits(name, size):
    """nm_raster_frames on two frames of one topology (the fine prism and its swapped form; the torus from two cameras): the geometry is
    nm_raster_mesh's, bit for bit, frame by frame -- tests/test_hip_raster_frames.py's first statement -- and render_utils.render_mesh_frames
    gives the bytes of each frame rendered alone"""
    from neuman_hip import raster, render_utils
    W, H = size
    cam0, second, cam1 = RASTER[name]
    faces = np.array(SS.shape(name)['faces'])
    verts = torch.stack([cu(SS.shape(name)['verts']), cu(SS.shape(second)['verts'])])
    caps = [SS.capture(cam0, W, H), SS.capture(cam1, W, H)]
    R = raster.rasterizer_for(faces, verts.shape[1])
    cams = raster.batch_cameras(caps, verts.device)
    colours = cu(np.random.default_rng(2).uniform(0.1, 0.9, (verts.shape[1], 3)))                    # (white on white would show nothing)
    out, face_id, zbuf, bary = R.render_frames(verts, cams, colours, want_geometry=True)
    covered = []
    for b in range(2):
        f1, z1, b1, _ = R.rasterize(verts[b], raster.camera_of(caps[b]))
        covered.append(int((f1 >= 0).sum()))
        assert covered[-1] > 50
        assert torch.equal(face_id[b], f1) and same_bits(zbuf[b], z1) and same_bits(bary[b], b1), (name, size, b)
    images = render_utils.render_mesh_frames(verts, faces, caps, colours=colours)
    assert images.dtype == torch.uint8 and tuple(images.shape) == (2, H, W, 3) and torch.equal(images, out)
    for b in range(2):
        alone = render_utils.render_mesh_frames(verts[b:b + 1], faces, caps[b:b + 1], colours=colours)
        assert torch.equal(alone[0], images[b]), (name, size, b)
        assert bool((images[b][face_id[b] < 0] == 255).all()) and bool((images[b][face_id[b] >= 0] != 255).any(-1).all())
    assert not torch.equal(face_id[0], face_id[1])
    print(f"[sharp] frames {name} {W}x{H}: two frames, covered {covered} px; face_id, zbuf and bary the one-frame entry's bits, the images those of each frame alone")


# ---- silhouette --------------------------------------------------------------------------------------------------------------------------
SIGMA = 1e-3                                                 # blur radius about 3 px at 96 x 64: the hole is wider


def _hole(seen):
    """uncovered pixels with covered ones to the left, to the right, above and below: the torus' hole"""
    left, right = np.maximum.accumulate(seen, 1), np.maximum.accumulate(seen[:, ::-1], 1)[:, ::-1]
    up, down = np.maximum.accumulate(seen, 0), np.maximum.accumulate(seen[::-1], 0)[::-1]
    return ~seen & left & right & up & down


def test_silhouette_of_the_torus_with_its_hole():
    """the parity statement of tests/test_hip_silhouette.py (forward, n_cand, gradient against the float64 helper); inside the hole, further than
    the blur radius from any face, alpha is exactly 0 and an upstream gradient there reaches no vertex"""
    from neuman_hip import raster
    s = SS.shape('torus')
    verts, faces = np.array(s['verts']), np.array(s['faces'])
    cap = SS.capture(SS.TORUS_HOLE_CAMERAS[0], 96, 64)
    r64, tol, f32dev = TS._reference('sharp: torus hole', verts, faces, cap, SIGMA)
    dev = TS._device(verts, faces, cap, SIGMA, g_alpha=r64['g_alpha'])
    assert int((r64['alpha'] > 0).sum()) > 50 and np.abs(r64['g_verts']).max() > 0
    TS._compare('sharp: torus hole', dev, r64, tol, f32dev)
    hole = _hole(r64['n_cand'] > 0)
    g_hole = (np.random.default_rng(5).standard_normal(hole.shape) * hole).astype(np.float32)
    v = cu(verts)
    R = raster.rasterizer_for(faces, v.shape[0])
    cam, blur = raster.camera_of(cap), raster.default_blur_radius(SIGMA)
    alpha, keep, n_cand = R.silhouette(v, cam, SIGMA, blur, want_count=True)
    g = R.silhouette_backward(v, cam, SIGMA, blur, keep, cu(g_hole))
    h = torch.as_tensor(hole).cuda()
    print(f"[sharp] silhouette torus, sigma {SIGMA:g}: {int(hole.sum())} px in the hole beyond the blur radius; there alpha != 0 at {int((alpha[h] != 0).sum())}, "
          f"n_cand != 0 at {int((n_cand[h] != 0).sum())}; gradient of a loss on the hole alone: largest component {float(g.abs().max()):.1e}")
    assert hole.sum() >= 100
    assert bool((alpha[h] == 0).all()) and bool((keep[h] == 1).all()) and bool((n_cand[h] == 0).all())
    assert bool((g == 0).all())


def test_silhouette_batch_of_two_torus_views():
    """the batched entry on (torus view A, torus view B): the one-frame entries' bits, forward and backward"""
    from neuman_hip import raster
    s = SS.shape('torus')
    faces = np.array(s['faces'])
    verts = cu(s['verts'])[None].expand(2, -1, 3).contiguous()
    caps = [SS.capture(c, 96, 64) for c in SS.TORUS_HOLE_CAMERAS]
    R = raster.Rasterizer(faces, verts.shape[1])
    g = TQ._g_alpha(2, 64, 96)
    one = TQ._one_by_one(R, verts, caps, SIGMA, g)
    bat = TQ._batched(R, verts, caps, SIGMA, g)
    for b in range(2):
        assert int((one[0][b] > 0).sum()) > 50 and float(one[3][b].abs().max()) > 0 and _hole(one[2][b].cpu().numpy() > 0).sum() >= 100
    assert not torch.equal(one[0][0], one[0][1])
    TQ._same(bat, one, 'torus views A, B')
    R.close()
    print(f"[sharp] silhouette batch, torus from {SS.TORUS_HOLE_CAMERAS}: alpha, keep, n_cand and g_verts of both frames the one-frame entries' bits; alpha > 0 on "
          f"{[int((one[0][b] > 0).sum()) for b in range(2)]} px, holes of {[int(_hole(one[2][b].cpu().numpy() > 0).sum()) for b in range(2)]} px")
