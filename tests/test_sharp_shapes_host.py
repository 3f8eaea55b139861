"""CPU: the inputs of tests/test_hip_sharp_shapes.py have the power that file claims (tests/helpers/sharp_shapes.py, float64 only).

Why this file exists: on synthetic.capsule_mesh -- convex, smooth -- the sign of nm_signed_distance comes out right whichever of the seven
vectors of the winning face is read, so tests/test_hip_render.py::test_signed_distance cannot see a swapped edge index, a vertex pseudonormal
from the wrong corner, an edge sum that found no second face or an angle-weighted normal replaced by the face normal
(`test_the_capsule_queries_flip_on_no_slot` keeps that on record).  On the sharp shapes every such substitution flips at least MIN_FLIPS of
the queries the device is held to; that is a condition on the query sets, asserted here, not a measurement.  Each test prints [sharp-host]
lines; profiles/sharp_shapes.md keeps a copy."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import raster_ref as RR  # noqa: E402
import sharp_shapes as SS  # noqa: E402


def test_the_shapes_are_what_the_helper_says():
    sizes = {n: (len(SS.shape(n)['verts']), len(SS.shape(n)['faces'])) for n in SS.CLOSED + SS.UNSIGNED}
    assert sizes['star_prism'] == (22, 40) and sizes['star_prism_fine'][1] == 2560 and sizes['torus'][1] == 1024
    assert sizes['star_prism_swapped'] == sizes['star_prism_fine'] and sizes['star_prism_fin'] == (23, 41)
    fine, swapped = SS.shape('star_prism_fine'), SS.shape('star_prism_swapped')
    assert np.array_equal(fine['faces'], swapped['faces']) and not np.array_equal(fine['verts'], swapped['verts'])      # an nm_mesh_update's target
    for n in SS.CLOSED + SS.UNSIGNED:
        s = SS.shape(n)
        f = s['faces']
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
        directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        _, count = np.unique(e, axis=0, return_counts=True)
        if n in SS.CLOSED:                                                                         # closed, oriented: every edge once each way
            assert (count == 2).all() and len(np.unique(directed, axis=0)) == len(directed), n
            assert SS.signed_volume(s['verts'], f) > 0, n                                          # outward
        elif n == 'star_prism_open':
            assert set(count) == {1, 2} and (count == 1).sum() == 80, n                            # the top rim: 10 edges, split three times
        else:
            assert sorted(set(count)) == [1, 2, 3] and (count == 3).sum() == 1 and (count == 1).sum() == 2, n
        assert np.abs(s['verts']).max() <= 1.0 and (np.ptp(s['verts'], axis=0)[:2] > 0.5).all(), n   # unit scale
    a, b = SS.shape('star_prism'), fine                                                            # the same solid, to the bit
    assert SS.signed_volume(a['verts'], a['faces']) == pytest.approx(SS.signed_volume(b['verts'], b['faces']), rel=1e-14)
    assert np.ptp(SS.shape('thin_plate')['verts'][:, 2]) == pytest.approx(1e-3, rel=1e-6)


@pytest.mark.parametrize("name", SS.CLOSED)
def test_sign_truths_agree_and_few_queries_are_excluded(name):
    s, q, t = SS.shape_truth(name)
    ok = ~t['excluded']
    n_ex = int((~ok).sum())
    neg = t['sign'] < 0
    wn_bad = int(((neg != (t['winding'] > 0.5)) & ok).sum())
    an_bad = int(((neg != t['inside']) & ok).sum()) if 'inside' in t else None
    print(f"[sharp-host] {name}: V {len(s['verts'])}, F {len(s['faces'])}, {len(q)} queries, {neg.mean():.2f} inside, excluded {n_ex} "
          f"({100.0 * n_ex / len(q):.2f} %); feet on face / edge / vertex {int((t['region'] == 0).sum())} / "
          f"{int(((t['region'] >= 1) & (t['region'] <= 3)).sum())} / {int((t['region'] >= 4).sum())}; pseudonormal sign vs winding number: {wn_bad} "
          f"differ, vs the analytic inside test: {'n/a' if an_bad is None else f'{an_bad} differ'}; flips per substituted slot {SS.flips(t)}")
    assert 2900 <= len(q) <= 3100 and q.dtype == np.float32
    assert n_ex <= SS.MAX_EXCLUDED * len(q)
    assert wn_bad == 0
    assert an_bad in (None, 0)
    assert ('inside' in t) == (name != 'torus')
    assert 0.01 < neg.mean() < 0.6 and (t['region'] == 0).sum() > 500 and (t['region'] >= 4).sum() > 50      # both sides, every kind of foot
    if name == 'thin_plate':                                                                        # winner and runner-up within rounding
        mid = np.abs(q[:, 2]) < 2e-3
        assert mid.sum() > 600 and (neg & mid).sum() > 20


@pytest.mark.parametrize("name", SS.UNSIGNED)
def test_open_and_three_face_edges_are_asked_about(name):
    """no inside to compare with: what is asserted is that the queries reach the edges with one and with three faces"""
    s, q, t = SS.shape_truth(name)
    f = s['faces']
    key = np.sort(np.stack([f, np.roll(f, -1, 1)], -1), -1)                                         # [F,3,2]: edge e of face f
    flat, inv, count = np.unique(key.reshape(-1, 2), axis=0, return_inverse=True, return_counts=True)
    on_edge = (t['region'] >= 1) & (t['region'] <= 3)
    faces_on = count[inv.reshape(-1, 3)[t['face'][on_edge], t['region'][on_edge] - 1]]
    want = 1 if name == 'star_prism_open' else 3
    n_ex = int(t['excluded'].sum())
    print(f"[sharp-host] {name}: V {len(s['verts'])}, F {len(f)}, {len(q)} queries, excluded {n_ex}; feet on an edge with 1 / 2 / 3 faces: "
          f"{int((faces_on == 1).sum())} / {int((faces_on == 2).sum())} / {int((faces_on == 3).sum())}; flips per substituted slot {SS.flips(t)}")
    assert (faces_on == want).sum() >= 20 and n_ex <= SS.MAX_EXCLUDED * len(q)


@pytest.mark.parametrize("name", SS.SHARP)
def test_every_wrong_slot_flips_signs_on_the_sharp_shapes(name):
    _, q, t = SS.shape_truth(name)
    fl = SS.flips(t)
    print(f"[sharp-host] {name}: signs flipped of {int((~t['excluded']).sum())} when slot k stands in for the correct vector: "
          + ", ".join(f"{SS.SLOTS[k]} {fl[k]}" for k in range(7)))
    assert min(fl) >= SS.MIN_FLIPS, fl


@pytest.mark.parametrize("case", ["smpl_size", "small"])
def test_the_capsule_queries_flip_on_no_slot(case):
    """the queries tests/test_hip_render.py::test_signed_distance holds to the oracle, through the same function: no substitution shows"""
    verts, faces, pts = SS.capsule_queries(case)
    t = SS.truth(verts, faces, pts, closed=False)
    fl = SS.flips(t)
    print(f"[sharp-host] capsule {case}: F {len(faces)}, signs flipped of {int((~t['excluded']).sum())} per substituted slot: {fl}")
    assert (~t['excluded']).sum() >= 390 and fl == [0] * 7


@pytest.mark.parametrize("name,camera", [("star_prism_fine", SS.STAR_CAMERA), ("torus", SS.TORUS_CAMERA)])
def test_depth_complexity_of_the_raster_views(name, camera):
    s = SS.shape(name)
    for W, H in ((96, 64), (50, 37)):
        cam = RR.camera_of(SS.capture(camera, W, H))
        r64 = RR.rasterize(s['verts'], s['faces'], cam, np.float64, analyse=True)
        count = SS.coverage(s['verts'], s['faces'], cam)
        cov, amb = int((r64['face_id'] >= 0).sum()), int(r64['ambiguous'].sum())
        print(f"[sharp-host] {name} from {camera} at {W} x {H}: covered {cov} px, ambiguous {amb}; pixels under 0, 1, 2, ... faces: {np.bincount(count.ravel()).tolist()}")
        assert np.array_equal(count > 0, r64['face_id'] >= 0)
        assert amb <= 0.01 * cov
        if (W, H) == (96, 64):
            assert (count >= 4).sum() >= 100
        else:
            assert (count >= 4).sum() >= 30
