"""Without a device: nm_mesh_lattice_rows and nm_raster_frames_lattice (csrc/mesh_lattice.hip, csrc/raster_frames.hip; the header's 'mesh
lattice') in the header, in `_lib.SIGNATURES` and in the library, their refusals and the Python layer's; tests/helpers/mesh_lattice_ref.py
(rules L1-L3 in numpy) on closed forms; and the condition of the quality test of tests/test_hip_mesh_lattice.py shown for the helper alone, with
the ambiguity cap on the images that test renders."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import mesh_lattice_ref as LR  # noqa: E402
import mesh_simplify_ref as MS  # noqa: E402
import raster_ref as RR  # noqa: E402

from neuman_hip import _lib  # noqa: E402

ARITY = {"nm_mesh_lattice_rows": 8, "nm_raster_frames_lattice": 18}


@pytest.mark.parametrize("name", list(ARITY))
def test_the_entries_are_declared_bound_and_exported_with_matching_arity(name):
    src = open(os.path.join(HERE, "..", "include", "neuman_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in neuman_hip.h"
    assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == ARITY[name]


def test_every_refusal_comes_before_any_device_work():
    lib = _lib.lib()
    dummy = (ctypes.c_char * 256)()                                     # stands in for every device pointer: the checks run before any is read
    d = ctypes.cast(dummy, ctypes.c_void_p)
    good = dict(faces=d, F=4, V=5, rows=d, w=3, R=8, out=d)
    bad = [dict(faces=None), dict(rows=None), dict(out=None), dict(w=0), dict(w=-2), dict(R=0), dict(R=-1), dict(R=65), dict(F=0), dict(F=-1),
           dict(F=1 << 31), dict(V=0), dict(V=1 << 31)]
    for over in bad:
        k = dict(good, **over)
        rc = lib.nm_mesh_lattice_rows(k['faces'], k['F'], k['V'], k['rows'], k['w'], k['R'], k['out'], None)
        assert rc == -1 and b"nm_mesh_lattice_rows:" in lib.nm_last_error(), over
    nan, inf = float('nan'), float('inf')
    as_d = lambda *x: (ctypes.c_double * 3)(*x)                         # noqa: E731
    good = dict(h=d, verts=d, w2c=d, intr=d, B=2, W=8, H=8, fc=d, R=4, normals=d, light=as_d(2, 2, -2), bg=d, bg_z=d, out=d, face_id=d, zbuf=d, bary=d)
    bad = [dict(h=None), dict(verts=None), dict(w2c=None), dict(intr=None), dict(out=None), dict(B=0), dict(B=-3), dict(B=1 << 16), dict(W=0), dict(H=0),
           dict(W=-1), dict(W=1 << 16, H=1 << 16), dict(light=None), dict(normals=None), dict(light=as_d(nan, 0, 0)), dict(light=as_d(0, inf, 0)),
           dict(light=as_d(0, 0, -inf)), dict(fc=None), dict(R=0), dict(R=-1), dict(R=65)]
    for over in bad:
        k = dict(good, **over)
        rc = lib.nm_raster_frames_lattice(k['h'], k['verts'], k['w2c'], k['intr'], k['B'], k['W'], k['H'], k['fc'], k['R'], k['normals'], k['light'], k['bg'],
                                          k['bg_z'], k['out'], k['face_id'], k['zbuf'], k['bary'], None)
        assert rc == -1 and b"nm_raster_frames_lattice:" in lib.nm_last_error(), over


class _Fake(torch.Tensor):
    """a CPU tensor that says it lives on the device (tests/test_raster_frames_host.py): the layer's checks run, on a box without one, up to the
    first call that needs it"""
    is_cuda = True


def _tensor(*shape, dtype=torch.float32):
    if torch.cuda.is_available():
        return torch.zeros(*shape, dtype=dtype, device='cuda')
    return torch.zeros(*shape, dtype=dtype).as_subclass(_Fake)


def test_the_python_layer_refuses_both_colour_sources_and_a_second_dimension_that_is_no_lattice_size():
    from neuman_hip import mesh_texture, raster, render_utils, synthetic
    assert [mesh_texture.lattice_size(R) for R in (1, 2, 3, 8, 64)] == [3, 6, 10, 45, 2145]
    for R in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError):
            mesh_texture.lattice_size(R)
    for S in range(1, 2200):
        Rs = [R for R in range(1, 65) if LR.lattice_size(R) == S]
        if Rs:
            assert raster.lattice_resolution_of(torch.zeros(7, S, 3), 7, "t") == Rs[0]
        else:
            with pytest.raises(_lib.NeumanHipError, match="face_colours must be"):
                raster.lattice_resolution_of(torch.zeros(7, S, 3), 7, "t")
    for shape in ((6, 6, 3), (7, 6, 4), (7, 6), (7, 2211, 3)):             # another mesh's; four channels; no channels; R = 65
        with pytest.raises(_lib.NeumanHipError, match="face_colours must be"):
            raster.lattice_resolution_of(torch.zeros(*shape), 7, "t")
    faces = np.array([[0, 1, 2]])
    caps = [synthetic.SimpleCapture(8, 6, c2w=synthetic.spherical_c2w(30., -20., 1.3)) for _ in range(2)]
    v = _tensor(2, 3, 3)
    with pytest.raises(ValueError, match="not both"):
        render_utils.render_mesh_frames(v, faces, caps, colours=_tensor(3, 3), face_colours=_tensor(1, 6, 3))
    for fc in (_tensor(1, 5, 3), _tensor(2, 6, 3), _tensor(1, 6, 3, dtype=torch.float64), torch.zeros(1, 6, 3)):
        with pytest.raises(_lib.NeumanHipError, match="face_colours must be"):
            render_utils.render_mesh_frames(v, faces, caps, face_colours=fc)
    with pytest.raises(ValueError):
        mesh_texture.bake_face_colours(lambda p, d: p, v[0], faces, v[0], 0)
    with pytest.raises(TypeError):
        mesh_texture.bake_face_colours(3.0, v[0], faces, v[0], 2)
    with pytest.raises(ValueError):
        mesh_texture.lattice_resolution(v[0], faces, 0.0)


# ---- the helper on closed forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 6, 7, 8, 64])
def test_the_node_index_is_a_bijection_onto_the_node_count(R):
    S = LR.lattice_size(R)
    pairs = [(i1, i2) for i2 in range(R + 1) for i1 in range(R + 1 - i2)]
    assert len(pairs) == S == (R + 1) * (R + 2) // 2
    assert [LR.node_index(R, i1, i2) for i1, i2 in pairs] == list(range(S))          # rows by i2, row i2 has R + 1 - i2 entries
    i1, i2 = LR.nodes(R)
    assert list(zip(i1.tolist(), i2.tolist())) == pairs
    assert (LR.node_index(R, 0, 0), LR.node_index(R, R, 0), LR.node_index(R, 0, R)) == (0, R, S - 1)      # the corners of vertices 0, 1, 2


def _points(n, seed):
    """random barycentrics (b1, b2) inside the triangle and random faces"""
    rng = np.random.default_rng(seed)
    b = rng.dirichlet((1, 1, 1), n)
    return b[:, 1], b[:, 2], rng.integers(0, 5, n)


TRI = np.array([[0.1, 0.2, 0.3], [1.0, -0.5, 0.7], [0.4, 0.9, -0.2], [2.0, 1.0, 0.5], [-1.0, 0.3, 0.8]])
FACES = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 2], [3, 4, 1], [0, 3, 4]])


@pytest.mark.parametrize("R", [1, 2, 5, 8, 64])
def test_the_lattice_of_an_affine_function_looked_up_anywhere_returns_that_function(R):
    affine = lambda p: p @ np.array([[0.3, -1.0], [0.7, 0.2], [-0.4, 0.5]]) + np.array([0.25, -0.5])      # noqa: E731
    lat = LR.rows(affine(TRI), FACES, R, np.float64)                                # L2 of the vertices' values ...
    pos = LR.rows(TRI, FACES, R, np.float64)
    assert np.abs(lat - affine(pos.reshape(-1, 3)).reshape(lat.shape)).max() < 1e-14   # ... is the function at L2 of the vertices
    b1, b2, f = _points(4000, R)
    got, idx, upper = LR.lookup(lat, f, R, b1, b2)
    p = (1 - b1 - b2)[:, None] * TRI[FACES[f, 0]] + b1[:, None] * TRI[FACES[f, 1]] + b2[:, None] * TRI[FACES[f, 2]]
    assert np.abs(got - affine(p)).max() < 1e-13
    assert (idx >= 0).all() and (idx < LR.lattice_size(R)).all() and (upper.any() or R == 1) and not upper.all()
    got32, _, _ = LR.lookup(lat.astype(np.float32), f, R, b1.astype(np.float32), b2.astype(np.float32), np.float32)
    assert got32.dtype == np.float32 and np.abs(got32 - affine(p)).max() < 2e-5 * R    # the float32 run: u = b R amplifies b's rounding by R


@pytest.mark.parametrize("R", [1, 3, 8, 64])
def test_a_lookup_at_a_node_returns_the_node(R):
    lat = np.random.default_rng(R).random((5, LR.lattice_size(R), 3))
    i1, i2 = LR.nodes(R)
    for f in range(5):
        got, _, _ = LR.lookup(lat, np.full(i1.shape, f), R, i1 / R, i2 / R)
        assert np.abs(got - lat[f]).max() < 1e-13
    if R in (1, 2, 4, 8, 16, 32, 64):                                               # i / R and (i / R) R are exact: the node itself, bit for bit
        lat32 = lat.astype(np.float32)
        got, _, _ = LR.lookup(lat32, np.zeros(i1.shape, np.int64), R, (i1 / R).astype(np.float32), (i2 / R).astype(np.float32), np.float32)
        assert np.array_equal(got, lat32[0])


def test_the_two_sub_triangle_formulas_agree_on_their_shared_edge():
    R = 6
    lat = np.random.default_rng(1).random((1, LR.lattice_size(R), 3))
    t = np.linspace(0.0, 1.0, 41)[1:-1]
    for i1 in range(R - 1):
        for i2 in range(R - 1 - i1):                                                # the cells that have an upper half
            f1, f2 = t, 1.0 - t                                                     # the shared edge: f1 + f2 = 1
            on_edge = (1 - t)[:, None] * lat[0, LR.node_index(R, i1, i2 + 1)] + t[:, None] * lat[0, LR.node_index(R, i1 + 1, i2)]
            for eps, want_upper in ((-1e-9, False), (1e-9, True)):                  # a hair below the edge and a hair above it
                got, _, upper = LR.lookup(lat, np.zeros(t.shape, np.int64), R, (i1 + f1 + eps) / R, (i2 + f2 + eps) / R)
                assert (upper == want_upper).all() and np.abs(got - on_edge).max() < 1e-8
    # the hypotenuse cells have no upper half: f1 + f2 a rounding above 1 there stays in the lower one, with a weight a rounding below 0
    got, idx, upper = LR.lookup(lat, [0], R, [(R - 1 + 0.5) / R], [0.5 / R + 1e-12])
    assert not upper.any() and idx[0].tolist() == [LR.node_index(R, R - 1, 0), LR.node_index(R, R, 0), LR.node_index(R, R - 1, 1)]


def test_resolution_one_blends_the_corners_as_rule_f2_blends_vertex_colours():
    colours = np.random.default_rng(2).random((5, 3))
    lat = LR.rows(colours, FACES, 1, np.float64)
    assert lat.shape == (5, 3, 3) and np.array_equal(lat, colours[FACES])          # the nodes ARE the corners, in the face's vertex order
    b1, b2, f = _points(1000, 3)
    got, idx, upper = LR.lookup(lat, f, 1, b1, b2)
    want = (1 - b1 - b2)[:, None] * colours[FACES[f, 0]] + b1[:, None] * colours[FACES[f, 1]] + b2[:, None] * colours[FACES[f, 2]]
    assert not upper.any() and (idx == [0, 1, 2]).all() and np.abs(got - want).max() < 1e-15
    # barycentrics outside the triangle and a NaN still read nodes of the face
    for R in (1, 4):
        _, idx, _ = LR.lookup(LR.rows(colours, FACES, R, np.float64), [0] * 5, R, [-0.5, 2.0, np.nan, 0.7, np.inf], [2.0, 2.0, 0.3, np.nan, -np.inf])
        assert (idx >= 0).all() and (idx < LR.lattice_size(R)).all()


# ---- the quality test's condition, for the helper alone ----------------------------------------------------------------------------------------
def thinned_capsule():
    """the capsule of the quality test thinned by tests/helpers/mesh_simplify_ref.py -> (verts float32 [K,3], faces int64 [F',3])"""
    from neuman_hip import synthetic
    verts, faces = synthetic.capsule_mesh(*LR.STRIPE_SHAPE)
    lo, h, dims = MS.grid(LR.STRIPE_BOX, LR.STRIPE_CELL)
    thin = MS.simplify(verts, faces, lo, h, dims)
    return verts, thin['verts'], thin['faces'].astype(np.int64)


def test_the_stripe_condition_holds_for_the_helper_and_its_images_keep_the_ambiguity_cap():
    """A sine of four thinned edge lengths per period: per-vertex colours sample it four times per period, an R = 8 lattice 32 times.  Linear
    interpolation's error goes with the spacing squared, so the lattice should be some 64 times nearer; the test asks for 4 times, which
    leaves 16 for faces of uneven size and for the bytes' own step of 1/255."""
    full, verts, faces = thinned_capsule()
    assert 4 * len(verts) < len(full) and len(faces) > 200                          # thinned by more than four, and still a mesh
    wavelength = 4.0 * LR.mean_edge(verts, faces)
    assert 0.2 < wavelength < 0.5                                                   # (more than a period across the capsule's 0.5)
    colours = LR.stripes(verts, wavelength).astype(np.float32)
    lattice = LR.stripes(LR.rows(verts, faces, LR.STRIPE_R, np.float32).reshape(-1, 3), wavelength).astype(np.float32).reshape(len(faces), -1, 3)
    err_v = err_l = n = 0
    for cap in LR.stripe_cameras():
        cam = RR.camera_of(cap)
        r64 = RR.rasterize(verts, faces, cam, analyse=True)                          # the cap of tests/test_raster_frames_host.py, on these images
        cov, amb = int((r64['face_id'] >= 0).sum()), int(r64['ambiguous'].sum())
        assert cov > 500 and amb <= 0.01 * cov, (amb, cov)
        fr = LR.frame(verts, faces, cam, np.float32)
        by_vertex = LR.FR.render(verts, faces, cam, np.float32, colours=colours)
        by_lattice = LR.shade(fr, lattice, LR.STRIPE_R, np.float32, lit=False)
        assert np.array_equal(by_vertex['face_id'], fr['face_id'])
        e_v, k = LR.colour_errors(by_vertex['out'], fr, verts, faces, wavelength)
        e_l, _ = LR.colour_errors(by_lattice['out'], fr, verts, faces, wavelength)
        err_v, err_l, n = err_v + e_v, err_l + e_l, n + k
    print(f"[mesh lattice] helper: {len(verts)} vertices, {len(faces)} faces, wavelength {wavelength:.4f}; mean |colour error| per vertex "
          f"{err_v / n:.5f}, R = {LR.STRIPE_R} lattice {err_l / n:.5f}, ratio {err_l / err_v:.4f}")
    assert err_l < 0.25 * err_v
