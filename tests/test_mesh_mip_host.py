"""Without a device: nm_mesh_lattice_pyramid_size, nm_mesh_lattice_pyramid and nm_raster_frames_lattice_mip (csrc/mesh_lattice.hip,
csrc/raster_frames.hip; the header's 'mesh mip') in the header, in `_lib.SIGNATURES` and in the library, their refusals and the Python layer's;
tests/helpers/mesh_mip_ref.py (rules M1-M3 in numpy) on closed forms; and the condition of the quality test of tests/test_hip_mesh_mip.py shown
for the helper alone ([mesh mip] line: the ratio profiles/mesh_mip.md quotes)."""
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
import mesh_mip_ref as MR  # noqa: E402
import mesh_simplify_ref as MS  # noqa: E402
import raster_ref as RR  # noqa: E402

from neuman_hip import _lib  # noqa: E402

ARITY = {"nm_mesh_lattice_pyramid_size": 3, "nm_mesh_lattice_pyramid": 7, "nm_raster_frames_lattice_mip": 20}


@pytest.mark.parametrize("name", list(ARITY))
def test_the_entries_are_declared_bound_and_exported_with_matching_arity(name):
    src = open(os.path.join(HERE, "..", "include", "neuman_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in neuman_hip.h"
    assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == ARITY[name]


def test_the_level_counts_and_the_pyramid_sizes():
    from neuman_hip import mesh_texture
    assert [mesh_texture.lattice_levels(R) for R in (1, 2, 3, 4, 6, 8, 12, 16, 48, 63, 64)] == [1, 2, 1, 3, 2, 4, 3, 5, 5, 1, 7]
    # what lattice_pyramid makes by default: without a coarsest level of resolution 1 (corners alone, which rule M1 copies), at least one
    assert [mesh_texture.filtered_levels(R) for R in (1, 2, 3, 4, 6, 8, 12, 16, 48, 63, 64)] == [1, 1, 1, 2, 2, 3, 3, 4, 5, 1, 6]
    for R in range(1, 65):
        k = mesh_texture.filtered_levels(R)
        assert 1 <= k <= mesh_texture.lattice_levels(R) and (k == 1 or R >> (k - 1) >= 2) and (k == mesh_texture.lattice_levels(R) or R >> k == 1)
    for R in (0, 65, -2, 8.0, True):
        with pytest.raises(ValueError):
            mesh_texture.lattice_levels(R)
    lib = _lib.lib()
    for R in range(1, 65):
        assert mesh_texture.lattice_levels(R) == MR.lattice_levels(R)
        for levels in range(1, MR.lattice_levels(R) + 1):
            total = ctypes.c_int64(-1)
            assert lib.nm_mesh_lattice_pyramid_size(R, levels, ctypes.byref(total)) == 0
            assert total.value == MR.nodes_before(R, levels) == sum((((R >> l) + 1) * ((R >> l) + 2)) // 2 for l in range(levels))
        total = ctypes.c_int64(-1)
        for levels in (0, -1, MR.lattice_levels(R) + 1):
            assert lib.nm_mesh_lattice_pyramid_size(R, levels, ctypes.byref(total)) == -1 and b"nm_mesh_lattice_pyramid_size:" in lib.nm_last_error()
        assert total.value == -1                                                    # nothing is written by a refused call
    total = ctypes.c_int64(-1)
    for R in (0, -8, 65, 128):
        assert lib.nm_mesh_lattice_pyramid_size(R, 1, ctypes.byref(total)) == -1
    assert lib.nm_mesh_lattice_pyramid_size(8, 4, None) == -1
    assert total.value == -1
    assert MR.nodes_before(8, 4) == 45 + 15 + 6 + 3 and MR.nodes_before(64, 7) == 2145 + 561 + 153 + 45 + 15 + 6 + 3


def test_every_refusal_comes_before_any_device_work():
    lib = _lib.lib()
    dummy = (ctypes.c_char * 256)()                                     # stands in for every device pointer: the checks run before any is read
    d = ctypes.cast(dummy, ctypes.c_void_p)
    good = dict(lattice=d, F=4, R0=8, levels=4, w=3, out=d)
    bad = [dict(lattice=None), dict(out=None), dict(w=0), dict(w=-1), dict(w=65), dict(R0=0), dict(R0=-8), dict(R0=65), dict(levels=0), dict(levels=-1),
           dict(levels=5), dict(R0=6, levels=3), dict(R0=7, levels=2), dict(R0=64, levels=8), dict(F=0), dict(F=-1), dict(F=1 << 31), dict(F=(1 << 31) // 3 + 1)]
    for over in bad:
        k = dict(good, **over)
        rc = lib.nm_mesh_lattice_pyramid(k['lattice'], k['F'], k['R0'], k['levels'], k['w'], k['out'], None)
        assert rc == -1 and b"nm_mesh_lattice_pyramid:" in lib.nm_last_error(), over
    nan, inf = float('nan'), float('inf')
    as_d = lambda *x: (ctypes.c_double * 3)(*x)                         # noqa: E731
    good = dict(h=d, verts=d, w2c=d, intr=d, B=2, W=8, H=8, pyr=d, R0=8, levels=4, lod=1.0, normals=d, light=as_d(2, 2, -2), bg=d, bg_z=d, out=d, face_id=d, zbuf=d,
                bary=d)
    bad = [dict(h=None), dict(verts=None), dict(w2c=None), dict(intr=None), dict(out=None), dict(B=0), dict(B=-3), dict(B=1 << 16), dict(W=0), dict(H=0),
           dict(W=-1), dict(W=1 << 16, H=1 << 16), dict(light=None), dict(normals=None), dict(light=as_d(nan, 0, 0)), dict(light=as_d(0, inf, 0)),
           dict(pyr=None), dict(R0=0), dict(R0=-1), dict(R0=65), dict(levels=0), dict(levels=-1), dict(levels=5), dict(R0=12, levels=4), dict(R0=5, levels=2),
           dict(levels=8, R0=64), dict(levels=40), dict(lod=nan), dict(lod=inf), dict(lod=-inf), dict(lod=-1.0), dict(lod=-1e-30)]
    for over in bad:
        k = dict(good, **over)
        rc = lib.nm_raster_frames_lattice_mip(k['h'], k['verts'], k['w2c'], k['intr'], k['B'], k['W'], k['H'], k['pyr'], k['R0'], k['levels'], k['lod'],
                                              k['normals'], k['light'], k['bg'], k['bg_z'], k['out'], k['face_id'], k['zbuf'], k['bary'], None)
        assert rc == -1 and b"nm_raster_frames_lattice_mip:" in lib.nm_last_error(), over


class _Fake(torch.Tensor):
    """a CPU tensor that says it lives on the device (tests/test_raster_frames_host.py): the layer's checks run, on a box without one, up to the
    first call that needs it"""
    is_cuda = True


def _tensor(*shape, dtype=torch.float32):
    if torch.cuda.is_available():
        return torch.zeros(*shape, dtype=dtype, device='cuda')
    return torch.zeros(*shape, dtype=dtype).as_subclass(_Fake)


def test_the_python_layer_refuses_a_lod_scale_without_a_pyramid_and_what_is_no_lattice():
    from neuman_hip import mesh_texture, raster, render_utils, synthetic
    faces = np.array([[0, 1, 2]])
    caps = [synthetic.SimpleCapture(8, 6, c2w=synthetic.spherical_c2w(30., -20., 1.3)) for _ in range(2)]
    v = _tensor(2, 3, 3)
    for kw in (dict(face_colours=_tensor(1, 6, 3)), dict(colours=_tensor(3, 3)), dict()):
        with pytest.raises(ValueError, match="lod_scale goes with a LatticePyramid"):
            render_utils.render_mesh_frames(v, faces, caps, lod_scale=1.0, **kw)
    pyr = mesh_texture.LatticePyramid(_tensor(2 * 9 * 3), 2, 2, 2, 3)                # another mesh's: two faces
    with pytest.raises(_lib.NeumanHipError, match="pyramid of a"):
        render_utils.render_mesh_frames(v, faces, caps, face_colours=pyr)
    with pytest.raises(_lib.NeumanHipError, match="pyramid of a"):
        render_utils.render_mesh_frames(v, faces, caps, face_colours=mesh_texture.LatticePyramid(_tensor(9 * 4), 2, 2, 1, 4))      # four columns: no colours
    pyr = mesh_texture.LatticePyramid(_tensor(9 * 3), 2, 2, 1, 3)
    with pytest.raises(ValueError, match="not both"):
        render_utils.render_mesh_frames(v, faces, caps, colours=_tensor(3, 3), face_colours=pyr)
    for lod in ("1", True, None.__class__):
        with pytest.raises(ValueError, match="lod_scale must be a number"):
            render_utils.render_mesh_frames(v, faces, caps, face_colours=pyr, lod_scale=lod)
    assert tuple(pyr.level(0).shape) == (1, 6, 3) and tuple(pyr.level(1).shape) == (1, 3, 3)
    assert pyr.level(1).data_ptr() == pyr.data.data_ptr() + 4 * 18 and pyr.level(1).is_contiguous()
    for k in (-1, 2, 1.0, True):
        with pytest.raises(ValueError):
            pyr.level(k)
    assert raster.lattice_resolution_of(pyr.level(1), 1, "t") == 1                   # a level is a lattice like any other
    for bad in (torch.zeros(1, 6, 3), np.zeros((1, 6, 3), np.float32)):             # CPU: there is no CPU path
        with pytest.raises(_lib.NeumanHipError, match="CUDA"):
            mesh_texture.lattice_pyramid(bad)
    for bad in (_tensor(1, 5, 3), _tensor(6, 3), _tensor(1, 6, 65), _tensor(1, 6, 3, dtype=torch.float64), _tensor(0, 6, 3)):
        with pytest.raises(_lib.NeumanHipError, match="face_colours must be"):
            mesh_texture.lattice_pyramid(bad)
    for levels in (0, 3, -1, 2.0, True):                                            # R = 2 allows 1 or 2
        with pytest.raises(ValueError, match="levels must be"):
            mesh_texture.lattice_pyramid(_tensor(1, 6, 3), levels)


# ---- the helper on closed forms ----------------------------------------------------------------------------------------------------------------
TRI = np.array([[0.1, 0.2, 0.3], [1.0, -0.5, 0.7], [0.4, 0.9, -0.2], [2.0, 1.0, 0.5], [-1.0, 0.3, 0.8]])
FACES = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 2], [3, 4, 1], [0, 3, 4]])


def test_which_nodes_a_level_has():
    """R0 = 4 is the smallest with an edge node in a coarser level (level 1, R = 2: its three mid-edge nodes), R0 = 6 the smallest with an
    interior one (level 1, R = 3: node (1, 1)); a one-hot fine lattice shows the weights"""
    for R0, want in ((2, (3, 0, 0)), (4, (3, 3, 0)), (6, (3, 6, 1)), (8, (3, 9, 3)), (64, (3, 93, 465))):
        i1, i2 = LR.nodes(R0 // 2)
        zeros = (i1 == 0).astype(int) + (i2 == 0) + (R0 // 2 - i1 - i2 == 0)
        assert ((zeros == 2).sum(), (zeros == 1).sum(), (zeros == 0).sum()) == want
    R0 = 6
    S = LR.lattice_size(R0)
    hot = np.eye(S, dtype=np.float32)[None]                                         # [1,S,S]: column k is the lattice that is 1 at node k
    W = MR.reduce(hot)[0]                                                           # [S(3),S]: row = coarse node, the weights of the fine nodes
    assert np.array_equal(W.sum(1), np.ones(LR.lattice_size(3), np.float32))        # every coarse node is an average
    n = lambda a, b: LR.node_index(R0, a, b)                                        # noqa: E731
    c = lambda a, b: LR.node_index(3, a, b)                                         # noqa: E731
    assert W[c(0, 0), n(0, 0)] == 1 and W[c(3, 0), n(6, 0)] == 1 and W[c(0, 3), n(0, 6)] == 1
    assert (W[c(1, 0), n(2, 0)], W[c(1, 0), n(1, 0)], W[c(1, 0), n(3, 0)]) == (0.5, 0.25, 0.25)                  # the edge i2 = 0
    assert (W[c(0, 2), n(0, 4)], W[c(0, 2), n(0, 3)], W[c(0, 2), n(0, 5)]) == (0.5, 0.25, 0.25)                  # the edge i1 = 0
    assert (W[c(2, 1), n(4, 2)], W[c(2, 1), n(3, 3)], W[c(2, 1), n(5, 1)]) == (0.5, 0.25, 0.25)                  # the hypotenuse
    inner = W[c(1, 1)]
    assert inner[n(2, 2)] == 0.25 and all(inner[n(2 + a, 2 + b)] == 0.125 for a, b in ((1, 0), (0, 1), (-1, 1), (-1, 0), (0, -1), (1, -1)))
    assert (inner != 0).sum() == 7


@pytest.mark.parametrize("R0", [2, 4, 6, 8, 12, 64])
def test_a_linear_lattice_stays_linear_at_every_level(R0):
    values = np.random.default_rng(R0).standard_normal((5, 4)).astype(np.float32)
    pyr = MR.pyramid(LR.rows(values, FACES, R0, np.float32))
    assert len(pyr) == MR.lattice_levels(R0) and [a.shape[1] for a in pyr] == [LR.lattice_size(R0 >> l) for l in range(len(pyr))]
    for l, got in enumerate(pyr):
        want = LR.rows(values, FACES, R0 >> l, np.float64)
        assert got.dtype == np.float32 and np.abs(got - want).max() < 4e-7 * np.abs(values).max() * (l + 1)
        R = R0 >> l
        corners = [LR.node_index(R, 0, 0), LR.node_index(R, R, 0), LR.node_index(R, 0, R)]
        assert np.array_equal(got[:, corners], values[FACES])                       # corners are copies all the way down


def test_faces_that_agree_on_a_shared_edge_agree_on_it_at_every_level():
    R0 = 8
    lat = np.random.default_rng(3).random((2, LR.lattice_size(R0), 3)).astype(np.float32)
    # face 0 = (0, 1, 2), face 1 = (2, 1, 3): the edge 1-2 is face 0's hypotenuse (i1 = R - k, i2 = k) and face 1's edge i2 = 0, run backwards
    for k in range(R0 + 1):
        lat[1, LR.node_index(R0, k, 0)] = lat[0, LR.node_index(R0, k, R0 - k)]
    for l, level in enumerate(MR.pyramid(lat)):
        R = R0 >> l
        for k in range(R + 1):
            assert np.array_equal(level[1, LR.node_index(R, k, 0)], level[0, LR.node_index(R, k, R - k)]), (l, k)


def test_the_level_of_a_face_from_its_size_on_the_screen():
    faces = np.array([[0, 1, 2]])
    for dtype in (np.float32, np.float64):
        for h, want_l, want_t in ((16.0, 0, 0.0), (8.0, 0, 0.0), (6.4, 0, 0.25), (4.0, 1, 0.0), (2.0, 2, 0.0), (1.6, 2, 0.25), (1.0, 3, 0.0), (0.0625, 3, 0.0)):
            sv = np.array([[10.0, 5.0], [10.0 + 3 * h, 5.0], [10.0 + h, 5.0 + h]])      # longest edge 3 h, height h: rho = 8 / h at R0 = 8
            l, t, rho = MR.level_of(sv, faces, [0], 8, 4, 1.0, dtype)
            assert (l[0], rho.dtype) == (want_l, dtype) and abs(t[0] - want_t) < 1e-6 and abs(rho[0] - 8 / h) < 1e-5 * 8 / h, (h, l, t, rho)
            assert MR.level_of(sv[[2, 0, 1]], faces, [0], 8, 4, 1.0, dtype)[0][0] == want_l      # whichever vertex comes first
            l, t, _ = MR.level_of(sv, faces, [0], 8, 2, 1.0, dtype)                     # fewer levels: the walk stops at the coarsest, t = 0 there
            assert l[0] == min(want_l, 1) and (t[0] == 0 if want_l >= 1 else abs(t[0] - want_t) < 1e-6)
            l, t, _ = MR.level_of(sv, faces, [0], 8, 4, 0.0, dtype)
            assert (l[0], t[0]) == (0, 0)                                               # lod_scale = 0: the plain lattice
            l, t, rho = MR.level_of(sv, faces, [0], 8, 4, 1e30, dtype)
            assert (l[0], t[0]) == (3, 0)                                               # a huge one: the coarsest level
        flat_face = np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]])                      # no area: rho = x / 0
        l, t, rho = MR.level_of(flat_face, faces, [0], 8, 4, 1.0, dtype)
        assert np.isposinf(rho[0]) and (l[0], t[0]) == (3, 0)
        l, t, rho = MR.level_of(flat_face, faces, [0], 8, 4, 0.0, dtype)                # 0 / 0
        assert np.isnan(rho[0]) and (l[0], t[0]) == (0, 0)
    assert MR.near_power_of_two(np.array([2.0, 4.00003, 4.0001, 1.0, 3.0, np.nan, np.inf, 0.0, 7.99995])).tolist() == [True, True, False, False, False, False,
                                                                                                                       False, False, True]


# ---- the quality test's condition, for the helper alone ----------------------------------------------------------------------------------------
def thinned_capsule():
    """the capsule of the quality test thinned by tests/helpers/mesh_simplify_ref.py -> (verts float32 [K,3], faces int64 [F',3])"""
    from neuman_hip import synthetic
    verts, faces = synthetic.capsule_mesh(*LR.STRIPE_SHAPE)
    lo, h, dims = MS.grid(LR.STRIPE_BOX, LR.STRIPE_CELL)
    thin = MS.simplify(verts, faces, lo, h, dims)
    return thin['verts'], thin['faces'].astype(np.int64)


def test_the_minified_stripe_condition_holds_for_the_helper_with_the_default_levels():
    """Stripes of half a mean edge per period (four node spacings at R = 8), drawn from so far that a period is 1.25 pixels: the plain lattice
    point-samples a pattern the pixel grid cannot carry.  The mean absolute error against the 4 x supersampled, box-averaged source must be
    lower with the pyramid `lattice_pyramid` makes by default (`filtered_levels`: 8, 4, 2) at lod_scale 1 than with the plain lattice; that
    ratio is the one tests/test_hip_mesh_mip.py holds the device to and profiles/mesh_mip.md quotes.

    Measured here (195 vertices, 386 faces, 517 fully covered pixels in the three frames): plain 0.17574; the default pyramid at lod_scale
    0.5: 0.11034, 1: 0.14571 (ratio 0.8291), 2: 0.14620.  With the R = 1 level included (levels=4) -- 0.5: 0.12134, 1: 0.21176 (ratio
    1.2049), 2: 0.24587: worse than the plain lattice, because that level is the three corners, which rule M1 copies, so faces small enough
    to reach it show the stripes point-sampled at the vertices (that level alone scores 0.246, a flat grey 0.139, level 1 alone 0.100).
    Hence the default; the figures of the full pyramid are printed, not asserted."""
    from neuman_hip import mesh_texture
    verts, faces = thinned_capsule()
    wavelength = MR.stripe_wavelength(verts, faces)
    R0 = LR.STRIPE_R
    lattice = LR.stripes(LR.rows(verts, faces, R0, np.float32).reshape(-1, 3), wavelength).astype(np.float32).reshape(len(faces), -1, 3)
    pyr = MR.pyramid(lattice)
    usual = mesh_texture.filtered_levels(R0)
    assert (len(pyr), usual) == (4, 3)
    arms = [(levels, lod) for levels in (usual, 4) for lod in (0.5, 1.0, 2.0)]
    err = dict.fromkeys(['plain'] + arms, 0.0)
    n, seen = 0, set()
    for cap, big in zip(MR.far_cameras(wavelength), MR.far_cameras(wavelength, MR.SUPER)):
        cam = RR.camera_of(cap)
        sup = RR.rasterize(verts, faces, RR.camera_of(big), np.float32)
        truth, full = MR.box_truth(sup['face_id'], sup['bary'], verts, faces, wavelength)
        fr = LR.frame(verts, faces, cam, np.float32)
        full &= fr['face_id'] >= 0
        e, k = MR.mean_abs_error(LR.shade(fr, lattice, R0, np.float32, lit=False)['out'], truth, full)
        err['plain'], n = err['plain'] + e, n + k
        for levels, lod in arms:
            mip = MR.shade(fr, pyr[:levels], R0, lod, MR.screen_vertices(verts, cam), faces, np.float32, lit=False)
            err[levels, lod] += MR.mean_abs_error(mip['out'], truth, full)[0]
            if (levels, lod) == (usual, 1.0):
                seen |= set(np.unique(mip['level'][full]).tolist())
    print(f"[mesh mip] helper: {len(verts)} vertices, {len(faces)} faces, wavelength {wavelength:.4f} = {MR.STRIPE_PIXELS} px; {n // 3} fully covered pixels in the "
          f"three frames, levels seen {sorted(seen)}; mean |colour error| plain R = {R0} lattice {err['plain'] / n:.5f}, pyramid "
          + ", ".join(f"{levels} levels at lod_scale {lod}: {err[levels, lod] / n:.5f}" for levels, lod in arms)
          + f"; ratio of the default at lod_scale 1: {err[usual, 1.0] / err['plain']:.4f}, of all 4 levels: {err[4, 1.0] / err['plain']:.4f}")
    assert n // 3 > 300 and len(seen) >= 2
    assert err[usual, 1.0] < err['plain']
