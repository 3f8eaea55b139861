"""Without a device: the mesh smoothing entry points' argument checks (before any device work), the workspace's size against the header's
figures, the Python surface's refusals, the size table of tests/helpers/smooth_sizes.py against the kernels' source, and the numpy
restatement of the contract (tests/helpers/mesh_smooth_ref.py) on meshes whose answers are known -- the yardstick of
tests/test_hip_mesh_smooth.py, checked where it can run."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import isosurface_ref as IR  # noqa: E402
import mesh_components_ref as MR  # noqa: E402
import mesh_smooth_ref as SR  # noqa: E402
import smooth_sizes as SS  # noqa: E402

from neuman_hip import _lib, mesh_extract, mesh_smooth  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
TOO_MANY = 1 << 31

OCTA_VERTS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCTA_FACES = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)      # outward


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


# ---- the size table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SS.TABLE))
def test_size_table_matches_the_source(name):
    value, path, pattern = SS.TABLE[name]
    with open(os.path.join(ROOT, path)) as f:
        found = re.findall(pattern, f.read())
    assert found, f"{name}: {pattern!r} matches no line of {path}: the table in tests/helpers/smooth_sizes.py is stale"
    for groups in found:
        product = 1
        for g in (groups if isinstance(groups, tuple) else (groups,)):
            product *= int(g)
        assert product == value, f"{name}: {path} now says {product}, the table {value}"


def test_every_derived_size_is_past_its_threshold():
    C = SS.C
    src = ''
    for path in (SS.TABLE['SPAN'][1], SS.CSRC + 'mesh_smooth.hip'):               # the shared header, then the file that launches its kernels
        with open(os.path.join(ROOT, path)) as f:
            src += f.read()
    assert re.search(r'span_scan_kernel, dim3\(1\), dim3\(kThreads\)', src) and not re.search(r'span_scan_kernel, dim3\(1\), dim3\(\d', src)
    assert re.search(r'if \(n <= kSortInThread\)', src)                               # the threshold is inclusive: SORT entries are the last in-thread
    assert C.SPAN % C.THREADS == 0
    rows, cols = SS.GRID_SMALL
    assert rows * cols == SS.TWO_SPANS_AND_ONE == 2 * C.SPAN + 1 and SS.spans(rows * cols) == 3
    rows, cols = SS.GRID_PAST_THE_SCAN
    V = rows * cols
    assert V > C.SPAN * C.THREADS and SS.spans(V) > C.THREADS and SS.per_thread(SS.spans(V)) == 2      # a scan thread owns two spans
    assert V % C.SPAN != 0                                                            # ... and the last span is not full
    assert SS.CONE_JUST_PAST == C.SORT + 1 and SS.CONE_FAR_PAST == 4 * C.SORT
    assert SS.CONE_NEIGHBOURS_PAST <= C.SORT < 2 * SS.CONE_NEIGHBOURS_PAST            # the list in-thread, its neighbour ids not
    for valence in (SS.CONE_NEIGHBOURS_PAST, SS.CONE_JUST_PAST, SS.CONE_FAR_PAST):
        for apex_last in (False, True):
            verts, faces, apex = SS.cone(valence, apex_last)
            off, inc, boundary = SR.adjacency(faces, verts.shape[0])
            k = np.diff(off)
            assert k[apex] == valence and 2 * valence > C.SORT and (np.delete(k, apex) == 2).all()      # the apex alone takes the heap sort
            fill_order = np.flatnonzero((faces == apex).any(1))                       # = every face, in index order ...
            assert np.array_equal(inc[off[apex]:off[apex + 1]], fill_order) and (np.diff(faces[:, 1]) < 0).any()      # ... which is not the rim's order
    # an interior vertex of the grid: six faces, twelve neighbour ids -- in-thread; nothing on a grid reaches the heap sort
    verts, faces = SS.grid_mesh(*SS.GRID_SMALL)
    assert np.diff(SR.adjacency(faces, verts.shape[0])[0]).max() == 6 and 2 * 6 <= C.SORT


# ---- the entry points' refusals -----------------------------------------------------------------------------------------------------------
def _host_block(nbytes):
    block = (ctypes.c_char * (nbytes + 64))()
    return block, ctypes.c_void_p((ctypes.addressof(block) + 15) // 16 * 16)


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    lib = _lib.lib()
    too_many_faces = (TOO_MANY + 2) // 3                                              # the smallest F with 3 F >= 2^31
    for V, F in ((-1, 4), (4, -1), (TOO_MANY, 4), (4, too_many_faces), (4, TOO_MANY)):
        assert lib.nm_mesh_adjacency_workspace_bytes(V, F) == -1 and b"nm_mesh_adjacency_workspace_bytes" in lib.nm_last_error(), (V, F)
    assert lib.nm_mesh_adjacency_workspace_bytes(TOO_MANY - 1, too_many_faces - 1) > 0
    V, F = 9, 7
    nbytes = lib.nm_mesh_adjacency_workspace_bytes(V, F)
    assert 0 < nbytes <= 1000
    # the checks run before any pointer is looked at: a block of host memory stands in for the device arrays
    block, d = _host_block(8192)
    at = lambda k: ctypes.c_void_p(d.value + 1024 * k)                                # distinct, non-overlapping stand-ins
    n = ctypes.c_int64(-7)
    good = dict(faces=at(0), F=F, V=V, inc_off=at(1), inc=at(2), boundary=at(3), ws=d, nbytes=nbytes)
    sizes = [dict(F=-1), dict(V=-1), dict(F=too_many_faces), dict(V=TOO_MANY)]
    space = [dict(ws=None), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(ws=ctypes.c_void_p(d.value + 4))]
    for over in [dict(faces=None), dict(inc_off=None), dict(inc=None)] + sizes + space:
        a = dict(good, **over)
        rc = lib.nm_mesh_adjacency(a['faces'], a['F'], a['V'], a['inc_off'], a['inc'], a['boundary'], a['ws'], a['nbytes'], ctypes.byref(n), None)
        assert rc == -1 and b"nm_mesh_adjacency:" in lib.nm_last_error(), over
    assert lib.nm_mesh_adjacency(at(0), F, V, at(1), at(2), None, d, nbytes, None, None) == -1 and b"null count pointer" in lib.nm_last_error()
    assert n.value == -7
    # nm_mesh_smooth
    good = dict(rows=at(3), width=3, V=V, faces=at(0), F=F, inc_off=at(1), inc=at(2), hold=None, lam=0.5, mu=-0.53, n=2, out=at(4), scratch=at(5))
    bad = [dict(rows=None), dict(out=None), dict(scratch=None), dict(faces=None), dict(inc_off=None), dict(inc=None), dict(width=0), dict(width=65),
           dict(width=-3), dict(n=-1), dict(lam=float('nan')), dict(lam=float('inf')), dict(mu=float('-inf')), dict(mu=float('nan')),
           dict(out=at(3)), dict(scratch=at(3)), dict(scratch=at(4)),                  # aliased: rows = out, rows = scratch, out = scratch
           dict(out=ctypes.c_void_p(at(3).value + 4 * (V * 3 - 1)))] + sizes          # ... and overlapping by one float
    for over in bad:
        a = dict(good, **over)
        rc = lib.nm_mesh_smooth(a['rows'], a['width'], a['V'], a['faces'], a['F'], a['inc_off'], a['inc'], a['hold'], a['lam'], a['mu'], a['n'], a['out'],
                                a['scratch'], None)
        assert rc == -1 and b"nm_mesh_smooth:" in lib.nm_last_error(), over
    # nm_mesh_vertex_normals
    good = dict(verts=at(3), B=1, V=V, faces=at(0), F=F, inc_off=at(1), inc=at(2), normals=at(4))
    bad = [dict(verts=None), dict(normals=None), dict(faces=None), dict(inc_off=None), dict(inc=None), dict(B=0), dict(B=-1), dict(B=TOO_MANY),
           dict(B=(TOO_MANY + V - 1) // V), dict(normals=at(3))] + sizes
    for over in bad:
        a = dict(good, **over)
        rc = lib.nm_mesh_vertex_normals(a['verts'], a['B'], a['V'], a['faces'], a['F'], a['inc_off'], a['inc'], a['normals'], None)
        assert rc == -1 and b"nm_mesh_vertex_normals:" in lib.nm_last_error(), over
    # no vertex: nothing to do, no pointer needed
    assert lib.nm_mesh_smooth(None, 3, 0, None, 0, None, None, None, 0.5, -0.53, 4, None, None, None) == 0
    assert lib.nm_mesh_vertex_normals(None, 2, 0, None, 0, None, None, None, None) == 0
    del block


def test_workspace_matches_the_headers_figures():
    """4 bytes per vertex, 24 per face, 16 per span of vertices, 64 of header (+ padding below 32); under the ceiling of 8 V + 24 F + 256"""
    lib = _lib.lib()
    with open(os.path.join(ROOT, "include", "neuman_hip.h")) as f:
        header = f.read()
    m = re.search(r"nm_mesh_adjacency_workspace_bytes\(V, F\) bytes = (\d+) bytes per vertex .*?\+ (\d+) bytes per face .*?\+ (\d+) bytes per (\d+) vertices "
                  r".*?\+ (\d+) and\s+\*?\s*padding below (\d+)", header, re.S)
    assert m, "the header no longer states the workspace's size in this form"
    per_vertex, per_face, per_span, span, head, pad = (int(g) for g in m.groups())
    assert (per_vertex, per_face, span) == (4, 24, SS.C.SPAN)
    for V, F in ((0, 0), (1, 0), (0, 1), (21, 18), (1000, 2001), (262656, 523264), (3_000_001, 6_000_007), (TOO_MANY - 1, (TOO_MANY - 1) // 3)):
        stated = per_vertex * V + per_face * F + per_span * SS.spans(V) + head
        got = lib.nm_mesh_adjacency_workspace_bytes(V, F)
        assert stated <= got < stated + pad and got % 16 == 0, (V, F, got, stated)
        assert got <= 8 * V + 24 * F + 256


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    if torch.cuda.is_available():
        pytest.skip("GPU box: the refusal path is exercised on the CPU-only runner")
    verts, faces = torch.from_numpy(OCTA_VERTS), torch.from_numpy(OCTA_FACES)
    with pytest.raises(_lib.NeumanHipError):
        mesh_smooth.adjacency(faces, 6)
    with pytest.raises(_lib.NeumanHipError):
        mesh_smooth.adjacency(OCTA_FACES, 6)
    with pytest.raises(_lib.NeumanHipError):
        mesh_smooth.smooth_mesh(verts, faces)
    with pytest.raises(_lib.NeumanHipError):
        mesh_smooth.smooth_mesh(verts, faces, iterations=0)
    with pytest.raises(_lib.NeumanHipError):
        mesh_smooth.vertex_normals(verts, faces)
    with pytest.raises(_lib.NeumanHipError):
        mesh_smooth.vertex_normals(verts[None], faces)


def test_extract_net_mesh_refuses_a_bad_smooth_before_the_net_is_looked_at():
    for bad in (-1, 1.5, True, None, '3'):
        with pytest.raises(ValueError):
            mesh_extract.extract_net_mesh(None, SS.SPHERE_BOX, 8, 0.5, smooth=bad)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_restatement_on_the_octahedron():
    """every vertex's neighbours are the four of the equator around its axis, which sum to zero: one step with t gives exactly (1 - t) x,
    and the area-weighted normals are the unit axes"""
    off, inc, boundary = SR.adjacency(OCTA_FACES, 6)
    assert off.tolist() == [0, 4, 8, 12, 16, 20, 24] and not boundary.any() and off.dtype == inc.dtype == np.int32 and boundary.dtype == np.uint8
    assert inc[off[4]:off[5]].tolist() == [0, 1, 2, 3] and inc[off[0]:off[1]].tolist() == [0, 3, 4, 7]
    got = SR.step(OCTA_VERTS, OCTA_FACES, 0.5)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits((OCTA_VERTS * np.float32(0.5)).astype(np.float32) + np.float32(0)))
    assert np.array_equal(SR.smooth(OCTA_VERTS, OCTA_FACES, 1, 0.5, 0.0), got)
    assert np.array_equal(SR.smooth(OCTA_VERTS, OCTA_FACES, 0, 0.5, -0.53), OCTA_VERTS)
    two = SR.smooth(OCTA_VERTS, OCTA_FACES, 1, 0.5, -1.0)                             # then (1 + 1) x 0.5 x: back where it was
    assert np.array_equal(two, OCTA_VERTS)
    assert np.array_equal(SR.vertex_normals(OCTA_VERTS, OCTA_FACES), OCTA_VERTS)
    frames = np.stack([OCTA_VERTS, OCTA_VERTS * np.float32(3), -OCTA_VERTS])          # the mirror image turns every face over
    assert np.array_equal(SR.vertex_normals(frames, OCTA_FACES), np.stack([OCTA_VERTS, OCTA_VERTS, OCTA_VERTS]))
    held = SR.step(OCTA_VERTS, OCTA_FACES, 0.5, hold=np.array([0, 1, 0, 0, 0, 1]))
    assert np.array_equal(held[[1, 5]], OCTA_VERTS[[1, 5]]) and not np.array_equal(held, got)


def test_restatement_on_the_hand_written_mesh():
    off, inc, boundary = SR.adjacency(SS.HAND_FACES, SS.HAND_VERTS)
    assert np.array_equal(off, SS.HAND_INC_OFF) and inc.shape == (SS.HAND_N_INCIDENT,) and np.array_equal(boundary, SS.HAND_BOUNDARY)
    assert inc[off[0]:off[1]].tolist() == SS.HAND_LIST_OF_0
    assert all((np.diff(inc[off[v]:off[v + 1]]) > 0).all() for v in range(SS.HAND_VERTS))
    x = SS.hand_rows(3)
    got = SR.smooth(x, SS.HAND_FACES, 1, 0.5, 0.0)
    # a degenerate face and an unreferenced vertex change nothing: the mesh without them gives the same rows, and their vertices keep their bits
    fewer = SS.HAND_FACES[:-1]
    assert np.array_equal(bits(SR.smooth(x, fewer, 1, 0.5, 0.0)), bits(got)) and np.array_equal(bits(got[18:]), bits(x[18:]))
    assert np.array_equal(SR.adjacency(fewer, SS.HAND_VERTS)[0], off) and np.array_equal(SR.adjacency(fewer, SS.HAND_VERTS)[2], boundary)
    # the NaN at vertex 6 reaches its tetrahedron in that column after one step and nothing else
    nan = np.isnan(got)
    assert nan[4:8, 2].all() and nan.sum() == 4
    # vertex 8 has one face (8, 9, 13): by hand
    s = (np.float64(0) + np.float64(x[9, 0])) + np.float64(x[13, 0])
    want = np.float32(np.float64(x[8, 0]) + np.float64(np.float32(0.5)) * (s / 2.0 - np.float64(x[8, 0])))
    assert got[8, 0] == want
    normals = SR.vertex_normals(x, SS.HAND_FACES)
    assert not normals[18:].any() and not normals[4:8].any()                          # an empty list; a sum that is not finite
    assert np.abs(np.linalg.norm(normals[:4].astype(np.float64), axis=1) - 1).max() < 1e-6
    # permuting the faces' rows permutes nothing the boundary depends on
    perm = np.random.default_rng(SS.SEED).permutation(SS.HAND_FACES.shape[0])
    assert np.array_equal(SR.adjacency(SS.HAND_FACES[perm], SS.HAND_VERTS)[2], boundary)
    for bad in (-1, SS.HAND_VERTS, MR.I32_MAX, MR.I32_MIN):
        f = SS.HAND_FACES.copy()
        f[5, 2] = bad
        assert SR.invalid_faces(f, SS.HAND_VERTS).tolist() == [5]
        with pytest.raises(ValueError):
            SR.adjacency(f, SS.HAND_VERTS)


def test_restatement_flags_exactly_the_rim_of_an_open_mesh():
    for rows, cols in ((2, 6), (5, 4), SS.GRID_SMALL):
        verts, faces = SS.grid_mesh(rows, cols)
        off, inc, boundary = SR.adjacency(faces, rows * cols)
        assert np.array_equal(boundary.astype(bool), SS.grid_rim(rows, cols)), (rows, cols)
        assert inc.shape[0] == 3 * faces.shape[0] == 6 * (rows - 1) * (cols - 1)
    for valence in (5, SS.CONE_JUST_PAST):
        verts, faces, apex = SS.cone(valence, apex_last=True)
        boundary = SR.adjacency(faces, valence + 1)[2]
        assert boundary[apex] == 0 and np.delete(boundary, apex).all()
    # held rim: the interior of the grid moves, the rim keeps its bits
    verts, faces = SS.grid_mesh(5, 4)
    rim = SS.grid_rim(5, 4)
    got = SR.smooth(verts, faces, 2, 0.5, -0.53, hold=rim)
    assert np.array_equal(got[rim], verts[rim]) and (got[~rim] != verts[~rim]).any(1).all()


def test_the_property_tests_conditions_hold_for_the_restatement():
    """tests/test_hip_mesh_smooth.py's property test on the same field through the restatements alone: the noisy sphere is one closed piece;
    10 Taubin iterations bring the RMS radial deviation down and move the mean radius less than 10 plain Laplacian steps do; the face normals
    of the smoothed mesh agree in direction with the field's gradient normals at every vertex"""
    m = IR.extract(SS.noisy_sphere_field(), SS.SPHERE_BOX, 0.0)
    verts, faces = m['verts'], m['faces']
    assert MR.labels(faces, m['n_verts'])[2] == 1 and IR.edge_census(faces)[0] and m['n_verts'] > 2 * SS.C.SPAN
    off, inc, boundary = SR.adjacency(faces, m['n_verts'])
    assert not boundary.any() and inc.shape[0] == 3 * m['n_faces']
    taubin = SR.smooth(verts, faces, 10, 0.5, -0.53)
    laplace = SR.smooth(verts, faces, 10, 0.5, 0.0)
    r0, dev0 = SR.radial(verts, SS.SPHERE_CENTRE)
    r1, dev1 = SR.radial(taubin, SS.SPHERE_CENTRE)
    r2, dev2 = SR.radial(laplace, SS.SPHERE_CENTRE)
    assert dev1 < dev0
    assert abs(r1 - r0) < abs(r2 - r0)
    normals = SR.vertex_normals(taubin, faces)
    assert ((normals.astype(np.float64) * m['normals'].astype(np.float64)).sum(1) > 0).all()
    assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1).max() < 1e-6
