"""Without a device: the mesh clean-up entry points' argument checks (before any device work), the workspace's size against the header's
figures, the Python surface's refusals, the size table of tests/helpers/component_sizes.py against the kernels' source, and the numpy
restatement of the contract (tests/helpers/mesh_components_ref.py) on meshes whose components are known -- the yardstick of
tests/test_hip_mesh_components.py, checked where it can run."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import component_sizes as CS  # noqa: E402
import isosurface_ref as IR  # noqa: E402
import mesh_components_ref as MR  # noqa: E402

from neuman_hip import _lib, mesh_extract  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
TOO_MANY = 1 << 31


# ---- the size table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CS.TABLE))
def test_size_table_matches_the_source(name):
    value, path, pattern = CS.TABLE[name]
    with open(os.path.join(ROOT, path)) as f:
        found = re.findall(pattern, f.read())
    assert found, f"{name}: {pattern!r} matches no line of {path}: the table in tests/helpers/component_sizes.py is stale"
    for groups in found:
        product = 1
        for g in (groups if isinstance(groups, tuple) else (groups,)):
            product *= int(g)
        assert product == value, f"{name}: {path} now says {product}, the table {value}"


def test_every_derived_size_is_past_its_threshold():
    C = CS.C
    src = ''
    for path in (CS.TABLE['SPAN'][1], CS.CSRC + 'mesh_components.hip'):           # the shared header, then the file that launches its kernels
        with open(os.path.join(ROOT, path)) as f:
            src += f.read()
    assert re.search(r'span_scan_kernel, dim3\(1\), dim3\(kThreads\)', src) and not re.search(r'span_scan_kernel, dim3\(1\), dim3\(\d', src)
    assert C.SPAN % C.THREADS == 0
    assert CS.PAST_ONE_SPAN == C.SPAN + 1 and CS.spans(CS.PAST_ONE_SPAN) == 2
    assert CS.PAST_THE_SCAN == C.SPAN * C.THREADS + 1 == 262145
    assert CS.spans(CS.PAST_THE_SCAN) == C.THREADS + 1 and CS.per_thread(CS.spans(CS.PAST_THE_SCAN)) == 2      # a scan thread owns two spans
    assert CS.STRIP_VERTS == CS.PAST_THE_SCAN
    assert CS.DISJOINT_VERTS == C.SPAN * C.THREADS + 3 and CS.per_thread(CS.spans(CS.DISJOINT_VERTS)) == 2
    n_tri = CS.DISJOINT_VERTS // 3
    assert CS.spans(n_tri) > 64 and CS.DISJOINT_VERTS % 3 == 1                     # many spans of faces and of components; one vertex left over
    assert CS.FAN_FACES >= 65536 and CS.spans(CS.FAN_FACES) >= 64
    a, b = CS.strip_cuts(CS.STRIP_VERTS)
    assert 3 <= a < b - 3 and b <= CS.STRIP_VERTS - 3
    assert CS.spans(a) != CS.spans(b)                                              # the pieces' representatives lie in different spans


# ---- the entry points' refusals -----------------------------------------------------------------------------------------------------------
def _host_block(nbytes):
    block = (ctypes.c_char * (nbytes + 64))()
    return block, ctypes.c_void_p((ctypes.addressof(block) + 15) // 16 * 16)


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    lib = _lib.lib()
    for V, F in ((-1, 4), (4, -1), (TOO_MANY, 4), (4, TOO_MANY)):
        assert lib.nm_mesh_components_workspace_bytes(V, F) == -1 and b"nm_mesh_components_workspace_bytes" in lib.nm_last_error(), (V, F)
    V, F, C = 9, 7, 3
    nbytes = lib.nm_mesh_components_workspace_bytes(V, F)
    assert 0 < nbytes <= 4000
    # the checks run before any pointer is looked at: a block of host memory stands in for the device arrays
    block, d = _host_block(4096)
    n = ctypes.c_int64(-7)
    good = dict(faces=d, F=F, V=V, label=d, ws=d, nbytes=nbytes, C=C, keep=d)
    sizes = [dict(F=-1), dict(V=-1), dict(F=TOO_MANY), dict(V=TOO_MANY)]
    space = [dict(ws=None), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(ws=ctypes.c_void_p(d.value + 4))]
    for over in [dict(faces=None), dict(label=None)] + sizes + space:
        a = dict(good, **over)
        rc = lib.nm_mesh_components(a['faces'], a['F'], a['V'], a['label'], None, a['ws'], a['nbytes'], ctypes.byref(n), None)
        assert rc == -1 and b"nm_mesh_components:" in lib.nm_last_error(), over
    assert lib.nm_mesh_components(d, F, V, d, d, d, nbytes, None, None) == -1 and b"nm_mesh_components:" in lib.nm_last_error()
    assert n.value == -7
    counts = [dict(C=-1), dict(C=TOO_MANY)]
    for over in [dict(faces=None), dict(label=None)] + sizes + counts:
        a = dict(good, **over)
        rc = lib.nm_mesh_component_stats(a['faces'], a['F'], a['V'], a['label'], d, a['C'], d, d, d, None)
        assert rc == -1 and b"nm_mesh_component_stats" in lib.nm_last_error(), over
    for cv, cf, verts, box in ((None, d, d, d), (d, None, d, d), (d, d, None, d)):                  # the last: comp_box without verts
        assert lib.nm_mesh_component_stats(d, F, V, d, verts, C, cv, cf, box, None) == -1 and b"nm_mesh_component_stats" in lib.nm_last_error()
    nv, nf = ctypes.c_int64(-7), ctypes.c_int64(-7)
    for over in [dict(faces=None), dict(label=None), dict(keep=None)] + sizes + counts + space:
        a = dict(good, **over)
        mesh = (a['faces'], a['F'], a['V'], a['label'], a['keep'], a['C'], a['ws'], a['nbytes'])
        assert lib.nm_mesh_select_count(*mesh, ctypes.byref(nv), ctypes.byref(nf), None) == -1 and b"nm_mesh_select_count" in lib.nm_last_error(), over
        assert lib.nm_mesh_select_fill(*mesh, d, d, 0, 0, None) == -1 and b"nm_mesh_select_fill" in lib.nm_last_error(), over
    mesh = (d, F, V, d, d, C, d, nbytes)
    for pv, pf in ((None, ctypes.byref(nf)), (ctypes.byref(nv), None)):
        assert lib.nm_mesh_select_count(*mesh, pv, pf, None) == -1 and b"nm_mesh_select_count" in lib.nm_last_error()
    assert nv.value == -7 and nf.value == -7
    for vs, fo, a, b in ((None, d, 3, 3), (d, None, 3, 3), (d, d, -1, 3), (d, d, 3, -1), (d, d, TOO_MANY, 3)):
        assert lib.nm_mesh_select_fill(*mesh, vs, fo, a, b, None) == -1 and b"nm_mesh_select_fill" in lib.nm_last_error()
    # no nm_mesh_select_count ever filled this workspace: whatever the counts, they disagree with what it holds
    for a, b in ((0, 0), (3, 3)):
        assert lib.nm_mesh_select_fill(*mesh, d, d, a, b, None) == -1
        assert b"nm_mesh_select_fill" in lib.nm_last_error() and b"nm_mesh_select_count" in lib.nm_last_error()
    del block


def test_an_empty_mesh_needs_no_device():
    """V = F = 0: no component, no launch; the selection of nothing is two empty outputs, and the counts are then remembered"""
    lib = _lib.lib()
    nbytes = lib.nm_mesh_components_workspace_bytes(0, 0)
    assert 0 < nbytes <= 256
    block, d = _host_block(nbytes)
    n, nv, nf = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert lib.nm_mesh_components(None, 0, 0, None, None, d, nbytes, ctypes.byref(n), None) == 0 and n.value == 0
    assert lib.nm_mesh_component_stats(None, 0, 0, None, None, 0, None, None, None, None) == 0
    mesh = (None, 0, 0, None, None, 0, d, nbytes)
    assert lib.nm_mesh_select_count(*mesh, ctypes.byref(nv), ctypes.byref(nf), None) == 0 and (nv.value, nf.value) == (0, 0)
    assert lib.nm_mesh_select_fill(*mesh, None, None, 0, 0, None) == 0
    assert lib.nm_mesh_select_fill(*mesh, d, d, 1, 0, None) == -1 and b"nm_mesh_select_count left 0, 0" in lib.nm_last_error()
    assert lib.nm_mesh_components(None, 0, 0, None, None, d, nbytes, ctypes.byref(n), None) == 0       # ... which forgets the selection
    assert lib.nm_mesh_select_fill(*mesh, None, None, 0, 0, None) == -1
    del block


def test_workspace_matches_the_headers_figures():
    """9 bytes per vertex, 4 per face, 16 per span of either, 64 of header (+ padding below 64); under the ceiling of 16 V + 8 F + 256"""
    lib = _lib.lib()
    with open(os.path.join(ROOT, "include", "neuman_hip.h")) as f:
        header = f.read()
    m = re.search(r"nm_mesh_components_workspace_bytes\(V, F\) bytes = (\d+) bytes per vertex .*?\+ (\d+) bytes per face .*?\+ (\d+) bytes per (\d+) vertices "
                  r"and per \d+ faces .*?\+ (\d+) and padding below (\d+)", header, re.S)
    assert m, "the header no longer states the workspace's size in this form"
    per_vertex, per_face, per_span, span, head, pad = (int(g) for g in m.groups())
    assert (per_vertex, per_face, span) == (9, 4, CS.C.SPAN)
    for V, F in ((0, 0), (1, 0), (0, 1), (12, 6), (1000, 2001), (CS.PAST_THE_SCAN, 2 * CS.PAST_THE_SCAN), (3_000_001, 6_000_007), (TOO_MANY - 1, TOO_MANY - 1)):
        stated = per_vertex * V + per_face * F + per_span * (CS.spans(V) + CS.spans(F)) + head
        got = lib.nm_mesh_components_workspace_bytes(V, F)
        assert stated <= got < stated + pad and got % 16 == 0, (V, F, got, stated)
        assert got <= 16 * V + 8 * F + 256
    n = 10_000_000
    assert abs(lib.nm_mesh_components_workspace_bytes(n, 0) / n - (per_vertex + per_span / span)) < 1e-4
    assert abs(lib.nm_mesh_components_workspace_bytes(0, n) / n - (per_face + per_span / span)) < 1e-4


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    if torch.cuda.is_available():
        pytest.skip("GPU box: the refusal path is exercised on the CPU-only runner")
    verts, faces = torch.zeros(12, 3), torch.from_numpy(CS.HAND_FACES)
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.components(faces, 12)
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.components(CS.HAND_FACES, 12)
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.clean_mesh(verts, faces)
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.clean_mesh(verts, faces, largest=None, min_faces=2)
    comps = mesh_extract.Components(torch.zeros(12, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), 1, None, None, None)
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.select_components(verts, faces, comps, torch.ones(1, dtype=torch.bool))


def test_bad_clean_up_requests_are_refused_on_the_host():
    verts, faces = torch.zeros(12, 3), torch.from_numpy(CS.HAND_FACES)
    for bad in (dict(largest=0), dict(largest=-2), dict(largest=1.5), dict(largest=True), dict(largest='1'), dict(min_faces=-1), dict(min_faces=2.5),
                dict(min_faces=None), dict(min_faces=False)):
        with pytest.raises(ValueError):
            mesh_extract.clean_mesh(verts, faces, **bad)
        with pytest.raises(ValueError):
            mesh_extract.extract_net_mesh(None, CS.BLOB_BOX, 8, 0.5, **bad)           # refused before the net is looked at
        with pytest.raises(ValueError):
            mesh_extract.keep_mask(torch.zeros(3, dtype=torch.int32), **bad)
    # nothing to do: the input mesh itself, whatever device it lives on
    out = mesh_extract.clean_mesh(verts, faces, verts, largest=None, min_faces=0)
    assert len(out) == 3 and out[0] is verts and out[1] is faces and out[2] is verts


def test_keep_mask_is_the_restatements_choice():
    """torch on a [C] tensor (here on the host; clean_mesh runs it on the device): ties go to the lower id"""
    nf = np.array([7, 30, 30, 2, 30, 9, 0], np.int32)
    for largest in (None, 1, 2, 3, 4, 7, 50):
        for min_faces in (0, 1, 8, 30, 31):
            got = mesh_extract.keep_mask(torch.from_numpy(nf), largest, min_faces)
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy().astype(bool), MR.keep_largest(nf, largest, min_faces)), (largest, min_faces)
    assert mesh_extract.keep_mask(torch.from_numpy(nf), 2, 0).tolist() == [0, 1, 1, 0, 0, 0, 0]
    assert mesh_extract.keep_mask(torch.zeros(0, dtype=torch.int32), 1, 0).shape == (0,)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_restatement_on_the_hand_written_mesh():
    vl, fl, n = MR.labels(CS.HAND_FACES, CS.HAND_VERTS)
    assert n == 4 and vl.dtype == fl.dtype == np.int32
    assert vl.tolist() == [-1, 0, 1, 2, 0, 2, 1, 2, 3, 2, 1, -1] == CS.HAND_VERT_LABEL.tolist()
    assert fl.tolist() == [2, 0, 1, 3, 2, 1] == CS.HAND_FACE_LABEL.tolist()
    verts = np.arange(36, dtype=np.float32).reshape(12, 3) * np.float32(0.5) - np.float32(4)
    verts[5, 1] = np.nan                                                               # skipped
    verts[8] = (np.nan, np.inf, -0.0)                                                  # a component of one vertex: no usable x
    cv, cf, box = MR.stats(CS.HAND_FACES, vl, n, verts)
    assert cv.tolist() == [2, 3, 4, 1] == CS.HAND_COMP_VERTS.tolist() and cf.tolist() == [1, 2, 2, 1] == CS.HAND_COMP_FACES.tolist()
    assert box.dtype == np.float32 and box.shape == (4, 6)
    assert box[0].tolist() == [-2.5, -2.0, -1.5, 2.0, 2.5, 3.0]                        # vertices 1 and 4
    assert box[2].tolist() == [0.5, 1.0, 1.5, 9.5, 10.0, 10.5]                         # 3, 5, 7, 9 without 5's y
    assert box[3, 0] == np.inf and box[3, 3] == -np.inf and box[3, 1] == box[3, 4] == np.inf
    assert box[3, 2] == 0 and np.signbit(box[3, 2]) and np.signbit(box[3, 5])
    assert MR.stats(CS.HAND_FACES, vl, n)[2] is None
    # selection: components 0 and 2
    src, out = MR.select(CS.HAND_FACES, vl, [1, 0, 1, 0])
    assert src.tolist() == [1, 3, 4, 5, 7, 9] and out.tolist() == [[3, 1, 4], [0, 0, 2], [4, 5, 3]]
    src, out = MR.select(CS.HAND_FACES, vl, np.zeros(4, bool))
    assert src.shape == (0,) and out.shape == (0, 3) and src.dtype == out.dtype == np.int32
    src, out = MR.select(CS.HAND_FACES, vl, np.ones(4, np.uint8))
    assert src.tolist() == list(range(1, 11)) and np.array_equal(out, CS.HAND_FACES - 1)      # only the unreferenced vertices go
    # invalid faces
    for bad in (-1, 12, MR.I32_MAX, MR.I32_MIN):
        f = CS.HAND_FACES.copy()
        f[4, 1] = bad
        assert MR.invalid_faces(f, 12).tolist() == [4]
        with pytest.raises(ValueError):
            MR.labels(f, 12)
    # empty inputs
    vl, fl, n = MR.labels(np.zeros((0, 3), np.int32), 5)
    assert n == 0 and vl.tolist() == [-1] * 5 and fl.shape == (0,)
    vl, fl, n = MR.labels(np.zeros((0, 3), np.int32), 0)
    assert n == 0 and vl.shape == (0,) and fl.shape == (0,)


def test_restatement_on_the_three_blob_isosurface():
    want = CS.BLOB_EXPECTED
    m = IR.extract(CS.blob_field(), CS.BLOB_BOX, 0.0)
    assert (m['n_verts'], m['n_faces']) == (want['n_verts'], want['n_faces'])
    vl, fl, n = MR.labels(m['faces'], m['n_verts'])
    assert n == 3 and (vl >= 0).all()
    reps = tuple(int(np.flatnonzero(vl == c)[0]) for c in range(n))
    assert reps == want['representatives']
    cv, cf, box = MR.stats(m['faces'], vl, n, m['verts'])
    assert tuple(cv.tolist()) == want['comp_verts'] and tuple(cf.tolist()) == want['comp_faces']
    assert int((np.diff(vl) != 0).sum()) == want['label_changes']                     # interleaved along the vertex index: compaction is no slice
    assert np.array_equal(fl, vl[m['faces'][:, 1]]) and np.array_equal(fl, vl[m['faces'][:, 2]])
    for c in range(n):                                                                # every box is its sphere's, to within a cell
        centre, r0 = min(CS.BLOBS, key=lambda b: np.abs(np.asarray(b[0]) - (box[c, :3] + box[c, 3:]) / 2).max())
        assert np.abs(box[c, :3] - (np.asarray(centre) - r0)).max() < 2 / 24 and np.abs(box[c, 3:] - (np.asarray(centre) + r0)).max() < 2 / 24
        keep = np.arange(n) == c
        src, out = MR.select(m['faces'], vl, keep)
        assert src.shape[0] == cv[c] and out.shape[0] == cf[c] and np.array_equal(src, np.flatnonzero(vl == c))
        closed, boundary, repeated = IR.edge_census(out)
        assert closed and repeated == 0 and boundary.shape[0] == 0
        assert IR.euler_characteristic(src.shape[0], out) == 2
        assert np.array_equal(m['verts'][src][out], m['verts'][m['faces'][fl == c]])  # the same triangles, in the same order
    src, out = MR.select(m['faces'], vl, np.ones(n, bool))
    assert np.array_equal(src, np.arange(m['n_verts'])) and np.array_equal(out, m['faces'])


def test_restatement_on_the_large_cases_is_what_their_construction_says():
    """the strip, the fan and the disjoint triangles of the GPU test: labels known by construction, each in a few seconds"""
    V = CS.STRIP_VERTS
    for order in ('ascending', 'descending', 'permuted'):
        faces, piece = CS.strip(V, order)
        vl, fl, n = MR.labels(faces, V)
        assert n == 1 and not vl.any() and not fl.any(), order
        faces, piece = CS.strip(V, order, CS.strip_cuts(V))
        vl, fl, n = MR.labels(faces, V)
        assert n == 3 and np.array_equal(vl, CS.expected_labels_of_pieces(piece)), order
        assert np.bincount(vl).min() >= 3
    for hub_last in (False, True):
        faces, Vf = CS.fan(CS.FAN_FACES, hub_last)
        vl, fl, n = MR.labels(faces, Vf)
        assert n == 1 and not vl.any() and Vf == CS.FAN_FACES + 2
    V = CS.DISJOINT_VERTS
    faces = CS.disjoint_triangles(V)
    vl, fl, n = MR.labels(faces, V)
    assert n == V // 3 and np.array_equal(vl[:3 * n], np.repeat(np.arange(n), 3)) and vl[-1] == -1
    assert np.array_equal(fl, np.arange(n))
    cv, cf, _ = MR.stats(faces, vl, n)
    assert (cv == 3).all() and (cf == 1).all()
    src, out = MR.select(faces, vl, np.arange(n) % 2 == 0)
    assert src.shape[0] == 3 * ((n + 1) // 2) and np.array_equal(out, CS.disjoint_triangles(src.shape[0]))


def test_two_translated_spheres_tie_on_the_face_count():
    m = IR.extract(CS.two_equal_spheres_field(), CS.BLOB_BOX, 0.0)
    vl, fl, n = MR.labels(m['faces'], m['n_verts'])
    cv, cf, _ = MR.stats(m['faces'], vl, n)
    assert n == 2 and cf[0] == cf[1] and cv[0] == cv[1]
    assert MR.keep_largest(cf, 1).tolist() == [True, False]
