"""Without a device: the isosurface entry points' argument checks (before any device work), save_ply byte for byte, the Python surface's
refusals, and the numpy restatement of the contract (tests/helpers/isosurface_ref.py) on surfaces whose topology and size are known -- the
yardstick of tests/test_hip_isosurface.py, checked where it can run."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import isosurface_ref as IR  # noqa: E402

from neuman_hip import _lib, mesh_extract, synthetic  # noqa: E402

BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
CENTRE = (0.013, -0.021, 0.017)                       # off the grid: no vertex value equals the level


def _box(*v):
    return (ctypes.c_float * 6)(*v)


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    lib = _lib.lib()
    assert lib.nm_isosurface_workspace_bytes(9, 9, 9) > 2 * 729
    for dims in ((1, 9, 9), (9, 0, 9), (9, 9, -3), (2048, 2048, 512)):
        assert lib.nm_isosurface_workspace_bytes(*dims) == -1 and b"nm_isosurface_workspace_bytes" in lib.nm_last_error(), dims
    # the checks run before any pointer is looked at: a block of host memory stands in for the device arrays
    block = (ctypes.c_char * 4096)()
    d = ctypes.c_void_p((ctypes.addressof(block) + 15) // 16 * 16)
    nbytes = lib.nm_isosurface_workspace_bytes(5, 4, 3)
    assert 0 < nbytes <= 4000
    good = dict(field=d, dims=(5, 4, 3), box=_box(*BOX), level=0.25, ws=d, nbytes=nbytes)
    nan, inf = float('nan'), float('inf')
    bad = [dict(field=None), dict(box=None), dict(ws=None), dict(dims=(1, 4, 3)), dict(dims=(5, 4, 0)), dict(dims=(2048, 2048, 512)),
           dict(box=_box(-1, -1, -1, 1, nan, 1)), dict(box=_box(-inf, -1, -1, 1, 1, 1)), dict(box=_box(-1, -1, 1, 1, 1, -1)),
           dict(box=_box(-1, 1, -1, 1, 1, 1)), dict(level=nan), dict(level=inf), dict(nbytes=nbytes - 1), dict(nbytes=0),
           dict(ws=ctypes.c_void_p(d.value + 4))]
    nv, nf = ctypes.c_int64(-7), ctypes.c_int64(-7)
    for over in bad:
        a = dict(good, **over)
        rc = lib.nm_isosurface_count(a['field'], *a['dims'], a['box'], a['level'], a['ws'], a['nbytes'], ctypes.byref(nv), ctypes.byref(nf), None)
        assert rc == -1 and b"nm_isosurface_count" in lib.nm_last_error(), over
        rc = lib.nm_isosurface_fill(a['field'], *a['dims'], a['box'], a['level'], a['ws'], a['nbytes'], d, d, d, 10, 10, None)
        assert rc == -1 and b"nm_isosurface_fill" in lib.nm_last_error(), over
    assert nv.value == -7 and nf.value == -7
    a = good
    for pv, pf in ((None, ctypes.byref(nf)), (ctypes.byref(nv), None)):
        assert lib.nm_isosurface_count(a['field'], *a['dims'], a['box'], a['level'], a['ws'], a['nbytes'], pv, pf, None) == -1
        assert b"nm_isosurface_count" in lib.nm_last_error()
    for verts, faces, cv, cf in ((None, d, 10, 10), (d, None, 10, 10), (d, d, -1, 10), (d, d, 10, -1)):
        assert lib.nm_isosurface_fill(a['field'], *a['dims'], a['box'], a['level'], a['ws'], a['nbytes'], verts, None, faces, cv, cf, None) == -1
        assert b"nm_isosurface_fill" in lib.nm_last_error()


def test_workspace_is_a_few_bytes_per_grid_vertex():
    """no 32-bit index per edge (28 B per vertex): flags, face counts and prefix counts, as the header states"""
    lib = _lib.lib()
    n = 513
    per_vertex = lib.nm_isosurface_workspace_bytes(n, n, n) / n ** 3
    assert 2.5 <= per_vertex < 2.55


def test_save_ply_round_trips_a_tetrahedron_byte_for_byte(tmp_path):
    verts = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    faces = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]
    normals = [[-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [0.5, 0.5, 0.5]]
    colours = [[0.0, 0.5, 1.0], [1.0, 0.0, 0.25], [2.0, -1.0, 0.1], [0.2, 0.4, 0.6]]
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "element face 4\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    bytes_of = [[0, 128, 255], [255, 0, 64], [255, 0, 26], [51, 102, 153]]
    body = b"".join(struct.pack("<6f3B", *v, *n, *c) for v, n, c in zip(verts, normals, bytes_of))
    body += b"".join(struct.pack("<B3i", 3, *f) for f in faces)
    path = tmp_path / "tet.ply"
    mesh_extract.save_ply(path, torch.tensor(verts), torch.tensor(faces, dtype=torch.int32), torch.tensor(normals), np.array(colours))
    assert path.read_bytes() == head + body
    # positions and faces alone
    plain = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
             "element face 4\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    mesh_extract.save_ply(path, verts, faces)
    assert path.read_bytes() == plain + b"".join(struct.pack("<3f", *v) for v in verts) + b"".join(struct.pack("<B3i", 3, *f) for f in faces)
    with pytest.raises(ValueError):
        mesh_extract.save_ply(path, verts, [[0, 1, 4]])
    with pytest.raises(ValueError):
        mesh_extract.save_ply(path, verts, faces, normals[:3])


def test_cpu_tensors_and_the_time_conditioned_net_are_refused():
    if torch.cuda.is_available():
        pytest.skip("GPU box: the refusal path is exercised on the CPU-only runner")
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.extract_mesh(torch.zeros(4, 4, 4), BOX, 0.5)
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.extract_mesh(np.zeros((4, 4, 4), np.float32), BOX, 0.5)
    net = synthetic.make_joiner(0)
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.density_grid(net, BOX, 8)
    with pytest.raises(_lib.NeumanHipError):
        mesh_extract.extract_net_mesh(net, BOX, (6, 5, 4), 0.5)


def test_bad_requests_are_refused_on_the_host():
    j4 = synthetic.make_variant_joiner(6, raw_pos_dim=4)
    with pytest.raises(NotImplementedError):
        mesh_extract.density_grid(j4, BOX, 8)
    with pytest.raises(NotImplementedError):
        mesh_extract.extract_net_mesh(j4, BOX, 8, 0.5)
    net = synthetic.make_joiner(0)
    for res in (1, (8, 8), (8, 1, 8), (2048, 2048, 512)):
        with pytest.raises(ValueError):
            mesh_extract.density_grid(net, BOX, res)
    with pytest.raises(ValueError):
        mesh_extract.density_grid(net, (0, 0, 0, 1, 1, 0), 8)
    with pytest.raises(TypeError):
        mesh_extract.extract_mesh(torch.zeros(4, 4, 4), BOX)                     # level is required: no default


def test_tables_of_the_restatement():
    tets = IR.tetrahedra()
    assert [c for c, _ in tets] == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
    assert [odd for _, odd in tets] == [0, 1, 1, 0, 0, 1]
    for mask in range(16):
        tris = IR.tet_case(mask)
        k = bin(mask).count("1")
        assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[k]
        for t in tris:                                                           # every triangle vertex sits on an edge that is crossed
            assert all(((mask >> p) & 1) != ((mask >> q) & 1) and p < q for p, q in t)
        # the complementary pattern is the same surface seen from the other side
        flipped = [[t[0], t[2], t[1]] for t in IR.tet_case(15 - mask)]
        assert sorted(map(sorted, tris)) == sorted(map(sorted, flipped))
    # one corner of the unit tetrahedron (0, x, x + y, x + y + z) inside: the triangle's normal points away from that corner
    P = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], float)
    for c in range(4):
        (tri,) = IR.tet_case(1 << c)
        a, b, d = [(P[p] + P[q]) / 2 for p, q in tri]
        centroid = (a + b + d) / 3
        assert np.dot(np.cross(b - a, d - a), centroid - P[c]) > 0


@pytest.mark.parametrize("cells", [24, 16])
def test_restatement_on_a_sphere(cells):
    r0 = 0.6
    dims = (cells + 1,) * 3
    m = IR.extract(IR.sphere_field(dims, BOX, CENTRE, r0), BOX, 0.0)
    closed, boundary, repeated = IR.edge_census(m['faces'])
    assert closed and repeated == 0 and boundary.shape[0] == 0
    assert IR.euler_characteristic(m['n_verts'], m['faces']) == 2
    h = 2.0 / cells
    L = np.sqrt(3.0) * h
    e = L * L / (8 * (r0 - L))                                                    # linear interpolation of a distance field over an edge <= L
    r = np.linalg.norm(m['verts'].astype(np.float64) - np.array(CENTRE), axis=1)
    assert np.abs(r - r0).max() <= e
    vol = IR.signed_volume(m['verts'], m['faces'])
    inner = r0 - e - L * L / (8 * (r0 - e))
    assert 4 / 3 * np.pi * inner ** 3 <= vol <= 4 / 3 * np.pi * (r0 + e) ** 3
    radial = (m['verts'].astype(np.float64) - np.array(CENTRE)) / r[:, None]
    assert (np.einsum('ij,ij->i', m['normals'].astype(np.float64), radial) > 0.99).all()
    # the float64 variant: the same topology, positions a few ulp away
    m64 = IR.extract(IR.sphere_field(dims, BOX, CENTRE, r0), BOX, 0.0, np.float64)
    assert np.array_equal(m64['faces'], m['faces']) and m64['verts'].dtype == np.float64
    assert np.abs(m64['verts'] - m['verts']).max() <= 4 * 2.0 ** -23


def test_restatement_on_a_torus_two_spheres_and_a_non_cubic_grid():
    dims = (25, 25, 25)
    m = IR.extract(IR.torus_field(dims, BOX, CENTRE, 0.55, 0.22), BOX, 0.0)
    assert IR.edge_census(m['faces'])[0] and IR.euler_characteristic(m['n_verts'], m['faces']) == 0
    s = 0.013
    two = np.maximum(IR.sphere_field(dims, BOX, (0.45 + s, s, s), 0.3), IR.sphere_field(dims, BOX, (-0.45 + s, s, s), 0.3))
    m = IR.extract(two, BOX, 0.0)
    assert IR.edge_census(m['faces'])[0] and IR.euler_characteristic(m['n_verts'], m['faces']) == 4
    box = (-1.0, -0.8, -0.7, 1.1, 0.9, 0.75)
    m = IR.extract(IR.sphere_field((19, 14, 11), box, CENTRE, 0.55), box, 0.0)
    assert IR.edge_census(m['faces'])[0] and IR.euler_characteristic(m['n_verts'], m['faces']) == 2
    assert IR.signed_volume(m['verts'], m['faces']) > 0


def test_restatement_winds_degenerate_triangles_consistently():
    """grid values exactly equal to the level (outside, by rule M2) collapse triangles to zero area; the surface stays closed and every
    directed edge still has its reverse exactly once; a NaN is outside and nothing non-finite comes out"""
    dims = (13, 12, 11)
    f = IR.sphere_field(dims, BOX, (0.0, 0.0, 0.0), 0.5)
    f[np.abs(f) < 0.08] = 0.0
    assert (f == 0).sum() > 50
    m = IR.extract(f, BOX, 0.0)
    assert m['n_faces'] > 0 and IR.edge_census(m['faces'])[0]
    v = m['verts'][m['faces'].astype(np.int64)]
    assert (np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) == 0).any()
    g = IR.sphere_field(dims, BOX, CENTRE, 0.5)
    g[5, 6, 4] = np.nan
    g[6, 6, 7] = np.inf
    g[3, 5, 5] = -np.inf
    m = IR.extract(g, BOX, 0.0)
    assert IR.edge_census(m['faces'])[0] and np.isfinite(m['verts']).all() and np.isfinite(m['normals']).all()
