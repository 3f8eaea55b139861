"""Without a device: nm_mesh_atlas_size, nm_mesh_atlas_pack and nm_mesh_atlas_sample (csrc/mesh_atlas.hip; the header's 'mesh atlas', rules
A1-A5) in the header, in `_lib.SIGNATURES` and in the library; rule A1 against tests/helpers/mesh_atlas_ref.py; every refusal of the entries
and of neuman_hip.mesh_export; the helper alone on what the header derives from the rules; and the three files `write_obj` writes, byte for
byte."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import mesh_atlas_ref as AR  # noqa: E402
import mesh_lattice_ref as LR  # noqa: E402

from neuman_hip import _lib, mesh_export  # noqa: E402

ARITY = {"nm_mesh_atlas_size": 5, "nm_mesh_atlas_pack": 5, "nm_mesh_atlas_sample": 8}
RS = (1, 2, 3, 5, 8)
FS = (1, 2, 3, 7, 10)


@pytest.mark.parametrize("name", list(ARITY))
def test_the_entries_are_declared_bound_and_exported_with_matching_arity(name):
    src = open(os.path.join(HERE, "..", "include", "neuman_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in neuman_hip.h"
    assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == ARITY[name]


# ---- A1 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 7, 8, 64])
def test_atlas_size_is_the_helpers(R):
    for F in list(range(1, 41)) + [599, 600, 3040, 3041, 5000, 13776]:
        W, H, nbx = got = mesh_export.atlas_size(F, R)
        assert got == AR.atlas_size(F, R), (F, R)
        assert all(type(x) is int for x in got)
        P, (BW, BH) = (F + 1) // 2, AR.block(R)
        nby = H // BH
        assert W == nbx * BW and H == nby * BH and nbx * nby >= P > nbx * (nby - 1)      # the blocks fit, and no row of them is empty
        assert nbx * nbx * BW >= P * BH and (nbx == 1 or (nbx - 1) * (nbx - 1) * BW < P * BH)


def test_atlas_size_examples_and_refusals():
    assert mesh_export.atlas_size(13776, 8) == (864, 864, 72)
    assert mesh_export.atlas_size(600, 8) == (180, 180, 15)
    assert mesh_export.atlas_size(10, 5)[:2] == (18, 18)
    assert mesh_export.atlas_size(1, 1)[:2] == (5, 2)
    assert AR.atlas_size(1 << 20, 64) is None
    with pytest.raises(_lib.NeumanHipError, match="nm_mesh_atlas_size"):
        mesh_export.atlas_size(1 << 20, 64)
    for F, R in ((0, 8), (-1, 8), (4, 0), (4, 65), (4, -1), (4.0, 8), (4, 8.0), (True, 8), (4, True)):
        with pytest.raises(ValueError):
            mesh_export.atlas_size(F, R)
    lib = _lib.lib()
    W, H, nbx = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    ok = dict(F=10, R=5, W=ctypes.byref(W), H=ctypes.byref(H), nbx=ctypes.byref(nbx))
    bad = [dict(F=0), dict(F=-1), dict(R=0), dict(R=65), dict(R=-1), dict(W=None), dict(H=None), dict(nbx=None), dict(F=1 << 20, R=64),
           dict(F=1 << 62, R=1), dict(F=(1 << 63) - 1, R=64)]
    for over in bad:
        k = dict(ok, **over)
        assert lib.nm_mesh_atlas_size(k['F'], k['R'], k['W'], k['H'], k['nbx']) == -1 and b"nm_mesh_atlas_size:" in lib.nm_last_error(), over
        assert (W.value, H.value, nbx.value) == (-7, -7, -7)                               # a refusal writes nothing
    # the largest atlases the rule admits are still within its 16384 x 16384, and the first F beyond is refused
    for R in (1, 8, 64):
        BW, BH = AR.block(R)
        lo, hi = 1, 1 << 40
        while hi - lo > 1:                                                                 # the last F the helper accepts
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if AR.atlas_size(mid, R) else (lo, mid)
        assert lib.nm_mesh_atlas_size(lo, R, ok['W'], ok['H'], ok['nbx']) == 0 and (W.value, H.value, nbx.value) == AR.atlas_size(lo, R)
        assert max(W.value, H.value) <= 16384
        assert lib.nm_mesh_atlas_size(hi, R, ok['W'], ok['H'], ok['nbx']) == -1


def test_every_refusal_of_the_device_entries_comes_before_any_device_work():
    lib = _lib.lib()
    dummy = (ctypes.c_char * 256)()                                     # stands in for every device pointer: the checks run before any is read
    d = ctypes.cast(dummy, ctypes.c_void_p)
    good = dict(fc=d, F=4, R=8, atlas=d)
    for over in [dict(fc=None), dict(atlas=None), dict(F=0), dict(F=-1), dict(R=0), dict(R=-1), dict(R=65), dict(F=1 << 20, R=64), dict(F=1 << 62)]:
        k = dict(good, **over)
        assert lib.nm_mesh_atlas_pack(k['fc'], k['F'], k['R'], k['atlas'], None) == -1 and b"nm_mesh_atlas_pack:" in lib.nm_last_error(), over
    good = dict(atlas=d, F=4, R=8, face_id=d, bary=d, n=5, out=d)
    for over in [dict(atlas=None), dict(face_id=None), dict(bary=None), dict(out=None), dict(F=0), dict(F=-1), dict(R=0), dict(R=-1), dict(R=65),
                 dict(F=1 << 20, R=64), dict(F=1 << 62), dict(n=0), dict(n=-1)]:
        k = dict(good, **over)
        rc = lib.nm_mesh_atlas_sample(k['atlas'], k['F'], k['R'], k['face_id'], k['bary'], k['n'], k['out'], None)
        assert rc == -1 and b"nm_mesh_atlas_sample:" in lib.nm_last_error(), over


class _Fake(torch.Tensor):
    """a CPU tensor that says it lives on the device (tests/test_mesh_lattice_host.py): the layer's checks run, on a box without one, up to
    the first call that needs it"""
    is_cuda = True


def _tensor(*shape, dtype=torch.float32):
    if torch.cuda.is_available():
        return torch.zeros(*shape, dtype=dtype, device='cuda')
    return torch.zeros(*shape, dtype=dtype).as_subclass(_Fake)


def test_the_python_layer_refuses_cpu_tensors_and_shapes_that_are_no_lattice_or_atlas(tmp_path):
    E = _lib.NeumanHipError
    with pytest.raises(E, match="pack_atlas: face_colours must be a CUDA"):
        mesh_export.pack_atlas(torch.zeros(2, 6, 3))
    with pytest.raises(E, match="pack_atlas"):
        mesh_export.pack_atlas(np.zeros((2, 6, 3), np.float32))
    for fc in (_tensor(2, 5, 3), _tensor(2, 6, 4), _tensor(2, 6), _tensor(0, 6, 3), _tensor(2, 6, 3, dtype=torch.float64), _tensor(2, 2211, 3)):
        with pytest.raises(E, match="pack_atlas: face_colours must be"):
            mesh_export.pack_atlas(fc)
    W, H, _ = mesh_export.atlas_size(4, 2)
    atlas, face_id, bary = _tensor(H, W, 3), _tensor(5, 7, dtype=torch.int32), _tensor(5, 7, 3)
    for a, i, b in ((torch.zeros(H, W, 3), face_id, bary), (atlas, torch.zeros(5, 7, dtype=torch.int32), bary), (atlas, face_id, torch.zeros(5, 7, 3))):
        with pytest.raises(E, match="must be a CUDA"):
            mesh_export.sample_atlas(a, 4, 2, i, b)
    for a, i, b in ((_tensor(H, W + 1, 3), face_id, bary), (_tensor(H, W, 4), face_id, bary), (_tensor(H, W, 3, dtype=torch.float64), face_id, bary),
                    (atlas, _tensor(5, 7, dtype=torch.int64), bary), (atlas, face_id, _tensor(5, 7, 2)), (atlas, face_id, _tensor(7, 5, 3)),
                    (atlas, face_id, _tensor(5, 7, 3, dtype=torch.float64))):
        with pytest.raises(E, match="sample_atlas:"):
            mesh_export.sample_atlas(a, 4, 2, i, b)
    with pytest.raises(ValueError):
        mesh_export.sample_atlas(atlas, 4, 0, face_id, bary)
    with pytest.raises(E, match="export_mesh: face_colours must be a CUDA"):
        mesh_export.export_mesh(str(tmp_path / "m.obj"), np.zeros((3, 3)), [[0, 1, 2]], torch.zeros(1, 6, 3))
    assert os.listdir(tmp_path) == []


# ---- the helper alone, float64 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RS)
def test_the_four_sets_partition_a_block_and_the_reflection_swaps_them(R):
    kind = AR.classify(R)
    BW, BH = AR.block(R)
    assert kind.shape == (BH, BW) and BW == R + 4 and BH == R + 1
    counts = [int((kind == k).sum()) for k in range(4)]
    S = LR.lattice_size(R)
    assert counts == [S, R + 1, R + 1, S] and sum(counts) == BW * BH                   # every texel in exactly one set; two faces' worth
    y, x = np.indices(kind.shape)
    assert np.array_equal(kind[R - y, R + 3 - x], 3 - kind)                            # lower <-> upper, nodes <-> nodes, gutter <-> gutter
    i1, i2 = LR.nodes(R)
    assert (kind[i2, i1] == AR.LOWER_NODE).all() and (kind[R - i2, R + 3 - i1] == AR.UPPER_NODE).all()


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("R", RS)
def test_every_texel_of_a_used_half_block_is_assigned_exactly_once_and_to_its_own_face(R, F):
    lat = np.random.default_rng(10 * R + F).random((F, LR.lattice_size(R), 3)) + 1.0   # no node is 0: an unwritten texel shows
    atlas, writes = AR.pack(lat, R, np.float64)
    owner, kind = AR.owners(F, R)
    W, H, nbx = AR.atlas_size(F, R)
    assert atlas.shape == (H, W, 3) and np.array_equal(writes, (owner >= 0).astype(np.int64))
    assert (atlas[owner < 0] == 0).all() and not np.signbit(atlas[owner < 0]).any() and (atlas[owner >= 0] != 0).all()
    assert sorted(np.unique(owner[owner >= 0]).tolist()) == list(range(F))             # half blocks are disjoint: a map, onto the faces
    half = LR.lattice_size(R) + R + 1
    assert (np.bincount(owner[owner >= 0], minlength=F) == half).all()
    for f in range(F):                                                                 # scatter and gather agree on whose texel is whose
        i1, i2 = LR.nodes(R)
        X, Y = AR.place(f, i1, i2, R, nbx)
        assert (owner[Y, X] == f).all() and (kind[Y, X] == (AR.UPPER_NODE if f % 2 else AR.LOWER_NODE)).all()
        assert np.array_equal(atlas[Y, X], lat[f])                                     # a node texel is its node
        gx = np.arange(1, R + 2)
        X, Y = AR.place(f, gx, R + 1 - gx, R, nbx)
        assert (owner[Y, X] == f).all() and (kind[Y, X] == (AR.UPPER_GUTTER if f % 2 else AR.LOWER_GUTTER)).all()
        assert np.array_equal(atlas[Y[-1], X[-1]], lat[f, LR.node_index(R, R, 0)])     # the corner gutter texel (R+1, 0)


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("R", RS)
def test_the_sample_at_a_nodes_barycentrics_is_the_node(R, F):
    lat = np.random.default_rng(R + 100 * F).random((F, LR.lattice_size(R), 3))
    atlas, _ = AR.pack(lat, R, np.float64)
    i1, i2 = LR.nodes(R)
    for f in range(F):
        got, _ = AR.sample(atlas, F, R, np.full(i1.shape, f), i1 / R, i2 / R, np.float64)
        assert np.abs(got - lat[f]).max() < 1e-13


def _points(n, F, seed):
    rng = np.random.default_rng(seed)
    b = rng.dirichlet((1, 1, 1), n)
    return b[:, 1], b[:, 2], rng.integers(0, F, n)


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("R", RS)
def test_hypotenuse_cells_give_rule_l3_and_every_other_cell_stays_within_a_quarter_of_its_second_difference(R, F):
    lat = np.random.default_rng(7 * R + F).random((F, LR.lattice_size(R), 3))
    atlas, _ = AR.pack(lat, R, np.float64)
    b1, b2, f = _points(3000, F, R * F)
    got, info = AR.sample(atlas, F, R, f, b1, b2, np.float64)
    want, _, upper = LR.lookup(lat, f, R, b1, b2, np.float64)
    f1, f2, D = info['f1'][:, None], info['f2'][:, None], info['D']
    hyp = info['i1'] + info['i2'] == R - 1
    assert hyp.any() and (hyp.all() or R > 1) and not upper[hyp].any()
    assert np.abs(D[hyp]).max() < 1e-14 and np.abs(got - want)[hyp].max() < 1e-14      # the gutter makes D vanish: bilinear IS the linear blend
    extra = np.where(upper[:, None], (1 - f1) * (1 - f2), f1 * f2) * D
    assert np.abs((got - want) - extra).max() < 1e-14
    assert (np.abs(got - want) <= np.abs(D) / 4 + 1e-14).all()
    # the sampler's texels are the face's own, whatever the barycentrics
    owner, _ = AR.owners(F, R)
    assert (owner[info['Y'], info['X']] == f[:, None]).all()
    wild = np.array([-0.5, 2.0, np.nan, 0.7, np.inf, -np.inf, 1e30, -1e30, 1.0, 0.0])
    for f0 in range(F):
        _, info = AR.sample(atlas, F, R, np.full(len(wild), f0), wild, wild[::-1], np.float64)
        assert (owner[info['Y'], info['X']] == f0).all()
    got, info = AR.sample(atlas, F, R, [-1, F, 1 << 30], [0.2] * 3, [0.3] * 3, np.float64)
    assert not info['valid'].any() and (got == 0).all()


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("R", RS)
def test_texture_coordinates_are_corner_texel_centres_and_a_plain_viewer_shows_the_sampler(R, F):
    uv = mesh_export.atlas_uvs(F, R)
    assert uv.dtype == np.float64 and uv.shape == (F, 3, 2) and np.array_equal(uv, AR.uvs(F, R))
    W, H, nbx = AR.atlas_size(F, R)
    owner, kind = AR.owners(F, R)
    x, y = uv[..., 0] * W - 0.5, (1.0 - uv[..., 1]) * H - 0.5                          # texel coordinates of the corners: whole numbers
    X, Y = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    assert np.abs(x - X).max() < 1e-9 and np.abs(y - Y).max() < 1e-9
    assert (owner[Y, X] == np.arange(F)[:, None]).all() and np.isin(kind[Y, X], (AR.LOWER_NODE, AR.UPPER_NODE)).all()
    assert len({(a, b) for a, b in zip(X.ravel().tolist(), Y.ravel().tolist())}) == 3 * F          # no two faces share a vt
    for k, (i1, i2) in enumerate(((0, 0), (R, 0), (0, R))):
        px, py = AR.place(np.arange(F), i1, i2, R, nbx)
        assert np.array_equal(px, X[:, k]) and np.array_equal(py, Y[:, k])
    # a viewer that knows nothing of blocks: interpolate the face's vt, filter the image bilinearly -> rule A5's value; the four texels under
    # any point of the UV triangle are the face's own half block (the sampler's texels, checked above)
    lat = np.random.default_rng(R + F).random((F, LR.lattice_size(R), 3))
    atlas, _ = AR.pack(lat, R, np.float64)
    b1, b2, f = _points(2000, F, 3 * R + F)
    b = np.stack([1 - b1 - b2, b1, b2], 1)
    seen = AR.viewer_sample(atlas, (b[:, :, None] * uv[f]).sum(1))
    got, _ = AR.sample(atlas, F, R, f, b1, b2, np.float64)
    assert np.abs(seen - got).max() < 1e-9


# ---- the three files -----------------------------------------------------------------------------------------------------------------------------
VERTS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.1]], np.float32)
FACES = [[0, 1, 2], [1, 3, 2]]
NORMALS = [[0, 0, 1], [0, 0, 1], [0, 0, 1], [-0.5, 0.25, 0.75]]
OBJ_HEAD = """mtllib two.mtl
usemtl atlas
v 0 0 0
v 1 0 0
v 0 1 0
v 1 1 0.100000001
"""
OBJ_VN = """vn 0 0 1
vn 0 0 1
vn 0 0 1
vn -0.5 0.25 0.75
"""
OBJ_VT = """vt 0.1000000000 0.7500000000
vt 0.3000000000 0.7500000000
vt 0.1000000000 0.2500000000
vt 0.9000000000 0.2500000000
vt 0.7000000000 0.2500000000
vt 0.9000000000 0.7500000000
"""
OBJ_F = "f 1/1 2/2 3/3\nf 2/4 4/5 3/6\n"
OBJ_F_N = "f 1/1/1 2/2/2 3/3/3\nf 2/4/2 4/5/4 3/6/3\n"
MTL = "newmtl atlas\nKd 1 1 1\nmap_Kd two.png\n"


def _image(F, R, seed=0):
    W, H, _ = AR.atlas_size(F, R)
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("with_normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("suffix", ["", ".obj"])
def test_write_obj_byte_for_byte(tmp_path, suffix, with_normals):
    image = _image(2, 1)                                                               # 5 x 2: one block
    uv = mesh_export.atlas_uvs(2, 1)
    as_given = [(VERTS, FACES, uv, image, NORMALS), (torch.from_numpy(VERTS), torch.tensor(FACES, dtype=torch.int32), torch.from_numpy(uv),
                                                     torch.from_numpy(image), torch.tensor(NORMALS)),
                (VERTS.tolist(), np.array(FACES, np.int64), uv.tolist(), image, np.array(NORMALS))]
    for n, (v, f, t, a, nrm) in enumerate(as_given):                                   # arrays, tensors, nested lists: the same bytes
        sub = tmp_path / f"given{n}"
        sub.mkdir()
        paths = mesh_export.write_obj(str(sub / ("two" + suffix)), v, f, t, a, normals=nrm if with_normals else None)
        assert paths == tuple(str(sub / ("two" + e)) for e in (".obj", ".mtl", ".png")) and sorted(os.listdir(sub)) == ["two.mtl", "two.obj", "two.png"]
        want = OBJ_HEAD + (OBJ_VN if with_normals else "") + OBJ_VT + (OBJ_F_N if with_normals else OBJ_F)
        assert open(paths[0], "rb").read() == want.encode("ascii")
        assert open(paths[1], "rb").read() == MTL.encode("ascii")
        assert np.array_equal(AR.read_png(paths[2]), image)                            # the PNG decodes to the atlas bytes
        obj, decoded = AR.read_export(paths[0])                                        # ... and the parser follows mtllib and map_Kd to it
        assert np.array_equal(decoded, image) and np.array_equal(obj['f_v'], FACES) and np.array_equal(obj['f_t'], np.arange(6).reshape(2, 3))
        assert np.array_equal(obj['v'].astype(np.float32), VERTS) and np.abs(obj['vt'].reshape(2, 3, 2) - uv).max() < 1e-10
        assert (obj['f_n'] is None) != with_normals and (not with_normals or np.array_equal(obj['f_n'], FACES))


def test_write_obj_refusals(tmp_path):
    uv, image = mesh_export.atlas_uvs(2, 1), _image(2, 1)
    path = str(tmp_path / "two.obj")
    nan_v, inf_v = VERTS.copy(), VERTS.copy()
    nan_v[2, 1], inf_v[0, 0] = np.nan, np.inf
    bad = [dict(faces=[[0, 1, 4], [1, 3, 2]]), dict(faces=[[0, 1, 2], [-1, 3, 2]]), dict(verts=nan_v), dict(verts=inf_v),     # index, finite
           dict(faces=[[0, 1, 2]]), dict(uvs=mesh_export.atlas_uvs(3, 1)), dict(normals=NORMALS[:3]), dict(faces=np.zeros((0, 3), np.int64)),   # counts
           dict(verts=VERTS[:, :2]), dict(faces=[[0, 1, 2, 3], [1, 3, 2, 0]]), dict(uvs=uv[:, :2]), dict(faces=[[0, 1, 2], [1, 3]]),
           dict(faces=[[0, 1, 2.5], [1, 3, 2]]),
           dict(atlas_u8=_image(2, 1)[:, :4]), dict(atlas_u8=_image(4, 1)), dict(atlas_u8=image.astype(np.float32) / 255),    # the atlas
           dict(atlas_u8=image[..., 0]), dict(atlas_u8=np.concatenate([image, image[..., :1]], -1)), dict(atlas_u8=image.transpose(1, 0, 2))]
    for over in bad:
        k = dict(dict(verts=VERTS, faces=FACES, uvs=uv, atlas_u8=image, normals=None), **over)
        with pytest.raises(ValueError, match="write_obj:"):
            mesh_export.write_obj(path, k['verts'], k['faces'], k['uvs'], k['atlas_u8'], k['normals'])
    assert os.listdir(tmp_path) == []                                                  # a refusal writes no file
    assert _image(2, 3).shape == (4, 7, 3)                                             # any R's atlas of F faces is taken
    mesh_export.write_obj(path, VERTS, FACES, mesh_export.atlas_uvs(2, 3), _image(2, 3))
    assert AR.read_png(str(tmp_path / "two.png")).shape == (4, 7, 3)
