"""-m gpu: the rasterisers exactly where pixel centres lie on edges -- nm_raster_mesh, nm_raster_phong, nm_raster_frames and
nm_raster_silhouette (with its batch form) on the quarter-pixel scenes of tests/helpers/raster_exact.py, against that file's integer and
rational reference, at EVERY pixel and with NO tolerance.

The other parity tests of this family (test_hip_raster.py, test_hip_raster_frames.py, test_hip_silhouette.py, the lattice and mip tests)
compare with the float64 helper and must leave out the pixels it calls ambiguous: a centre within 1e-4 of an edge, two depths within 1e-4.
On these scenes nothing is ambiguous: every float32 operand of csrc/raster_device.h's edge_functions, covers, tile_box and depth_test is
exact, depth and barycentrics are one correctly rounded float32 division of exactly known numbers (the build has no fast-math flag and
-ffp-contract=off), so the reference predicts the device's bits -- a centre on a shared edge belongs to both faces, one on a vertex to the
whole fan, an exact depth tie goes to the lower face id, a box that ends on a tile seam or the image border still reaches the pixel whose
centre lies on it, and a face of zero area or with a vertex at z <= 0 never appears.  tests/test_raster_exact_host.py checks the reference
itself and that each scene still has the centres on edges and vertices it declares.

The one thing not compared is the sign of a zero: a barycentric of exactly 0 may come out as -0.0 (a difference of products of either sign),
which the contract does not speak of; zeros are compared as equal, everything else bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import raster_exact as RX  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = list(RX.SCENES)
_DEV = {}


def _bits(a):
    """float32 -> its bits, -0.0 as +0.0"""
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.int32)


def _rasterize(sc, faces=None, shade=False):
    from neuman_hip import raster
    faces = sc.faces if faces is None else faces
    v = torch.tensor(sc.verts).cuda()
    out = raster.rasterizer_for(faces, len(sc.verts)).rasterize(v, sc.camera, shade=shade)
    return {k: a.cpu().numpy() for k, a in zip(('face_id', 'zbuf', 'bary', 'rgba'), out) if a is not None}


def _mesh_run(name):
    """nm_raster_mesh on a scene: run once, shared, never written to"""
    if name not in _DEV:
        _DEV[name] = _rasterize(RX.SCENES[name])
        for a in _DEV[name].values():
            a.setflags(write=False)
    return _DEV[name]


def _assert_exact(tag, name, dev, ex):
    """ids at every pixel, depth and barycentrics bit for bit; the figures are printed before anything is asserted"""
    n = {k: int((_bits(dev[k]) != _bits(ex[k])).sum()) for k in ('zbuf', 'bary')}
    n['face_id'] = int((dev['face_id'] != ex['face_id']).sum())
    cov = ex['face_id'] >= 0
    with np.errstate(invalid='ignore'):
        ulp = {k: int(np.abs(_bits(dev[k]).astype(np.int64) - _bits(ex[k]))[cov].max()) if cov.any() else 0 for k in ('zbuf', 'bary')}
    print(f"[raster-exact] {tag} {name}: {ex['face_id'].size} px compared, {int(cov.sum())} covered, {ex['on_edge']} centres on an edge, {ex['on_vertex']} on a "
          f"vertex; mismatches: face_id {n['face_id']}, zbuf {n['zbuf']} (worst {ulp['zbuf']} ulp), bary {n['bary']} (worst {ulp['bary']} ulp)")
    assert dev['face_id'].dtype == np.int32 and dev['face_id'].shape == ex['face_id'].shape
    assert n['face_id'] == 0, np.argwhere(dev['face_id'] != ex['face_id'])[:8].tolist()
    assert n['zbuf'] == 0 and n['bary'] == 0, (n, ulp)


@pytest.mark.parametrize("name", NAMES)
def test_raster_mesh(name):
    sc, ex = RX.SCENES[name], RX.exact_of(name)
    dev = _mesh_run(name)
    _assert_exact('nm_raster_mesh', name, dev, ex)
    again = _rasterize(sc)
    for k in dev:
        assert np.array_equal(again[k].view(np.int32), dev[k].view(np.int32)), k             # two runs: the same bits, signs of zeros included
    # a permuted face list: the same depths; the same faces where the expected result does not depend on the ids
    perm = np.random.default_rng(len(sc.faces)).permutation(len(sc.faces))
    p = _rasterize(sc, sc.faces[perm])
    assert np.array_equal(_bits(p['zbuf']), _bits(dev['zbuf']))
    if not sc.id_dependent:
        cov = dev['face_id'] >= 0
        assert np.array_equal(p['face_id'] >= 0, cov) and np.array_equal(perm[p['face_id'][cov]], dev['face_id'][cov])
    elif len(sc.faces) <= 16:                                   # where it does (ties): the permuted list is a scene of its own, with its own lower ids
        moved = RX.Scene(name + '-permuted', sc.verts, sc.faces[perm], sc.W, sc.H, sc.fx, sc.fy, sc.cx, sc.cy, sc.w2c[:, 3])
        _assert_exact('nm_raster_mesh, faces permuted,', name, p, RX.exact_rasterize(moved))


@pytest.mark.parametrize("name", NAMES)
def test_raster_phong(name):
    sc, ex = RX.SCENES[name], RX.exact_of(name)
    dev = _rasterize(sc, shade=True)
    _assert_exact('nm_raster_phong', name, dev, ex)
    plain = _mesh_run(name)
    for k in ('face_id', 'zbuf', 'bary'):
        assert np.array_equal(dev[k].view(np.int32), plain[k].view(np.int32)), k
    cov = ex['face_id'] >= 0
    assert np.all(dev['rgba'][..., 3][cov] == 1) and np.all(dev['rgba'][~cov] == np.array([1, 1, 1, 0], np.float32))
    assert np.array_equal(dev['rgba'][..., 3] == 1, cov)


def _three_frames(sc):
    """the scene as frame 1 between two other scenes of the same topology: its vertices mirrored, and moved"""
    v = sc.verts
    verts = np.stack([v * np.array([-1, 1, 1], np.float32), v, v + np.array([0.375, -0.25, 0.5], np.float32)])
    w2c = np.tile(np.eye(4), (3, 1, 1))
    w2c[:, :3] = sc.w2c
    intr = np.tile(np.array([sc.fx, sc.fy, sc.cx, sc.cy]), (3, 1))
    return torch.as_tensor(verts).cuda(), (torch.as_tensor(w2c).cuda(), torch.as_tensor(intr).cuda(), sc.W, sc.H)


@pytest.mark.parametrize("name", NAMES)
def test_raster_frames(name):
    from neuman_hip import raster
    sc, ex = RX.SCENES[name], RX.exact_of(name)
    R = raster.rasterizer_for(sc.faces, len(sc.verts))
    verts, cams = _three_frames(sc)
    H, W = sc.H, sc.W
    bg = np.random.default_rng(7).integers(0, 200, (3, H, W, 3), dtype=np.uint8)       # never the white mesh's 255
    bg_d = torch.as_tensor(bg).cuda()

    def run(bg_z=None):
        out, face_id, zbuf, bary = R.render_frames(verts, cams, background=bg_d, background_z=None if bg_z is None else torch.as_tensor(bg_z).cuda(),
                                                   want_geometry=True)
        return out.cpu().numpy(), dict(face_id=face_id[1].cpu().numpy(), zbuf=zbuf[1].cpu().numpy(), bary=bary[1].cpu().numpy())

    cov = ex['face_id'] >= 0
    out, geo = run()
    _assert_exact('nm_raster_frames', name, geo, ex)
    assert np.array_equal((out[1] != bg[1]).any(-1), cov) and np.all(out[1][cov] == 255)     # the background's bytes on exactly the uncovered pixels
    # F4 is strict: a background at exactly the face's depth hides the mesh, one float32 further away does not; the geometry reports the mesh alone
    bg_z = np.full((3, H, W), np.inf, np.float32)
    bg_z[1] = np.where(cov, ex['zbuf'], np.float32(1e9))
    out_eq, geo_eq = run(bg_z)
    _assert_exact('nm_raster_frames, bg_z == z', name, geo_eq, ex)
    assert np.array_equal(out_eq[1], bg[1])
    bg_z[1] = np.where(cov, np.nextafter(ex['zbuf'], np.float32(np.inf)), np.float32(1e9))
    out_gt, _ = run(bg_z)
    assert np.array_equal(out_gt[1], out[1])
    for b in (0, 2):
        assert np.array_equal(out_eq[b], out[b])


def _silhouette(sc, blur_radius, batch=False):
    from neuman_hip import raster
    R = raster.rasterizer_for(sc.faces, len(sc.verts))
    if batch:
        verts, cams = _three_frames(sc)
        out = [a[1] for a in R.silhouette_batch(verts, cams, blur_radius=blur_radius, want_count=True)]
    else:
        out = R.silhouette(torch.tensor(sc.verts).cuda(), sc.camera, blur_radius=blur_radius, want_count=True)
    return dict(zip(('alpha', 'keep', 'n_cand'), (a.cpu().numpy() for a in out)))


@pytest.mark.parametrize("name", NAMES)
def test_raster_silhouette(name):
    sc, ex = RX.SCENES[name], RX.exact_of(name)
    n_cover = ex['n_cover']
    hard, soft = _silhouette(sc, 0.0), _silhouette(sc, None)
    print(f"[raster-exact] nm_raster_silhouette {name}: {n_cover.size} px compared, n_cand != n_cover on {int((hard['n_cand'] != n_cover).sum())} at blur 0, "
          f"n_cand < n_cover on {int((soft['n_cand'] < n_cover).sum())} at the default blur")
    # blur 0: a candidate is a face that covers the centre, by the rasteriser's own closed-edge test and rejection
    assert np.array_equal(hard['n_cand'], n_cover), np.argwhere(hard['n_cand'] != n_cover)[:8].tolist()
    assert np.all(hard['alpha'][n_cover == 0] == 0) and np.all(hard['keep'][n_cover == 0] == 1) and np.all(hard['alpha'][n_cover > 0] >= 0.5)
    assert np.all(soft['n_cand'] >= n_cover) and np.all(soft['alpha'][n_cover > 0] >= 0.5)
    if name.startswith('fan'):                                  # at the hub every edge distance is 0: each of the k faces gives exactly 1/2
        hub = int(float(name.split('-')[1][3:]))
        k = int(n_cover[hub, hub])
        assert k == 8 and hard['keep'][hub, hub] == np.float32(0.5 ** k) and soft['keep'][hub, hub] == np.float32(0.5 ** k)
        assert hard['alpha'][hub, hub] == np.float32(1 - 0.5 ** k)
    if name == 'rejected':                                      # the dropped faces add nothing, at either radius: the bits of the scene without them
        for blur, got in ((0.0, hard), (None, soft)):
            want = _silhouette(RX.SCENES['rejected-without'], blur)
            for k in got:
                assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (blur, k)
    for blur, one in ((0.0, hard), (None, soft)):               # the batch entry, the scene as frame 1 of 3: the one-frame bits
        many = _silhouette(sc, blur, batch=True)
        for k in one:
            assert np.array_equal(many[k].view(np.int32), one[k].view(np.int32)), (blur, k)
