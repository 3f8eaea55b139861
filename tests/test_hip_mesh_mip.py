"""-m gpu: nm_mesh_lattice_pyramid and nm_raster_frames_lattice_mip (csrc/mesh_lattice.hip, csrc/raster_frames.hip; include/neuman_hip.h 'mesh
mip', rules M1-M3 and F2''), neuman_hip.mesh_texture.lattice_pyramid and the LatticePyramid route of Rasterizer.render_frames /
render_mesh_frames.

M1 is checked as bits against tests/helpers/mesh_mip_ref.py.  The level choice is checked by exact equalities against nm_raster_frames_lattice
(lod_scale = 0 is level 0, a huge one the coarsest level), the blend against the float64 helper as tests/test_hip_mesh_lattice.py checks F2':
the device is allowed 4 x the float32 helper's own worst deviation from the float64 one, applied through raster_frames_ref.byte_range, never
more than 1 byte, away from the pixels the float64 run calls ambiguous and from those whose rho lies within 1e-5 relative of a power of two
(where sqrtf's and the division's last bit can move the level).  Every output of every raw call sits inside a larger allocation whose guard
elements must stay as they were.  The measured figures are printed ([mesh mip] lines)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mesh_lattice_ref as LR  # noqa: E402
import mesh_mip_ref as MR  # noqa: E402
import raster_frames_ref as FR  # noqa: E402
import raster_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64                                                       # guard elements before and after every output
BUFS = {'out': (torch.uint8, 3, 77), 'face_id': (torch.int32, 1, -77), 'zbuf': (torch.float32, 1, 123.0), 'bary': (torch.float32, 3, 123.0)}
GEOMETRY = ('face_id', 'zbuf', 'bary')
R0 = 8
FAR = 3.0                                                    # "the same mesh from three times the distance"
_SCENE, _FRAME, _PYRAMID = {}, {}, {}


def _scene(name):
    """the scene's numpy arrays (read-only), its device tensors, its batched cameras (its own, and the same views from FAR times the distance)
    and its handle: built once, shared, never written to"""
    if name not in _SCENE:
        from neuman_hip import raster, synthetic
        s = FR.scene(name)
        rng = np.random.default_rng(7)
        s['bg'] = rng.integers(0, 256, (len(s['caps']), s['H'], s['W'], 3), dtype=np.uint8)
        for a in s.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        s['d'] = {k: torch.from_numpy(np.array(s[k])).cuda() for k in ('verts', 'normals', 'colours', 'bg')}
        s['far_caps'] = [synthetic.SimpleCapture(s['W'], s['H'], c2w=synthetic.spherical_c2w(c[0], c[1], FAR * c[2]))
                         for c in (FR.CAMERAS[i] for i in FR.SCENES[name][3])]
        s['cams'] = raster.batch_cameras(s['caps'], 'cuda')
        s['far_cams'] = raster.batch_cameras(s['far_caps'], 'cuda')
        s['rast'] = raster.Rasterizer(s['faces'], s['verts'].shape[1])
        _SCENE[name] = s
    return _SCENE[name]


def _pyramid(name, R=R0):
    """random node colours [F,S,3] in [0, 1] for a scene's mesh and the helper's pyramid of them -> (list of numpy levels, the flat device
    tensor, the device tensors of the levels): made once, shared, never written to"""
    if (name, R) not in _PYRAMID:
        lat = np.random.default_rng(100 + R).random((len(_scene(name)['faces']), LR.lattice_size(R), 3)).astype(np.float32)
        levels = MR.pyramid(lat)
        for a in levels:
            a.setflags(write=False)
        _PYRAMID[name, R] = (levels, torch.from_numpy(MR.flat(levels)).cuda(), [torch.from_numpy(np.array(a)).cuda() for a in levels])
    return _PYRAMID[name, R]


def _frame(name, b, dtype, far=False):
    """the helper's lit frame of a white mesh (geometry, shade, background; the float64 one with its ambiguity map) and the frame's screen
    vertices: one per scene, frame, camera and dtype serves every pyramid, lit and unlit"""
    key = (name, b, np.dtype(dtype).name, far)
    if key not in _FRAME:
        s = _scene(name)
        cam = RR.camera_of(s['far_caps' if far else 'caps'][b])
        fr = LR.frame(s['verts'][b], s['faces'], cam, dtype, normals=s['normals'][b], bg=s['bg'][b], analyse=dtype is np.float64)
        fr['sv'] = MR.screen_vertices(s['verts'][b], cam, dtype)
        for a in fr.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _FRAME[key] = fr
    return _FRAME[key]


def _raw(entry, rast, verts, cams, colours, extra=(), normals=None, light=RR.LIGHT, bg=None, bg_z=None, want_rc=0):
    """one raw call of nm_raster_frames (extra ()), nm_raster_frames_lattice (extra (R,)) or nm_raster_frames_lattice_mip (extra (R0, levels,
    lod_scale)) with every output between guard elements -> dict of numpy arrays [B,...] (and 'error': nm_last_error())"""
    from neuman_hip import _lib
    w2c, intr, W, H = cams
    B = int(verts.shape[0])
    n = B * H * W
    mem = {k: torch.full((G + n * c + G,), fill, device='cuda', dtype=dt) for k, (dt, c, fill) in BUFS.items()}
    ptr = {k: ctypes.c_void_p(mem[k].data_ptr() + G * mem[k].element_size()) for k in mem}
    light_p = None if normals is None else (ctypes.c_double * 3)(*light)
    P = _lib.dev_ptr
    head = (rast._h, P(verts), P(w2c, torch.float64), P(intr, torch.float64), B, W, H)
    tail = (P(normals), light_p, P(bg, torch.uint8), P(bg_z), ptr['out'], ptr['face_id'], ptr['zbuf'], ptr['bary'], _lib.stream_ptr())
    rc = getattr(_lib.lib(), entry)(*head, P(colours), *extra, *tail)
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _lib.lib().nm_last_error())
    res = dict(error=_lib.lib().nm_last_error().decode())
    for k, (dt, c, fill) in BUFS.items():
        a = mem[k].cpu().numpy()
        assert np.all(a[:G] == fill) and np.all(a[G + n * c:] == fill), k                    # the guard elements
        res[k] = a[G:G + n * c].reshape((B, H, W) if c == 1 else (B, H, W, c))
    return res


def _mip(rast, verts, cams, pyramid, levels, lod_scale, R=R0, **kw):
    return _raw("nm_raster_frames_lattice_mip", rast, verts, cams, pyramid, (R, levels, lod_scale), **kw)


def _lat(rast, verts, cams, face_colours, R, **kw):
    return _raw("nm_raster_frames_lattice", rast, verts, cams, face_colours, (R,), **kw)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- M1 ------------------------------------------------------------------------------------------------------------------------------------
def _pyramid_call(lattice, F, R, levels, w, in_place=False, want_rc=0, null=None):
    """one raw nm_mesh_lattice_pyramid call, out between guard elements -> (the flat pyramid float32 [F total w], nm_last_error()).  in_place:
    level 0 is put into out first and out is passed as the lattice too"""
    from neuman_hip import _lib
    n = F * MR.nodes_before(R, max(min(levels, MR.lattice_levels(R)), 1)) * w
    mem = torch.full((G + n + G,), 123.0, device='cuda', dtype=torch.float32)
    out = ctypes.c_void_p(mem.data_ptr() + 4 * G)
    if in_place:
        mem[G:G + lattice.numel()] = lattice.reshape(-1)
    src = out if in_place else _lib.dev_ptr(lattice)
    rc = _lib.lib().nm_mesh_lattice_pyramid(None if null == 'lattice' else src, F, R, levels, w, None if null == 'out' else out, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _lib.lib().nm_last_error())
    a = mem.cpu().numpy()
    assert np.all(a[:G] == 123.0) and np.all(a[G + n:] == 123.0)
    return a[G:G + n], _lib.lib().nm_last_error().decode()


@pytest.mark.parametrize("w", [1, 3, 5])
@pytest.mark.parametrize("R", [1, 2, 4, 6, 12, 64])
def test_every_level_is_the_helpers_bits_and_level_zero_the_inputs_bytes(R, w):
    """R = 1: one level, a copy.  R = 2: a coarser level of corners alone.  R = 4: the smallest with edge nodes in a coarser level (R = 2's
    mid-edge nodes).  R = 6 and 12 stop at an odd level (3), whose node (1, 1) is the smallest interior coarse node.  R = 64: seven levels,
    several workgroups a launch"""
    F = 3
    lat = (np.random.default_rng(1000 * R + w).standard_normal((F, LR.lattice_size(R), w)) * 3).astype(np.float32)
    d_lat = torch.from_numpy(lat).cuda()
    want = MR.pyramid(lat)
    assert len(want) == MR.lattice_levels(R)
    for levels in sorted({1, len(want)}):
        for in_place in (False, True):
            got, _ = _pyramid_call(d_lat, F, R, levels, w, in_place)
            assert _same_bits(got[:lat.size], lat.reshape(-1))                               # level 0: the input byte for byte
            assert _same_bits(got, MR.flat(want[:levels])), (R, w, levels, in_place)
    assert _same_bits(d_lat.cpu().numpy(), lat)                                              # the input is only read


def test_a_lattice_of_vertex_rows_reduces_to_the_lattices_of_the_coarser_resolutions():
    """Linear stays linear: lattice_rows at R = 8 reduced is lattice_rows at 4, 2 and 1 within one float32 ulp.  The rows are colours in
    [0, 1), and the ulp meant is that of their range, 2^-23: rule L2's own value carries roundings of that size whatever the node's
    magnitude (w0 r0 + w1 r1 is rounded at the size of its terms, not of the result), so an ulp of each element would ask for more than
    L2 gives.  Corners are copies: the vertices' rows bit for bit at every level."""
    from neuman_hip import mesh_texture
    s = _scene('three_frames_96x64')
    d_faces = torch.from_numpy(s['faces'].astype(np.int32)).cuda()
    pyr = mesh_texture.lattice_pyramid(mesh_texture.lattice_rows(s['d']['colours'], d_faces, R0), levels=4)      # all of them: down to R = 1
    assert (pyr.R, pyr.levels, pyr.F, pyr.w) == (R0, 4, len(s['faces']), 3) and pyr.data.dtype == torch.float32 and pyr.data.dim() == 1
    ulp = float(np.spacing(np.float32(0.5)) * 2)
    assert ulp == 2.0 ** -23 and float(s['colours'].max()) < 1 and float(s['colours'].min()) >= 0
    for k in range(4):
        R = R0 >> k
        got = pyr.level(k).cpu().numpy()
        want = mesh_texture.lattice_rows(s['d']['colours'], d_faces, R).cpu().numpy()
        assert got.shape == want.shape == (len(s['faces']), LR.lattice_size(R), 3)
        diff = float(np.abs(got.astype(np.float64) - want).max())
        print(f"[mesh mip] vertex rows at R = {R0} reduced to R = {R}: largest difference from lattice_rows {diff:.3e} = {diff / ulp:.2f} ulp of 1")
        assert diff <= ulp
        corners = [LR.node_index(R, 0, 0), LR.node_index(R, R, 0), LR.node_index(R, 0, R)]
        assert _same_bits(got[:, corners], s['colours'][s['faces']])
    assert _same_bits(pyr.data.cpu().numpy(), MR.flat(MR.pyramid(LR.rows(s['colours'], s['faces'], R0, np.float32))))


def test_two_faces_that_agree_on_their_common_edge_agree_on_it_at_every_level():
    lat = np.random.default_rng(3).random((2, LR.lattice_size(R0), 3)).astype(np.float32)
    # face 0 = (0, 1, 2), face 1 = (2, 1, 3): the edge 1-2 is face 0's hypotenuse (i1 = k, i2 = R - k) and face 1's edge i2 = 0 (i1 = k)
    for k in range(R0 + 1):
        lat[1, LR.node_index(R0, k, 0)] = lat[0, LR.node_index(R0, k, R0 - k)]
    got, _ = _pyramid_call(torch.from_numpy(lat).cuda(), 2, R0, 4, 3)
    for l in range(4):
        R, S = R0 >> l, LR.lattice_size(R0 >> l)
        level = got[2 * MR.nodes_before(R0, l) * 3:][:2 * S * 3].reshape(2, S, 3)
        for k in range(R + 1):
            assert _same_bits(level[1, LR.node_index(R, k, 0)], level[0, LR.node_index(R, k, R - k)]), (l, k)
    # and with face 1's edge i1 = 0 on face 0's edge i2 = 0, each in its own indexing
    for k in range(R0 + 1):
        lat[1, LR.node_index(R0, 0, k)] = lat[0, LR.node_index(R0, k, 0)]
    got, _ = _pyramid_call(torch.from_numpy(lat).cuda(), 2, R0, 4, 3)
    for l in range(4):
        R, S = R0 >> l, LR.lattice_size(R0 >> l)
        level = got[2 * MR.nodes_before(R0, l) * 3:][:2 * S * 3].reshape(2, S, 3)
        for k in range(R + 1):
            assert _same_bits(level[1, LR.node_index(R, 0, k)], level[0, LR.node_index(R, k, 0)]), (l, k)


def test_a_bad_levels_w_65_or_a_null_pointer_is_refused_and_nothing_is_written():
    lat = torch.zeros((3, LR.lattice_size(12), 65), device='cuda')
    for R, levels, w, null in ((12, 4, 3, None), (12, 0, 3, None), (12, -1, 3, None), (7, 2, 3, None), (8, 5, 3, None), (12, 3, 65, None), (12, 3, 0, None),
                               (12, 3, 3, 'lattice'), (12, 3, 3, 'out')):
        got, error = _pyramid_call(lat, 3, R, levels, w, want_rc=-1, null=null)
        assert "nm_mesh_lattice_pyramid:" in error and (got == 123.0).all(), (R, levels, w, null, error)


# ---- M2: the level choice by exact equalities against nm_raster_frames_lattice -------------------------------------------------------------
@pytest.mark.parametrize("lit", [True, False], ids=["lit", "unlit"])
@pytest.mark.parametrize("name", list(FR.SCENES))
def test_lod_scale_zero_is_level_zero_and_a_huge_one_the_coarsest_level_byte_for_byte(name, lit):
    s = _scene(name)
    d = s['d']
    _, d_pyr, d_levels = _pyramid(name)
    normals = d['normals'] if lit else None
    old = _raw("nm_raster_frames", s['rast'], d['verts'], s['cams'], d['colours'], normals=normals, bg=d['bg'])
    for lod, k, levels in ((0.0, 0, 4), (1e30, 3, 4), (1e30, 1, 2), (0.0, 0, 1), (1e30, 0, 1)):
        dev = _mip(s['rast'], d['verts'], s['cams'], d_pyr, levels, lod, normals=normals, bg=d['bg'])
        want = _lat(s['rast'], d['verts'], s['cams'], d_levels[k], R0 >> k, normals=normals, bg=d['bg'])
        assert int((dev['face_id'] >= 0).sum()) > 50
        assert np.array_equal(dev['out'], want['out']), (name, lod, levels)
        for key in GEOMETRY:
            assert _same_bits(dev[key], old[key]), (name, lod, key)
    # an odd resolution has one level: at lod_scale = 1 the plain entry
    lat7 = torch.from_numpy(np.random.default_rng(107).random((len(s['faces']), LR.lattice_size(7), 3)).astype(np.float32)).cuda()
    dev = _mip(s['rast'], d['verts'], s['cams'], lat7, 1, 1.0, R=7, normals=normals, bg=d['bg'])
    want = _lat(s['rast'], d['verts'], s['cams'], lat7, 7, normals=normals, bg=d['bg'])
    assert all(_same_bits(dev[key], want[key]) for key in BUFS)


# ---- M2 and M3: the blend against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lit", [True, False], ids=["lit", "unlit"])
@pytest.mark.parametrize("name,lod", [('past_the_scan_240x240', 1.0), ('past_the_scan_240x240', 3.0), ('three_frames_96x64', 1.0)])
def test_random_node_colours_against_the_float64_helper_near_and_far(name, lod, lit):
    """the scenes' own cameras and the same views from three times the distance: past_the_scan_240x240 (faces some 15 pixels wide) shows
    levels 0 to 3 at either lod_scale, three_frames_96x64 (faces two or three pixels wide) levels 1 to 3"""
    s = _scene(name)
    d = s['d']
    levels, d_pyr, _ = _pyramid(name)
    normals = d['normals'] if lit else None
    seen = set()
    for far in (False, True):
        cams = s['far_cams' if far else 'cams']
        dev = _mip(s['rast'], d['verts'], cams, d_pyr, 4, lod, normals=normals, bg=d['bg'])
        old = _raw("nm_raster_frames", s['rast'], d['verts'], cams, d['colours'], normals=normals, bg=d['bg'])
        for k in GEOMETRY:
            assert _same_bits(dev[k], old[k]), (name, far, k)
        for b in range(min(len(s['caps']), 3)):
            f64, f32 = _frame(name, b, np.float64, far), _frame(name, b, np.float32, far)
            r64 = MR.shade(f64, levels, R0, lod, f64['sv'], s['faces'], np.float64, lit=lit, bg=s['bg'][b])
            r32 = MR.shade(f32, levels, R0, lod, f32['sv'], s['faces'], np.float32, lit=lit, bg=s['bg'][b])
            cov = f64['face_id'] >= 0
            near2 = MR.near_power_of_two(r64['rho']) & cov
            amb = f64['ambiguous'] | near2
            ok, both = ~amb, ~amb & cov
            seen |= set(np.unique(r64['level'][both]).tolist())
            tol, f32dev = FR.colour_tolerance(r64, r32, ok & (r64['level'] == r32['level']))
            lo, hi = FR.byte_range(r64['colour'], tol)
            got = dev['out'][b]
            outside = int(((got < lo) | (got > hi))[both].sum())
            byte_err = int(np.abs(got[both].astype(np.int32) - r64['out'][both]).max())
            print(f"[mesh mip] {name} frame {b} {'far' if far else 'near'} lod_scale {lod} {'lit' if lit else 'unlit'}: covered {int(cov.sum())} px, ambiguous "
                  f"{int(f64['ambiguous'].sum())} + {int(near2.sum())} by rho, levels {np.bincount(r64['level'][cov], minlength=4).tolist()}; colour: float32 helper "
                  f"vs float64 {f32dev:.2e}, allowed {tol:.2e}, bytes outside what it allows {outside}, bytes off by at most {byte_err}")
            assert int(cov.sum()) > 50 and int(amb.sum()) <= 0.01 * int(cov.sum())
            assert np.array_equal(dev['face_id'][b][ok], f64['face_id'][ok])
            assert outside == 0 and byte_err <= 1
            none = dev['face_id'][b] < 0
            assert np.array_equal(got[none], s['bg'][b][none])
    assert len(seen) >= 3, seen


def test_a_nan_at_level_zero_only_gives_byte_zero_exactly_where_the_level_choice_reaches_level_zero():
    name, lod = 'past_the_scan_240x240', 1.0
    s = _scene(name)
    d = s['d']
    levels, d_pyr, _ = _pyramid(name)
    poisoned = d_pyr.clone()
    poisoned[:levels[0].size].view(-1, 3)[:, 1] = float('nan')                                 # the green of every level-0 node, and of no other level's
    clean = _mip(s['rast'], d['verts'], s['cams'], d_pyr, 4, lod, bg=d['bg'])
    dev = _mip(s['rast'], d['verts'], s['cams'], poisoned, 4, lod, bg=d['bg'])
    hits = 0
    for b in range(len(s['caps'])):
        sv = MR.screen_vertices(s['verts'][b], RR.camera_of(s['caps'][b]))
        cov = dev['face_id'][b] >= 0
        # the level as rule M2's float32 arithmetic gives it for the device's own winners
        l, t, rho = MR.level_of(sv, s['faces'], dev['face_id'][b][cov], R0, 4, lod, np.float32)
        sure = ~MR.near_power_of_two(rho)
        hit = np.zeros(cov.shape, bool)
        hit[cov] = l == 0
        certain = np.ones(cov.shape, bool)
        certain[cov] = sure
        assert hit.sum() > 1000 and (cov & ~hit).sum() > 100
        assert (dev['out'][b][hit & certain][:, 1] == 0).all()                               # level 0 is read: a NaN whatever t is
        assert np.array_equal(dev['out'][b][~hit & certain], clean['out'][b][~hit & certain])      # level 0 is not read at l >= 1
        assert np.array_equal(dev['out'][b][..., [0, 2]], clean['out'][b][..., [0, 2]])
        hits += int(hit.sum())
    assert hits > 5000


# ---- batch, bad camera, background ---------------------------------------------------------------------------------------------------------
def test_frame_b_of_a_batch_is_the_one_frame_call_on_it_and_two_runs_give_the_same_bytes():
    name = 'three_frames_96x64'
    s = _scene(name)
    d = s['d']
    d_pyr = _pyramid(name)[1]
    whole, again = (_mip(s['rast'], d['verts'], s['cams'], d_pyr, 4, 1.0, normals=d['normals'], bg=d['bg']) for _ in range(2))
    for k in BUFS:
        assert _same_bits(whole[k], again[k]), k                                             # F7
    w2c, intr, W, H = s['cams']
    for b in range(3):
        one = _mip(s['rast'], d['verts'][b:b + 1], (w2c[b:b + 1].contiguous(), intr[b:b + 1].contiguous(), W, H), d_pyr, 4, 1.0, normals=d['normals'][b:b + 1],
                   bg=d['bg'][b:b + 1])
        for k in BUFS:
            assert _same_bits(one[k][0], whole[k][b]), (b, k)


def test_a_frame_with_a_nan_camera_between_ordinary_frames():
    name = 'three_frames_96x64'
    s = _scene(name)
    d = s['d']
    d_pyr = _pyramid(name)[1]
    good = _mip(s['rast'], d['verts'], s['cams'], d_pyr, 4, 1.0, normals=d['normals'], bg=d['bg'])
    w2c, intr, W, H = s['cams']
    w2c = w2c.clone()
    w2c[1, 2, 1] = float('nan')
    bad = _mip(s['rast'], d['verts'], (w2c, intr, W, H), d_pyr, 4, 1.0, normals=d['normals'], bg=d['bg'], want_rc=-1)
    assert "nm_raster_frames_lattice_mip:" in bad['error'] and "frame 1" in bad['error'], bad['error']
    assert (bad['face_id'][1] == -1).all() and np.isposinf(bad['zbuf'][1]).all() and (bad['bary'][1] == 0).all() and np.array_equal(bad['out'][1], s['bg'][1])
    for k in BUFS:                                                                           # F6: reported AFTER every frame's outputs are written
        assert _same_bits(bad[k][0], good[k][0]) and _same_bits(bad[k][2], good[k][2]), k


def test_bg_and_bg_z_byte_for_byte():
    name = 'three_frames_96x64'
    s = _scene(name)
    d = s['d']
    args = (s['rast'], d['verts'], s['cams'], _pyramid(name)[1], 4, 1.0)
    free = _mip(*args, normals=d['normals'], bg=d['bg'])
    cov = free['face_id'] >= 0
    assert np.array_equal(free['out'][~cov], s['bg'][~cov]) and (free['out'][cov] != s['bg'][cov]).any(-1).mean() > 0.9
    z = torch.from_numpy(free['zbuf']).cuda()
    at = _mip(*args, normals=d['normals'], bg=d['bg'], bg_z=z)
    assert np.array_equal(at['out'], s['bg'])                                                # bg_z = zbuf: out == bg byte for byte
    behind = _mip(*args, normals=d['normals'], bg=d['bg'], bg_z=torch.nextafter(z, torch.full_like(z, float('inf'))))
    assert np.array_equal(behind['out'], free['out'])                                        # one step behind: the unoccluded result
    checker = (np.indices(cov.shape).sum(0) % 2).astype(bool)
    mixed = _mip(*args, normals=d['normals'], bg=d['bg'], bg_z=torch.from_numpy(np.where(checker, np.nan, np.inf).astype(np.float32)).cuda())
    assert np.array_equal(mixed['out'], np.where(checker[..., None], s['bg'], free['out']))  # a NaN hides the mesh, +inf never does
    for r in (at, behind, mixed):                                                            # the geometry reports the mesh alone
        for k in GEOMETRY:
            assert _same_bits(r[k], free[k]), k
    white = _mip(*args, normals=d['normals'])
    assert (white['out'][~cov] == 255).all() and np.array_equal(white['out'][cov], free['out'][cov])      # bg = None gives white
    assert (_mip(*args, normals=d['normals'], bg_z=z)['out'] == 255).all()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_the_pyramid_filters_a_stripe_pattern_finer_than_the_pixels():
    """The test that states the feature.  mesh_lattice_ref's capsule thinned on the device; colour = 0.5 + 0.5 sin(2 pi x / wavelength), half
    a mean edge per period (four node spacings of the R = 8 lattice), seen from so far that a period is 1.25 pixels at the capsule's centre.
    Truth: the float64 source at the surface points of a frame of four times the size (the device's geometry), averaged over each pixel's
    4 x 4 sub-samples; only pixels whose 16 sub-samples are all covered count.  The mean absolute error of the pyramid's frame --
    `lattice_pyramid` and `render_mesh_frames` as a caller gets them, lod_scale 1 -- must be below the plain lattice's, and the device's
    ratio may exceed the numpy helper's, on the same mesh and truth, by at most 10 %.

    Measured on an MI355X: plain 0.17574, pyramid 0.14571, ratio 0.8291, the helper on the same mesh and truth 0.8291;
    tests/test_mesh_mip_host.py, the helper alone: the same figures.  With the R = 1 level included
    (levels=4) the ratio is 1.2049, measured on the device and by the helper alike: that level is the three corners, which rule M1 copies,
    so it is the stripes point-sampled at the vertices.  That is why `lattice_pyramid` leaves it out unless asked."""
    from neuman_hip import mesh_simplify, mesh_texture, raster, render_utils, synthetic
    full, full_faces = synthetic.capsule_mesh(*LR.STRIPE_SHAPE)
    verts, faces = mesh_simplify.simplify_mesh(torch.from_numpy(full).cuda(), torch.from_numpy(full_faces.astype(np.int32)).cuda(), LR.STRIPE_CELL,
                                               aabb=LR.STRIPE_BOX)
    v, f = verts.cpu().numpy(), faces.cpu().numpy().astype(np.int64)
    wavelength = MR.stripe_wavelength(v, f)

    def source(points, dirs):
        return (0.5 + 0.5 * torch.sin(2.0 * np.pi * points[:, :1].double() / wavelength)).float().expand(-1, 3)

    normals = torch.from_numpy(RR.vertex_normals(v, f).astype(np.float32)).cuda()
    face_colours = mesh_texture.bake_face_colours(source, verts, faces, normals, LR.STRIPE_R)
    pyramid = mesh_texture.lattice_pyramid(face_colours)
    # the default: every level that has a filtered node, 8, 4 and 2 (mesh_texture.filtered_levels)
    assert (pyramid.R, pyramid.levels, pyramid.F, pyramid.w) == (LR.STRIPE_R, 3, len(f), 3) and torch.equal(pyramid.level(0), face_colours)
    caps, big = MR.far_cameras(wavelength), MR.far_cameras(wavelength, MR.SUPER)
    world = verts[None].expand(len(caps), -1, -1).contiguous()
    by_lattice = render_utils.render_mesh_frames(world, f, caps, face_colours=face_colours).cpu().numpy()
    by_pyramid = render_utils.render_mesh_frames(world, f, caps, face_colours=pyramid).cpu().numpy()
    assert np.array_equal(by_pyramid, render_utils.render_mesh_frames(world, f, caps, face_colours=pyramid, lod_scale=1.0).cpu().numpy())      # the default
    rast = raster.rasterizer_for(f, len(v))
    _, face_id, _, bary = rast.render_frames(world, raster.batch_cameras(caps, 'cuda'), want_geometry=True)
    _, sup_id, _, sup_bary = rast.render_frames(world, raster.batch_cameras(big, 'cuda'), want_geometry=True)
    lat = face_colours.cpu().numpy()
    levels = MR.pyramid(lat, pyramid.levels)
    err = dict(plain=0.0, mip=0.0, ref_plain=0.0, ref_mip=0.0)
    n = 0
    for b in range(len(caps)):
        truth, full_px = MR.box_truth(sup_id[b].cpu().numpy(), sup_bary[b].cpu().numpy(), v, f, wavelength)
        cam = RR.camera_of(caps[b])
        fr = LR.frame(v, f, cam, np.float32)
        score = full_px & (face_id[b].cpu().numpy() >= 0) & (fr['face_id'] >= 0)
        ref_plain = LR.shade(fr, lat, LR.STRIPE_R, np.float32, lit=False)['out']
        ref_mip = MR.shade(fr, levels, LR.STRIPE_R, 1.0, MR.screen_vertices(v, cam), f, np.float32, lit=False)['out']
        for key, img in (('plain', by_lattice[b]), ('mip', by_pyramid[b]), ('ref_plain', ref_plain), ('ref_mip', ref_mip)):
            e, k = MR.mean_abs_error(img, truth, score)
            err[key] += e
        n += k
    ratio, ref_ratio = err['mip'] / err['plain'], err['ref_mip'] / err['ref_plain']
    print(f"[mesh mip] device: {len(v)} vertices, {len(f)} faces, wavelength {wavelength:.4f} = {MR.STRIPE_PIXELS} px; {n // 3} fully covered pixels in the three "
          f"frames; mean |colour error| plain R = {LR.STRIPE_R} lattice {err['plain'] / n:.5f}, pyramid {err['mip'] / n:.5f}, ratio {ratio:.4f}; the helper on the "
          f"same mesh and truth: plain {err['ref_plain'] / n:.5f}, pyramid {err['ref_mip'] / n:.5f}, ratio {ref_ratio:.4f}")
    assert n // 3 > 300
    assert ratio <= 1.10 * ref_ratio
    assert err['mip'] < err['plain']


def test_render_mesh_frames_with_a_pyramid_does_not_depend_on_the_chunking():
    from neuman_hip import _lib, mesh_texture, render_utils
    name = 'past_the_scan_240x240'
    s = _scene(name)
    d, B = s['d'], 5
    levels, d_pyr, d_levels = _pyramid(name)
    pyramid = mesh_texture.lattice_pyramid(d_levels[0], levels=4)
    assert torch.equal(pyramid.data, d_pyr) and all(torch.equal(pyramid.level(k), d_levels[k]) for k in range(4))
    usual = mesh_texture.lattice_pyramid(d_levels[0])                                        # the default leaves the corners-only level out
    assert usual.levels == mesh_texture.filtered_levels(R0) == 3 and torch.equal(usual.data, d_pyr[:usual.data.numel()])
    short = mesh_texture.lattice_pyramid(d_levels[0], levels=2)
    assert short.levels == 2 and torch.equal(short.data, d_pyr[:short.data.numel()])
    kw = dict(normals=d['normals'], background=d['bg'], face_colours=pyramid)
    for lod in (None, 3.0):
        whole = render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], frames_per_call=B, lod_scale=lod, **kw)
        assert whole.dtype == torch.uint8 and tuple(whole.shape) == (B, 240, 240, 3) and whole.is_cuda
        raw = _mip(s['rast'], d['verts'], s['cams'], d_pyr, 4, 1.0 if lod is None else lod, normals=d['normals'], bg=d['bg'])
        assert np.array_equal(whole.cpu().numpy(), raw['out'])
        for step in (2, 1, None):                                                            # 2 + 2 + 1; one by one; the default
            assert torch.equal(render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], frames_per_call=step, lod_scale=lod, **kw), whole), step
    out, face_id, zbuf, bary = s['rast'].render_frames(d['verts'], s['cams'], normals=d['normals'], background=d['bg'], want_geometry=True, face_colours=pyramid,
                                                       lod_scale=3.0)
    assert torch.equal(out, whole) and all(_same_bits(t.cpu().numpy(), raw[k]) for t, k in ((face_id, 'face_id'), (zbuf, 'zbuf'), (bary, 'bary')))
    # a plain tensor goes where it goes today, and a level is a plain tensor
    plain = render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], normals=d['normals'], background=d['bg'], face_colours=pyramid.level(1))
    assert np.array_equal(plain.cpu().numpy(), _lat(s['rast'], d['verts'], s['cams'], d_levels[1], R0 >> 1, normals=d['normals'], bg=d['bg'])['out'])
    with pytest.raises(ValueError, match="lod_scale goes with"):
        render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], face_colours=d_levels[0], lod_scale=1.0)
    with pytest.raises(ValueError, match="lod_scale goes with"):
        s['rast'].render_frames(d['verts'], s['cams'], face_colours=d_levels[0], lod_scale=0.0)
    for lod in (float('nan'), float('inf'), -1.0):
        with pytest.raises(_lib.NeumanHipError, match="lod_scale"):
            render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], face_colours=pyramid, lod_scale=lod)
    with pytest.raises(ValueError, match="not both"):
        s['rast'].render_frames(d['verts'], s['cams'], d['colours'], face_colours=pyramid)
    with pytest.raises(_lib.NeumanHipError):
        mesh_texture.lattice_pyramid(d_levels[0].cpu())


def test_export_mesh_and_pack_atlas_accept_a_level_of_a_pyramid(tmp_path):
    from neuman_hip import mesh_export, mesh_texture
    s = _scene('three_frames_96x64')
    _, _, d_levels = _pyramid('three_frames_96x64')
    pyramid = mesh_texture.lattice_pyramid(d_levels[0])
    atlas = mesh_export.pack_atlas(pyramid.level(1))
    assert torch.equal(atlas, mesh_export.pack_atlas(d_levels[1].clone()))
    verts = s['d']['verts'][0].contiguous()
    faces = torch.from_numpy(s['faces'].astype(np.int32)).cuda()
    paths = mesh_export.export_mesh(str(tmp_path / "body.obj"), verts, faces, pyramid.level(1))
    assert all(os.path.getsize(p) > 0 for p in paths)


def test_lattice_levels_and_lattice_resolution_rounded_up_to_a_power_of_two():
    from neuman_hip import mesh_texture, synthetic
    assert [mesh_texture.lattice_levels(R) for R in (1, 2, 3, 4, 6, 8, 12, 64)] == [1, 2, 1, 3, 2, 4, 3, 7]
    v, f = synthetic.capsule_mesh(12, 10)
    verts, faces = torch.from_numpy(v).cuda(), torch.from_numpy(f.astype(np.int32)).cuda()
    longest = max(float(np.linalg.norm(v[f[:, k]].astype(np.float64) - v[f[:, (k + 1) % 3]], axis=1).max()) for k in range(3))
    for texel, want, want2 in ((longest * 10, 1, 1), (longest / 1.5, 2, 2), (longest / 2.5, 3, 4), (longest / 4.5, 5, 8), (longest / 7.99, 8, 8),
                               (longest / 8.5, 9, 16), (longest / 32.5, 33, 64), (longest / 1000, 64, 64)):
        for kw, expect in ((dict(), want), (dict(pow2=False), want), (dict(pow2=True), want2)):
            R = mesh_texture.lattice_resolution(verts, faces, texel, **kw)
            assert type(R) is int and R == expect, (texel, kw, R, expect)
        assert mesh_texture.lattice_levels(want2) == want2.bit_length()                      # a power of two: the pyramid goes down to R = 1
