"""-m gpu: nm_raster_frames (csrc/raster_frames.hip; include/neuman_hip.h 'mesh frames', rules F1-F7), raster.Rasterizer.render_frames and
render_utils.render_mesh_frames / depth_to_camera_z.

F1 is checked as bits against nm_raster_mesh frame by frame; F2, F3 and F5 against the float64 restatement tests/helpers/raster_frames_ref.py,
calibrated as tests/test_hip_raster.py calibrates: the helper also runs in float32, and the device is allowed 4 x that run's own worst
deviation from the float64 run on the same input (floor: 1e-6 relative).  The device returns the colour as bytes only, so the allowance on the
colour is applied where it can be seen: the device's byte must be one that F5 makes of SOME colour within the allowance of the float64 colour
(raster_frames_ref.byte_range), and is never off by more than 1.  All of that away from the pixels the float64 run itself calls ambiguous
(tests/test_raster_frames_host.py holds them to 1 % of the covered pixels on the CPU).  F4 and F7 are byte for byte.  Every output of every raw
call sits inside a larger allocation whose guard elements must stay as they were.  The measured deviations are printed ([raster frames] lines)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import raster_frames_ref as FR  # noqa: E402
import raster_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

G = 64                                                       # guard elements before and after every output
BUFS = {'out': (torch.uint8, 3, 77), 'face_id': (torch.int32, 1, -77), 'zbuf': (torch.float32, 1, 123.0), 'bary': (torch.float32, 3, 123.0)}
_SCENE, _REF = {}, {}


def _scene(name):
    """the scene's numpy arrays (read-only), its device tensors, its batched cameras and its handle: built once, shared, never written to"""
    if name not in _SCENE:
        from neuman_hip import raster
        s = FR.scene(name)
        for a in s.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        s['d'] = {k: torch.from_numpy(np.array(s[k])).cuda() for k in ('verts', 'normals', 'colours')}
        s['cams'] = raster.batch_cameras(s['caps'], 'cuda')
        s['rast'] = raster.Rasterizer(s['faces'], s['verts'].shape[1])
        rng = np.random.default_rng(7)
        s['bg'] = rng.integers(0, 256, (len(s['caps']), s['H'], s['W'], 3), dtype=np.uint8)
        s['bg'].setflags(write=False)
        s['d']['bg'] = torch.from_numpy(np.array(s['bg'])).cuda()
        _SCENE[name] = s
    return _SCENE[name]


def _reference(name, b, variant):
    """float64 run (with its ambiguity map), the tolerances on zbuf and bary and the one on the colour, of one frame of one scene under one
    variant of the inputs: computed once, shared, never written to"""
    key = (name, b, variant)
    if key not in _REF:
        s = _scene(name)
        kw = _variant(s, variant, np)
        kw = {k: (v[b] if k == 'normals' and v is not None else v) for k, v in kw.items()}
        cam = RR.camera_of(s['caps'][b])
        r64 = FR.render(s['verts'][b], s['faces'], cam, np.float64, bg=s['bg'][b], analyse=True, **kw)
        r32 = FR.render(s['verts'][b], s['faces'], cam, np.float32, bg=s['bg'][b], **kw)
        ok = ~r64['ambiguous']
        tol, dev = RR.tolerances(r64, r32, ok)
        tol['colour'], dev['colour'] = FR.colour_tolerance(r64, r32, ok)
        for a in r64.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = (r64, tol, dev)
    return _REF[key]


VARIANTS = ('colours_and_normals', 'colours_alone', 'normals_alone', 'a_nan_colour')


def _variant(s, variant, where):
    """the colours and normals of a variant, as numpy arrays (where = np) or as the scene's device tensors"""
    src = s if where is np else s['d']
    colours = None if variant == 'normals_alone' else src['colours']
    if variant == 'a_nan_colour':
        colours = np.array(s['colours'])
        colours[::7, 1] = np.nan                                                             # the green of every seventh vertex
        colours = colours if where is np else torch.from_numpy(colours).cuda()
    return dict(colours=colours, normals=src['normals'] if variant in ('colours_and_normals', 'normals_alone') else None)


def _frames(rast, verts, cams, colours=None, normals=None, light=RR.LIGHT, bg=None, bg_z=None, want_rc=0):
    """one raw nm_raster_frames call with every output between guard elements -> dict of numpy arrays [B,...] (and 'error': nm_last_error())"""
    from neuman_hip import _lib
    w2c, intr, W, H = cams
    B = int(verts.shape[0])
    n = B * H * W
    mem = {k: torch.full((G + n * c + G,), fill, device='cuda', dtype=dt) for k, (dt, c, fill) in BUFS.items()}
    ptr = {k: ctypes.c_void_p(mem[k].data_ptr() + G * mem[k].element_size()) for k in mem}
    light_p = None if normals is None else (ctypes.c_double * 3)(*light)
    P = _lib.dev_ptr
    rc = _lib.lib().nm_raster_frames(rast._h, P(verts), P(w2c, torch.float64), P(intr, torch.float64), B, W, H, P(colours), P(normals), light_p,
                                     P(bg, torch.uint8), P(bg_z), ptr['out'], ptr['face_id'], ptr['zbuf'], ptr['bary'], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _lib.lib().nm_last_error())
    res = dict(error=_lib.lib().nm_last_error().decode())
    for k, (dt, c, fill) in BUFS.items():
        a = mem[k].cpu().numpy()
        assert np.all(a[:G] == fill) and np.all(a[G + n * c:] == fill), k                    # the guard elements
        res[k] = a[G:G + n * c].reshape((B, H, W) if c == 1 else (B, H, W, c))
    return res


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _sub(cams, idx):
    w2c, intr, W, H = cams
    return w2c[idx].contiguous(), intr[idx].contiguous(), W, H


# ---- F1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FR.SCENES))
def test_geometry_is_nm_raster_meshs_bits_frame_by_frame_wherever_the_frame_sits(name):
    """96 x 64 with three cameras and vertex sets; 50 x 37 (neither side a multiple of the tile); five frames of 225 tiles (1125 (frame, tile)
    pairs for a scan of 1024 threads); 16 x 16 with every face in one tile's list"""
    from neuman_hip import raster
    s = _scene(name)
    d, B = s['d'], len(s['caps'])
    whole = _frames(s['rast'], d['verts'], s['cams'], d['colours'], d['normals'], bg=d['bg'])
    for b in range(B):
        face_id, zbuf, bary, _ = s['rast'].rasterize(d['verts'][b], raster.camera_of(s['caps'][b]))
        assert int((face_id >= 0).sum()) > 50
        for k, one in (('face_id', face_id), ('zbuf', zbuf), ('bary', bary)):
            assert _same_bits(whole[k][b], one.cpu().numpy()), (name, b, k)
    # the first frame at the end of a batch, and alone
    order = list(range(1, B)) + [0]
    moved = _frames(s['rast'], d['verts'][order].contiguous(), _sub(s['cams'], order), d['colours'], d['normals'][order].contiguous(), bg=d['bg'][order].contiguous())
    alone = _frames(s['rast'], d['verts'][:1], _sub(s['cams'], [0]), d['colours'], d['normals'][:1], bg=d['bg'][:1])
    for k in BUFS:
        assert _same_bits(moved[k][B - 1], whole[k][0]) and _same_bits(alone[k][0], whole[k][0]), (name, k)
        assert _same_bits(moved[k][:B - 1], whole[k][1:]), (name, k)


# ---- F2, F3, F5 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [('three_frames_96x64', v) for v in VARIANTS] + [(n, 'colours_and_normals') for n in list(FR.SCENES)[1:]])
def test_colour_light_and_bytes_against_the_float64_helper(name, variant):
    s = _scene(name)
    dev = _frames(s['rast'], s['d']['verts'], s['cams'], bg=s['d']['bg'], **_variant(s, variant, torch))
    for b in range(len(s['caps'])):
        r64, tol, f32dev = _reference(name, b, variant)
        amb, cov = r64['ambiguous'], r64['face_id'] >= 0
        ok, both = ~amb, ~amb & cov
        err = {k: float(np.abs(dev[k][b][both].astype(np.float64) - r64[k][both]).max()) for k in ('zbuf', 'bary')}
        lo, hi = FR.byte_range(r64['colour'], tol['colour'])
        got = dev['out'][b]
        outside = int(((got < lo) | (got > hi))[both].sum())
        byte_err = int(np.abs(got[both].astype(np.int32) - r64['out'][both]).max())
        print(f"[raster frames] {name} frame {b} {variant}: covered {int(cov.sum())} px, ambiguous {int(amb.sum())}, face-id mismatches off them "
              f"{int((dev['face_id'][b] != r64['face_id'])[ok].sum())}; device vs float64 | float32 helper vs float64 | allowed: "
              + ", ".join(f"{k} {err[k]:.2e} | {f32dev[k]:.2e} | {tol[k]:.2e}" for k in err)
              + f"; colour: float32 helper vs float64 {f32dev['colour']:.2e}, allowed {tol['colour']:.2e}, bytes outside what it allows {outside}, "
              f"bytes off by at most {byte_err}")
        assert int(cov.sum()) > 50 and int(amb.sum()) <= 0.01 * int(cov.sum())
        assert np.array_equal(dev['face_id'][b][ok], r64['face_id'][ok])
        for k in err:
            assert err[k] <= tol[k], (k, err[k], tol[k])
        assert outside == 0 and byte_err <= 1
        none = dev['face_id'][b] < 0
        assert np.array_equal(got[none], s['bg'][b][none])                                   # F5: every other pixel takes bg's bytes
        if variant == 'a_nan_colour':
            nan = np.isnan(r64['colour'][..., 1]) & both
            assert nan.sum() > 20 and (got[nan][:, 1] == 0).all() and not np.isnan(r64['colour'][..., 0]).any()


# ---- F4 ------------------------------------------------------------------------------------------------------------------------------------
def test_occlusion_is_a_strict_comparison_that_leaves_the_geometry_alone():
    s = _scene('three_frames_96x64')
    d = s['d']
    args = (s['rast'], d['verts'], s['cams'], d['colours'], d['normals'])
    free = _frames(*args, bg=d['bg'])
    cov = free['face_id'] >= 0
    assert (free['out'][cov] != s['bg'][cov]).any(-1).mean() > 0.9                           # (the mesh shows: random bytes rarely equal its own)
    z = torch.from_numpy(free['zbuf']).cuda()
    at = _frames(*args, bg=d['bg'], bg_z=z)
    assert np.array_equal(at['out'], s['bg'])                                                # bg_z = zbuf: out == bg byte for byte
    behind = _frames(*args, bg=d['bg'], bg_z=torch.nextafter(z, torch.full_like(z, float('inf'))))
    assert np.array_equal(behind['out'], free['out'])                                        # one step behind: the unoccluded result
    checker = (np.indices(cov.shape).sum(0) % 2).astype(bool)
    mixed = _frames(*args, bg=d['bg'], bg_z=torch.from_numpy(np.where(checker, np.nan, np.inf).astype(np.float32)).cuda())
    assert np.array_equal(mixed['out'], np.where(checker[..., None], s['bg'], free['out']))  # a NaN hides the mesh, +inf never does
    assert (cov & checker).sum() > 100 and (cov & ~checker).sum() > 100
    for r in (at, behind, mixed):                                                            # the geometry reports the mesh alone
        for k in ('face_id', 'zbuf', 'bary'):
            assert _same_bits(r[k], free[k]), k
    white = _frames(*args)
    assert (white['out'][~cov] == 255).all() and np.array_equal(white['out'][cov], free['out'][cov])      # bg = None gives white
    assert (_frames(*args, bg_z=z)['out'] == 255).all()


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_a_frame_behind_the_camera_and_a_frame_with_a_nan_camera_between_ordinary_frames():
    from neuman_hip import raster, synthetic
    s = _scene('three_frames_96x64')
    d = s['d']
    good = _frames(s['rast'], d['verts'], s['cams'], d['colours'], d['normals'], bg=d['bg'])
    # the middle frame seen by a camera that looks the other way: every vertex behind it, empty lists
    caps = list(s['caps'])
    caps[1] = synthetic.SimpleCapture(s['W'], s['H'], c2w=caps[1].cam_pose.camera_to_world @ np.diag([1., -1., -1., 1.]))
    away = _frames(s['rast'], d['verts'], raster.batch_cameras(caps, 'cuda'), d['colours'], d['normals'], bg=d['bg'])
    # ... and with a NaN in its w2c: found on the device, reported after every frame's outputs are written
    w2c, intr, W, H = s['cams']
    w2c = w2c.clone()
    w2c[1, 2, 1] = float('nan')
    bad = _frames(s['rast'], d['verts'], (w2c, intr, W, H), d['colours'], d['normals'], bg=d['bg'], want_rc=-1)
    assert "nm_raster_frames:" in bad['error'] and "frame 1" in bad['error'], bad['error']
    for r in (away, bad):
        assert (r['face_id'][1] == -1).all() and np.isposinf(r['zbuf'][1]).all() and (r['bary'][1] == 0).all() and np.array_equal(r['out'][1], s['bg'][1])
        for k in BUFS:
            assert _same_bits(r[k][0], good[k][0]) and _same_bits(r[k][2], good[k][2]), k
    intr = intr.clone()
    intr[2, 0] = float('inf')
    worse = _frames(s['rast'], d['verts'], (w2c, intr, W, H), d['colours'], d['normals'], bg=d['bg'], want_rc=-1)
    assert "frame 1" in worse['error'] and (worse['face_id'][1:] == -1).all() and _same_bits(worse['out'][0], good['out'][0])      # the FIRST such frame


# ---- F7 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['three_frames_96x64', 'one_tile_16x16'])
def test_two_runs_are_byte_identical_and_the_order_of_the_faces_does_not_show(name):
    from neuman_hip import raster
    s = _scene(name)
    d = s['d']
    a, b = (_frames(s['rast'], d['verts'], s['cams'], d['colours'], d['normals'], bg=d['bg']) for _ in range(2))
    for k in BUFS:
        assert _same_bits(a[k], b[k]), k
    perm = np.random.default_rng(5).permutation(len(s['faces']))
    p = _frames(raster.Rasterizer(s['faces'][perm], s['verts'].shape[1]), d['verts'], s['cams'], d['colours'], d['normals'], bg=d['bg'])
    assert _same_bits(p['zbuf'], a['zbuf'])                                                  # bit-identical
    for f in range(len(s['caps'])):
        ok = ~_reference(name, f, 'colours_and_normals')[0]['ambiguous']
        cov = ok & (a['face_id'][f] >= 0)
        assert np.array_equal(p['face_id'][f] >= 0, a['face_id'][f] >= 0) and np.array_equal(perm[p['face_id'][f][cov]], a['face_id'][f][cov])
        assert np.array_equal(p['out'][f][ok], a['out'][f][ok])


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_render_mesh_frames_does_not_depend_on_the_chunking_and_takes_both_background_shapes():
    from neuman_hip import render_utils
    s = _scene('past_the_scan_240x240')
    d, B = s['d'], 5
    kw = dict(colours=d['colours'], normals=d['normals'], background=d['bg'])
    whole = render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], frames_per_call=B, **kw)
    assert whole.dtype == torch.uint8 and tuple(whole.shape) == (B, 240, 240, 3) and whole.is_cuda
    raw = _frames(s['rast'], d['verts'], s['cams'], d['colours'], d['normals'], bg=d['bg'])
    assert np.array_equal(whole.cpu().numpy(), raw['out'])
    for step in (2, 1, None):                                                                # 2 + 2 + 1; one by one; the default
        assert torch.equal(render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], frames_per_call=step, **kw), whole), step
    assert torch.equal(render_utils.render_mesh_frames(d['verts'], s['faces'], s['cams'], **kw), whole)          # batch_cameras' tuple for the captures
    one = d['bg'][3].contiguous()                                                            # [H,W,3]: the same background for all frames
    shared = render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], colours=d['colours'], normals=d['normals'], background=one, frames_per_call=2)
    tiled = render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], colours=d['colours'], normals=d['normals'],
                                            background=one[None].expand(B, -1, -1, -1).contiguous())
    assert torch.equal(shared, tiled) and not torch.equal(shared, whole)
    # Rasterizer.render_frames: the same call, with the geometry
    out, face_id, zbuf, bary = s['rast'].render_frames(d['verts'], s['cams'], d['colours'], d['normals'], background=d['bg'], want_geometry=True)
    assert torch.equal(out, whole) and _same_bits(face_id.cpu().numpy(), raw['face_id']) and _same_bits(zbuf.cpu().numpy(), raw['zbuf'])
    assert _same_bits(bary.cpu().numpy(), raw['bary'])
    # background_depth: a plane across the capsule, given as the renderers give depth (distance along the ray)
    plane = float(np.median(raw['zbuf'][np.isfinite(raw['zbuf'])]))
    rays = [render_utils.depth_to_camera_z(torch.ones((240, 240), device='cuda'), c) for c in s['caps']]          # z per unit of distance
    depth = torch.stack([plane / r for r in rays])
    bg_z = torch.stack([render_utils.depth_to_camera_z(depth[b], s['caps'][b]) for b in range(B)])
    assert float((bg_z - plane).abs().max()) < 1e-5 * plane
    cut = render_utils.render_mesh_frames(d['verts'], s['faces'], s['caps'], background_depth=depth, frames_per_call=2, **kw)
    want = _frames(s['rast'], d['verts'], s['cams'], d['colours'], d['normals'], bg=d['bg'], bg_z=bg_z)['out']
    assert np.array_equal(cut.cpu().numpy(), want)
    hidden = (want != raw['out']).any(-1)
    assert hidden.sum() > 500 and (~hidden & (raw['face_id'] >= 0)).sum() > 500              # the plane hides part of the capsule and shows the rest


def test_bind_pose_render_end_to_end():
    """a small canonical mesh (the body's capsule grown by 15 %) bound to the synthetic body, posed by two twists, rendered with the posed normals"""
    from neuman_hip import mesh_pose, render_utils, synthetic
    body_v, body_f = synthetic.capsule_mesh(12, 10)
    verts = torch.from_numpy(body_v * np.float32(1.15)).cuda()
    normals = torch.from_numpy(RR.vertex_normals(body_v, body_f).astype(np.float32)).cuda()
    colours = torch.from_numpy(np.random.default_rng(3).random((len(body_v), 3)).astype(np.float32)).cuda()
    binding = mesh_pose.bind_mesh(verts, body_v, body_f)
    T = torch.from_numpy(np.stack([synthetic.twist_transforms(body_v, twist)[1] for twist in (0.8, -0.5)])).cuda()
    posed, posed_n = mesh_pose.pose_mesh(verts, binding, T, normals=normals, check=True)
    caps = [synthetic.SimpleCapture(48, 48, c2w=synthetic.spherical_c2w(a, -20, 4.0), far=8.0) for a in (30, 120)]
    frames = render_utils.render_mesh_frames(posed, body_f, caps, colours=colours, normals=posed_n)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 48, 48, 3)
    from neuman_hip import raster
    out, face_id, zbuf, bary = raster.rasterizer_for(body_f, len(body_v)).render_frames(posed, raster.batch_cameras(caps, 'cuda'), colours, posed_n, want_geometry=True)
    assert torch.equal(out, frames)
    for b in range(2):
        f1, z1, b1 = render_utils.rasterize_mesh(posed[b], body_f, caps[b])
        assert _same_bits(face_id[b].cpu().numpy(), f1.cpu().numpy()) and _same_bits(zbuf[b].cpu().numpy(), z1.cpu().numpy())
        assert _same_bits(bary[b].cpu().numpy(), b1.cpu().numpy())
        cov = (f1 >= 0)
        assert 30 < int(cov.sum()) < 48 * 48
        assert bool((frames[b][~cov] == 255).all()) and bool((frames[b][cov] != 255).any(-1).float().mean() > 0.9)
    assert not torch.equal(frames[0], frames[1])
