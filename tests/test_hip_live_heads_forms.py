"""nm_mlp_forward_live / _listed_live / _samples_live / _ray_chunk_live -- the trunk launch + colour-head launch pair of nm_mlp_forward_rays_live
(csrc/mlp_i8s.hip TRUNK, csrc/mlp_i8h.hip) for the other four input forms -- each against its whole-network sibling on the same inputs and the same
prefilled `out`: every density equal, the colours of records with stored density > 0 equal, every other listed record's colour exactly 0, every
unlisted record untouched, everything finite, and the composite of the two equal.  Shapes sit at the edges of the 256-sample tile, the 32-sample
wave and the piece (`chunk_samples`)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_live_heads import _net  # noqa: E402  (the four nets: bench_fine | fog | empty | plain)

from neuman_hip import _lib, occupancy, render_utils, vanilla  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ['bench_fine', 'fog', 'empty', 'plain']
I8 = _lib.NM_PREC_I8X3
FILL = 7.0
_NETS = {}


def net_of(kind):
    if kind not in _NETS:
        _NETS[kind] = _net(kind)
    return _NETS[kind]


def _rays(R, S, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    o = torch.randn((R, 3), device='cuda', generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn((R, 3), device='cuda', generator=g), dim=-1)
    z = torch.sort(torch.rand((R, S), device='cuda', generator=g) * 3.0, dim=1).values.contiguous()
    return o, d, z


def _points(n, seed):
    """n points spread like the samples of _rays, each with a direction of its own"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    o = torch.randn((n, 3), device='cuda', generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn((n, 3), device='cuda', generator=g), dim=-1)
    pts = (o + d * (torch.rand((n, 1), device='cuda', generator=g) * 3.0)).contiguous()
    dirs = torch.nn.functional.normalize(torch.randn((n, 3), device='cuda', generator=g), dim=-1).contiguous()
    return pts, dirs


def _ws(n_max, chunk):
    nbytes = _lib.lib().nm_mlp_live_workspace_bytes(n_max, chunk)
    assert nbytes > 0
    return torch.empty(nbytes, device='cuda', dtype=torch.uint8), nbytes


def _p(t, dtype=torch.float32):
    return _lib.dev_ptr(t, dtype)


def _pair(kind, whole, live, shape, listed, z, d, scale_name):
    """whole(out) / live(out) run the two entries on an `out` prefilled with FILL; listed: bool mask over the records, the ones the call writes;
    z [R,S], d [R,3]: what the records are composited with"""
    ref = torch.full(shape + (4,), FILL, device='cuda')
    got = torch.full(shape + (4,), FILL, device='cuda')
    _lib.check(whole(ref), "whole-network sibling")
    _lib.check(live(got), "live entry")
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and torch.isfinite(got).all()
    alive = listed & (ref[..., 3] > 0)
    dead = listed & ~alive
    n = int(listed.sum())
    frac = int(alive.sum()) / max(n, 1)
    print(f"[live forms] {scale_name} {kind}: {n} listed of {listed.numel()}, live fraction {frac:.3f}")
    assert torch.equal(ref[~listed], torch.full_like(ref[~listed], FILL))          # (the sibling itself leaves the unlisted alone)
    if kind == 'plain':
        assert torch.equal(got, ref)
        return
    if n >= 256:                                                                   # (at least a tile's worth: fewer listed samples are a shape edge, not a mix of classes)
        if kind == 'bench_fine':
            assert 0.1 <= frac <= 0.9
        if kind == 'fog':
            assert frac == 1.0
        if kind == 'empty':
            assert frac == 0.0
    assert torch.equal(got[..., 3], ref[..., 3])
    assert torch.equal(got[..., :3][alive], ref[..., :3][alive])
    assert (got[..., :3][dead] == 0).all()
    assert (got[~listed] == FILL).all()
    a = render_utils.raw2outputs(ref.reshape(z.shape + (4,)), z, d)
    b = render_utils.raw2outputs(got.reshape(z.shape + (4,)), z, d)
    for i, name in ((0, 'rgb'), (4, 'depth'), (2, 'acc')):
        assert torch.equal(a[i], b[i]), name


# ---- points (in_mode 0): n = 5 (less than a wave), 703 (two tiles and a ragged third; chunk 300: three pieces, the last of 103), 8193 (33 tiles)
POINT_CASES = [(5, 0, 1.0), (703, 0, 1.0), (703, 300, 1.0), (8193, 0, 1.0), (703, 300, 0.7)]


@pytest.mark.parametrize("n,chunk,scale", POINT_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_points(kind, n, chunk, scale):
    net, L = net_of(kind), _lib.lib()
    pts, dirs = _points(n, seed=5)
    assert not torch.equal(dirs[0], dirs[1])                                       # a head that took one direction per row would fail
    ws, nbytes = _ws(n, chunk)
    z = torch.linspace(0.0, 3.0, n, device='cuda').reshape(1, n).contiguous()      # composited as ONE ray of n samples
    d1 = dirs[:1].contiguous()
    h = net.handle()
    _pair(kind,
          lambda out: L.nm_mlp_forward(h, _p(pts), _p(dirs), n, I8, scale, _p(out), _lib.stream_ptr()),
          lambda out: L.nm_mlp_forward_live(h, _p(pts), _p(dirs), n, I8, scale, _p(out), _p(ws, torch.uint8), nbytes, chunk, _lib.stream_ptr()),
          (n,), torch.ones(n, dtype=torch.bool, device='cuda'), z, d1, f"points n={n} chunk={chunk} scale={scale}")


# ---- listed points (in_mode 4): n_points = 1000, chunk_samples = 256; every third index (host-counted), and lengths 0, 1, 255, 257 read from the
# device under n_max = 1000 (four pieces: the lengths fall before, on and past the first piece's end)
LISTED_CASES = [('third', None, 1.0), ('dev', 0, 1.0), ('dev', 1, 1.0), ('dev', 255, 1.0), ('dev', 257, 1.0), ('dev', 257, 0.7)]


@pytest.mark.parametrize("how,length,scale", LISTED_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_listed_points(kind, how, length, scale):
    net, L = net_of(kind), _lib.lib()
    n_points, chunk = 1000, 256
    pts, dirs = _points(n_points, seed=6)
    if how == 'third':
        idx = torch.arange(0, n_points, 3, device='cuda', dtype=torch.int32)
        n_dev, n_max, n_list = None, idx.numel(), idx.numel()
    else:
        g = torch.Generator(device='cuda').manual_seed(7)
        idx = torch.randperm(n_points, device='cuda', generator=g).to(torch.int32).contiguous()   # entries past the count must not be read as listed
        n_dev, n_max, n_list = torch.tensor([length, 0], device='cuda', dtype=torch.int32), n_points, length
    listed = torch.zeros(n_points, dtype=torch.bool, device='cuda')
    listed[idx[:n_list].long()] = True
    ws, nbytes = _ws(n_max, chunk)
    z = torch.linspace(0.0, 3.0, n_points, device='cuda').reshape(1, n_points).contiguous()
    h = net.handle()
    nd = _p(n_dev, torch.int32) if n_dev is not None else None
    _pair(kind,
          lambda out: L.nm_mlp_forward_listed(h, _p(pts), _p(dirs), n_points, _p(idx, torch.int32), nd, n_max, I8, scale, _p(out), _lib.stream_ptr()),
          lambda out: L.nm_mlp_forward_listed_live(h, _p(pts), _p(dirs), n_points, _p(idx, torch.int32), nd, n_max, I8, scale, _p(out), _p(ws, torch.uint8),
                                                   nbytes, chunk, _lib.stream_ptr()),
          (n_points,), listed, z, dirs[:1].contiguous(), f"listed {how} {length} scale={scale}")


# ---- listed samples (in_mode 3): R x S = 37 x 19, the list of nm_occ_compact_samples on a random grid (p = 0.5), and the empty list; chunk 256
@pytest.mark.parametrize("how,scale", [('grid', 1.0), ('none', 1.0), ('grid', 0.7)])
@pytest.mark.parametrize("kind", KINDS)
def test_listed_samples(kind, how, scale):
    net, L = net_of(kind), _lib.lib()
    R, S, chunk = 37, 19, 256
    o, d, z = _rays(R, S, seed=8)
    g = torch.Generator().manual_seed(9)
    grid = occupancy.OccupancyGrid.from_mask(occupancy.rays_aabb(o, d, 0.0, 3.0), torch.rand((8, 8, 8), generator=g) < 0.5, device='cuda')
    idx, counts = grid.compact(o, d, z)
    if how == 'none':
        counts = torch.zeros(2, device='cuda', dtype=torch.int32)
    n_list = int(counts[0].item())
    assert how == 'none' or 0.2 * R * S < n_list < 0.8 * R * S
    listed = torch.zeros(R * S, dtype=torch.bool, device='cuda')
    listed[idx[:n_list].long()] = True
    ws, nbytes = _ws(R * S, chunk)
    h = net.handle()
    _pair(kind,
          lambda out: L.nm_mlp_forward_samples(h, _p(o), _p(d), _p(z), R, S, _p(idx, torch.int32), _p(counts, torch.int32), R * S, I8, scale, _p(out),
                                               _lib.stream_ptr()),
          lambda out: L.nm_mlp_forward_samples_live(h, _p(o), _p(d), _p(z), R, S, _p(idx, torch.int32), _p(counts, torch.int32), R * S, I8, scale, _p(out),
                                                    _p(ws, torch.uint8), nbytes, chunk, _lib.stream_ptr()),
          (R, S), listed.reshape(R, S), z, d, f"samples {how} scale={scale}")


# ---- a chunk of listed rays (in_mode 2): R = 41, S_total = 48; chunks at the start, inside and at the end of the ray; 17 listed rays of which the
# device counts 0, 1 or 17; chunk_samples = 64: pieces of 4 rays (S = 16: five pieces, the last of one ray) or 8 rays (S = 8)
CHUNK_CASES = [(s0, S, cnt, 1.0) for (s0, S) in ((0, 16), (16, 16), (40, 8)) for cnt in (0, 1, 17)] + [(16, 16, 17, 0.7)]


@pytest.mark.parametrize("s0,S,count,scale", CHUNK_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_ray_chunk(kind, s0, S, count, scale):
    net, L = net_of(kind), _lib.lib()
    R, S_total, chunk = 41, 48, 64
    o, d, z = _rays(R, S_total, seed=10)
    g = torch.Generator(device='cuda').manual_seed(11)
    rays = torch.randperm(R, device='cuda', generator=g)[:17].to(torch.int32).contiguous()
    n_dev = torch.tensor([count], device='cuda', dtype=torch.int32)
    listed = torch.zeros((R, S_total), dtype=torch.bool, device='cuda')
    listed[rays[:count].long(), s0:s0 + S] = True
    ws, nbytes = _ws(17 * S, chunk)
    h = net.handle()
    _pair(kind,
          lambda out: L.nm_mlp_forward_ray_chunk(h, _p(o), _p(d), _p(z), S_total, _p(rays, torch.int32), _p(n_dev, torch.int32), 17, s0, S, I8, scale, _p(out),
                                                 _lib.stream_ptr()),
          lambda out: L.nm_mlp_forward_ray_chunk_live(h, _p(o), _p(d), _p(z), S_total, _p(rays, torch.int32), _p(n_dev, torch.int32), 17, s0, S, I8, scale,
                                                      _p(out), _p(ws, torch.uint8), nbytes, chunk, _lib.stream_ptr()),
          (R, S_total), listed, z, d, f"ray chunk s0={s0} S={S} count={count} scale={scale}")


# ---- the host mirror: role='composite' takes the same routes
def test_joiner_forward_composite_role(monkeypatch):
    monkeypatch.setattr(vanilla, 'LIVE_MIN_SAMPLES', 0)                              # (the mirror keeps small passes whole by default)
    net = net_of('bench_fine')
    pts, dirs = _points(703, seed=5)
    with torch.no_grad():
        ref = net(pts, dirs, role='shading')
        got = net(pts, dirs, role='composite', chunk_samples=300)
    alive = ref[..., 3] > 0
    assert 0.1 <= alive.float().mean().item() <= 0.9
    assert torch.equal(got[..., 3], ref[..., 3]) and torch.equal(got[..., :3][alive], ref[..., :3][alive])
    assert (got[..., :3][~alive] == 0).all()


def test_occupancy_forward_composite_role(monkeypatch):
    monkeypatch.setattr(vanilla, 'LIVE_MIN_SAMPLES', 0)
    net = net_of('bench_fine')
    R, S = 37, 19
    o, d, z = _rays(R, S, seed=8)
    g = torch.Generator().manual_seed(9)
    grid = occupancy.OccupancyGrid.from_mask(occupancy.rays_aabb(o, d, 0.0, 3.0), torch.rand((8, 8, 8), generator=g) < 0.5, device='cuda')
    occupancy.attach(net, grid)
    try:
        with torch.no_grad():
            ref = occupancy.forward_rays(net, o, d, z, role='shading')
            got = occupancy.forward_rays(net, o, d, z, role='composite', chunk_samples=256)
            pts = (o[:, None] + d[:, None] * z[..., None]).reshape(-1, 3)
            dirs = _points(R * S, seed=12)[1]
            refp = occupancy.forward_points(net, pts, dirs, role='shading')
            gotp = occupancy.forward_points(net, pts, dirs, role='composite', chunk_samples=256)
    finally:
        occupancy.detach(net)
    for r, q in ((ref, got), (refp, gotp)):
        alive = r[..., 3] > 0
        assert 0 < int(alive.sum()) < alive.numel()
        assert torch.equal(q[..., 3], r[..., 3]) and torch.equal(q[..., :3][alive], r[..., :3][alive])
        assert (q[..., :3][~alive] == 0).all() and (r[..., :3][(r[..., 3] < 0)] != 0).any()


def test_small_passes_stay_whole_by_default():
    """below vanilla.LIVE_MIN_SAMPLES role='composite' is the whole-network launch: colours on dead samples too"""
    net = net_of('bench_fine')
    pts, dirs = _points(703, seed=5)
    assert 703 < vanilla.LIVE_MIN_SAMPLES
    with torch.no_grad():
        assert torch.equal(net(pts, dirs, role='composite'), net(pts, dirs, role='shading'))
