"""-m gpu: early ray termination together with an occupancy grid in the background passes (render_utils.MARCH_WITH_GRID,
march_pass_rays grid=, OccupancyGrid.compact_ray_chunk: nm_occ_compact_ray_chunk, occupancy.forward_listed_samples).

The contract: a marched pass with a grid is, bit for bit, the marched pass without one whose network records were zeroed wherever the
grid's whole-pass list (OccupancyGrid.compact, the existing kernel) skips the sample -- the same raw, so the same cuts, the same adaptive
chunk lengths and the same frame.  Grid (a) is wrong on some rays and grid (b) is random: neither matters to that statement."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import posed_scene as PS  # noqa: E402

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.0, 3.14


def cu(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to('cuda', torch.float32).contiguous()


def random_grid(occ, box, res=16, p=0.5, seed=11):
    g = torch.Generator().manual_seed(seed)
    return occ.OccupancyGrid.from_mask(box, torch.rand(res, res, res, generator=g) < p, device='cuda')


def skipped_mask(grid, o, d, z):
    """[R, S] bool: the samples the grid's whole-pass list (nm_occ_compact_samples) leaves out"""
    idx, counts = grid.compact(o.contiguous(), d.contiguous(), z.contiguous())
    keep = torch.zeros(z.numel(), dtype=torch.bool, device=z.device)
    keep[idx[:int(counts[0])].long()] = True
    return ~keep.reshape(z.shape)


@pytest.fixture(scope="module")
def scene():
    """the 4096-ray slice of tests/test_hip_march.py's scene, its sample positions and the three grids"""
    from neuman_hip import occupancy, ray_utils, render_utils, synthetic
    net = synthetic.make_joiner(1, preset='opaque').cuda()
    cap = synthetic.SimpleCapture(800, 800)
    o, d = ray_utils.shot_all_rays_dev(cap, torch.device('cuda'))
    sel = torch.arange(390 * 800, 390 * 800 + 4096, device='cuda')
    o, d = o[sel].contiguous(), d[sel].contiguous()
    R = o.shape[0]
    near, far = torch.zeros(R, device='cuda'), torch.full((R,), FAR, device='cuda')

    def coarse_z(S):
        return ray_utils.sample_z(o, d, near, far, S)[2].contiguous()
    zc = coarse_z(128)
    w = render_utils.raw2outputs(net.forward_rays(o, d, zc, sigma_only=True), zc, d)[3]
    zf = ray_utils.importance_z(zc, w, 128).contiguous()
    box = occupancy.rays_aabb(o, d, NEAR, FAR)
    mid, half = (box[:3] + box[3:]) / 2, (box[3:] - box[:3]) / 2
    grids = {'a': occupancy.OccupancyGrid.from_net(net, box, res=32, dilate=0),
             'b': random_grid(occupancy, torch.cat([mid - 0.6 * half, mid + 0.6 * half])),       # smaller than the rays' extent: samples outside occur
             'c': occupancy.OccupancyGrid.from_mask(box, torch.ones(16, 16, 16, dtype=torch.bool), device='cuda')}
    return dict(net=net, o=o, d=d, zc=zc, zf=zf, coarse_z=coarse_z, grids=grids, box=box, occ=occupancy, render=render_utils, ray=ray_utils, syn=synthetic)


class Zeroing:
    """net.forward_ray_chunk wrapped: the real launch, then the records the grid's whole-pass list skips are zeroed.  `zeroed` counts the
    records of live rays' chunks that were (what the grid saves); the skip mask is taken per sample array (coarse and final positions)."""

    def __init__(self, net, grid):
        self.net, self.grid, self.zeroed, self._masks = net, grid, 0, []

    def mask(self, o, d, z):
        for z_, m in self._masks:
            if z_ is z:
                return m
        m = skipped_mask(self.grid, o, d, z)
        self._masks.append((z, m))
        return m

    def __enter__(self):
        real = self.net.forward_ray_chunk

        def wrapped(origin, direction, z_vals, ray_idx, n_rays_dev, s0, chunk, out, **kw):
            real(origin, direction, z_vals, ray_idx, n_rays_dev, s0, chunk, out, **kw)
            skip = self.mask(origin, direction, z_vals)
            rays = ray_idx[:int(n_rays_dev[0])].long()
            self.zeroed += int(skip[rays, s0:s0 + chunk].sum())
            out.masked_fill_(skip.unsqueeze(-1), 0.0)
            return out
        self.net.forward_ray_chunk = wrapped
        return self

    def __exit__(self, *exc):
        del self.net.forward_ray_chunk                          # (the instance attribute: the class's method is back)
        return False


# ---- 1. the chunk's list against the existing whole-pass list -----------------------------------------------------------------------
def check_list(grid, o, d, z, keep, ray_idx, n, s0, c, with_count=True, filler=None):
    """compact_ray_chunk on the first n entries of ray_idx against {r*S+s : r in ray_idx[:n], s0 <= s < s0+c} & (the whole-pass list), in
    candidate order; the entries past n hold `filler`: valid rays that are not live, so a kernel reading past the count fails the comparison"""
    R, S = z.shape
    if ray_idx is None:
        listed, arg, n_rays = torch.arange(n, device='cuda'), None, (n if not with_count else R)
    else:
        listed = ray_idx[:n].long()
        arg = torch.cat([ray_idx[:n], filler]).to(torch.int32).contiguous()
        n_rays = arg.shape[0]
    n_dev = torch.tensor([n, 12345], device='cuda', dtype=torch.int32) if with_count else None
    idx, counts = grid.compact_ray_chunk(o, d, z, arg, n_dev, s0, c, n_rays=n_rays)
    cand = (listed[:, None] * S + torch.arange(s0, s0 + c, device='cuda')[None]).reshape(-1)
    want = cand[keep.reshape(-1)[cand]].to(torch.int32)
    kept, dropped = (int(x) for x in counts.tolist())
    assert idx.dtype == torch.int32 and idx.shape[0] == n_rays * c
    assert (kept, dropped) == (want.numel(), n * c - want.numel()), (n, s0, c, kept, dropped, want.numel())
    assert torch.equal(idx[:kept], want), (n, s0, c)
    return kept, dropped


@pytest.mark.parametrize("which", ["a", "b"])
def test_chunk_list_equals_the_whole_pass_list(scene, which):
    grid = scene['grids'][which]
    R, S = 300, 40
    o, d = scene['o'][:R].contiguous(), scene['d'][:R].contiguous()
    z = scene['coarse_z'](S)[:R].contiguous()
    keep = ~skipped_mask(grid, o, d, z)
    assert 0 < int(keep.sum()) < keep.numel()
    g = torch.Generator(device='cuda').manual_seed(3)
    perm = torch.randperm(R, device='cuda', generator=g)
    tot_kept = tot_dropped = 0
    sizes = [(c, n) for c in (1, 7, 16, 40) for n in (0, 1, 257, R)]
    sizes += [(1, 255), (1, 256), (1, 257), (16, 16), (3, 85), (11, 93), (16, 64), (5, 205)]        # n*c = 255, 256, 257 | 256, 255 | 1023, 1024, 1025
    for c, n in sizes:
        live = perm[:n].sort().values                                                               # ascending, as nm_compact_hits' lists are
        filler = perm[n:][:min(R - n, 64)]                                                          # rays that are not live, valid indices
        for s0 in sorted({0, (S - c) // 2, S - c}):
            k, s = check_list(grid, o, d, z, keep, live, n, s0, c, filler=filler)
            tot_kept, tot_dropped = tot_kept + k, tot_dropped + s
    assert tot_kept > 0 and tot_dropped > 0
    # an unsorted list: candidate order, not index order
    check_list(grid, o, d, z, keep, perm[:100], 100, 5, 16, filler=perm[100:140])
    # no ray_idx: rays 0 .. n-1, with the count on the device (under a larger bound) and without it
    for c, s0 in ((7, 3), (40, 0)):
        check_list(grid, o, d, z, keep, None, 257, s0, c, with_count=True)
        check_list(grid, o, d, z, keep, None, 0, s0, c, with_count=True)
        check_list(grid, o, d, z, keep, None, R, s0, c, with_count=False)
        check_list(grid, o, d, z, keep, None, 123, s0, c, with_count=False)


@pytest.mark.parametrize("n_live,c", [(2100, 128), (4096, 257)])
def test_chunk_list_over_many_blocks(scene, n_live, c):
    """2100 live rays x 128 = 268 800 candidates; and 4096 x 257 = 1 052 672, past occ_scan_kernel's first sweep of 1024 blocks of 1024"""
    grid = scene['grids']['a']
    o, d = scene['o'], scene['d']
    R, S = o.shape[0], c + 3
    z = scene['coarse_z'](S)
    keep = ~skipped_mask(grid, o, d, z)
    perm = torch.randperm(R, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4))
    live = perm[:n_live].sort().values
    filler = perm[n_live:] if n_live < R else perm[:0]
    kept, dropped = check_list(grid, o, d, z, keep, live, n_live, 2, c, filler=filler)
    assert kept > 0 and dropped > 0


# ---- 2. the march's contract, on every ray, bit for bit -----------------------------------------------------------------------------
def both_marches(scene, grid, z, eps, chunk, adaptive, **kw):
    net, o, d, R = scene['net'], scene['o'], scene['d'], scene['render']
    st_l, st_r = {}, {}
    left = R.march_pass_rays(net, o, d, z, eps, chunk=chunk, adaptive=adaptive, stats=st_l, grid=grid, **kw)
    with Zeroing(net, grid) as wrap:
        right = R.march_pass_rays(net, o, d, z, eps, chunk=chunk, adaptive=adaptive, stats=st_r, **kw)
    assert 'grid_skipped' not in st_r
    print(f"[march+grid] eps {eps:g} chunk {chunk} adaptive {adaptive}: evaluated {st_l['evaluated'] / st_l['total']:.3f} with the grid, "
          f"{st_r['evaluated'] / st_r['total']:.3f} without; dropped by the grid {st_l['grid_skipped'] / st_l['total']:.3f}; launches {st_l['launches']}")
    assert torch.equal(left, right)
    assert st_l['launches'] == st_r['launches'] and st_l['total'] == st_r['total'] == z.numel()
    assert st_l['evaluated'] == st_r['evaluated'] - wrap.zeroed
    assert st_l['evaluated'] + st_l['grid_skipped'] == st_r['evaluated']
    return left, st_l


SCHEDULES = [(16, False), (48, False), (None, None)]             # fixed chunks of 16 and 48; the adaptive schedule (on when eps > 0)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("chunk,adaptive", SCHEDULES)
@pytest.mark.parametrize("eps", [0.0, 1e-4, 1e-3])
def test_marched_shading_pass_equals_the_zeroed_march(scene, which, chunk, adaptive, eps):
    _, st = both_marches(scene, scene['grids'][which], scene['zf'], eps, chunk, adaptive)
    assert st['grid_skipped'] > 0
    if eps > 0:
        assert st['evaluated'] + st['grid_skipped'] < st['total']                        # both effects: rays were cut, samples were dropped


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("chunk,adaptive", SCHEDULES)
def test_marched_density_pass_equals_the_zeroed_march(scene, which, chunk, adaptive):
    _, st = both_marches(scene, scene['grids'][which], scene['zc'], scene['render'].TERMINATION_COARSE, chunk, adaptive, role=None, sigma_only=True)
    assert st['grid_skipped'] > 0


def test_marched_pass_with_an_occluder_and_merged_intervals(scene):
    R = scene['o'].shape[0]
    g = torch.Generator(device='cuda').manual_seed(9)
    z2 = (1.0 + torch.rand(R, 64, device='cuda', generator=g)).sort(1).values.contiguous()
    dz = scene['render'].merged_intervals([scene['zf'], z2])[0].contiguous()
    occluder = (z2[:, -1].contiguous(), torch.rand(R, device='cuda', generator=g) * 0.5)
    _, st = both_marches(scene, scene['grids']['a'], scene['zf'], 1e-4, None, None, occluder=occluder, dz=dz)
    assert st['grid_skipped'] > 0 and st['evaluated'] + st['grid_skipped'] < st['total']


# ---- 3. eps = 0 with a grid = the gridded whole pass --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("sigma_only", [False, True])
@pytest.mark.parametrize("chunk", [32, 100])
def test_march_without_termination_equals_the_gridded_pass(scene, which, sigma_only, chunk):
    net, o, d, grid = scene['net'], scene['o'], scene['d'], scene['grids'][which]
    z = scene['zc'] if sigma_only else scene['zf']
    role = None if sigma_only else 'shading'
    scene['occ'].attach(net, grid)
    try:
        st_w = {}
        whole = scene['occ'].forward_rays(net, o, d, z, role=role, sigma_only=sigma_only, stats=st_w)
    finally:
        scene['occ'].detach(net)
    st = {}
    marched = scene['render'].march_pass_rays(net, o, d, z, 0.0, chunk=chunk, role=role, sigma_only=sigma_only, stats=st, grid=grid)
    assert torch.equal(marched, whole)
    assert st['evaluated'] == st_w['evaluated'] and st['evaluated'] + st['grid_skipped'] == st['total'] == z.numel()


def test_march_without_termination_on_the_live_route(scene):
    """4096 x 256 samples in chunks of 128: a chunk holds 2^19 samples, LIVE_MIN_SAMPLES -- trunk and colour head on the listed samples that
    have density (nm_mlp_forward_samples_live), as the gridded whole pass"""
    from neuman_hip import vanilla
    net, o, d, z, grid = scene['net'], scene['o'], scene['d'], scene['zf'], scene['grids']['a']
    assert o.shape[0] * 128 == vanilla.LIVE_MIN_SAMPLES and net.live_route('i8x3', 'composite', o.shape[0] * 128)
    scene['occ'].attach(net, grid)
    try:
        whole = scene['occ'].forward_rays(net, o, d, z, precision='i8x3', role='composite')
    finally:
        scene['occ'].detach(net)
    marched = scene['render'].march_pass_rays(net, o, d, z, 0.0, chunk=128, precision='i8x3', role='composite', grid=grid)
    assert torch.equal(marched, whole)
    plain = scene['render'].march_pass_rays(net, o, d, z, 0.0, chunk=128, precision='i8x3', role='shading', grid=grid)
    dead = marched[..., 3] <= 0
    assert bool(dead.any()) and bool((marched[..., :3][dead] == 0).all()) and torch.equal(marched[~dead], plain[~dead])


# ---- 4. a grid with every cell occupied ---------------------------------------------------------------------------------------------
def test_full_grid_changes_nothing(scene):
    net, o, d, z = scene['net'], scene['o'], scene['d'], scene['zf']
    st0, st1 = {}, {}
    plain = scene['render'].march_pass_rays(net, o, d, z, 1e-4, stats=st0)
    gridded = scene['render'].march_pass_rays(net, o, d, z, 1e-4, stats=st1, grid=scene['grids']['c'])
    assert torch.equal(plain, gridded)
    assert st1['evaluated'] == st0['evaluated'] and st1['grid_skipped'] == 0 and st1['launches'] == st0['launches']


# ---- 5. the renderers, switch on ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body():
    from neuman_hip import ray_utils, render_utils, synthetic
    g = PS.load()
    g['R'], g['ray'] = render_utils, ray_utils
    g['mesh'] = ray_utils.mesh_to_device(g['posed_verts'], np.ascontiguousarray(g['faces'][:, :3], np.int32), g['T'], 'cuda')
    g['meshes'] = [ray_utils.mesh_to_device(v, np.ascontiguousarray(g['faces'][:, :3], np.int32), t, 'cuda') for v, t in zip(g['posed_l'], g['T_l'])]
    g['bkg'] = synthetic.make_joiner(1, preset='opaque').cuda()
    g['human'] = synthetic.make_joiner(2, 'rotate', preset='opaque').cuda()
    return g


@contextlib.contextmanager
def settings(R, eps, switch):
    old = R.TERMINATION_EPS, R.MARCH_WITH_GRID
    R.TERMINATION_EPS, R.MARCH_WITH_GRID = eps, switch
    try:
        yield
    finally:
        R.TERMINATION_EPS, R.MARCH_WITH_GRID = old


def renderer_case(R, occ, net, grid, run, bound):
    """run(trace) -> tuple of frame tensors, the net `net` serving the background passes"""
    parent = run(None)
    occ.attach(net, grid)
    try:
        with settings(R, 1e-4, False), pytest.raises(NotImplementedError):              # the switch is what admits the combination
            run(None)
        with settings(R, 1e-4, True):
            tr = {}
            both = run(tr)
            untraced = run(None)
        with settings(R, 0.0, True):
            tr_g = {}
            grid_only = run(tr_g)
    finally:
        occ.detach(net)
    with settings(R, 1e-4, True), Zeroing(net, grid):
        tr_z = {}
        zeroed = run(tr_z)
    for a_, b_ in zip(both, zeroed):
        assert torch.equal(a_, b_)
    for a_, b_ in zip(both, untraced):
        assert torch.equal(a_, b_)
    assert torch.equal(torch.cat(tr['bkg_z']), torch.cat(tr_z['bkg_z']))
    assert torch.equal(torch.cat(tr['bkg_z']), torch.cat(tr_g['bkg_z']))
    e = (both[0] - grid_only[0]).abs().max().item()
    m, mc = tr['march'][0], tr['march_coarse'][0]
    print(f"[march+grid] colour Linf vs the grid-only frame {e:.2e} (bound {bound:g}); shading pass evaluated {m['evaluated'] / m['total']:.3f}, dropped by "
          f"the grid {m['grid_skipped'] / m['total']:.3f}; coarse pass evaluated {mc['evaluated'] / mc['total']:.3f}, dropped {mc['grid_skipped'] / mc['total']:.3f}")
    assert e <= bound
    assert m['evaluated'] < m['total'] and m['grid_skipped'] > 0
    assert mc['evaluated'] < mc['total'] and mc['grid_skipped'] > 0
    assert 'occupancy' not in tr and 'occupancy_coarse' not in tr
    after = run(None)
    for a_, b_ in zip(parent, after):
        assert torch.equal(a_, b_)


def test_vanilla_renderer_with_both(scene):
    R, net = scene['render'], scene['net']
    o, d = scene['o'][:2048].contiguous(), scene['d'][:2048].contiguous()
    renderer_case(R, scene['occ'], net, scene['grids']['a'], lambda trace: R.render_vanilla_rays(net, net, o, d, NEAR, FAR, 128, 128, trace=trace), 1e-4)


@pytest.mark.parametrize("which", ["hybrid", "multi"])
def test_posed_renderers_with_both(body, which):
    from neuman_hip import occupancy
    R, bkg, human = body['R'], body['bkg'], body['human']
    c = PS.cap(body, which)
    o, d = (cu(x) for x in PS.frame_rays(c))
    grid = occupancy.OccupancyGrid.from_net(bkg, occupancy.rays_aabb(o, d, c.near['bkg'], c.far['bkg']), res=32, dilate=0)

    def run(trace):
        if which == 'hybrid':
            return R.render_hybrid_rays(bkg, bkg, human, o, d, c.near['bkg'], c.far['bkg'], cu(body['posed_verts']), body['mesh'], 128, 128, trace=trace)
        return R.render_multi_rays(bkg, bkg, [human] * 3, o, d, c.near['bkg'], c.far['bkg'], [cu(v) for v in body['posed_l']], body['meshes'], 192, 128,
                                   trace=trace)
    renderer_case(R, occupancy, bkg, grid, run, {'hybrid': 2e-4, 'multi': 4e-4}[which])


def test_fused_background_call_gives_way(scene):
    """bkg_pass_rays_fused with a grid, termination and the switch: the unfused passes, marched with the grid"""
    R, net, occ = scene['render'], scene['net'], scene['occ']
    o, d = scene['o'][:512].contiguous(), scene['d'][:512].contiguous()
    near, far = torch.zeros(512, device='cuda'), torch.full((512,), FAR, device='cuda')
    occ.attach(net, scene['grids']['a'])
    try:
        with settings(R, 1e-4, True):
            raw_f, z_f = R.bkg_pass_rays_fused(net, net, o, d, near, far, 64, 64, True)
            raw_u, z_u = R.bkg_pass_rays(net, net, o, d, near, far, 64, 64, True)
    finally:
        occ.detach(net)
    assert torch.equal(z_f, z_u) and torch.equal(raw_f, raw_u)
    skip = skipped_mask(scene['grids']['a'], o, d, z_f)
    assert bool(skip.any()) and bool((raw_f[skip] == 0).all())
