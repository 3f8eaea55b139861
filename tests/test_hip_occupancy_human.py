"""-m gpu: occupancy-grid empty-space skipping for the human passes (nm_render_rays_human_occ, nm_occ_compact_points,
in_mode 4 of csrc/mlp_device.h; neuman_hip/occupancy.py, render_utils.human_pass_rays / human_march_rays).

The contract that holds on every ray: the frame with a grid is the every-sample pass's raw with the skipped samples zeroed, then composited
-- bit for bit.  The expected frames below run the same renderer with a stand-in for human_pass_rays that evaluates every sample (no grid)
and zeroes the samples the grid skips."""
import types

import pytest
import torch

from test_hip_human_trainer import setup  # noqa: F401  (the trainer's fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from neuman_hip import _lib, occupancy, ray_utils, render_utils, synthetic
    dev = torch.device('cuda')
    verts_c, faces = synthetic.capsule_mesh(20, 24)
    posed, T = synthetic.twist_transforms(verts_c)
    cap = synthetic.SimpleCapture(64, 64, fx=1.6 * 64, c2w=synthetic.spherical_c2w(40., 0., 3.0))
    o, d = render_utils._pixel_rays(cap, dev)
    return types.SimpleNamespace(lib=_lib, occ=occupancy, ray=ray_utils, render=render_utils, syn=synthetic, dev=dev, o=o, d=d, faces=faces,
                                 can=torch.from_numpy(verts_c).to(dev), posed=torch.from_numpy(posed).to(dev),
                                 mesh=ray_utils.mesh_to_device(posed, faces, T, dev), box=occupancy.canonical_aabb(verts_c, 0.1))


def human(M, seed=2, mapping='rotate'):
    return M.syn.make_joiner(seed, mapping, preset='opaque').to(M.dev)


def mask_grid(M, seed, p=0.5, res=16, box=None):
    g = torch.Generator().manual_seed(seed)
    return M.occ.OccupancyGrid.from_mask(M.box if box is None else box, torch.rand(res, res, res, generator=g) < p, device=M.dev)


def keep_mask(grid, n, idx, counts):
    keep = torch.zeros(n, dtype=torch.bool, device=idx.device)
    keep[idx[:int(counts[0])].long()] = True
    return keep


def masked_pass(M, grids):
    """human_pass_rays evaluating every sample (the nets carry no grid), then zeroing what `grids[id(net)]` skips"""
    orig = M.render.human_pass_rays

    def fn(human_net, o, d, near, far, samples_per_ray, mesh=None, render_can=False, sigma_scale=1.0, precision=None, trace=None):
        assert M.occ.grid_of(human_net) is None
        tr = {}
        raw, z = orig(human_net, o, d, near, far, samples_per_ray, mesh, render_can, sigma_scale, precision, tr)
        g = grids[id(human_net)]
        if render_can:
            keep = keep_mask(g, z.numel(), *g.compact(o.contiguous(), d.contiguous(), z))
        else:
            keep = keep_mask(g, z.numel(), *g.compact_points(tr['can_pts'][0]))
        return torch.where(keep.reshape(z.shape)[..., None], raw, torch.zeros_like(raw)), z
    return fn


def both(M, monkeypatch, nets_grids, render, expected_trace=True):
    """(frame with the grids attached, frame of the every-sample pass with the skipped samples zeroed)"""
    for n_, g in nets_grids:
        M.occ.detach(n_)
    with monkeypatch.context() as mp:
        mp.setattr(M.render, 'human_pass_rays', masked_pass(M, {id(n_): g for n_, g in nets_grids}))
        want = render({} if expected_trace else None)
    for n_, g in nets_grids:
        M.occ.attach(n_, g)
    try:
        got = render(None)
    finally:
        for n_, _ in nets_grids:
            M.occ.detach(n_)
    return got, want


def assert_same(got, want):
    for a, b in zip(got, want):
        assert torch.equal(a, b), float((a - b).abs().max())


# ---- 1. the listed launch and the point compaction --------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ['fp16x3', 'bf16x3', 'bf16', 'i8x3'])
@pytest.mark.parametrize("plain", [False, True])
def test_listed_launch_equals_forward_row_for_row(M, precision, plain):
    net = M.syn.make_variant_joiner(3, use_viewdirs=False).to(M.dev) if plain else human(M)
    n = 5000
    g = torch.Generator(device=M.dev).manual_seed(1)
    pts = (torch.rand((n, 3), device=M.dev, generator=g) - 0.5) * 1.5
    dirs = torch.nn.functional.normalize(torch.randn((n, 3), device=M.dev, generator=g), dim=-1)
    idx = torch.nonzero(torch.rand(n, device=M.dev, generator=g) < 0.4).reshape(-1).to(torch.int32)
    cnt = torch.tensor([idx.numel(), 0], device=M.dev, dtype=torch.int32)
    L = M.lib.lib()
    prec = M.lib.PRECISIONS[precision]
    with torch.no_grad():
        full = net(pts, dirs, precision=precision)
        out = torch.zeros((n, 4), device=M.dev)
        M.lib.check(L.nm_mlp_forward_listed(net.handle(), M.lib.dev_ptr(pts), M.lib.dev_ptr(dirs), n, M.lib.dev_ptr(idx, torch.int32),
                                            M.lib.dev_ptr(cnt, torch.int32), n, prec, 1.0, M.lib.dev_ptr(out), M.lib.stream_ptr()), "listed")
        # the count on the device bounds the launch: a list longer than *n_dev evaluates only its head
        half = torch.tensor([idx.numel() // 2, 0], device=M.dev, dtype=torch.int32)
        out2 = torch.zeros((n, 4), device=M.dev)
        M.lib.check(L.nm_mlp_forward_listed(net.handle(), M.lib.dev_ptr(pts), M.lib.dev_ptr(dirs), n, M.lib.dev_ptr(idx, torch.int32),
                                            M.lib.dev_ptr(half, torch.int32), n, prec, 1.0, M.lib.dev_ptr(out2), M.lib.stream_ptr()), "listed")
    li = idx.long()
    assert torch.equal(out[li], full[li])
    rest = torch.ones(n, dtype=torch.bool, device=M.dev)
    rest[li] = False
    assert int(rest.sum()) > 0 and bool((out[rest] == 0).all())
    h = li[:idx.numel() // 2]
    assert torch.equal(out2[h], full[h]) and int((out2 != 0).any(1).sum()) <= h.numel()


def test_compact_points_equals_a_torch_restatement(M):
    grid = mask_grid(M, 5, p=0.4, res=16)
    lo, hi = grid.aabb[:3].to(M.dev), grid.aabb[3:].to(M.dev)
    inv = torch.tensor(16.0) / (grid.aabb[3:] - grid.aabb[:3])
    g = torch.Generator(device=M.dev).manual_seed(7)
    pts = lo + (hi - lo) * (torch.rand((20000, 3), device=M.dev, generator=g) * 1.4 - 0.2)      # ~ a third outside the box
    # points on cell faces (the lattice itself, in float32 as the box is cut) and on the box's faces
    k = torch.arange(17, device=M.dev, dtype=torch.float32)
    face = lo + k[:, None] * ((hi - lo) / 16.0)
    pts = torch.cat([pts, face, face.flip(0)[:, [1, 2, 0]], torch.stack([lo, hi]), torch.full((1, 3), float('nan'), device=M.dev)]).contiguous()
    idx, counts = grid.compact_points(pts)
    t = (pts - lo) * inv.to(M.dev)
    inside = ((t >= 0) & (t < 16)).all(1)
    c = torch.clamp(torch.nan_to_num(t, nan=0.0).long(), 0, 15)
    cell_occ = grid.to_mask()[c[:, 0], c[:, 1], c[:, 2]]
    want = torch.nonzero(~inside | cell_occ).reshape(-1)
    n = int(counts[0])
    assert n == want.numel() and int(counts[1]) == pts.shape[0] - n
    assert torch.equal(idx[:n].long(), want)
    assert 0 < int(inside.sum()) < pts.shape[0] and bool(cell_occ[inside].any()) and not bool(cell_occ[inside].all())


# ---- 2. the contract on every ray --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("render_can", [True, False])
def test_smpl_nerf_frame_is_the_masked_every_sample_frame(M, monkeypatch, render_can):
    net = human(M)
    grid = mask_grid(M, 1)
    verts, mesh = (M.can, None) if render_can else (M.posed, M.mesh)

    def render(trace):
        with torch.no_grad():
            return M.render.render_smpl_nerf_rays(net, M.o, M.d, verts, mesh, 64, True, render_can, 0.2, 1.0, None, trace)
    got, want = both(M, monkeypatch, [(net, grid)], render)
    assert_same(got, want)
    with torch.no_grad():
        plain = render(None)
    assert not torch.equal(got[0], plain[0])                     # the grid is consulted: it skips samples with sigma > 0
    M.occ.attach(net, grid)
    tr = {}
    with torch.no_grad():
        render(tr)
    M.occ.detach(net)
    st = tr['occupancy_human']
    ev, tot = sum(x['evaluated'] for x in st), sum(x['total'] for x in st)
    print(f"[occ human] render_can={render_can}: evaluated {ev} of {tot}")
    assert 0 < ev < tot


@pytest.mark.parametrize("render_can", [True, False])
def test_all_occupied_grid_reproduces_the_frame(M, render_can):
    net = human(M)
    grid = mask_grid(M, 0, p=2.0)
    verts, mesh = (M.can, None) if render_can else (M.posed, M.mesh)
    with torch.no_grad():
        want = M.render.render_smpl_nerf_rays(net, M.o, M.d, verts, mesh, 64, True, render_can, 0.2, 1.0)
        M.occ.attach(net, grid)
        got = M.render.render_smpl_nerf_rays(net, M.o, M.d, verts, mesh, 64, True, render_can, 0.2, 1.0)
        M.occ.detach(net)
    assert_same(got, want)


@pytest.mark.parametrize("render_can", [True, False])
def test_rays_whose_skipped_samples_are_empty_are_unchanged(M, render_can):
    """the undilated from_net grid on the opaque preset: fewer samples evaluated, and every ray whose skipped samples all have
    relu(sigma) = 0 in the every-sample pass is bit-identical.  (Seed 1 with the posenc encoding: its sigma > 0 set covers about half of the
    canonical box's 64^3 cells; the rotate-encoded seed-2 net of the other tests is positive in every cell.)"""
    net = human(M, 1, 'posenc')
    verts, mesh = (M.can, None) if render_can else (M.posed, M.mesh)
    with torch.no_grad():
        grid = M.occ.OccupancyGrid.from_net(net, M.box, res=64, dilate=0)
        tr0 = {}
        want = M.render.render_smpl_nerf_rays(net, M.o, M.d, verts, mesh, 64, True, render_can, 0.2, 1.0, None, tr0)
        M.occ.attach(net, grid)
        tr = {}
        got = M.render.render_smpl_nerf_rays(net, M.o, M.d, verts, mesh, 64, True, render_can, 0.2, 1.0, None, tr)
        M.occ.detach(net)
        hit = tr0['hit'][0].long()
        near, far = tr0['near'][0][hit], tr0['far'][0][hit]
        ho, hd = M.o[hit].contiguous(), M.d[hit].contiguous()
        raw, z = M.render.human_pass_rays(net, ho, hd, near, far, 64, mesh, render_can, 1.0, None, tp := {})
        if render_can:
            keep = keep_mask(grid, z.numel(), *grid.compact(ho, hd, z))
        else:
            keep = keep_mask(grid, z.numel(), *grid.compact_points(tp['can_pts'][0]))
    missed = (~keep.reshape(z.shape) & (raw[..., 3] > 0)).sum(1)
    good = hit[missed == 0]
    st = tr['occupancy_human'][0]
    print(f"[occ human from_net] render_can={render_can}: evaluated {st['evaluated']} of {st['total']}, {good.numel()} of {hit.numel()} hit rays exact")
    assert st['evaluated'] < 0.9 * st['total']
    assert good.numel() > 0
    for a, b in zip(got, want):
        assert torch.equal(a[good], b[good])


def test_hybrid_frame_takes_the_unfused_path_and_meets_the_contract(M, monkeypatch):
    coarse, fine, net = M.syn.make_joiner(0).to(M.dev), M.syn.make_joiner(1).to(M.dev), human(M)
    grid = mask_grid(M, 3)
    calls = []
    fused = M.render.render_hybrid_rays_fused
    monkeypatch.setattr(M.render, 'render_hybrid_rays_fused', lambda *a, **k: calls.append(1) or fused(*a, **k))

    def render(trace):
        with torch.no_grad():
            return M.render.render_hybrid_rays(coarse, fine, net, M.o, M.d, 0.0, 3.14, M.posed, M.mesh, 32, 32, True, 0.2, None, trace)
    got, want = both(M, monkeypatch, [(net, grid)], render)
    assert not calls                                              # a human grid: the fused call gives way
    assert_same(got, want)
    with torch.no_grad():
        render(None)
    assert calls                                                  # and without one it is taken again


def test_multi_person_frame_meets_the_contract(M, monkeypatch):
    coarse, fine = M.syn.make_joiner(0).to(M.dev), M.syn.make_joiner(1).to(M.dev)
    nets = [human(M, 2), human(M, 4)]
    posed2 = (M.posed + torch.tensor([0.3, 0.0, 0.1], device=M.dev)).contiguous()
    mesh2 = M.ray.mesh_to_device(posed2.cpu().numpy(), M.faces, M.mesh.T.cpu().numpy(), M.dev)
    grids = [mask_grid(M, 8), mask_grid(M, 9, p=0.3)]

    def render(trace):
        with torch.no_grad():
            return M.render.render_multi_rays(coarse, fine, nets, M.o, M.d, 0.0, 3.14, [M.posed, posed2], [M.mesh, mesh2], 32, 32, True, 0.2, None, trace)
    got, want = both(M, monkeypatch, list(zip(nets, grids)), render)
    assert_same(got, want)


# ---- 3. early termination ----------------------------------------------------------------------------------------------------
def test_march_with_a_grid(M):
    net = human(M)
    grid = mask_grid(M, 11)
    with torch.no_grad():
        near, far = M.ray.geometry_guided_near_far(M.o, M.d, M.posed, 0.2)
        hit, _ = M.ray.compact_hits(near, far)
        h = hit.long()
        ho, hd, hn, hf = M.o[h].contiguous(), M.d[h].contiguous(), near[h].contiguous(), far[h].contiguous()
        every, z = M.render.human_pass_rays(net, ho, hd, hn, hf, 64, M.mesh, False, 1.0, None, tr := {})
        raw0, z0 = M.render.human_march_rays(net, ho, hd, hn, hf, 64, M.mesh, 1e-3)
        M.occ.attach(net, grid)
        tg = {}
        raw1, z1 = M.render.human_march_rays(net, ho, hd, hn, hf, 64, M.mesh, 1e-3, trace=tg)
        M.occ.detach(net)
        keep = keep_mask(grid, z.numel(), *grid.compact_points(tr['can_pts'][0])).reshape(z.shape)
        c0 = M.render.raw2outputs(raw0, z0, hd, want_weights=False)
        c1 = M.render.raw2outputs(raw1, z1, hd, want_weights=False)
    assert torch.equal(z0, z) and torch.equal(z1, z)
    ev1 = (raw1 != 0).any(-1)
    assert bool(ev1.any()) and torch.equal(raw1[ev1], every[ev1])   # every evaluated sample is the every-sample pass's
    assert not bool(ev1[~keep].any())                               # nothing the grid skips is evaluated
    # rays whose skipped samples all have relu(sigma) = 0 march exactly as without the grid
    good = ((~keep) & (every[..., 3] > 0)).sum(1) == 0
    assert int(good.sum()) > 0
    for a, b in zip((c0[0], c0[2], c0[4]), (c1[0], c1[2], c1[4])):
        assert torch.equal(a[good], b[good])
    st = tg['occupancy_human'][0]
    assert 0 < st['evaluated'] < st['total']


def test_background_grid_with_termination_is_still_refused(M, monkeypatch):
    coarse = M.syn.make_joiner(1, preset='opaque').to(M.dev)
    M.occ.attach(coarse, mask_grid(M, 0, p=2.0))
    monkeypatch.setattr(M.render, 'TERMINATION_EPS', 1e-3)
    n, f = torch.zeros(M.o.shape[0], device=M.dev), torch.full((M.o.shape[0],), 3.14, device=M.dev)
    with pytest.raises(NotImplementedError), torch.no_grad():
        M.render.bkg_pass_rays(coarse, coarse, M.o, M.d, n, f, 16, 16, True)
    M.occ.detach(coarse)


# ---- 4. training never consults a grid ---------------------------------------------------------------------------------------
def test_human_trainer_step_ignores_the_grid(setup):  # noqa: F811
    from neuman_hip import occupancy
    S = setup
    params = [p for p in S.net.parameters() if p.requires_grad]

    def step():
        for p in params:
            p.grad = None
        torch.manual_seed(11)
        ld = S.loss.loss_func(S.batch)
        loss = sum(ld.values())
        loss.backward()
        return float(loss.detach()), [p.grad.detach().clone() if p.grad is not None else None for p in params]

    l0, g0 = step()
    l1, g1 = step()
    hn = S.net.coarse_human_net
    occupancy.attach(hn, occupancy.OccupancyGrid.from_mask(((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)),
                                                           torch.rand(16, 16, 16, generator=torch.Generator().manual_seed(0)) < 0.3))
    try:
        l2, g2 = step()
    finally:
        occupancy.detach(hn)
    spread_l = abs(l1 - l0)
    assert abs(l2 - l0) <= 2 * spread_l + 1e-6 * abs(l0)
    for a, b, c in zip(g0, g1, g2):
        assert (a is None) == (c is None)
        if a is None:
            continue
        spread = float((a - b).abs().max())
        assert float((a - c).abs().max()) <= 2 * spread + 1e-6 * float(a.abs().max()) + 1e-30
