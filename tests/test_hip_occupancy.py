"""-m gpu: occupancy-grid empty-space skipping (neuman_hip/occupancy.py, csrc/occupancy.hip, in_mode 3 of csrc/mlp_device.h).

A skipped sample keeps raw = 0 -- weight 0, as relu(sigma) = 0 gives -- so every ray whose skipped samples all have relu(sigma) = 0 in the
every-sample evaluation must come out bit-identical; the other rays are counted and reported, not gated."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_occupancy_host import restated_offsets

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.0, 3.14


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import types
    from neuman_hip import occupancy, ray_utils, render_utils, synthetic
    return types.SimpleNamespace(occ=occupancy, ray=ray_utils, render=render_utils, syn=synthetic)


def frame_rays(M, W):
    return M.render._pixel_rays(M.syn.SimpleCapture(W, W), torch.device('cuda'))


def skipped_mask(grid, o, d, z):
    """[R, S] bool: the samples the grid skips (nm_occ_compact_samples' complement)"""
    idx, counts = grid.compact(o.contiguous(), d.contiguous(), z.contiguous())
    keep = torch.zeros(z.numel(), dtype=torch.bool, device=z.device)
    keep[idx[:int(counts[0])].long()] = True
    return ~keep.reshape(z.shape)


def missed_per_ray(grid, o, d, z, sigma):
    """skipped samples whose every-sample relu(sigma) is > 0, per ray"""
    return (skipped_mask(grid, o, d, z) & (sigma > 0)).sum(1)


def two_pass_misses(M, coarse, fine, o, d, trace0, gc, gf, precision=None):
    """per ray: misses of the coarse pass (on its stratified samples) + of the fine pass (on the final samples), both taken from the
    every-sample run's trace"""
    cz, fz = torch.cat(trace0['coarse_z']), torch.cat(trace0['bkg_z'])
    with torch.no_grad():
        sc = coarse.forward_rays(o, d, cz, precision=precision, role=None, sigma_only=True)[..., 3]
        sf = fine.forward_rays(o, d, fz, precision=precision, role='shading')[..., 3]
    return missed_per_ray(gc, o, d, cz, sc) + missed_per_ray(gf, o, d, fz, sf)


# ---- 1. the grid's bits against a restatement in torch -------------------------------------------------------------------------
@pytest.mark.parametrize("dilate,thr", [(1, 0.0), (0, 0.0), (1, 50.0)])
def test_grid_bits_match_a_torch_restatement(M, dilate, thr):
    net = M.syn.make_joiner(1, preset='opaque').cuda()
    res, probes, seed = 32, 8, 3
    box = M.occ.rays_aabb(*frame_rays(M, 64), NEAR, FAR)
    grid = M.occ.OccupancyGrid.from_net(net, box, res=res, probes=probes, dilate=dilate, sigma_threshold=thr, seed=seed)
    lo, hi = box[:3].cuda(), box[3:].cuda()
    cs = (hi - lo) / torch.tensor(float(res), device='cuda')
    off = torch.as_tensor(restated_offsets(probes, seed)).cuda()                      # [P, 3]
    ii = torch.arange(res, device='cuda', dtype=torch.float32)
    cell = torch.stack(torch.meshgrid(ii, ii, ii, indexing='ij'), -1)               # [i, j, k, 3]
    pts = lo + (cell[:, :, :, None, :] + off) * cs                                  # [res, res, res, P, 3]
    dirs = torch.zeros_like(pts)
    dirs[..., 0] = 1.0
    with torch.no_grad():
        sigma = net(pts.reshape(-1, 3), dirs.reshape(-1, 3))[:, 3].reshape(res, res, res, probes)
    mx = sigma.max(-1).values
    k = 2 * dilate + 1

    def dil(m):
        return F.max_pool3d(m.float()[None, None], k, 1, dilate)[0, 0] > 0 if dilate else m
    want = dil(mx > thr)
    unsure = dil((mx - thr).abs() <= 1e-3)
    got = grid.to_mask()
    frac = float(got.float().mean())
    print(f"[occupancy] grid {res}^3 x {probes} probes, dilate {dilate}, threshold {thr}: occupied {frac:.3f}, cells near the threshold "
          f"{int(unsure.sum())}, differing bits elsewhere {int((got != want)[~unsure].sum())}")
    assert torch.equal(got[~unsure], want[~unsure])
    assert 0.0 < frac < 1.0


# ---- 2. fog: every cell occupied, nothing skipped, frames equal ----------------------------------------------------------------
@pytest.mark.parametrize("precision", ["mixed", "fp16x3"])
def test_fog_grid_is_a_no_op(M, precision):
    coarse = M.syn.make_joiner(0, preset='fog').cuda()
    fine = M.syn.make_joiner(1, preset='fog').cuda()
    o, d = frame_rays(M, 800)
    box = M.occ.rays_aabb(o, d, NEAR, FAR)
    rgb0, dep0 = M.render.render_vanilla_rays(coarse, fine, o, d, NEAR, FAR, 128, 128, True, precision=precision)
    gc = M.occ.OccupancyGrid.from_net(coarse, box, precision=precision)
    gf = M.occ.OccupancyGrid.from_net(fine, box, precision=precision)
    assert gc.occupied_fraction() == 1.0 and gf.occupied_fraction() == 1.0
    M.occ.attach(coarse, gc)
    M.occ.attach(fine, gf)
    tr = {}
    try:
        rgb1, dep1 = M.render.render_vanilla_rays(coarse, fine, o, d, NEAR, FAR, 128, 128, True, precision=precision, trace=tr)
    finally:
        M.occ.detach(coarse)
        M.occ.detach(fine)
    for key in ('occupancy_coarse', 'occupancy'):
        st = tr[key][0]
        assert st['evaluated'] == st['total'] == 640000 * (128 if key == 'occupancy_coarse' else 256), (key, st)
    assert torch.equal(rgb0, rgb1) and torch.equal(dep0, dep1)


# ---- 3. opaque: exact wherever the grid is right ------------------------------------------------------------------------------
# The opaque field's encoding reaches 2^9 rad / unit: its sigma > 0 set is finer than a 128^3 cell (~0.02), so the default conservative
# grid (dilate 1) is ~93 % occupied and skips ~4 % of the coarse samples.  The undilated grid skips the 30 % the
# skipping is for, with misses on most rays: measured and reported here, its exactness checked on the rays it gets right.
@pytest.mark.parametrize("dilate,min_skipped", [(1, 0.03), (0, 0.30)])
def test_opaque_frame_is_exact_on_rays_the_grid_gets_right(M, dilate, min_skipped):
    net = M.syn.make_joiner(1, preset='opaque').cuda()                                # seed 1 for both passes, as bench.py's termination leg
    o, d = frame_rays(M, 800)
    tr0 = {}
    rgb0, dep0 = M.render.render_vanilla_rays(net, net, o, d, NEAR, FAR, 128, 128, True, trace=tr0)
    grid = M.occ.OccupancyGrid.from_net(net, M.occ.rays_aabb(o, d, NEAR, FAR), dilate=dilate)
    M.occ.attach(net, grid)
    tr1 = {}
    try:
        rgb1, dep1 = M.render.render_vanilla_rays(net, net, o, d, NEAR, FAR, 128, 128, True, trace=tr1)
    finally:
        M.occ.detach(net)
    miss = two_pass_misses(M, net, net, o, d, tr0, grid, grid)
    clean = miss == 0
    sc, sf = tr1['occupancy_coarse'][0], tr1['occupancy'][0]
    e_other = float((rgb1 - rgb0).abs()[~clean].max()) if bool((~clean).any()) else 0.0
    print(f"[occupancy] opaque 800x800 128+128, dilate {dilate}: grid occupied {grid.occupied_fraction():.3f}; evaluated coarse "
          f"{sc['evaluated'] / sc['total']:.3f}, fine {sf['evaluated'] / sf['total']:.3f}; rays with missed samples {int((~clean).sum())} of "
          f"{clean.numel()} ({int(miss.sum())} samples), L-inf there {e_other:.3e}")
    assert torch.equal(rgb0[clean], rgb1[clean]) and torch.equal(dep0[clean], dep1[clean])
    assert sc['evaluated'] <= (1.0 - min_skipped) * sc['total']
    if dilate:
        assert float(clean.float().mean()) > 0.9                                       # (the comparison above covers most of the frame)


# ---- 4. user masks --------------------------------------------------------------------------------------------------------------
def test_user_masks(M):
    coarse, fine = M.syn.make_joiner(0).cuda(), M.syn.make_joiner(1).cuda()
    o, d = frame_rays(M, 200)
    box = M.occ.rays_aabb(o, d, NEAR, FAR)
    rgb0, dep0 = M.render.render_vanilla_rays(coarse, fine, o, d, NEAR, FAR, 64, 64, True)
    for full in (True, False):
        mask = torch.full((64, 64, 64), full, dtype=torch.bool)
        g = M.occ.OccupancyGrid.from_mask(box, mask)
        M.occ.attach(coarse, g)
        M.occ.attach(fine, g)
        try:
            rgb1, dep1 = M.render.render_vanilla_rays(coarse, fine, o, d, NEAR, FAR, 64, 64, True)
        finally:
            M.occ.detach(coarse)
            M.occ.detach(fine)
        if full:
            assert torch.equal(rgb0, rgb1) and torch.equal(dep0, dep1)
        else:
            assert bool((rgb1 == 1.0).all()) and bool((dep1 == 0.0).all())


# ---- 5. the hybrid renderer -----------------------------------------------------------------------------------------------------
def test_hybrid_frame_is_exact_on_rays_the_grid_gets_right(M):
    verts_c, faces = M.syn.capsule_mesh(n_rings=10, n_seg=12)
    posed, T = M.syn.twist_transforms(verts_c)
    cap = M.syn.SimpleCapture(96, 96, fx=192., c2w=M.syn.spherical_c2w(20., -10., 3.0), near=0.5, far=4.0)
    bkg = M.syn.make_joiner(1, preset='opaque').cuda()
    human = M.syn.make_joiner(2, 'rotate').cuda()
    o, d = M.render._pixel_rays(cap, torch.device('cuda'))
    faces3 = np.ascontiguousarray(np.asarray(faces)[:, :3], np.int32)
    mesh = M.ray.mesh_to_device(posed, faces3, T, 'cuda')
    pv = torch.as_tensor(np.ascontiguousarray(posed)).to('cuda', torch.float32)
    args = (o, d, cap.near['bkg'], cap.far['bkg'], pv, mesh, 64, 64)
    tr0 = {}
    rgb0, dep0, acc0 = M.render.render_hybrid_rays(bkg, bkg, human, *args, geo_threshold=0.2, trace=tr0)
    rgbf, depf, accf = M.render.render_hybrid_rays(bkg, bkg, human, *args, geo_threshold=0.2)         # the fused path
    assert torch.equal(rgb0, rgbf)
    grid = M.occ.OccupancyGrid.from_net(bkg, M.occ.rays_aabb(o, d, cap.near['bkg'], cap.far['bkg']), res=64)
    M.occ.attach(bkg, grid)
    tr1 = {}
    try:
        rgb1, dep1, acc1 = M.render.render_hybrid_rays(bkg, bkg, human, *args, geo_threshold=0.2, trace=tr1)
        rgb2, _, _ = M.render.render_hybrid_rays(bkg, bkg, human, *args, geo_threshold=0.2)           # no trace: the fused call gives way
    finally:
        M.occ.detach(bkg)
    assert torch.equal(rgb1, rgb2)
    clean = two_pass_misses(M, bkg, bkg, o, d, tr0, grid, grid) == 0
    sc = tr1['occupancy_coarse'][0]
    hits = int(torch.cat(tr0['hit']).numel()) if 'hit' in tr0 else 0
    print(f"[occupancy] hybrid 96x96: {hits} body rays; coarse evaluated {sc['evaluated'] / sc['total']:.3f}; rays with missed background samples "
          f"{int((~clean).sum())} of {clean.numel()}")
    assert hits > 0 and sc['evaluated'] < sc['total']
    assert torch.equal(rgb0[clean], rgb1[clean]) and torch.equal(dep0[clean], dep1[clean]) and torch.equal(acc0[clean], acc1[clean])


# ---- 6. refusals on the device path ---------------------------------------------------------------------------------------------
def test_termination_with_a_grid_is_refused(M, monkeypatch):
    net = M.syn.make_joiner(1, preset='opaque').cuda()
    o, d = frame_rays(M, 16)
    M.occ.attach(net, M.occ.OccupancyGrid.from_net(net, M.occ.rays_aabb(o, d, NEAR, FAR), res=16))
    monkeypatch.setattr(M.render, 'TERMINATION_EPS', 1e-3)
    try:
        with pytest.raises(NotImplementedError):
            M.render.render_vanilla_rays(net, net, o, d, NEAR, FAR, 16, 16, True)
    finally:
        M.occ.detach(net)


def test_time_conditioned_net_is_refused_on_device(M):
    j4 = M.syn.make_variant_joiner(6, raw_pos_dim=4).cuda()
    with pytest.raises(NotImplementedError):
        M.occ.OccupancyGrid.from_net(j4, ((0, 0, 0), (1, 1, 1)), res=8)


# ---- 7. the sample-list launch on its own ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16x3", "i8x3", "bf16x3", "bf16"])
@pytest.mark.parametrize("sigma_only", [False, True])
def test_sample_list_launch_equals_forward_rays(M, precision, sigma_only):
    from neuman_hip import _lib
    net = M.syn.make_joiner(0).cuda()
    g = torch.Generator(device='cuda').manual_seed(5)
    R, S = 3001, 48
    o = torch.randn(R, 3, device='cuda', generator=g) * 0.3
    d = torch.randn(R, 3, device='cuda', generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    z = torch.sort(torch.rand(R, S, device='cuda', generator=g) * 3.0, dim=1).values.contiguous()
    with torch.no_grad():
        ref = net.forward_rays(o, d, z, precision=precision, sigma_only=sigma_only).reshape(-1, 4)
    n = 50021
    idx = torch.randperm(R * S, device='cuda', generator=g)[:n].to(torch.int32)       # any order, not only the compaction's
    entry = _lib.lib().nm_mlp_sigma_samples if sigma_only else _lib.lib().nm_mlp_forward_samples
    for n_dev in (torch.tensor([n], device='cuda', dtype=torch.int32), None):
        out = torch.zeros(R, S, 4, device='cuda')
        n_max = R * S if n_dev is not None else n                                     # a device count under a generous bound, or the exact length
        _lib.check(entry(net.handle(), _lib.dev_ptr(o), _lib.dev_ptr(d), _lib.dev_ptr(z), R, S, _lib.dev_ptr(idx, torch.int32),
                         _lib.dev_ptr(n_dev, torch.int32), n_max, _lib.PRECISIONS[precision], 1.0, _lib.dev_ptr(out), _lib.stream_ptr()), "samples")
        flat = out.reshape(-1, 4)
        sel = idx.long()
        assert torch.equal(flat[sel], ref[sel])
        rest = torch.ones(R * S, dtype=torch.bool, device='cuda')
        rest[sel] = False
        assert bool((flat[rest] == 0).all())
