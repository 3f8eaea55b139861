"""forward_rays(role='composite') -- nm_mlp_forward_rays_live: a trunk launch that writes every density and lists the samples whose stored
density is not <= 0, then a colour-head launch over that list (csrc/mlp_i8s.hip TRUNK, csrc/mlp_i8h.hip) -- against forward_rays(role='shading'),
the one launch that evaluates the whole network on every sample.  A listed sample's record is bit-identical, every other sample's colour is exactly
0 (its compositing weight is exactly 0), and so the composite is bit-identical."""
import pytest
import torch

from neuman_hip import render_utils, synthetic

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5), (257, 64), (1000, 129)]          # less than one wave | 64 tiles and a ragged one | odd S: waves and head tiles straddle rays


def _net(kind):
    if kind == 'bench_fine':                          # both classes of sample
        net = synthetic.make_joiner(1)
    elif kind == 'fog':                               # every sample live: the list at capacity
        net = synthetic.make_joiner(0, preset='fog')
    elif kind == 'empty':                             # no live sample: the head launch runs on a count of 0
        net = synthetic.make_joiner(0)
        with torch.no_grad():
            net.nerf.alpha_linear.bias.fill_(-1e3)
    elif kind == 'plain':                             # no colour head to split off: the whole-network launch
        net = synthetic.make_variant_joiner(5, posenc='posenc', use_viewdirs=False)
    else:
        raise ValueError(kind)
    net.precision = 'mixed'
    return net.to('cuda')


def _rays(R, S, seed=3):
    g = torch.Generator(device='cuda').manual_seed(seed)
    o = torch.randn((R, 3), device='cuda', generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn((R, 3), device='cuda', generator=g), dim=-1)
    z = torch.sort(torch.rand((R, S), device='cuda', generator=g) * 3.0, dim=1).values.contiguous()
    return o, d, z


def _check(net, kind, R, S, **kw):
    o, d, z = _rays(R, S)
    scale = {k: v for k, v in kw.items() if k == 'sigma_scale'}
    with torch.no_grad():
        ref = net.forward_rays(o, d, z, role='shading', **scale)
        got = net.forward_rays(o, d, z, role='composite', **kw)
    assert torch.isfinite(ref).all() and torch.isfinite(got).all()
    live = ref[..., 3] > 0
    frac = live.float().mean().item()
    print(f"[live heads] {kind} {R}x{S} {kw}: live fraction {frac:.3f}")
    if kind == 'plain':
        assert torch.equal(got, ref)
        return
    if kind == 'bench_fine':                          # each class at least 10 % of the samples
        assert 0.1 <= frac <= 0.9
    if kind == 'fog':
        assert frac == 1.0
    if kind == 'empty':
        assert frac == 0.0
    assert torch.equal(got[..., 3], ref[..., 3])
    assert torch.equal(got[..., :3][live], ref[..., :3][live])
    assert (got[..., :3][~live] == 0).all()
    a = render_utils.raw2outputs(ref, z, d)
    b = render_utils.raw2outputs(got, z, d)
    for i, name in ((0, 'rgb'), (4, 'depth'), (2, 'acc')):
        assert torch.equal(a[i], b[i]), name


@pytest.mark.parametrize("R,S", SHAPES)
@pytest.mark.parametrize("kind", ['bench_fine', 'fog', 'empty', 'plain'])
def test_composite_role_equals_shading_where_it_is_seen(kind, R, S):
    _check(_net(kind), kind, R, S)


def test_chunked_walk():
    """chunk_samples = 4096 at S = 64: 64 rays per chunk, five chunks, the last of one ray -- the list and its counter are reused"""
    _check(_net('bench_fine'), 'bench_fine', 257, 64, chunk_samples=4096)


def test_sigma_scale():
    """liveness is decided on the STORED density sigma * sigma_scale"""
    _check(_net('bench_fine'), 'bench_fine', 257, 64, sigma_scale=0.7)


def test_render_vanilla_rays_is_bit_equal_to_the_whole_network_passes():
    """the frame path that takes the tag (render_vanilla_rays -> bkg_shade(composite_only=True)) at the benchmark's 128 + 128 samples, where one tile of the trunk is one ray"""
    coarse, fine = synthetic.make_joiner(0).to('cuda'), _net('bench_fine')
    coarse.precision = 'mixed'
    R, S, N = 64, 128, 128
    o, d, _ = _rays(R, 1, seed=11)
    near, far = 0.2, 3.0
    with torch.no_grad():
        rgb, depth = render_utils.render_vanilla_rays(coarse, fine, o, d, near, far, S, N, True)
        n = torch.full((R,), near, device='cuda')
        f = torch.full((R,), far, device='cuda')
        z, raw = render_utils.bkg_place_z(coarse, fine, o, d, n, f, S, N, True)
        assert raw is None and z.shape == (R, S + N)
        raw = fine.forward_rays(o, d, z, role='shading')
        want = render_utils.raw2outputs(raw, z, d, white_bkg=True, want_weights=False)
    live = (raw[..., 3] > 0).float().mean().item()
    print(f"[live heads] render_vanilla_rays {R} rays {S}+{N}: live fraction {live:.3f}")
    assert torch.equal(rgb, want[0]) and torch.equal(depth, want[4])
