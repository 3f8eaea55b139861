"""nerf_mlp_i8s_fused_kernel (csrc/mlp_i8f.hip; nm_mlp_forward_rays_fused, and nm_mlp_forward_rays_live under NEUMAN_LIVE_FUSED=1): the trunk /
colour-head pair as one persistent launch in which every workgroup shades the live samples of its own trunk tiles.  Every case compares `out` with
the pair's (NEUMAN_LIVE_FUSED=0) and with the whole-network launch's: every density equal, the colour of every sample whose stored density is not
<= 0 equal, every other colour exactly 0 -- bit for bit -- and the trunk and head tiles each workgroup reports having run with what
tests/helpers/live_fused_tiles.py predicts from the whole-network launch's densities."""
import os

import pytest
import torch

from helpers import live_fused_tiles as T
from neuman_hip import _lib, render_utils, synthetic, vanilla

pytestmark = pytest.mark.gpu

_NETS = {}
_CACHE = {}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def net_of(kind):
    """'mixed': make_joiner as is | 'all': the alpha bias raised, every sample live | 'none': lowered, none live | 'other': another net"""
    if kind not in _NETS:
        net = synthetic.make_joiner(7 if kind == 'other' else 1)
        with torch.no_grad():
            if kind == 'all':
                net.nerf.alpha_linear.bias.fill_(1e3)
            elif kind == 'none':
                net.nerf.alpha_linear.bias.fill_(-1e3)
        net.precision = 'mixed'
        _NETS[kind] = net.to('cuda')
    return _NETS[kind]


def rays(R, S, seed=3):
    g = torch.Generator(device='cuda').manual_seed(seed)
    o = torch.randn((R, 3), device='cuda', generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn((R, 3), device='cuda', generator=g), dim=-1)
    z = torch.sort(torch.rand((R, S), device='cuda', generator=g) * 3.0, dim=1).values.contiguous()
    return o, d, z


class switch:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get('NEUMAN_LIVE_FUSED')
        os.environ['NEUMAN_LIVE_FUSED'] = self.value

    def __exit__(self, *a):
        if self.old is None:
            del os.environ['NEUMAN_LIVE_FUSED']
        else:
            os.environ['NEUMAN_LIVE_FUSED'] = self.old


def fused(net, o, d, z, sigma_scale=1.0, ws=None):
    """nm_mlp_forward_rays_fused on a workspace of exactly its size (or the caller's) -> (out, workspace)"""
    R, S = z.shape
    nbytes = int(_lib.lib().nm_mlp_live_fused_workspace_bytes(R * S))
    assert nbytes == T.workspace_bytes(R * S)
    if ws is None:
        ws = torch.full((nbytes,), 0xA5, device='cuda', dtype=torch.uint8)
    out = torch.full((R, S, 4), 7.0, device='cuda')
    _lib.check(_lib.lib().nm_mlp_forward_rays_fused(net.handle(), _lib.dev_ptr(o), _lib.dev_ptr(d), _lib.dev_ptr(z), R, S, float(sigma_scale), _lib.dev_ptr(out),
                                                   _lib.dev_ptr(ws, torch.uint8), nbytes, _lib.stream_ptr()), "nm_mlp_forward_rays_fused")
    return out, ws


def bits(t):
    return t.contiguous().view(torch.int32)


def references(kind, R, S, sigma_scale=1.0, seed=3):
    """the whole-network launch's and the pair's records for a case, computed once"""
    key = (kind, R, S, sigma_scale, seed)
    if key not in _CACHE:
        net = net_of(kind)
        o, d, z = rays(R, S, seed)
        with torch.no_grad(), switch('0'):
            whole = net.forward_rays(o, d, z, role='shading', sigma_scale=sigma_scale)
            pair = net.forward_rays(o, d, z, role='composite', sigma_scale=sigma_scale)
        _CACHE[key] = (o, d, z, whole, pair)
    return _CACHE[key]


def compare(got, whole, pair):
    live = ~(whole[..., 3] <= 0)                                    # (a NaN density is live)
    assert torch.equal(bits(got[..., 3]), bits(whole[..., 3])) and torch.equal(bits(got[..., 3]), bits(pair[..., 3]))
    assert torch.equal(bits(got[..., :3][live]), bits(whole[..., :3][live]))
    assert (bits(got[..., :3][~live]) == 0).all()
    assert torch.equal(bits(got), bits(pair))
    return live


def tiles_of(ws, n):
    g = T.groups(n)
    t = ws[g * T.LIST_BYTES:g * T.LIST_BYTES + 8 * g].view(torch.int32).view(g, 2).cpu()
    return t[:min(g, cus())]


def check_tiles(ws, live):
    """-> the live counts of every workgroup's trunk tiles; the tiles it reports are the ones the rule gives"""
    flat = live.reshape(-1).cpu().tolist()
    grid = min(T.groups(len(flat)), cus())
    counts = T.group_counts(flat, grid)
    ran = tiles_of(ws, len(flat))
    for wg, c in enumerate(counts):
        assert ran[wg].tolist() == [len(c), T.head_tiles(c)[0]], (wg, c, ran[wg].tolist())
    return counts


def run(kind, R, S, sigma_scale=1.0):
    o, d, z, whole, pair = references(kind, R, S, sigma_scale)
    got, ws = fused(net_of(kind), o, d, z, sigma_scale)
    live = compare(got, whole, pair)
    frac = live.float().mean().item()
    counts = check_tiles(ws, live)
    print(f"[live fused] {kind} {R}x{S} scale {sigma_scale}: live fraction {frac:.3f}, head tiles {sum(T.head_tiles(c)[0] for c in counts)}")
    if kind == 'all':
        assert frac == 1.0
    if kind == 'none':
        assert frac == 0.0 and int(tiles_of(ws, R * S)[:, 1].sum()) == 0
    return counts


def five_tiles_shape():
    return 5 * 256 * cus() // 48, 48                                 # S = 48: a wave's 32 samples span rays, a head tile's entries come from many


# one sample | the edges of a tile | every workgroup one tile, then one of them two | five tiles each at S = 48
SHAPES = ['1x1', '255x1', '256x1', '257x1', 'CUx256', 'CU+1x256', 'five']


def shape_of(name):
    if name == 'five':
        return five_tiles_shape()
    r, s = name.split('x')
    return {'CU': cus(), 'CU+1': cus() + 1}.get(r) or int(r), int(s)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ['mixed', 'all', 'none'])
def test_fused_equals_pair_and_whole_network(kind, shape):
    R, S = shape_of(shape)
    counts = run(kind, R, S)
    if shape == 'CU+1x256':
        assert [len(c) for c in counts] == [2] + [1] * (cus() - 1)
    if shape == 'five':
        assert all(len(c) == 5 for c in counts)
        if kind == 'all':                                           # head tiles between the trunk tiles: every hand-over of the ring is walked
            k = T.schedule(counts[0])[0]
            assert all(T.schedule(c)[0] == k for c in counts) and {a + b for a, b in zip(k, k[1:])} == {'TT', 'TH', 'HH', 'HT'}
        if kind == 'mixed':
            assert any('T' in T.schedule(c)[0][T.schedule(c)[0].index('H'):] for c in counts if sum(c) >= 256), "no head tile with a trunk tile behind it"


@pytest.mark.parametrize("when,fraction", [(2, 0.55), (3, 0.40), (5, 0.22)])
def test_list_first_full_on_a_given_tile(when, fraction):
    """the alpha bias tuned so that `fraction` of the samples are live: some workgroup's list first holds 256 entries after its second, its third,
    its last trunk tile"""
    R, S = five_tiles_shape()
    kind = f'tuned{when}'
    if kind not in _NETS:
        base = net_of('mixed')
        o, d, z = rays(R, S)
        with torch.no_grad():
            sigma = base.forward_rays(o, d, z, role='shading')[..., 3]
            net = synthetic.make_joiner(1)
            net.nerf.alpha_linear.bias.sub_(torch.quantile(sigma.reshape(-1)[:1 << 20].cpu(), 1.0 - fraction))
        net.precision = 'mixed'
        _NETS[kind] = net.to('cuda')
    counts = run(kind, R, S)
    firsts = [T.first_full(c) for c in counts]
    print(f"[live fused] first full after tile: {sorted(set(firsts))}")
    assert when in firsts


@pytest.mark.parametrize("extra", [1, 255])
def test_remainder_of_one_and_of_255_entries(extra):
    """every sample live, one tile per workgroup and `extra` samples more: workgroup 0 lists 256 + extra entries, a full head tile and the remainder"""
    counts = run('all', 256 * cus() + extra, 1)
    assert counts[0] == [256, extra] and T.head_tiles(counts[0]) == (2, extra)
    counts = run('all', extra, 1)
    assert counts == [[extra]]


def test_sigma_scale():
    """liveness is decided on the STORED density sigma * sigma_scale"""
    run('mixed', *five_tiles_shape(), sigma_scale=0.7)


def test_nan_density_is_live():
    """a NaN density counts as live, as in the pair (`not <= 0`).  The library refuses a net with a NaN weight (tests/test_mlp_pack_edges.py), so
    the NaN comes from sigma_scale: every stored density is NaN, every sample is listed, every colour is the whole-network launch's"""
    R, S = 700, 3
    o, d, z, whole, pair = references('mixed', R, S, float('nan'))
    assert torch.isnan(whole[..., 3]).all()
    got, ws = fused(net_of('mixed'), o, d, z, float('nan'))
    live = compare(got, whole, pair)
    assert live.all() and torch.equal(bits(got[..., :3]), bits(whole[..., :3]))
    check_tiles(ws, live)


def test_stale_entries_of_another_net():
    """two calls on one workspace that is not cleared between them, the second with another net: its lists start from the first call's entries"""
    R, S = five_tiles_shape()
    o, d, z, whole, pair = references('all', R, S)
    _, ws = fused(net_of('all'), o, d, z)
    o2, d2, z2, whole2, pair2 = references('other', R, S, seed=5)
    got, ws = fused(net_of('other'), o2, d2, z2, ws=ws)
    check_tiles(ws, compare(got, whole2, pair2))


def test_non_default_stream():
    R, S = five_tiles_shape()
    o, d, z, whole, pair = references('mixed', R, S)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        got, ws = fused(net_of('mixed'), o, d, z)
    st.synchronize()
    check_tiles(ws, compare(got, whole, pair))


def test_switch_through_render_vanilla_rays(monkeypatch):
    """NEUMAN_LIVE_FUSED at both values through the frame path, 64 rays x (16 + 16) samples: equal frames; under 1 the workspace's last block holds
    the fused launch's tile counts, under 0 nothing has written there"""
    coarse, fine = synthetic.make_joiner(0).to('cuda'), net_of('mixed')
    coarse.precision = 'mixed'
    R, S, N = 64, 16, 16
    n = R * (S + N)
    o, d, _ = rays(R, 1, seed=11)
    handed = []
    inner = vanilla.live_workspace_for

    def spy(*a, **k):
        ws, nbytes = inner(*a, **k)
        ws.fill_(0xFF)
        handed.append(ws)
        return ws, nbytes

    monkeypatch.setattr(vanilla, 'live_workspace_for', spy)
    frames = {}
    for value in ('0', '1'):
        del handed[:]
        with torch.no_grad(), switch(value):
            frames[value] = render_utils.render_vanilla_rays(coarse, fine, o, d, 0.2, 3.0, S, N, True)
        assert handed and handed[-1].numel() >= T.workspace_bytes(n)
        ran = tiles_of(handed[-1], n)
        if value == '1':
            assert ran[:, 0].tolist() == [1] * T.groups(n) and (ran[:, 1] <= 1).all()
        else:
            assert (ran == -1).all()
    for a, b in zip(frames['0'], frames['1']):
        assert torch.equal(a, b)
    assert torch.isfinite(frames['1'][0]).all()
