"""The encoding fragments of a stage held in registers (csrc/mlp_i8as.h Enc, load_enc, k_bf): stage 0, the stage-5 skip and the views layer
read them from LDS once instead of once per output block.  No float operation changed, so every comparison is bit for bit:

  * the whole-network launch (nerf_mlp_i8s_kernel<WHOLE>) against the wave-specialised kernel of csrc/mlp.hip (NEUMAN_I8_KERNEL=w, another
    process: nerf_mlp_i8w_kernel shares none of these helpers);
  * the trunk / colour-head pair (NEUMAN_LIVE_FUSED=0: nerf_mlp_i8s_kernel<TRUNK>, nerf_head_i8s_kernel) and the one persistent launch
    (nerf_mlp_i8s_fused_kernel) against it: every density, the colour of every sample whose stored density is not <= 0, 0 elsewhere, and the
    tile counts every workgroup leaves in the workspace against tests/helpers/live_fused_tiles.py;
  * the plain-head net (<PLAIN>), which runs on this kernel only, against its records from before the change (tests/golden/i8_plain_head.npz).

Shapes: sample counts that leave clamped rows in a wave, a whole empty wave and a ragged last tile; rays of 256, 96 and 40 samples; a full grid
with two tiles per workgroup and a third for the first (the encoding area of a wave goes from positions to directions and back); both encodings,
band tables that are octaves and ones that are not; nets with every sample live and with none."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import i8_encoding_cases as C  # noqa: E402
import live_fused_tiles as T  # noqa: E402

from neuman_hip import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "i8_plain_head.npz")
RAY_CASES = sorted(k for k in C.ray_cases() if not k.endswith('_full')) + ['posenc_full', 'all_full', 'general_rotate_full']


@pytest.fixture(scope="module")
def wave_specialised(tmp_path_factory):
    """every case's whole-network records from nerf_mlp_i8w_kernel, computed once"""
    assert os.environ.get("NEUMAN_I8_KERNEL", "as") == "as", "this module wants the default kernel in-process"
    path = tmp_path_factory.mktemp("i8w") / "w.pt"
    subprocess.run([sys.executable, C.__file__, str(path)], check=True, env=dict(os.environ, NEUMAN_I8_KERNEL="w"), timeout=600)
    return torch.load(path)


class live_fused:
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


def bits(t):
    return t.contiguous().view(torch.int32)


def fused(net, o, d, z, sigma_scale):
    """nm_mlp_forward_rays_fused on a workspace of exactly its size -> (out, workspace)"""
    R, S = z.shape
    nbytes = int(_lib.lib().nm_mlp_live_fused_workspace_bytes(R * S))
    assert nbytes == T.workspace_bytes(R * S)
    ws = torch.full((nbytes,), 0xA5, device='cuda', dtype=torch.uint8)
    out = torch.full((R, S, 4), 7.0, device='cuda')
    _lib.check(_lib.lib().nm_mlp_forward_rays_fused(net.handle(), _lib.dev_ptr(o), _lib.dev_ptr(d), _lib.dev_ptr(z), R, S, float(sigma_scale), _lib.dev_ptr(out),
                                                   _lib.dev_ptr(ws, torch.uint8), nbytes, _lib.stream_ptr()), "nm_mlp_forward_rays_fused")
    return out, ws


@pytest.mark.parametrize("case", RAY_CASES)
def test_ray_form_bit_identical_on_every_route(case, wave_specialised):
    kind, R, S, scale = C.resolve(case)
    net = C.net_of(kind)
    o, d, z = C.rays(R, S)
    ref = wave_specialised[case].cuda()
    with torch.no_grad(), live_fused('0'):
        whole = net.forward_rays(o, d, z, precision='i8x3', sigma_scale=scale)
        pair = net.forward_rays(o, d, z, precision='i8x3', sigma_scale=scale, role='composite')
    got, ws = fused(net, o, d, z, scale)
    assert torch.isfinite(ref).all()
    assert torch.equal(bits(whole), bits(ref)), f"whole-network launch: max |diff| {(whole - ref).abs().max().item():.3e}"
    live = ~(ref[..., 3] <= 0)
    for name, out in (('pair', pair), ('fused', got)):
        assert torch.equal(bits(out[..., 3]), bits(ref[..., 3])), name
        assert torch.equal(bits(out[..., :3][live]), bits(ref[..., :3][live])), name
        assert (bits(out[..., :3][~live]) == 0).all(), name
    assert torch.equal(bits(got), bits(pair))
    frac = live.float().mean().item()
    if kind == 'all':
        assert frac == 1.0
    if kind == 'none':
        assert frac == 0.0
    # the trunk and head tiles every workgroup ran
    flat = live.reshape(-1).cpu().tolist()
    g = T.groups(len(flat))
    grid = min(g, C.cus())
    counts = T.group_counts(flat, grid)
    ran = ws[g * T.LIST_BYTES:g * T.LIST_BYTES + 8 * g].view(torch.int32).view(g, 2).cpu()[:grid]
    for wg, c in enumerate(counts):
        assert ran[wg].tolist() == [len(c), T.head_tiles(c)[0]], (wg, c, ran[wg].tolist())
    if case.endswith('_full'):
        assert [len(c) for c in counts] == [3] + [2] * (grid - 1)
        order = ''.join(T.schedule(counts[0])[0])
        if kind == 'all':
            assert 'THT' in order or 'THHT' in order, order                 # positions, directions, positions again in one wave's encoding area
    print(f"[i8 encoding regs] {case}: live fraction {frac:.3f}, head tiles {sum(T.head_tiles(c)[0] for c in counts)}")


@pytest.mark.parametrize("case", sorted(C.point_cases()))
def test_point_form_equals_the_wave_specialised_kernel(case, wave_specialised):
    kind, n = C.point_cases()[case]
    p, d = C.points(n)
    with torch.no_grad():
        whole = C.net_of(kind)(p, d, precision='i8x3')
    ref = wave_specialised[case].cuda()
    assert torch.isfinite(ref).all() and torch.equal(bits(whole), bits(ref))


@pytest.mark.parametrize("kind", ['plain_posenc', 'plain_rotate'])
def test_plain_head_equals_its_records_from_before(kind):
    """the records of the first n of the 513 points are the same whatever n is (a row's arithmetic is its own): every count is checked on a prefix"""
    gold = {k[len(kind) + 1:]: torch.from_numpy(v) for k, v in np.load(GOLDEN).items() if k.startswith(kind + '_')}
    inputs = {k: gold[k] for k in ('p', 'dv', 'o', 'd', 'z')}
    got = C.plain_outputs(kind, inputs)
    assert torch.isfinite(gold['pts']).all() and torch.isfinite(gold['rays']).all()
    assert torch.equal(bits(got['pts']), bits(gold['pts']))
    assert torch.equal(bits(got['rays']), bits(gold['rays']))
    net = C.net_of(kind)
    for n in C.COUNTS[:-1]:
        with torch.no_grad():
            out = net(inputs['p'][:n].cuda(), inputs['dv'][:n].cuda(), precision='i8x3').cpu()
        assert torch.equal(bits(out), bits(gold['pts'][:n])), n
