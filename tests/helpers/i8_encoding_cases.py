"""The cases of tests/test_hip_i8_encoding_regs.py: nets, seeded inputs, and the whole-network NM_PREC_I8X3 outputs of the kernel the library
picks (nerf_mlp_i8s_kernel by default, nerf_mlp_i8w_kernel of csrc/mlp.hip under NEUMAN_I8_KERNEL=w -- the library reads the switch once per
process, so the test runs this file as a script for the other side):

    python i8_encoding_cases.py OUT.pt             the whole-network outputs of every ray and point case
    python i8_encoding_cases.py --golden OUT.npz   the plain-head net's inputs and outputs (tests/golden/i8_plain_head.npz was written by this on the
                                                   commit before the encoding fragments moved to registers: the plain head has no second kernel)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "ml-neuman_amd"))
import torch  # noqa: E402

from neuman_hip import synthetic  # noqa: E402

TILE = 256
COUNTS = [1, 31, 32, 33, 255, 256, 257, 513]        # clamped rows in a wave | a whole wave | one row of the next | a ragged tile | ... | a third tile of one row
GENERAL = dict(pos_min_freq=1, dir_max_freq=2.5)    # band tables that are no octaves: fill_pe_wave's pe_feature path for both encodings

_NETS = {}


def net_of(kind):
    """'posenc' / 'rotate': the octave path of both encodings | 'general' / 'general_rotate': the pe_feature path | 'all' / 'none': every sample
    live, none | 'plain_posenc' / 'plain_rotate': the use_viewdirs=False net"""
    if kind not in _NETS:
        if kind == 'posenc':
            net = synthetic.make_joiner(1)
        elif kind == 'rotate':
            net = synthetic.make_joiner(2, 'rotate')
        elif kind == 'general':
            net = synthetic.make_variant_joiner(9, **GENERAL)
        elif kind == 'general_rotate':
            net = synthetic.make_variant_joiner(9, posenc='rotate', **GENERAL)
        elif kind in ('all', 'none'):
            net = synthetic.make_joiner(1)
            with torch.no_grad():
                net.nerf.alpha_linear.bias.fill_(1e3 if kind == 'all' else -1e3)
        elif kind.startswith('plain_'):
            net = synthetic.make_variant_joiner(5, posenc=kind[6:], use_viewdirs=False)
        else:
            raise ValueError(kind)
        _NETS[kind] = net.to('cuda')
    return _NETS[kind]


def rays(R, S, seed=3):
    g = torch.Generator(device='cuda').manual_seed(seed)
    o = torch.randn((R, 3), device='cuda', generator=g) * 0.3
    d = torch.nn.functional.normalize(torch.randn((R, 3), device='cuda', generator=g), dim=-1)
    z = torch.sort(torch.rand((R, S), device='cuda', generator=g) * 3.0, dim=1).values.contiguous()
    return o, d, z


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ray_cases():
    """name -> (net, R, S, sigma_scale)"""
    c = {}
    for n in COUNTS:                                                   # S = 1: every sample a ray of its own
        c[f"posenc_{n}x1"] = ('posenc', n, 1, 1.3)
    for kind in ('rotate', 'general', 'general_rotate'):
        for n in (33, 513):
            c[f"{kind}_{n}x1"] = (kind, n, 1, 1.0)
    for kind in ('posenc', 'rotate', 'general'):
        for R, S in ((1, 256), (3, 256), (3, 96), (6, 96), (1, 40), (7, 40), (13, 40)):      # one ray per tile | tiles straddle rays
            c[f"{kind}_{R}x{S}"] = (kind, R, S, 0.7 if S == 96 else 1.0)
    for kind in ('all', 'none'):
        for R, S in ((257, 1), (13, 40)):
            c[f"{kind}_{R}x{S}"] = (kind, R, S, 1.0)
    # two tiles for every workgroup of a full grid and a ragged third for the first: a trunk tile after a head tile after a trunk tile
    for kind in ('posenc', 'all', 'general_rotate'):
        c[f"{kind}_full"] = (kind, FULL, 1, 1.0)
    return c


FULL = -1                                                              # R of the full-grid cases: known on the device only


def resolve(case):
    kind, R, S, scale = ray_cases()[case]
    return kind, (2 * TILE * cus() + 77 if R == FULL else R), S, scale


def point_cases():
    """the point form of the whole-network launch: name -> (net, n)"""
    return {f"{kind}_pts_{n}": (kind, n) for kind in ('posenc', 'general_rotate') for n in COUNTS}


def points(n, seed=5):
    o, d, z = rays(n, 1, seed)
    return (o + d * z).contiguous(), d


def whole_outputs():
    outs = {}
    with torch.no_grad():
        for name in ray_cases():
            kind, R, S, scale = resolve(name)
            o, d, z = rays(R, S)
            outs[name] = net_of(kind).forward_rays(o, d, z, precision='i8x3', sigma_scale=scale).cpu()
        for name, (kind, n) in point_cases().items():
            p, d = points(n)
            outs[name] = net_of(kind)(p, d, precision='i8x3').cpu()
    return outs


PLAIN_RAYS = (13, 40, 1.3)


def plain_outputs(kind, inputs=None):
    """the plain-head net on 513 points and on 13 rays x 40 samples -> dict of CPU tensors, inputs included"""
    if inputs is None:
        p, dv = points(COUNTS[-1])
        o, d, z = rays(*PLAIN_RAYS[:2])
        inputs = dict(p=p.cpu(), dv=dv.cpu(), o=o.cpu(), d=d.cpu(), z=z.cpu())
    dev = {k: v.cuda() for k, v in inputs.items()}
    net = net_of(kind)
    with torch.no_grad():
        out = dict(inputs)
        out['pts'] = net(dev['p'], dev['dv'], precision='i8x3').cpu()
        out['rays'] = net.forward_rays(dev['o'], dev['d'], dev['z'], precision='i8x3', sigma_scale=PLAIN_RAYS[2]).cpu()
    return out


if __name__ == "__main__":
    if sys.argv[1] == '--golden':
        import numpy as np
        np.savez_compressed(sys.argv[2], **{f"{kind}_{k}": v.numpy() for kind in ('plain_posenc', 'plain_rotate') for k, v in plain_outputs(kind).items()})
    else:
        torch.save(whole_outputs(), sys.argv[1])
