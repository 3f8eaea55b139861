"""Nets at the edges of the operand range, the float64 network they are judged against, and the bounds the suite states per arithmetic.

Every comparison of a network kernel with a high-precision reference elsewhere in the suite runs on torch's default initialisation: inside a layer
every row has the same scale, no bias is larger than its weights, and no layer is ever dead.  EDGE_NETS edits one such net at a time into what a
trained, pruned or diverged net looks like: a unit whose incoming weights are small against its bias, an outlier row or column, a dead layer, a
layer dead on part of every tile, a whole layer rescaled, a non-finite parameter.  Shared by tests/test_mlp_pack_edges.py (the CPU emulations of
the three weight images) and tests/test_hip_mlp_edges.py (the device kernels)."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from neuman_hip import _lib, synthetic
from oracle import nerf_mlp
from oracle.nerf_mlp import JoinerSpec


def embed64(x, mapping, min_freq, max_freq, n_freqs):
    """The encoding in float64.  posenc: float64 sin / cos of the float32 product x * band -- the bands are powers of two, so that product is the
    exact argument; rotate: the oracle's float32 encoding (its argument x.B^T is a rounded float32 sum: the factor 30 on a rotate net's bounds)."""
    if mapping != 'posenc':
        return nerf_mlp.embed(x, mapping, min_freq, max_freq, n_freqs).astype(np.float64)
    x = np.asarray(x, np.float32)
    out = [x.astype(np.float64)]
    for f in nerf_mlp.posenc_bands(min_freq, max_freq, n_freqs):
        a = (x * f).astype(np.float32).astype(np.float64)
        out += [np.sin(a), np.cos(a)]
    return np.concatenate(out, -1)


def f64_network(sd, spec, pts, dirs, plain=False, hidden=False):
    """The network in float64 on float32 weights -> (rgb [N,3], sigma [N]); hidden=True: (rgb, sigma, [the post-activation output of the eight
    trunk layers, feature, views]) -- the stages 0..9 of nm_mlp_forward_debug (0..7 for the plain head, use_viewdirs=False)."""
    sd64 = {k: v.astype(np.float64) for k, v in sd.items()}
    x_pe = embed64(pts, spec.mapping, *spec.pos)
    lin = lambda h, n: h @ sd64[f'nerf.{n}.weight'].T + sd64[f'nerf.{n}.bias']      # noqa: E731
    h, hs = x_pe, []
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(8):
            h = np.maximum(lin(h, f'pts_linears.{i}'), 0)                            # (np.maximum hands a NaN on, like torch.relu)
            hs.append(h)
            if i == 4:
                h = np.concatenate([x_pe, h], -1)
        if plain:
            out = lin(h, 'output_linear')
            rgb, sigma = out[:, :3], out[:, 3]
        else:
            d_pe = embed64(dirs, spec.mapping, *spec.dir)
            sigma = lin(h, 'alpha_linear')[:, 0]
            feature = lin(h, 'feature_linear')
            views = np.maximum(lin(np.concatenate([feature, d_pe], -1), 'views_linears.0'), 0)
            hs += [feature, views]
            rgb = lin(views, 'rgb_linear')
    return (rgb, sigma, hs) if hidden else (rgb, sigma)


# ---- the bounds against float64 the suite states for ordinary nets (tests/test_hip_mlp.py): (rgb, sigma per max(1, |sigma|max)) ----------------------
BOUNDS = {
    'fp32': (1e-4, 2e-4),          # test_stage_by_stage
    'bf16x3': (1e-4, 2e-4),        # test_stage_by_stage
    'fp16x3': (1e-4, 2e-4),        # test_fp16x3_operand_range
    'i8x3': (4e-4, 2e-3),          # test_i8x3_stage_by_stage
}
ROTATE_FACTOR = 30                 # error inherited from the rotate encoding's float32 argument (the same tests)
# per stage of nm_mlp_forward_debug, per max(1, |reference|max): test_stage_by_stage / test_i8x3_stage_by_stage
STAGE_BOUNDS = {'fp32': 2e-5, 'fp16x3': 2e-5, 'bf16x3': 6e-5, 'i8x3': 3e-4}


def bounds(prec, sigma64, mapping='posenc', scale=1.0):
    """(rgb bound, sigma bound) of one arithmetic on one set of points; `scale`: a test's own documented factor (0.5 for the emulations, the largest
    hidden activation for large coordinates)"""
    s = scale * (ROTATE_FACTOR if mapping == 'rotate' else 1)
    return BOUNDS[prec][0] * s, BOUNDS[prec][1] * s * max(1.0, float(np.abs(sigma64).max()))


# ---- the nets ---------------------------------------------------------------------------------------------------------------------------------------
BASES = {
    'posenc': lambda: (synthetic.make_joiner(1), JoinerSpec(), False),
    'rotate': lambda: (synthetic.make_joiner(2, 'rotate'), JoinerSpec(mapping='rotate'), False),
    'plain': lambda: (synthetic.make_variant_joiner(5, use_viewdirs=False), JoinerSpec(), True),
}
EdgeNet = namedtuple('EdgeNet', 'name kind base edit finite')
UNIT = 5                           # the edited unit: output feature 5 of its layer


def _layer(m, where):
    return {'p3': lambda: m.pts_linears[3], 'p6': lambda: m.pts_linears[6], 'skip5': lambda: m.pts_linears[5], 'feature': lambda: m.feature_linear,
            'views': lambda: m.views_linears[0], 'rgb': lambda: m.rgb_linear, 'out': lambda: m.output_linear}[where]()


def _small_unit(where, f):
    def edit(m):
        lin = _layer(m, where)
        lin.weight[UNIT].mul_(f)
        lin.bias[UNIT] = 0.5
    return edit


def _large_row(row):
    return lambda m: m.pts_linears[3].weight[row].mul_(1000.0)


def _large_col(m):
    m.pts_linears[3].weight[:, 9].mul_(1000.0)


def _dead_layer(m):
    m.pts_linears[2].bias.fill_(-100.0)


def _dead_part(m):
    """layer 0 fires only where x0 > ~0.6: dead and live samples share every 32-sample tile"""
    m.pts_linears[0].weight.mul_(0.01)
    m.pts_linears[0].weight[:, 0] = 4.0
    m.pts_linears[0].bias.fill_(-2.5)


def _scaled_layer(f):
    def edit(m):
        m.pts_linears[2].weight.mul_(f)
        m.pts_linears[2].bias.mul_(f)
        m.pts_linears[3].weight.mul_(1.0 / f)
    return edit


def _poison(where, what):
    def edit(m):
        lin = _layer(m, where)
        if what == 'nan_weight':
            lin.weight[1, 4] = float('nan')
        elif what == 'inf_weight':
            lin.weight[1, 4] = float('inf')
        else:
            lin.bias[1] = float('nan')
    return edit


def _table():
    t = []
    for where in ('p3', 'p6', 'feature', 'views', 'skip5'):
        for f in (1e-1, 1e-3, 1e-6, 0.0):
            t.append(EdgeNet(f'small_unit-{where}-x{f:g}', 'small_unit', 'posenc', _small_unit(where, f), True))
    # (slot_feature8: bit 2 of a feature's index is the lane half that holds it -- one outlier row in each half)
    t += [EdgeNet('large_unit-row9', 'large_unit', 'posenc', _large_row(9), True), EdgeNet('large_unit-row13', 'large_unit', 'posenc', _large_row(13), True),
          EdgeNet('large_unit-col9', 'large_unit', 'posenc', _large_col, True),
          EdgeNet('dead_layer', 'dead_layer', 'posenc', _dead_layer, True), EdgeNet('dead_part', 'dead_part', 'posenc', _dead_part, True),
          EdgeNet('scaled_layer-x0.001', 'scaled_layer', 'posenc', _scaled_layer(1e-3), True),
          EdgeNet('scaled_layer-x400', 'scaled_layer', 'posenc', _scaled_layer(400.0), True)]
    for base in ('rotate', 'plain'):
        t += [EdgeNet(f'small_unit-p3-x1e-06-{base}', 'small_unit', base, _small_unit('p3', 1e-6), True),
              EdgeNet(f'small_unit-p6-x0.001-{base}', 'small_unit', base, _small_unit('p6', 1e-3), True),
              EdgeNet(f'large_unit-row13-{base}', 'large_unit', base, _large_row(13), True),
              EdgeNet(f'dead_part-{base}', 'dead_part', base, _dead_part, True)]
    for where in ('p3', 'rgb'):
        for what in ('nan_weight', 'inf_weight', 'nan_bias'):
            t.append(EdgeNet(f'nonfinite-{what}-{where}', 'nonfinite', 'posenc', _poison(where, what), False))
    t.append(EdgeNet('nonfinite-nan_weight-out-plain', 'nonfinite', 'plain', _poison('out', 'nan_weight'), False))
    return t


EDGE_NETS = _table()
FINITE_NETS = [c for c in EDGE_NETS if c.finite]
NONFINITE_NETS = [c for c in EDGE_NETS if not c.finite]
# the tensor of NeRF.ordered_params() a `nonfinite` case poisons, as nm_last_error() names it
POISONED_TENSOR = {'p3': {'nan_weight': 'pts_linears.3.weight', 'inf_weight': 'pts_linears.3.weight', 'nan_bias': 'pts_linears.3.bias'},
                   'rgb': {'nan_weight': 'rgb_linear.weight', 'inf_weight': 'rgb_linear.weight', 'nan_bias': 'rgb_linear.bias'},
                   'out': {'nan_weight': 'output_linear.weight'}}


def poisoned_tensor(case):
    _, what, where = case.name.split('-')[:3]
    return POISONED_TENSOR[where][what]


def build(case):
    """-> (Joiner on the CPU with the edit applied, its float32 state as numpy, JoinerSpec, plain head?)"""
    j, spec, plain = BASES[case.base]()
    with torch.no_grad():
        case.edit(j.nerf)
    return j, synthetic.state_numpy(j), spec, plain


def sample_points(n, seed=7, lim=1.5, far=0):
    """n seeded points uniform in +-lim (the first `far` of them at +-1000 per coordinate) and unit directions"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-lim, lim, size=(n, 3)).astype(np.float32)
    dirs = rng.normal(size=(n, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    if far:
        pts[:far] = rng.choice([-1000.0, 1000.0], size=(far, 3)).astype(np.float32)
    return pts, dirs


# ---- the three host packers ---------------------------------------------------------------------------------------------------------------------------
PACKERS = {'bf16x3': ('nm_mlp_pack_bytes', 'nm_mlp_pack'), 'fp16x3': ('nm_mlp_pack_bytes', 'nm_mlp_pack_f16'), 'i8x3': ('nm_mlp_pack_i8_bytes', 'nm_mlp_pack_i8')}
FILL = 0xA5


def pack(joiner, spec, plain, which):
    """-> (return code, image bytes, nm_last_error()).  The buffer is pre-filled with FILL so that a packer that refuses can be seen to have written nothing."""
    lib = _lib.lib()
    desc = _lib.MlpDesc(8, 256, 4, _lib.NM_PE_ROTATE if spec.mapping == 'rotate' else _lib.NM_PE_POSENC, 10, 4, 1 if plain else 0)
    host = [p.detach().contiguous() for p in joiner.nerf.ordered_params()]
    arr = (ctypes.c_void_p * 24)(*([t.data_ptr() for t in host] + [None] * (24 - len(host))))
    nbytes = getattr(lib, PACKERS[which][0])(ctypes.byref(desc))
    img = ctypes.create_string_buffer(bytes([FILL]) * nbytes, nbytes)
    rc = getattr(lib, PACKERS[which][1])(ctypes.byref(desc), arr, img)
    return rc, img.raw, lib.nm_last_error().decode()


def emulation(which):
    import mlp_emulate
    return {'bf16x3': mlp_emulate.emulate, 'fp16x3': mlp_emulate.emulate_f16, 'i8x3': mlp_emulate.emulate8}[which]
