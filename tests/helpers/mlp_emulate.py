"""numpy emulations of the data flow of the three MFMA weight images (nm_mlp_pack: split bf16, csrc/mlp.hip; nm_mlp_pack_f16: split fp16;
nm_mlp_pack_i8: per-row-scaled int16 as two int8 limbs, csrc/mlp_i8s.hip / mlp_i8as.h) and the layout helpers they share.  Activations are
addressed by (chunk, element) k-slots exactly as the LDS arrays are, weights are read back from the fragment positions a lane would load, and every
layer output is re-slotted the way the epilogue does.  Used by tests/test_mlp_pack.py (ordinary nets), tests/test_mlp_pack_edges.py and
tests/test_hip_mlp_edges.py (nets at the edges of the operand range)."""
import numpy as np

from oracle import nerf_mlp

STAGES = {0: (8, 4, 4), 5: (8, 20, 4), 8: (9, 16, 0), 9: (4, 18, 2), 10: (1, 8, 0)}  # nblk, steps, pe_steps


def shape(s):
    return STAGES.get(s, (8, 16, 0))


def w_off(s):
    return sum(shape(i)[0] * shape(i)[1] * 2048 for i in range(s))


def b_off(s):
    return sum(shape(i)[0] * 32 for i in range(s))


def slot_feature(c, e):
    return 32 * (c >> 2) + 8 * (2 * ((c >> 1) & 1) + (e >> 2)) + 4 * (c & 1) + (e & 3)


def bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def stage_weights(img, s):
    """W_eff [nblk*32, steps*16] = hi + lo, columns ordered by k-slot (step, lane half g, element j)."""
    nblk, steps, _ = shape(s)
    frag = np.frombuffer(img, dtype=np.uint16, count=nblk * steps * 1024, offset=w_off(s)).reshape(nblk, steps, 2, 64, 8)
    w = bf16_to_f32(frag[:, :, 0]) + bf16_to_f32(frag[:, :, 1])          # [nblk, steps, lane, j]
    w = w.reshape(nblk, steps, 2, 32, 8)                                    # lane = g*32 + row
    return w.transpose(0, 3, 1, 2, 4).reshape(nblk * 32, steps * 16)       # [n, (t, g, j)]


def slots_from_features(h, nchunks):
    """[N, F] natural features -> [N, nchunks*8] in k-slot order (what the epilogue leaves in LDS)."""
    idx = np.array([slot_feature(c, e) for c in range(nchunks) for e in range(8)])
    return h[:, idx]


def emulate(img, pts, dirs, spec, plain=False):
    total_w = w_off(11)
    bias = np.frombuffer(img, dtype=np.float32, offset=total_w + 4 * 2048)
    x_pe = nerf_mlp.embed(pts, spec.mapping, *spec.pos)
    d_pe = nerf_mlp.embed(dirs, spec.mapping, *spec.dir)
    P = np.zeros((pts.shape[0], 64), np.float32)
    P[:, :x_pe.shape[1]] = x_pe
    Pd = np.zeros((pts.shape[0], 32), np.float32)
    Pd[:, :d_pe.shape[1]] = d_pe

    def run(s, act_slots, n_out):
        W = stage_weights(img, s)
        assert W.shape[1] == act_slots.shape[1], (s, W.shape, act_slots.shape)
        b = bias[b_off(s):b_off(s) + W.shape[0]]
        return (act_slots.astype(np.float64) @ W.T.astype(np.float64) + b)[:, :n_out].astype(np.float32)

    h = np.maximum(run(0, P, 256), 0)
    for s in range(1, 8):
        a = slots_from_features(h, 32)
        if s == 5:
            a = np.concatenate([P, a], 1)                                   # PE steps first (mlp.hip stage loop)
        h = np.maximum(run(s, a, 256), 0)
    o8 = run(8, slots_from_features(h, 32), 288)
    if plain:                                                           # output_linear's (r, g, b, sigma) stand where the alpha row is otherwise
        assert np.abs(o8[:, :256]).max() == 0 and np.abs(o8[:, 260:]).max() == 0
        return o8[:, 256:260]
    feature, sigma = o8[:, :256], o8[:, 256]
    assert np.abs(o8[:, 257:]).max() == 0
    v = np.maximum(run(9, np.concatenate([slots_from_features(feature, 32), Pd], 1), 128), 0)   # h steps first, then d_pe
    o10 = run(10, slots_from_features(v, 16), 32)
    assert np.abs(o10[:, 3:]).max() == 0
    return np.concatenate([o10[:, :3], sigma[:, None]], 1)

def emulate_f16(img, pts, dirs, spec, plain=False):
    """The NM_PREC_FP16X3 data flow (csrc/mlp.hip): fp16 hi/lo parts of W * 2^k_s from the image, activations and encodings
    split into fp16 parts of X * 2^5, the three kept products wh.xh + wh.xl + wl.xh accumulated wide, biases * 2^(k_s+5),
    the epilogue's exact * 2^-k_s and the outputs' exact * 2^-(k_s+5) (per-stage factors read from the image)."""
    total_w = w_off(11)
    bias = np.frombuffer(img, dtype=np.float32, offset=total_w + 4 * 2048)
    acc2out = bias[b_off(11) + 11:b_off(11) + 22]
    assert np.array_equal(bias[b_off(11):b_off(11) + 11] / 32, acc2out)

    def parts(s):
        nblk, steps, _ = shape(s)
        frag = np.frombuffer(img, dtype=np.float16, count=nblk * steps * 1024, offset=w_off(s)).reshape(nblk, steps, 2, 2, 32, 8)
        f = frag.astype(np.float64).transpose(2, 0, 4, 1, 3, 5).reshape(2, nblk * 32, steps * 16)     # [hi|lo][n][(t, g, j)]
        return f[0], f[1]

    def split(x):                                                                                       # X * 32 -> fp16 hi, lo
        xs = np.clip((x * np.float32(32.0)).astype(np.float32), -65504, 65504)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
        return hi.astype(np.float64), lo.astype(np.float64)

    def run(s, act_slots, n_out):
        wh, wl = parts(s)
        xh, xl = split(act_slots)
        b = bias[b_off(s):b_off(s) + wh.shape[0]].astype(np.float64)
        return ((xh @ wh.T + xl @ wh.T + xh @ wl.T) + b)[:, :n_out].astype(np.float32)                  # Y * 2^13

    x_pe = nerf_mlp.embed(pts, spec.mapping, *spec.pos)
    d_pe = nerf_mlp.embed(dirs, spec.mapping, *spec.dir)
    P = np.zeros((pts.shape[0], 64), np.float32)
    P[:, :x_pe.shape[1]] = x_pe
    Pd = np.zeros((pts.shape[0], 32), np.float32)
    Pd[:, :d_pe.shape[1]] = d_pe
    # (the kernel multiplies by 2^-k_s and stores X * 2^5; here X itself: one exact multiplication either way)
    h = np.maximum(run(0, P, 256), 0) * acc2out[0]
    for s in range(1, 8):
        a = slots_from_features(h, 32)
        if s == 5:
            a = np.concatenate([P, a], 1)
        h = np.maximum(run(s, a, 256), 0) * acc2out[s]
    o8 = run(8, slots_from_features(h, 32), 288) * acc2out[8]
    if plain:
        return o8[:, 256:260]
    feature, sigma = o8[:, :256], o8[:, 256]
    v = np.maximum(run(9, np.concatenate([slots_from_features(feature, 32), Pd], 1), 128), 0) * acc2out[9]
    o10 = run(10, slots_from_features(v, 16), 32) * acc2out[10]
    return np.concatenate([o10[:, :3], sigma[:, None]], 1)

# ---------------------------------------------------------------------------------------------------------------------
# NM_PREC_I8X3 image: per-row-scaled int16 as two int8 limbs (mlp_layout.h), emulated with exact integer arithmetic
# ---------------------------------------------------------------------------------------------------------------------
STAGES8 = {0: (8, 0, 4), 5: (8, 8, 4), 8: (9, 8, 0), 9: (4, 8, 2), 10: (1, 4, 0)}   # nblk, i8 steps (32 k), bf steps (16 k)


def shape8(s):
    return STAGES8.get(s, (8, 8, 0))


def w_off8(s):
    return sum(shape8(i)[0] * (shape8(i)[1] + shape8(i)[2]) * 2048 for i in range(s))


def slot_feature8(c, e):
    return 32 * (c >> 1) + (e & 3) + 8 * (e >> 2) + 4 * (c & 1)


def stage_weights8(img, s):
    """(Wq [nblk*32, i8steps*32] int64 in k-slot order, Wpe [nblk*32, bfsteps*16] f32 in k-slot order)."""
    nblk, n8, nbf = shape8(s)
    per = n8 + nbf
    raw = np.frombuffer(img, dtype=np.uint8, count=nblk * per * 2048, offset=w_off8(s)).reshape(nblk, per, 2048)
    wq = np.zeros((nblk * 32, n8 * 32), np.int64)
    if n8:
        limbs = raw[:, :n8].copy().view(np.int8).reshape(nblk, n8, 2, 2, 32, 16).astype(np.int64)    # [nb, t, limb, g, r, e]
        q = 256 * limbs[:, :, 0] + limbs[:, :, 1]                                                      # [nb, t, g, r, e]
        wq = q.transpose(0, 3, 1, 2, 4).reshape(nblk * 32, n8 * 32)                                     # [n, (t, g, e)]
    wpe = np.zeros((nblk * 32, nbf * 16), np.float32)
    if nbf:
        frag = raw[:, n8:].copy().view(np.uint16).reshape(nblk, nbf, 2, 2, 32, 8)                      # [nb, t, hi|lo, g, r, j]
        w = bf16_to_f32(frag[:, :, 0]) + bf16_to_f32(frag[:, :, 1])
        wpe = w.transpose(0, 3, 1, 2, 4).reshape(nblk * 32, nbf * 16)
    return wq, wpe


def quant_rows(h):
    """X = rint(x / sx), sx = max|x| / 32639 per row, split into balanced int8 limbs."""
    m = np.abs(h).max(axis=1, keepdims=True)
    s = np.where(m > 0, m / 32639.0, 1.0).astype(np.float32)
    q = np.rint(h / s).astype(np.int64)
    lo = ((q + 128) & 255) - 128
    hi = (q - lo) >> 8
    assert np.abs(hi).max() <= 128 and np.abs(lo).max() <= 128 and (256 * hi + lo == q).all()
    return s, hi, lo


def emulate8(img, pts, dirs, spec, plain=False, hidden=None):
    """hidden: a list that receives the post-activation output of every stage in true units (stages 0..9 of nm_mlp_forward_debug)"""
    tail = w_off8(11) + 4 * 2048
    nb_f = b_off(11)
    # hidden state of stage s is kept in per-feature units: true value = stored * units[s][n] (mlp_host.hip pack_image8);
    # biases and the encoding rows are stored in those units, kappa[s] is the stage's scalar folded into the row scale
    units = np.frombuffer(img, dtype=np.float32, count=nb_f, offset=tail)
    bias = np.frombuffer(img, dtype=np.float32, count=nb_f, offset=tail + 4 * nb_f)
    kappa = np.frombuffer(img, dtype=np.float32, count=16, offset=tail + 8 * nb_f)
    x_pe = nerf_mlp.embed(pts, spec.mapping, *spec.pos)
    d_pe = nerf_mlp.embed(dirs, spec.mapping, *spec.dir)
    P = np.zeros((pts.shape[0], 64), np.float32)
    P[:, :x_pe.shape[1]] = x_pe
    Pd = np.zeros((pts.shape[0], 32), np.float32)
    Pd[:, :d_pe.shape[1]] = d_pe

    def run(s, h, pe, n_out):
        wq, wpe = stage_weights8(img, s)
        nrow = wq.shape[0]
        out = np.zeros((pts.shape[0], nrow), np.float64)
        if h is not None:
            nchunks = wq.shape[1] // 16
            idx = np.array([slot_feature8(c, e) for c in range(nchunks) for e in range(16)])
            sx, xh, xl = quant_rows(h[:, idx])
            wl = ((wq + 128) & 255) - 128
            wh = (wq - wl) >> 8
            t = 65536 * (xh @ wh.T) + 256 * (xh @ wl.T + xl @ wh.T)            # the xl*wl term is dropped, like the kernel
            assert np.abs(t // 256).max() < 2 ** 31                             # the kernel combines (hh << 8) + cross in int32
            out += t * (sx * kappa[s]).astype(np.float64)
        if pe is not None:
            out += pe.astype(np.float64) @ wpe.T.astype(np.float64)
        return (out + bias[b_off(s):b_off(s) + nrow])[:, :n_out].astype(np.float32)

    keep = (lambda s, x: hidden.append(x * units[b_off(s):b_off(s) + x.shape[1]])) if hidden is not None else (lambda s, x: None)
    h = np.maximum(run(0, None, P, 256), 0)
    keep(0, h)
    for s in range(1, 8):
        h = np.maximum(run(s, h, P if s == 5 else None, 256), 0)
        keep(s, h)
    o8 = run(8, h, None, 288)
    if plain:                                                           # output_linear's (r, g, b, sigma) stand where the alpha row is otherwise
        assert np.abs(o8[:, :256]).max() == 0 and np.abs(o8[:, 260:]).max() == 0
        return o8[:, 256:260] * units[b_off(8) + 256:b_off(8) + 260]
    feature, sigma = o8[:, :256], o8[:, 256] * units[b_off(8) + 256]
    keep(8, feature)
    v = np.maximum(run(9, feature, Pd, 128), 0)
    keep(9, v)
    o10 = run(10, v, None, 32) * units[b_off(10):b_off(10) + 32]
    assert all(0 < units[b_off(s):b_off(s + 1)].min() and units[b_off(s):b_off(s + 1)].max() <= 1.0 for s in range(11))
    return np.concatenate([o10[:, :3], sigma[:, None]], 1)
