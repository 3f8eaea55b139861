"""CPU check of the MFMA weight image (nm_mlp_pack) against the oracle MLP.

The packed image is consumed here by a numpy *emulation of the kernel's data flow* (csrc/mlp.hip): activations are
addressed by (chunk, element) k-slots exactly as the LDS arrays are, weights are read back from the fragment
positions a lane would load ([stage][block][k-step][hi|lo][lane][8]), and every layer output is re-slotted the way
the epilogue's ds_write_b128 does.  If the emulation reproduces the oracle network, the host packer, the k-slot
permutation (mlp_layout.h) and the stage table agree with each other -- without a GPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

from neuman_hip import _lib
from oracle import nerf_mlp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from mlp_emulate import b_off, emulate, emulate8, emulate_f16, slot_feature, w_off, w_off8  # noqa: E402


@pytest.mark.parametrize("seed", [0, 2])
def test_pack_matches_oracle(nets, seed):
    joiner, sd, spec = nets[seed]
    lib = _lib.lib()
    desc = _lib.MlpDesc(8, 256, 4, _lib.NM_PE_ROTATE if spec.mapping == 'rotate' else _lib.NM_PE_POSENC, 10, 4)
    nbytes = lib.nm_mlp_pack_bytes(ctypes.byref(desc))
    assert nbytes == w_off(11) + 4 * 2048 + 4 * b_off(11) + 4 * 24       # (+ the fp16 image's per-stage scale table)
    host = [p.detach().contiguous() for p in joiner.nerf.ordered_params()]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in host])
    img = ctypes.create_string_buffer(nbytes)
    _lib.check(lib.nm_mlp_pack(ctypes.byref(desc), arr, img), "nm_mlp_pack")
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1.5, 1.5, size=(64, 3)).astype(np.float32)
    dirs = rng.normal(size=(64, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    got = emulate(img.raw, pts, dirs, spec)
    ref = nerf_mlp.joiner_forward(sd, spec, pts, dirs)
    # weights carry 16 significant bits (bf16 hi + bf16 lo); activations are exact here
    assert np.abs(got[:, :3] - ref[:, :3]).max() < 2e-4
    assert np.abs(got[:, 3] - ref[:, 3]).max() < 2e-3 * max(1.0, np.abs(ref[:, 3]).max())


@pytest.mark.parametrize("seed", [0, 2, "big"])
def test_pack_f16_is_float32_class(nets, seed):
    """The split-fp16 image and data flow reproduce an f64 evaluation of the network ~10x closer than split bf16 does:
    float32-sgemm class (the oracle's own f32 evaluation is ~1e-6 from f64 on sigma)."""
    if seed == "big":                                  # weights far outside fp16's range at the default 2^8 scaling: the 'opaque' preset's
        from neuman_hip import synthetic                # alpha head (|w| up to 2500) and a hidden layer scaled by 1000
        from oracle.nerf_mlp import JoinerSpec
        import torch
        joiner = synthetic.make_joiner(1, preset='opaque')
        with torch.no_grad():
            joiner.nerf.pts_linears[2].weight.mul_(1e-3)           # tiny activations into ...
            joiner.nerf.pts_linears[2].bias.mul_(1e-3)
            joiner.nerf.pts_linears[3].weight.mul_(3000.0)         # ... a layer of huge weights (|w| up to 190: 2^8 would overflow)
            joiner.nerf.pts_linears[3].bias.mul_(3.0)
            joiner.nerf.pts_linears[4].weight.mul_(1.0 / 3)
        sd, spec = synthetic.state_numpy(joiner), JoinerSpec()
    else:
        joiner, sd, spec = nets[seed]
    lib = _lib.lib()
    desc = _lib.MlpDesc(8, 256, 4, _lib.NM_PE_ROTATE if spec.mapping == 'rotate' else _lib.NM_PE_POSENC, 10, 4)
    nbytes = lib.nm_mlp_pack_bytes(ctypes.byref(desc))
    host = [p.detach().contiguous() for p in joiner.nerf.ordered_params()]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in host])
    img = ctypes.create_string_buffer(nbytes)
    _lib.check(lib.nm_mlp_pack_f16(ctypes.byref(desc), arr, img), "nm_mlp_pack_f16")
    tab = np.frombuffer(img.raw, dtype=np.float32, offset=w_off(11) + 4 * 2048 + 4 * b_off(11), count=11)
    assert tab[1] == 1.0 / 256 and (np.log2(tab) == np.round(np.log2(tab))).all()
    if seed == "big":
        assert tab[3] > 1.0 / 256 and tab[8] > 1.0 / 256                         # those stages had to give up weight scale
    # the packer's own fp16 rounding is IEEE round-to-nearest-even (checked against numpy's)
    w0 = sd['nerf.pts_linears.1.weight']
    frag = np.frombuffer(img.raw, dtype=np.float16, count=1024, offset=w_off(1)).reshape(2, 2, 32, 8)   # block 0, step 0
    for g in range(2):
        for j in range(8):
            col = slot_feature(g, j)
            ws = (w0[:32, col] * np.float32(256)).astype(np.float32)                      # stage 1: k = 8 for every net here
            hi = ws.astype(np.float16)
            np.testing.assert_array_equal(frag[0, g, :, j], hi)
            np.testing.assert_array_equal(frag[1, g, :, j], (ws - hi.astype(np.float32)).astype(np.float16))
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1.5, 1.5, size=(64, 3)).astype(np.float32)
    dirs = rng.normal(size=(64, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    got = emulate_f16(img.raw, pts, dirs, spec)
    sd64 = {k: v.astype(np.float64) for k, v in sd.items()}
    x_pe = nerf_mlp.embed(pts, spec.mapping, *spec.pos).astype(np.float64)
    d_pe = nerf_mlp.embed(dirs, spec.mapping, *spec.dir).astype(np.float64)
    lin = lambda h, n: h @ sd64[f'nerf.{n}.weight'].T + sd64[f'nerf.{n}.bias']
    h = x_pe
    for i in range(8):
        h = np.maximum(lin(h, f'pts_linears.{i}'), 0)
        if i == 4:
            h = np.concatenate([x_pe, h], -1)
    sigma = lin(h, 'alpha_linear')[:, 0]
    rgb = lin(np.maximum(lin(np.concatenate([lin(h, 'feature_linear'), d_pe], -1), 'views_linears.0'), 0), 'rgb_linear')
    e_rgb, e_sig = np.abs(got[:, :3] - rgb).max(), np.abs(got[:, 3] - sigma).max()
    print(f"[pack f16] seed {seed}: vs f64 network  rgb {e_rgb:.2e}  sigma {e_sig:.2e}  (|sigma| max {np.abs(sigma).max():.2f})")
    assert e_rgb < 3e-6 * max(1.0, np.abs(rgb).max()) and e_sig < 1e-6 * max(1.0, np.abs(sigma).max())


def test_pack_rejects_unsupported_nets():
    lib = _lib.lib()
    for bad in [(6, 256, 4, 0, 10, 4), (8, 128, 4, 0, 10, 4), (8, 256, 4, 0, 11, 4), (8, 256, 4, 3, 10, 4)]:
        desc = _lib.MlpDesc(*bad)
        assert lib.nm_mlp_pack_bytes(ctypes.byref(desc)) == -1
        assert b"nm_mlp" in lib.nm_last_error()


@pytest.mark.parametrize("seed", [0, 2])
def test_pack_i8_matches_oracle(nets, seed):
    joiner, sd, spec = nets[seed]
    lib = _lib.lib()
    desc = _lib.MlpDesc(8, 256, 4, _lib.NM_PE_ROTATE if spec.mapping == 'rotate' else _lib.NM_PE_POSENC, 10, 4)
    nbytes = lib.nm_mlp_pack_i8_bytes(ctypes.byref(desc))
    assert nbytes == w_off8(11) + 4 * 2048 + 8 * b_off(11) + 64
    host = [p.detach().contiguous() for p in joiner.nerf.ordered_params()]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in host])
    img = ctypes.create_string_buffer(nbytes)
    _lib.check(lib.nm_mlp_pack_i8(ctypes.byref(desc), arr, img), "nm_mlp_pack_i8")
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1.5, 1.5, size=(64, 3)).astype(np.float32)
    dirs = rng.normal(size=(64, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    got = emulate8(img.raw, pts, dirs, spec)
    ref = nerf_mlp.joiner_forward(sd, spec, pts, dirs)
    print(np.abs(got[:, :3] - ref[:, :3]).max(), np.abs(got[:, 3] - ref[:, 3]).max())
    assert np.abs(got[:, :3] - ref[:, :3]).max() < 3e-4
    assert np.abs(got[:, 3] - ref[:, 3]).max() < 2e-3 * max(1.0, np.abs(ref[:, 3]).max())


def test_pack_i8s_stream_is_the_block_image_in_consumption_order(nets):
    """nm_mlp_pack_i8s (what the activation-stationary i8x3 kernel streams through its LDS ring, csrc/mlp_i8s.hip): the 2 KB k-steps of the
    nm_mlp_pack_i8 block image, each exactly once, in the order the kernel's flat ring-block table consumes them -- stage 0; the hidden
    stages with stage 5's four encoding steps per block BEHIND its eight i8 blocks; stage 8 with the alpha block FIRST; 9; 10 -- then zeros."""
    joiner, sd, spec = nets[0]
    lib = _lib.lib()
    desc = _lib.MlpDesc(8, 256, 4, _lib.NM_PE_POSENC, 10, 4)
    host = [p.detach().contiguous() for p in joiner.nerf.ordered_params()]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in host])
    img = ctypes.create_string_buffer(lib.nm_mlp_pack_i8_bytes(ctypes.byref(desc)))
    _lib.check(lib.nm_mlp_pack_i8(ctypes.byref(desc), arr, img), "nm_mlp_pack_i8")
    nbytes = lib.nm_mlp_pack_i8s_bytes(ctypes.byref(desc))
    assert nbytes == w_off8(11) + 4 * 2048
    stream = ctypes.create_string_buffer(nbytes)
    _lib.check(lib.nm_mlp_pack_i8s(ctypes.byref(desc), arr, stream), "nm_mlp_pack_i8s")
    steps = {0: (8, 4), 5: (8, 12), 8: (9, 8), 9: (4, 10), 10: (1, 4)}                     # stage -> (blocks, k-steps per block) of the block image
    frag = lambda st, nb, t: w_off8(st) + (nb * steps.get(st, (8, 8))[1] + t) * 2048      # noqa: E731
    order = [(0, nb, t) for nb in range(8) for t in range(4)]
    for st in range(1, 8):
        order += [(st, nb, t) for nb in range(8) for t in range(8)]
        if st == 5:
            order += [(5, nb, 8 + t) for nb in range(8) for t in range(4)]
    order += [(8, 8, t) for t in range(8)] + [(8, nb, t) for nb in range(8) for t in range(8)]
    order += [(9, nb, t) for nb in range(4) for t in range(10)] + [(10, 0, t) for t in range(4)]
    assert len(order) * 2048 == w_off8(11) and len(set(order)) == len(order)
    for k, (st, nb, t) in enumerate(order):
        assert stream.raw[k * 2048:(k + 1) * 2048] == img.raw[frag(st, nb, t):frag(st, nb, t) + 2048], (k, st, nb, t)
    assert stream.raw[w_off8(11):] == bytes(4 * 2048)
    # the kernel's ring-block table (block_steps in csrc/mlp_i8s.hip) covers exactly this stream
    table = [4] * 8 + [8] * 69 + [10] * 4 + [4]
    assert len(table) == 82 and sum(table) * 2048 == w_off8(11)


@pytest.mark.parametrize("mapping", ["posenc", "rotate"])
def test_pack_i8_plain_head_matches_oracle(mapping):
    """the use_viewdirs=False net (models/vanilla.py:116-117, 145): output_linear's four rows in the alpha block of the i8 image, stages 9 / 10 empty;
    and its stream for nerf_mlp_i8s_kernel<true>: the tile ends after that block, followed by the NEXT tile's blocks 0 and 1 padded to 8 steps --
    what the kernel's unchanged two-blocks-ahead ring copies while it multiplies blocks 67 and 68"""
    from neuman_hip import synthetic
    j = synthetic.make_variant_joiner(5, posenc=mapping, use_viewdirs=False)
    sd = synthetic.state_numpy(j)
    spec = nerf_mlp.JoinerSpec(mapping=mapping)
    lib = _lib.lib()
    desc = _lib.MlpDesc(8, 256, 4, _lib.NM_PE_ROTATE if mapping == 'rotate' else _lib.NM_PE_POSENC, 10, 4, 1)
    host = [p.detach().contiguous() for p in j.nerf.ordered_params()]
    assert len(host) == 18
    arr = (ctypes.c_void_p * 18)(*[t.data_ptr() for t in host])
    img = ctypes.create_string_buffer(lib.nm_mlp_pack_i8_bytes(ctypes.byref(desc)))
    _lib.check(lib.nm_mlp_pack_i8(ctypes.byref(desc), arr, img), "nm_mlp_pack_i8")
    rng = np.random.default_rng(7)
    pts = rng.uniform(-1.5, 1.5, size=(64, 3)).astype(np.float32)
    dirs = rng.normal(size=(64, 3)).astype(np.float32)
    got = emulate8(img.raw, pts, dirs, spec, plain=True)
    ref = nerf_mlp.joiner_forward(sd, spec, pts, dirs)
    s = 30 if mapping == 'rotate' else 1
    print(np.abs(got[:, :3] - ref[:, :3]).max(), np.abs(got[:, 3] - ref[:, 3]).max())
    assert np.abs(got[:, :3] - ref[:, :3]).max() < 3e-4 * s
    assert np.abs(got[:, 3] - ref[:, 3]).max() < 2e-3 * s * max(1.0, np.abs(ref[:, 3]).max())
    # ---- the stream
    nbytes = lib.nm_mlp_pack_i8s_bytes(ctypes.byref(desc))
    stream = ctypes.create_string_buffer(nbytes)
    _lib.check(lib.nm_mlp_pack_i8s(ctypes.byref(desc), arr, stream), "nm_mlp_pack_i8s")
    steps = {0: (8, 4), 5: (8, 12), 8: (9, 8), 9: (4, 10), 10: (1, 4)}
    frag = lambda st, nb, t: w_off8(st) + (nb * steps.get(st, (8, 8))[1] + t) * 2048      # noqa: E731
    order = [(0, nb, t) for nb in range(8) for t in range(4)]
    for st in range(1, 8):
        order += [(st, nb, t) for nb in range(8) for t in range(8)]
        if st == 5:
            order += [(5, nb, 8 + t) for nb in range(8) for t in range(4)]
    order += [(8, 8, t) for t in range(8)]
    assert len(order) == 520
    order += [(0, 0, t) for t in range(4)] + [None] * 4 + [(0, 1, t) for t in range(4)] + [None] * 4
    for k, e in enumerate(order):
        want = bytes(2048) if e is None else img.raw[frag(*e):frag(*e) + 2048]
        assert stream.raw[k * 2048:(k + 1) * 2048] == want, (k, e)
    assert stream.raw[len(order) * 2048:] == bytes(nbytes - len(order) * 2048)
    # the ring-block table the kernel walks (block_steps in csrc/mlp_i8s.hip): 69 blocks, then two 8-step look-aheads
    table = [4] * 8 + [8] * 61 + [8, 8]
    assert sum(table) == len(order)
