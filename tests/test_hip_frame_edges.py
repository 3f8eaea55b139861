"""-m gpu: the byte egress and the image metrics (ml-neuman_amd/csrc/frame.hip) through raw C calls at their value and sweep edges: every rounding
boundary of nm_frame_to_uint8, the non-finite and non-positive opacities of nm_layers_to_rgba8, nm_ssd_u8 past its grid cap, nm_ssim_u8 into its
third sweep and on images whose variances are exactly 0.  Outputs and workspaces lie between guard elements inside larger allocations.  The sizes
come from tests/helpers/loss_sizes.py, which tests/test_loss_host.py holds against the sources."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import frame as OF

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import loss_sizes as LS        # noqa: E402

pytestmark = pytest.mark.gpu

G = 64
F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
TINY = F32(1e-45)


def _lib():
    from neuman_hip import _lib as L
    return L


class Guarded:
    """n elements between two guards of G inside one allocation"""

    def __init__(self, n, dtype, fill, sentinel):
        self.n, self.sentinel = n, sentinel
        self.buf = torch.full((G + n + G,), sentinel, dtype=dtype, device='cuda')
        self.inner = self.buf[G:G + n]
        self.inner.fill_(fill)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + G * self.buf.element_size())

    def check(self, what):
        assert bool((self.buf[:G] == self.sentinel).all()) and bool((self.buf[G + self.n:] == self.sentinel).all()), (what, "a guard element changed")

    def numpy(self):
        return self.inner.cpu().numpy()


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device='cuda')


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def ok(rc, what):
    assert rc == 0, (what, _lib().lib().nm_last_error().decode())
    torch.cuda.synchronize()


# ---- nm_frame_to_uint8 -------------------------------------------------------------------------------------------------------------------
def to_uint8(x):
    x = np.ascontiguousarray(x, F32)
    src, dst = dev(x), Guarded(x.size, torch.uint8, 0x5A, 0xA5)
    ok(_lib().lib().nm_frame_to_uint8(ptr(src), x.size, dst.ptr, _lib().stream_ptr()), "nm_frame_to_uint8")
    dst.check("nm_frame_to_uint8")
    return dst.numpy()


def around(v):
    v = F32(v)
    return [np.nextafter(v, -INF), v, np.nextafter(v, INF)]


def test_to_uint8_at_every_rounding_boundary():
    """the three floats around (k + 0.5) / 255 -- where the byte steps -- and around k / 255, for every byte k, against the oracle's float64 rule"""
    x = np.asarray([f for k in range(256) for c in ((k + 0.5) / 255.0, k / 255.0) for f in around(c)], F32)
    got, want = to_uint8(x), OF.to_uint8(x)
    np.testing.assert_array_equal(got, want)
    assert set(want.tolist()) == set(range(256))                    # (the table does reach every byte)
    centre = got.reshape(256, 2, 3)[:, 1, :]
    assert (centre == np.arange(256)[:, None]).all()                # k / 255 and both neighbours give k
    steps = got.reshape(256, 2, 3)[:255, 0, :].astype(int)
    assert (np.diff(steps, axis=1) >= 0).all() and ((steps[:, 2] - steps[:, 0]) <= 1).all() and (steps[:, 0] >= np.arange(255)).all()


def test_to_uint8_on_zeros_denormals_infinities_and_nan():
    x = np.asarray([0.0, -0.0, TINY, -TINY, 1e-39, -1e-39, 1e-30, -1e-30, INF, -INF, np.nextafter(F32(1), F32(2)), 1.0, np.nextafter(F32(1), F32(0)), 3e38,
                    -3e38, NAN, -NAN], F32)
    want = [0, 0, 0, 0, 0, 0, 0, 0, 255, 0, 255, 255, 255, 255, 0, 0, 0]                  # +-inf: 255 and 0; a NaN gives 0 (the header's rule)
    assert to_uint8(x).tolist() == want
    finite = ~np.isnan(x)
    np.testing.assert_array_equal(OF.to_uint8(x[finite]), np.asarray(want, np.uint8)[finite])
    every_nan = np.asarray([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff], np.uint32).view(F32)   # quiet, signalling, payloads
    assert np.isnan(every_nan).all() and to_uint8(every_nan).tolist() == [0] * 6


@pytest.mark.parametrize("n", LS.BYTE_SIZES)
def test_to_uint8_sizes(n):
    x = np.random.default_rng(n).uniform(-0.1, 1.1, n).astype(F32)
    x[-1] = NAN if n > 1 else x[-1]
    x[0] = np.nextafter(F32(0.5 / 255), F32(1))
    want = OF.to_uint8(np.where(np.isnan(x), 0, x))
    np.testing.assert_array_equal(to_uint8(x), want)


# ---- nm_layers_to_rgba8 ------------------------------------------------------------------------------------------------------------------
ACC = np.asarray([0.0, -0.0, -1.0, TINY, 1e-30, 0.5, 1.0, np.nextafter(F32(1), F32(2)), 7.0, INF, NAN], F32)


def layer_table():
    """every opacity beside every colour of the issue's table -> (rgb [n,3], acc [n]); the three channels of a pixel take three different colours"""
    rows_rgb, rows_acc = [], []
    for a in ACC:
        colours = np.asarray([0.0, -0.0, -1.0, a, F32(2) * a, 1e30, INF, NAN], F32)
        for i in range(len(colours)):
            rows_rgb.append([colours[i], colours[(i + 1) % 8], colours[(i + 3) % 8]])
            rows_acc.append(a)
    return np.asarray(rows_rgb, F32), np.asarray(rows_acc, F32)


def rgba_rule(rgb, acc):
    """the header's rule in numpy: colour = the float32 quotient rgb / acc, 0 where acc <= 0, clamped to [0, 1]; alpha = clamp(acc, 0, 1); each
    by nm_frame_to_uint8's rule, a NaN giving 0 -> [n,4] uint8 in R, G, B, A order"""
    with np.errstate(all='ignore'):
        q = np.where((acc <= 0)[:, None], F32(0), rgb.astype(F32) / acc.astype(F32)[:, None]).astype(F32)
    ch = np.concatenate([q, acc[:, None]], 1)
    return OF.to_uint8(np.where(np.isnan(ch), 0.0, ch))


def layers_to_rgba8(rgb, acc):
    n = len(acc)
    out = Guarded(4 * n, torch.uint8, 0x5A, 0xA5)
    d_rgb, d_acc = dev(rgb), dev(acc)                               # (named, so that they outlive the call)
    ok(_lib().lib().nm_layers_to_rgba8(ptr(d_rgb), ptr(d_acc), n, out.ptr, _lib().stream_ptr()), "nm_layers_to_rgba8")
    out.check("nm_layers_to_rgba8")
    return out.numpy().reshape(n, 4)


def test_layers_to_rgba8_on_every_opacity_and_colour_edge():
    rgb, acc = layer_table()
    assert len(acc) == 88
    got, want = layers_to_rgba8(rgb, acc), rgba_rule(rgb, acc)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, [(rgb[i].tolist(), float(acc[i]), got[i].tolist(), want[i].tolist()) for i in bad[:8]]
    # what the rule comes to, spelled out where it matters: no colour without opacity, whatever the colour sums hold; a NaN anywhere gives 0
    nothing = acc <= 0
    assert nothing.sum() == 24 and not got[nothing].any()
    assert (got[np.isnan(acc)] == 0).all() and (got[:, :3][np.isnan(rgb)] == 0).all()
    tiny = (acc == TINY) | (acc == F32(1e-30))                      # the quotient of two tiny numbers is an ordinary number; an overflowing one saturates
    assert (got[tiny, 3] == 0).all() and (got[tiny, :3][rgb[tiny] == acc[tiny, None]] == 255).all() and (got[tiny, :3][rgb[tiny] == F32(1e30)] == 255).all()
    assert (got[acc == INF, :3][np.isfinite(rgb[acc == INF])] == 0).all() and (got[acc == INF, 3] == 255).all()


def test_layers_to_rgba8_byte_order():
    """R, G, B, A in memory, pixel after pixel"""
    rgb = np.asarray([[0.1, 0.2, 0.3], [0.25, 0.5, 0.125]], F32)
    acc = np.asarray([1.0, 0.5], F32)
    got = layers_to_rgba8(rgb, acc)
    assert got.tolist() == [[26, 51, 77, 255], [127, 255, 64, 127]] == rgba_rule(rgb, acc).tolist()
    assert got.reshape(-1).tolist() == [26, 51, 77, 255, 127, 255, 64, 127]


@pytest.mark.parametrize("n", LS.BYTE_SIZES)
def test_layers_to_rgba8_sizes(n):
    rng = np.random.default_rng(n)
    acc = rng.uniform(-0.1, 1.1, n).astype(F32)
    rgb = (rng.uniform(-0.1, 1.2, (n, 3)) * np.abs(acc)[:, None]).astype(F32)
    acc[-1] = 0.0
    rgb[-1] = 0.7
    np.testing.assert_array_equal(layers_to_rgba8(rgb, acc), rgba_rule(rgb, acc))


# ---- nm_ssd_u8 ---------------------------------------------------------------------------------------------------------------------------
def ssd(a, b, n):
    out = Guarded(1, torch.int64, -1, 0x5A5A5A5A)
    ok(_lib().lib().nm_ssd_u8(ptr(a), ptr(b), n, out.ptr, _lib().stream_ptr()), "nm_ssd_u8")
    out.check("nm_ssd_u8")
    return int(out.numpy()[0])


@pytest.fixture(scope="module")
def big_bytes():
    """two device arrays of the largest size, 255 and 0 throughout, shared by the nm_ssd_u8 tests (which use prefixes and put back what they change)"""
    n = LS.SSD_PAST_THE_CAP
    return torch.full((n,), 255, dtype=torch.uint8, device='cuda'), torch.zeros(n, dtype=torch.uint8, device='cuda')


def test_ssd_past_the_grid_cap(big_bytes):
    a, b = big_bytes
    n = LS.SSD_PAST_THE_CAP
    assert ssd(a, b, n) == 65025 * n == ssd(b, a, n)
    for m in LS.SSD_SIZES_CAP:                                      # the cap itself and one byte more
        assert ssd(a, b, m) == 65025 * m
    assert ssd(a, a, n) == 0


def test_ssd_sees_one_byte_at_each_end(big_bytes):
    a, _ = big_bytes
    n = LS.SSD_PAST_THE_CAP
    c = a.clone()
    c[0], c[n - 1] = 255 - 3, 255 - 200
    assert ssd(a, c, n) == 3 * 3 + 200 * 200 == ssd(c, a, n)
    assert ssd(a, c, n - 1) == 9 and ssd(a[1:], c[1:], n - 1) == 40000


@pytest.mark.parametrize("n", LS.SSD_SIZES_SMALL)
def test_ssd_small_sizes(n):
    rng = np.random.default_rng(n)
    a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    a[-1], b[-1] = 255, 0
    want = int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    assert ssd(dev(a), dev(b), n) == want


# ---- nm_ssim_u8 --------------------------------------------------------------------------------------------------------------------------
def ssim(pred, gt):
    H, W, Ch = pred.shape
    out = Guarded(1, torch.float64, float('nan'), -123456.0)
    ws = Guarded(LS.C.SSIM_MAX_BLOCKS, torch.float64, float('nan'), -123456.0)
    a, b = dev(pred), dev(gt)
    ok(_lib().lib().nm_ssim_u8(ptr(a), ptr(b), H, W, Ch, out.ptr, ws.ptr, _lib().stream_ptr()), "nm_ssim_u8")
    out.check("nm_ssim_u8: ssim")
    ws.check("nm_ssim_u8: workspace")
    return float(out.numpy()[0])


def textured(shape):
    """the pair tests/test_hip_frame.py draws"""
    rng = np.random.default_rng(shape[0])
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    base = (127 + 100 * np.sin(xx / 9.0)[..., None] * np.cos(yy / 13.0)[..., None] + rng.normal(0, 6, shape)).clip(0, 255)
    return (base + rng.normal(0, 9, shape)).clip(0, 255).astype(np.uint8), base.astype(np.uint8)


@pytest.mark.parametrize("shape", LS.SSIM_SHAPES)
def test_ssim_textured_pair_at_the_new_shapes(shape):
    pred, gt = textured(shape)
    got, ref = ssim(pred, gt), OF.ssim_uint8(pred, gt)
    print(f"[ssim] {shape}: device {got!r} oracle {ref!r} difference {abs(got - ref):.2e}")
    assert got == pytest.approx(ref, abs=1e-12), (got, ref)
    back = ssim(gt, pred)
    assert back == pytest.approx(got, abs=1e-15)                    # symmetric in its arguments (the existing test's bound)
    assert ssim(pred, gt) == got                                    # and the same bits on a second run
    assert ssim(gt, gt) == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize("shape", LS.SSIM_SHAPES)
def test_ssim_constant_images(shape):
    """the kernel's variances are exactly 0: equal constants give exactly 1, different ones the closed form of the luminance factor.  Every item
    is the same number, so what is left is the summation's own error: with one thread adding the 4096 partials in turn it reached 4.6e-15 at
    (254, 255) on the two largest shapes (up to 1e-13 for other constants); the tree of ssim_final_kernel keeps it below 5e-16"""
    C1 = (0.01 * 255.0) ** 2
    for a, b in ((0, 0), (255, 255), (77, 77), (0, 255), (3, 200), (254, 255)):
        x, y = np.full(shape, a, np.uint8), np.full(shape, b, np.uint8)
        got = ssim(x, y)
        if a == b:
            assert got == 1.0, (a, got)
        else:
            want = (2.0 * a * b + C1) / (a * a + b * b + C1)
            assert abs(got - want) <= 1e-15, (a, b, got, want)
            assert ssim(y, x) == got
    x, y = np.full(shape, 3, np.uint8), np.full(shape, 200, np.uint8)
    assert ssim(x, y) == pytest.approx(OF.ssim_uint8(x, y), abs=1e-12)


@pytest.mark.parametrize("shape", LS.SSIM_SHAPES)
def test_ssim_checkerboard_against_its_inverse(shape):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    board = np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[..., None], shape[2], 2)
    got, ref = ssim(board, 255 - board), OF.ssim_uint8(board, 255 - board)
    print(f"[ssim] checkerboard {shape}: device {got!r} oracle {ref!r} difference {abs(got - ref):.2e}")
    assert got < -0.5                                               # anticorrelated: strongly negative
    assert got == pytest.approx(ref, abs=1e-12), (got, ref)
    assert ssim(255 - board, board) == pytest.approx(got, abs=1e-15)
    assert ssim(board, board) == pytest.approx(1.0, abs=1e-15)
