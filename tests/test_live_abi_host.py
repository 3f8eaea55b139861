"""The nm_mlp_*_live entries on the host: the workspace arithmetic of nm_mlp_live_workspace_bytes and the argument errors every entry reports
before it looks at the handle or enqueues anything -- no device needed."""
import ctypes

import pytest

from neuman_hip import _lib

NM_ERR_ARG = -1
CHUNK = 1 << 21                      # NM_LIVE_CHUNK_SAMPLES
I8, F16 = _lib.NM_PREC_I8X3, _lib.NM_PREC_FP16X3


def counters(n_max, chunk):
    """the bytes behind the list: the list's own counter (256) and one int32 per piece, for at most 2 ceil(n_max / chunk) + 2 pieces (a piece of
    whole rays is more than half of chunk_samples), rounded up to 256"""
    pieces = 2 * ((n_max + chunk - 1) // chunk) + 2
    return 256 + (pieces * 4 + 255) // 256 * 256


def test_workspace_bytes():
    W = _lib.lib().nm_mlp_live_workspace_bytes
    assert W(-1, 0) == -1 and W(-5, 256) == -1
    assert W(0, 0) == counters(0, CHUNK)
    # one piece with every entry live: 520 B per entry, the piece = min(n_max, chunk) rounded up to 256
    assert W(1, 0) == 256 * 520 + counters(1, CHUNK)
    assert W(256, 0) == 256 * 520 + counters(256, CHUNK)
    assert W(257, 0) == 512 * 520 + counters(257, CHUNK)
    assert W(703, 300) == 512 * 520 + counters(703, 300)             # the piece (300), not n_max, is what is rounded
    assert W(100, 300) == 256 * 520 + counters(100, 300)             # n_max < chunk
    assert W(10 * CHUNK, 0) == W(10 * CHUNK, -3) == W(10 * CHUNK, CHUNK) == CHUNK * 520 + counters(10 * CHUNK, CHUNK)
    assert W(1 << 40, 1000) == 1024 * 520 + counters(1 << 40, 1000)  # 64-bit sizes


def _calls(L, handle, out, ws, ws_bytes, n, prec):
    z = ctypes.c_void_p(0)
    a = ctypes.c_void_p(4096)                                          # never dereferenced: every call below fails before that
    return {
        'nm_mlp_forward_live': lambda: L.nm_mlp_forward_live(handle, a, a, n, prec, 1.0, out, ws, ws_bytes, 0, z),
        'nm_mlp_forward_listed_live': lambda: L.nm_mlp_forward_listed_live(handle, a, a, n, a, None, n, prec, 1.0, out, ws, ws_bytes, 0, z),
        'nm_mlp_forward_samples_live': lambda: L.nm_mlp_forward_samples_live(handle, a, a, a, n, 1, a, None, n, prec, 1.0, out, ws, ws_bytes, 0, z),
        'nm_mlp_forward_ray_chunk_live': lambda: L.nm_mlp_forward_ray_chunk_live(handle, a, a, a, 1, a, None, n, 0, 1, prec, 1.0, out, ws, ws_bytes, 0, z),
    }


ENTRIES = ['nm_mlp_forward_live', 'nm_mlp_forward_listed_live', 'nm_mlp_forward_samples_live', 'nm_mlp_forward_ray_chunk_live']


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors(entry):
    L = _lib.lib()
    n = 1000
    need = L.nm_mlp_live_workspace_bytes(n, 0)
    good, ws = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    fake = ctypes.c_void_p(1 << 22)                                   # a handle that is never looked at
    # a null handle
    assert _calls(L, None, good, ws, need, n, I8)[entry]() == NM_ERR_ARG
    assert b"null handle" in L.nm_last_error()
    # a misaligned out, a misaligned workspace
    assert _calls(L, fake, ctypes.c_void_p((1 << 20) + 4), ws, need, n, I8)[entry]() == NM_ERR_ARG
    assert b"16-byte aligned" in L.nm_last_error()
    assert _calls(L, fake, good, ctypes.c_void_p((1 << 21) + 8), need, n, I8)[entry]() == NM_ERR_ARG
    assert b"16-byte aligned" in L.nm_last_error()
    # a short workspace, no workspace
    assert _calls(L, fake, good, ws, need - 1, n, I8)[entry]() == NM_ERR_ARG
    assert b"workspace of" in L.nm_last_error()
    assert _calls(L, fake, good, None, need, n, I8)[entry]() == NM_ERR_ARG
    # another precision needs no workspace: the call gets as far as the handle
    assert _calls(L, None, good, None, 0, n, F16)[entry]() == NM_ERR_ARG
    assert b"null handle" in L.nm_last_error()
