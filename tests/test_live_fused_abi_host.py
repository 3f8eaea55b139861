"""nm_mlp_live_fused_workspace_bytes and nm_mlp_forward_rays_fused on the host: the workspace arithmetic and the argument errors the entry
reports before it looks at the handle or enqueues anything -- no device needed (as tests/test_live_abi_host.py for the pair's entries)."""
import ctypes

from helpers import live_fused_tiles as T
from neuman_hip import _lib

NM_ERR_ARG = -1


def test_workspace_bytes():
    W = _lib.lib().nm_mlp_live_fused_workspace_bytes
    assert W(-1) == -1 and W(-(1 << 40)) == -1
    assert W(0) == 0
    # a list of 768 entries of 520 B per workgroup, a workgroup per 256-sample tile up to 256 of them, then two int32 each rounded up to 256 B
    assert W(1) == W(255) == W(256) == 768 * 520 + 256
    assert W(257) == 2 * 768 * 520 + 256
    assert W(32 * 256) == 32 * 768 * 520 + 256 and W(32 * 256 + 1) == 33 * 768 * 520 + 512
    assert W(256 * 256) == W(256 * 256 + 1) == W(640000 * 256) == W(1 << 40) == 256 * 768 * 520 + 2048
    for n in (1, 300, 5000, 70000, 1 << 22):
        assert W(n) == T.workspace_bytes(n)
    # a frame's pair workspace (one 2^21-sample chunk with every sample live) holds it: the fused launch is what a frame takes
    assert W(640000 * 256) <= _lib.lib().nm_mlp_forward_rays_live_workspace_bytes(640000, 256, 0)


def _call(L, handle, out, ws, ws_bytes, R=10, S=100, ptr=ctypes.c_void_p(4096)):
    return L.nm_mlp_forward_rays_fused(handle, ptr, ptr, ptr, R, S, 1.0, out, ws, ws_bytes, ctypes.c_void_p(0))


def test_argument_errors():
    L = _lib.lib()
    need = L.nm_mlp_live_fused_workspace_bytes(1000)
    good, ws = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    fake = ctypes.c_void_p(1 << 22)                                   # a handle that is never looked at: every call below fails before that
    assert _call(L, None, good, ws, need) == NM_ERR_ARG
    assert b"null handle" in L.nm_last_error()
    assert _call(L, fake, ctypes.c_void_p((1 << 20) + 4), ws, need) == NM_ERR_ARG
    assert b"16-byte aligned" in L.nm_last_error()
    assert _call(L, fake, good, ctypes.c_void_p((1 << 21) + 8), need) == NM_ERR_ARG
    assert b"16-byte aligned" in L.nm_last_error()
    assert _call(L, fake, good, ws, need - 1) == NM_ERR_ARG
    assert b"workspace of" in L.nm_last_error()
    assert _call(L, fake, good, None, need) == NM_ERR_ARG
    assert b"workspace of" in L.nm_last_error()
    assert _call(L, fake, good, ws, need, ptr=None) == NM_ERR_ARG
    assert b"null pointer" in L.nm_last_error()
    for R, S in ((-1, 100), (10, 0), (1 << 31, 1), (1 << 24, 128)):   # the list carries a record as int32: R * S < 2^31
        assert _call(L, fake, good, ws, 1 << 40, R=R, S=S) == NM_ERR_ARG
        assert b"bad sizes" in L.nm_last_error()
    # no rays: nothing to do, no workspace needed -- but still a handle
    assert _call(L, None, good, None, 0, R=0) == NM_ERR_ARG
    assert b"null handle" in L.nm_last_error()
