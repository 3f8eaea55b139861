"""CPU: the multi-person fused entries (include/neuman_hip.h: nm_merge_composite_lists_wide, nm_render_rays_multi, nm_render_rays_multi_live,
nm_render_rays_multi_workspace_floats) validate their arguments before any device work, name the entry that was called, and size the workspace
as the call lays it out."""
import ctypes
import os

import pytest

from neuman_hip import _lib, render_utils

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("nm_merge_composite_lists_wide", "nm_render_rays_multi", "nm_render_rays_multi_live", "nm_render_rays_multi_workspace_floats")
# nm_merge_composite_lists_wide's launch (csrc/merge_wide.hip): at most 4 waves (rays) per block and 4096 blocks; tests/test_hip_merge_wide.py sizes
# its grid-stride case from these
WIDE_MAX_WAVES = 4
WIDE_GRID_MAX_BLOCKS = 4096
P = 0x10000                                                       # a non-null, 16-byte aligned address nothing dereferences: validation comes first


def err():
    return _lib.lib().nm_last_error().decode()


def wide(k, z, raw, S, R=4, rows=None, ptr=P):
    arr = ctypes.c_void_p * max(len(z), 1)
    return _lib.lib().nm_merge_composite_lists_wide(k, arr(*z), arr(*raw), None if rows is None else arr(*rows), (ctypes.c_int * max(len(S), 1))(*S), R,
                                                    ptr, 1, ptr, ptr, ptr, None)


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "neuman_hip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and f"{name}(" in header, name


@pytest.mark.parametrize("k", [0, 33, -1])
def test_wide_merge_refuses_a_list_count_outside_1_to_32(k):
    n = max(k, 1)
    assert wide(k, [P] * n, [P] * n, [4] * n) == -1
    assert "nm_merge_composite_lists_wide" in err() and "32" in err()


def test_wide_merge_refuses_null_empty_and_misaligned_lists():
    assert wide(2, [P, None], [P, P], [4, 4]) == -1 and "nm_merge_composite_lists_wide: list 1 is null" in err()
    assert wide(2, [P, P], [P, None], [4, 4]) == -1 and "nm_merge_composite_lists_wide: list 1 is null" in err()
    assert wide(3, [P, P, P], [P, P, P], [4, 0, 4]) == -1 and "nm_merge_composite_lists_wide: list 1 is empty" in err()
    assert wide(2, [P, P], [P, P + 8], [4, 4]) == -1 and "nm_merge_composite_lists_wide" in err() and "aligned" in err()
    assert wide(2, [P, P], [P, P], [4, 4], ptr=None) == -1 and "nm_merge_composite_lists_wide: null pointer" in err()
    lib = _lib.lib()
    assert lib.nm_merge_composite_lists_wide(2, None, None, None, None, 0, None, 1, None, None, None, None) == -1 and "nm_merge_composite_lists_wide" in err()


def test_wide_merge_staging_limit_is_the_one_the_host_mirror_uses():
    """the limit is checked before the empty batch returns, so it can be read without a device: WIDE_MERGE_MAX_SAMPLES merged samples pass, one more
    is refused with the entry point and the limit in the message; 1 + 8 lists at 320 + 8 x 192 (BASELINE config 5 with eight actors) fit"""
    M = render_utils.WIDE_MERGE_MAX_SAMPLES
    assert wide(1, [None], [None], [M], R=0) == 0
    assert wide(1, [None], [None], [M + 1], R=0) == -1
    assert "nm_merge_composite_lists_wide" in err() and str(M) in err() and str(M + 1) in err()
    assert wide(32, [None] * 32, [None] * 32, [M // 32] * 32, R=0) == 0
    assert wide(32, [None] * 32, [None] * 32, [M // 32 + 1] * 32, R=0) == -1
    assert wide(9, [None] * 9, [None] * 9, [320] + [192] * 8, R=0) == 0
    assert 320 + 8 * 192 <= M
    assert render_utils.multi_merge_stages(8, 192, 128) and render_utils.multi_merge_stages(3, 192, 128)
    assert not render_utils.multi_merge_stages(4, 2048, 1024) and not render_utils.multi_merge_stages(32, 4, 4)
    assert render_utils.multi_merge_stages(31, 4, 4)


def test_launch_sizes_read_so_in_the_source():
    import re
    src = open(os.path.join(ROOT, "ml-neuman_amd", "csrc", "merge_wide.hip")).read()
    assert [int(x) for x in re.findall(r"constexpr int kWideMaxWaves = (\d+);", src)] == [WIDE_MAX_WAVES]
    assert re.findall(r"b > (\d+) \? (\d+) : b", src) == [(str(WIDE_GRID_MAX_BLOCKS),) * 2]
    # 14 merged samples (the grid-stride case of tests/test_hip_merge_wide.py) leave room for WIDE_MAX_WAVES waves in a block's 64 KiB
    assert (64 * 1024 - 912) // (512 + 16 * ((14 * 12 + 15) // 16)) >= WIDE_MAX_WAVES


def multi(live, R=4, S=16, N=16, Sh=16, A=1, ptr=P, actor_ptr=P, V=10):
    lib = _lib.lib()
    arr = ctypes.c_void_p * max(A, 1)
    acts = [arr(*[actor_ptr] * A) if A and actor_ptr else None for _ in range(4)]
    Vs = (ctypes.c_int * max(A, 1))(*[V] * A) if A and actor_ptr else None
    args = [ptr, ptr, A, acts[0], acts[1], acts[2], acts[3], Vs, 0.2, ptr, ptr, R, 0.1, 5.0, S, N, Sh, ptr, ptr, ptr, ptr, 1, 4, 3, 4, 3, ptr, ptr, ptr]
    if live:
        return lib.nm_render_rays_multi_live(*args, ptr, 1 << 40, 0, None)
    return lib.nm_render_rays_multi(*args, None)


@pytest.mark.parametrize("live", [False, True])
def test_render_rays_multi_validates_before_device_work_and_names_the_entry_called(live):
    who = "nm_render_rays_multi_live" if live else "nm_render_rays_multi"
    other = "nm_render_rays_multi:" if live else "nm_render_rays_multi_live"
    for kw in (dict(ptr=None), dict(actor_ptr=None), dict(Sh=1), dict(Sh=0), dict(S=0), dict(N=-1), dict(A=-1), dict(A=32), dict(R=-1), dict(V=0)):
        assert multi(live, **kw) == -1, kw
        assert who in err() and other not in err(), (kw, err())
    # shapes the merge cannot stage: refused up front, for the narrow (A <= 3) and the wide kernel alike
    assert multi(live, S=4000, N=4000, A=1) == -1 and who in err() and "merged samples" in err()
    assert multi(live, S=1024, N=1024, Sh=2048, A=4) == -1 and who in err() and str(render_utils.WIDE_MERGE_MAX_SAMPLES) in err()
    # the empty batch is an ordinary case, with or without actors, with null arrays
    assert multi(live, R=0, ptr=None) == 0 and multi(live, R=0, A=0, ptr=None, actor_ptr=None) == 0


def align4(n):
    return (n + 3) & ~3


def layout_floats(R, S, N, Sh, A):
    """the layout nm_render_rays_multi states (csrc/render.hip multi_layout), every sub-array 16-byte aligned"""
    lib = _lib.lib()
    Sb = S + N
    shared = [R, R, lib.nm_render_rays_bkg_workspace_floats(R, S, N), R * Sb * 4, R * Sb, R, R * 4, R, R, R, 4, lib.nm_compact_workspace_ints(R), R * 3, R * 3, R, R,
              lib.nm_render_rays_human_workspace_floats(R, Sh, 1), R]
    per_actor = [(R + 1) * Sh * 4, (R + 1) * Sh, R]
    return sum(align4(x) for x in shared) + A * sum(align4(x) for x in per_actor)


def test_multi_workspace_is_positive_monotone_and_equals_the_layout():
    f = _lib.lib().nm_render_rays_multi_workspace_floats
    base = dict(R=1000, S=16, N=16, Sh=16, A=3)
    assert f(*base.values()) > 0 and f(0, 1, 0, 2, 0) > 0
    for name, values in (("R", [0, 1, 2, 3, 5, 999, 1000, 1001, 4096, 1 << 20]), ("S", [1, 2, 3, 15, 16, 17, 192]), ("N", [0, 1, 2, 16, 17, 128]),
                         ("Sh", [2, 3, 4, 16, 17, 192]), ("A", [0, 1, 2, 3, 4, 5, 8, 31])):
        sizes = []
        for v in values:
            a = dict(base, **{name: v})
            sizes.append(f(a['R'], a['S'], a['N'], a['Sh'], a['A']))
            assert sizes[-1] == layout_floats(a['R'], a['S'], a['N'], a['Sh'], a['A']), (name, v)
        assert sizes == sorted(sizes), (name, sizes)
    assert f(1 << 20, 192, 128, 192, 8) * 4 > 1 << 32              # sizes past 2^32 bytes are computed in 64 bits


def test_fused_route_is_off_by_default_and_the_switch_is_the_documented_one():
    src = open(os.path.join(ROOT, "ml-neuman_amd", "neuman_hip", "render_utils.py")).read()
    assert 'MULTI_FUSED = os.environ.get("NEUMAN_MULTI_FUSED", "0") == "1"' in src
    assert 'FUSED_MULTI_RAYS = int(os.environ.get("NEUMAN_FUSED_MULTI_RAYS"' in src
    if "NEUMAN_MULTI_FUSED" not in os.environ:
        assert render_utils.MULTI_FUSED is False
