"""CPU check of the two stream cuts behind nm_mlp_forward_rays_live (nm_mlp_pack_i8s_live): the trunk launch walks ring blocks 0..68 of
nm_mlp_pack_i8s' consumption-order stream, the head launch blocks 69..81 -- byte for byte the same k-steps, so the pair multiplies exactly the
weights the whole-network launch does."""
import ctypes

import pytest

from neuman_hip import _lib, synthetic

STEP = 2048
TRUNK_STEPS, HEAD_STEPS = 520, 108          # 8 x 4 + 7 x 8 x 8 + 8 x 4 + 8 (through the alpha block) | 8 x 8 + 4 x 10 + 4


def _streams(joiner, mapping):
    lib = _lib.lib()
    desc = _lib.MlpDesc(8, 256, 4, _lib.NM_PE_ROTATE if mapping == 'rotate' else _lib.NM_PE_POSENC, 10, 4)
    host = [p.detach().contiguous() for p in joiner.nerf.ordered_params()]
    arr = (ctypes.c_void_p * 24)(*[t.data_ptr() for t in host])
    whole = ctypes.create_string_buffer(lib.nm_mlp_pack_i8s_bytes(ctypes.byref(desc)))
    _lib.check(lib.nm_mlp_pack_i8s(ctypes.byref(desc), arr, whole), "nm_mlp_pack_i8s")
    nt, nh = lib.nm_mlp_pack_i8s_trunk_bytes(ctypes.byref(desc)), lib.nm_mlp_pack_i8s_head_bytes(ctypes.byref(desc))
    trunk, head = ctypes.create_string_buffer(nt), ctypes.create_string_buffer(nh)
    _lib.check(lib.nm_mlp_pack_i8s_live(ctypes.byref(desc), arr, trunk, head), "nm_mlp_pack_i8s_live")
    return whole.raw, trunk.raw, head.raw


@pytest.mark.parametrize("seed,mapping,preset", [(1, 'posenc', None), (2, 'rotate', None), (0, 'posenc', 'opaque')])
def test_cuts_are_the_whole_stream(seed, mapping, preset):
    joiner = synthetic.make_joiner(seed, mapping, preset=preset) if preset else synthetic.make_joiner(seed, mapping)
    whole, trunk, head = _streams(joiner, mapping)
    assert len(whole) == (TRUNK_STEPS + HEAD_STEPS + 4) * STEP
    assert len(trunk) == (TRUNK_STEPS + 16 + 4) * STEP and len(head) == (HEAD_STEPS + 4) * STEP
    assert trunk[:TRUNK_STEPS * STEP] == whole[:TRUNK_STEPS * STEP]
    assert head[:HEAD_STEPS * STEP] == whole[TRUNK_STEPS * STEP:(TRUNK_STEPS + HEAD_STEPS) * STEP]
    assert head[HEAD_STEPS * STEP:] == bytes(4 * STEP)
    # the trunk's ring looks two blocks ahead as if the feature blocks (8 steps each) followed: the NEXT tile's blocks 0 and 1 (4 steps each)
    # stand there, each padded with zeros to 8 steps; then zeros
    pad = trunk[TRUNK_STEPS * STEP:]
    for nb in range(2):
        assert pad[nb * 8 * STEP:(nb * 8 + 4) * STEP] == whole[nb * 4 * STEP:(nb + 1) * 4 * STEP], nb
        assert pad[(nb * 8 + 4) * STEP:(nb + 1) * 8 * STEP] == bytes(4 * STEP), nb
    assert pad[16 * STEP:] == bytes(4 * STEP)


def test_plain_head_net_is_refused():
    lib = _lib.lib()
    desc = _lib.MlpDesc(8, 256, 4, _lib.NM_PE_POSENC, 10, 4, 1)
    assert lib.nm_mlp_pack_i8s_trunk_bytes(ctypes.byref(desc)) == -1 and lib.nm_mlp_pack_i8s_head_bytes(ctypes.byref(desc)) == -1
    j = synthetic.make_variant_joiner(5, posenc='posenc', use_viewdirs=False)
    host = [p.detach().contiguous() for p in j.nerf.ordered_params()]
    arr = (ctypes.c_void_p * 24)(*([t.data_ptr() for t in host] + [None] * (24 - len(host))))
    buf = ctypes.create_string_buffer(16)
    assert lib.nm_mlp_pack_i8s_live(ctypes.byref(desc), arr, buf, buf) == -1
    assert b"plain-head" in lib.nm_last_error()
