"""-m gpu: the N > 1 code path with real kernels under a process group, as far as a one-GPU box can execute it
(the 1/2/4/8-GPU curve itself is the driver's to measure):

* the RCCL gather collective on an initialised "nccl" group of ONE rank (render_sharded with force_collective), device tensors;
* bench.py's exact timed step through that group (`--dist`);
* two processes sharing the GPU, each rendering its own interleaved tiles on the device, frame assembled through gloo --
  bit-identical to the unsharded frame;
* the four reference-named frame drivers (render_vanilla, render_smpl_nerf, render_hybrid_nerf = BASELINE config 4,
  render_hybrid_nerf_multi_persons = config 5) called under a process group: both ways above, bit-identical frames on rank 0,
  None on the other rank.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def env_for(rank, world, port):
    e = dict(os.environ)
    e.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
             HSA_ENABLE_IPC_MODE_LEGACY="0")
    return e


def last_json(text):
    return json.loads([ln for ln in text.strip().splitlines() if ln.startswith("{")][-1])


def test_rccl_gather_on_a_group_of_one_rank():
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "dist_frame_check.py"), "nccl"], env=env_for(0, 1, free_port()),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r.stdout)
    print(out)
    assert out["bit_identical"] and out["finite"] and out["tiles"] == 24


def test_bench_step_through_an_initialised_nccl_group():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--dist", "--timed-only"],
                       env=env_for(0, 1, free_port()), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = last_json(r.stdout)
    print({k: line[k] for k in ("value", "ms_per_step", "n_gpus")})
    assert line["n_gpus"] == 1 and line["value"] > 1e5 and line["roofline"]["launches"] == 1


def test_two_ranks_share_the_gpu_and_assemble_real_tiles_over_gloo():
    port = free_port()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "helpers", "dist_frame_check.py"), "gloo"], env=env_for(r, 2, port),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    out = last_json(outs[0][0])
    print(out)
    assert out["bit_identical"] and out["finite"] and out["world"] == 2


def test_bench_self_launch_paths_on_a_one_gpu_box():
    """`python bench.py --gpus 2` started by hand on this one-GPU box prints ONE JSON error line (exit code 2) instead of dying on an
    assertion; with as many GPUs as asked it runs itself under torch.distributed.run in a child process (the CPU suite runs that start-up with gloo,
    tests/test_parallel_gloo.py); the line of an N = 1 run through the process group carries the multi-GPU evidence fields."""
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2, r.stderr[-2000:]
    assert last_json(r.stdout)["n_gpus_visible"] == n - 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--dist", "--timed-only"],
                       env=env_for(0, 1, free_port()), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    mg = last_json(r.stdout)["multi_gpu"]
    print(mg)
    assert mg["rccl_world"] == 1 and mg["backend"] == "nccl" and mg["rays_per_rank"] == [640000] and mg["frame_assembly_ms_per_rank"][0] > 0


DRIVERS = ("render_vanilla", "render_smpl_nerf", "render_hybrid_nerf", "render_hybrid_nerf_multi_persons")


def test_frame_drivers_shard_through_rccl_on_a_group_of_one_rank():
    """BASELINE configs 4 / 5 'ray-batch sharded ... with RCCL gather': the drivers themselves shard when a process group exists
    (render_utils._frame -> parallel.render_frame_sharded).  One rank, real RCCL gather, device tensors."""
    env = env_for(0, 1, free_port())
    env["NEUMAN_FORCE_COLLECTIVE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "dist_drivers_check.py"), "nccl"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r.stdout)
    print(out)
    for k in DRIVERS:
        assert out[k]["bit_identical"] and out[k]["finite"], (k, out[k])
    assert 0.02 < out["render_hybrid_nerf"]["hit_fraction"] < 0.9


@pytest.mark.parametrize("world", [2, 4])
def test_frame_drivers_shard_across_ranks_sharing_the_gpu(world):
    """two ranks -- and four (the ranks and this process all hold the one GPU, which takes at most six processes at once) --, each rendering the rays of its interleaved tiles through the SAME driver call (hit compaction, the hybrid C call and
    the three-actor merge all see half a frame), gloo assembly: the hybrid and the three-actor frames are bit-identical to the
    unsharded ones"""
    port = free_port()
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "helpers", "dist_drivers_check.py"), "gloo"], env=env_for(r, world, port),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate(timeout=1200) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    out = last_json(outs[0][0])
    print(out)
    assert out["world"] == world
    for k in DRIVERS:
        assert out[k]["bit_identical"] and out[k]["finite"], (k, out[k])
        assert sum(out[k]["rays_per_rank"]) == out["rays"] and len(out[k]["rays_per_rank"]) == world


def test_interleaved_tiles_balance_the_hit_rays_at_world_8():
    """hit rays cluster in the image centre, so tiles are interleaved.  For the C4 (1280x720, one body) and C5 (1920x1080,
    three bodies) cameras the per-rank count of hit rays (x actors) at world 8 is within 5 % of the mean with the frame renderers'
    tile (parallel.FRAME_TILE); one device computes every rank's list (tools/bench_configs.py --imbalance)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_configs.py"), "--imbalance"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 3
    for ln in lines:
        msg = {k: round(v["hit_ray_imbalance"], 4) for k, v in ln.items() if isinstance(v, dict)}
        print(ln["config"], "hit fraction", round(ln["hit_fraction"], 3), msg)
        for w in (2, 4, 8):
            assert ln[f"world{w}_frame_tile"]["hit_ray_imbalance"] <= 0.05, (ln["config"], w, ln[f"world{w}_frame_tile"])
            assert sum(ln[f"world{w}_frame_tile"]["rays_per_rank"]) == ln["rays"]
