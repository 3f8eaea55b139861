#!/usr/bin/env python
"""Occupancy-grid empty-space skipping on the workload it is for: one 800x800 frame, 128 coarse + 128 importance
samples per ray, synthetic.make_joiner(1, preset='opaque') as coarse and fine net (bench.py's early-termination leg).

    python tools/occupancy_bench.py [--steps 10] [--res 128] [--probes 8] [--dilate 1] [--out FILE]

Prints one JSON line: the grid's build time (median of --steps builds), its occupied fraction, the evaluated fraction of each
pass, ms per frame and rays/s with and without the grid (median of --steps frames each, interleaved; HIP events on the
stream), and the frame with the grid against the every-sample frame: L-inf and the count of rays that differ at all."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-neuman_amd")]

import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--probes", type=int, default=8)
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from neuman_hip import _lib, occupancy, render_utils, synthetic
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    W, S, NI, near, far = 800, 128, 128, 0.0, 3.14
    net = synthetic.make_joiner(1, preset='opaque').to(dev)
    o, d = render_utils._pixel_rays(synthetic.SimpleCapture(W, W), dev)
    box = occupancy.rays_aabb(o, d, near, far)

    def frame():
        return render_utils.render_vanilla_rays(net, net, o, d, near, far, S, NI, True)

    def build():
        return occupancy.OccupancyGrid.from_net(net, box, res=a.res, probes=a.probes, dilate=a.dilate)

    with torch.no_grad():
        grid = build()                                                          # warm-up (handle, code objects)
        builds = [timed(build)[0] for _ in range(a.steps)]
        grid = build()
        rgb0, dep0 = frame()
        occupancy.attach(net, grid)
        tr = {}
        rgb1, dep1 = render_utils.render_vanilla_rays(net, net, o, d, near, far, S, NI, True, trace=tr)
        occupancy.detach(net)
        t_all, t_grid = [], []
        for _ in range(a.steps):                                                # interleaved: the two see the same clocks
            t_all.append(timed(frame)[0])
            occupancy.attach(net, grid)
            t_grid.append(timed(frame)[0])
            occupancy.detach(net)
    R = o.shape[0]
    diff = (rgb1 - rgb0).abs().max(1).values
    ms_all, ms_grid = statistics.median(t_all), statistics.median(t_grid)
    sc, sf = tr['occupancy_coarse'][0], tr['occupancy'][0]
    res = {
        "what": f"{W}x{W} frame, {S} + {NI} samples/ray, make_joiner(1, preset='opaque') as coarse and fine net, grid {a.res}^3 x {a.probes} probes, "
                f"dilate {a.dilate}, threshold 0, box = the frame's ray segments (occupancy.rays_aabb); median of {a.steps}",
        "device": torch.cuda.get_device_name(dev),
        "grid_build_ms": round(statistics.median(builds), 3),
        "grid_occupied_fraction": round(grid.occupied_fraction(), 4),
        "evaluated_fraction_coarse": round(sc['evaluated'] / sc['total'], 4),
        "evaluated_fraction_fine": round(sf['evaluated'] / sf['total'], 4),
        "ms_per_frame_every_sample": round(ms_all, 3),
        "ms_per_frame_grid": round(ms_grid, 3),
        "rays_per_s_every_sample": round(R / ms_all * 1e3),
        "rays_per_s_grid": round(R / ms_grid * 1e3),
        "speedup": round(ms_all / ms_grid, 3),
        "rgb_linf_vs_every_sample": float(diff.max()),
        "depth_linf_vs_every_sample": float((dep1 - dep0).abs().max()),
        "rays_differing": int((diff > 0).sum()),
        "rays": R,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
