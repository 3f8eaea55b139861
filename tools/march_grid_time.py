#!/usr/bin/env python
"""What early ray termination and an occupancy grid are worth TOGETHER in the background passes (render_utils.MARCH_WITH_GRID, DESIGN.md
K11): one 800x800 frame, 128 coarse + 128 importance samples per ray, synthetic.make_joiner(1, preset='opaque') as coarse and fine net,
grids from OccupancyGrid.from_net with dilate 1 (the default) and 0.

    python tools/march_grid_time.py [--steps 7] [--eps 1e-4] [--res 128] [--out FILE]

Four routes per grid: plain (every sample), termination (TERMINATION_EPS = --eps), grid (the grid attached), both (grid, termination and
the switch).  One process; every route is warmed up first (code objects, handles, workspaces, every chunk shape the adaptive march takes),
then the routes are alternated A B C D A B C D ... so that clock and thermal drift spreads over all of them; device events around whole frames
(render_vanilla_rays, untraced); the median and the spread of --steps frames per route.  The evaluated fractions come from one traced frame
per route.  Prints one JSON line per grid and, with --out, appends them to FILE."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-neuman_amd")]

import torch  # noqa: E402

ROUTES = ("plain", "termination", "grid", "both")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def fractions(trace):
    """evaluated / total of the coarse and the shading pass of a traced frame, and what the grid dropped of the live rays' candidates"""
    out = {}
    for name, keys in (("coarse", ("march_coarse", "occupancy_coarse")), ("fine", ("march", "occupancy"))):
        st = [s for k in keys for s in trace.get(k, [])]
        if not st:
            out[name] = 1.0
            continue
        tot = sum(s['total'] for s in st)
        out[name] = round(sum(s['evaluated'] for s in st) / tot, 4)
        if any('grid_skipped' in s for s in st):
            out[name + "_grid_skipped"] = round(sum(s.get('grid_skipped', 0) for s in st) / tot, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from neuman_hip import _lib, occupancy, render_utils, synthetic
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    W, S, NI, near, far = 800, 128, 128, 0.0, 3.14
    net = synthetic.make_joiner(1, preset='opaque').to(dev)
    o, d = render_utils._pixel_rays(synthetic.SimpleCapture(W, W), dev)
    box = occupancy.rays_aabb(o, d, near, far)
    keep = (render_utils.TERMINATION_EPS, render_utils.MARCH_WITH_GRID)

    def frame(route, grid, trace=None):
        render_utils.TERMINATION_EPS = a.eps if route in ("termination", "both") else 0.0
        render_utils.MARCH_WITH_GRID = route == "both"
        if route in ("grid", "both"):
            occupancy.attach(net, grid)
        try:
            return render_utils.render_vanilla_rays(net, net, o, d, near, far, S, NI, True, trace=trace)
        finally:
            occupancy.detach(net)
            render_utils.TERMINATION_EPS, render_utils.MARCH_WITH_GRID = keep

    with torch.no_grad():
        for dilate in (1, 0):
            grid = occupancy.OccupancyGrid.from_net(net, box, res=a.res, dilate=dilate)
            frames, frac = {}, {}
            for r in ROUTES:                                                       # warm-up: two frames each, the second one traced
                frame(r, grid)
                tr = {}
                frames[r] = frame(r, grid, tr)[0]
                frac[r] = fractions(tr)
            torch.cuda.synchronize()
            ms = {r: [] for r in ROUTES}
            for _ in range(a.steps):
                for r in ROUTES:
                    ms[r].append(timed(lambda: frame(r, grid))[0])
            line = {"tool": "march_grid_time", "device": torch.cuda.get_device_name(0), "frame": f"{W}x{W}", "samples": f"{S}+{NI}", "preset": "opaque",
                    "eps": a.eps, "grid": f"{a.res}^3 dilate {dilate}", "occupied": round(grid.occupied_fraction(), 4), "steps": a.steps, "routes": {}}
            for r in ROUTES:
                line["routes"][r] = {"ms_median": round(statistics.median(ms[r]), 2), "ms_min": round(min(ms[r]), 2), "ms_max": round(max(ms[r]), 2),
                                     "evaluated": frac[r],
                                     "linf_vs_plain": float((frames[r] - frames["plain"]).abs().max()),
                                     "linf_vs_grid": float((frames[r] - frames["grid"]).abs().max())}
            print(json.dumps(line), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
