#!/usr/bin/env python
"""What the marched background passes cost as ONE C call each (render_utils.MARCH_FUSED, nm_march_pass) against the route that exists
(march_pass_rays, adaptive chunks with one host read per chunk): 128 coarse + 128 importance samples per ray,
synthetic.make_joiner(1, preset='opaque') as coarse and fine net, termination at --eps.

    python tools/march_fused_time.py [--steps 7] [--eps 1e-4] [--out FILE]

Three routes: adaptive (MARCH_FUSED off: today's default), fused16 and fused32 (MARCH_FUSED on, TERMINATION_CHUNK = 16 / 32), on two batches:
the 800x800 frame and its first 131072 rays (the size the hybrid renderers cut a frame into).  One process; every route is warmed up first,
then the routes are alternated A B C A B C ... so that clock and thermal drift spreads over all of them; device events around whole
render_vanilla_rays calls (untraced); the median and the spread of --steps calls per route.  The evaluated fractions and launch counts come
from one traced call per route.  Prints one JSON line per batch and, with --out, appends them to FILE."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-neuman_amd")]

import torch  # noqa: E402

ROUTES = {"adaptive": (False, 32), "fused16": (True, 16), "fused32": (True, 32)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def counts(trace):
    """evaluated / total and the MLP launches of the coarse and the shading pass of a traced call"""
    out = {}
    for name, key in (("coarse", "march_coarse"), ("fine", "march")):
        st = trace.get(key, [])
        out[name] = round(sum(s['evaluated'] for s in st) / max(1, sum(s['total'] for s in st)), 4)
        out[name + "_launches"] = sum(s['launches'] for s in st)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from neuman_hip import _lib, render_utils, synthetic
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    W, S, NI, near, far = 800, 128, 128, 0.0, 3.14
    net = synthetic.make_joiner(1, preset='opaque').to(dev)
    o_all, d_all = render_utils._pixel_rays(synthetic.SimpleCapture(W, W), dev)
    keep = (render_utils.TERMINATION_EPS, render_utils.MARCH_FUSED, render_utils.TERMINATION_CHUNK)

    def call(route, o, d, trace=None):
        render_utils.TERMINATION_EPS = a.eps
        render_utils.MARCH_FUSED, render_utils.TERMINATION_CHUNK = ROUTES[route]
        try:
            return render_utils.render_vanilla_rays(net, net, o, d, near, far, S, NI, True, trace=trace)
        finally:
            render_utils.TERMINATION_EPS, render_utils.MARCH_FUSED, render_utils.TERMINATION_CHUNK = keep

    with torch.no_grad():
        plain_all = render_utils.render_vanilla_rays(net, net, o_all, d_all, near, far, S, NI, True)[0]
        for label, n in ((f"{W}x{W} frame", W * W), ("131072 rays", 1 << 17)):
            o, d, plain = o_all[:n].contiguous(), d_all[:n].contiguous(), plain_all[:n]
            frames, cnt = {}, {}
            for r in ROUTES:                                                       # warm-up: two calls each, the second one traced
                call(r, o, d)
                tr = {}
                frames[r] = call(r, o, d, tr)[0]
                cnt[r] = counts(tr)
            torch.cuda.synchronize()
            ms = {r: [] for r in ROUTES}
            for _ in range(a.steps):
                for r in ROUTES:
                    ms[r].append(timed(lambda: call(r, o, d))[0])
            line = {"tool": "march_fused_time", "device": torch.cuda.get_device_name(0), "batch": label, "samples": f"{S}+{NI}", "preset": "opaque",
                    "eps": a.eps, "steps": a.steps, "routes": {}}
            for r in ROUTES:
                line["routes"][r] = {"ms_median": round(statistics.median(ms[r]), 2), "ms_min": round(min(ms[r]), 2), "ms_max": round(max(ms[r]), 2),
                                     **cnt[r], "linf_vs_plain": float((frames[r] - plain).abs().max())}
            print(json.dumps(line), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
