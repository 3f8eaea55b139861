"""Frame time and peak device memory of the multi-person renderer's two routes on the C5-like synthetic scene (tools/bench_configs.py: 1920 x 1080,
background 192 + 128 samples, 192 per actor): today's route (MULTI_FUSED off: the compact one-kernel merge up to three actors, full per-actor arrays
merged list by list beyond) against the fused call (MULTI_FUSED on: nm_render_rays_multi).  One process, the routes alternating A B A B after
one warm-up frame each; two JSON lines per actor count: the frames, then the merge + composite kernels alone on 2^17 rays.  The frames of the two routes are compared bit for bit.

    python tools/multi_fused_time.py [--actors 3,5,8] [--small] [--rounds 2] [--max-rays N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ml-neuman_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", default="3,5,8")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-rays", type=int, default=0, help="rays per launch of both routes (0: render_utils.MAX_RAYS_PER_LAUNCH as it is)")
    args = ap.parse_args()
    from neuman_hip import ray_utils, render_utils, synthetic
    if args.max_rays:
        render_utils.MAX_RAYS_PER_LAUNCH = args.max_rays
    dev = torch.device("cuda", 0)
    coarse, fine, human = (synthetic.make_joiner(0).to(dev), synthetic.make_joiner(1).to(dev), synthetic.make_joiner(2, 'rotate').to(dev))
    verts_c, faces = synthetic.capsule_mesh() if not args.small else synthetic.capsule_mesh(20, 24)
    posed, T = synthetic.twist_transforms(verts_c)
    w, h = (480, 270) if args.small else (1920, 1080)
    cap = synthetic.SimpleCapture(w, h, fx=1.2 * w, c2w=synthetic.spherical_c2w(20., -5., 3.5), near=0.0, far=3.14)
    coords = np.argwhere(np.ones(cap.shape))[:, ::-1]
    o, d = ray_utils.shot_rays(cap, coords)
    o, d = torch.from_numpy(o).to(dev, torch.float32).contiguous(), torch.from_numpy(d).to(dev, torch.float32).contiguous()
    with torch.no_grad():
        for A in [int(x) for x in args.actors.split(",")]:
            vs, ms = [], []
            for k, dx in enumerate(np.linspace(-0.7, 0.7, A) if A <= 3 else np.linspace(-1.4, 1.4, A)):
                shift = np.array([dx, 0, 0.1 * (k % 3)], np.float32)
                p2 = (posed + shift).astype(np.float32)
                T2 = T.copy()
                T2[:, :3, 3] += shift
                vs.append(torch.from_numpy(p2).to(dev))
                ms.append(ray_utils.mesh_to_device(p2, faces, T2, dev))
            hit = torch.zeros(o.shape[0], device=dev, dtype=torch.int32)
            for v in vs:
                near, far = ray_utils.geometry_guided_near_far(o, d, v, 0.2)
                hit += (near < far).to(torch.int32)

            def frame(fused):
                render_utils.MULTI_FUSED = fused
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                out = render_utils.render_multi_rays(coarse, fine, [human] * A, o, d, 0.0, 3.14, vs, ms, 192, 128, True, 0.2)
                torch.cuda.synchronize()
                return out, (time.perf_counter() - t0) * 1e3, (torch.cuda.max_memory_allocated() - base) / 2 ** 30

            ref, _, _ = frame(False)                              # warm-up of either route; their frames
            new, _, _ = frame(True)
            same = bool(torch.equal(ref[0], new[0]) and torch.equal(ref[1], new[1]))
            del ref, new
            ms_, gb = {False: [], True: []}, {False: [], True: []}
            for _ in range(args.rounds):                          # A B A B
                for fused in (False, True):
                    _, t, g = frame(fused)
                    ms_[fused].append(t)
                    gb[fused].append(g)
            print(json.dumps({"actors": A, "rays": int(o.shape[0]), "rays_per_launch": render_utils.MAX_RAYS_PER_LAUNCH, "hit_rays_x_actors": int(hit.sum()), "rays_hit_by_two_or_more": int((hit >= 2).sum()),
                              "frames_bit_identical": same, "parent_route_ms": ms_[False], "fused_ms": ms_[True],
                              "parent_route_peak_gib": max(gb[False]), "fused_peak_gib": max(gb[True]),
                              "speedup_of_medians": float(np.median(ms_[False]) / np.median(ms_[True]))}), flush=True)
            torch.cuda.empty_cache()
            # the merge + composite alone, every ray hitting every actor (the kernels' worst case): one wide kernel against list by list
            Rm = 1 << 17
            g = torch.Generator(device=dev).manual_seed(A)
            zs = [torch.sort(torch.rand((Rm, n), device=dev, generator=g) * 3.0, dim=1)[0].contiguous() for n in [320] + [192] * A]
            raws = [torch.randn((Rm, z.shape[1], 4), device=dev, generator=g) for z in zs]
            dm = d[:Rm].contiguous()

            def list_by_list():
                z_all, raw_all = zs[0], raws[0]
                for z, raw in zip(zs[1:], raws[1:]):
                    z_all, raw_all = render_utils.merge_sorted(z_all, raw_all, z, raw)
                return render_utils.raw2outputs(raw_all, z_all, dm, want_weights=False)[0]

            def timed(fn):
                ts = []
                for it in range(4):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if it:
                        ts.append(e0.elapsed_time(e1))
                return out, float(np.median(ts))
            one = (render_utils.merge_composite_lists if A <= 3 else render_utils.merge_composite_lists_wide)
            ref_m, t_lists = timed(list_by_list)
            new_m, t_one = timed(lambda: one(zs, raws, dm)[0])
            print(json.dumps({"actors": A, "merge_only_rays": Rm, "merged_samples": 320 + 192 * A, "kernel": one.__name__, "list_by_list_ms": t_lists,
                              "one_kernel_ms": t_one, "bit_identical": bool(torch.equal(ref_m, new_m))}), flush=True)
            del zs, raws, ref_m, new_m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
