"""Time of one SMPL overlay (render_utils.overlay_smpl: vertex pass, face setup + binning, raster + shade, byte select, and the image's trip
to the device and back) of the 13 776-face body at 1280x720 and 1920x1080, beside the frame time of the posed NeRF render of the same body
from the same camera (the 'C3 posed' workload of tools/bench_configs.py at that size).  One warm-up, then the median of --runs calls, each
ended by a device synchronise.  One JSON line per size.

    python tools/overlay_time.py [--runs 50] [--no-posed] [--sizes 1280x720,1920x1080]

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/overlay_time.py --no-posed` (a run of its own: tracing
slows the host); profiles/raster.md keeps both.
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


def median_ms(fn, runs):
    fn()                                                          # warm-up: code objects, the handle, the scratch at this size
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--no-posed", action="store_true", help="skip the posed NeRF frame the overlay is put beside")
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    args = ap.parse_args()
    from neuman_hip import _lib, raster, ray_utils, render_utils, synthetic
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    verts_c, faces = synthetic.capsule_mesh()
    posed, T = synthetic.twist_transforms(verts_c)
    v_dev = torch.from_numpy(posed).to(dev)
    human = synthetic.make_joiner(2, 'rotate').to(dev)
    with torch.no_grad():
        for size in args.sizes.split(","):
            w, h = (int(x) for x in size.split("x"))
            cap = synthetic.SimpleCapture(w, h, fx=1.2 * w, c2w=synthetic.spherical_c2w(20., -5., 3.0))
            image = np.random.default_rng(0).integers(0, 256, (h, w, 3), dtype=np.uint8)
            R = raster.rasterizer_for(faces, v_dev.shape[0])
            cam = raster.camera_of(cap)
            med, lo, hi = median_ms(lambda: render_utils.overlay_smpl(image, v_dev, faces, cap), args.runs)
            dmed, dlo, dhi = median_ms(lambda: R.rasterize(v_dev, cam, want_bary=False, shade=True), args.runs)
            mask = render_utils.body_mask(v_dev, faces, cap)
            line = {"what": "overlay_smpl", "size": size, "faces": int(len(faces)), "covered_fraction": float(mask.float().mean()),
                    "overlay_ms": med, "overlay_ms_min_max": [lo, hi], "device_passes_ms": dmed, "device_passes_ms_min_max": [dlo, dhi], "runs": args.runs}
            if not args.no_posed:
                mesh = ray_utils.mesh_to_device(posed, faces, T, dev)
                o, d = render_utils._pixel_rays(cap, dev)
                pmed, plo, phi = median_ms(lambda: render_utils.render_smpl_nerf_rays(human, o, d, v_dev, mesh, 128, True, False, 0.2, 1.0), min(args.runs, 3))
                line.update({"posed_render_ms": pmed, "posed_render_ms_min_max": [plo, phi], "overlay_over_posed": med / pmed})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
