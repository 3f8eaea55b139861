"""Time of the soft silhouette (render_utils.soft_silhouette: csrc/silhouette.hip's forward and backward) of the 13 776-face body at 1280x720
and 1920x1080 at the reference's sigma (1e-4, blur_radius log(1/1e-4 - 1) sigma), the largest number of candidates in a pixel there (how far
the header's rule S4 is from pytorch3d's 100 faces per pixel), and one iteration of optimize_smpl (neuman_hip/optimize_smpl.py: skinning,
joints, silhouette, backward, Adam step) on the synthetic SMPL-like body -- beside the same iteration with the silhouette replaced by a
constant, which shows the share of the new kernels.  One warm-up, then the median of --runs calls, each ended by a device synchronise.
One JSON line per size.

    python tools/silhouette_time.py [--runs 50] [--no-fit] [--sizes 1280x720,1920x1080]

For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/silhouette_time.py --no-fit --runs 20` (a run of its
own: tracing slows the host); profiles/silhouette.md keeps both.
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


def fit_capture(w, h, body, faces):
    """a capture for optimize_smpl: the synthetic body at rest is the start, the same body with its upper arms turned the target"""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import render_utils, synthetic
    cap = synthetic.SimpleCapture(w, h, c2w=synthetic.spherical_c2w(20., -10., 3.0))
    cap.binary_mask, cap.keypoints, cap.densepose = np.zeros((h, w), np.float32), np.zeros((17, 3)), np.arange(25)
    start = dict(pose=np.zeros(72, np.float32), betas=np.zeros(10, np.float32))
    align = np.eye(4)[:, :3]
    obj = O.Objective(cap, start, faces, body, align, 1.0)
    target = np.zeros(72, np.float32)
    target[[16 * 3 + 1, 16 * 3 + 2, 17 * 3 + 1, 17 * 3 + 2]] = 0.15
    with torch.no_grad():
        wv, wj = O.vertext_forward(torch.as_tensor(target).cuda(), obj.betas, obj.align, body, 1.0)
        cap.binary_mask = render_utils.body_mask(wv[0], faces, cap).float().cpu().numpy()
        proj = O.project_joints(wj[0], obj.K, obj.w2c, obj.shape).cpu().numpy()
    cap.keypoints[:, 2] = 1.0
    for s, c in O._SMPL_FROM_COCO.items():
        cap.keypoints[c, :2] = proj[s]
    return cap, start, align


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--no-fit", action="store_true", help="skip the optimize_smpl iteration")
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    args = ap.parse_args()
    from neuman_hip import _lib, raster, render_utils, smpl, synthetic
    from neuman_hip import optimize_smpl as O
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    verts_c, faces = synthetic.capsule_mesh()
    posed, _ = synthetic.twist_transforms(verts_c)
    v_dev = torch.from_numpy(posed).to(dev)
    sigma = raster.SIGMA
    for size in args.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        cap = synthetic.SimpleCapture(w, h, fx=1.2 * w, c2w=synthetic.spherical_c2w(20., -5., 3.0))
        R = raster.rasterizer_for(faces, v_dev.shape[0])
        cam = raster.camera_of(cap)
        g = torch.randn((h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        alpha, keep, n_cand = R.silhouette(v_dev, cam, sigma, want_count=True)

        def both():
            v = v_dev.clone().requires_grad_(True)
            render_utils.soft_silhouette(v, faces, cap, sigma).backward(g)

        fmed, flo, fhi = median_ms(lambda: R.silhouette(v_dev, cam, sigma), args.runs)
        bmed, blo, bhi = median_ms(both, args.runs)
        line = {"what": "soft_silhouette", "size": size, "faces": int(len(faces)), "sigma": sigma, "blur_radius": raster.default_blur_radius(sigma),
                "reach_px": float(np.sqrt(raster.default_blur_radius(sigma)) * min(w, h) / 2), "covered_fraction": float((alpha > 0.5).float().mean()),
                "soft_pixels": int(((alpha > 0) & (alpha < 1)).sum()), "max_n_cand": int(n_cand.max()), "pixels_over_100_candidates": int((n_cand > 100).sum()),
                "forward_ms": fmed, "forward_ms_min_max": [flo, fhi], "forward_backward_ms": bmed, "forward_backward_ms_min_max": [blo, bhi], "runs": args.runs}
        if not args.no_fit:
            model = synthetic.smpl_like_model(0)
            body = smpl.SMPLDiff(model, dev)
            mfaces = model['f'].astype(np.int32)
            fcap, start, align = fit_capture(w, h, body, mfaces)
            for name, sil in (("fit_iteration_ms", None), ("fit_iteration_constant_silhouette_ms", lambda v: torch.zeros((h, w), device=dev) + 0 * v.sum())):
                obj = O.Objective(fcap, start, mfaces, body, align, 1.0, sigma, silhouette=sil)
                pose = torch.nn.Parameter(torch.zeros(72, device=dev))
                optim = torch.optim.Adam([{"params": pose, "lr": 5e-3}])

                def step():
                    optim.zero_grad()
                    obj.loss(pose).backward()
                    optim.step()

                med, lo, hi = median_ms(step, args.runs)
                line.update({name: med, name + "_min_max": [lo, hi]})
            with torch.no_grad():
                wv, _ = O.vertext_forward(torch.zeros(72, device=dev), obj.betas, obj.align, body, 1.0)
            line["fit_max_n_cand"] = int(raster.rasterizer_for(mfaces, 6890).silhouette(wv[0], raster.camera_of(fcap), sigma, want_count=True)[2].max())
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
