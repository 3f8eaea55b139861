"""Time of one fit iteration per frame for a sequence of N frames of the 13 776-face synthetic body at 1280x720: a Python loop of
optimize_smpl's iteration over the frames (one Objective and one Adam per frame: N skinning chains, N silhouettes and N host reads per
sweep) beside optimize_smpl_sequence's iteration (SequenceObjective and one Adam on [B,72] per chunk) at frames_per_batch 1, 8 and 32.
A sweep is one iteration of every frame; the four ways take turns, sweep by sweep, so that they see the same clocks.  One warm-up sweep
each, then the median of --runs sweeps, each ended by a device synchronise; ms per frame-iteration = sweep / N.  One JSON line.

    python tools/sequence_fit_time.py [--frames 32] [--runs 12] [--size 1280x720] [--only loop|seq1|seq8|seq32]

For the launches per iteration and the per-kernel split run one way alone under
`rocprofv3 --kernel-trace --stats -- python tools/sequence_fit_time.py --only seq32 --runs 10` (a run of its own: tracing slows the host);
profiles/sequence_fit.md keeps both.
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


def sequence(n, w, h, body, faces):
    """n captures for the fit: the synthetic body at rest is every frame's start; frame i's target is the body with its upper arms turned by
    an angle of its own, seen by a camera of its own"""
    from neuman_hip import optimize_smpl as O
    from neuman_hip import raster, render_utils, synthetic
    caps, smpls, aligns = [], [], {}
    eye = torch.eye(4, device='cuda')
    for i in range(n):
        cap = synthetic.SimpleCapture(w, h, c2w=synthetic.spherical_c2w(20. + 0.5 * i, -10. + 0.2 * i, 3.0 + 0.01 * i))
        cap.image_path = f"images/{i:05d}.png"
        target = np.zeros(72, np.float32)
        target[[16 * 3 + 1, 16 * 3 + 2, 17 * 3 + 1, 17 * 3 + 2]] = 0.05 + 0.005 * i
        w2c, fx, fy, cx, cy, _, _ = raster.camera_of(cap)
        K = torch.tensor([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]], device='cuda')
        with torch.no_grad():
            wv, wj = O.vertext_forward(torch.as_tensor(target).cuda(), torch.zeros(10, device='cuda'), eye, body, 1.0)
            cap.binary_mask = render_utils.body_mask(wv[0], faces, cap).float().cpu().numpy()
            proj = O.project_joints(wj[0], K, torch.as_tensor(w2c).cuda().float(), (h, w)).cpu().numpy()
        cap.keypoints = np.zeros((17, 3))
        cap.keypoints[:, 2] = 1.0
        for s, c in O._SMPL_FROM_COCO.items():
            cap.keypoints[c, :2] = proj[s]
        cap.densepose = np.arange(25)
        caps.append(cap)
        smpls.append(dict(pose=np.zeros(72, np.float32), betas=np.zeros(10, np.float32)))
        aligns[f"{i:05d}.png"] = np.eye(4)[:, :3]
    return caps, smpls, aligns


def make_sweep(caps, smpls, aligns, faces, body, sigma, frames_per_batch):
    """-> a function that runs one iteration of every frame: frames_per_batch None = optimize_smpl's loop body frame by frame, else
    optimize_smpl_sequence's per chunk"""
    from neuman_hip import optimize_smpl as O
    dev = body.v_template.device
    limits = torch.from_numpy(O.clip_smpl_vals()).float().to(dev)
    states = []
    if frames_per_batch is None:
        for i, cap in enumerate(caps):
            obj = O.Objective(cap, smpls[i], faces, body, aligns[os.path.basename(cap.image_path)], 1.0, sigma)
            pose = torch.nn.Parameter(torch.zeros(72, device=dev))
            states.append((obj, pose, torch.optim.Adam([{"params": pose, "lr": 5e-3}]), torch.from_numpy(O.turn_smpl_gradient_on(cap.densepose)).float().to(dev)))
    else:
        for lo in range(0, len(caps), frames_per_batch):
            chunk = caps[lo:lo + frames_per_batch]
            obj = O.SequenceObjective(chunk, smpls[lo:lo + frames_per_batch], faces, body, aligns, 1.0, sigma)
            pose = torch.nn.Parameter(torch.zeros((len(chunk), 72), device=dev))
            mask = torch.from_numpy(np.stack([O.turn_smpl_gradient_on(c.densepose) for c in chunk])).float().to(dev)
            states.append((obj, pose, torch.optim.Adam([{"params": pose, "lr": 5e-3}]), mask))

    def sweep():
        for obj, pose, optim, grad_mask in states:
            optim.zero_grad()
            obj.loss(pose).backward()
            valid_mask = ((pose < limits[..., 1]) * (pose > limits[..., 0])).float()
            pose.grad = pose.grad * grad_mask * valid_mask
            optim.step()

    return sweep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--only", default=None, help="loop, seq1, seq8 or seq32: time (or profile) one way alone")
    args = ap.parse_args()
    from neuman_hip import _lib, raster, smpl, synthetic
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    w, h = (int(x) for x in args.size.split("x"))
    model = synthetic.smpl_like_model(0)
    body = smpl.SMPLDiff(model, dev)
    faces = model['f'].astype(np.int32)
    caps, smpls, aligns = sequence(args.frames, w, h, body, faces)
    ways = {"loop": None, "seq1": 1, "seq8": 8, "seq32": 32}
    if args.only:
        ways = {args.only: ways[args.only]}
    sweeps = {name: make_sweep(caps, smpls, aligns, faces, body, raster.SIGMA, fpb) for name, fpb in ways.items()}
    times = {name: [] for name in sweeps}
    for run in range(args.runs + 1):                              # run 0 is the warm-up: code objects, handles, scratch at this size
        for name, sweep in sweeps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sweep()
            torch.cuda.synchronize()
            if run:
                times[name].append((time.perf_counter() - t0) * 1e3 / args.frames)
    line = {"what": "sequence_fit", "size": args.size, "frames": args.frames, "faces": int(len(faces)), "sigma": raster.SIGMA, "runs": args.runs}
    for name, ts in times.items():
        ts = sorted(ts)
        line[name + "_ms_per_frame_iteration"] = ts[len(ts) // 2]
        line[name + "_min_max"] = [ts[0], ts[-1]]
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    line["silhouette_scratch_bytes_per_frame"] = 16 * 6890 + 48 * len(faces) + 12 * tiles + 24 * len(faces)
    line["skinning_workspace_bytes_per_frame"] = int(4 * (_lib.lib().nm_smpl_vertex_batch_workspace_floats(body._hip_handle(), 2) - _lib.lib().nm_smpl_vertex_batch_workspace_floats(body._hip_handle(), 1)))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
