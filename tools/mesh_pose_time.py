"""Time of the mesh pose entry point (csrc/mesh_pose.hip: nm_mesh_pose_batch) on an extraction-sized mesh: the surface 0.03 outside
synthetic.capsule_mesh() extracted by mesh_extract.extract_mesh from the analytic offset field on a 128^3 grid, bound to the capsule, posed by
the transforms of synthetic.smpl_like_model over --frames frames of synthetic.smpl_like_frames (nm_smpl_frames: float64, V + J rows; and the
same values as float32), with and without normals.  Beside it, on the same device in the same run, the torch expression of rules P2 / P3
(gather [b,N,3,4,4], float64 multiply-sum), which is what a caller had to write before; it runs --torch-chunk frames at a time, since its
gathered operand is 384 bytes per vertex and frame.  The entry point is timed alone, its outputs allocated before: HIP events on the current
stream around --inner back-to-back calls, --warmup warm-ups, the median (and the minimum) of --runs such windows, per call; two more arms bind
every vertex to row 0, which leaves the loads and the arithmetic and takes the gathering away.  Bytes/s counts what the call has to move at
least: the output plus the shared 36-byte row (tri, bary, point; 48 with the normal) of every vertex once.  One JSON line per arm; --md writes
the table profiles/mesh_pose.md keeps.

    timeout -k 10 600 python tools/mesh_pose_time.py [--frames 64] [--runs 20] [--inner 10] [--md profiles/mesh_pose.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ml-neuman_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

OFFSET = 0.03
BOX = (-0.32, -0.67, -0.22, 0.32, 0.67, 0.22)
RES = 128


def event_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def capsule_surface(dev):
    """-> (verts, faces, normals, body vertices, body faces): the offset surface of the capsule from the device's own extractor"""
    from neuman_hip import mesh_extract, ray_utils, synthetic
    body_v, body_f = synthetic.capsule_mesh()
    body = ray_utils.Mesh(body_v, body_f, None, dev)
    ax = [torch.linspace(BOX[a], BOX[3 + a], RES, device=dev) for a in range(3)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    grid = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()
    field = (OFFSET - ray_utils.signed_distance_dev(grid, body)[0]).reshape(RES, RES, RES).contiguous()
    verts, faces, normals = mesh_extract.clean_mesh(*mesh_extract.extract_mesh(field, BOX, 0.0))
    return verts, faces, normals, body_v, body_f


def torch_pose(T, tri, bary64, pts64, chunk):
    """rules P2 / P3 as torch writes them: gather, float64 multiply-sum, float32 at the end"""
    out = []
    for b0 in range(0, T.shape[0], chunk):
        M = (T[b0:b0 + chunk, tri] * bary64[None, :, :, None, None]).sum(2)                      # [b,N,4,4] out of [b,N,3,4,4]
        out.append(((M[..., :3, :3] * pts64[None, :, None, :]).sum(-1) + M[..., :3, 3]).to(torch.float32))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--torch-chunk", type=int, default=8)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    from neuman_hip import _lib, mesh_pose, smpl, synthetic
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    verts, faces, normals, body_v, body_f = capsule_surface(dev)
    N = int(verts.shape[0])
    binding = mesh_pose.bind_mesh(verts, body_v, body_f)
    body = smpl.SMPL(synthetic.smpl_like_model(), device=dev)
    poses, betas, align = synthetic.smpl_like_frames(args.frames)
    aligns = np.tile(np.eye(4), (args.frames, 1, 1))
    for i, name in enumerate(sorted(align)):
        aligns[i][:, :3] = align[name]
    T64 = body.frames(poses, betas, aligns, 1.0, True)[0]
    T32 = T64.to(torch.float32)
    B, rows = int(T64.shape[0]), int(T64.shape[1])
    lines = []
    out_pts, out_normals = torch.empty((B, N, 3), device=dev), torch.empty((B, N, 3), device=dev)
    # every vertex bound to row 0: the same loads and arithmetic with nothing to gather, which is what the call costs when its transforms come for free
    row0 = mesh_pose.Binding(torch.zeros_like(binding.tri), binding.bary)
    arms = [("f64", T64, None, binding), ("f64 + normals", T64, normals, binding), ("f32", T32, None, binding), ("f32 + normals", T32, normals, binding),
            ("f64, every vertex bound to row 0", T64, None, row0), ("f32, every vertex bound to row 0", T32, None, row0)]
    for name, T, nrm, bnd in arms:
        def calls():                                            # the entry point alone, outputs allocated before: --inner launches back to back per timed window
            for _ in range(args.inner):
                mesh_pose._launch(verts, nrm, T, bnd.tri, bnd.bary, False, out_pts, None if nrm is None else out_normals, None)
        med, lo = (t / args.inner for t in event_ms(calls, args.warmup, args.runs))
        moved = B * N * (12 if nrm is None else 24) + N * (36 if nrm is None else 48)
        gathered = B * N * 3 * 12 * T.element_size()            # rows 0-2 of three transforms per vertex and frame, as the threads ask for them
        lines.append({"arm": "nm_mesh_pose_batch " + name, "ms_median": med, "ms_min": lo, "bytes": moved, "GB_per_s": moved / med / 1e6,
                      "table_bytes": T.numel() * T.element_size(), "gathered_bytes": gathered})
    med, lo = event_ms(lambda: mesh_pose.pose_mesh(verts, binding, T64, normals=normals), args.warmup, args.runs)
    moved = B * N * 24 + N * 48
    lines.append({"arm": "pose_mesh f64 + normals (the Python call: checks, two allocations, one launch)", "ms_median": med, "ms_min": lo, "bytes": moved,
                  "GB_per_s": moved / med / 1e6, "table_bytes": T64.numel() * 8, "gathered_bytes": B * N * 288})
    tri, bary64, pts64 = binding.tri.long(), binding.bary.double(), verts.double()
    med, lo = event_ms(lambda: torch_pose(T64, tri, bary64, pts64, args.torch_chunk), 1, max(3, args.runs // 4))
    moved = B * N * 12 + N * 36
    lines.append({"arm": f"torch gather + float64 multiply-sum, {args.torch_chunk} frames at a time", "ms_median": med, "ms_min": lo, "bytes": moved,
                  "GB_per_s": moved / med / 1e6, "table_bytes": T64.numel() * 8, "gathered_bytes": B * N * 384})
    ours = mesh_pose.pose_mesh(verts, binding, T64)
    theirs = torch_pose(T64, tri, bary64, pts64, args.torch_chunk)
    agree = float((ours - theirs).abs().max())                  # (torch's sum over the three corners may associate differently: not bit for bit)
    head = {"device": torch.cuda.get_device_name(0), "verts": N, "faces": int(faces.shape[0]), "grid": RES, "frames": B, "table_rows": rows,
            "runs": args.runs, "warmup": args.warmup, "inner": args.inner, "max_abs_difference_to_torch": agree}
    print(json.dumps(head), flush=True)
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.md:
        with open(args.md, "w") as f:
            f.write("# Mesh pose (`csrc/mesh_pose.hip`): time of `nm_mesh_pose_batch`\n\n")
            f.write(f"`python tools/mesh_pose_time.py --frames {B} --runs {args.runs} --inner {args.inner}` on one {head['device']}: HIP events on the current stream "
                    f"around {args.inner} back-to-back calls of the entry point with its outputs allocated before (around one call for the Python and torch arms), "
                    f"{args.warmup} warm-ups, median and minimum of {args.runs} windows, per call.  Nothing in the tests depends on these numbers.\n\n")
            f.write(f"The mesh: the surface {OFFSET} outside `synthetic.capsule_mesh()` extracted on a {RES}^3 grid, {N} vertices, {head['faces']} faces, bound to the "
                    f"capsule; {B} frames of `synthetic.smpl_like_frames` through `nm_smpl_frames` ({rows} rows per frame).  Bytes = the output plus every vertex's "
                    "shared row (tri, bary, point; the normal) once.\n\n")
            f.write("| arm | ms (median) | ms (min) | output + binding, MB | GB/s of those | transform tables, MB | gathered by the threads, MB |\n|---|---|---|---|---|---|---|\n")
            for line in lines:
                f.write(f"| {line['arm']} | {line['ms_median']:.3f} | {line['ms_min']:.3f} | {line['bytes'] / 1e6:.1f} | {line['GB_per_s']:.0f} | "
                        f"{line['table_bytes'] / 1e6:.1f} | {line['gathered_bytes'] / 1e6:.0f} |\n")
            f.write(f"\nLargest absolute difference between `pose_mesh` and the torch expression on this mesh: {agree:.3g}.\n")


if __name__ == "__main__":
    main()
