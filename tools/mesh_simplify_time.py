"""Time of the mesh simplification (csrc/mesh_simplify.hip) on the mesh extract_mesh makes of a sphere's signed distance on a 128^3 grid
(profiles/mesh_smooth.md's), at cells of 2 and 4 grid steps: the whole `simplify_mesh` call under both placements (adjacency given, box given:
one read-back), and its count and fill phases alone through the entry points `simplify_mesh` calls; beside them, in the same run and alternating
with them, the route a caller has without these kernels, in torch on the same device: torch.unique on the cell keys, index_add_ means in
float64, the face remap and torch.unique(dim=0) over the surviving faces (mean placement only, unreferenced cells kept, duplicates by sorted
corners).  HIP events around each call on the current stream, warm-ups first, the median and the minimum of --runs.

Then what the thinner mesh buys downstream, in the same process: bind_mesh + pose_mesh_frames + render_mesh_frames for --frames frames at
--size x --size on the full and on the simplified mesh (host clock around each stage, a device synchronise at its end).

One JSON line.  profiles/mesh_simplify.md keeps the line and what follows from it.

    timeout -k 10 600 python tools/mesh_simplify_time.py [--runs 20] [--res 128] [--frames 64] [--size 512]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ml-neuman_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
CENTRE, RADIUS = (0.013, -0.021, 0.017), 0.6


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_route(verts, faces, lo, h, dims):
    """mean placement as a caller writes it today -> (verts', faces')"""
    c = torch.floor((verts.double() - lo) / h).long()
    c = torch.minimum(c.clamp(min=0), dims - 1)
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    cells, label = torch.unique(key, return_inverse=True)
    K = cells.shape[0]
    s = torch.zeros((K, 3), dtype=torch.float64, device=verts.device).index_add_(0, label, verts.double())
    n = torch.zeros((K,), dtype=torch.float64, device=verts.device).index_add_(0, label, torch.ones_like(label, dtype=torch.float64))
    f = label[faces.long()]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])]
    f = torch.unique(f.sort(1).values, dim=0)
    return (s / n[:, None]).float(), f.int()


class Phases:
    """the two entry points behind simplify_mesh, buffers allocated outside the timed window"""

    def __init__(self, verts, faces, lo, h, dims, adj):
        from neuman_hip import _lib, mesh_smooth
        self.L = _lib.lib()
        V, F = int(verts.shape[0]), int(faces.shape[0])
        self.nbytes = int(self.L.nm_mesh_simplify_workspace_bytes(V, F, *dims))
        self.ws = torch.empty((self.nbytes,), device=verts.device, dtype=torch.uint8)
        self.vc = torch.empty((V,), device=verts.device, dtype=torch.int32)
        self.mesh = (ctypes.c_void_p(verts.data_ptr()), V, ctypes.c_void_p(faces.data_ptr()), F, (ctypes.c_float * 3)(*lo), h, *dims)
        self.lists = (ctypes.c_void_p(adj.inc_off.data_ptr()), mesh_smooth._inc_ptr(adj))
        self.k, self.nf = ctypes.c_int64(0), ctypes.c_int64(0)
        self.count()
        K, Fo = int(self.k.value), int(self.nf.value)
        self.vo = torch.empty((K, 3), device=verts.device)
        self.fo = torch.empty((Fo, 3), device=verts.device, dtype=torch.int32)
        self.src = torch.empty((Fo,), device=verts.device, dtype=torch.int32)

    def count(self):
        from neuman_hip import _lib
        _lib.check(self.L.nm_mesh_simplify_count(*self.mesh, ctypes.c_void_p(self.vc.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()), self.nbytes,
                                                 ctypes.byref(self.k), ctypes.byref(self.nf), _lib.stream_ptr()), "nm_mesh_simplify_count")

    def fill(self, placement):
        from neuman_hip import _lib
        lists = self.lists if placement else (None, None)
        _lib.check(self.L.nm_mesh_simplify_fill(*self.mesh, placement, *lists, ctypes.c_void_p(self.ws.data_ptr()), self.nbytes, ctypes.c_void_p(self.vo.data_ptr()),
                                                ctypes.c_void_p(self.fo.data_ptr()), ctypes.c_void_p(self.src.data_ptr()), int(self.k.value), int(self.nf.value),
                                                _lib.stream_ptr()), "nm_mesh_simplify_fill")


def downstream(verts, faces, frames, size, rounds=3):
    """bind + pose + render of `frames` frames -> median ms of each stage over `rounds` rounds after one warm-up"""
    from neuman_hip import mesh_pose, mesh_smooth, render_utils, smpl, synthetic
    dev = verts.device
    body_v, body_f = synthetic.capsule_mesh()
    body = smpl.SMPL(synthetic.smpl_like_model(), device=dev)
    poses, betas, align = synthetic.smpl_like_frames(frames)
    aligns = np.tile(np.eye(4), (frames, 1, 1))
    for i, name in enumerate(sorted(align)):
        aligns[i][:, :3] = align[name]
    caps = [synthetic.SimpleCapture(size, size, c2w=synthetic.spherical_c2w(30., -20., 3.2)) for _ in range(frames)]
    normals = mesh_smooth.vertex_normals(verts, faces)
    colours = torch.rand((verts.shape[0], 3), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    ts = {"bind_ms": [], "pose_ms": [], "render_ms": []}
    covered = 0
    for r in range(rounds + 1):
        stamps = []
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        binding = mesh_pose.bind_mesh(verts, body_v, body_f)
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        posed, posed_n = mesh_pose.pose_mesh_frames(body, poses, betas, aligns, 1.0, verts, binding, normals)
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        images = render_utils.render_mesh_frames(posed, faces, caps, colours=colours, normals=posed_n)
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        if r > 0:
            for name, a, b in zip(ts, stamps[:-1], stamps[1:]):
                ts[name].append((b - a) * 1e3)
        covered = int((images != 255).any(-1).sum()) // frames
    out = {name: sorted(v)[len(v) // 2] for name, v in ts.items()}
    out["covered_pixels_per_frame"] = covered
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    import isosurface_ref as IR
    from neuman_hip import _lib, mesh_extract, mesh_simplify, mesh_smooth
    _lib.require_gpu()
    torch.cuda.set_device(0)
    field = torch.from_numpy(IR.sphere_field((args.res,) * 3, BOX, CENTRE, RADIUS)).cuda()
    verts, faces, _ = mesh_extract.extract_mesh(field, BOX, 0.0)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    adj = mesh_smooth.adjacency(faces, V)
    line = {"device": torch.cuda.get_device_name(0), "mesh": f"sphere_{args.res}", "verts": V, "faces": F, "runs": args.runs, "cells": {}}
    step = 2.0 / (args.res - 1)
    simplified = None
    for steps in (2, 4):
        cell = steps * step
        lo, h, dims = mesh_simplify.grid_of(BOX, cell)
        ph = Phases(verts, faces, lo, h, dims, adj)
        lo_t, dims_t = torch.tensor(lo, device='cuda', dtype=torch.float64), torch.tensor(dims, device='cuda')
        calls = {
            "simplify_quadric_ms": lambda: mesh_simplify.simplify_mesh(verts, faces, cell, aabb=BOX, adj=adj),
            "simplify_mean_ms": lambda: mesh_simplify.simplify_mesh(verts, faces, cell, aabb=BOX, placement='mean'),
            "count_ms": ph.count,
            "fill_quadric_ms": lambda: ph.fill(1),
            "fill_mean_ms": lambda: ph.fill(0),
            "torch_mean_ms": lambda: torch_route(verts, faces, lo_t, h, dims_t),
        }
        for _ in range(3):                                     # warm-up of every shape the timed window uses
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for _ in range(args.runs):                             # alternating: the kernels and the baseline see the same machine
            for name, fn in calls.items():
                times[name].append(timed(fn)[0])
        rec = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
        rec.update({name.replace("_ms", "_min_ms"): min(ts) for name, ts in times.items()})
        out = calls["simplify_quadric_ms"]()
        mean = calls["simplify_mean_ms"]()
        tv, tf = calls["torch_mean_ms"]()
        vc = ph.vc.long()
        used = torch.unique(vc[vc >= 0])
        rec.update({"cell": cell, "dims": list(dims), "verts_out": int(out[0].shape[0]), "faces_out": int(out[1].shape[0]),
                    "torch_verts_out": int(tv.shape[0]), "torch_faces_out": int(tf.shape[0]),
                    "largest_cluster": int(torch.bincount(vc[vc >= 0]).max()), "clusters": int(used.shape[0]),
                    "radius_rms_error_quadric": float(((out[0].double() - torch.tensor(CENTRE, device='cuda', dtype=torch.float64)).norm(dim=1) - RADIUS).pow(2).mean().sqrt()),
                    "radius_rms_error_mean": float(((mean[0].double() - torch.tensor(CENTRE, device='cuda', dtype=torch.float64)).norm(dim=1) - RADIUS).pow(2).mean().sqrt()),
                    "torch_over_simplify_mean": rec["torch_mean_ms"] / rec["simplify_mean_ms"]})
        line["cells"][f"{steps}_steps"] = rec
        if steps == 4:
            simplified = out
    line["downstream_full"] = downstream(verts, faces, args.frames, args.size)
    line["downstream_simplified_4_steps"] = downstream(simplified[0], simplified[1], args.frames, args.size)
    line["frames"], line["size"] = args.frames, args.size
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
