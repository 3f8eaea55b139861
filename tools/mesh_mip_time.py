"""What filtering under minification costs the frame renderer (csrc/raster_frames.hip: nm_raster_frames_lattice_mip; csrc/mesh_lattice.hip:
nm_mesh_lattice_pyramid), on the workload of tools/mesh_lattice_time.py: the sphere extract_mesh makes of a signed distance on a 128^3 grid
(some 82 000 vertices), thinned by simplify_mesh at cells of 4 grid steps, turned about the vertical axis over --frames frames, lit, with an
R = --resolution lattice and its pyramid of every level (`lattice_levels(R)`, one more than `lattice_pyramid` makes by default for a power of
two).  Four arms on the same meshes in one process, at --size x --size and at a quarter of that (the same views, so the
faces are a quarter as wide and the level choice moves two levels up):

  a  lattice, full size          nm_raster_frames_lattice: the plain lookup
  b  pyramid, full size          nm_raster_frames_lattice_mip at lod_scale 1: b minus a prices the level choice and the second lookup
  c  lattice, quarter size
  d  pyramid, quarter size

The arms alternate (a, b, c, d, a, ...) for --rounds rounds after --warmup unrecorded rounds; every arm renders the whole sequence through
`render_mesh_frames` --repeat times back to back, ends in a device synchronise and is timed by the host clock, outputs allocated inside.
Per-frame time = window / (repeat x frames); median and extremes over the rounds.  Beside them `lattice_pyramid` by itself, HIP events
around the call, the median of --rounds runs after warm-ups, and the share of covered pixels per level at both sizes (from the numpy
restatement of rule M2 on the first frame).  One JSON line per figure; --md writes the measured part of profiles/mesh_mip.md.

    timeout -k 10 600 python tools/mesh_mip_time.py [--frames 64] [--size 512] [--rounds 7] [--md profiles/mesh_mip_measured.md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ml-neuman_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mesh_lattice_time import BOX, CENTRE, RADIUS, event_ms, turned  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--resolution", type=int, default=8)
    ap.add_argument("--lod-scale", type=float, default=1.0)
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import isosurface_ref as IR
    import mesh_mip_ref as MR
    import raster_ref as RR
    from neuman_hip import _lib, mesh_extract, mesh_simplify, mesh_smooth, mesh_texture, raster, render_utils, synthetic
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    field = torch.from_numpy(IR.sphere_field((args.res,) * 3, BOX, CENTRE, RADIUS)).to(dev)
    full_v, full_f, _ = mesh_extract.extract_mesh(field, BOX, 0.0)
    cell = 4 * 2.0 / (args.res - 1)
    thin_v, thin_f = mesh_simplify.simplify_mesh(full_v, full_f, cell, aabb=BOX)
    thin_n = mesh_smooth.vertex_normals(thin_v, thin_f)
    R = args.resolution
    net = synthetic.make_joiner(0).to(dev)
    lattice = mesh_texture.bake_face_colours(net, thin_v, thin_f, thin_n, R)
    full = mesh_texture.lattice_levels(R)                                             # every level, the R = 1 one included: the most there is to build and to read
    pyramid = mesh_texture.lattice_pyramid(lattice, levels=full)
    sizes = {"full": args.size, "quarter": max(args.size // 4, 1)}
    caps = {k: [synthetic.SimpleCapture(s, s, c2w=synthetic.spherical_c2w(30., -20., 2.2)) for _ in range(args.frames)] for k, s in sizes.items()}
    batch = {k: raster.batch_cameras(c, dev) for k, c in caps.items()}
    verts, normals = turned(thin_v, thin_n, args.frames)
    faces = thin_f.cpu().numpy()

    def arm(size, colours, **kw):
        return lambda: render_utils.render_mesh_frames(verts, faces, batch[size], normals=normals, face_colours=colours, **kw)

    arms = {
        f"a lattice, {sizes['full']} x {sizes['full']}": arm("full", lattice),
        f"b pyramid, {sizes['full']} x {sizes['full']}": arm("full", pyramid, lod_scale=args.lod_scale),
        f"c lattice, {sizes['quarter']} x {sizes['quarter']}": arm("quarter", lattice),
        f"d pyramid, {sizes['quarter']} x {sizes['quarter']}": arm("quarter", pyramid, lod_scale=args.lod_scale),
    }
    times = {k: [] for k in arms}
    for r in range(args.warmup + args.rounds):
        for name, fn in arms.items():                                                 # a b c d a b c d ...: the arms share whatever the machine does meanwhile
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.repeat):
                fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3 / (args.repeat * args.frames))
    for _ in range(args.warmup):
        mesh_texture.lattice_pyramid(lattice, levels=full)
    torch.cuda.synchronize()
    build = sorted(event_ms(lambda: mesh_texture.lattice_pyramid(lattice, levels=full)) for _ in range(args.rounds))
    shares = {}
    for k in sizes:                                                                   # which levels the first frame's pixels take, per the restatement of M2
        _, face_id, _, _ = raster.rasterizer_for(faces, int(thin_v.shape[0])).render_frames(verts[:1], tuple(t[:1] if isinstance(t, torch.Tensor) else t for t in batch[k]),
                                                                                            want_geometry=True)
        fid = face_id[0].cpu().numpy()
        sv = MR.screen_vertices(verts[0].cpu().numpy(), RR.camera_of(caps[k][0]))
        l, _, _ = MR.level_of(sv, faces, fid[fid >= 0], R, pyramid.levels, args.lod_scale)
        shares[k] = (np.bincount(l, minlength=pyramid.levels) / max(l.size, 1)).round(3).tolist()
    head = {"device": torch.cuda.get_device_name(0), "thin_verts": int(thin_v.shape[0]), "thin_faces": int(thin_f.shape[0]), "R": R, "levels": pyramid.levels,
            "lattice_bytes": int(lattice.numel() * 4), "pyramid_bytes": int(pyramid.data.numel() * 4), "lod_scale": args.lod_scale, "frames": args.frames,
            "sizes": sizes, "repeat": args.repeat, "rounds": args.rounds, "warmup": args.warmup, "level_shares_first_frame": shares}
    print(json.dumps(head), flush=True)
    lines = []
    for name, ts in times.items():
        ts = sorted(ts)
        lines.append({"arm": name, "ms_per_frame_median": ts[len(ts) // 2], "ms_per_frame_min": ts[0], "ms_per_frame_max": ts[-1]})
        print(json.dumps(lines[-1]), flush=True)
    print(json.dumps({"build": "lattice_pyramid", "ms_median": build[len(build) // 2], "ms_min": build[0], "ms_max": build[-1]}), flush=True)
    if args.md:
        a, b, c, d = (line["ms_per_frame_median"] for line in lines)
        with open(args.md, "w") as f:
            f.write(f"`python tools/mesh_mip_time.py --frames {args.frames} --size {args.size} --repeat {args.repeat} --rounds {args.rounds}` on one {head['device']}: the sphere of "
                    f"`tools/mesh_lattice_time.py` thinned at 4 grid steps to {head['thin_verts']} vertices and {head['thin_faces']} faces; the R = {R} lattice is "
                    f"{head['lattice_bytes'] / 2 ** 20:.2f} MiB, its pyramid of {pyramid.levels} levels {head['pyramid_bytes'] / 2 ** 20:.2f} MiB.  {args.frames} lit frames, "
                    f"lod_scale {args.lod_scale}.  The arms alternate in one process, {args.warmup} unrecorded rounds first; a timed window is the sequence {args.repeat} times "
                    f"back to back, per-frame time = window / ({args.repeat} x {args.frames}) (host clock, device synchronise at the end).  Share of the first frame's "
                    f"covered pixels per level 0 .. {pyramid.levels - 1}: {shares['full']} at full size, {shares['quarter']} at a quarter.\n\n")
            f.write("| arm | ms per frame (median) | min | max |\n|---|---|---|---|\n")
            for line in lines:
                f.write(f"| {line['arm']} | {line['ms_per_frame_median']:.4f} | {line['ms_per_frame_min']:.4f} | {line['ms_per_frame_max']:.4f} |\n")
            f.write(f"\n| build (HIP events) | ms (median) | min | max |\n|---|---|---|---|\n| lattice_pyramid | {build[len(build) // 2]:.3f} | {build[0]:.3f} | {build[-1]:.3f} |\n")
            f.write(f"\nThe pyramid costs {b - a:+.4f} ms per frame at full size ({b / a:.2f} x the plain lattice) and {d - c:+.4f} at a quarter ({d / c:.2f} x).\n")


if __name__ == "__main__":
    main()
