"""What a colour lattice costs the frame renderer and what it saves (csrc/raster_frames.hip: nm_raster_frames_lattice; csrc/mesh_lattice.hip), on
the mesh of tools/mesh_simplify_time.py: the sphere extract_mesh makes of a signed distance on a 128^3 grid (some 82 000 vertices), thinned by
simplify_mesh at cells of 4 grid steps, turned about the vertical axis over --frames frames at --size x --size, lit.  Three arms on the same
cameras in one process:

  a  thinned, vertex colours     the thinned mesh with one colour per vertex through nm_raster_frames: the cheap preview of today
  b  thinned, R = 8 lattice      the same mesh with an R = --resolution lattice through nm_raster_frames_lattice: a minus b prices the lookup
  c  full, vertex colours        the unthinned mesh with one colour per vertex: what a caller draws today for comparable colour detail

The arms alternate (a, b, c, a, ...) for --rounds rounds after --warmup unrecorded rounds; every arm renders the whole sequence through
`render_mesh_frames` --repeat times back to back (a thinned sequence alone takes well under a millisecond: too short a window), ends in a
device synchronise and is timed by the host clock, outputs allocated inside.  Per-frame time = window / (repeat x frames); median and extremes
over the rounds.  Beside them the bake of the lattice by itself, HIP events around the call, the median of --rounds
runs after warm-ups: `lattice_rows` alone (one set of node rows, w = 3) and `bake_face_colours` with a synthetic net as the source (two sets
of node rows and the net's forward at every node).  One JSON line per figure; --md writes the measured part of profiles/mesh_lattice.md.

    timeout -k 10 600 python tools/mesh_lattice_time.py [--frames 64] [--size 512] [--rounds 7] [--md profiles/mesh_lattice_measured.md]
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

BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
CENTRE, RADIUS = (0.013, -0.021, 0.017), 0.6


def turned(verts, normals, frames):
    """the mesh turned about the y axis over half a turn -> (verts [B,V,3], normals [B,V,3])"""
    ang = torch.linspace(0.0, np.pi, frames, device=verts.device, dtype=torch.float64)
    R = torch.zeros((frames, 3, 3), device=verts.device, dtype=torch.float64)
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = torch.cos(ang), torch.sin(ang), 1.0, -torch.sin(ang), torch.cos(ang)
    turn = lambda x: torch.einsum('bij,vj->bvi', R, x.double()).float().contiguous()      # noqa: E731
    return turn(verts), turn(normals)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--resolution", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import isosurface_ref as IR
    from neuman_hip import _lib, mesh_extract, mesh_simplify, mesh_smooth, mesh_texture, raster, render_utils, synthetic
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    field = torch.from_numpy(IR.sphere_field((args.res,) * 3, BOX, CENTRE, RADIUS)).to(dev)
    full_v, full_f, full_n = mesh_extract.extract_mesh(field, BOX, 0.0)
    cell = 4 * 2.0 / (args.res - 1)
    thin_v, thin_f = mesh_simplify.simplify_mesh(full_v, full_f, cell, aabb=BOX)
    thin_n = mesh_smooth.vertex_normals(thin_v, thin_f)
    R = args.resolution
    net = synthetic.make_joiner(0).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    colours = {"full": torch.rand((full_v.shape[0], 3), device=dev, generator=gen), "thin": torch.rand((thin_v.shape[0], 3), device=dev, generator=gen)}
    lattice = mesh_texture.bake_face_colours(net, thin_v, thin_f, thin_n, R)
    caps = [synthetic.SimpleCapture(args.size, args.size, c2w=synthetic.spherical_c2w(30., -20., 2.2)) for _ in range(args.frames)]
    batch = raster.batch_cameras(caps, dev)
    seq = {"full": turned(full_v, full_n, args.frames), "thin": turned(thin_v, thin_n, args.frames)}
    faces = {"full": full_f.cpu().numpy(), "thin": thin_f.cpu().numpy()}
    arms = {
        "a thinned, vertex colours": lambda: render_utils.render_mesh_frames(seq["thin"][0], faces["thin"], batch, colours=colours["thin"], normals=seq["thin"][1]),
        f"b thinned, R = {R} lattice": lambda: render_utils.render_mesh_frames(seq["thin"][0], faces["thin"], batch, normals=seq["thin"][1], face_colours=lattice),
        "c full, vertex colours": lambda: render_utils.render_mesh_frames(seq["full"][0], faces["full"], batch, colours=colours["full"], normals=seq["full"][1]),
    }
    times = {k: [] for k in arms}
    for r in range(args.warmup + args.rounds):
        for name, fn in arms.items():                                                 # a b c a b c ...: the arms share whatever the machine does meanwhile
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.repeat):
                fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3 / (args.repeat * args.frames))
    covered = int((list(arms.values())[1]() != 255).any(-1).sum()) // args.frames
    bakes = {
        "lattice_rows, w = 3": lambda: mesh_texture.lattice_rows(thin_v, thin_f, R),
        "bake_face_colours, synthetic net": lambda: mesh_texture.bake_face_colours(net, thin_v, thin_f, thin_n, R),
    }
    bake_ms = {}
    for name, fn in bakes.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        bake_ms[name] = sorted(event_ms(fn) for _ in range(args.rounds))
    head = {"device": torch.cuda.get_device_name(0), "full_verts": int(full_v.shape[0]), "full_faces": int(full_f.shape[0]), "thin_verts": int(thin_v.shape[0]),
            "thin_faces": int(thin_f.shape[0]), "R": R, "nodes": int(lattice.shape[0] * lattice.shape[1]), "lattice_bytes": int(lattice.numel() * 4),
            "frames": args.frames, "size": args.size, "repeat": args.repeat, "rounds": args.rounds, "warmup": args.warmup, "covered_pixels_per_frame": covered}
    print(json.dumps(head), flush=True)
    lines = []
    for name, ts in times.items():
        ts = sorted(ts)
        lines.append({"arm": name, "ms_per_frame_median": ts[len(ts) // 2], "ms_per_frame_min": ts[0], "ms_per_frame_max": ts[-1]})
        print(json.dumps(lines[-1]), flush=True)
    for name, ts in bake_ms.items():
        lines.append({"bake": name, "ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1]})
        print(json.dumps(lines[-1]), flush=True)
    if args.md:
        a, b, c = (line["ms_per_frame_median"] for line in lines[:3])
        with open(args.md, "w") as f:
            f.write(f"`python tools/mesh_lattice_time.py --frames {args.frames} --size {args.size} --repeat {args.repeat} --rounds {args.rounds}` on one {head['device']}: the sphere of "
                    f"`tools/mesh_simplify_time.py`, {head['full_verts']} vertices and {head['full_faces']} faces, thinned at 4 grid steps to {head['thin_verts']} "
                    f"vertices and {head['thin_faces']} faces; an R = {R} lattice is {head['nodes']} nodes, {head['lattice_bytes'] / 2 ** 20:.1f} MiB.  "
                    f"{args.frames} frames of {args.size} x {args.size}, lit, {covered} pixels per frame show the mesh.  The arms alternate in one process, "
                    f"{args.warmup} unrecorded rounds first; a timed window is the sequence {args.repeat} times back to back, per-frame time = window / "
                    f"({args.repeat} x {args.frames}) (host clock, device synchronise at the end).\n\n")
            f.write("| arm | ms per frame (median) | min | max |\n|---|---|---|---|\n")
            for line in lines[:3]:
                f.write(f"| {line['arm']} | {line['ms_per_frame_median']:.4f} | {line['ms_per_frame_min']:.4f} | {line['ms_per_frame_max']:.4f} |\n")
            f.write("\n| bake (HIP events) | ms (median) | min | max |\n|---|---|---|---|\n")
            for line in lines[3:]:
                f.write(f"| {line['bake']} | {line['ms_median']:.3f} | {line['ms_min']:.3f} | {line['ms_max']:.3f} |\n")
            nearer = abs(b - a) < abs(c - b)
            f.write(f"\nThe lookup costs {b - a:+.4f} ms per frame ({b / a:.2f} x arm a); the unthinned mesh costs {c / a:.2f} x arm a.  "
                    + ("Arm b sits nearer a than c, as expected." if nearer else "Arm b does NOT sit nearer a than c: the expectation fails here.") + "\n")


if __name__ == "__main__":
    main()
