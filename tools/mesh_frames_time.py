"""Time of a rasterised preview of an animated, coloured mesh by two routes, on the same data in one process:

  loop    what a caller could write before nm_raster_frames existed: per frame one `Rasterizer.rasterize` (nm_raster_mesh: one call and one
          blocking 4-byte read-back), then in torch the gather of the vertex colours through face_id and bary, the byte conversion and the
          select over a white background
  frames  `render_utils.render_mesh_frames` (csrc/raster_frames.hip: nm_raster_frames, the sequence in chunks of `mesh_frames_per_call`
          frames, one read-back per chunk), without normals as the loop has none; a third arm adds the diffuse light on per-frame normals

The sequence is synthetic: synthetic.capsule_mesh(--rings, --segments) (312 000 faces by default) turned about its long axis a little more
every frame, random vertex colours, one camera, --frames frames at --size x --size.  The arms alternate (loop, frames, lit, loop, ...) for
--rounds rounds after --warmup unrecorded rounds; every arm ends in a device synchronise and is timed by the host clock around the whole
sequence, outputs allocated inside (they are part of both routes).  Per-frame time = sequence time / frames; median and extremes over the
rounds.  The two routes' bytes are compared on the way (torch's blend associates as the kernel's does, but the comparison is reported, not
assumed).  One JSON line per arm; --md writes the table profiles/mesh_frames.md keeps.

    timeout -k 10 900 python tools/mesh_frames_time.py [--frames 64] [--size 512] [--rounds 7] [--md profiles/mesh_frames.md]
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


def sequence(rings, segments, frames, size, dev):
    """-> (verts [B,V,3], normals [B,V,3], colours [V,3], faces int32 [F,3] (numpy), faces on the device, captures)"""
    from neuman_hip import synthetic
    base, faces = synthetic.capsule_mesh(rings, segments)
    faces = faces.astype(np.int32)
    radius = np.array([0.25, 0.6, 0.15])
    nrm = base.astype(np.float64) / radius ** 2                                       # the ellipsoid's gradient: its outward normal
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ang = np.linspace(0.0, np.pi, frames)
    R = np.stack([np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) for a in ang])
    verts = torch.from_numpy(np.einsum('bij,vj->bvi', R, base.astype(np.float64)).astype(np.float32)).to(dev)
    normals = torch.from_numpy(np.einsum('bij,vj->bvi', R, nrm).astype(np.float32)).to(dev)
    colours = torch.from_numpy(np.random.default_rng(0).random((len(base), 3)).astype(np.float32)).to(dev)
    caps = [synthetic.SimpleCapture(size, size, c2w=synthetic.spherical_c2w(30., -20., 1.9)) for _ in range(frames)]
    return verts, normals, colours, faces, torch.from_numpy(faces).to(dev), caps


def loop_route(rast, verts, cams, colours, faces_dev):
    out = []
    for b in range(verts.shape[0]):
        face_id, _, bary, _ = rast.rasterize(verts[b], cams[b])
        covered = face_id >= 0
        corner = colours[faces_dev[face_id.clamp(min=0).long()].long()]               # [H,W,3 corners,3 channels]
        c = (bary[..., 0:1] * corner[..., 0, :] + bary[..., 1:2] * corner[..., 1, :]) + bary[..., 2:3] * corner[..., 2, :]
        byte = (c * 255.0).clamp(0.0, 255.0).to(torch.uint8)
        out.append(torch.where(covered[..., None], byte, torch.full_like(byte, 255)))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rings", type=int, default=400)
    ap.add_argument("--segments", type=int, default=390)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    from neuman_hip import _lib, raster, render_utils
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    verts, normals, colours, faces, faces_dev, caps = sequence(args.rings, args.segments, args.frames, args.size, dev)
    B, V, F = int(verts.shape[0]), int(verts.shape[1]), int(faces.shape[0])
    rast = raster.rasterizer_for(faces, V)
    cams = [raster.camera_of(c) for c in caps]
    batch = raster.batch_cameras(caps, dev)
    arms = {
        "loop": lambda: loop_route(rast, verts, cams, colours, faces_dev),
        "frames": lambda: render_utils.render_mesh_frames(verts, faces, batch, colours=colours),
        "frames, lit": lambda: render_utils.render_mesh_frames(verts, faces, batch, colours=colours, normals=normals),
    }
    times = {k: [] for k in arms}
    for r in range(args.warmup + args.rounds):
        for name, fn in arms.items():                                                 # A B C A B C ...: the arms share whatever the machine does meanwhile
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3 / B)
    a, b = arms["loop"]().cpu().numpy(), arms["frames"]().cpu().numpy()
    differ = int((a != b).any(-1).sum())
    worst = int(np.abs(a.astype(np.int32) - b).max())
    covered = int((b != 255).any(-1).sum())
    head = {"device": torch.cuda.get_device_name(0), "verts": V, "faces": F, "frames": B, "size": args.size, "rounds": args.rounds, "warmup": args.warmup,
            "frames_per_call": min(B, render_utils.mesh_frames_per_call(V, F, args.size, args.size)), "pixels_not_white": covered,
            "pixels_where_the_routes_differ": differ, "largest_byte_difference": worst}
    print(json.dumps(head), flush=True)
    lines = []
    for name, ts in times.items():
        ts = sorted(ts)
        lines.append({"arm": name, "ms_per_frame_median": ts[len(ts) // 2], "ms_per_frame_min": ts[0], "ms_per_frame_max": ts[-1]})
        print(json.dumps(lines[-1]), flush=True)
    if args.md:
        med = {line["arm"]: line["ms_per_frame_median"] for line in lines}
        ratio = med["loop"] / med["frames"]
        with open(args.md, "w") as f:
            f.write("# Mesh frames (`csrc/raster_frames.hip`): a rasterised preview of an animated mesh, two routes\n\n")
            f.write(f"`python tools/mesh_frames_time.py --frames {B} --size {args.size} --rounds {args.rounds}` on one {head['device']}: the arms alternate in one "
                    f"process, {args.warmup} unrecorded rounds first; each arm renders the whole sequence, ends in a device synchronise and is timed by the "
                    f"host clock, outputs allocated inside; per-frame time = sequence time / frames, so a timed window is {B} times the figures below.  "
                    "Nothing in the tests depends on these numbers.\n\n")
            f.write(f"The sequence: `synthetic.capsule_mesh({args.rings}, {args.segments})`, {V} vertices, {F} faces, turned about its long axis over {B} frames, "
                    f"random vertex colours, {args.size} x {args.size}; {covered // B} pixels per frame show the mesh on average.  `loop` is the route a caller "
                    "had before: per frame one `Rasterizer.rasterize` (one call, one blocking read-back), a torch gather of the colours through `face_id` "
                    f"and `bary`, a byte conversion.  `frames` is `render_mesh_frames` ({head['frames_per_call']} frames per call by its default).\n\n")
            f.write("| arm | ms per frame (median) | min | max |\n|---|---|---|---|\n")
            for line in lines:
                f.write(f"| {line['arm']} | {line['ms_per_frame_median']:.3f} | {line['ms_per_frame_min']:.3f} | {line['ms_per_frame_max']:.3f} |\n")
            verdict = (f"`frames` takes {1 / ratio:.2f} of `loop`'s time per frame ({ratio:.2f} x faster)." if ratio > 1 else
                       f"The batch is NOT faster here: `frames` takes {1 / ratio:.2f} of `loop`'s time per frame.")
            f.write(f"\n{verdict}  The two routes' images differ in {differ} of {B * args.size * args.size} pixels (largest byte difference {worst}).\n")


if __name__ == "__main__":
    main()
