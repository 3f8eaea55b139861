"""What packing a texture atlas and sampling it cost (csrc/mesh_atlas.hip: nm_mesh_atlas_pack, nm_mesh_atlas_sample), on the mesh of
tools/mesh_lattice_time.py: the sphere extract_mesh makes of a signed distance on a 128^3 grid (some 82 000 vertices), thinned by simplify_mesh
at cells of 4 grid steps, with an R = --resolution lattice.  Arms, alternating in one process:

  a  pack_atlas                  one launch, one thread per texel
  b  torch advanced indexing     the same packing from index tables made beforehand (not timed): three gathers of node rows, an add, a
                                 subtract and two selects per texel; its atlas must equal arm a's bit for bit
  c  sample_atlas                on the face_id and bary `Rasterizer.render_frames(want_geometry=True)` returns for --frames frames of
                                 --size x --size (every pixel a point; the uncovered ones answer (0, 0, 0) and read nothing)

The arms alternate (a, b, c, a, ...) for --rounds rounds after --warmup unrecorded rounds; a timed window is the call --repeat (a, b) or
--repeat-sample (c) times back to back, outputs allocated inside, ending in a device synchronise, by the host clock.  Time per call = window /
repeats; median and extremes over the rounds.  One JSON line per figure; --md writes the measured part of profiles/mesh_atlas.md.

    timeout -k 10 600 python tools/mesh_atlas_time.py [--frames 64] [--size 512] [--rounds 7] [--md profiles/mesh_atlas_measured.md]
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


def index_tables(F, R, dev):
    """what arm b gathers by, per texel of the atlas in row order: the flat node rows a, b, c [H W] int64 (value = a for a node texel and the
    corner gutter's copy, (a + b) - c for a gutter texel), gutter [H W] bool, used [H W] bool"""
    import mesh_atlas_ref as AR
    import mesh_lattice_ref as LR
    W, H, nbx = AR.atlas_size(F, R)
    BW, BH = AR.block(R)
    owner, kind = AR.owners(F, R)
    Y, X = np.indices((H, W))
    x, y = X % BW, Y % BH
    upper = kind >= AR.UPPER_GUTTER
    x, y = np.where(upper, R + 3 - x, x), np.where(upper, R - y, y)                    # the face's own local texel
    used = owner >= 0
    corner = used & (x == R + 1)
    gutter = used & (x + y == R + 1) & ~corner
    S = LR.lattice_size(R)
    base = np.maximum(owner, 0) * S

    def node(i1, i2, where):                                                           # node 0 of face 0 where the table is gathered but not used
        return np.where(where, base + LR.node_index(R, np.where(where, i1, 0), np.where(where, i2, 0)), 0)

    a = np.where(gutter, node(x, y - 1, gutter), node(np.where(corner, R, x), y, used & ~gutter))
    b, c = node(x - 1, y, gutter), node(x - 1, y - 1, gutter)
    assert min(a.min(), b.min(), c.min()) >= 0 and max(a.max(), b.max(), c.max()) < F * S
    as_dev = lambda t, dt: torch.from_numpy(np.ascontiguousarray(t.reshape(-1))).to(dev, dt)       # noqa: E731
    return as_dev(a, torch.int64), as_dev(b, torch.int64), as_dev(c, torch.int64), as_dev(gutter, torch.bool), as_dev(owner >= 0, torch.bool), (H, W)


def torch_pack(face_colours, tables):
    a, b, c, gutter, used, (H, W) = tables
    rows = face_colours.reshape(-1, 3)
    value = torch.where(gutter[:, None], (rows[a] + rows[b]) - rows[c], rows[a])
    return torch.where(used[:, None], value, torch.zeros((), device=rows.device)).reshape(H, W, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--resolution", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=2000)
    ap.add_argument("--repeat-sample", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import isosurface_ref as IR
    from neuman_hip import _lib, mesh_export, mesh_extract, mesh_simplify, mesh_smooth, mesh_texture, raster, synthetic
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    field = torch.from_numpy(IR.sphere_field((args.res,) * 3, BOX, CENTRE, RADIUS)).to(dev)
    full_v, full_f, _ = mesh_extract.extract_mesh(field, BOX, 0.0)
    thin_v, thin_f = mesh_simplify.simplify_mesh(full_v, full_f, 4 * 2.0 / (args.res - 1), aabb=BOX)
    thin_n = mesh_smooth.vertex_normals(thin_v, thin_f)
    R, F = args.resolution, int(thin_f.shape[0])
    lattice = mesh_texture.bake_face_colours(synthetic.make_joiner(0).to(dev), thin_v, thin_f, thin_n, R)
    W, H, _ = mesh_export.atlas_size(F, R)
    tables = index_tables(F, R, dev)
    atlas = mesh_export.pack_atlas(lattice)
    same = bool(torch.equal(atlas.view(torch.int32), torch_pack(lattice, tables).view(torch.int32)))
    caps = [synthetic.SimpleCapture(args.size, args.size, c2w=synthetic.spherical_c2w(30., -20., 2.2)) for _ in range(args.frames)]
    ang = torch.linspace(0.0, np.pi, args.frames, device=dev, dtype=torch.float64)                # the mesh turned about the y axis over half a turn
    turn = torch.zeros((args.frames, 3, 3), device=dev, dtype=torch.float64)
    turn[:, 0, 0], turn[:, 0, 2], turn[:, 1, 1], turn[:, 2, 0], turn[:, 2, 2] = torch.cos(ang), torch.sin(ang), 1.0, -torch.sin(ang), torch.cos(ang)
    world = torch.einsum('bij,vj->bvi', turn, thin_v.double()).float().contiguous()
    _, face_id, _, bary = raster.rasterizer_for(thin_f.cpu().numpy(), int(thin_v.shape[0])).render_frames(world, raster.batch_cameras(caps, dev), want_geometry=True)
    points, covered = face_id.numel(), int((face_id >= 0).sum())
    arms = {
        "a pack_atlas": (lambda: mesh_export.pack_atlas(lattice), args.repeat),
        "b torch advanced indexing": (lambda: torch_pack(lattice, tables), args.repeat),
        "c sample_atlas": (lambda: mesh_export.sample_atlas(atlas, F, R, face_id, bary), args.repeat_sample),
    }
    times = {k: [] for k in arms}
    for r in range(args.warmup + args.rounds):
        for name, (fn, repeat) in arms.items():                                       # a b c a b c ...: the arms share whatever the machine does meanwhile
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(repeat):
                fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3 / repeat)
    head = {"device": torch.cuda.get_device_name(0), "thin_verts": int(thin_v.shape[0]), "faces": F, "R": R, "atlas": [W, H], "atlas_bytes": W * H * 12,
            "lattice_bytes": int(lattice.numel() * 4), "torch_pack_same_bits": same, "frames": args.frames, "size": args.size, "points": points,
            "covered_points": covered, "repeat": args.repeat, "repeat_sample": args.repeat_sample, "rounds": args.rounds, "warmup": args.warmup}
    print(json.dumps(head), flush=True)
    lines = []
    for name, ts in times.items():
        ts = sorted(ts)
        lines.append({"arm": name, "ms_per_call_median": ts[len(ts) // 2], "ms_per_call_min": ts[0], "ms_per_call_max": ts[-1]})
        print(json.dumps(lines[-1]), flush=True)
    if not same:
        raise SystemExit("arm b's atlas is not arm a's")
    if args.md:
        a, b, c = (line["ms_per_call_median"] for line in lines)
        moved = 16 * points + 12 * covered                                             # face_id read and out written; bary read where covered; the texels apart
        with open(args.md, "w") as f:
            f.write(f"`python tools/mesh_atlas_time.py --frames {args.frames} --size {args.size} --repeat {args.repeat} --repeat-sample {args.repeat_sample} --rounds "
                    f"{args.rounds}` on one {head['device']}: the sphere of `tools/mesh_lattice_time.py` thinned to {head['thin_verts']} vertices and {F} faces; its "
                    f"R = {R} lattice ({head['lattice_bytes'] / 2 ** 20:.1f} MiB) packs into an atlas of {W} x {H} texels ({W * H * 12 / 2 ** 20:.1f} MiB as float32).  "
                    f"The sampler's points are the {args.frames} x {args.size} x {args.size} = {points} pixels of the rasteriser's geometry, {covered} of them on the "
                    f"mesh.  The arms alternate in one process, {args.warmup} unrecorded rounds first; a timed window is the call {args.repeat} (a, b) or "
                    f"{args.repeat_sample} (c) times back to back (host clock, device synchronise at the end).  Arm b's atlas equals arm a's bit for bit.\n\n")
            f.write("| arm | ms per call (median) | min | max |\n|---|---|---|---|\n")
            for line in lines:
                f.write(f"| {line['arm']} | {line['ms_per_call_median']:.4f} | {line['ms_per_call_min']:.4f} | {line['ms_per_call_max']:.4f} |\n")
            f.write(f"\nThe torch packing takes {b / a:.2f} x `pack_atlas`'s time.  `sample_atlas` needs {moved / 1e6:.0f} MB per call (16 bytes a point, 12 more where "
                    f"the mesh covers it, the texels apart), {moved / (c * 1e-3) / 1e9:.0f} GB/s over the whole call.\n")


if __name__ == "__main__":
    main()
