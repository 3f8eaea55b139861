"""Time of the isosurface extractor (csrc/isosurface.hip): nm_isosurface_count (classify, scan, the 16-byte read-back) and nm_isosurface_fill
on grids of 129^3, 257^3 and 513^3 vertices, on an off-centre sphere's distance field and on the density of synthetic.make_joiner(0) at its
median level; mesh_extract.density_grid (the net's evaluation, which is not part of the extraction) is timed apart.  HIP events around each
call, --warmup calls first, then the median of --runs.  One JSON line per (field, size).

    python tools/isosurface_time.py [--runs 20] [--warmup 3] [--sizes 129,257,513] [--fields sphere,net]

Bytes: what the extraction has to move -- the field once (4 B per vertex) with the bricks' one-vertex halo ((17/16)^3), the outputs once
(24 B per mesh vertex, 12 B per face) -- over the time of count + fill, beside the HBM peak of MI355X_MICROARCH (8.0 TB/s).  The workspace
traffic (2.5 B per grid vertex written, then read by the scan and, sparsely, by the fill) is listed separately: it is the method's own cost.
profiles/isosurface.md keeps the lines."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ml-neuman_amd"))
import torch  # noqa: E402

HBM_PEAK = 8.0e12
BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)


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
    return ts[len(ts) // 2], ts[0], ts[-1]


def sphere(n, dev):
    ax = torch.linspace(-1.0, 1.0, n, device=dev, dtype=torch.float64)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing='ij')
    return (0.6 - torch.sqrt((x - 0.013) ** 2 + (y + 0.021) ** 2 + (z - 0.017) ** 2)).to(torch.float32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="129,257,513")
    ap.add_argument("--fields", default="sphere,net")
    args = ap.parse_args()
    from neuman_hip import _lib, mesh_extract, synthetic
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.lib()
    box_c = (ctypes.c_float * 6)(*BOX)
    net = synthetic.make_joiner(0).to(dev) if "net" in args.fields.split(",") else None
    for what in args.fields.split(","):
        for n in (int(s) for s in args.sizes.split(",")):
            line = {"what": "isosurface", "field": what, "grid_vertices": [n, n, n], "runs": args.runs, "warmup": args.warmup}
            if what == "net":
                reps = 1 if n > 300 else 3
                med, lo, hi = event_ms(lambda: mesh_extract.density_grid(net, BOX, n), 1, reps)
                field = mesh_extract.density_grid(net, BOX, n)
                level = float(field.flatten()[:: max(1, field.numel() // 1000003)].median())
                line.update({"density_grid_ms": med, "density_grid_ms_min_max": [lo, hi], "density_grid_runs": reps,
                             "density_grid_samples_per_s": n ** 3 / (med * 1e-3)})
            else:
                field, level = sphere(n, dev), 0.0
            nbytes = int(L.nm_isosurface_workspace_bytes(n, n, n))
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            nv, nf = ctypes.c_int64(0), ctypes.c_int64(0)

            def count():
                _lib.check(L.nm_isosurface_count(_lib.dev_ptr(field), n, n, n, box_c, level, _lib.dev_ptr(ws, torch.uint8), nbytes, ctypes.byref(nv),
                                                 ctypes.byref(nf), _lib.stream_ptr()), "nm_isosurface_count")
            count()
            verts = torch.empty((nv.value, 3), device=dev)
            normals = torch.empty((nv.value, 3), device=dev)
            faces = torch.empty((nf.value, 3), device=dev, dtype=torch.int32)

            def fill():
                _lib.check(L.nm_isosurface_fill(_lib.dev_ptr(field), n, n, n, box_c, level, _lib.dev_ptr(ws, torch.uint8), nbytes, _lib.dev_ptr(verts),
                                                _lib.dev_ptr(normals), _lib.dev_ptr(faces, torch.int32), nv.value, nf.value, _lib.stream_ptr()),
                           "nm_isosurface_fill")

            def both():
                count()
                fill()
            c_med, c_lo, c_hi = event_ms(count, args.warmup, args.runs)
            f_med, f_lo, f_hi = event_ms(fill, args.warmup, args.runs)
            b_med, b_lo, b_hi = event_ms(both, args.warmup, args.runs)
            e_med, e_lo, e_hi = event_ms(lambda: mesh_extract.extract_mesh(field, BOX, level), args.warmup, args.runs)
            need = n ** 3 * 4 * (17 / 16) ** 3 + nv.value * 24 + nf.value * 12
            line.update({"level": level, "n_verts": nv.value, "n_faces": nf.value, "count_ms": c_med, "count_ms_min_max": [c_lo, c_hi], "fill_ms": f_med,
                         "fill_ms_min_max": [f_lo, f_hi], "count_plus_fill_ms": b_med, "count_plus_fill_ms_min_max": [b_lo, b_hi],
                         "extract_mesh_ms": e_med, "extract_mesh_ms_min_max": [e_lo, e_hi], "bytes_field_with_halo_and_outputs": need,
                         "workspace_bytes": nbytes, "bytes_per_s": need / (b_med * 1e-3), "share_of_hbm_peak_8TBps": need / (b_med * 1e-3) / HBM_PEAK,
                         "count_field_bytes_per_s": n ** 3 * 4 * (17 / 16) ** 3 / (c_med * 1e-3)})
            print(json.dumps(line), flush=True)
            del field, ws, verts, normals, faces


if __name__ == "__main__":
    main()
