"""Time of the mesh clean-up (csrc/mesh_components.hip) entry point by entry point, on the mesh of the grid tests/helpers/mesh_sizes.py names
PRODUCTION_MESH (a gyroid's level set) and on the disjoint triangles of tests/helpers/component_sizes.py; beside them, on the same grid in the
same run, nm_isosurface_count + nm_isosurface_fill (the extraction the clean-up follows) and the numpy restatement's wall time on the host.
HIP events around each call on the current stream, one warm-up, the median of --runs; the two entry points that read back are timed with their
synchronisation, as a caller sees them.  One JSON line per mesh.

    python tools/mesh_clean_time.py [--runs 20]

profiles/mesh_components.md keeps the lines and what follows from them.
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


def event_ms(fn, runs):
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
    return sorted(ts)[len(ts) // 2]


def time_mesh(name, faces_np, n_verts, verts_np, runs):
    import mesh_components_ref as MR
    from neuman_hip import _lib
    L = _lib.lib()
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = lambda: _lib.stream_ptr()
    I32 = torch.int32
    F, V = int(faces_np.shape[0]), int(n_verts)
    faces = torch.from_numpy(faces_np).cuda()
    verts = torch.from_numpy(verts_np).cuda()
    nbytes = int(L.nm_mesh_components_workspace_bytes(V, F))
    ws = torch.empty((nbytes,), device='cuda', dtype=torch.uint8)
    vl, fl = torch.empty((V,), device='cuda', dtype=I32), torch.empty((F,), device='cuda', dtype=I32)
    n = ctypes.c_int64(0)
    label = lambda: _lib.check(L.nm_mesh_components(P(faces), F, V, P(vl), P(fl), P(ws), nbytes, ctypes.byref(n), st()), "nm_mesh_components")
    t_label = event_ms(label, runs)
    C = int(n.value)
    cv, cf = torch.empty((C,), device='cuda', dtype=I32), torch.empty((C,), device='cuda', dtype=I32)
    cb = torch.empty((C, 6), device='cuda', dtype=torch.float32)
    t_stats = event_ms(lambda: _lib.check(L.nm_mesh_component_stats(P(faces), F, V, P(vl), P(verts), C, P(cv), P(cf), P(cb), st()), "stats"), runs)
    keep = torch.zeros((C,), device='cuda', dtype=torch.uint8)
    keep[int(cf.argmax())] = 1                                                        # the largest component alone
    nv, nf = ctypes.c_int64(0), ctypes.c_int64(0)
    mesh = (P(faces), F, V, P(vl), P(keep), C, P(ws), nbytes)
    count = lambda: _lib.check(L.nm_mesh_select_count(*mesh, ctypes.byref(nv), ctypes.byref(nf), st()), "nm_mesh_select_count")
    t_count = event_ms(count, runs)
    src = torch.empty((int(nv.value),), device='cuda', dtype=I32)
    out = torch.empty((int(nf.value), 3), device='cuda', dtype=I32)
    t_fill = event_ms(lambda: _lib.check(L.nm_mesh_select_fill(*mesh, P(src), P(out), int(nv.value), int(nf.value), st()), "nm_mesh_select_fill"), runs)
    g = torch.empty((int(nv.value), 3), device='cuda', dtype=torch.float32)
    t_gather = event_ms(lambda: _lib.check(L.nm_gather_rows(P(verts), P(src), None, int(nv.value), 3, P(g), st()), "nm_gather_rows"), runs)
    t_bytes = event_ms(lambda: L.nm_mesh_components_workspace_bytes(V, F), runs)
    t0 = time.perf_counter()
    r_vl, r_fl, r_n = MR.labels(faces_np, V)
    r_stats = MR.stats(faces_np, r_vl, r_n, verts_np)
    MR.select(faces_np, r_vl, np.arange(r_n) == int(r_stats[1].argmax()))
    t_numpy = (time.perf_counter() - t0) * 1e3
    assert r_n == C and np.array_equal(r_vl, vl.cpu().numpy())
    return {"mesh": name, "verts": V, "faces": F, "components": C, "kept_verts": int(nv.value), "kept_faces": int(nf.value), "runs": runs,
            "workspace_bytes": nbytes, "nm_mesh_components_workspace_bytes_ms": t_bytes, "nm_mesh_components_ms": t_label,
            "nm_mesh_component_stats_ms": t_stats, "nm_mesh_select_count_ms": t_count, "nm_mesh_select_fill_ms": t_fill, "gather_verts_ms": t_gather,
            "clean_up_ms": t_label + t_stats + t_count + t_fill + t_gather, "numpy_restatement_ms": t_numpy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    args = ap.parse_args()
    import component_sizes as CS
    import isosurface_ref as IR
    import mesh_sizes as MS
    from neuman_hip import _lib, mesh_extract
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dims, freq, level = MS.ISO_CASES[MS.PRODUCTION_MESH]
    field = torch.from_numpy(IR.gyroid_field(dims, MS.ISO_BOX, freq)).cuda()
    t_extract = event_ms(lambda: mesh_extract.extract_mesh(field, MS.ISO_BOX, level), args.runs)     # nm_isosurface_count + nm_isosurface_fill and the allocations between
    verts, faces, _ = mesh_extract.extract_mesh(field, MS.ISO_BOX, level)
    line = time_mesh(MS.PRODUCTION_MESH, faces.cpu().numpy(), verts.shape[0], verts.cpu().numpy(), args.runs)
    line.update({"grid": list(dims), "isosurface_count_and_fill_ms": t_extract, "clean_up_over_extraction": line["clean_up_ms"] / t_extract})
    print(json.dumps(line), flush=True)
    V = CS.DISJOINT_VERTS
    rng = np.random.default_rng(0)
    print(json.dumps(time_mesh("disjoint_triangles", CS.disjoint_triangles(V), V, rng.normal(size=(V, 3)).astype(np.float32), args.runs)), flush=True)


if __name__ == "__main__":
    main()
