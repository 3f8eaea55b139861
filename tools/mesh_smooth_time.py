"""Time of the mesh smoothing (csrc/mesh_smooth.hip) on the mesh extract_mesh makes of a sphere's signed distance on a 128^3 grid: the
adjacency (with its one read-back, as a caller sees it), 10 Taubin iterations, and the vertex normals; beside them, in the same run and
alternating with them, what a caller has without these kernels: the same umbrella operator and the same area-weighted normals written with
torch index_add_ in float64 on the same device (its index tensors built outside the timed window).  HIP events around each call on the
current stream, two warm-ups, the median of --runs.  One JSON line.

    python tools/mesh_smooth_time.py [--runs 20] [--res 128]

profiles/mesh_smooth.md keeps the line and what follows from it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ml-neuman_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
CENTRE, RADIUS = (0.013, -0.021, 0.017), 0.6
ITERATIONS, LAM, MU = 10, 0.5, -0.53


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median(ts):
    return sorted(ts)[len(ts) // 2]


class TorchBaseline:
    """the umbrella of rule S3 and the normals of rule S5 with index_add_ in float64: the same arithmetic, the sums in whatever order the
    device's atomics take them"""

    def __init__(self, faces, n_verts):
        f = faces.long()
        proper = (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])
        f = f[proper]
        self.f = f
        self.v = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
        self.p = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
        self.q = torch.cat([f[:, 2], f[:, 0], f[:, 1]])
        k = torch.bincount(self.v, minlength=n_verts)
        self.moves = (k > 0)[:, None]
        self.two_k = (2 * k.clamp(min=1)).double()[:, None]

    def step(self, x, t):
        s = torch.zeros_like(x)
        s.index_add_(0, self.v, x[self.p])
        s.index_add_(0, self.v, x[self.q])
        return torch.where(self.moves, x + t * (s / self.two_k - x), x)

    def smooth(self, rows):
        x = rows.double()
        for _ in range(ITERATIONS):
            x = self.step(x.float().double(), float(np.float32(LAM)))
            x = self.step(x.float().double(), float(np.float32(MU)))
        return x.float()

    def normals(self, verts):
        x = verts.double()
        a, b, c = x[self.f[:, 0]], x[self.f[:, 1]], x[self.f[:, 2]]
        cross = torch.linalg.cross(b - a, c - a)
        n = torch.zeros_like(x)
        for k in range(3):
            n.index_add_(0, self.f[:, k], cross)
        return (n / n.norm(dim=1, keepdim=True)).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--res", type=int, default=128)
    args = ap.parse_args()
    import isosurface_ref as IR
    from neuman_hip import _lib, mesh_extract, mesh_smooth
    _lib.require_gpu()
    torch.cuda.set_device(0)
    field = torch.from_numpy(IR.sphere_field((args.res,) * 3, BOX, CENTRE, RADIUS)).cuda()
    verts, faces, _ = mesh_extract.extract_mesh(field, BOX, 0.0)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    base = TorchBaseline(faces, V)
    adj = mesh_smooth.adjacency(faces, V)
    calls = {
        "adjacency_ms": lambda: mesh_smooth.adjacency(faces, V),
        "smooth_ms": lambda: mesh_smooth.smooth_mesh(verts, faces, ITERATIONS, LAM, MU, adj=adj),
        "torch_smooth_ms": lambda: base.smooth(verts),
    }
    smoothed = calls["smooth_ms"]()
    calls["normals_ms"] = lambda: mesh_smooth.vertex_normals(smoothed, faces, adj=adj)
    calls["torch_normals_ms"] = lambda: base.normals(smoothed)
    for _ in range(2):                                         # warm-up of every shape the timed window uses
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(args.runs):                                 # alternating: the kernels and the baseline see the same machine
        for name, fn in calls.items():
            times[name].append(timed(fn)[0])
    line = {name: median(ts) for name, ts in times.items()}
    line.update({name.replace("_ms", "_min_ms"): min(ts) for name, ts in times.items()})
    d_smooth = float((calls["torch_smooth_ms"]() - smoothed).abs().max())
    d_normals = float((calls["torch_normals_ms"]() - calls["normals_ms"]()).abs().max())
    valence = (adj.inc_off[1:] - adj.inc_off[:-1])
    line.update({"mesh": f"sphere_{args.res}", "verts": V, "faces": F, "n_incident": int(adj.inc.shape[0]), "max_valence": int(valence.max()),
                 "boundary_verts": int(adj.boundary.sum()), "iterations": ITERATIONS, "runs": args.runs,
                 "smooth_plus_normals_ms": line["smooth_ms"] + line["normals_ms"],
                 "torch_smooth_plus_normals_ms": line["torch_smooth_ms"] + line["torch_normals_ms"],
                 "max_abs_difference_smooth": d_smooth, "max_abs_difference_normals": d_normals})
    line["torch_over_kernels"] = line["torch_smooth_plus_normals_ms"] / line["smooth_plus_normals_ms"]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
