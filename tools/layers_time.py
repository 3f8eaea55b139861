"""Time nm_merge_composite_layers against nm_merge_composite_lists on the shape of merge_composite_kernel's own comment (csrc/ray_ops.hip):
524 288 rays x (320 + 3 x 192) merged samples.  Device events, one process: warm up, then the two kernels ALTERNATE, median of 7 each.
Prints one JSON line (profiles/layers.md records it).

    python tools/layers_time.py [--rays 524288] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-neuman_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from neuman_hip import _lib, render_utils as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=524288)
    ap.add_argument("--sizes", type=int, nargs="+", default=[320, 192, 192, 192])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    g = torch.Generator(device='cuda').manual_seed(0)
    zs, raws = [], []
    for i, S in enumerate(a.sizes):
        zs.append(torch.sort(torch.rand((a.rays, S), device='cuda', generator=g) * 3.0 + 0.3 * i, dim=1)[0].contiguous())
        raws.append((torch.randn((a.rays, S, 4), device='cuda', generator=g) * torch.tensor([1., 1., 1., 4.], device='cuda')).contiguous())
    d = torch.nn.functional.normalize(torch.randn((a.rays, 3), device='cuda', generator=g), dim=-1).contiguous()
    runs = {'nm_merge_composite_lists': lambda: R.merge_composite_lists(zs, raws, d, True),
            'nm_merge_composite_lists_wide': lambda: R.merge_composite_lists_wide(zs, raws, d, True),
            'nm_merge_composite_layers': lambda: R.merge_composite_layers(zs, raws, d, True)}
    for f in runs.values():                                        # warm up (and the output allocations of the caching allocator)
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {n: [] for n in runs}
    for _ in range(7):
        for n, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1))
    ref, lay = runs['nm_merge_composite_lists'](), runs['nm_merge_composite_layers']()
    line = dict(rays=a.rays, sizes=a.sizes, device=torch.cuda.get_device_name(0), same_bits=all(torch.equal(x, y) for x, y in zip(ref, lay[:3])),
                median_ms={n: round(statistics.median(v), 3) for n, v in ms.items()}, all_ms={n: [round(x, 3) for x in v] for n, v in ms.items()})
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
