"""The bench frame's fine pass (640 000 rays x 256 samples on the bench's own sample positions): the whole-network launch (role='shading') against the
trunk / head pair (role='composite', nm_mlp_forward_rays_live) at several chunk sizes and against the pair as one persistent launch
(NEUMAN_LIVE_FUSED=1, csrc/mlp_i8f.hip) -- HIP events, best and all of 3 -- and the live fraction the device finds.  profiles/live_heads.md and
profiles/live_fused.md record runs.

--sweep: the small passes instead -- n points of the same scene (the fine net's own live fraction) through Joiner.forward, whole-network launch
against the pair (a counter reset plus two launches) inside one shared live workspace as the renderers run it, 20 launches each after 3 to warm
up, for n = 2^8 .. 2^20: the smallest n at which the pair is not slower is vanilla.LIVE_MIN_SAMPLES.  profiles/live_heads_all_passes.md records a run."""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "ml-neuman_amd"))
import torch  # noqa: E402

from neuman_hip import ray_utils, render_utils, synthetic, vanilla  # noqa: E402

dev = torch.device('cuda')
coarse, fine = synthetic.make_joiner(0).to(dev), synthetic.make_joiner(1).to(dev)
coarse.precision = fine.precision = 'mixed'


def sweep():
    vanilla.LIVE_MIN_SAMPLES = 0
    g = torch.Generator(device=dev).manual_seed(0)
    n_max = 1 << 20
    cap = synthetic.SimpleCapture(800, 800)
    o, d = ray_utils.shot_all_rays_dev(cap, dev)
    pick = torch.randint(0, o.shape[0], (n_max,), device=dev, generator=g)
    zz = float(cap.near['bkg']) + torch.rand((n_max, 1), device=dev, generator=g) * (float(cap.far['bkg']) - float(cap.near['bkg']))
    pts, dirs = (o[pick] + d[pick] * zz).contiguous(), d[pick].contiguous()

    def timed(n, role, reps=20):
        p, v = pts[:n].contiguous(), dirs[:n].contiguous()
        for _ in range(3):
            out = fine(p, v, role=role)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            out = fine(p, v, role=role)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3, out

    with torch.no_grad(), vanilla.live_workspace(n_max, dev):
        for k in range(8, 21):
            n = 1 << k
            w1, ref = timed(n, 'shading')
            l1, got = timed(n, 'composite')
            w2, _ = timed(n, 'shading')
            l2, _ = timed(n, 'composite')
            alive = ref[..., 3] > 0
            same = torch.equal(got[..., 3], ref[..., 3]) and torch.equal(got[..., :3][alive], ref[..., :3][alive])
            print(f"n 2^{k:<2d} = {n:8d}  live {alive.float().mean().item():.3f}  whole {w1:9.1f} {w2:9.1f} us  pair {l1:9.1f} {l2:9.1f} us  "
                  f"pair - whole {min(l1, l2) - min(w1, w2):+9.1f} us  live records equal: {same}", flush=True)


if '--sweep' in sys.argv:
    sweep()
    sys.exit(0)
cap = synthetic.SimpleCapture(800, 800)
o, d = ray_utils.shot_all_rays_dev(cap, dev)
R = o.shape[0]
with torch.no_grad():
    n = torch.full((R,), float(cap.near['bkg']), device=dev)
    f = torch.full((R,), float(cap.far['bkg']), device=dev)
    z, _ = render_utils.bkg_place_z(coarse, fine, o, d, n, f, 128, 128, True)
    ref = fine.forward_rays(o, d, z, role='shading')
    torch.cuda.synchronize()
    live = int((ref[..., 3] > 0).sum())
    print(f"rays {R}, samples {z.numel()}, live {live} = {live / z.numel():.4f}", flush=True)
    arms = ([('whole', dict(role='shading')), ('fused', dict(role='composite'))] + [(f'live 2^{k}', dict(role='composite', chunk_samples=1 << k)) for k in (20, 21, 22, 23, 24)]
            + [('whole', dict(role='shading')), ('fused', dict(role='composite')), ('live 2^21', dict(role='composite', chunk_samples=1 << 21))])
    for tag, kw in arms:
        os.environ['NEUMAN_LIVE_FUSED'] = '1' if tag == 'fused' else '0'           # (read per call: the one persistent launch | the pair in chunks)
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fine.forward_rays(o, d, z, **kw)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        same = torch.equal(out[..., 3], ref[..., 3]) and torch.equal(out[..., :3][ref[..., 3] > 0], ref[..., :3][ref[..., 3] > 0])
        print(f"{tag:12s} best {min(ms):7.2f} ms  all {' '.join(f'{m:.2f}' for m in ms)}  live records equal: {same}", flush=True)
        del out
