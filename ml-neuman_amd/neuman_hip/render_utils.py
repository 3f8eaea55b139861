"""HIP-backed mirror of the reference's utils/render_utils.py:69-461.

Same public signatures and return conventions (numpy float32 frames) as the reference's raw2outputs and
its four frame renderers.  What differs is the execution plan:

* the reference loops over `rays_per_batch` chunks with 6-8 host<->device copies each; here a frame is
  rendered in launches of up to `MAX_RAYS_PER_LAUNCH` rays (rays are independent, so chunking never changes a
  pixel) and nothing returns to the host before the frame is assembled;
* pts/dirs are never materialised for camera-ray passes: the MLP kernel builds `o + d*z` itself;
* boolean-mask indexing is a ballot/prefix-sum compaction + row gather/scatter on the device;
* rays are generated on the device too (the reference's f64 chain per ray, `nm_shot_rays`): 25 doubles cross the
  boundary per frame instead of 15 MB of rays.

The `*_rays` functions work on device tensors (what bench.py and the multi-GPU path call); the reference
named functions wrap them with ray generation and the final download.
"""
import contextlib
import ctypes
import os

import numpy as np
import torch

from . import _lib, occupancy, parallel, ray_utils, vanilla
from .ray_utils import DEFAULT_GEO_THRESH

MAX_RAYS_PER_LAUNCH = int(os.environ.get("NEUMAN_MAX_RAYS_PER_LAUNCH", 1 << 20))
# Early ray termination in the shading pass of the background renderers (march_pass_rays): rays whose transmittance has fallen
# below this are not evaluated any further.  0 = off: every sample is evaluated, as the reference does (render_utils.py:139-151),
# and the frame is bit-identical to the unchunked path.  eps > 0 changes a pixel by at most eps per channel.
TERMINATION_EPS = float(os.environ.get("NEUMAN_TERMINATION_EPS", "0"))
TERMINATION_CHUNK = int(os.environ.get("NEUMAN_TERMINATION_CHUNK", "32"))
# With termination on, the COARSE pass of a two-pass render is marched too, at this transmittance whatever eps is: the weights it then
# never computes are all below it, and 4e-13 is less than half a float32 ulp of the 1e-5 that sample_pdf adds to every weight
# (ray_utils.py:168: spacing of float32 at 1e-5 = 9.1e-13) -- `weights + 1e-5` is the same float32 number with or without them, so
# the importance samples are BIT-IDENTICAL to the full evaluation's.  (A cut at eps * 1e-3 = 1e-7 was tried first: it perturbs the
# CDF at float32-rounding level, which the inverse CDF amplifies in near-empty bins: 1.6e-4 on the worst pixel of a frame.)
TERMINATION_COARSE = float(os.environ.get("NEUMAN_TERMINATION_COARSE", "4e-13"))
TERMINATION_MIN_CHUNK = 16
# Early ray termination TOGETHER with an occupancy grid on a background net: the marched passes (march_pass_rays with grid=) evaluate, chunk
# by chunk, only the occupied samples of the live rays (nm_occ_compact_ray_chunk).  Off: the combination is refused (_occupancy_on), as it
# has been since grids exist.  Off by default: its frame time has not earned it a default (profiles/march_grid.md), and the rule of
# profiles/live_heads.md admits a route as a default only on a measured gain.  NEUMAN_MARCH_WITH_GRID=1 turns it on.
MARCH_WITH_GRID = os.environ.get("NEUMAN_MARCH_WITH_GRID", "0") == "1"
# The marched background passes as ONE C call each (march_pass_rays_fused: nm_march_pass -- uniform chunks of TERMINATION_CHUNK samples, the step
# between two chunks on the device over the live rays only, no host read per chunk).  Taken by bkg_place_z / bkg_shade for a net without a grid,
# outside the live-heads route; bit-identical to march_pass_rays(adaptive=False).  Off by default: the rule of profiles/live_heads.md admits a
# route as a default only on a measured gain (profiles/march_fused.md).  NEUMAN_MARCH_FUSED=1 turns it on.
MARCH_FUSED = os.environ.get("NEUMAN_MARCH_FUSED", "0") == "1"
FUSED_HYBRID_RAYS = int(os.environ.get("NEUMAN_FUSED_HYBRID_RAYS", 1 << 17))
# The multi-person renderer's batch body as ONE C call (render_multi_rays_fused: nm_render_rays_multi, any number of actors merged and composited
# by one kernel), in batches of FUSED_MULTI_RAYS rays.  Bit-identical to the step-by-step body and tested.  Off by default: measured on the 1080p
# frame (profiles/multi_fused.md) it is 2-4 % slower than today's route at 4-14 x less peak memory, and the rule of profiles/live_heads.md admits a
# route as a default only on a measured gain.  NEUMAN_MULTI_FUSED=1 turns it on.
MULTI_FUSED = os.environ.get("NEUMAN_MULTI_FUSED", "0") == "1"
FUSED_MULTI_RAYS = int(os.environ.get("NEUMAN_FUSED_MULTI_RAYS", 1 << 17))
MERGE_MAX_SAMPLES = (64 * 1024) // 12            # merged samples per ray nm_merge_composite_lists stages in LDS (csrc/ray_ops.hip) ...
WIDE_MERGE_MAX_SAMPLES = 8014                    # ... and nm_merge_composite_lists_wide (csrc/merge_wide.hip, kWideMaxSamples)
WIDE_MERGE_MAX_LISTS = 32
# The colour head on live samples only (vanilla.Joiner role='composite': nm_mlp_forward_*_live, nm_render_rays_*_live) in every composited pass
# of render_smpl_nerf, render_hybrid_nerf and render_hybrid_nerf_multi_persons, and in render_vanilla's gridded, marched and single-net passes.
# Off: those passes run the whole network on every sample they evaluate (frames are bit-identical either way).  render_vanilla's plain path takes
# the route whatever this says.
#
# The composite-only rule.  A pass may take the live route only when its `raw` reaches nothing but raw2outputs, merge_composite,
# merge_composite_lists, merge_sorted followed by raw2outputs, transmittance_of, or nm_transmittance_chunk*.  These read a colour only as
# weight x sigmoid(colour).  The weight is exactly 0 for any interval, merged ones included, when the stored density is <= 0.
#
# Off by default: the routes are bit-exact and tested, but their frame times on configs 3-5 have not been measured yet, and the rule of
# profiles/live_heads.md admits a route as a default only on a measured gain (profiles/live_heads_all_passes.md).  NEUMAN_LIVE_HEADS=1 turns them on.
LIVE_HEADS = os.environ.get("NEUMAN_LIVE_HEADS", "0") == "1"
_RAW_COMPOSITED_ONLY = False                     # set by the renderers around their bodies (raw_composited_only); read by human_pass_rays / human_march_rays


@contextlib.contextmanager
def raw_composited_only(n_max, device):
    """Inside the block the `raw` of human_pass_rays and human_march_rays is used under the composite-only rule above (a renderer's body), so
    they may take the live route; called directly they return whole-network records.  n_max: the samples of the largest composited pass of
    the block -- ONE live workspace serves them all (vanilla.live_workspace: allocated at the first live pass)."""
    global _RAW_COMPOSITED_ONLY
    prev = _RAW_COMPOSITED_ONLY
    _RAW_COMPOSITED_ONLY = True
    try:
        with vanilla.live_workspace(n_max, device):
            yield
    finally:
        _RAW_COMPOSITED_ONLY = prev


def _human_role():
    return 'composite' if LIVE_HEADS and _RAW_COMPOSITED_ONLY else 'shading'


# ------------------------------------------------------------------------------------------------
# a5 raw2outputs
# ------------------------------------------------------------------------------------------------
def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkg=True, want_weights=True):
    """reference render_utils.py:69-105 -> (rgb_map, disp_map, acc_map, weights, depth_map)."""
    _lib.require_gpu()
    R, S = z_vals.shape
    dev = raw.device
    noise = None
    if raw_noise_std > 0.:
        noise = (torch.randn((R, S), device=dev) * raw_noise_std).contiguous()          # render_utils.py:93
    if torch.is_grad_enabled() and raw.requires_grad:                                   # a training step: autograd through `raw`
        from . import train
        return train.composite_train(raw, z_vals, rays_d, white_bkg, noise)
    raw = raw.to(torch.float32).contiguous()
    z_vals = z_vals.to(torch.float32).contiguous()
    rays_d = rays_d.to(torch.float32).contiguous()
    rgb = torch.empty((R, 3), device=dev, dtype=torch.float32)
    disp = torch.empty(R, device=dev, dtype=torch.float32)
    acc = torch.empty(R, device=dev, dtype=torch.float32)
    depth = torch.empty(R, device=dev, dtype=torch.float32)
    weights = torch.empty((R, S), device=dev, dtype=torch.float32) if want_weights else None
    _lib.check(_lib.lib().nm_composite(_lib.dev_ptr(raw, name='raw'), _lib.dev_ptr(z_vals, name='z_vals'),
                                       _lib.dev_ptr(rays_d, name='rays_d'), R, S, int(bool(white_bkg)), _lib.dev_ptr(noise),
                                       _lib.dev_ptr(rgb), _lib.dev_ptr(disp), _lib.dev_ptr(acc), _lib.dev_ptr(weights),
                                       _lib.dev_ptr(depth), _lib.stream_ptr()), "nm_composite")
    return rgb, disp, acc, weights, depth


def merge_sorted(za, rawa, zb, rawb):
    """sort(cat([za, zb])) + gather of cat([rawa, rawb]) (render_utils.py:330-337); both lists sorted per ray."""
    _lib.require_gpu()
    R, Sa = za.shape
    Sb = zb.shape[1]
    z = torch.empty((R, Sa + Sb), device=za.device, dtype=torch.float32)
    raw = torch.empty((R, Sa + Sb, 4), device=za.device, dtype=torch.float32)
    _lib.check(_lib.lib().nm_merge_sorted(_lib.dev_ptr(za.contiguous()), _lib.dev_ptr(rawa.contiguous()), Sa,
                                          _lib.dev_ptr(zb.contiguous()), _lib.dev_ptr(rawb.contiguous()), Sb, R,
                                          _lib.dev_ptr(z), _lib.dev_ptr(raw), _lib.stream_ptr()), "nm_merge_sorted")
    return z, raw


# ------------------------------------------------------------------------------------------------
# device-level ray renderers
# ------------------------------------------------------------------------------------------------
def _chunks(n):
    for i in range(0, n, MAX_RAYS_PER_LAUNCH):
        yield i, min(i + MAX_RAYS_PER_LAUNCH, n)


def _note(trace, **kw):
    """`trace` (a dict, or None) collects a renderer's intermediates -- sample positions, hit lists, warped points -- so that
    tests can hand exactly those to the CPU oracle (conditional parity) while running the product code path itself."""
    if trace is not None:
        for k, v in kw.items():
            trace.setdefault(k, []).append(v)


def _transmittance_chunk(raw, z, dz, d, live, counts, R, s0, c, S, T):
    """T[live] *= prod over samples s0 .. s0+c-1 of raw2outputs' factors; intervals from z, or the given ones (merged lists)"""
    if dz is None:
        _lib.check(_lib.lib().nm_transmittance_chunk(_lib.dev_ptr(raw), _lib.dev_ptr(z), _lib.dev_ptr(d), _lib.dev_ptr(live, torch.int32),
                                                     _lib.dev_ptr(counts, torch.int32), R, s0, c, S, _lib.dev_ptr(T), _lib.stream_ptr()),
                   "nm_transmittance_chunk")
    else:
        _lib.check(_lib.lib().nm_transmittance_chunk_dz(_lib.dev_ptr(raw), _lib.dev_ptr(dz), _lib.dev_ptr(d), _lib.dev_ptr(live, torch.int32),
                                                        _lib.dev_ptr(counts, torch.int32), R, s0, c, S, _lib.dev_ptr(T), _lib.stream_ptr()),
                   "nm_transmittance_chunk_dz")


def merged_intervals(z_lists):
    """For every sample of every list ([R, S_k] each, sorted per ray; k <= 32, nm_merged_intervals' own limit -- the background list and up to
    31 actors): the distance to its successor in the MERGED order of all the
    lists (stable, earlier list first -- the order of the reference's sort(cat(...)), render_utils.py:330-337, 441-448); the last
    sample of the merged list gets raw2outputs' 1e10 (render_utils.py:86).  -> one [R, S_k] tensor per list.  These are the
    intervals the samples will be composited with once the lists are merged: what an early-termination cut has to be decided on.
    One kernel (nm_merged_intervals: a binary search per foreign list, nothing sorted)."""
    _lib.require_gpu()
    k, R = len(z_lists), z_lists[0].shape[0]
    zs = [z.to(torch.float32).contiguous() for z in z_lists]
    dz = [torch.empty_like(z) for z in zs]
    arr = ctypes.c_void_p * k
    _lib.check(_lib.lib().nm_merged_intervals(k, arr(*[z.data_ptr() for z in zs]), (ctypes.c_int * k)(*[int(z.shape[1]) for z in zs]), R,
                                              arr(*[x.data_ptr() for x in dz]), _lib.stream_ptr()), "nm_merged_intervals")
    return dz


def march_pass_rays(net, o, d, z, eps, chunk=None, precision=None, role='shading', stats=None, sigma_only=False, occluder=None,
                    adaptive=None, dz=None, grid=None):
    """A pass with early ray termination: the S sorted samples of every ray are evaluated front to back in chunks of `chunk`; after
    each chunk the rays whose transmittance (the running product of raw2outputs' factors, nm_transmittance_chunk) is below `eps`
    leave the list (ballot / prefix-sum compaction on the device, nm_compact_hits) and the next MLP launch covers the compacted live
    rays only (nm_mlp_forward_ray_chunk; `sigma_only`: nm_mlp_sigma_ray_chunk, a coarse pass).  Samples never evaluated keep
    sigma = 0, i.e. weight exactly 0 in raw2outputs; what they would have contributed is bounded by the transmittance at the cut:
    < eps per channel.

    occluder = (z_far [R], T_occ [R]): the ray's list will be merged with another whose samples all lie in front of z_far and whose
    total transmittance is T_occ (the hybrid renderers: the human samples).  Once the march is past z_far the transmittance of the
    MERGED list is T * T_occ, and that is what is compared with eps.  `dz` [R,S]: the samples' intervals in the merged list
    (merged_intervals) -- merging shortens the interval behind every sample that gets a foreign successor, so a transmittance
    taken over the list's OWN intervals is not an upper bound of the merged one; with `dz` (here and in T_occ) T * T_occ is the
    merged list's transmittance itself (before z_far: an upper bound of it, T_occ counted as 1).

    adaptive (default: eps > 0): ONE host read per chunk -- the live count.  No launch once nobody is live; the chunk is halved
    (not below TERMINATION_MIN_CHUNK) while more than 2 % of the live rays were cut by the last one -- rays are only ever cut at a chunk
    boundary, so near the cut a chunk is half its length of wasted evaluations per ray -- and doubled back otherwise.
    adaptive=False: fixed chunks, no host synchronisation between them (and with eps = 0, bit-identical to the unchunked launch).

    grid (an occupancy.OccupancyGrid; None: every sample of the live rays, also for a net that has a grid attached): each chunk lists the
    occupied samples of the live rays (OccupancyGrid.compact_ray_chunk: the cell test of the whole-pass list, on the device) and evaluates
    that list (occupancy.forward_listed_samples).  A skipped sample keeps raw = 0: the factor 1 - 0 + 1e-10 of the transmittance, what a
    sample with relu(sigma) = 0 gets -- cuts, chunk lengths and everything after the evaluation are those of the march whose skipped records
    were zeroed.  With eps = 0 the result is occupancy.forward_rays'.

    -> raw [R,S,4]; `stats` (a dict) receives the evaluation counts: 'evaluated' (samples the network ran on), 'total', 'launches' and -- with
    a grid -- 'grid_skipped' (candidates of live rays the grid dropped); accumulated on the device, read once at the end."""
    _lib.require_gpu()
    chunk = chunk or TERMINATION_CHUNK
    adaptive = (eps > 0) if adaptive is None else bool(adaptive)
    R, S = z.shape
    dev = z.device
    raw = torch.zeros((R, S, 4), device=dev, dtype=torch.float32)
    T = torch.ones(R, device=dev, dtype=torch.float32)
    thr = torch.full((R,), float(eps), device=dev, dtype=torch.float32)
    live = torch.arange(R, device=dev, dtype=torch.int32)
    counts = torch.tensor([R, 0], device=dev, dtype=torch.int32)
    ws = torch.empty(int(_lib.lib().nm_compact_workspace_ints(R)), device=dev, dtype=torch.int32)
    evaluated = torch.zeros(2, device=dev, dtype=torch.int64) if stats is not None else None     # (network evaluations, dropped by the grid)
    o, d, z = o.contiguous(), d.contiguous(), z.contiguous()
    if grid is not None:
        net._guard(o, d, z)
    s0, n_live, launches = 0, R, 0
    while s0 < S:
        c = min(chunk, S - s0)
        if grid is None:
            if evaluated is not None:
                evaluated[0] += counts[0].to(torch.int64) * c
            net.forward_ray_chunk(o, d, z, live, counts, s0, c, raw, precision=precision, role=role, sigma_only=sigma_only)
        else:
            # the live rays' occupied samples of the chunk only; like forward_ray_chunk, the launch is sized by the list's length R
            idx, kept = grid.compact_ray_chunk(o, d, z, live, counts, s0, c, n_rays=R)
            if evaluated is not None:
                evaluated += kept
            occupancy.forward_listed_samples(net, o, d, z, idx, kept, R * c, raw, precision=precision, role=role, sigma_only=sigma_only)
        launches += 1
        s0 += c
        if s0 >= S or eps <= 0:                                   # (eps = 0: nothing is ever dropped, not even rays whose T underflowed to 0)
            continue
        _transmittance_chunk(raw, z, dz, d, live, counts, R, s0 - c, c, S, T)
        T_eff = T if occluder is None else T * torch.where(z[:, s0] >= occluder[0], occluder[1], torch.ones_like(T))
        nxt = torch.empty(R, device=dev, dtype=torch.int32)
        counts = torch.zeros(2, device=dev, dtype=torch.int32)
        _lib.check(_lib.lib().nm_compact_hits(_lib.dev_ptr(thr), _lib.dev_ptr(T_eff.contiguous()), R, _lib.dev_ptr(nxt, torch.int32), None,
                                              _lib.dev_ptr(counts, torch.int32), _lib.dev_ptr(ws, torch.int32), _lib.stream_ptr()), "nm_compact_hits")
        live = nxt
        if adaptive:
            n_new = int(counts[0].item())
            if n_new == 0:
                break
            cut = 1.0 - n_new / max(1, n_live)
            chunk = max(TERMINATION_MIN_CHUNK, chunk // 2) if cut > 0.02 else min(max(chunk, TERMINATION_CHUNK), chunk * 2)
            n_live = n_new
    if stats is not None:
        n, skipped = evaluated.tolist()
        stats['evaluated'] = stats.get('evaluated', 0) + n
        if grid is not None:
            stats['grid_skipped'] = stats.get('grid_skipped', 0) + skipped
        stats['total'] = stats.get('total', 0) + R * S
        stats['launches'] = stats.get('launches', 0) + launches
    return raw


def march_pass_rays_fused(net, o, d, z, eps, chunk=None, precision=None, role='shading', stats=None, sigma_only=False, occluder=None, dz=None):
    """march_pass_rays(adaptive=False, grid=None) as ONE C call (nm_march_pass): the same chunk launches, and between two of them the
    transmittance, the occluder's factor, the cut and the compaction on the device over the live rays only (three launches, against a
    transmittance launch, a handful of ATen ops and a compaction over all R rays) -- the same records, the same counts, bit for bit.  The
    whole-network chunk launch only: role='composite' runs what 'shading' runs (the live-heads route stays with march_pass_rays).
    -> raw [R,S,4]; `stats` as march_pass_rays' ('evaluated', 'total', 'launches'), read once at the end."""
    _lib.require_gpu()
    chunk = int(chunk or TERMINATION_CHUNK)
    R, S = z.shape
    dev = z.device
    o, d, z = o.contiguous(), d.contiguous(), z.contiguous()
    net._guard(o, d, z)
    raw = torch.empty((R, S, 4), device=dev, dtype=torch.float32)
    n_ws = int(_lib.lib().nm_march_pass_workspace_floats(R))
    ws = _ws(n_ws, dev)
    evaluated = torch.empty(2, device=dev, dtype=torch.int64) if stats is not None else None
    occ_z, occ_T = (None, None) if occluder is None else (occluder[0].to(torch.float32).contiguous(), occluder[1].to(torch.float32).contiguous())
    _lib.check(_lib.lib().nm_march_pass(
        net.handle(), _lib.dev_ptr(o, name='origin'), _lib.dev_ptr(d, name='direction'), _lib.dev_ptr(z, name='z_vals'), R, S, chunk, float(eps),
        int(bool(sigma_only)), net._prec(precision, role), 1.0, _lib.dev_ptr(None if dz is None else dz.contiguous(), name='dz'),
        _lib.dev_ptr(occ_z, name='occluder z_far'), _lib.dev_ptr(occ_T, name='occluder T'), _lib.dev_ptr(ws), n_ws, _lib.dev_ptr(raw),
        _lib.dev_ptr(evaluated, torch.int64), _lib.stream_ptr()), "nm_march_pass")
    if stats is not None:
        stats['evaluated'] = stats.get('evaluated', 0) + (int(evaluated[0].item()) if R else 0)
        stats['total'] = stats.get('total', 0) + R * S
        stats['launches'] = stats.get('launches', 0) + -(-S // chunk)
    return raw


def _march_fused(net, role):
    """Does a marched background pass of `net` take the one-call route?  MARCH_FUSED, no grid on the net (nm_march_pass evaluates every sample of
    its live rays) and not the live-heads route (role 'composite' is only ever passed with LIVE_HEADS: nm_mlp_forward_ray_chunk_live)."""
    return MARCH_FUSED and occupancy.grid_of(net) is None and role != 'composite'


def transmittance_of(raw, z, d, dz=None):
    """prod_i (1 - alpha_i + 1e-10) over a whole list: raw2outputs' factors (render_utils.py:85-95) -> T [R].  With the list's own
    intervals (the last one 1e10), or -- `dz`, merged_intervals -- with the intervals it has once merged with other lists."""
    R, S = z.shape
    T = torch.ones(R, device=z.device, dtype=torch.float32)
    _transmittance_chunk(raw.contiguous(), z.contiguous(), None if dz is None else dz.contiguous(), d.contiguous(), None, None, R, 0, S, S, T)
    return T


def human_march_rays(human_net, o, d, near, far, samples_per_ray, mesh, eps, sigma_scale=1.0, precision=None, chunk=None, trace=None,
                     stats=None, dz=None):
    """human_pass_rays (posed) with early ray termination -> (raw [R,S,4], z [R,S]).  The warp is the expensive step here, and a ray that
    has entered an opaque body needs neither the closest-point queries nor the network behind the surface.  Front to back in chunks; the
    live rays' samples of a chunk are gathered, warped (one sample past the chunk: the canonical direction of a sample is the forward
    difference to the next warped point, ray_utils.py:62-64 -- the last sample of a ray repeats its predecessor's), evaluated and
    scattered back; rays whose transmittance over their own (human) samples is below eps are dropped (chunks of `chunk` samples, doubled
    after every chunk that cut fewer than 2 % of the live rays, halved otherwise).  `dz` [R,S] (the hybrid renderers): the samples'
    intervals in the list they will be MERGED into (merged_intervals) -- merging puts foreign samples inside the human intervals, which
    shortens them and RAISES the transmittance, so the cut is decided on the product of the human factors over the merged intervals:
    the merged list's transmittance can only be lower than that (the foreign samples' own factors are <= 1 + 1e-10), and what is skipped
    weighs < eps in the composite.  Without `dz` (render_smpl_nerf: the list is composited alone) the list's own intervals.  Every
    evaluated sample is bit-identical to human_pass_rays' (per-sample arithmetic; tests/test_hip_march.py).  With an occupancy grid on the
    net (occupancy.attach, K11b) a chunk evaluates only its occupied canonical points; the others keep raw = 0.  Inside a renderer's body
    (raw_composited_only) with LIVE_HEADS the colour of an evaluated sample whose density is <= 0 is 0 (role='composite')."""
    _lib.require_gpu()
    R, S = o.shape[0], int(samples_per_ray)
    dev = o.device
    chunk = chunk or TERMINATION_MIN_CHUNK
    pts, _, z = ray_utils.sample_z(o.contiguous(), d.contiguous(), near.reshape(-1).contiguous(), far.reshape(-1).contiguous(), S, want_points=True)
    raw = torch.zeros((R, S, 4), device=dev, dtype=torch.float32)
    T = torch.ones(R, device=dev, dtype=torch.float32)
    d = d.contiguous()
    live = torch.arange(R, device=dev)
    s0, evaluated, launches = 0, 0, 0
    grid = occupancy.grid_of(human_net)
    occ_stats = {} if grid is not None else None
    while s0 < S and live.numel() > 0:
        c = min(chunk, S - s0)
        a = s0 - 1 if (s0 + c == S and c == 1) else s0                               # a lone last sample takes its predecessor along
        b = min(S, s0 + c + 1)
        can_pts, can_dirs, _ = ray_utils.warp_to_canonical_dev(pts[live, a:b].contiguous(), mesh)
        k = s0 - a
        if grid is None:
            out = human_net(can_pts[:, k:k + c].contiguous(), can_dirs[:, k:k + c].contiguous(), precision=precision, sigma_scale=sigma_scale,
                            role=_human_role())
            evaluated += live.numel() * c
        else:                                                                       # the chunk's occupied canonical points only (K11b)
            out = occupancy.forward_points(human_net, can_pts[:, k:k + c].contiguous(), can_dirs[:, k:k + c].contiguous(), precision=precision,
                                           sigma_scale=sigma_scale, role=_human_role(), stats=occ_stats)
        raw[live, s0:s0 + c] = out
        launches += 1
        s0 += c
        if s0 >= S or eps <= 0:
            continue
        idx = live.to(torch.int32)
        cnt = torch.tensor([idx.numel(), 0], device=dev, dtype=torch.int32)
        _transmittance_chunk(raw, z, dz, d, idx, cnt, R, s0 - c, c, S, T)
        n_live = live.numel()
        live = live[T[live] >= eps]
        # (march_pass_rays' rule: short chunks while rays are being cut, doubling when nothing happens)
        chunk = max(TERMINATION_MIN_CHUNK, chunk // 2) if live.numel() < 0.98 * n_live else chunk * 2
    if occ_stats is not None:
        evaluated = occ_stats.get('evaluated', 0)
        _note(trace, occupancy_human={'evaluated': evaluated, 'total': R * S})
    if stats is not None:
        stats['human_evaluated'] = stats.get('human_evaluated', 0) + evaluated
        stats['human_total'] = stats.get('human_total', 0) + R * S
        stats['human_launches'] = stats.get('human_launches', 0) + launches
    _note(trace, human_z=z)
    return raw, z


def _given_near_far(given, actor, i, j, o, d, verts, geo_threshold):
    """near / far of one actor for rays [i, j) of the call: computed (nm_near_far), or replayed from `given` (see bkg_pass_rays)"""
    if given is not None and 'near_far' in given:
        n, f = given['near_far'][actor]
        return n[i:j].to(torch.float32).contiguous(), f[i:j].to(torch.float32).contiguous()
    return ray_utils.geometry_guided_near_far(o, d, verts, geo_threshold)


def _ws(n_floats, device):
    return torch.empty(max(int(n_floats), 4), device=device, dtype=torch.float32)


def bkg_pass_rays_fused(coarse_net, fine_net, o, d, near, far, samples_per_ray, importance_samples_per_ray, white_bkg, precision=None):
    """bkg_pass_rays as ONE C call (nm_render_rays_bkg: sample -> coarse density pass -> compositing weights -> importance samples ->
    fine pass, enqueued back to back; same kernels, same bits).  What the trainers' frozen background evaluation uses: at 2048 rays
    the five launches are shorter than the Python between them."""
    _lib.require_gpu()
    if _occupancy_on(coarse_net, fine_net):                # the fused call evaluates every sample: a grid takes the unfused passes
        raw, z = bkg_pass_rays(coarse_net, fine_net, o.contiguous(), d.contiguous(), near.reshape(-1).contiguous(), far.reshape(-1).contiguous(),
                               samples_per_ray, importance_samples_per_ray, white_bkg, precision)
        return raw, z
    R, S = o.shape[0], int(samples_per_ray)
    N = int(importance_samples_per_ray) if fine_net is not None else 0
    dev = o.device
    for n_ in (coarse_net, fine_net):
        if n_ is not None:
            n_._guard(o, d, near)
    raw = torch.empty((R, S + N, 4), device=dev, dtype=torch.float32)
    z = torch.empty((R, S + N), device=dev, dtype=torch.float32)
    ws = _ws(_lib.lib().nm_render_rays_bkg_workspace_floats(R, S, N), dev)
    t_vals = torch.linspace(0., 1., steps=S, device=dev)
    u = torch.linspace(0., 1., steps=N, device=dev) if N else None
    _lib.check(_lib.lib().nm_render_rays_bkg(
        coarse_net.handle(), fine_net.handle() if fine_net is not None else None, _lib.dev_ptr(o.contiguous()), _lib.dev_ptr(d.contiguous()),
        _lib.dev_ptr(near.reshape(-1).contiguous()), _lib.dev_ptr(far.reshape(-1).contiguous()), R, S, N, _lib.dev_ptr(t_vals), _lib.dev_ptr(u),
        int(bool(white_bkg)), coarse_net._prec(precision, None if fine_net is not None else 'shading'),
        fine_net._prec(precision, 'shading') if fine_net is not None else 0, _lib.dev_ptr(ws), _lib.dev_ptr(raw), _lib.dev_ptr(z), None, None, None,
        _lib.stream_ptr()), "nm_render_rays_bkg")
    return raw, z


def _occupancy_on(*nets):
    """Does a background pass of these nets skip empty space (occupancy.attach)?  Refuses the combination with early termination unless
    MARCH_WITH_GRID (the marched passes then take the grid: bkg_place_z, bkg_shade)."""
    on = any(occupancy.grid_of(n_) is not None for n_ in nets)
    if on and TERMINATION_EPS > 0 and not MARCH_WITH_GRID:
        raise NotImplementedError("an occupancy grid together with early ray termination (TERMINATION_EPS > 0) is not served: "
                                  "detach the grid or set TERMINATION_EPS = 0 (or take the switched route: NEUMAN_MARCH_WITH_GRID=1, "
                                  "render_utils.MARCH_WITH_GRID)")
    return on


def _occupancy_pass(net, o, d, z, precision, role, sigma_only, trace, key):
    """net.forward_rays on the samples its grid keeps (occupancy.forward_rays); `trace` receives {key: {'evaluated', 'total'}}."""
    stats = {} if trace is not None else None
    raw = occupancy.forward_rays(net, o, d, z, precision=precision, role=role, sigma_only=sigma_only, stats=stats)
    _note(trace, **{key: stats})
    return raw


def bkg_place_z(coarse_net, fine_net, o, d, near, far, samples_per_ray, importance_samples_per_ray, white_bkg, precision=None, trace=None,
                composite_only=False):
    """Where the background list's FINAL samples are (render_utils.py:131-147, 287-293): the stratified samples, or -- with a fine net --
    the coarse density pass, its compositing weights and the importance samples merged in.  -> (z [R,S'], raw of the coarse pass when it
    is the pass that is composited [no fine net; evaluated here unless termination is on], else None).  composite_only: as bkg_shade, for that
    raw (the single-net pass, gridded or whole).  A grid on the coarse net together with TERMINATION_EPS > 0 (MARCH_WITH_GRID, else
    refused): the coarse pass of a two-net render is marched at TERMINATION_COARSE on its occupied samples (trace key march_coarse); the
    single-net pass is left to bkg_shade, as without a grid.  MARCH_FUSED: the marched coarse pass of a net without a grid is one C call
    (march_pass_rays_fused)"""
    role = 'composite' if composite_only and LIVE_HEADS else 'shading'
    occ = _occupancy_on(coarse_net)
    _, _, z = ray_utils.sample_z(o, d, near, far, samples_per_ray)
    if occ and TERMINATION_EPS <= 0:
        # empty-space skipping (occupancy.py): skipped samples keep raw = 0 -- weight 0, as relu(sigma) = 0 gives
        if fine_net is None:
            return z, _occupancy_pass(coarse_net, o, d, z, precision, role, False, trace, 'occupancy_coarse')
        raw = _occupancy_pass(coarse_net, o, d, z, precision, None, True, trace, 'occupancy_coarse')
        z_fine, w = ray_utils.importance_z_from_raw(raw, z, d, importance_samples_per_ray, want_weights=trace is not None)
        _note(trace, coarse_z=z, coarse_w=w)
        return z_fine, None
    if fine_net is None:
        return z, (None if TERMINATION_EPS > 0 else coarse_net.forward_rays(o, d, z, precision=precision, role=role))
    # with a fine net the coarse pass only places the importance samples (only its density is used, render_utils.py:139-141: the
    # colour head is skipped) and is not the pass the mixed precision policy tags 'shading' (vanilla.Joiner._prec)
    if TERMINATION_EPS > 0:
        # marched at TERMINATION_COARSE on its own transmittance only (where the importance samples go must not depend on what the
        # list is merged with later)
        stats = {} if trace is not None else None
        if _march_fused(coarse_net, None):
            raw = march_pass_rays_fused(coarse_net, o, d, z, TERMINATION_COARSE, precision=precision, role=None, stats=stats, sigma_only=True)
        else:
            raw = march_pass_rays(coarse_net, o, d, z, TERMINATION_COARSE, precision=precision, role=None, stats=stats, sigma_only=True,
                                  grid=occupancy.grid_of(coarse_net) if occ else None)
        _note(trace, march_coarse=stats)
    else:
        raw = coarse_net.forward_rays(o, d, z, precision=precision, role=None, sigma_only=True)
    # raw2outputs' weights -> sample_pdf -> sorted merge: one kernel (the weights reach HBM only for a trace)
    z_fine, w = ray_utils.importance_z_from_raw(raw, z, d, importance_samples_per_ray, want_weights=trace is not None)
    _note(trace, coarse_z=z, coarse_w=w)
    return z_fine, None


def bkg_shade(net, o, d, z, precision=None, trace=None, occluder=None, dz=None, composite_only=False):
    """The background pass that is composited, on its final samples (render_utils.py:148-151, 294-297): whole, or -- TERMINATION_EPS > 0 --
    marched front to back at eps (`occluder`, `dz`: march_pass_rays), or -- a grid attached (occupancy.attach) -- on its occupied samples.
    composite_only: the caller feeds the raw to raw2outputs and to nothing else, so the whole pass may leave the colour of a sample without
    density at 0 (Joiner.forward_rays role='composite': its weight is exactly 0); with LIVE_HEADS so may the marched and the gridded pass.
    A grid together with TERMINATION_EPS > 0 (MARCH_WITH_GRID, else refused): the marched pass on the occupied samples of its live rays
    (march_pass_rays grid=; trace key march, with 'grid_skipped').  MARCH_FUSED: the marched pass of a net without a grid, outside the
    live-heads route, is one C call (march_pass_rays_fused: fixed chunks, no host read between them; same trace keys)"""
    role = 'composite' if composite_only and LIVE_HEADS else 'shading'
    occ = _occupancy_on(net)
    if occ and TERMINATION_EPS <= 0:
        return _occupancy_pass(net, o, d, z, precision, role, False, trace, 'occupancy')
    if TERMINATION_EPS > 0:
        stats = {} if trace is not None else None
        if _march_fused(net, role):
            raw = march_pass_rays_fused(net, o, d, z, TERMINATION_EPS, precision=precision, role=role, stats=stats, occluder=occluder, dz=dz)
        else:
            raw = march_pass_rays(net, o, d, z, TERMINATION_EPS, precision=precision, role=role, stats=stats, occluder=occluder, dz=dz,
                                  grid=occupancy.grid_of(net) if occ else None)
        _note(trace, march=stats)
        return raw
    return net.forward_rays(o, d, z, precision=precision, role='composite' if composite_only else 'shading')


def bkg_pass_rays(coarse_net, fine_net, o, d, near, far, samples_per_ray, importance_samples_per_ray, white_bkg,
                  precision=None, trace=None, given_z=None, occluder=None, dz=None, composite_only=False):
    """Coarse (+ fine) background evaluation of R rays -> (raw [R,S',4], z [R,S'])  (render_utils.py:131-151, 287-297):
    bkg_place_z + bkg_shade (`composite_only`: see there).

    `given_z` [R, S'] (tests only, like `trace`): replay recorded final sample positions instead of deriving them -- the shading
    network is evaluated on exactly those.  The renderers pass it from their `given` dict ({'bkg_z': [R,S'], 'near_far':
    [(near [R], far [R]) per actor]}, device tensors indexed like the call's rays): the two steps that are ill conditioned in
    float32 -- the inverse CDF behind the importance samples and the cancellation under geometry_guided_near_far's square root
     -- are taken from a recording of the reference's own run, so that everything else can be held to 1e-4
    on every pixel against the reference's frames (tests/test_hip_posed_golden.py)."""
    net = fine_net if fine_net is not None else coarse_net
    if given_z is not None:
        z = given_z.to(torch.float32).contiguous()
        _note(trace, bkg_z=z)
        return net.forward_rays(o, d, z, precision=precision, role='shading'), z
    z, raw = bkg_place_z(coarse_net, fine_net, o, d, near, far, samples_per_ray, importance_samples_per_ray, white_bkg, precision, trace,
                         composite_only)
    if raw is None:
        raw = bkg_shade(net, o, d, z, precision, trace, occluder, dz, composite_only)
    _note(trace, bkg_z=z)
    return raw, z


def render_vanilla_rays(coarse_net, fine_net, o, d, near, far, samples_per_ray, importance_samples_per_ray, white_bkg=True,
                        precision=None, trace=None, given=None):
    """Device core of render_vanilla: o, d [R,3] CUDA f32, scalar near/far -> (rgb [R,3], depth [R]) CUDA."""
    R = o.shape[0]
    rgb = torch.empty((R, 3), device=o.device, dtype=torch.float32)
    depth = torch.empty(R, device=o.device, dtype=torch.float32)
    S_max = int(samples_per_ray) + (int(importance_samples_per_ray) if fine_net is not None else 0)
    with vanilla.live_workspace(min(R, MAX_RAYS_PER_LAUNCH) * S_max, o.device):                 # one live workspace for every pass and chunk of the call
        for i, j in _chunks(R):
            oc, dc = o[i:j], d[i:j]
            n = torch.full((j - i,), float(near), device=o.device, dtype=torch.float32)
            f = torch.full((j - i,), float(far), device=o.device, dtype=torch.float32)
            raw, z = bkg_pass_rays(coarse_net, fine_net, oc, dc, n, f, samples_per_ray, importance_samples_per_ray, white_bkg,
                                   precision, trace, given['bkg_z'][i:j] if given is not None and 'bkg_z' in given else None, composite_only=True)
            rgb[i:j], _, _, _, depth[i:j] = raw2outputs(raw, z, dc, white_bkg=white_bkg, want_weights=False)
    return rgb, depth


def human_pass_rays(human_net, o, d, near, far, samples_per_ray, mesh=None, render_can=False, sigma_scale=1.0, precision=None,
                    trace=None):
    """Human-net evaluation of (already compacted) hit rays -> (raw [R,S,4], z [R,S])  (render_utils.py:213-229, 320-329): ONE C call
    per actor pass (nm_render_rays_human: sample -> warp -> network, enqueued back to back)."""
    _lib.require_gpu()
    R, S = o.shape[0], int(samples_per_ray)
    dev = o.device
    human_net._guard(o, d, near)
    posed = not render_can
    grid = occupancy.grid_of(human_net)
    raw = torch.empty((R, S, 4), device=dev, dtype=torch.float32)
    z = torch.empty((R, S), device=dev, dtype=torch.float32)
    t_vals = torch.linspace(0., 1., steps=S, device=dev)
    # inside a renderer's body (raw_composited_only) the colour head runs on the samples with density only: the *_live sibling of either call
    live = _human_role() == 'composite' and human_net.live_route(precision, 'composite', R * S)
    lws, lbytes = vanilla.live_workspace_for(R * S, 0, dev) if live else (None, 0)
    tail = (_lib.dev_ptr(lws, torch.uint8), lbytes, 0, _lib.stream_ptr()) if live else (_lib.stream_ptr(),)
    if grid is None:
        ws = _ws(_lib.lib().nm_render_rays_human_workspace_floats(R, S, int(posed)), dev)
        entry = _lib.lib().nm_render_rays_human_live if live else _lib.lib().nm_render_rays_human
        _lib.check(entry(
            human_net.handle(), mesh.handle if posed else None, _lib.dev_ptr(mesh.T, torch.float64, 'T') if posed else None, _lib.dev_ptr(o.contiguous()),
            _lib.dev_ptr(d.contiguous()), _lib.dev_ptr(near.reshape(-1).contiguous()), _lib.dev_ptr(far.reshape(-1).contiguous()), R, S, _lib.dev_ptr(t_vals), 1,
            float(sigma_scale), human_net._prec(precision, 'shading'), _lib.dev_ptr(ws), _lib.dev_ptr(raw), _lib.dev_ptr(z), None, None, None, *tail),
            "nm_render_rays_human_live" if live else "nm_render_rays_human")
    else:
        # empty-space skipping (occupancy.py, K11b): the grid is tested on the canonical points -- o + d z (canonical render) or the warped
        # points (posed); skipped samples keep raw = 0.  Same workspace prefix as nm_render_rays_human (the trace below reads it).
        grid.check_device(dev)
        counts = torch.zeros(2, device=dev, dtype=torch.int32)
        ws = _ws(_lib.lib().nm_render_rays_human_occ_workspace_floats(R, S, int(posed)), dev)
        entry = _lib.lib().nm_render_rays_human_occ_live if live else _lib.lib().nm_render_rays_human_occ
        _lib.check(entry(
            human_net.handle(), mesh.handle if posed else None, _lib.dev_ptr(mesh.T, torch.float64, 'T') if posed else None,
            _lib.dev_ptr(grid.bits, torch.int32), grid.res, grid.box_c(), _lib.dev_ptr(o.contiguous()), _lib.dev_ptr(d.contiguous()),
            _lib.dev_ptr(near.reshape(-1).contiguous()), _lib.dev_ptr(far.reshape(-1).contiguous()), R, S, _lib.dev_ptr(t_vals), 1, float(sigma_scale),
            human_net._prec(precision, 'shading'), _lib.dev_ptr(ws), _lib.dev_ptr(raw), _lib.dev_ptr(z), _lib.dev_ptr(counts, torch.int32), None, None, None,
            *tail), "nm_render_rays_human_occ_live" if live else "nm_render_rays_human_occ")
        if trace is not None:
            _note(trace, occupancy_human={'evaluated': int(counts[0].item()), 'total': R * S})
    if trace is not None:
        if posed:
            n3 = (R * S * 3 + 3) & ~3
            _note(trace, human_z=z, can_pts=ws[n3:n3 + R * S * 3].reshape(R, S, 3).clone(), can_dirs=ws[2 * n3:2 * n3 + R * S * 3].reshape(R, S, 3).clone())
        else:
            _note(trace, human_z=z)
    return raw, z


def merge_composite(za, rawa, zb, rawb, rays_d, white_bkg=True):
    """merge_sorted + raw2outputs of the merged list as ONE C call (render_utils.py:330-345) -> (rgb [R,3], depth [R], acc [R])"""
    _lib.require_gpu()
    R, Sa = za.shape
    Sb = zb.shape[1]
    dev = za.device
    rgb = torch.empty((R, 3), device=dev, dtype=torch.float32)
    depth = torch.empty(R, device=dev, dtype=torch.float32)
    acc = torch.empty(R, device=dev, dtype=torch.float32)
    ws = _ws(_lib.lib().nm_merge_composite_workspace_floats(R, Sa, Sb), dev)
    _lib.check(_lib.lib().nm_merge_composite(_lib.dev_ptr(za.contiguous()), _lib.dev_ptr(rawa.contiguous()), Sa, _lib.dev_ptr(zb.contiguous()),
                                             _lib.dev_ptr(rawb.contiguous()), Sb, R, _lib.dev_ptr(rays_d.contiguous()), int(bool(white_bkg)), _lib.dev_ptr(ws),
                                             _lib.dev_ptr(rgb), _lib.dev_ptr(depth), _lib.dev_ptr(acc), _lib.stream_ptr()), "nm_merge_composite")
    return rgb, depth, acc


def merge_composite_lists(z_lists, raw_lists, rays_d, white_bkg=True, rows=None):
    """k <= 4 sorted lists per ray -> merged order -> raw2outputs' sums, ONE kernel, the merged list never in HBM
    (render_utils.py:330-345, 441-456).  rows[l] (int32 [R] or None): list l's tensors are indexed by rows[l][ray] -- a list that
    exists for ALL rays of a batch read in place for the compacted hit rays.  -> (rgb [R,3], depth [R], acc [R]); bit-identical to
    merge_sorted list by list + raw2outputs."""
    _lib.require_gpu()
    k = len(z_lists)
    R = rays_d.shape[0]
    dev = rays_d.device
    zs = [z.to(torch.float32).contiguous() for z in z_lists]
    raws = [r_.to(torch.float32).contiguous() for r_ in raw_lists]
    rows = [None] * k if rows is None else [None if x is None else x.to(torch.int32).contiguous() for x in rows]
    for l_ in range(k):
        if rows[l_] is None and zs[l_].shape[0] != R:
            raise _lib.NeumanHipError(f"merge_composite_lists: list {l_} has {zs[l_].shape[0]} rows for {R} rays")
    arr = ctypes.c_void_p * k
    rgb = torch.empty((R, 3), device=dev, dtype=torch.float32)
    depth = torch.empty(R, device=dev, dtype=torch.float32)
    acc = torch.empty(R, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().nm_merge_composite_lists(
        k, arr(*[z.data_ptr() for z in zs]), arr(*[r_.data_ptr() for r_ in raws]), arr(*[None if x is None else x.data_ptr() for x in rows]),
        (ctypes.c_int * k)(*[int(z.shape[1]) for z in zs]), R, _lib.dev_ptr(rays_d.contiguous()), int(bool(white_bkg)), _lib.dev_ptr(rgb), _lib.dev_ptr(depth),
        _lib.dev_ptr(acc), _lib.stream_ptr()), "nm_merge_composite_lists")
    return rgb, depth, acc


def merge_composite_lists_wide(z_lists, raw_lists, rays_d, white_bkg=True, rows=None):
    """merge_composite_lists for 1 .. 32 lists (nm_merge_composite_lists_wide, K7c: the background and any number of actors in ONE kernel, the
    merged list never in HBM; at most WIDE_MERGE_MAX_SAMPLES merged samples per ray).  Same arguments, same result: bit-identical to
    merge_sorted list by list + raw2outputs, and up to four lists to merge_composite_lists."""
    _lib.require_gpu()
    k = len(z_lists)
    R = rays_d.shape[0]
    dev = rays_d.device
    if not 1 <= k <= WIDE_MERGE_MAX_LISTS or len(raw_lists) != k:
        raise _lib.NeumanHipError(f"merge_composite_lists_wide: 1 <= k <= {WIDE_MERGE_MAX_LISTS} lists with their records (k={k})")
    zs = [z.to(torch.float32).contiguous() for z in z_lists]
    raws = [r_.to(torch.float32).contiguous() for r_ in raw_lists]
    rows = [None] * k if rows is None else [None if x is None else x.to(torch.int32).contiguous() for x in rows]
    for l_ in range(k):
        if rows[l_] is None and zs[l_].shape[0] != R:
            raise _lib.NeumanHipError(f"merge_composite_lists_wide: list {l_} has {zs[l_].shape[0]} rows for {R} rays")
    arr = ctypes.c_void_p * k
    rgb = torch.empty((R, 3), device=dev, dtype=torch.float32)
    depth = torch.empty(R, device=dev, dtype=torch.float32)
    acc = torch.empty(R, device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().nm_merge_composite_lists_wide(
        k, arr(*[z.data_ptr() for z in zs]), arr(*[r_.data_ptr() for r_ in raws]), arr(*[None if x is None else x.data_ptr() for x in rows]),
        (ctypes.c_int * k)(*[int(z.shape[1]) for z in zs]), R, _lib.dev_ptr(rays_d.contiguous()), int(bool(white_bkg)), _lib.dev_ptr(rgb), _lib.dev_ptr(depth),
        _lib.dev_ptr(acc), _lib.stream_ptr()), "nm_merge_composite_lists_wide")
    return rgb, depth, acc


def merge_composite_layers(z_lists, raw_lists, rays_d, white_bkg=True, rows=None):
    """merge_composite_lists_wide with per-list layers (nm_merge_composite_layers, K7d): same arguments, the same rgb / depth / acc bit for bit, and
    for every list l the sums over its own samples with the weights they have in the MERGED list: layer_rgb [R,k,3] (premultiplied, no background
    added), layer_depth [R,k], layer_acc [R,k].  -> (rgb, depth, acc, layer_rgb, layer_depth, layer_acc)"""
    _lib.require_gpu()
    k = len(z_lists)
    R = rays_d.shape[0]
    dev = rays_d.device
    if not 1 <= k <= WIDE_MERGE_MAX_LISTS or len(raw_lists) != k:
        raise _lib.NeumanHipError(f"merge_composite_layers: 1 <= k <= {WIDE_MERGE_MAX_LISTS} lists with their records (k={k})")
    zs = [z.to(torch.float32).contiguous() for z in z_lists]
    raws = [r_.to(torch.float32).contiguous() for r_ in raw_lists]
    rows = [None] * k if rows is None else [None if x is None else x.to(torch.int32).contiguous() for x in rows]
    for l_ in range(k):
        if rows[l_] is None and zs[l_].shape[0] != R:
            raise _lib.NeumanHipError(f"merge_composite_layers: list {l_} has {zs[l_].shape[0]} rows for {R} rays")
    arr = ctypes.c_void_p * k
    rgb = torch.empty((R, 3), device=dev, dtype=torch.float32)
    depth = torch.empty(R, device=dev, dtype=torch.float32)
    acc = torch.empty(R, device=dev, dtype=torch.float32)
    layer_rgb = torch.empty((R, k, 3), device=dev, dtype=torch.float32)
    layer_depth = torch.empty((R, k), device=dev, dtype=torch.float32)
    layer_acc = torch.empty((R, k), device=dev, dtype=torch.float32)
    _lib.check(_lib.lib().nm_merge_composite_layers(
        k, arr(*[z.data_ptr() for z in zs]), arr(*[r_.data_ptr() for r_ in raws]), arr(*[None if x is None else x.data_ptr() for x in rows]),
        (ctypes.c_int * k)(*[int(z.shape[1]) for z in zs]), R, _lib.dev_ptr(rays_d.contiguous()), int(bool(white_bkg)), _lib.dev_ptr(rgb), _lib.dev_ptr(depth),
        _lib.dev_ptr(acc), _lib.dev_ptr(layer_rgb), _lib.dev_ptr(layer_depth), _lib.dev_ptr(layer_acc), _lib.stream_ptr()), "nm_merge_composite_layers")
    return rgb, depth, acc, layer_rgb, layer_depth, layer_acc


def render_smpl_nerf_rays(human_net, o, d, posed_verts, mesh, samples_per_ray, white_bkg=True, render_can=False,
                          geo_threshold=DEFAULT_GEO_THRESH, interval_comp=1.0, precision=None, trace=None, given=None):
    """Device core of render_smpl_nerf -> (rgb [R,3], depth [R], acc [R]) CUDA.  `given`: see bkg_pass_rays."""
    R = o.shape[0]
    rgb = torch.full((R, 3), 1.0 if white_bkg else 0.0, device=o.device, dtype=torch.float32)    # misses, :199-205
    depth = torch.zeros(R, device=o.device, dtype=torch.float32)
    acc = torch.zeros(R, device=o.device, dtype=torch.float32)
    with raw_composited_only(min(R, MAX_RAYS_PER_LAUNCH) * int(samples_per_ray), o.device):      # (raw -> raw2outputs, nothing else)
        _render_smpl_nerf_batches(human_net, o, d, posed_verts, mesh, samples_per_ray, white_bkg, render_can, geo_threshold, interval_comp, precision, trace, given,
                                  rgb, depth, acc)
    return rgb, depth, acc


def _render_smpl_nerf_batches(human_net, o, d, posed_verts, mesh, samples_per_ray, white_bkg, render_can, geo_threshold, interval_comp, precision, trace, given,
                              rgb, depth, acc):
    R = o.shape[0]
    for i, j in _chunks(R):
        oc, dc = o[i:j].contiguous(), d[i:j].contiguous()
        near, far = _given_near_far(given, 0, i, j, oc, dc, posed_verts, geo_threshold)
        _note(trace, near=near, far=far)
        hit, _ = ray_utils.compact_hits(near, far)
        if hit.numel() == 0:
            continue
        ho, hd = ray_utils.gather_rows(oc, hit), ray_utils.gather_rows(dc, hit)
        hn, hf = ray_utils.gather_rows(near, hit), ray_utils.gather_rows(far, hit)
        _note(trace, hit=hit + i)
        if TERMINATION_EPS > 0 and not render_can:
            mstats = {} if trace is not None else None
            raw, z = human_march_rays(human_net, ho, hd, hn, hf, samples_per_ray, mesh, TERMINATION_EPS, interval_comp, precision, None, trace, mstats)
            _note(trace, march_human=mstats)
        else:
            raw, z = human_pass_rays(human_net, ho, hd, hn, hf, samples_per_ray, mesh, render_can, interval_comp, precision, trace)
        _rgb, _, _acc, _, _depth = raw2outputs(raw, z, hd, white_bkg=white_bkg, want_weights=False)
        ray_utils.scatter_rows(rgb[i:j], hit, _rgb)
        ray_utils.scatter_rows(depth[i:j], hit, _depth)
        ray_utils.scatter_rows(acc[i:j], hit, _acc)


def render_hybrid_rays(coarse_bkg, fine_bkg, human_net, o, d, bkg_near, bkg_far, posed_verts, mesh, samples_per_ray,
                       importance_samples_per_ray, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH, precision=None, trace=None,
                       given=None):
    """Device core of render_hybrid_nerf -> (rgb [R,3], depth [R], acc [R]) CUDA  (render_utils.py:276-356).  `given`: see bkg_pass_rays.
    With TERMINATION_EPS > 0 the background's sample positions are settled first, then the human pass and the background shading pass
    are marched, each on the transmittance its samples have in the MERGED list (merged_intervals: the body's factors over the merged
    intervals bound the merged transmittance from above; behind the body the background sees its own x the body's): a pixel moves
    by < 2 eps, for bodies of any opacity (tests/test_hip_march.py: opaque and semi-transparent).
    The plain case (no trace, no replay, no termination, no occupancy grid on any of the nets) is ONE C call per batch: render_hybrid_rays_fused,
    bit-identical.  Every raw of the body falls under the composite-only rule (LIVE_HEADS above): raw2outputs, merge_composite_lists,
    transmittance_of and the marches' nm_transmittance_chunk* are all that read it."""
    S_max = int(samples_per_ray) + (int(importance_samples_per_ray) if fine_bkg is not None else 0)
    with raw_composited_only(min(o.shape[0], MAX_RAYS_PER_LAUNCH) * S_max, o.device):
        return _render_hybrid_rays(coarse_bkg, fine_bkg, human_net, o, d, bkg_near, bkg_far, posed_verts, mesh, samples_per_ray, importance_samples_per_ray,
                                   white_bkg, geo_threshold, precision, trace, given)


def _new_layers(layers, R, L, device):
    """the per-ray layer arrays of a layered render, zero (an actor a ray misses contributes nothing), into the caller's dict"""
    layers.update(layer_rgb=torch.zeros((R, L, 3), device=device, dtype=torch.float32), layer_depth=torch.zeros((R, L), device=device, dtype=torch.float32),
                  layer_acc=torch.zeros((R, L), device=device, dtype=torch.float32))
    return layers['layer_rgb'], layers['layer_depth'], layers['layer_acc']


def render_hybrid_layers_rays(coarse_bkg, fine_bkg, human_net, o, d, bkg_near, bkg_far, posed_verts, mesh, samples_per_ray,
                              importance_samples_per_ray, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH, precision=None, trace=None,
                              given=None):
    """render_hybrid_rays with the picture kept in layers: same arguments -> dict of rgb [R,3] and depth [R] (bit-identical to render_hybrid_rays)
    and layer_rgb [R,2,3], layer_depth [R,2], layer_acc [R,2]: layer 0 the background, layer 1 the actor, each the premultiplied sums of its own
    samples with the weights they have in the merged list (merge_composite_layers).  A ray that misses the body has the background-only
    composite in layer 0 and an empty actor layer.  The step-by-step body with its last merge exchanged; never the one-call route."""
    S_max = int(samples_per_ray) + (int(importance_samples_per_ray) if fine_bkg is not None else 0)
    layers = {}
    with raw_composited_only(min(o.shape[0], MAX_RAYS_PER_LAUNCH) * S_max, o.device):
        rgb, depth, _ = _render_hybrid_rays(coarse_bkg, fine_bkg, human_net, o, d, bkg_near, bkg_far, posed_verts, mesh, samples_per_ray,
                                            importance_samples_per_ray, white_bkg, geo_threshold, precision, trace, given, layers=layers)
    return dict(rgb=rgb, depth=depth, **layers)


def _render_hybrid_rays(coarse_bkg, fine_bkg, human_net, o, d, bkg_near, bkg_far, posed_verts, mesh, samples_per_ray, importance_samples_per_ray, white_bkg,
                        geo_threshold, precision, trace, given, layers=None):
    if layers is None and TERMINATION_EPS <= 0 and trace is None and given is None and not _occupancy_on(coarse_bkg, fine_bkg) and occupancy.grid_of(human_net) is None:
        return render_hybrid_rays_fused(coarse_bkg, fine_bkg, human_net, o, d, bkg_near, bkg_far, posed_verts, mesh, samples_per_ray,
                                        importance_samples_per_ray, white_bkg, geo_threshold, precision)
    R = o.shape[0]
    rgb = torch.empty((R, 3), device=o.device, dtype=torch.float32)
    depth = torch.empty(R, device=o.device, dtype=torch.float32)
    acc = torch.zeros(R, device=o.device, dtype=torch.float32)                                   # misses: acc forced 0, :311
    if layers is not None:
        l_rgb, l_depth, l_acc = _new_layers(layers, R, 2, o.device)
    for i, j in _chunks(R):
        oc, dc = o[i:j].contiguous(), d[i:j].contiguous()
        n = torch.full((j - i,), float(bkg_near), device=o.device, dtype=torch.float32)
        f = torch.full((j - i,), float(bkg_far), device=o.device, dtype=torch.float32)
        given_z = given['bkg_z'][i:j] if given is not None and 'bkg_z' in given else None

        def human_lists(merge_z=None):
            near, far = _given_near_far(given, 0, i, j, oc, dc, posed_verts, geo_threshold)
            _note(trace, near=near, far=far)
            hit, _ = ray_utils.compact_hits(near, far)
            if hit.numel() == 0:
                return hit, None, None, None, None
            ho, hd = ray_utils.gather_rows(oc, hit), ray_utils.gather_rows(dc, hit)
            hn, hf = ray_utils.gather_rows(near, hit), ray_utils.gather_rows(far, hit)
            _note(trace, hit=hit + i)
            if TERMINATION_EPS > 0:
                mstats = {} if trace is not None else None
                dz_h = None
                if merge_z is not None:                                                            # the intervals the body's samples have once merged
                    _, _, h_z0 = ray_utils.sample_z(ho, hd, hn, hf, samples_per_ray)
                    dz_h = merged_intervals([ray_utils.gather_rows(merge_z, hit), h_z0])[1]
                h_raw, h_z = human_march_rays(human_net, ho, hd, hn, hf, samples_per_ray, mesh, TERMINATION_EPS, 1.0, precision, None, trace, mstats,
                                              dz=dz_h)
                _note(trace, march_human=mstats)
            else:
                h_raw, h_z = human_pass_rays(human_net, ho, hd, hn, hf, samples_per_ray, mesh, False, 1.0, precision, trace)
            return hit, hd, hf, h_raw, h_z

        if TERMINATION_EPS > 0 and given_z is None:
            # sample positions first (they do not depend on the body), then the body -- it may hide the background -- then the
            # background shading pass; both marched on the transmittance of the MERGED list (merged_intervals): a pixel moves < 2 eps
            bkg_z, _ = bkg_place_z(coarse_bkg, fine_bkg, oc, dc, n, f, samples_per_ray, importance_samples_per_ray, white_bkg, precision, trace)
            _note(trace, bkg_z=bkg_z)
            dz_b = torch.cat([bkg_z[:, 1:] - bkg_z[:, :-1], torch.full_like(bkg_z[:, :1], 1e10)], 1)
            hit, hd, hf, h_raw, h_z = human_lists(bkg_z)
            occluder = None
            if hit.numel() > 0:
                z_far = torch.full((j - i,), float('inf'), device=o.device, dtype=torch.float32)
                T_occ = torch.ones(j - i, device=o.device, dtype=torch.float32)
                dz_bh, dz_h = merged_intervals([ray_utils.gather_rows(bkg_z, hit), h_z])
                ray_utils.scatter_rows(dz_b, hit, dz_bh)
                ray_utils.scatter_rows(z_far, hit, hf.reshape(-1))
                ray_utils.scatter_rows(T_occ, hit, transmittance_of(h_raw, h_z, hd, dz_h))
                occluder = (z_far, T_occ)
            bkg_raw = bkg_shade(fine_bkg if fine_bkg is not None else coarse_bkg, oc, dc, bkg_z, precision, trace, occluder, dz_b.contiguous(),
                                composite_only=LIVE_HEADS)
        else:
            bkg_raw, bkg_z = bkg_pass_rays(coarse_bkg, fine_bkg, oc, dc, n, f, samples_per_ray, importance_samples_per_ray,
                                           white_bkg, precision, trace, given_z, composite_only=LIVE_HEADS)
            hit, hd, hf, h_raw, h_z = human_lists()
        # every ray first gets the background-only composite (what the reference does for misses, :303-311) ...
        if layers is None:
            rgb[i:j], _, _, _, depth[i:j] = raw2outputs(bkg_raw, bkg_z, dc, white_bkg=white_bkg, want_weights=False)
        else:                                                      # (the same composite as a one-list layered merge: its premultiplied sums are layer 0)
            rgb[i:j], depth[i:j], _, lr, ld, la = merge_composite_layers([bkg_z], [bkg_raw], dc, white_bkg)
            l_rgb[i:j, 0], l_depth[i:j, 0], l_acc[i:j, 0] = lr[:, 0], ld[:, 0], la[:, 0]
        if hit.numel() == 0:
            continue
        # ... and hit rays are overwritten by the merged human + background composite (:313-353)
        if layers is None:
            _rgb, _depth, _ = merge_composite_lists([bkg_z, h_z], [bkg_raw, h_raw], hd, white_bkg, rows=[hit, None])     # (the background rows in place)
        else:
            _rgb, _depth, _, lr, ld, la = merge_composite_layers([bkg_z, h_z], [bkg_raw, h_raw], hd, white_bkg, rows=[hit, None])
            for dst, src in ((l_rgb, lr), (l_depth, ld), (l_acc, la)):
                ray_utils.scatter_rows(dst[i:j], hit, src)
        _, _, _acc, _, _ = raw2outputs(h_raw, h_z, hd, white_bkg=white_bkg, want_weights=False)          # :345-350
        ray_utils.scatter_rows(rgb[i:j], hit, _rgb)
        ray_utils.scatter_rows(depth[i:j], hit, _depth)
        ray_utils.scatter_rows(acc[i:j], hit, _acc)
    return rgb, depth, acc


def render_hybrid_rays_fused(coarse_bkg, fine_bkg, human_net, o, d, bkg_near, bkg_far, posed_verts, mesh, samples_per_ray,
                             importance_samples_per_ray, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH, precision=None, live=None):
    """render_hybrid_rays' batch body as ONE C call (nm_render_rays_hybrid): same kernels, same bits; no trace / replay / early
    termination hooks -- the plain path of a frame render.  live (default: LIVE_HEADS): nm_render_rays_hybrid_live -- the fine background pass
    and the hit rays' human pass evaluate the colour head on their live samples only; rgb, depth and acc are bit-identical."""
    _lib.require_gpu()
    R = o.shape[0]
    dev = o.device
    rgb = torch.empty((R, 3), device=dev, dtype=torch.float32)
    depth = torch.empty(R, device=dev, dtype=torch.float32)
    acc = torch.empty(R, device=dev, dtype=torch.float32)
    S, N, Sh = int(samples_per_ray), int(importance_samples_per_ray) if fine_bkg is not None else 0, int(samples_per_ray)
    verts = posed_verts.to(dev, torch.float32).contiguous()
    t_vals = torch.linspace(0., 1., steps=S, device=dev)
    u = torch.linspace(0., 1., steps=N, device=dev) if N else None
    # the C call sizes its hit-ray buffers for every ray of the batch (it cannot read the hit count back without a host
    # synchronisation): ~28 KB per ray at 128 + 128 + 128 samples, so batches of FUSED_HYBRID_RAYS rays (3.7 GB) and ONE workspace
    step = min(MAX_RAYS_PER_LAUNCH, FUSED_HYBRID_RAYS)
    ws = _ws(_lib.lib().nm_render_rays_hybrid_workspace_floats(min(R, step), S, N, Sh), dev)
    precs = (coarse_bkg._prec(precision, None if fine_bkg is not None else 'shading'), fine_bkg._prec(precision, 'shading') if fine_bkg is not None else 0,
             human_net._prec(precision, 'shading'))
    n_live = min(R, step) * max(S + N, Sh)                                           # the larger of the two composited passes of a batch
    live = (LIVE_HEADS if live is None else bool(live)) and n_live >= vanilla.LIVE_MIN_SAMPLES and _lib.NM_PREC_I8X3 in (precs[1] if N else precs[0], precs[2])
    lws, lbytes = vanilla.live_workspace_for(n_live, 0, dev) if live else (None, 0)
    tail = (_lib.dev_ptr(lws, torch.uint8), lbytes, 0, _lib.stream_ptr()) if live else (_lib.stream_ptr(),)
    entry = _lib.lib().nm_render_rays_hybrid_live if live else _lib.lib().nm_render_rays_hybrid
    for i in range(0, R, step):
        j = min(i + step, R)
        oc, dc = o[i:j].contiguous(), d[i:j].contiguous()
        n = j - i
        r_, d_, a_ = rgb[i:j], depth[i:j], acc[i:j]
        _lib.check(entry(
            coarse_bkg.handle(), fine_bkg.handle() if fine_bkg is not None else None, human_net.handle(), mesh.handle, _lib.dev_ptr(mesh.T, torch.float64, 'T'),
            _lib.dev_ptr(verts), verts.shape[0], float(geo_threshold), _lib.dev_ptr(oc), _lib.dev_ptr(dc), n, float(bkg_near), float(bkg_far), S, N, Sh,
            _lib.dev_ptr(t_vals), _lib.dev_ptr(u), _lib.dev_ptr(t_vals), int(bool(white_bkg)),
            precs[0], precs[1], precs[2], _lib.dev_ptr(ws), _lib.dev_ptr(r_), _lib.dev_ptr(d_), _lib.dev_ptr(a_), *tail),
            "nm_render_rays_hybrid_live" if live else "nm_render_rays_hybrid")
    return rgb, depth, acc


def multi_merge_stages(n_actors, samples_per_ray, importance_samples_per_ray):
    """Can the one-kernel merge of render_multi_rays_fused stage the background list and `n_actors` actor lists of these sizes?  (Up to three
    actors: nm_merge_composite_lists; beyond: nm_merge_composite_lists_wide.)"""
    total = int(samples_per_ray) + int(importance_samples_per_ray) + int(n_actors) * int(samples_per_ray)
    if n_actors <= 3:
        return total <= MERGE_MAX_SAMPLES
    return 1 + n_actors <= WIDE_MERGE_MAX_LISTS and total <= WIDE_MERGE_MAX_SAMPLES


def render_multi_rays_fused(coarse_bkg, fine_bkg, human_nets, o, d, bkg_near, bkg_far, posed_verts, meshes, samples_per_ray,
                            importance_samples_per_ray, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH, precision=None, live=None):
    """render_multi_rays' batch body as ONE C call per batch (nm_render_rays_multi; render_utils.py:390-456) for any number of actors:
    same kernels up to the merge, same bits; no trace / replay / early termination hooks -- the plain path of a frame render.  With more than
    three actors the lists are merged and composited by ONE kernel (nm_merge_composite_lists_wide) from compact per-actor arrays, instead of
    full [rays, S] arrays merged list by list through HBM.  live (default: LIVE_HEADS): nm_render_rays_multi_live, as render_hybrid_rays_fused.
    -> (rgb [R,3], depth [R])"""
    _lib.require_gpu()
    R = o.shape[0]
    dev = o.device
    A = len(human_nets)
    rgb = torch.empty((R, 3), device=dev, dtype=torch.float32)
    depth = torch.empty(R, device=dev, dtype=torch.float32)
    S, N, Sh = int(samples_per_ray), int(importance_samples_per_ray) if fine_bkg is not None else 0, int(samples_per_ray)
    if not multi_merge_stages(A, S, N):
        raise _lib.NeumanHipError(f"render_multi_rays_fused: {S + N} + {A} x {Sh} merged samples exceed what the one-kernel merge stages")
    verts = [v.to(dev, torch.float32).contiguous() for v in posed_verts]
    t_vals = torch.linspace(0., 1., steps=S, device=dev)
    u = torch.linspace(0., 1., steps=N, device=dev) if N else None
    far_z = torch.linspace(float(bkg_far) * 2, float(bkg_far) * 3, samples_per_ray, device=dev)        # :418-419
    # the C call sizes every actor's compact arrays for all rays of the batch (the hit counts are only known inside): batches of
    # FUSED_MULTI_RAYS rays and ONE workspace
    step = max(1, min(MAX_RAYS_PER_LAUNCH, FUSED_MULTI_RAYS))
    ws = _ws(_lib.lib().nm_render_rays_multi_workspace_floats(min(R, step), S, N, Sh, A), dev)
    last_net = fine_bkg if fine_bkg is not None else coarse_bkg
    precs = (coarse_bkg._prec(precision, None if fine_bkg is not None else 'shading'), fine_bkg._prec(precision, 'shading') if fine_bkg is not None else 0,
             human_nets[0]._prec(precision, 'shading') if A else 0)
    for h in human_nets[1:]:
        if h._prec(precision, 'shading') != precs[2]:
            raise _lib.NeumanHipError("render_multi_rays_fused: the actors' nets run at one precision")
    # the mixed policy's re-evaluation of every ray's last background sample (render_multi_rays)
    prec_last = _lib.PRECISIONS['fp16x3'] if (last_net._prec(precision, 'shading') == _lib.NM_PREC_I8X3 and (precision or last_net.precision) == 'mixed') else 0
    n_live = min(R, step) * max(S + N, Sh if A else 0)
    live = (LIVE_HEADS if live is None else bool(live)) and n_live >= vanilla.LIVE_MIN_SAMPLES and _lib.NM_PREC_I8X3 in (precs[1] if N else precs[0], precs[2])
    lws, lbytes = vanilla.live_workspace_for(n_live, 0, dev) if live else (None, 0)
    tail = (_lib.dev_ptr(lws, torch.uint8), lbytes, 0, _lib.stream_ptr()) if live else (_lib.stream_ptr(),)
    entry = _lib.lib().nm_render_rays_multi_live if live else _lib.lib().nm_render_rays_multi
    arr = ctypes.c_void_p * max(A, 1)
    humans = arr(*[h.handle() for h in human_nets]) if A else None
    mesh_h = arr(*[m.handle for m in meshes]) if A else None
    Ts = arr(*[_lib.dev_ptr(m.T, torch.float64, 'T') for m in meshes]) if A else None
    vs = arr(*[v.data_ptr() for v in verts]) if A else None
    Vs = (ctypes.c_int * max(A, 1))(*[int(v.shape[0]) for v in verts]) if A else None
    for i in range(0, R, step):
        j = min(i + step, R)
        oc, dc = o[i:j].contiguous(), d[i:j].contiguous()
        r_, d_ = rgb[i:j], depth[i:j]
        _lib.check(entry(
            coarse_bkg.handle(), fine_bkg.handle() if fine_bkg is not None else None, A, humans, mesh_h, Ts, vs, Vs, float(geo_threshold), _lib.dev_ptr(oc),
            _lib.dev_ptr(dc), j - i, float(bkg_near), float(bkg_far), S, N, Sh, _lib.dev_ptr(t_vals), _lib.dev_ptr(u), _lib.dev_ptr(t_vals), _lib.dev_ptr(far_z),
            int(bool(white_bkg)), precs[0], precs[1], prec_last, precs[2], _lib.dev_ptr(ws), _lib.dev_ptr(r_), _lib.dev_ptr(d_), *tail),
            "nm_render_rays_multi_live" if live else "nm_render_rays_multi")
    return rgb, depth


def render_multi_rays(coarse_bkg, fine_bkg, human_nets, o, d, bkg_near, bkg_far, posed_verts, meshes, samples_per_ray,
                      importance_samples_per_ray, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH, precision=None, trace=None,
                      given=None):
    """Device core of render_hybrid_nerf_multi_persons -> (rgb [R,3], depth [R]) CUDA  (render_utils.py:390-456).  `given`: see
    bkg_pass_rays.  TERMINATION_EPS > 0: as render_hybrid_rays (sample positions of all lists, then the actors, then the background
    shading pass, each marched on the transmittance of its samples over their intervals in the MERGED list; the background behind the
    farthest body a ray hits on its own x all the bodies'); a pixel moves by < (1 + actors) eps.  The composite-only rule (LIVE_HEADS above) holds
    for every raw of the body but one: with TERMINATION_EPS > 0 the marched background pass tells "never reached" from the colours of its last
    sample, so that pass stays whole-network ('shading')."""
    S_max = int(samples_per_ray) + (int(importance_samples_per_ray) if fine_bkg is not None else 0)
    with raw_composited_only(min(o.shape[0], MAX_RAYS_PER_LAUNCH) * S_max, o.device):
        return _render_multi_rays(coarse_bkg, fine_bkg, human_nets, o, d, bkg_near, bkg_far, posed_verts, meshes, samples_per_ray, importance_samples_per_ray,
                                  white_bkg, geo_threshold, precision, trace, given)


def render_multi_layers_rays(coarse_bkg, fine_bkg, human_nets, o, d, bkg_near, bkg_far, posed_verts, meshes, samples_per_ray,
                             importance_samples_per_ray, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH, precision=None, trace=None,
                             given=None):
    """render_multi_rays with the picture kept in layers: same arguments (up to 31 actors) -> dict of rgb [R,3] and depth [R] (bit-identical to
    render_multi_rays) and layer_rgb [R,L,3], layer_depth [R,L], layer_acc [R,L], L = 1 + actors: layer 0 the background, layer 1 + a actor a in
    the caller's order, each the premultiplied sums of its own samples with the weights they have in the merged list (merge_composite_layers).
    The step-by-step body with its last merge exchanged; never the one-call route."""
    S_max = int(samples_per_ray) + (int(importance_samples_per_ray) if fine_bkg is not None else 0)
    layers = {}
    with raw_composited_only(min(o.shape[0], MAX_RAYS_PER_LAUNCH) * S_max, o.device):
        rgb, depth = _render_multi_rays(coarse_bkg, fine_bkg, human_nets, o, d, bkg_near, bkg_far, posed_verts, meshes, samples_per_ray,
                                        importance_samples_per_ray, white_bkg, geo_threshold, precision, trace, given, layers=layers)
    return dict(rgb=rgb, depth=depth, **layers)


def _render_multi_rays(coarse_bkg, fine_bkg, human_nets, o, d, bkg_near, bkg_far, posed_verts, meshes, samples_per_ray, importance_samples_per_ray, white_bkg,
                       geo_threshold, precision, trace, given, layers=None):
    if (layers is None and MULTI_FUSED and TERMINATION_EPS <= 0 and trace is None and given is None and not _occupancy_on(coarse_bkg, fine_bkg)
            and all(occupancy.grid_of(h_) is None for h_ in human_nets)
            and len({h_._prec(precision, 'shading') for h_ in human_nets}) <= 1                   # (the call takes ONE precision for the actors' nets)
            and multi_merge_stages(len(human_nets), samples_per_ray, importance_samples_per_ray if fine_bkg is not None else 0)):
        return render_multi_rays_fused(coarse_bkg, fine_bkg, human_nets, o, d, bkg_near, bkg_far, posed_verts, meshes, samples_per_ray,
                                       importance_samples_per_ray, white_bkg, geo_threshold, precision)
    R = o.shape[0]
    rgb = torch.empty((R, 3), device=o.device, dtype=torch.float32)
    depth = torch.empty(R, device=o.device, dtype=torch.float32)
    if layers is not None:
        l_rgb, l_depth, l_acc = _new_layers(layers, R, 1 + len(human_nets), o.device)
    for i, j in _chunks(R):
        oc, dc = o[i:j].contiguous(), d[i:j].contiguous()
        nr = j - i
        n = torch.full((nr,), float(bkg_near), device=o.device, dtype=torch.float32)
        f = torch.full((nr,), float(bkg_far), device=o.device, dtype=torch.float32)
        far_z = torch.linspace(float(bkg_far) * 2, float(bkg_far) * 3, samples_per_ray, device=o.device)   # :418-419

        def actor_rays(a_):
            """one actor's hit list and the z of its list over ALL rays of the batch: its samples where it is hit, the zero-density
            placeholders elsewhere (render_utils.py:405-419)"""
            near, far = _given_near_far(given, a_, i, j, oc, dc, posed_verts[a_], geo_threshold)
            _note(trace, near=near, far=far)
            h_z = far_z[None].repeat(nr, 1).contiguous()
            hit, _ = ray_utils.compact_hits(near, far)
            _note(trace, hit=hit + i)
            if hit.numel() == 0:
                return hit, None, h_z
            ho, hd = ray_utils.gather_rows(oc, hit), ray_utils.gather_rows(dc, hit)
            hn, hf = ray_utils.gather_rows(near, hit), ray_utils.gather_rows(far, hit)
            return hit, (ho, hd, hn, hf), h_z

        def actor_lists_compact(a_):
            """the actor's list as COMPACT arrays for merge_composite_lists' `rows` indirection: the evaluated rows of the hit rays followed by ONE placeholder row
            (the zero-density samples at linspace(2 far, 3 far), render_utils.py:418-419) that every missed ray points at -> (z [n_hit + 1, S], raw [n_hit + 1, S, 4],
            rows [nr] int32).  The same values the full [nr, S] arrays hold, without filling, scattering and streaming 16 KB per missed ray and actor."""
            near, far = _given_near_far(given, a_, i, j, oc, dc, posed_verts[a_], geo_threshold)
            _note(trace, near=near, far=far)
            hit, _ = ray_utils.compact_hits(near, far)
            _note(trace, hit=hit + i)
            n_hit = int(hit.numel())
            rows = torch.full((nr,), n_hit, device=o.device, dtype=torch.int32)
            pad_raw = torch.zeros((1, samples_per_ray, 4), device=o.device, dtype=torch.float32)
            if n_hit == 0:
                _note(trace, human_z=None, can_pts=None, can_dirs=None)
                return far_z[None].contiguous(), pad_raw, rows
            ho, hd = ray_utils.gather_rows(oc, hit), ray_utils.gather_rows(dc, hit)
            hn, hf = ray_utils.gather_rows(near, hit), ray_utils.gather_rows(far, hit)
            r_, z_ = human_pass_rays(human_nets[a_], ho, hd, hn, hf, samples_per_ray, meshes[a_], False, 1.0, precision, trace)
            rows[hit.to(torch.int64)] = torch.arange(n_hit, device=o.device, dtype=torch.int32)
            return torch.cat([z_, far_z[None]], 0), torch.cat([r_, pad_raw], 0), rows

        def actor_lists(a_, rays=None, dz=None):
            """the actor's list evaluated -> (h_z [nr,S], h_raw [nr,S,4], (hit, far, transmittance over `dz`) when marched)"""
            hit, hr, h_z = rays if rays is not None else actor_rays(a_)
            h_raw = torch.zeros((nr, samples_per_ray, 4), device=o.device, dtype=torch.float32)
            occ = None
            if hit.numel() > 0:
                ho, hd, hn, hf = hr
                if TERMINATION_EPS > 0:
                    mstats = {} if trace is not None else None
                    dz_h = ray_utils.gather_rows(dz, hit) if dz is not None else None
                    r_, z_ = human_march_rays(human_nets[a_], ho, hd, hn, hf, samples_per_ray, meshes[a_], TERMINATION_EPS, 1.0, precision, None, trace,
                                              mstats, dz=dz_h)
                    _note(trace, march_human=mstats)
                    occ = (hit, hf.reshape(-1), transmittance_of(r_, z_, hd, dz_h))
                else:
                    r_, z_ = human_pass_rays(human_nets[a_], ho, hd, hn, hf, samples_per_ray, meshes[a_], False, 1.0, precision, trace)
                ray_utils.scatter_rows(h_raw.reshape(nr, -1), hit, r_.reshape(hit.shape[0], -1))
                ray_utils.scatter_rows(h_z, hit, z_)
            else:
                _note(trace, human_z=None, can_pts=None, can_dirs=None)
            return h_z, h_raw, occ

        lists = None
        given_z = given['bkg_z'][i:j] if given is not None and 'bkg_z' in given else None
        if TERMINATION_EPS > 0 and given_z is None:
            # sample positions of every list first (none depends on another list's densities), then the bodies -- they may hide the
            # background -- then the background shading pass, each marched on the transmittance its samples have in the MERGED list
            z_all, _ = bkg_place_z(coarse_bkg, fine_bkg, oc, dc, n, f, samples_per_ray, importance_samples_per_ray, white_bkg, precision, trace)
            _note(trace, bkg_z=z_all)
            rays_l = [actor_rays(a_) for a_ in range(len(human_nets))]
            for hit, hr, h_z in rays_l:                                                              # (z of the hit rows, as human_march_rays will sample them)
                if hit.numel() > 0:
                    ray_utils.scatter_rows(h_z, hit, ray_utils.sample_z(hr[0], hr[1], hr[2], hr[3], samples_per_ray)[2])
            dz_l = merged_intervals([z_all] + [h_z for _, _, h_z in rays_l])
            lists = [actor_lists(a_, rays_l[a_], dz_l[1 + a_]) for a_ in range(len(human_nets))]
            z_far = torch.full((nr,), float('-inf'), device=o.device, dtype=torch.float32)
            T_occ = torch.ones(nr, device=o.device, dtype=torch.float32)
            for _, _, occ in lists:
                if occ is not None:
                    hit, hf, Th = occ
                    idx = hit.to(torch.int64)
                    z_far[idx] = torch.maximum(z_far[idx], hf)
                    T_occ[idx] = T_occ[idx] * Th
            z_far = torch.where(torch.isinf(z_far), torch.full_like(z_far, float('inf')), z_far)  # rays that hit nobody: never
            raw_all = bkg_shade(fine_bkg if fine_bkg is not None else coarse_bkg, oc, dc, z_all, precision, trace, (z_far, T_occ), dz_l[0])
        else:
            raw_all, z_all = bkg_pass_rays(coarse_bkg, fine_bkg, oc, dc, n, f, samples_per_ray, importance_samples_per_ray,
                                           white_bkg, precision, trace, given_z, composite_only=LIVE_HEADS)
        # In this renderer the terminal 1e10 interval sits on an actor's zero-density placeholder whenever a ray misses one
        # (render_utils.py:418-419), so the LAST background sample is followed by a finite interval of ~far..2 far instead:
        # alpha = 1 - exp(-sigma * 3.14..) is then ~300x as sensitive to that one sigma as a sample inside the ray is.  Under the
        # mixed policy (i8x3 shading passes) that single sample per ray is re-evaluated in the float32-class arithmetic.
        last_net = fine_bkg if fine_bkg is not None else coarse_bkg
        if last_net._prec(precision, 'shading') == _lib.NM_PREC_I8X3 and (precision or last_net.precision) == 'mixed':
            last = last_net.forward_rays(oc, dc, z_all[:, -1:].contiguous(), precision='fp16x3')[:, 0, :]
            if TERMINATION_EPS > 0:                                                              # a sample the march never reached (or, marched with a grid, that the grid skipped) stays unevaluated
                last = torch.where((raw_all[:, -1, :] == 0).all(-1, keepdim=True), raw_all[:, -1, :], last)
            raw_all[:, -1, :] = last
        if layers is not None:                                                                   # the same lists, compact or full, through the layered merge
            if lists is None and MULTI_COMPACT:
                cl = [actor_lists_compact(a_) for a_ in range(len(human_nets))]
                zs, raws, rws = [z_all] + [c[0] for c in cl], [raw_all] + [c[1] for c in cl], [None] + [c[2] for c in cl]
            else:
                lists = [actor_lists(a_) for a_ in range(len(human_nets))] if lists is None else lists
                zs, raws, rws = [z_all] + [l_[0] for l_ in lists], [raw_all] + [l_[1] for l_ in lists], None
            rgb[i:j], depth[i:j], _, l_rgb[i:j], l_depth[i:j], l_acc[i:j] = merge_composite_layers(zs, raws, dc, white_bkg, rows=rws)
            continue
        if lists is None and len(human_nets) <= 3 and MULTI_COMPACT:
            cl = [actor_lists_compact(a_) for a_ in range(len(human_nets))]
            rgb[i:j], depth[i:j], _ = merge_composite_lists([z_all] + [c[0] for c in cl], [raw_all] + [c[1] for c in cl], dc, white_bkg, rows=[None] + [c[2] for c in cl])
            continue
        if lists is None:
            lists = [actor_lists(a_) for a_ in range(len(human_nets))]
        if len(lists) <= 3:                                                                      # :441-456 as one kernel: 4-way merge + composite
            rgb[i:j], depth[i:j], _ = merge_composite_lists([z_all] + [l_[0] for l_ in lists], [raw_all] + [l_[1] for l_ in lists], dc, white_bkg)
        else:                                                                                    # more than three actors: list by list
            for h_z, h_raw, _ in lists:
                z_all, raw_all = merge_sorted(z_all, raw_all, h_z, h_raw)
            rgb[i:j], _, _, _, depth[i:j] = raw2outputs(raw_all, z_all, dc, white_bkg=white_bkg, want_weights=False)
    return rgb, depth


# ------------------------------------------------------------------------------------------------
# the reference's frame renderers (same signatures, numpy out)
# ------------------------------------------------------------------------------------------------
def _device_of(net):
    dev = next(net.parameters()).device
    if dev.type != 'cuda':
        raise _lib.NeumanHipError("the network must live on the HIP device (net.cuda()): there is no CPU render path")
    return dev


MULTI_COMPACT = os.environ.get("NEUMAN_MULTI_COMPACT", "1") != "0"   # the multi-person merge reads compact per-actor lists through row indices (0: full [R, S] arrays, A/B)
HOST_RAYS = os.environ.get("NEUMAN_HOST_RAYS", "0") == "1"     # A/B switch: generate rays with the host (numpy) mirror and upload them


def _pixel_rays(cap, device):
    """shot_rays over every pixel, (x, y) row-major (render_utils.py:185-186)."""
    h, w = cap.shape
    if HOST_RAYS:
        coords = np.argwhere(np.ones(cap.shape))[:, ::-1]
        o, d = ray_utils.shot_rays(cap, coords)
        return (torch.from_numpy(o).to(device, torch.float32).contiguous(),
                torch.from_numpy(d).to(device, torch.float32).contiguous())
    i = torch.arange(h * w, device=device, dtype=torch.int32)
    return ray_utils.shot_rays_dev(cap, torch.stack([i % w, i // w], dim=1))


def _all_rays(cap, device):
    """shot_all_rays (render_utils.py:125-128)."""
    if HOST_RAYS:
        o, d = ray_utils.shot_all_rays(cap)
        return (torch.from_numpy(o).to(device, torch.float32).contiguous(),
                torch.from_numpy(d).to(device, torch.float32).contiguous())
    return ray_utils.shot_all_rays_dev(cap, device)


def _frame(rays_fn, o, d):
    """The frame's rays through `rays_fn` -> tuple of per-ray tensors: on this device alone, or -- under an initialised process
    group (parallel.sharding_active) -- the rays of this rank's interleaved tiles only, with ONE gather assembling the frame on
    rank 0 (None on the other ranks; parallel.render_frame_sharded)."""
    if parallel.sharding_active():
        return parallel.render_frame_sharded(rays_fn, o, d)
    return rays_fn(o, d)


# ------------------------------------------------------------------------------------------------
# frame egress (reference render_test_views.py:83-92, 27-41): uint8 pixels and their PSNR, on the device
# ------------------------------------------------------------------------------------------------
def frame_to_uint8(frame):
    """What `imageio.imsave(path, out)` makes of a renderer's float frame before encoding: clip to [0, 1],
    `uint8(x * 255 + 0.499999999)`.  CUDA f32 tensor of any shape -> uint8 tensor of the same shape."""
    _lib.require_gpu()
    src = frame.to(torch.float32).contiguous()
    dst = torch.empty(src.shape, device=src.device, dtype=torch.uint8)
    _lib.check(_lib.lib().nm_frame_to_uint8(_lib.dev_ptr(src), src.numel(), ctypes.c_void_p(dst.data_ptr()), _lib.stream_ptr()),
               "nm_frame_to_uint8")
    return dst


def psnr_uint8(gt, pred):
    """skimage.metrics.peak_signal_noise_ratio(gt, pred) for uint8 frames (render_test_views.py:35): 10 log10(255^2 / mse)."""
    _lib.require_gpu()
    if gt.dtype != torch.uint8 or pred.dtype != torch.uint8 or gt.shape != pred.shape or not (gt.is_cuda and pred.is_cuda):
        raise _lib.NeumanHipError("psnr_uint8 takes two CUDA uint8 tensors of the same shape")
    gt, pred = gt.contiguous(), pred.contiguous()
    ssd = torch.empty(1, device=gt.device, dtype=torch.int64)
    _lib.check(_lib.lib().nm_ssd_u8(ctypes.c_void_p(gt.data_ptr()), ctypes.c_void_p(pred.data_ptr()), gt.numel(),
                                    ctypes.c_void_p(ssd.data_ptr()), _lib.stream_ptr()), "nm_ssd_u8")
    mse = float(ssd.item()) / gt.numel()
    return float('inf') if mse == 0 else 10.0 * float(np.log10(255.0 ** 2 / mse))


def save_png(path, frame):
    """imageio.imsave(path, frame) for the renderers' output (render_test_views.py:83-88, render_360.py:77-81): a float frame goes
    through `frame_to_uint8` on the device, then an 8-bit RGB / grey PNG is written with the standard library (zlib): same
    pixels as imageio's file, not the same bytes (deflate settings differ)."""
    import struct
    import zlib
    if isinstance(frame, np.ndarray):
        frame = torch.as_tensor(np.ascontiguousarray(frame))
    if frame.dtype != torch.uint8:
        frame = frame_to_uint8(frame.to('cuda', torch.float32))
    a = frame.cpu().numpy()
    if a.ndim == 2:
        a = a[..., None]
    h, w, c = a.shape
    if c not in (1, 3, 4):
        raise ValueError(f"save_png: {c} channels")
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * c)], 1).tobytes()          # filter type 0 on every row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def ssim_uint8(pred, gt):
    """skimage.metrics.structural_similarity(pred, gt, multichannel=True) for uint8 [H,W,C] frames (render_test_views.py:33)."""
    _lib.require_gpu()
    if gt.dtype != torch.uint8 or pred.dtype != torch.uint8 or gt.shape != pred.shape or gt.dim() != 3 or not (gt.is_cuda and pred.is_cuda):
        raise _lib.NeumanHipError("ssim_uint8 takes two CUDA uint8 tensors [H,W,C] of the same shape")
    gt, pred = gt.contiguous(), pred.contiguous()
    out = torch.empty(1, device=gt.device, dtype=torch.float64)
    ws = torch.empty(4096, device=gt.device, dtype=torch.float64)
    H, W, C = gt.shape
    _lib.check(_lib.lib().nm_ssim_u8(ctypes.c_void_p(pred.data_ptr()), ctypes.c_void_p(gt.data_ptr()), H, W, C, ctypes.c_void_p(out.data_ptr()),
                                     ctypes.c_void_p(ws.data_ptr()), _lib.stream_ptr()), "nm_ssim_u8")
    return float(out.item())


def render_vanilla(coarse_net, cap, fine_net=None, rays_per_batch=32768, samples_per_ray=64, importance_samples_per_ray=128,
                   white_bkg=True, near_far_source='bkg', return_depth=False, ablate_nerft=False):
    """reference render_utils.py:108-161."""
    device = _device_of(coarse_net)
    if ablate_nerft:
        # the frame's time is one constant (render_utils.py:134-148): the 4-D-encoding nets at that time ARE 3-D-encoding nets with two
        # other bias vectors (vanilla.frozen_time_joiner) -- everything below, sharding included, is the ordinary path on the MFMA kernels
        from . import vanilla
        cur_time = cap.frame_id['frame_id'] / cap.frame_id['total_frames']
        coarse_net = vanilla.frozen_time_joiner(coarse_net, cur_time)
        fine_net = vanilla.frozen_time_joiner(fine_net, cur_time) if fine_net is not None else None
    with torch.no_grad():
        o, d = _all_rays(cap, device)
        out = _frame(lambda oo, dd: render_vanilla_rays(coarse_net, fine_net, oo, dd, cap.near[near_far_source], cap.far[near_far_source],
                                                        samples_per_ray, importance_samples_per_ray, white_bkg), o, d)
        if out is None:                                                                          # a rank other than 0 of a sharded render
            return None
        rgb, depth = out
        rgb = rgb.reshape(*cap.shape, -1).cpu().numpy()
        depth = depth.reshape(*cap.shape).cpu().numpy()
    return (rgb, depth) if return_depth else rgb


def render_smpl_nerf(net, cap, posed_verts, faces, Ts, rays_per_batch=32768, samples_per_ray=64, white_bkg=True,
                     render_can=False, geo_threshold=DEFAULT_GEO_THRESH, return_depth=False, return_mask=False,
                     interval_comp=1.0):
    """reference render_utils.py:164-246."""
    device = _device_of(net)
    with torch.no_grad():
        o, d = _pixel_rays(cap, device)
        verts = torch.as_tensor(np.ascontiguousarray(posed_verts, dtype=np.float32)).to(device)
        mesh = None if render_can else ray_utils.mesh_to_device(posed_verts, faces, Ts, device)
        out = _frame(lambda oo, dd: render_smpl_nerf_rays(net.coarse_human_net, oo, dd, verts, mesh, samples_per_ray, white_bkg, render_can,
                                                          geo_threshold, interval_comp), o, d)
        if out is None:
            return None
        rgb, depth, acc = out
        rgb = rgb.reshape(*cap.shape, -1).cpu().numpy()
        depth = depth.reshape(*cap.shape).cpu().numpy()
        acc = acc.reshape(*cap.shape).cpu().numpy()
    if return_depth and return_mask:
        return rgb, depth, acc
    if return_depth:
        return rgb, depth
    if return_mask:
        return rgb, acc
    return rgb


def render_hybrid_nerf(net, cap, posed_verts, faces, Ts, rays_per_batch=32768, samples_per_ray=64,
                       importance_samples_per_ray=128, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH, return_depth=False):
    """reference render_utils.py:249-362."""
    device = _device_of(net)
    with torch.no_grad():
        o, d = _pixel_rays(cap, device)
        verts = torch.as_tensor(np.ascontiguousarray(posed_verts, dtype=np.float32)).to(device)
        mesh = ray_utils.mesh_to_device(posed_verts, faces, Ts, device)
        out = _frame(lambda oo, dd: render_hybrid_rays(net.coarse_bkg_net, net.fine_bkg_net, net.coarse_human_net, oo, dd, cap.near['bkg'],
                                                       cap.far['bkg'], verts, mesh, samples_per_ray, importance_samples_per_ray, white_bkg,
                                                       geo_threshold)[:2], o, d)
        if out is None:
            return None
        rgb, depth = out
        rgb = rgb.reshape(*cap.shape, -1).cpu().numpy()
        depth = depth.reshape(*cap.shape).cpu().numpy()
    return (rgb, depth) if return_depth else rgb


def render_hybrid_nerf_multi_persons(bkg_model, cap, human_models, posed_verts, faces, Ts, rays_per_batch=32768,
                                     samples_per_ray=64, importance_samples_per_ray=128, white_bkg=True,
                                     geo_threshold=DEFAULT_GEO_THRESH, return_depth=False):
    """reference render_utils.py:365-461."""
    device = _device_of(bkg_model)
    with torch.no_grad():
        o, d = _pixel_rays(cap, device)
        verts = [torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(device) for v in posed_verts]
        meshes = [ray_utils.mesh_to_device(v, f, t, device) for v, f, t in zip(posed_verts, faces, Ts)]
        out = _frame(lambda oo, dd: render_multi_rays(bkg_model.coarse_bkg_net, bkg_model.fine_bkg_net,
                                                      [m.coarse_human_net for m in human_models], oo, dd, cap.near['bkg'], cap.far['bkg'], verts,
                                                      meshes, samples_per_ray, importance_samples_per_ray, white_bkg, geo_threshold), o, d)
        if out is None:
            return None
        rgb, depth = out
        rgb = rgb.reshape(*cap.shape, -1).cpu().numpy()
        depth = depth.reshape(*cap.shape).cpu().numpy()
    return (rgb, depth) if return_depth else rgb


# ------------------------------------------------------------------------------------------------
# layered frames: the hybrid renderers' picture per source (background, each actor); no counterpart in the reference
# ------------------------------------------------------------------------------------------------
_LAYER_KEYS = ('rgb', 'depth', 'layer_rgb', 'layer_depth', 'layer_acc')


def _layers_frame(out, cap):
    """the per-ray tensors of a layered render (in _LAYER_KEYS' order) -> dict of numpy arrays [H,W,...]"""
    return {k_: x.reshape(*cap.shape, *x.shape[1:]).cpu().numpy() for k_, x in zip(_LAYER_KEYS, out)}


def render_hybrid_nerf_layers(net, cap, posed_verts, faces, Ts, rays_per_batch=32768, samples_per_ray=64,
                              importance_samples_per_ray=128, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH):
    """render_hybrid_nerf in layers (render_hybrid_layers_rays): dict of numpy rgb [H,W,3], depth [H,W] -- the frame render_hybrid_nerf returns -- and
    layer_rgb [H,W,2,3], layer_depth [H,W,2], layer_acc [H,W,2]: layer 0 the background, layer 1 the actor, premultiplied.  None on the ranks
    other than 0 of a sharded render."""
    device = _device_of(net)
    with torch.no_grad():
        o, d = _pixel_rays(cap, device)
        verts = torch.as_tensor(np.ascontiguousarray(posed_verts, dtype=np.float32)).to(device)
        mesh = ray_utils.mesh_to_device(posed_verts, faces, Ts, device)

        def rays_fn(oo, dd):
            out = render_hybrid_layers_rays(net.coarse_bkg_net, net.fine_bkg_net, net.coarse_human_net, oo, dd, cap.near['bkg'], cap.far['bkg'], verts, mesh,
                                            samples_per_ray, importance_samples_per_ray, white_bkg, geo_threshold)
            return tuple(out[k_] for k_ in _LAYER_KEYS)
        out = _frame(rays_fn, o, d)
        return None if out is None else _layers_frame(out, cap)


def render_hybrid_nerf_multi_persons_layers(bkg_model, cap, human_models, posed_verts, faces, Ts, rays_per_batch=32768, samples_per_ray=64,
                                            importance_samples_per_ray=128, white_bkg=True, geo_threshold=DEFAULT_GEO_THRESH):
    """render_hybrid_nerf_multi_persons in layers (render_multi_layers_rays): dict of numpy rgb [H,W,3], depth [H,W] and layer_rgb [H,W,L,3],
    layer_depth [H,W,L], layer_acc [H,W,L], L = 1 + actors: layer 0 the background, layer 1 + a actor a, premultiplied.  None on the ranks other
    than 0 of a sharded render."""
    device = _device_of(bkg_model)
    with torch.no_grad():
        o, d = _pixel_rays(cap, device)
        verts = [torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(device) for v in posed_verts]
        meshes = [ray_utils.mesh_to_device(v, f, t, device) for v, f, t in zip(posed_verts, faces, Ts)]

        def rays_fn(oo, dd):
            out = render_multi_layers_rays(bkg_model.coarse_bkg_net, bkg_model.fine_bkg_net, [m.coarse_human_net for m in human_models], oo, dd,
                                           cap.near['bkg'], cap.far['bkg'], verts, meshes, samples_per_ray, importance_samples_per_ray, white_bkg, geo_threshold)
            return tuple(out[k_] for k_ in _LAYER_KEYS)
        out = _frame(rays_fn, o, d)
        return None if out is None else _layers_frame(out, cap)


def layers_to_rgba_uint8(layer_rgb, layer_acc):
    """Premultiplied layers [..., 3] and their opacity [...] -> straight-alpha RGBA uint8 [..., 4] on the device (nm_layers_to_rgba8), what save_png
    writes as a 4-channel PNG: colour clamp(rgb / acc, 0, 1), 0 where acc <= 0; alpha clamp(acc, 0, 1); quantised as frame_to_uint8 does."""
    _lib.require_gpu()
    acc = torch.as_tensor(layer_acc).to('cuda', torch.float32).contiguous()
    rgb = torch.as_tensor(layer_rgb).to(acc.device, torch.float32).contiguous()
    if rgb.shape != (*acc.shape, 3):
        raise _lib.NeumanHipError(f"layers_to_rgba_uint8: layer_rgb {tuple(rgb.shape)} is not layer_acc {tuple(acc.shape)} + (3,)")
    dst = torch.empty((*acc.shape, 4), device=acc.device, dtype=torch.uint8)
    _lib.check(_lib.lib().nm_layers_to_rgba8(_lib.dev_ptr(rgb), _lib.dev_ptr(acc), acc.numel(), ctypes.c_void_p(dst.data_ptr()), _lib.stream_ptr()),
               "nm_layers_to_rgba8")
    return dst


def compose_over(layer_rgb, layer_acc, image, layers=None):
    """The chosen layers over an image: sum_l layer_rgb_l + (1 - sum_l layer_acc_l) image, l in `layers` (default: every actor layer, 1 .. L-1 -- the
    rendered actors over a photograph instead of over the background NeRF).  layer_rgb [...,L,3], layer_acc [...,L], image [...,3] (or a
    colour [3]); plain torch on the tensors' device."""
    layer_rgb, layer_acc = torch.as_tensor(layer_rgb), torch.as_tensor(layer_acc)
    idx = list(range(1, layer_acc.shape[-1])) if layers is None else [int(l_) for l_ in layers]
    image = torch.as_tensor(image).to(layer_rgb.device, layer_rgb.dtype)
    return layer_rgb[..., idx, :].sum(-2) + (1.0 - layer_acc[..., idx].sum(-1))[..., None] * image


# ------------------------------------------------------------------------------------------------
# the body as a rasterised mesh (reference render_utils.py:464-501; csrc/raster.hip, the contract in include/neuman_hip.h)
# ------------------------------------------------------------------------------------------------
def _raster_of(verts, faces, cap, **kw):
    from . import raster
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise _lib.NeumanHipError("verts must be a CUDA (HIP) tensor: the rasteriser has no CPU path")
    _lib.require_gpu()
    return raster.rasterizer_for(faces, verts.shape[0]).rasterize(verts, raster.camera_of(cap), **kw)


def rasterize_mesh(verts, faces, cap):
    """The mesh as `cap` sees it -> (face_id [H,W] int32, -1 where nothing covers the pixel centre; zbuf [H,W] f32 camera depth, +inf there;
    bary [H,W,3] f32 perspective-correct barycentrics of the winning face), device tensors.  verts [V,3] CUDA f32, faces [F,3]."""
    with torch.no_grad():
        return _raster_of(verts, faces, cap)[:3]


def body_mask(verts, faces, cap):
    """bool [H,W] on the device: the pixels whose centre the mesh covers."""
    with torch.no_grad():
        return _raster_of(verts, faces, cap, want_bary=False)[0] >= 0


def overlay_smpl(img, verts, faces, cap):
    """reference render_utils.py:485-501: the Phong-shaded white body over `img` (uint8 [H,W,3] numpy) -> uint8 [H,W,3] numpy.  Pixels the body
    does not cover keep img's bytes."""
    from . import raster
    with torch.no_grad():
        rgba = _raster_of(verts, faces, cap, want_bary=False, shade=True)[3]
        image = torch.as_tensor(np.ascontiguousarray(img))
        if image.dtype != torch.uint8:
            raise _lib.NeumanHipError(f"overlay_smpl: img must be uint8, got {image.dtype}")
        return raster.overlay_rgba(rgba, image[..., :3].contiguous().to(rgba.device)).cpu().numpy()


def soft_silhouette(verts, faces, cap, sigma=1e-4, blur_radius=None):
    """reference preprocess/optimize_smpl.py:84-102, 249-250: the body's soft silhouette as `cap` sees it -> alpha [H,W] f32 on the device,
    differentiable with respect to verts [V,3] (CUDA f32).  blur_radius defaults to log(1/1e-4 - 1) sigma (:92).  Every face within the blur
    radius counts, not the 100 nearest (the header's rule S4)."""
    from . import raster
    if not isinstance(verts, torch.Tensor) or not verts.is_cuda:
        raise _lib.NeumanHipError("verts must be a CUDA (HIP) tensor: the silhouette has no CPU path")
    _lib.require_gpu()
    return raster.soft_silhouette(raster.rasterizer_for(faces, verts.shape[0]), verts, raster.camera_of(cap), sigma, blur_radius)


def soft_silhouette_batch(world_verts, faces, caps, sigma=1e-4, blur_radius=None):
    """`soft_silhouette` for the frames of a sequence as one call: world_verts [B,V,3] (a CUDA tensor), caps the B captures (one image size;
    ValueError otherwise) or what `raster.batch_cameras` made of them -> alpha [B,H,W] f32, differentiable with respect to world_verts.
    Frame b's alpha and gradient are `soft_silhouette`'s bits on frame b."""
    from . import raster
    if not isinstance(world_verts, torch.Tensor) or not world_verts.is_cuda:
        raise _lib.NeumanHipError("world_verts must be a CUDA (HIP) tensor: the silhouette has no CPU path")
    _lib.require_gpu()
    cameras = caps if isinstance(caps, tuple) else raster.batch_cameras(caps, world_verts.device)
    return raster.soft_silhouette_batch(raster.rasterizer_for(faces, world_verts.shape[1]), world_verts, cameras, sigma, blur_radius)


# ------------------------------------------------------------------------------------------------
# the frames of an animated mesh (csrc/raster_frames.hip; the header's 'mesh frames', rules F1-F7): what mesh_extract made and mesh_pose posed,
# as images
# ------------------------------------------------------------------------------------------------
MESH_FRAMES_SCRATCH = 256 << 20                                # bytes of scratch render_mesh_frames' default chunk aims at


def mesh_frames_per_call(V, F, W, H, budget=MESH_FRAMES_SCRATCH):
    """The frames one nm_raster_frames call takes under `budget` bytes of the scratch the header states: 16 V + 12 ceil(W / 16) ceil(H / 16)
    per frame and 4 per list entry -- two entries per face assumed, which is what a mesh of faces smaller than a tile makes (a face enters
    the list of every tile its screen box touches); at least 1, at most the entry's 65535."""
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    return int(max(1, min(65535, budget // (16 * V + 12 * tiles + 8 * F))))


def depth_to_camera_z(depth, cap):
    """A renderer's depth map of `cap` (float32 [H,W] tensor: distances along the pixels' rays) -> camera-space z [H,W], what
    `render_mesh_frames` compares the mesh's depth with (rule F4): the distance times the component of the renderer's own unit ray
    direction (`_all_rays`) along the camera's optical axis."""
    from . import raster
    h, w = cap.shape
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or tuple(depth.shape) != (h, w):
        raise _lib.NeumanHipError(f"depth_to_camera_z: depth must be a float32 [{h}, {w}] tensor, got {getattr(depth, 'dtype', type(depth))} "
                                  f"{tuple(getattr(depth, 'shape', ()))}")
    d = _all_rays(cap, depth.device)[1]
    axis = torch.as_tensor(raster.camera_of(cap)[0][2, :3]).to(depth.device, torch.float32)      # the third row of R_w2c: the optical axis in world space
    return depth * (d @ axis).reshape(h, w)


def render_mesh_frames(world_verts, faces, caps, colours=None, normals=None, background=None, background_depth=None, light=None, frames_per_call=None, *,
                       face_colours=None, lod_scale=None):
    """The frames of a posed mesh as images -> uint8 [B,H,W,3] on the device.  world_verts [B,V,3] and normals [B,V,3] (optional: they switch
    the diffuse light on) as `mesh_pose.pose_mesh_frames` returns them, faces [F,3], colours [V,3] float32 as `mesh_extract.extract_net_mesh`
    returns them (None: white); caps the B captures (one image size; ValueError otherwise) or what `raster.batch_cameras` made of them.
    background uint8 [B,H,W,3], or [H,W,3] for all frames (None: white); background_depth float32 [B,H,W], the renderers' depth maps of the
    same captures: the mesh shows where it is nearer (`depth_to_camera_z` makes the comparison a camera-space one; it needs the captures
    themselves).  light: the world-space position of the point light, `raster.LIGHT` by default.  Every tensor is a CUDA tensor on one
    device and is taken as it is: nothing is converted.  The sequence goes through nm_raster_frames `frames_per_call` frames at a time
    (default: `mesh_frames_per_call`), every call writing its frames straight into the result, which does not depend on the chunking.
    face_colours [F,S,3] float32: a colour lattice of the canonical mesh as `mesh_texture.bake_face_colours` makes it, in place of `colours`
    (ValueError for both): every frame is shaded from it (nm_raster_frames_lattice; the header's 'mesh lattice').  face_colours a
    `mesh_texture.LatticePyramid` (`mesh_texture.lattice_pyramid` of such a lattice): the frames are filtered under minification
    (nm_raster_frames_lattice_mip; the header's 'mesh mip'), every face at the level its size in that frame asks for; lod_scale (default
    1.0, finite and >= 0; larger is blurrier, 0 the plain lattice) goes with a pyramid only (ValueError otherwise)."""
    from . import raster
    who = "render_mesh_frames"
    if colours is not None and face_colours is not None:
        raise ValueError(f"{who}: give colours (one per vertex) or face_colours (a lattice per face), not both")
    pyramid, _ = raster.pyramid_of(face_colours, lod_scale, len(faces), who)

    def dense(t, name, dtype, shapes):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.NeumanHipError(f"{who}: {name} must be a CUDA (HIP) tensor: there is no CPU path")
        if t.dtype != dtype or tuple(t.shape) not in shapes or t.device != dev:
            raise _lib.NeumanHipError(f"{who}: {name} must be {dtype} {' or '.join(str(list(s)) for s in shapes)} on {dev}, got {t.dtype} {list(t.shape)} "
                                      f"on {t.device}")
        return t.detach().contiguous()

    if not isinstance(world_verts, torch.Tensor) or not world_verts.is_cuda:
        raise _lib.NeumanHipError(f"{who}: world_verts must be a CUDA (HIP) tensor: there is no CPU path")
    dev = world_verts.device
    if world_verts.dim() != 3 or world_verts.shape[0] < 1 or world_verts.shape[2] != 3 or world_verts.dtype != torch.float32:
        raise _lib.NeumanHipError(f"{who}: world_verts must be float32 [B >= 1, V, 3], got {world_verts.dtype} {list(world_verts.shape)}")
    world_verts = world_verts.detach().contiguous()
    B, V = int(world_verts.shape[0]), int(world_verts.shape[1])
    cameras = caps if isinstance(caps, tuple) else raster.batch_cameras(caps, dev)
    w2c, intr, W, H = cameras
    if tuple(w2c.shape) != (B, 4, 4) or tuple(intr.shape) != (B, 4):
        raise _lib.NeumanHipError(f"{who}: {w2c.shape[0]} cameras for {B} frames")
    colours = dense(colours, "colours", torch.float32, [(V, 3)])
    if pyramid is not None:
        dense(pyramid.data, "face_colours.data", torch.float32, [tuple(pyramid.data.shape)])
    elif face_colours is not None:
        raster.lattice_resolution_of(face_colours, len(faces), who)
        face_colours = dense(face_colours, "face_colours", torch.float32, [tuple(face_colours.shape)])
    normals = dense(normals, "normals", torch.float32, [(B, V, 3)])
    background = dense(background, "background", torch.uint8, [(B, H, W, 3), (H, W, 3)])
    background_depth = dense(background_depth, "background_depth", torch.float32, [(B, H, W)])
    if background_depth is not None and isinstance(caps, tuple):
        raise _lib.NeumanHipError(f"{who}: background_depth needs the captures themselves, not their batch_cameras: the depth maps' rays come from them")
    _lib.require_gpu()
    step = mesh_frames_per_call(V, len(faces), W, H) if frames_per_call is None else int(frames_per_call)
    if step < 1:
        raise _lib.NeumanHipError(f"{who}: frames_per_call = {step}")
    step = min(step, B, 65535)
    rast = raster.rasterizer_for(faces, V)
    light = raster.LIGHT if light is None else light
    with torch.no_grad(), torch.cuda.device(dev):
        out = torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8)
        shared = background.expand(step, H, W, 3).contiguous() if background is not None and background.dim() == 3 else None
        for b0 in range(0, B, step):
            b1 = min(b0 + step, B)
            bg = None if background is None else (shared[:b1 - b0] if shared is not None else background[b0:b1])
            bg_z = None if background_depth is None else torch.stack([depth_to_camera_z(background_depth[b], caps[b]) for b in range(b0, b1)])
            rast.render_frames(world_verts[b0:b1], (w2c[b0:b1], intr[b0:b1], W, H), colours, None if normals is None else normals[b0:b1], light, bg, bg_z,
                               out=out[b0:b1], face_colours=face_colours, lod_scale=lod_scale)
    return out
