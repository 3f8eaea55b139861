"""Occupancy-grid empty-space skipping for the background and human passes (csrc/occupancy.hip).

The reference evaluates every sample of every ray (utils/render_utils.py:131-151, 287-297).  A net with a grid attached
(`attach`) has its background passes -- render_utils.bkg_place_z / bkg_shade, i.e. render_vanilla, render_hybrid_nerf,
render_hybrid_nerf_multi_persons and the sharded frame path -- evaluate only the samples whose cell is occupied (or that lie
outside the grid's box); the others keep raw = 0, which raw2outputs turns into alpha = 0 and weight 0, exactly what a sample
with relu(sigma) = 0 gets.  On every ray whose skipped samples all have relu(sigma) = 0 in the every-sample evaluation the
frame, its depth and the coarse weights (so the importance samples) are therefore bit-identical.  Off by default: with no grid
attached nothing changes.

    grid = OccupancyGrid.from_net(coarse, aabb=((-2, -2, -4), (2, 2, 0)))
    attach(coarse, grid); attach(fine, OccupancyGrid.from_net(fine, aabb=...))

Human nets (K11b).  A grid attached to a human net (HumanNeRF.coarse_human_net, either head) lives in CANONICAL space and serves
every human pass -- render_utils.human_pass_rays (nm_render_rays_human_occ), so render_smpl_nerf (canonical and posed) and the human
legs of render_hybrid_nerf / render_hybrid_nerf_multi_persons (one grid per actor's net), and human_march_rays (early termination).
The canonical render tests the grid on o + d z; the posed pass on the WARPED canonical points (nm_warp_to_canonical, then
nm_occ_compact_points).  The fused hybrid call gives way to the unfused passes while any grid is attached.

    grid = OccupancyGrid.from_net(human.coarse_human_net, canonical_aabb(static_verts, 0.1))
    attach(human.coarse_human_net, grid)

A gridded pass whose raw is composited and nothing else (role='composite': render_utils.LIVE_HEADS and the composite-only rule there) also
leaves the colour head to the evaluated samples that have density: forward_rays / forward_points run nm_mlp_forward_samples_live /
nm_mlp_forward_listed_live, the fused human pass nm_render_rays_human_occ_live; the frame is bit-identical.

Together with early ray termination (render_utils.MARCH_WITH_GRID, NEUMAN_MARCH_WITH_GRID=1; off by default, and then the combination is
refused as before): the marched background passes (render_utils.march_pass_rays with grid=) list, chunk by chunk, the occupied samples of the
LIVE rays only (OccupancyGrid.compact_ray_chunk: nm_occ_compact_ray_chunk -- the same cell test on the same point as `compact`, so every
sample's decision is the same bit) and evaluate that list into the march's raw (forward_listed_samples); a skipped sample keeps raw = 0,
the factor 1 - 0 + 1e-10 of the running transmittance, which the march already handles for relu(sigma) = 0.

Training never consults a grid: the trainers evaluate their nets through the training forward (Joiner.forward in train() mode,
neuman_hip/train.py) on the points of the batch, which knows nothing of grids -- a human-trainer step is the same with or without
one (tests/test_hip_occupancy_human.py).  Rebuild the grid (from_net) after training has moved the density.

Cells: `res`^3 over the box, cell (i, j, k) along (x, y, z); masks are boolean tensors indexed [i, j, k].
"""
import ctypes

import torch

from . import _lib

_ATTR = '_occupancy_grid'


def probe_offsets(probes, seed):
    """[probes, 3] float32: the sub-cell offsets in [0, 1) of the probes, the same in every cell (nm_occ_probe_offset)."""
    L = _lib.lib()
    return torch.tensor([[L.nm_occ_probe_offset(int(probes), int(seed), k, a) for a in range(3)] for k in range(int(probes))], dtype=torch.float32)


def _check_box(aabb):
    box = torch.as_tensor(aabb, dtype=torch.float32).reshape(-1).cpu()
    if box.numel() != 6 or not bool(torch.isfinite(box).all()) or not bool((box[:3] < box[3:]).all()):
        raise ValueError(f"aabb must be (lo xyz, hi xyz) with finite lo < hi on every axis, got {box.tolist()}")
    return box


def _check_res(res):
    res = int(res)
    if not (4 <= res <= 256 and res % 4 == 0):
        raise ValueError(f"res must be a multiple of 4 in 4..256, got {res}")
    return res


def _refuse_time_net(net):
    if getattr(getattr(net, 'pos_pe', None), 'input_dims', 3) != 3:
        raise NotImplementedError("occupancy grids serve static background nets only: the time-conditioned net (raw_pos_dim = 4, "
                                  "--ablate_nerft) has no fixed density field to grid")


def rays_aabb(o, d, near, far, pad=1e-3):
    """The smallest box holding every sample of rays o + d z, z in [near, far] (their end points: the passes' samples lie on the
    segments between them), grown by `pad` of its extent per side -> (lo xyz, hi xyz) float32 on the host."""
    o, d = o.reshape(-1, 3).float(), d.reshape(-1, 3).float()
    near = torch.as_tensor(near, dtype=torch.float32, device=o.device).reshape(-1, 1)
    far = torch.as_tensor(far, dtype=torch.float32, device=o.device).reshape(-1, 1)
    ends = torch.cat([o + d * near, o + d * far], 0)
    lo, hi = ends.min(0).values.cpu(), ends.max(0).values.cpu()
    g = (hi - lo).clamp_min(1e-6) * pad
    return torch.cat([lo - g, hi + g])


def canonical_aabb(static_verts, margin=0.1):
    """The box of a human net's grid: the canonical body's vertices (e.g. the static / da-pose SMPL vertices, [V,3]) grown by `margin`
    scene units per side -> (lo xyz, hi xyz) float32 on the host.  The body's density lives near its surface; what lies outside the
    box is always evaluated (conservatively occupied)."""
    v = torch.as_tensor(static_verts).reshape(-1, 3).to(torch.float32).cpu()
    if v.shape[0] == 0 or not bool(torch.isfinite(v).all()):
        raise ValueError("canonical_aabb: static_verts must be a non-empty finite [V,3] array")
    m = float(margin)
    if not m >= 0.0:
        raise ValueError(f"canonical_aabb: margin must be >= 0, got {margin}")
    return _check_box(torch.cat([v.min(0).values - m, v.max(0).values + m]))


class OccupancyGrid:
    """res^3 occupancy bits over an axis-aligned box: `bits` int32 [res^3 / 32] (bit c = (k res + j) res + i of word c >> 5)."""

    def __init__(self, aabb, res, bits, meta=None):
        self.aabb = _check_box(aabb)
        self.res = _check_res(res)
        bits = torch.as_tensor(bits)
        if bits.dtype != torch.int32 or bits.numel() != self.res ** 3 // 32:
            raise ValueError(f"bits must be int32 [{self.res ** 3 // 32}], got {bits.dtype} [{bits.numel()}]")
        self.bits = bits.reshape(-1).contiguous()
        self.meta = dict(meta or {})

    # ---- construction ---------------------------------------------------------------------
    @classmethod
    def from_net(cls, net, aabb, res=128, probes=8, dilate=1, sigma_threshold=0.0, seed=0, precision=None):
        """Cell occupied <=> some cell within `dilate` of it (per axis) has max sigma > sigma_threshold over its `probes` points
        (probe_offsets), evaluated by the net's density-only launch at the precision of its coarse pass (role None)."""
        _refuse_time_net(net)
        box, res = _check_box(aabb), _check_res(res)
        if not 1 <= int(probes) <= 64:
            raise ValueError(f"probes must be in 1..64, got {probes}")
        if not 0 <= int(dilate) <= 8:
            raise ValueError(f"dilate must be in 0..8, got {dilate}")
        if not float(sigma_threshold) >= 0.0:
            raise ValueError(f"sigma_threshold must be >= 0, got {sigma_threshold}")
        net._guard()
        dev = next(net.parameters()).device
        L = _lib.lib()
        ws = torch.empty(int(L.nm_occ_build_workspace_floats(res, int(probes))), device=dev, dtype=torch.float32)
        bits = torch.empty(res ** 3 // 32, device=dev, dtype=torch.int32)
        box_c = (ctypes.c_float * 6)(*box.tolist())
        with torch.no_grad():
            _lib.check(L.nm_occ_build(net.handle(), box_c, res, int(probes), int(dilate), float(sigma_threshold), int(seed),
                                      net._prec(precision, None), _lib.dev_ptr(ws), ws.numel(), _lib.dev_ptr(bits, torch.int32),
                                      _lib.stream_ptr()), "nm_occ_build")
        return cls(box, res, bits, dict(source='net', probes=int(probes), dilate=int(dilate), sigma_threshold=float(sigma_threshold), seed=int(seed)))

    @classmethod
    def from_mask(cls, aabb, mask, device=None):
        """A user-supplied occupancy (e.g. from the COLMAP points): bool [res, res, res] indexed [i, j, k] along (x, y, z)."""
        mask = torch.as_tensor(mask)
        if mask.dtype != torch.bool or mask.dim() != 3 or len(set(mask.shape)) != 1:
            raise ValueError(f"mask must be a cubic bool tensor [res, res, res], got {mask.dtype} {tuple(mask.shape)}")
        res = _check_res(mask.shape[0])
        flat = mask.permute(2, 1, 0).reshape(-1, 32).to(torch.int64)                 # cell c = (k res + j) res + i
        words = (flat << torch.arange(32, dtype=torch.int64, device=flat.device)).sum(dim=1)
        words = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
        dev = device if device is not None else (mask.device if mask.is_cuda else None)
        return cls(aabb, res, words.to(dev) if dev is not None else words, dict(source='mask'))

    # ---- inspection / persistence -----------------------------------------------------------
    def to_mask(self):
        """bool [res, res, res] indexed [i, j, k]."""
        w = self.bits.to(torch.int64) & 0xffffffff
        b = ((w[:, None] >> torch.arange(32, dtype=torch.int64, device=w.device)) & 1).bool()
        return b.reshape(self.res, self.res, self.res).permute(2, 1, 0).contiguous()

    def occupied_fraction(self):
        w = self.bits.to(torch.int64) & 0xffffffff
        n = int(((w[:, None] >> torch.arange(32, dtype=torch.int64, device=w.device)) & 1).sum())
        return n / self.res ** 3

    def to(self, device):
        return OccupancyGrid(self.aabb, self.res, self.bits.to(device), self.meta)

    def state_dict(self):
        return {'aabb': self.aabb.clone(), 'res': self.res, 'bits': self.bits.cpu().clone(), 'meta': dict(self.meta)}

    @classmethod
    def from_state_dict(cls, sd, device=None):
        bits = sd['bits'] if device is None else sd['bits'].to(device)
        return cls(sd['aabb'], int(sd['res']), bits, sd.get('meta'))

    # ---- the sample list of a pass ----------------------------------------------------------
    def box_c(self):
        return (ctypes.c_float * 6)(*self.aabb.tolist())

    def check_device(self, dev):
        if self.bits.device != dev:
            raise _lib.NeumanHipError(f"the grid lives on {self.bits.device}, the rays on {dev}: attach() the grid to the net on its device")

    def compact_points(self, pts):
        """-> (point_idx int32 [n]: indices of the points pts [n,3] to evaluate, ascending, the first counts[0] live; counts int32 [2] =
        (evaluated, skipped)), both on the device (nm_occ_compact_points)"""
        pts = pts.reshape(-1, 3).contiguous()
        n = pts.shape[0]
        dev = pts.device
        self.check_device(dev)
        idx = torch.empty(n, device=dev, dtype=torch.int32)
        counts = torch.zeros(2, device=dev, dtype=torch.int32)
        L = _lib.lib()
        ws = torch.empty(int(L.nm_occ_compact_workspace_ints(n)), device=dev, dtype=torch.int32)
        _lib.check(L.nm_occ_compact_points(_lib.dev_ptr(self.bits, torch.int32), self.res, self.box_c(), _lib.dev_ptr(pts, name='pts'), n,
                                           _lib.dev_ptr(idx, torch.int32), _lib.dev_ptr(counts, torch.int32), _lib.dev_ptr(ws, torch.int32),
                                           _lib.stream_ptr()), "nm_occ_compact_points")
        return idx, counts

    def compact(self, o, d, z):
        """-> (sample_idx int32 [R*S]: flat indices r*S + s of the samples to evaluate, ascending, the first counts[0] live;
        counts int32 [2] = (evaluated, skipped)), both on the device"""
        R, S = z.shape
        dev = z.device
        if self.bits.device != dev:
            raise _lib.NeumanHipError(f"the grid lives on {self.bits.device}, the rays on {dev}: attach() the grid to the net on its device")
        idx = torch.empty(R * S, device=dev, dtype=torch.int32)
        counts = torch.zeros(2, device=dev, dtype=torch.int32)
        L = _lib.lib()
        ws = torch.empty(int(L.nm_occ_compact_workspace_ints(R * S)), device=dev, dtype=torch.int32)
        _lib.check(L.nm_occ_compact_samples(_lib.dev_ptr(self.bits, torch.int32), self.res, (ctypes.c_float * 6)(*self.aabb.tolist()),
                                            _lib.dev_ptr(o, name='origin'), _lib.dev_ptr(d, name='direction'), _lib.dev_ptr(z, name='z_vals'),
                                            R, S, _lib.dev_ptr(idx, torch.int32), _lib.dev_ptr(counts, torch.int32), _lib.dev_ptr(ws, torch.int32),
                                            _lib.stream_ptr()), "nm_occ_compact_samples")
        return idx, counts


    def compact_ray_chunk(self, o, d, z, ray_idx, n_rays_dev, s0, c, n_rays=None):
        """The occupied samples among samples s0 .. s0+c-1 of the live rays of a march (nm_occ_compact_ray_chunk): ray_idx int32 (only its
        first *n_rays_dev entries are live and read; None: rays 0 .. n-1), n_rays_dev int32 on the device (None: all n_rays), n_rays the
        upper bound (default: len(ray_idx), or R) -> (sample_idx int32 [n_rays*c]: flat indices r*S + s in candidate order, the first
        counts[0] live; counts int32 [2] = (kept, skipped of the live rays' candidates)), both on the device"""
        R, S = z.shape
        dev = z.device
        self.check_device(dev)
        if n_rays is None:
            n_rays = int(ray_idx.shape[0]) if ray_idx is not None else R
        n_rays, c = int(n_rays), int(c)
        idx = torch.empty(n_rays * c, device=dev, dtype=torch.int32)
        counts = torch.zeros(2, device=dev, dtype=torch.int32)
        L = _lib.lib()
        ws = torch.empty(int(L.nm_occ_compact_workspace_ints(n_rays * c)), device=dev, dtype=torch.int32)
        _lib.check(L.nm_occ_compact_ray_chunk(_lib.dev_ptr(self.bits, torch.int32), self.res, self.box_c(), _lib.dev_ptr(o, name='origin'),
                                              _lib.dev_ptr(d, name='direction'), _lib.dev_ptr(z, name='z_vals'), R, S,
                                              _lib.dev_ptr(ray_idx, torch.int32, 'ray_idx'), _lib.dev_ptr(n_rays_dev, torch.int32, 'n_rays_dev'), n_rays,
                                              int(s0), c, _lib.dev_ptr(idx, torch.int32), _lib.dev_ptr(counts, torch.int32), _lib.dev_ptr(ws, torch.int32),
                                              _lib.stream_ptr()), "nm_occ_compact_ray_chunk")
        return idx, counts


def attach(net, grid):
    """Give `net` (a background Joiner, or a human net: a grid in canonical space) an occupancy grid: its render passes skip the grid's
    empty cells from now on.  Coarse and fine nets have different densities: each gets its own grid (the same object may serve a net used
    for both); so does each actor's human net."""
    _refuse_time_net(net)
    if not isinstance(grid, OccupancyGrid):
        raise TypeError(f"attach() takes an OccupancyGrid, got {type(grid).__name__}")
    dev = next(net.parameters()).device
    setattr(net, _ATTR, grid if grid.bits.device == dev else grid.to(dev))
    return net


def detach(net):
    """Remove the net's grid (every sample is evaluated again)."""
    if hasattr(net, _ATTR):
        delattr(net, _ATTR)
    return net


def grid_of(net):
    return getattr(net, _ATTR, None) if net is not None else None


def forward_listed_samples(net, o, d, z, idx, n_dev, n_max, out, precision=None, role=None, sigma_only=False, chunk_samples=0):
    """The first *n_dev (int32 on the device; None: n_max) samples listed in idx (flat indices r*S + s; n_max: the list's upper bound) of
    rays o + d z [R,S] evaluated into the caller's `out` [R,S,4]; nothing else of out is touched.  sigma_only: nm_mlp_sigma_samples;
    role='composite' where Joiner.live_route says so for n_max samples: nm_mlp_forward_samples_live with the open live workspace
    (vanilla.live_workspace), in pieces of `chunk_samples`; nm_mlp_forward_samples otherwise."""
    R, S = z.shape
    L = _lib.lib()
    n_max = int(n_max)
    if net.live_route(precision, role, n_max, sigma_only):
        from .vanilla import live_workspace_for
        ws, nbytes = live_workspace_for(n_max, chunk_samples, z.device)
        _lib.check(L.nm_mlp_forward_samples_live(net.handle(), _lib.dev_ptr(o, name='origin'), _lib.dev_ptr(d, name='direction'), _lib.dev_ptr(z, name='z_vals'),
                                                 R, S, _lib.dev_ptr(idx, torch.int32), _lib.dev_ptr(n_dev, torch.int32), n_max, net._prec(precision, role), 1.0,
                                                 _lib.dev_ptr(out), _lib.dev_ptr(ws, torch.uint8), nbytes, int(chunk_samples), _lib.stream_ptr()),
                   "nm_mlp_forward_samples_live")
    else:
        entry = L.nm_mlp_sigma_samples if sigma_only else L.nm_mlp_forward_samples
        _lib.check(entry(net.handle(), _lib.dev_ptr(o, name='origin'), _lib.dev_ptr(d, name='direction'), _lib.dev_ptr(z, name='z_vals'), R, S,
                         _lib.dev_ptr(idx, torch.int32), _lib.dev_ptr(n_dev, torch.int32), n_max, net._prec(precision, role), 1.0,
                         _lib.dev_ptr(out), _lib.stream_ptr()), "nm_mlp_sigma_samples" if sigma_only else "nm_mlp_forward_samples")
    return out


def forward_rays(net, o, d, z, precision=None, role=None, sigma_only=False, stats=None, chunk_samples=0):
    """net.forward_rays over the grid's occupied samples only: raw [R,S,4], zero on every skipped sample.  `stats` (a dict)
    receives 'evaluated' / 'total' sample counts (one host read).  role='composite': as Joiner.forward_rays -- the colour head runs on the
    evaluated samples with density only (nm_mlp_forward_samples_live, in pieces of `chunk_samples`; Joiner.live_route says when)."""
    grid = grid_of(net)
    net._guard(o, d, z)
    o, d, z = o.contiguous(), d.contiguous(), z.contiguous()
    R, S = z.shape
    raw = torch.zeros((R, S, 4), device=z.device, dtype=torch.float32)
    if R == 0:
        return raw
    idx, counts = grid.compact(o, d, z)
    forward_listed_samples(net, o, d, z, idx, counts, R * S, raw, precision=precision, role=role, sigma_only=sigma_only, chunk_samples=chunk_samples)
    if stats is not None:
        stats['evaluated'] = stats.get('evaluated', 0) + int(counts[0].item())
        stats['total'] = stats.get('total', 0) + R * S
    return raw


def forward_points(net, pts, dirs, precision=None, sigma_scale=1.0, role=None, stats=None, chunk_samples=0):
    """net(pts, dirs) on the points its grid keeps only (nm_occ_compact_points + nm_mlp_forward_listed): [..., 4], zero on every skipped
    point.  `stats` (a dict) receives 'evaluated' / 'total' point counts (one host read).  role='composite': as forward_rays
    (nm_mlp_forward_listed_live)."""
    grid = grid_of(net)
    net._guard(pts, dirs)
    shp = pts.shape[:-1]
    p = pts.reshape(-1, 3).contiguous()
    d = dirs.reshape(-1, 3).contiguous()
    n = p.shape[0]
    out = torch.zeros((n, 4), device=p.device, dtype=torch.float32)
    if n == 0:
        return out.reshape(*shp, 4)
    idx, counts = grid.compact_points(p)
    if net.live_route(precision, role, n):
        from .vanilla import live_workspace_for
        ws, nbytes = live_workspace_for(n, chunk_samples, p.device)
        _lib.check(_lib.lib().nm_mlp_forward_listed_live(net.handle(), _lib.dev_ptr(p, name='pts'), _lib.dev_ptr(d, name='dirs'), n, _lib.dev_ptr(idx, torch.int32),
                                                         _lib.dev_ptr(counts, torch.int32), n, net._prec(precision, role), float(sigma_scale), _lib.dev_ptr(out),
                                                         _lib.dev_ptr(ws, torch.uint8), nbytes, int(chunk_samples), _lib.stream_ptr()),
                   "nm_mlp_forward_listed_live")
    else:
        _lib.check(_lib.lib().nm_mlp_forward_listed(net.handle(), _lib.dev_ptr(p, name='pts'), _lib.dev_ptr(d, name='dirs'), n, _lib.dev_ptr(idx, torch.int32),
                                                    _lib.dev_ptr(counts, torch.int32), n, net._prec(precision, role), float(sigma_scale), _lib.dev_ptr(out),
                                                    _lib.stream_ptr()), "nm_mlp_forward_listed")
    if stats is not None:
        stats['evaluated'] = stats.get('evaluated', 0) + int(counts[0].item())
        stats['total'] = stats.get('total', 0) + n
    return out.reshape(*shp, 4)
