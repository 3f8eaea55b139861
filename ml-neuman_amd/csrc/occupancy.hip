// K11 / K11b: occupancy grid for empty-space skipping in the background and human passes (reference utils/render_utils.py:131-151, 287-297 evaluate
// every sample; a sample skipped here keeps raw = 0, which raw2outputs turns into alpha = 0 and weight 0 -- exactly what a sample with
// relu(sigma) = 0 gets, so on every ray whose skipped samples all have relu(sigma) = 0 the frame is unchanged bit for bit).
//
//   * nm_occ_build: a res^3 bitfield over an axis-aligned box.  A cell's value is the max sigma over `probes` points at the same jittered
//     sub-cell offsets in every cell (offsets: nm_occ_probe_offset), evaluated by the density-only launch (nm_mlp_sigma_rays) with each
//     cell row laid out as one ray along +x per probe; thresholded, dilated by `dilate` cells (a (2 dilate + 1)^3 max) and packed.
//   * nm_occ_compact_samples: the flat indices r * S + s of the samples of R x S rays whose cell is occupied (or that lie outside the
//     box), ascending, and their count -- both on the device: wave ballot + popcount prefix, a two-level scan (nearfar.hip's scheme, K2b).
//   * nm_occ_compact_points (K11b): the same for the points of an [n,3] array -- the warped canonical points of a posed human pass; the
//     same cell test and scan, only the point source differs.
//   * nm_occ_compact_ray_chunk: the same for ONE CHUNK of a front-to-back march (march.hip, render_utils.march_pass_rays): samples
//     s0 .. s0+S-1 of the rays a live list names, the list's length read on the device -- the flat indices r * S_total + s of the occupied ones,
//     in candidate order (ascending when the list is).  The same cell test on the same point, so a sample's decision is the bit
//     nm_occ_compact_samples makes for it: early ray termination and the grid work together (a skipped sample keeps raw = 0, the factor
//     1 - 0 + 1e-10 in the running transmittance, what the march already handles for relu(sigma) = 0).
//   * nm_mlp_forward_samples / nm_mlp_sigma_samples (mlp_host.hip, in_mode 3 of mlp_device.h) evaluate the listed samples only,
//     nm_mlp_forward_listed (in_mode 4) the listed points.
//
// Cell (i, j, k) along (x, y, z) is bit c = (k * res + j) * res + i, word c >> 5, bit c & 31.  Every buffer is the caller's.
#include <cmath>
#include "common.h"

namespace {

constexpr int kOccBlock = 1024;                     // compaction: one sample per thread, 16 waves
constexpr int kOccMaxProbes = 64;
constexpr int64_t kBuildOutFloats = 1ll << 23;      // density records per build launch: [rays, res, 4] floats (32 MB)

struct OccBox {
    float lo[3];
    float inv[3];                                   // res / (hi - lo): cell coordinate of a point
    int res;
};

// lowbias32 (a public-domain 32-bit integer hash): the probe jitter
uint32_t occ_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

int occ_lattice(int probes) {
    int m = 1;
    while (m * m * m < probes) ++m;
    return m;
}

struct ProbeArgs {
    float lo[3], cs[3];
    float off[kOccMaxProbes][3];
    int res, probes;
};

// ray rl of the batch (cell row `row0 + rl / probes`, probe rl % probes): origin (lo.x, y, z) of the row, direction +x, z [rl, i] = the
// x offset of cell i's probe -- so that sample (rl, i) is (lo.x + z, y, z), the probe point itself
__global__ __launch_bounds__(256) void occ_probe_rays_kernel(const ProbeArgs P, int64_t row0, int64_t n_rays, float* __restrict__ origin,
                                                             float* __restrict__ direction, float* __restrict__ z) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;    // element (rl, i) of z
    if (e >= n_rays * P.res) return;
    const int64_t rl = e / P.res;
    const int i = (int)(e - rl * P.res);
    const int p = (int)(rl % P.probes);
    z[e] = ((float)i + P.off[p][0]) * P.cs[0];
    if (i != 0) return;
    const int64_t row = row0 + rl / P.probes;
    const int j = (int)(row % P.res), k = (int)(row / P.res);
    origin[rl * 3 + 0] = P.lo[0];
    origin[rl * 3 + 1] = P.lo[1] + ((float)j + P.off[p][1]) * P.cs[1];
    origin[rl * 3 + 2] = P.lo[2] + ((float)k + P.off[p][2]) * P.cs[2];
    direction[rl * 3 + 0] = 1.f;
    direction[rl * 3 + 1] = 0.f;
    direction[rl * 3 + 2] = 0.f;
}

// max over the probes of each cell of the batch's rows -> maxsig [res^3] (the cells of rows row0 .. row0 + n_rows - 1)
__global__ __launch_bounds__(256) void occ_cell_max_kernel(const float4* __restrict__ raw, int64_t row0, int64_t n_rows, int res, int probes,
                                                           float* __restrict__ maxsig) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;    // cell of the batch: (row - row0) * res + i
    if (c >= n_rows * res) return;
    const int64_t rr = c / res;
    const int i = (int)(c - rr * res);
    float m = -INFINITY;
    for (int p = 0; p < probes; ++p) m = fmaxf(m, raw[(rr * probes + p) * res + i].w);
    maxsig[(row0 + rr) * res + i] = m;
}

// one word (32 cells) per thread: a cell is occupied when some cell within `dilate` of it (per axis, clipped to the grid) has max sigma > thr
__global__ __launch_bounds__(256) void occ_pack_kernel(const float* __restrict__ maxsig, int res, int dilate, float thr, uint32_t* __restrict__ bits) {
    const int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t ncell = (int64_t)res * res * res;
    if (w * 32 >= ncell) return;
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
        const int64_t c = w * 32 + b;
        const int i = (int)(c % res), j = (int)((c / res) % res), k = (int)(c / ((int64_t)res * res));
        bool occ = false;
        for (int dk = -dilate; dk <= dilate && !occ; ++dk) {
            const int kk = k + dk;
            if (kk < 0 || kk >= res) continue;
            for (int dj = -dilate; dj <= dilate && !occ; ++dj) {
                const int jj = j + dj;
                if (jj < 0 || jj >= res) continue;
                const float* rowp = maxsig + ((int64_t)kk * res + jj) * res;
                for (int di = -dilate; di <= dilate; ++di) {
                    const int ii = i + di;
                    if (ii >= 0 && ii < res && rowp[ii] > thr) {
                        occ = true;
                        break;
                    }
                }
            }
        }
        word |= (uint32_t)occ << b;
    }
    bits[w] = word;
}

// the cell test: occupied, or outside the box (or NaN) -- conservatively occupied
__device__ __forceinline__ bool point_occupied(const OccBox& B, const uint32_t* __restrict__ bits, const float (&p)[3]) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float t = (p[a] - B.lo[a]) * B.inv[a];
        if (!(t >= 0.f && t < (float)B.res)) return true;
        c[a] = min((int)t, B.res - 1);
    }
    const int64_t cell = ((int64_t)c[2] * B.res + c[1]) * B.res + c[0];
    return (bits[cell >> 5] >> (cell & 31)) & 1u;
}

// the points the compaction lists: sample i = r * S + s of rays + z, built exactly as mlp_device.h sample_input builds it (o + d * z,
// two roundings: -ffp-contract=off) ...
struct SamplePoints {
    const float* origin;
    const float* direction;
    const float* z;
    int S;
    __device__ __forceinline__ int64_t limit(int64_t n) const { return n; }
    __device__ __forceinline__ int32_t index(int64_t i) const { return (int32_t)i; }
    __device__ __forceinline__ void point(int64_t i, float (&p)[3]) const {
        const int64_t r = i / S;
        const float zz = z[i];
        const float* o = origin + r * 3;
        const float* d = direction + r * 3;
        p[0] = o[0] + d[0] * zz;
        p[1] = o[1] + d[1] * zz;
        p[2] = o[2] + d[2] * zz;
    }
};
// ... or point i of an [n,3] array (the warped canonical points of a posed human pass)
struct GivenPoints {
    const float* pts;
    __device__ __forceinline__ int64_t limit(int64_t n) const { return n; }
    __device__ __forceinline__ int32_t index(int64_t i) const { return (int32_t)i; }
    __device__ __forceinline__ void point(int64_t i, float (&p)[3]) const {
        p[0] = pts[i * 3];
        p[1] = pts[i * 3 + 1];
        p[2] = pts[i * 3 + 2];
    }
};

// ... or candidate j of a march's chunk: sample s0 + j % S of the (j / S)-th ray of a live list whose length *n_rays_dev stays on the
// device (nullable: n_rays; ray_idx nullable: rays 0 .. n-1).  Only the first n entries of ray_idx are read: the march's lists are
// uninitialised beyond their count.  Consecutive candidates are consecutive samples of a ray: z is read coalesced along s.  Every count
// fits an int (the entry checks n_rays * S and R * S_total < 2^31).
__device__ __forceinline__ int live_rays(const int32_t* __restrict__ n_rays_dev, int n_rays) {
    return n_rays_dev ? min(max(*n_rays_dev, 0), n_rays) : n_rays;
}
struct ChunkPoints {
    const float* origin;
    const float* direction;
    const float* z;
    const int32_t* ray_idx;
    const int32_t* n_rays_dev;
    int n_rays, S_total, s0, S;
    __device__ __forceinline__ int64_t limit(int64_t) const { return (int64_t)live_rays(n_rays_dev, n_rays) * S; }
    __device__ __forceinline__ int32_t index(int64_t j) const {
        const int k = (int)j / S;
        const int r = ray_idx ? ray_idx[k] : k;
        return r * S_total + s0 + ((int)j - k * S);
    }
    __device__ __forceinline__ void point(int64_t j, float (&p)[3]) const {
        const int i = index(j);
        const int r = i / S_total;
        const float zz = z[i];
        const float* o = origin + (int64_t)r * 3;
        const float* d = direction + (int64_t)r * 3;
        p[0] = o[0] + d[0] * zz;
        p[1] = o[1] + d[1] * zz;
        p[2] = o[2] + d[2] * zz;
    }
};

template <class Src>
__device__ __forceinline__ bool listed(const OccBox& B, const uint32_t* __restrict__ bits, const Src& src, int64_t i, int64_t n) {
    if (i >= src.limit(n)) return false;
    float p[3];
    src.point(i, p);
    return point_occupied(B, bits, p);
}

// pass 1: occupied points per block
template <class Src>
__global__ __launch_bounds__(kOccBlock) void occ_count_kernel(const OccBox B, const uint32_t* __restrict__ bits, const Src src, int64_t n,
                                                              int32_t* __restrict__ block_counts) {
    __shared__ int wave_cnt[kOccBlock / 64];
    const int64_t i = blockIdx.x * (int64_t)kOccBlock + threadIdx.x;
    const bool occ = listed(B, bits, src, i, n);
    const unsigned long long b = __ballot(occ);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < kOccBlock / 64; ++w) c += wave_cnt[w];
        block_counts[blockIdx.x] = c;
    }
}

// pass 2: exclusive scan of the block counts (one block); counts[0] = occupied, counts[1] = skipped of n points -- or, for a march's
// chunk (per_ray > 0), of live_rays(n_rays_dev, n_rays) * per_ray candidates
__global__ __launch_bounds__(1024) void occ_scan_kernel(int32_t* __restrict__ block_counts, int nblocks, int64_t n, const int32_t* __restrict__ n_rays_dev,
                                                        int n_rays, int per_ray, int32_t* __restrict__ counts) {
    __shared__ int wave_tot[16];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nblocks ? block_counts[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wave_tot[wid] = inc;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wid; ++w) woff += wave_tot[w];
        const int carry = carry_s;
        if (i < nblocks) block_counts[i] = carry + woff + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + woff + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (per_ray > 0) n = (int64_t)live_rays(n_rays_dev, n_rays) * per_ray;
        counts[0] = carry_s;
        counts[1] = (int32_t)(n - carry_s);
    }
}

// pass 3: the occupied points' indices, ascending
template <class Src>
__global__ __launch_bounds__(kOccBlock) void occ_write_kernel(const OccBox B, const uint32_t* __restrict__ bits, const Src src, int64_t n,
                                                              const int32_t* __restrict__ block_offsets, int32_t* __restrict__ idx) {
    __shared__ int wave_cnt[kOccBlock / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t i = blockIdx.x * (int64_t)kOccBlock + threadIdx.x;
    const bool occ = listed(B, bits, src, i, n);
    const unsigned long long b = __ballot(occ);
    if (lane == 0) wave_cnt[wid] = __popcll(b);
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wid; ++w) woff += wave_cnt[w];
    if (occ) idx[block_offsets[blockIdx.x] + woff + __popcll(b & ((1ull << lane) - 1ull))] = src.index(i);
}

bool box_ok(const float* aabb) {
    for (int a = 0; a < 3; ++a)
        if (!(aabb[a] < aabb[3 + a]) || !std::isfinite(aabb[a]) || !std::isfinite(aabb[3 + a])) return false;
    return true;
}

// the three passes: count per block, scan (counts = (kept, skipped)), write -- the count stays on the device
template <class Src>
int occ_compact(const char* what, const uint32_t* bits, int res, const float* aabb, const Src& src, int64_t n, int32_t* idx, int32_t* counts,
                int32_t* workspace, hipStream_t st, const int32_t* n_rays_dev = nullptr, int n_rays = 0, int per_ray = 0) {
    OccBox B;
    for (int a = 0; a < 3; ++a) {
        B.lo[a] = aabb[a];
        B.inv[a] = (float)res / (aabb[3 + a] - aabb[a]);
    }
    B.res = res;
    const int nblocks = (int)((n + kOccBlock - 1) / kOccBlock);
    if (nblocks > 0) {
        hipLaunchKernelGGL(occ_count_kernel<Src>, dim3(nblocks), dim3(kOccBlock), 0, st, B, bits, src, n, workspace);
        if (int e = nm::check_launch("occ_count_kernel")) return e;
    }
    hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(1024), 0, st, workspace, nblocks, n, n_rays_dev, n_rays, per_ray, counts);
    if (int e = nm::check_launch("occ_scan_kernel")) return e;
    if (nblocks > 0) {
        hipLaunchKernelGGL(occ_write_kernel<Src>, dim3(nblocks), dim3(kOccBlock), 0, st, B, bits, src, n, workspace, idx);
        if (int e = nm::check_launch("occ_write_kernel")) return e;
    }
    (void)what;
    return NM_OK;
}

}  // namespace

extern "C" {

float nm_occ_probe_offset(int probes, int seed, int k, int axis) {
    if (probes < 1 || probes > kOccMaxProbes || k < 0 || k >= probes || axis < 0 || axis > 2) return -1.f;
    const int m = occ_lattice(probes);
    const int sub = axis == 0 ? k % m : (axis == 1 ? (k / m) % m : k / (m * m));
    const uint32_t h = occ_hash((uint32_t)seed * 0x9e3779b9u + (uint32_t)(3 * k + axis));
    const float jit = (float)(h >> 8) * 0x1p-24f;                   // [0, 1), exact
    return ((float)sub + jit) / (float)m;                           // < 1
}

int64_t nm_occ_build_workspace_floats(int res, int probes) {
    if (res < 4 || res > 256 || probes < 1 || probes > kOccMaxProbes) return -1;
    const int64_t per_row = (int64_t)probes * (6 + 5 * (int64_t)res);           // origin, direction, z [res], raw [res][4]
    int64_t rows = kBuildOutFloats / ((int64_t)probes * res * 4);
    if (rows < 1) rows = 1;
    if (rows > (int64_t)res * res) rows = (int64_t)res * res;
    return (int64_t)res * res * res + rows * per_row + 4;
}

int nm_occ_build(nm_mlp_t mlp, const float* aabb, int res, int probes, int dilate, float sigma_threshold, int seed, int precision,
                 float* workspace, int64_t workspace_floats, uint32_t* bits, nm_stream_t stream) {
    NM_REQUIRE(mlp && aabb && workspace && bits, "nm_occ_build: null pointer");
    NM_REQUIRE(res >= 4 && res <= 256 && res % 4 == 0, "nm_occ_build: res %d outside 4..256 or not a multiple of 4", res);
    NM_REQUIRE(probes >= 1 && probes <= kOccMaxProbes, "nm_occ_build: probes %d outside 1..%d", probes, kOccMaxProbes);
    NM_REQUIRE(dilate >= 0 && dilate <= 8, "nm_occ_build: dilate %d outside 0..8", dilate);
    NM_REQUIRE(sigma_threshold >= 0.f && std::isfinite(sigma_threshold), "nm_occ_build: sigma_threshold must be finite and >= 0");
    NM_REQUIRE(box_ok(aabb), "nm_occ_build: the box must have finite lo < hi on every axis");
    const int64_t need = nm_occ_build_workspace_floats(res, probes);
    NM_REQUIRE(workspace_floats >= need, "nm_occ_build: workspace of %lld floats, %lld needed", (long long)workspace_floats, (long long)need);
    NM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "nm_occ_build: workspace must be 16-byte aligned");
    hipStream_t st = nm::as_stream(stream);
    ProbeArgs P;
    for (int a = 0; a < 3; ++a) {
        P.lo[a] = aabb[a];
        P.cs[a] = (aabb[3 + a] - aabb[a]) / (float)res;
    }
    for (int k = 0; k < probes; ++k)
        for (int a = 0; a < 3; ++a) P.off[k][a] = nm_occ_probe_offset(probes, seed, k, a);
    P.res = res;
    P.probes = probes;
    // the plain-head net (use_viewdirs=False: a human net without specular_can) has no density-only form at NM_PREC_I8X3: its whole-network
    // launch gives the same sigma
    const bool whole = precision == NM_PREC_I8X3 && nm::mlp_plain_head(mlp);
    const int64_t n_rows = (int64_t)res * res;
    int64_t batch = kBuildOutFloats / ((int64_t)probes * res * 4);
    if (batch < 1) batch = 1;
    if (batch > n_rows) batch = n_rows;
    float* maxsig = workspace;
    float* raw = maxsig + (int64_t)res * res * res;                       // 16-byte aligned: res^3 is a multiple of 64
    float* z = raw + batch * probes * res * 4;
    float* origin = z + batch * probes * res;
    float* direction = origin + batch * probes * 3;
    for (int64_t row0 = 0; row0 < n_rows; row0 += batch) {
        const int64_t nr = row0 + batch <= n_rows ? batch : n_rows - row0;
        const int64_t rays = nr * probes;
        hipLaunchKernelGGL(occ_probe_rays_kernel, dim3((unsigned)((rays * res + 255) / 256)), dim3(256), 0, st, P, row0, rays, origin, direction, z);
        if (int e = nm::check_launch("occ_probe_rays_kernel")) return e;
        if (int e = whole ? nm_mlp_forward_rays(mlp, origin, direction, z, rays, res, precision, 1.f, raw, stream)
                          : nm_mlp_sigma_rays(mlp, origin, direction, z, rays, res, precision, 1.f, raw, stream)) return e;
        hipLaunchKernelGGL(occ_cell_max_kernel, dim3((unsigned)((nr * res + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4*>(raw), row0,
                           nr, res, probes, maxsig);
        if (int e = nm::check_launch("occ_cell_max_kernel")) return e;
    }
    const int64_t words = (int64_t)res * res * res / 32;
    hipLaunchKernelGGL(occ_pack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, maxsig, res, dilate, sigma_threshold, bits);
    return nm::check_launch("occ_pack_kernel");
}

int64_t nm_occ_compact_workspace_ints(int64_t n_samples) { return (n_samples + kOccBlock - 1) / kOccBlock + 2; }

int nm_occ_compact_samples(const uint32_t* bits, int res, const float* aabb, const float* origin, const float* direction, const float* z_vals,
                           int64_t R, int S, int32_t* sample_idx, int32_t* counts, int32_t* workspace, nm_stream_t stream) {
    NM_REQUIRE(bits && aabb && counts && workspace, "nm_occ_compact_samples: null pointer");
    NM_REQUIRE(R == 0 || (origin && direction && z_vals && sample_idx), "nm_occ_compact_samples: null pointer");
    NM_REQUIRE(res >= 4 && res <= 256 && res % 4 == 0, "nm_occ_compact_samples: res %d outside 4..256 or not a multiple of 4", res);
    NM_REQUIRE(R >= 0 && S >= 1 && R * (int64_t)S < (1ll << 31), "nm_occ_compact_samples: bad sizes (R=%lld S=%d)", (long long)R, S);
    NM_REQUIRE(box_ok(aabb), "nm_occ_compact_samples: the box must have finite lo < hi on every axis");
    return occ_compact("nm_occ_compact_samples", bits, res, aabb, SamplePoints{origin, direction, z_vals, S}, R * (int64_t)S, sample_idx, counts, workspace,
                       nm::as_stream(stream));
}

int nm_occ_compact_points(const uint32_t* bits, int res, const float* aabb, const float* pts, int64_t n, int32_t* point_idx, int32_t* counts,
                          int32_t* workspace, nm_stream_t stream) {
    NM_REQUIRE(bits && aabb && counts && workspace, "nm_occ_compact_points: null pointer");
    NM_REQUIRE(n == 0 || (pts && point_idx), "nm_occ_compact_points: null pointer");
    NM_REQUIRE(res >= 4 && res <= 256 && res % 4 == 0, "nm_occ_compact_points: res %d outside 4..256 or not a multiple of 4", res);
    NM_REQUIRE(n >= 0 && n < (1ll << 31), "nm_occ_compact_points: bad size (n=%lld)", (long long)n);
    NM_REQUIRE(box_ok(aabb), "nm_occ_compact_points: the box must have finite lo < hi on every axis");
    return occ_compact("nm_occ_compact_points", bits, res, aabb, GivenPoints{pts}, n, point_idx, counts, workspace, nm::as_stream(stream));
}

int nm_occ_compact_ray_chunk(const uint32_t* bits, int res, const float* aabb, const float* origin, const float* direction, const float* z_vals,
                             int64_t R, int S_total, const int32_t* ray_idx, const int32_t* n_rays_dev, int64_t n_rays, int s0, int S,
                             int32_t* sample_idx, int32_t* counts, int32_t* workspace, nm_stream_t stream) {
    NM_REQUIRE(bits && aabb && counts && workspace, "nm_occ_compact_ray_chunk: null pointer");
    NM_REQUIRE(n_rays == 0 || (origin && direction && z_vals && sample_idx), "nm_occ_compact_ray_chunk: null pointer");
    NM_REQUIRE(res >= 4 && res <= 256 && res % 4 == 0, "nm_occ_compact_ray_chunk: res %d outside 4..256 or not a multiple of 4", res);
    NM_REQUIRE(box_ok(aabb), "nm_occ_compact_ray_chunk: the box must have finite lo < hi on every axis");
    NM_REQUIRE(S >= 1 && s0 >= 0 && (int64_t)s0 + S <= S_total, "nm_occ_compact_ray_chunk: bad chunk (s0=%d S=%d S_total=%d)", s0, S, S_total);
    NM_REQUIRE(R >= 0 && n_rays >= 0 && R * (int64_t)S_total < (1ll << 31) && n_rays * (int64_t)S < (1ll << 31),
               "nm_occ_compact_ray_chunk: bad sizes (R=%lld S_total=%d n_rays=%lld S=%d)", (long long)R, S_total, (long long)n_rays, S);
    NM_REQUIRE(ray_idx || n_rays <= R, "nm_occ_compact_ray_chunk: %lld rays listed without ray_idx, %lld given", (long long)n_rays, (long long)R);
    return occ_compact("nm_occ_compact_ray_chunk", bits, res, aabb,
                       ChunkPoints{origin, direction, z_vals, ray_idx, n_rays_dev, (int)n_rays, S_total, s0, S}, n_rays * (int64_t)S, sample_idx, counts,
                       workspace, nm::as_stream(stream), n_rays_dev, (int)n_rays, S);
}

}  // extern "C"
