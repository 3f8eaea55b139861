// Front-to-back marching of the shading pass: early ray termination + compaction of the live rays (BASELINE north star;
// the reference evaluates every sample of every ray, utils/render_utils.py:139-151).
//
// A pass of S_total sorted samples per ray is evaluated in chunks of S samples, nearest first.  After a chunk, each live
// ray's transmittance T = prod (1 - alpha_i + 1e-10) over everything evaluated so far (the factors of raw2outputs,
// render_utils.py:86-95) is updated by nm_transmittance_chunk; rays with T < eps are dropped from the list (ballot /
// prefix-sum compaction, nm_compact_hits with the predicate eps < T) and the next chunk's MLP launch
// (nm_mlp_forward_ray_chunk, csrc/mlp.hip in_mode 2) runs over the compacted (live rays x chunk samples) batch only.
// The records of samples that are never evaluated stay zero (sigma = 0: weight exactly 0 in nm_composite), so the
// composited colour differs from the full evaluation's by at most the weight that was cut off, sum_{dropped} w_i <= T < eps,
// per channel.  Nothing returns to the host between chunks: the list length lives on the device.
//
// nm_march_pass is the whole pass as ONE call: uniform chunks, and the step between two of them -- transmittance, the occluder's factor,
// the cut, the compacted list, the evaluation counter -- as three launches over the live rays only.  nm_render_rays_bkg_march is
// nm_render_rays_bkg with its passes marched.  Like every fused pass: no host synchronisation, no allocation, no copy to the host.
#include "common.h"

namespace {

// The factor of one chunk: prod over samples s0 .. s0+S-1 of ray r of raw2outputs' (1 - alpha_i + 1e-10), lanes over the chunk's samples, on every
// lane after the reduction.  GIVEN_DZ: `z` holds the samples' INTERVALS instead of their positions (a list that will be merged with others
// before it is composited: the interval behind a sample ends at its successor in the MERGED order, render_utils.py:330-345).  The ONE body of
// nm_transmittance_chunk* and of the fused march's boundary: the cuts are decided on T's bits.
template <bool GIVEN_DZ>
__device__ __forceinline__ float chunk_transmittance(const float* __restrict__ raw, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                     int64_t r, int s0, int S, int S_total, int lane) {
    const float* d = rays_d + r * 3;
    const float dn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);                       // render_utils.py:88
    const float* zr = z + r * S_total;
    const float4* rw = reinterpret_cast<const float4*>(raw) + r * S_total;
    float prod = 1.f;
    for (int t = lane; t < S; t += 64) {
        const int i = s0 + t;
        const float dist = (GIVEN_DZ ? zr[i] : (i + 1 < S_total ? zr[i + 1] - zr[i] : 1e10f)) * dn;   // render_utils.py:85-88
        const float alpha = 1.f - expf(-fmaxf(rw[i].w, 0.f) * dist);                       // :94
        prod *= 1.f - alpha + 1e-10f;                                                      // :95
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) prod *= __shfl_xor(prod, o, 64);
    return prod;
}

// one wave per live ray
template <bool GIVEN_DZ>
__global__ __launch_bounds__(256) void transmittance_chunk_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                  const float* __restrict__ rays_d, const int* __restrict__ ray_idx,
                                                                  const int* __restrict__ n_rays_dev, int n_rays, int s0, int S, int S_total,
                                                                  float* __restrict__ T) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6);
    const int nwaves = (int)((gridDim.x * (int64_t)blockDim.x) >> 6);
    const int n = n_rays_dev ? *n_rays_dev : n_rays;
    for (int j = wave; j < n; j += nwaves) {
        const int64_t r = ray_idx ? ray_idx[j] : j;
        const float prod = chunk_transmittance<GIVEN_DZ>(raw, z, rays_d, r, s0, S, S_total, lane);
        if (lane == 0) T[r] *= prod;
    }
}

// ---- the step between two chunks of a march, on the device (nm_march_pass) ------------------------------------------------------------------
// What march_pass_rays does on the host after a chunk -- nm_transmittance_chunk, T_eff = T x (the occluder's transmittance once the next
// sample is behind it), nm_compact_hits(eps, T_eff) over all R rays -- on the rays of the live list only, in three launches ordered by the
// stream and by nothing else: (1) transmittance + count, (2) single-block scan, (3) write.  Launches 1 and 3 run the SAME grid and cut the list
// positions 0 .. n-1 (n on the device) into the same contiguous, ascending segment per block, so the compacted list is ascending when the
// input list is.  Launch 3 decides on the T that launch 1 stored: the same float, the same decision.
constexpr int kBoundaryBlock = 256;
constexpr int kBoundaryMaxBlocks = 8192;                 // (the cap of nm_transmittance_chunk's grid: longer lists take more positions per block)

__device__ __forceinline__ int live_count(const int* __restrict__ n_dev, int n_max) {
    const int n = *n_dev;
    return n < 0 ? 0 : (n > n_max ? n_max : n);
}

// positions [begin, end) of block blockIdx.x: a multiple of 4 per block (one ray per wave and step in launch 1)
__device__ __forceinline__ void boundary_segment(int n, int& begin, int& end) {
    const int64_t per = (((int64_t)n + gridDim.x - 1) / gridDim.x + 3) & ~int64_t(3);
    const int64_t b = (int64_t)blockIdx.x * per;
    begin = (int)(b < n ? b : n);
    end = (int)(b + per < n ? b + per : n);
}

// eps < T_eff: nm_compact_hits' predicate on the value march_pass_rays forms with torch.where and ONE float32 multiply (a NaN drops the ray)
__device__ __forceinline__ bool march_keeps(float T, int64_t r, const float* __restrict__ z_vals, int S_total, int s_next,
                                            const float* __restrict__ occ_z_far, const float* __restrict__ occ_T, float eps) {
    const float behind = (occ_z_far && z_vals[r * S_total + s_next] >= occ_z_far[r]) ? occ_T[r] : 1.f;
    return eps < T * behind;
}

__global__ __launch_bounds__(256) void march_init_kernel(int n, float* __restrict__ T, int* __restrict__ live, int* __restrict__ counts,
                                                         long long* __restrict__ stats, long long first) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        T[i] = 1.f;
        live[i] = (int)i;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = n; counts[1] = 0;                    // (this list, dropped so far)
        counts[2] = 0; counts[3] = 0;
        if (stats) { stats[0] = first; stats[1] = 0; }
    }
}

// launch 1: one wave per live ray and step; T[r] *= the chunk's factor, then the ray's decision is counted
template <bool GIVEN_DZ>
__global__ __launch_bounds__(kBoundaryBlock) void march_boundary_count_kernel(const float* __restrict__ raw, const float* __restrict__ zi,
                                                                              const float* __restrict__ z_vals, const float* __restrict__ rays_d,
                                                                              const int* __restrict__ live, const int* __restrict__ n_dev, int n_max,
                                                                              int s0, int S, int S_total, int s_next, float eps,
                                                                              const float* __restrict__ occ_z_far, const float* __restrict__ occ_T,
                                                                              float* T, int* __restrict__ block_counts) {
    __shared__ int wave_cnt[kBoundaryBlock / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int begin, end;
    boundary_segment(live_count(n_dev, n_max), begin, end);
    int kept = 0;
    for (int j = begin + wid; j < end; j += kBoundaryBlock / 64) {
        const int64_t r = live[j];
        const float prod = chunk_transmittance<GIVEN_DZ>(raw, zi, rays_d, r, s0, S, S_total, lane);
        const float t = T[r] * prod;
        if (lane == 0) T[r] = t;
        kept += march_keeps(t, r, z_vals, S_total, s_next, occ_z_far, occ_T, eps) ? 1 : 0;
    }
    if (lane == 0) wave_cnt[wid] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < kBoundaryBlock / 64; ++w) c += wave_cnt[w];
        block_counts[blockIdx.x] = c;
    }
}

// launch 2: exclusive scan of the block counts (single block); the next list's length, and its evaluations into the running counter
__global__ __launch_bounds__(1024) void march_boundary_scan_kernel(int* __restrict__ block_counts, int nblocks, const int* __restrict__ n_dev,
                                                                   int n_max, int* __restrict__ counts_next, long long* __restrict__ stats,
                                                                   int c_next) {
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
        if (i < nblocks) block_counts[i] = carry + woff + inc - v;         // exclusive
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + woff + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int kept = carry_s;
        counts_next[0] = kept;
        counts_next[1] = live_count(n_dev, n_max) - kept;
        if (stats) stats[0] += (long long)kept * c_next;
    }
}

// launch 3: the kept rays of the block's segment, in order, behind the kept rays of the blocks before it
__global__ __launch_bounds__(kBoundaryBlock) void march_boundary_write_kernel(const float* __restrict__ T, const float* __restrict__ z_vals,
                                                                              const int* __restrict__ live, const int* __restrict__ n_dev, int n_max,
                                                                              int S_total, int s_next, float eps, const float* __restrict__ occ_z_far,
                                                                              const float* __restrict__ occ_T, const int* __restrict__ block_offsets,
                                                                              int* __restrict__ next) {
    __shared__ int wave_cnt[kBoundaryBlock / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int begin, end;
    boundary_segment(live_count(n_dev, n_max), begin, end);
    int off = block_offsets[blockIdx.x];
    for (int base = begin; base < end; base += kBoundaryBlock) {           // (uniform over the block: the barriers below are reached by all)
        const int j = base + (int)threadIdx.x;
        const bool in = j < end;
        const int r = in ? live[j] : 0;
        const bool keep = in && march_keeps(T[r], r, z_vals, S_total, s_next, occ_z_far, occ_T, eps);
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wave_cnt[wid] = __popcll(b);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < kBoundaryBlock / 64; ++w) {
            if (w < wid) woff += wave_cnt[w];
            tot += wave_cnt[w];
        }
        if (keep) next[off + woff + __popcll(b & ((1ull << lane) - 1ull))] = r;
        off += tot;
        __syncthreads();
    }
}

inline int64_t align4(int64_t n) { return (n + 3) & ~int64_t(3); }        // keep every sub-array 16-byte aligned

// T [R] | live list [R] x 2 (this chunk's, the next one's) | block counts | the lists' lengths int32[2] x 2
int64_t march_ws_floats(int64_t R) { return 3 * align4(R) + kBoundaryMaxBlocks + 4; }

bool chunked_precision(int p) { return p == NM_PREC_BF16X3 || p == NM_PREC_BF16 || p == NM_PREC_I8X3 || p == NM_PREC_FP16X3; }

// what both entries check of one marched pass before anything is enqueued
#define NM_MARCH_REQUIRE(who, mlp, precision, sigma_only)                                                                                        \
    NM_REQUIRE((precision) != NM_PREC_FP32, "%s: NM_PREC_FP32, the exact-f32 validation kernel, has no chunked form", who);                      \
    NM_REQUIRE(chunked_precision(precision), "%s: bad precision %d", who, (int)(precision));                                                     \
    NM_REQUIRE(!((sigma_only) && (precision) == NM_PREC_I8X3 && nm::mlp_plain_head(mlp)),                                                        \
               "%s: the plain-head (use_viewdirs=False) net has no density-only i8x3 form", who)

// One marched pass, every argument checked by the caller: uniform chunks front to back, the boundary between two of them on the device.
int march_pass(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int64_t R, int S_total, int chunk, float eps,
               int sigma_only, int precision, float sigma_scale, const float* dz, const float* occ_z_far, const float* occ_T, float* workspace,
               float* raw_out, int64_t* stats, nm_stream_t stream) {
    hipStream_t st = nm::as_stream(stream);
    float* T = workspace;
    int32_t* live[2] = {reinterpret_cast<int32_t*>(workspace + align4(R)), reinterpret_cast<int32_t*>(workspace + 2 * align4(R))};
    int32_t* blocks = reinterpret_cast<int32_t*>(workspace + 3 * align4(R));
    int32_t* counts = blocks + kBoundaryMaxBlocks;                         // [2][2]
    int rc;
    if ((rc = nm::check_hip(hipMemsetAsync(raw_out, 0, (size_t)R * S_total * 4 * sizeof(float), st), "nm_march_pass: zeroing raw_out"))) return rc;
    const bool cuts = eps > 0.f;                                           // (eps <= 0: nothing is ever dropped, not even rays whose T underflowed to 0)
    const int c0 = chunk < S_total ? chunk : S_total;
    const int64_t init_blocks = (R + 255) / 256;
    hipLaunchKernelGGL(march_init_kernel, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(256), 0, st, (int)R, T, live[0], counts,
                       reinterpret_cast<long long*>(stats), (long long)R * (cuts ? c0 : S_total));
    if ((rc = nm::check_launch("march_init_kernel"))) return rc;
    int64_t grid = (R + 3) / 4;
    if (grid > kBoundaryMaxBlocks) grid = kBoundaryMaxBlocks;
    int cur = 0;
    for (int s0 = 0; s0 < S_total;) {
        const int c = chunk < S_total - s0 ? chunk : S_total - s0;
        rc = sigma_only ? nm_mlp_sigma_ray_chunk(mlp, origin, direction, z_vals, S_total, live[cur], counts + 2 * cur, R, s0, c, precision, sigma_scale,
                                                 raw_out, stream)
                        : nm_mlp_forward_ray_chunk(mlp, origin, direction, z_vals, S_total, live[cur], counts + 2 * cur, R, s0, c, precision, sigma_scale,
                                                   raw_out, stream);
        if (rc) return rc;
        const int s_next = s0 + c;
        if (s_next < S_total && cuts) {
            const int c_next = chunk < S_total - s_next ? chunk : S_total - s_next;
            if (dz)
                hipLaunchKernelGGL(march_boundary_count_kernel<true>, dim3((unsigned)grid), dim3(kBoundaryBlock), 0, st, raw_out, dz, z_vals, direction,
                                   live[cur], counts + 2 * cur, (int)R, s0, c, S_total, s_next, eps, occ_z_far, occ_T, T, blocks);
            else
                hipLaunchKernelGGL(march_boundary_count_kernel<false>, dim3((unsigned)grid), dim3(kBoundaryBlock), 0, st, raw_out, z_vals, z_vals, direction,
                                   live[cur], counts + 2 * cur, (int)R, s0, c, S_total, s_next, eps, occ_z_far, occ_T, T, blocks);
            if ((rc = nm::check_launch("march_boundary_count_kernel"))) return rc;
            hipLaunchKernelGGL(march_boundary_scan_kernel, dim3(1), dim3(1024), 0, st, blocks, (int)grid, counts + 2 * cur, (int)R, counts + 2 * (1 - cur),
                               reinterpret_cast<long long*>(stats), c_next);
            if ((rc = nm::check_launch("march_boundary_scan_kernel"))) return rc;
            hipLaunchKernelGGL(march_boundary_write_kernel, dim3((unsigned)grid), dim3(kBoundaryBlock), 0, st, T, z_vals, live[cur], counts + 2 * cur, (int)R,
                               S_total, s_next, eps, occ_z_far, occ_T, blocks, live[1 - cur]);
            if ((rc = nm::check_launch("march_boundary_write_kernel"))) return rc;
            cur = 1 - cur;
        }
        s0 = s_next;
    }
    return NM_OK;
}

}  // namespace

extern "C" {

int nm_transmittance_chunk(const float* raw, const float* z_vals, const float* rays_d, const int32_t* ray_idx, const int32_t* n_rays_dev,
                           int64_t n_rays, int s0, int S, int S_total, float* T, nm_stream_t stream) {
    NM_REQUIRE(n_rays == 0 || (raw && z_vals && rays_d && T), "nm_transmittance_chunk: null pointer");
    NM_REQUIRE(n_rays >= 0 && n_rays < (1ll << 31) && S >= 1 && s0 >= 0 && s0 + S <= S_total, "nm_transmittance_chunk: bad sizes (s0=%d S=%d S_total=%d)",
               s0, S, S_total);
    NM_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 15) == 0, "nm_transmittance_chunk: raw must be 16-byte aligned");
    if (n_rays == 0) return NM_OK;
    int64_t blocks = (n_rays + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(transmittance_chunk_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, nm::as_stream(stream), raw, z_vals, rays_d, ray_idx,
                       n_rays_dev, (int)n_rays, s0, S, S_total, T);
    return nm::check_launch("transmittance_chunk_kernel");
}

int nm_transmittance_chunk_dz(const float* raw, const float* dz, const float* rays_d, const int32_t* ray_idx, const int32_t* n_rays_dev,
                              int64_t n_rays, int s0, int S, int S_total, float* T, nm_stream_t stream) {
    NM_REQUIRE(n_rays == 0 || (raw && dz && rays_d && T), "nm_transmittance_chunk_dz: null pointer");
    NM_REQUIRE(n_rays >= 0 && n_rays < (1ll << 31) && S >= 1 && s0 >= 0 && s0 + S <= S_total, "nm_transmittance_chunk_dz: bad sizes (s0=%d S=%d S_total=%d)",
               s0, S, S_total);
    NM_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 15) == 0, "nm_transmittance_chunk_dz: raw must be 16-byte aligned");
    if (n_rays == 0) return NM_OK;
    int64_t blocks = (n_rays + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(transmittance_chunk_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, nm::as_stream(stream), raw, dz, rays_d, ray_idx,
                       n_rays_dev, (int)n_rays, s0, S, S_total, T);
    return nm::check_launch("transmittance_chunk_kernel<dz>");
}

int64_t nm_march_pass_workspace_floats(int64_t R) { return R > 0 ? march_ws_floats(R) : 0; }

int nm_march_pass(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int64_t R, int S_total, int chunk, float eps,
                  int sigma_only, int precision, float sigma_scale, const float* dz, const float* occ_z_far, const float* occ_T, float* workspace,
                  int64_t workspace_floats, float* raw_out, int64_t* stats, nm_stream_t stream) {
    const char* who = "nm_march_pass";
    NM_REQUIRE(mlp, "%s: null handle", who);
    NM_REQUIRE(R == 0 || (origin && direction && z_vals && workspace && raw_out), "%s: null pointer", who);
    NM_REQUIRE(R >= 0 && R < (1ll << 31) && S_total >= 1 && chunk >= 1, "%s: bad sizes (R=%lld S_total=%d chunk=%d)", who, (long long)R, S_total, chunk);
    NM_REQUIRE((occ_z_far == nullptr) == (occ_T == nullptr), "%s: occ_z_far and occ_T go together", who);
    NM_MARCH_REQUIRE(who, mlp, precision, sigma_only);
    NM_REQUIRE((reinterpret_cast<uintptr_t>(raw_out) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "%s: raw_out and workspace must be 16-byte aligned", who);
    NM_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "%s: stats must be 8-byte aligned", who);
    NM_REQUIRE(workspace_floats >= nm_march_pass_workspace_floats(R), "%s: workspace of %lld floats, %lld needed", who, (long long)workspace_floats,
               (long long)nm_march_pass_workspace_floats(R));
    if (R == 0) return NM_OK;
    return march_pass(mlp, origin, direction, z_vals, R, S_total, chunk, eps, sigma_only, precision, sigma_scale, dz, occ_z_far, occ_T, workspace, raw_out,
                      stats, stream);
}

int64_t nm_render_rays_bkg_march_workspace_floats(int64_t R, int S, int N) {
    // two nets: coarse z [R,S] | coarse raw [R,S,4] |; per-ray scratch of the composite [R,6] | one march's workspace (the passes take it in turn)
    if (R <= 0) return 0;
    return (N > 0 ? align4(R * S) + align4(R * S * 4) : 0) + align4(R * 6) + march_ws_floats(R);
}

int nm_render_rays_bkg_march(nm_mlp_t coarse, nm_mlp_t fine, const float* origin, const float* direction, const float* near, const float* far,
                             int64_t R, int S, int N, const float* t_vals, const float* u, int white_bkg, int precision_coarse, int precision_fine,
                             float eps, float eps_coarse, int chunk, float* workspace, int64_t workspace_floats, float* raw_out, float* z_out,
                             float* rgb, float* depth, float* acc, int64_t* stats, nm_stream_t stream) {
    const char* who = "nm_render_rays_bkg_march";
    NM_REQUIRE(coarse, "%s: null handle", who);
    NM_REQUIRE(R == 0 || (origin && direction && near && far && t_vals && workspace && raw_out && z_out), "%s: null pointer", who);
    NM_REQUIRE(R >= 0 && R < (1ll << 31) && S >= 1 && N >= 0 && chunk >= 1, "%s: bad sizes (R=%lld S=%d N=%d chunk=%d)", who, (long long)R, S, N, chunk);
    NM_REQUIRE((N == 0) == (fine == nullptr), "%s: a fine net and N > 0 importance samples go together (S=%d N=%d)", who, S, N);
    NM_REQUIRE(N == 0 || (u && S >= 3), "%s: the importance samples need u [N] and S >= 3 (S=%d N=%d)", who, S, N);
    NM_REQUIRE(!rgb || (depth && acc), "%s: rgb, depth and acc go together", who);
    if (fine) {
        NM_MARCH_REQUIRE(who, coarse, precision_coarse, 1);
        NM_MARCH_REQUIRE(who, fine, precision_fine, 0);
    } else {
        NM_MARCH_REQUIRE(who, coarse, precision_coarse, 0);
    }
    NM_REQUIRE((reinterpret_cast<uintptr_t>(raw_out) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "%s: raw_out and workspace must be 16-byte aligned", who);
    NM_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "%s: stats must be 8-byte aligned", who);
    NM_REQUIRE(workspace_floats >= nm_render_rays_bkg_march_workspace_floats(R, S, N), "%s: workspace of %lld floats, %lld needed", who,
               (long long)workspace_floats, (long long)nm_render_rays_bkg_march_workspace_floats(R, S, N));
    if (R == 0) return NM_OK;
    int rc;
    float* zc = workspace;
    float* rawc = zc + (N > 0 ? align4(R * S) : 0);
    float* scratch = rawc + (N > 0 ? align4(R * S * 4) : 0);              // [R,6]: rgb [R,3] | disp | acc | depth; the composite's disp is discarded
    float* mws = scratch + align4(R * 6);
    if (!fine) {                                                  // one pass: its output is what is composited
        if ((rc = nm_ray_to_samples(origin, direction, near, far, R, S, t_vals, 0, nullptr, nullptr, nullptr, z_out, stream))) return rc;
        if ((rc = march_pass(coarse, origin, direction, z_out, R, S, chunk, eps, 0, precision_coarse, 1.f, nullptr, nullptr, nullptr, mws, raw_out, stats,
                             stream))) return rc;
        if (stats && (rc = nm::check_hip(hipMemsetAsync(stats + 2, 0, 2 * sizeof(int64_t), nm::as_stream(stream)), "nm_render_rays_bkg_march: stats"))) return rc;
    } else {
        // the coarse pass only places the importance samples: density only, cut on its own transmittance at eps_coarse (render_utils.py:139-147)
        if ((rc = nm_ray_to_samples(origin, direction, near, far, R, S, t_vals, 0, nullptr, nullptr, nullptr, zc, stream))) return rc;
        if ((rc = march_pass(coarse, origin, direction, zc, R, S, chunk, eps_coarse, 1, precision_coarse, 1.f, nullptr, nullptr, nullptr, mws, rawc,
                             stats ? stats + 2 : nullptr, stream))) return rc;
        if ((rc = nm_importance_from_raw(rawc, zc, direction, R, S, u, N, z_out, nullptr, stream))) return rc;
        if ((rc = march_pass(fine, origin, direction, z_out, R, S + N, chunk, eps, 0, precision_fine, 1.f, nullptr, nullptr, nullptr, mws, raw_out, stats,
                             stream))) return rc;
    }
    if (rgb && (rc = nm_composite(raw_out, z_out, direction, R, S + N, white_bkg, nullptr, rgb, scratch + 3 * R, acc, nullptr, depth, stream))) return rc;
    return NM_OK;
}

}  // extern "C"
