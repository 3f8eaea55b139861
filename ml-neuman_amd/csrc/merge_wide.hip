// K7c: the merge + composite tail of the multi-person renderer for ANY number of actors (reference utils/render_utils.py:441-456:
// sort(cat(z lists)), the gather of cat(raw lists), raw2outputs) as ONE kernel: up to 32 sorted lists per ray, the merged list never in HBM.
//
// ray_ops.hip's merge_composite_kernel keeps the state of its (at most four) lists in unrolled registers; that does not scale to 32.  Here:
//   * one wave per ray; the lists' z are staged in LDS, concatenated, by ONE flat loop over the St merged samples (a sample's list is found
//     by a 5-step search in the LDS table of list offsets), so a ray's loads are all in flight together whatever the number of lists;
//   * what is indexed by a lane-varying list number -- the arrays' base pointers, the rows[] indirections, the ray's row bases -- lives in
//     LDS tables (a block table filled once from the kernel arguments, a per-wave table filled per ray by lanes 0 .. k-1); what is indexed
//     by the wave-uniform loop over the foreign lists (their sizes and offsets) is read from the kernel arguments into SGPRs.  No
//     runtime-indexed register arrays: nothing goes to scratch;
//   * a sample's position in the merged order is its own index plus, per foreign list, the number of that list's samples that come first
//     (an earlier list's equal samples do, a later list's do not: the stable order, i.e. what nm_merge_sorted applied list by list gives),
//     found by branch-free fixed-step searches, two samples per lane so that the LDS round trips of a step overlap;
//   * the records are read from global memory in merged order by composite_ray (composite_device.h: the body every compositing kernel
//     shares), so rgb / depth / acc are bit-identical to nm_merge_sorted list by list + nm_composite, and for k <= 4 to nm_merge_composite_lists.
// Bound: like merge_composite_kernel by the latency of the per-ray chains (searches, the f64 transmittance scan), i.e. by waves in flight.
#include "common.h"
#include "composite_device.h"

namespace {

constexpr int kMaxWideLists = 32;                                  // (= ray_ops.hip's kMaxIntervalLists)
// dynamic LDS: the block's list table | per wave: the ray's row bases, then 8 B per merged sample
constexpr int kWideTabBytes = 3 * kMaxWideLists * 8 + 36 * 4;      // z, raw, rows base pointers [32] | list offsets [36], unused ones INT_MAX
constexpr int kWideWaveTabBytes = 2 * kMaxWideLists * 8;           // the ray's z and raw row pointers [32]
constexpr int kWideBytesPerSample = 8;                             // staged z | merged source (list << 16 | position among the staged z)
constexpr int kWideLdsBytes = 64 * 1024;                           // per block: the default dynamic-LDS limit, no launch attribute needed
constexpr int kWideMaxWaves = 4;
constexpr int kWideMaxSamples = (kWideLdsBytes - kWideTabBytes - kWideWaveTabBytes) / kWideBytesPerSample;      // 8014 merged samples
static_assert(kWideTabBytes % 16 == 0 && kWideWaveTabBytes % 16 == 0, "LDS carve offsets stay 16-byte aligned");

struct WideLists {
    const float* z[kMaxWideLists];
    const float4* raw[kMaxWideLists];
    const int32_t* rows[kMaxWideLists];
    int S[kMaxWideLists];
    int k, S_total;
};

// the list that merged-concatenation index e belongs to: the largest l with off[l] <= e (off[l] = INT_MAX from l = k on)
__device__ __forceinline__ int wide_list_of(const int* off, int e) {
    int l = 0;
#pragma unroll
    for (int half = kMaxWideLists / 2; half > 0; half >>= 1) l = off[l + half] <= e ? l + half : l;
    return l;
}

__global__ __launch_bounds__(64 * kWideMaxWaves) void merge_composite_wide_kernel(const WideLists L, int64_t R, const float* __restrict__ rays_d,
                                                                                  int white_bkg, int wave_bytes, float* __restrict__ rgb,
                                                                                  float* __restrict__ depth, float* __restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) char lds_wide[];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int k = L.k, St = L.S_total;
    const float** tab_z = reinterpret_cast<const float**>(lds_wide);
    const float4** tab_raw = reinterpret_cast<const float4**>(lds_wide + kMaxWideLists * 8);
    const int32_t** tab_rows = reinterpret_cast<const int32_t**>(lds_wide + 2 * kMaxWideLists * 8);
    int* tab_off = reinterpret_cast<int*>(lds_wide + 3 * kMaxWideLists * 8);
    if (threadIdx.x < 36) {
        int o = 0;
        for (int l = 0; l < k && l < (int)threadIdx.x; ++l) o += L.S[l];
        tab_off[threadIdx.x] = (int)threadIdx.x < k ? o : 0x7fffffff;
    }
    if (threadIdx.x == 0)
        for (int l = 0; l < k; ++l) {                              // (uniform index: scalar loads of the kernel arguments)
            tab_z[l] = L.z[l];
            tab_raw[l] = L.raw[l];
            tab_rows[l] = L.rows[l];
        }
    __syncthreads();
    char* wave_lds = lds_wide + kWideTabBytes + (size_t)wib * wave_bytes;
    const float** zbase = reinterpret_cast<const float**>(wave_lds);
    const float4** rbase = reinterpret_cast<const float4**>(wave_lds + kMaxWideLists * 8);
    float* lz = reinterpret_cast<float*>(wave_lds + kWideWaveTabBytes);
    unsigned* msrc = reinterpret_cast<unsigned*>(lz + St);        // (the merged z is read through it: lz[msrc & 0xffff], no second copy of z)
    for (int64_t r0 = blockIdx.x * (int64_t)wpb; r0 < R; r0 += (int64_t)gridDim.x * wpb) {
        const bool live = r0 + wib < R;
        const int64_t r = live ? r0 + wib : R - 1;
        if (lane < k) {                                            // lane l: where list l's row of this ray starts
            const int32_t* rw = tab_rows[lane];
            const int64_t row = rw ? (int64_t)rw[r] : r;
            const int64_t o = row * ((lane + 1 < k ? tab_off[lane + 1] : St) - tab_off[lane]);
            zbase[lane] = tab_z[lane] + o;
            rbase[lane] = tab_raw[lane] + (o - tab_off[lane]);        // (indexed by a sample's position among the staged z)
        }
        __syncthreads();
        for (int e = lane; e < St; e += 64) {
            const int l = wide_list_of(tab_off, e);
            lz[e] = zbase[l][e - tab_off[l]];
            msrc[e] = 0u;                                          // (a list whose z is not ordered -- NaN -- leaves merged slots unwritten: they stay in bounds)
        }
        __syncthreads();
        for (int e0 = 0; e0 < St; e0 += 128) {
            int e[2], a[2], own[2], pos[2];
            float v[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                e[q] = e0 + 64 * q + lane;
                const int ec = e[q] < St ? e[q] : St - 1;
                v[q] = lz[ec];
                a[q] = wide_list_of(tab_off, ec);
                own[q] = ec - tab_off[a[q]];
                pos[q] = own[q];
            }
            int om = 0;
            for (int m = 0; m < k; ++m) {                          // the foreign lists, one after another: m, its size and offset are wave-uniform
                const int Sm = L.S[m];
                const int steps = 32 - __clz(Sm);                  // (1 << steps) > Sm
                int cnt[2] = {0, 0};
                for (int st = steps - 1; st >= 0; --st) {
                    const int half = 1 << st;
                    float x[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int t = cnt[q] + half;
                        x[q] = lz[om + (t <= Sm ? t - 1 : 0)];
                    }
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int t = cnt[q] + half;
                        const bool first = m < a[q] ? x[q] <= v[q] : x[q] < v[q];
                        cnt[q] = (t <= Sm && first) ? t : cnt[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) pos[q] += m != a[q] ? cnt[q] : 0;
                om += Sm;
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (e[q] >= St) continue;
                msrc[pos[q]] = ((unsigned)a[q] << 16) | (unsigned)e[q];
            }
        }
        __syncthreads();
        const float dx = rays_d[r * 3 + 0], dy = rays_d[r * 3 + 1], dz = rays_d[r * 3 + 2];
        const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
        const CompositeSums c = composite_ray(St, dnorm, lane, nullptr,
                                              [&](int s) {
                                                  const unsigned src = msrc[s];
                                                  return rbase[src >> 16][src & 0xffffu];
                                              },
                                              [&](int s) { return lz[msrc[s] & 0xffffu]; }, [&](int, float) {});
        if (lane == 0 && live) composite_store(c, white_bkg, r, rgb, nullptr, acc, depth);
        __syncthreads();
    }
}

inline int wide_grid(int64_t items, int per_block) {
    int64_t b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

}  // namespace

namespace nm {

int wide_merge_max_samples() { return kWideMaxSamples; }

}  // namespace nm

extern "C" {

int nm_merge_composite_lists_wide(int k, const float* const* z, const float* const* raw, const int32_t* const* rows, const int* S, int64_t R,
                                  const float* rays_d, int white_bkg, float* rgb, float* depth, float* acc, nm_stream_t stream) {
    NM_REQUIRE(k >= 1 && k <= kMaxWideLists && z && raw && S, "nm_merge_composite_lists_wide: 1 <= k <= %d lists (k=%d)", kMaxWideLists, k);
    NM_REQUIRE(R >= 0 && (R == 0 || (rays_d && rgb && depth && acc)), "nm_merge_composite_lists_wide: null pointer");
    WideLists L;
    L.k = k;
    int64_t total = 0;
    for (int l = 0; l < kMaxWideLists; ++l) {
        const bool on = l < k;
        L.z[l] = on ? z[l] : nullptr;
        L.raw[l] = on ? reinterpret_cast<const float4*>(raw[l]) : nullptr;
        L.rows[l] = (on && rows) ? rows[l] : nullptr;
        L.S[l] = on ? S[l] : 0;
        if (on) {
            NM_REQUIRE(R == 0 || (z[l] && raw[l]), "nm_merge_composite_lists_wide: list %d is null", l);
            NM_REQUIRE(S[l] >= 1, "nm_merge_composite_lists_wide: list %d is empty", l);
            NM_REQUIRE((reinterpret_cast<uintptr_t>(raw[l]) & 15) == 0, "nm_merge_composite_lists_wide: raw arrays must be 16-byte aligned");
            total += S[l];
        }
    }
    NM_REQUIRE(total <= kWideMaxSamples, "nm_merge_composite_lists_wide: %lld merged samples, at most %d can be staged in LDS", (long long)total,
               kWideMaxSamples);
    L.S_total = (int)total;
    if (R == 0) return NM_OK;
    const int wave_bytes = kWideWaveTabBytes + ((L.S_total * kWideBytesPerSample + 15) & ~15);
    int waves = (kWideLdsBytes - kWideTabBytes) / wave_bytes;
    if (waves > kWideMaxWaves) waves = kWideMaxWaves;
    if (waves < 1) waves = 1;
    const size_t lds = (size_t)kWideTabBytes + (size_t)waves * wave_bytes;
    NM_REQUIRE(lds <= (size_t)kWideLdsBytes, "nm_merge_composite_lists_wide: %d merged samples, at most %d can be staged in LDS", L.S_total, kWideMaxSamples);
    hipLaunchKernelGGL(merge_composite_wide_kernel, dim3(wide_grid(R, waves)), dim3(64 * waves), lds, nm::as_stream(stream), L, R, rays_d, white_bkg,
                       wave_bytes, rgb, depth, acc);
    return nm::check_launch("merge_composite_wide_kernel");
}

}  // extern "C"
