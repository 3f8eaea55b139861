// The wide merge (merge_wide.hip, K7c) as device code shared by the kernels that end in it: nm_merge_composite_lists_wide and its layered
// form nm_merge_composite_layers (merge_layers.hip).  wide_merge_rays stages a ray's lists in LDS and settles every sample's place in the
// merged order; what is done with the merged list -- always composite_ray over it -- is the caller's `tail`.  Include after common.h.
#pragma once
#include "common.h"

namespace nm_wide {

constexpr int kMaxWideLists = 32;                                  // (= ray_ops.hip's kMaxIntervalLists)
// dynamic LDS: the block's list table | per wave: the ray's row bases, then 8 B per merged sample
constexpr int kWideTabBytes = 3 * kMaxWideLists * 8 + 36 * 4;      // z, raw, rows base pointers [32] | list offsets [36], unused ones INT_MAX
constexpr int kWideWaveTabBytes = 2 * kMaxWideLists * 8;           // the ray's z and raw row pointers [32]
constexpr int kWideBytesPerSample = 8;                             // staged z | merged source (list << 16 | position among the staged z)
constexpr int kWideLdsBytes = 64 * 1024;                           // per block: the default dynamic-LDS limit, no launch attribute needed
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

// The grid-stride loop over the rays, one wave per ray: stage, merge, then tail(r, live, lane, rbase, lz, msrc) with the merged list in LDS:
// merged sample s is record rbase[msrc[s] >> 16][msrc[s] & 0xffff] at depth lz[msrc[s] & 0xffff].  Called by every thread of the block.
template <class Tail>
__device__ __forceinline__ void wide_merge_rays(const WideLists& L, int64_t R, int wave_bytes, Tail tail) {
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
        tail(r, live, lane, rbase, lz, msrc);
        __syncthreads();
    }
}

// The entry points' shared argument check (`who`: the entry called) -> L; NM_OK or NM_ERR_ARG with the error set.  Nothing touches the device.
inline int wide_lists_from_args(const char* who, int k, const float* const* z, const float* const* raw, const int32_t* const* rows, const int* S, int64_t R,
                                int max_samples, WideLists& L) {
    NM_REQUIRE(k >= 1 && k <= kMaxWideLists && z && raw && S, "%s: 1 <= k <= %d lists (k=%d)", who, kMaxWideLists, k);
    L.k = k;
    int64_t total = 0;
    for (int l = 0; l < kMaxWideLists; ++l) {
        const bool on = l < k;
        L.z[l] = on ? z[l] : nullptr;
        L.raw[l] = on ? reinterpret_cast<const float4*>(raw[l]) : nullptr;
        L.rows[l] = (on && rows) ? rows[l] : nullptr;
        L.S[l] = on ? S[l] : 0;
        if (on) {
            NM_REQUIRE(R == 0 || (z[l] && raw[l]), "%s: list %d is null", who, l);
            NM_REQUIRE(S[l] >= 1, "%s: list %d is empty", who, l);
            NM_REQUIRE((reinterpret_cast<uintptr_t>(raw[l]) & 15) == 0, "%s: raw arrays must be 16-byte aligned", who);
            total += S[l];
        }
    }
    NM_REQUIRE(total <= max_samples, "%s: %lld merged samples, at most %d can be staged in LDS", who, (long long)total, max_samples);
    L.S_total = (int)total;
    return NM_OK;
}

// waves (rays) per block, at most max_waves, and the LDS of a launch over S_total merged samples
inline void wide_launch_shape(int S_total, int max_waves, int& waves, int& wave_bytes, size_t& lds) {
    wave_bytes = kWideWaveTabBytes + ((S_total * kWideBytesPerSample + 15) & ~15);
    waves = (kWideLdsBytes - kWideTabBytes) / wave_bytes;
    if (waves > max_waves) waves = max_waves;
    if (waves < 1) waves = 1;
    lds = (size_t)kWideTabBytes + (size_t)waves * wave_bytes;
}

}  // namespace nm_wide
