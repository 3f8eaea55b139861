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
// The stage / search / rank code is merge_wide_device.h's wide_merge_rays (shared with the layered form, merge_layers.hip); this file is its
// compositing tail and the entry point.
#include "common.h"
#include "composite_device.h"
#include "merge_wide_device.h"

namespace {

using namespace nm_wide;

constexpr int kWideMaxWaves = 4;

__global__ __launch_bounds__(64 * kWideMaxWaves) void merge_composite_wide_kernel(const WideLists L, int64_t R, const float* __restrict__ rays_d,
                                                                                  int white_bkg, int wave_bytes, float* __restrict__ rgb,
                                                                                  float* __restrict__ depth, float* __restrict__ acc) {
    wide_merge_rays(L, R, wave_bytes, [&](int64_t r, bool live, int lane, const float4** rbase, const float* lz, const unsigned* msrc) {
        const float dx = rays_d[r * 3 + 0], dy = rays_d[r * 3 + 1], dz = rays_d[r * 3 + 2];
        const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
        const CompositeSums c = composite_ray(L.S_total, dnorm, lane, nullptr,
                                              [&](int s) {
                                                  const unsigned src = msrc[s];
                                                  return rbase[src >> 16][src & 0xffffu];
                                              },
                                              [&](int s) { return lz[msrc[s] & 0xffffu]; }, [&](int, float) {});
        if (lane == 0 && live) composite_store(c, white_bkg, r, rgb, nullptr, acc, depth);
    });
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
    WideLists L;
    if (int rc = wide_lists_from_args("nm_merge_composite_lists_wide", k, z, raw, rows, S, R, kWideMaxSamples, L)) return rc;
    NM_REQUIRE(R >= 0 && (R == 0 || (rays_d && rgb && depth && acc)), "nm_merge_composite_lists_wide: null pointer");
    if (R == 0) return NM_OK;
    int waves, wave_bytes;
    size_t lds;
    wide_launch_shape(L.S_total, kWideMaxWaves, waves, wave_bytes, lds);
    hipLaunchKernelGGL(merge_composite_wide_kernel, dim3(wide_grid(R, waves)), dim3(64 * waves), lds, nm::as_stream(stream), L, R, rays_d, white_bkg,
                       wave_bytes, rgb, depth, acc);
    return nm::check_launch("merge_composite_wide_kernel");
}

}  // extern "C"
