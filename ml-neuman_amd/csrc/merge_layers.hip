// K7d: the merge + composite tail of the hybrid renderers WITH per-list layers: besides rgb / depth / acc of the merged list, for every source list
// l the sums of its own samples' terms -- layer_acc = sum w, layer_rgb = sum w sigmoid(rgb) (premultiplied, no background), layer_depth = sum w z --
// with w the weight the sample has in the MERGED list (the other lists' occlusion resolved).  The merged list never exists in HBM, so neither
// does the list a sample came from: the sums are formed where the merge kernels already know it (msrc = list << 16 | index).
//
//   * The merge is merge_wide_device.h's (one wave per ray, 1 .. 32 lists, 8 B of LDS per merged sample), the compositing is composite_ray
//     (composite_device.h, untouched), the body of every compositing kernel: rgb / depth / acc are bit-identical to nm_merge_composite_lists_wide.
//   * The body hands every sample's weight to a callback.  The callback forms the sample's terms as the body does and adds them to the accumulators
//     of the sample's list and +0.f to those of every other list: a lane's samples in merged order, chunk by chunk, then wave_sum, the scheme of
//     the totals.  With one list the layer IS the totals, bit for bit.  No atomics: two runs give the same bits.
//   * Many lists: UNROLLED GROUPS IN REGISTERS, no LDS table.  The kernel is a template on the number of accumulator sets NL in {2, 4, 8, 16, 32}
//     (the smallest that holds k); the 5 NL accumulators are selected by compare-and-add in fully unrolled loops, so every index is a constant and
//     nothing goes to scratch.  An LDS table of per-lane accumulators (1280 B per list and wave: 40 KB at 32 lists) would take the waves in flight
//     that bound these kernels (merge_composite_kernel's comment: 9.0 against 13.8 ms for 12 more bytes per sample); registers cost VALU work only,
//     5 NL selects + adds per chunk of 64 samples, beside k searches of ~log2(S) LDS round trips each.  At NL = 32 the 160 accumulators leave two
//     waves per SIMD, which a block of at most four waves never exceeds anyway.
//   * So the layered form stages exactly what the unlayered one does: nm_merge_composite_layers_max_samples(k) = 8014 for every k.
#include "common.h"
#include "composite_device.h"
#include "merge_wide_device.h"

namespace {

using namespace nm_wide;

constexpr int kLayersMaxWaves = 4;

template <int NL>
__global__ __launch_bounds__(64 * kLayersMaxWaves) void merge_composite_layers_kernel(const WideLists L, int64_t R, const float* __restrict__ rays_d,
                                                                                      int white_bkg, int wave_bytes, float* __restrict__ rgb,
                                                                                      float* __restrict__ depth, float* __restrict__ acc,
                                                                                      float* __restrict__ layer_rgb, float* __restrict__ layer_depth,
                                                                                      float* __restrict__ layer_acc) {
    wide_merge_rays(L, R, wave_bytes, [&](int64_t r, bool live, int lane, const float4** rbase, const float* lz, const unsigned* msrc) {
        const float dx = rays_d[r * 3 + 0], dy = rays_d[r * 3 + 1], dz = rays_d[r * 3 + 2];
        const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
        float ar[NL], ag[NL], ab[NL], ad[NL], aa[NL];              // (constant indices only: registers)
#pragma unroll
        for (int l = 0; l < NL; ++l) ar[l] = ag[l] = ab[l] = ad[l] = aa[l] = 0.f;
        const auto raw_at = [&](int s) {
            const unsigned src = msrc[s];
            return rbase[src >> 16][src & 0xffffu];
        };
        const auto z_at = [&](int s) { return lz[msrc[s] & 0xffffu]; };
        // composite_ray calls this with every sample's weight, just before it adds the sample's terms to the totals: the same expressions on the
        // same operands here (the record and depth are re-read, not re-evaluated differently), so a layer's terms are the totals' terms bit for bit
        const CompositeSums c = composite_ray(L.S_total, dnorm, lane, nullptr, raw_at, z_at, [&](int s, float w) {
            const float4 q = raw_at(s);
            const float tr = w * sigmoidf_(q.x), tg = w * sigmoidf_(q.y), tb = w * sigmoidf_(q.z), td = w * z_at(s);
            const int from = (int)(msrc[s] >> 16);
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const bool own = from == l;
                ar[l] += own ? tr : 0.f;
                ag[l] += own ? tg : 0.f;
                ab[l] += own ? tb : 0.f;
                ad[l] += own ? td : 0.f;
                aa[l] += own ? w : 0.f;
            }
        });
        if (lane == 0 && live) composite_store(c, white_bkg, r, rgb, nullptr, acc, depth);
        const int k = L.k;
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= k) continue;                                  // (wave-uniform)
            const float sr = wave_sum(ar[l]), sg = wave_sum(ag[l]), sb = wave_sum(ab[l]), sd = wave_sum(ad[l]), sa = wave_sum(aa[l]);
            if (lane == 0 && live) {
                const int64_t o = r * k + l;
                layer_rgb[o * 3 + 0] = sr; layer_rgb[o * 3 + 1] = sg; layer_rgb[o * 3 + 2] = sb;
                layer_acc[o] = sa;
                if (layer_depth) layer_depth[o] = sd;
            }
        }
    });
}

inline int layers_grid(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

}  // namespace

extern "C" {

int nm_merge_composite_layers_max_samples(int k) { return (k >= 1 && k <= kMaxWideLists) ? kWideMaxSamples : 0; }

int nm_merge_composite_layers(int k, const float* const* z, const float* const* raw, const int32_t* const* rows, const int* S, int64_t R,
                              const float* rays_d, int white_bkg, float* rgb, float* depth, float* acc, float* layer_rgb, float* layer_depth,
                              float* layer_acc, nm_stream_t stream) {
    WideLists L;
    if (int rc = wide_lists_from_args("nm_merge_composite_layers", k, z, raw, rows, S, R, nm_merge_composite_layers_max_samples(k), L)) return rc;
    NM_REQUIRE(R >= 0 && (R == 0 || (rays_d && rgb && depth && acc && layer_rgb && layer_acc)), "nm_merge_composite_layers: null pointer");
    if (R == 0) return NM_OK;
    int waves, wave_bytes;
    size_t lds;
    wide_launch_shape(L.S_total, kLayersMaxWaves, waves, wave_bytes, lds);
    const dim3 grid(layers_grid(R, waves)), block(64 * waves);
    hipStream_t st = nm::as_stream(stream);
#define NM_LAYERS_LAUNCH(NL)                                                                                                                        \
    hipLaunchKernelGGL(merge_composite_layers_kernel<NL>, grid, block, lds, st, L, R, rays_d, white_bkg, wave_bytes, rgb, depth, acc, layer_rgb, \
                       layer_depth, layer_acc)
    if (k <= 2) NM_LAYERS_LAUNCH(2);
    else if (k <= 4) NM_LAYERS_LAUNCH(4);
    else if (k <= 8) NM_LAYERS_LAUNCH(8);
    else if (k <= 16) NM_LAYERS_LAUNCH(16);
    else NM_LAYERS_LAUNCH(32);
#undef NM_LAYERS_LAUNCH
    return nm::check_launch("merge_composite_layers_kernel");
}

}  // extern "C"
