// NM_PREC_I8X3, the colour head alone: the second launch of nm_mlp_forward_rays_live and the other nm_mlp_forward_*_live entries.  The trunk launch (mlp_i8s.hip TRUNK) has written every
// sample's density and listed the samples compositing can see (stored density not <= 0) with their quantised stage-7 activations; this kernel runs
// feature_linear, the views layer and rgb_linear -- ring blocks 69..81 of nerf_mlp_i8s_kernel's tile, 324 of its 1884 MFMAs per 32 samples -- on the
// listed samples only and writes their colours beside the densities.  Same workgroup shape, ring and helpers (mlp_i8as.h), and operation for operation
// the arithmetic of that kernel's stages 8 (features), 9 and 10: a listed sample's record is bit-identical to the whole-network launch's.
// A wave's 32 samples are 32 consecutive list entries: whatever rays they come from, each takes its direction encoding from its own ray (in_mode 3:
// the entry is the record r * S_total + s of a ray form) or from its own point's direction (in_mode 4: the entry is the record k of a point form).
//
// Reference semantics: models/vanilla.py NeRF.forward (:136-144).
#include "mlp_i8as.h"

namespace {

// the head's ring blocks: feature_linear's eight output blocks (8 k-steps) | the views layer's four (8 limb + 2 encoding steps) | rgb_linear's one (4)
constexpr int kHeadBlocks = 13;
constexpr int kHeadSteps = 8 * 8 + 4 * 10 + 4;                // 108: steps [520, 628) of the tile's stream
struct HeadStream {
    static __host__ __device__ constexpr int steps(int i) {
        i = i >= kHeadBlocks ? i - kHeadBlocks : i;
        return i < 8 ? 8 : i < 12 ? 10 : 4;
    }
    static constexpr int kBytes = kHeadSteps * nm::kStepBytes;
};
typedef RingT<HeadStream> Ring;

__global__ __launch_bounds__(kWaves * 64, 2) void nerf_head_i8s_kernel(const Args8s A) {
    __shared__ uint4 lds[kPeU4 + kSlots * kSlotU4 + kBiasU4];
    const MlpArgs a = resolve_args(A.a);                                               // in_mode 3 / 4 over the list: a.n = its length
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, s = lane & 31;
    uint4* pw = lds + w * kPWaveU4;
    Ring R;
    R.src = reinterpret_cast<const char*>(A.image8) + lane * 16 + w * 1024;
    R.rd = lds + kPeU4 + lane;
    R.lds0 = (unsigned)(uintptr_t)(lds + kPeU4) + w * 1024;
    R.off = 0;
    R.slot = 0;
    {                                                                                   // the bias table
        float* lb = reinterpret_cast<float*>(lds + kPeU4 + kSlots * kSlotU4);
        for (int i = tid; i < nm::kBiasFloats + 16; i += kWaves * 64) lb[i] = A.consts8[nm::kBiasFloats + i];
    }
    __syncthreads();
    ring_piece(R, 0, 0, 0);                                                             // blocks 0 and 1 of the first tile (two pieces each)
    ring_piece(R, 0, 0, 1);
    ring_piece(R, HeadStream::steps(0) * nm::kStepBytes, 1, 0);
    ring_piece(R, HeadStream::steps(0) * nm::kStepBytes, 1, 1);
    R.off = (HeadStream::steps(0) + HeadStream::steps(1)) * nm::kStepBytes;
    const float u_r = A.consts8[nm::stage_b_off(10)], u_g = A.consts8[nm::stage_b_off(10) + 1], u_b = A.consts8[nm::stage_b_off(10) + 2];
    const float* kappa = reinterpret_cast<const float*>(lds + kPeU4 + kSlots * kSlotU4) + nm::kBiasFloats;
    unsigned bias_lds = (unsigned)(uintptr_t)(lds + kPeU4 + kSlots * kSlotU4) + 16 * g;        // this lane's half of every group of 8
    asm volatile("" : "+v"(bias_lds));
    lds_cfloat* bias = (lds_cfloat*)(uintptr_t)bias_lds;
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    for (int i = lane; i < kPWaveU4; i += 64) pw[i] = make_uint4(0, 0, 0, 0);          // pad slots: finite once

#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * kTile + w * kRows;                                  // this wave's first list entry (entries past n: clamped)
        asm volatile("" : "+s"(R.off));                                                 // (every tile walks the same 13 blocks: left a constant, the compiler keeps a
                                                                                        // copy address per piece across tiles, 24 register pairs, spilled)
        int64_t e = row0 + s;
        const bool mine = e < a.n;
        if (!mine) e = a.n - 1;
        X8 X;
        {
            const uint4* src = A.live.x + g * A.live.cap + e;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                X.h[k] = src[(4 * k) * A.live.cap];
                X.l[k] = src[(4 * k + 2) * A.live.cap];
            }
        }
        float sx = A.live.sx[e];
        const int rec = A.live.idx[e];
        fill_pe_wave(pw, true, a, row0, lane);                                          // the direction encoding of each entry's own ray
        // ---------------- stage 8: feature (linear, 256)
        {
            const float sxin = sx * (256.f * kappa[8]);
            f32x16 f[8];
            float m = 0.f;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                i32x16 t;
                k_i8<8>(t, X, ring_enter(R, b), R);
                dequant16(f[b], t, sxin, bias + nm::stage_b_off(8) + 32 * b);
                m = max16<false>(m, f[b]);
            }
            const float M = row_max(m), inv = inv_of(M);
#pragma unroll
            for (int b = 0; b < 8; ++b) quant16<false>(f[b], inv, X.h[b], X.l[b]);
            sx = scale_of(M);
        }
        // ---------------- stage 9: views layer, K = feature(256) ++ d_pe(32), N = 128, ReLU
        {
            const float sxin = sx * (256.f * kappa[9]);
            f32x16 f[4];
            float m = 0.f;
            Enc<2> E;
            load_enc(E, pw, g, s);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                i32x16 t;
                const uint4* ws = ring_enter(R, 8 + b);
                k_i8<8>(t, X, ws, R);
                dequant16(f[b], t, sxin, bias + nm::stage_b_off(9) + 32 * b);
                k_bf<2>(f[b], E, ws + 8 * kStepU4);
                m = max16<true>(m, f[b]);
            }
            const float M = row_max(m), inv = inv_of(M);
#pragma unroll
            for (int b = 0; b < 4; ++b) quant16<true>(f[b], inv, X.h[b], X.l[b]);
            sx = scale_of(M);
        }
        // ---------------- stage 10: rgb (rows 0..2 of one block), K = 128; the density of the record is the trunk's
        {
            i32x16 t;
            f32x16 fr;
            k_i8<4>(t, X, ring_enter(R, 12), R);
            dequant16(fr, t, sx * (256.f * kappa[10]), bias + nm::stage_b_off(10));
            if (g == 0 && mine) {
                float* o = a.out + (int64_t)rec * 4;
                o[0] = fr[0] * u_r; o[1] = fr[1] * u_g; o[2] = fr[2] * u_b;
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                    // the copy started for a tile that never comes
}

}  // namespace

namespace nm {

int launch_mlp_i8h(const MlpLaunch& L, const void* head8, int in_mode, const float* dirs, const float* direction, int S_total, const LiveList& live,
                   int64_t max_entries, float* out, hipStream_t stream) {
    Args8s A;
    MlpArgs& a = A.a;
    a.ray_idx = live.idx;                                                               // the records the trunk listed: out[rec], and the direction of
    a.n_rays_dev = live.count;                                                          // ray rec / S_total (in_mode 3) or dirs[rec] itself (in_mode 4)
    a.s0 = 0;
    a.S_total = S_total;
    a.wpack = nullptr; a.bias = nullptr;
    a.petab = L.petab;
    a.pts = nullptr; a.dirs = dirs; a.origin = nullptr; a.direction = direction; a.z = nullptr;
    a.out = out; a.dbg = nullptr; a.prof = nullptr; a.n = max_entries; a.S = S_total; a.in_mode = in_mode; a.stop_stage = -2; a.sigma_scale = 1.f;
    a.sigma_only = 0;
    a.save_h = nullptr; a.save_hv = nullptr; a.save_bits = nullptr; a.save_h16 = nullptr; a.save_feat16 = nullptr; a.save_hvbits = nullptr; a.save_x0h = nullptr; a.save_d0h = nullptr;
    a.pos = PeSpec{L.pe_kind, L.pos_nfreq, L.pos_octaves};
    a.dir = PeSpec{L.pe_kind, L.dir_nfreq, L.dir_octaves};
    A.consts8 = L.consts8;
    A.image8 = reinterpret_cast<const uint4*>(head8);
    A.live = live;
    const int64_t ntiles = (max_entries + kTile - 1) / kTile;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    const int grid = (int)(ntiles < cus ? ntiles : cus);
    hipLaunchKernelGGL(nerf_head_i8s_kernel, dim3(grid), dim3(kWaves * 64), 0, stream, A);
    return check_launch("nerf_head_i8s_kernel");
}

}  // namespace nm
