// NM_PREC_I8X3, activation-stationary: the same 16-bit fixed-point arithmetic as nerf_mlp_i8w_kernel (mlp.hip; DESIGN.md "K4-i8") with
// the roles of the two operands swapped.  There, a wave owns 64 FEATURES of 64 samples: the activations of the tile live in LDS (every wave
// reads all of them for every block it computes), the weights stream from L2 into every wave group separately (2 x 1.27 MB per 128
// samples), and requantisation needs the row maximum over all features = a partial-maximum exchange through LDS and two barriers per
// stage.  Here a wave owns 32 SAMPLES and ALL features:
//
//   * its input activations of a stage -- 256 features as two int8 limbs -- are 8 k-steps x {hi, lo} x 16 B per lane = 64 registers,
//     resident for the whole stage; the accumulator layout of v_mfma_i32_32x32x32_i8 gives a lane, for its sample, exactly the 16 k-slots
//     the next stage's B operand wants from it (mlp_layout.h slot_feature8), so the requantised outputs of block b ARE the next stage's
//     fragment of k-step b, in place -- activations never touch LDS, never cross lanes (one v_permlane32_swap for the row maximum);
//   * the row maximum is local to the wave: no exchange, no barrier; waves never wait for each other except for the weight ring;
//   * the weights are the A operands, one 1 KB fragment per limb and k-step, used for one MFMA triple.  All 8 waves of the workgroup want
//     the same fragments at about the same time, so the weight image -- re-cut on the host in exactly the order it is consumed
//     (mlp_host.hip pack_stream8s: 628 k-steps of 2 KB per 256-sample tile) -- is streamed ONCE per workgroup from L2 into an LDS ring
//     of whole ring blocks by LDS-DMA (global_load_lds_dwordx4: lane-linear, exactly the fragment format), two blocks ahead of the block
//     being multiplied; the only workgroup barrier is the one per ring block that hands a slot over.
//   Measurements, the variants tried and why the kernel is the way it is: profiles/r03_as_kernel_experiments.md, DESIGN.md "K4-i8s".
//
// Reference semantics: models/vanilla.py Embedder.forward (:82-92), NeRF.forward (:120-152), Joiner.forward (:162-166).
#include "mlp_i8as.h"

namespace {

// flat RING block index of a tile (what one barrier hands over): stage 0: 0-7 (4 steps) | 1-4: 8-39 | 5: 40-47 and its encoding part
// 48-51 (two output blocks x 4 steps each) | 6, 7: 52-67 | 8: 68-76 | 9: 77-80 (10 steps) | 10: 81 (4 steps)
constexpr int kTileBlocks = 82;
__host__ __device__ constexpr int block_steps(int i) {
    i = i >= kTileBlocks ? i - kTileBlocks : i;
    return i < 8 ? 4 : i < 77 ? 8 : i < 81 ? 10 : 4;
}
struct TileStream {                                          // what the ring walks: the whole tile, then the next one
    static __host__ __device__ constexpr int steps(int i) { return block_steps(i); }
    static constexpr int kBytes = (int)nm::kWeightBytes8;
};
typedef RingT<TileStream> Ring;

// PLAIN: the use_viewdirs=False net (--specular_can no; models/vanilla.py:116-117, 145): stages 0..7, then ring block 68 holds output_linear's four rows
// (r, g, b, sigma) where the alpha row is otherwise, and the tile ends there.  The instantiation differs from the default one by ONE wave-uniform exit
// (and the direction encodings it does not compute) and nothing else: this kernel sits at exactly 256 registers, and every other way of telling the
// compiler about the shorter tile (69 as a constant, or as a register, in the ring's look-ahead) made it spill 900-1000 bytes per lane; so the ring
// stays the default one's, and the STREAM is cut to fit it (mlp_host.hip pack_stream8s): where the look-ahead expects blocks 69 and 70 (8 steps each)
// it finds the next tile's blocks 0 and 1 (4 steps each, padded to 8), and the exit points the ring at block 2.  The exit tests a.sigma_only == 2 (set by
// the launch) rather than PLAIN alone, so that the code after it stays in the instantiation: without it the allocation of the stage loop changes too.
// TRUNK: the first of the two launches that shade live samples only (mlp_i8h.hip is the second; nm_mlp_forward_rays_live, nm_mlp_forward_*_live): the same exit after block 68 on
// the whole net's stream cut the same way.  It writes (0, 0, 0, sigma) and, for every sample whose stored density is not <= 0 -- the only ones whose colour
// compositing can see: alpha = 1 - exp(-relu(sigma) dist) is exactly 0 otherwise -- appends what the colour head needs to a global list: the stage-7
// activations it holds (X: 512 B), their row scale and the sample's record in `out` (whatever the input mode).  One ballot, one prefix count and one atomic add per wave; the list is
// [piece 2 t + limb][lane half g][entry][16 B], so that the head's wave loads 32 consecutive entries of a piece as 512 contiguous bytes per lane half,
// already in MFMA operand format.
// (HIP's second __launch_bounds__ argument is the minimum number of WAVES PER SIMD -- not CUDA's blocks per multiprocessor: 2 = the
// 8 waves of the ONE workgroup a CU holds, i.e. a 256-register budget per wave; the 147 KB of LDS allow no second workgroup anyway)
enum { WHOLE = 0, PLAIN = 1, TRUNK = 2 };                   // (the launch sets a.sigma_only = MODE + 1 for the two short tiles)
template <int MODE>
__global__ __launch_bounds__(kWaves * 64, 2) void nerf_mlp_i8s_kernel(const Args8s A) {
    __shared__ uint4 lds[kPeU4 + kSlots * kSlotU4 + kBiasU4];
    const MlpArgs a = resolve_args(A.a);
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
    ring_piece(R, 0, 0, 0);                                                             // blocks 0 and 1 of the first tile (one piece each)
    ring_piece(R, block_steps(0) * nm::kStepBytes, 1, 0);
    R.off = (block_steps(0) + block_steps(1)) * nm::kStepBytes;
    const float u_sigma = A.consts8[nm::stage_b_off(8) + 256];
    const float u_r = A.consts8[nm::stage_b_off(10)], u_g = A.consts8[nm::stage_b_off(10) + 1], u_b = A.consts8[nm::stage_b_off(10) + 2];
    const float* kappa = reinterpret_cast<const float*>(lds + kPeU4 + kSlots * kSlotU4) + nm::kBiasFloats;
    unsigned bias_lds = (unsigned)(uintptr_t)(lds + kPeU4 + kSlots * kSlotU4) + 16 * g;        // this lane's half of every group of 8:
    asm volatile("" : "+v"(bias_lds));                                                  // ONE address register, everything else an immediate
    lds_cfloat* bias = (lds_cfloat*)(uintptr_t)bias_lds;                                // (left alone, the compiler keeps one per block, hoisted
                                                                                        // out of the tile loop and spilled)
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    for (int i = lane; i < kPWaveU4; i += 64) pw[i] = make_uint4(0, 0, 0, 0);          // pad slots: finite once

#pragma unroll 1
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * kTile + w * kRows;                                  // this wave's first sample (rows past n: clamped)
        fill_pe_wave(pw, false, a, row0, lane);
        X8 X;
        float sx;                                                                       // the row scale of X: x = sx * (256 hi + lo) * unit[feature]
        // ---------------- stage 0: encodings only (split bf16), ReLU
        {
            f32x16 f[8];
            float m = 0.f;
            Enc<4> E;
            load_enc(E, pw, g, s);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const uint4* ws = ring_enter(R, b);
                bias16(f[b], bias + nm::stage_b_off(0) + 32 * b);
                k_bf<4, true>(f[b], E, ws, &R);
                m = max16<true>(m, f[b]);
            }
            const float M = row_max(m), inv = inv_of(M);
#pragma unroll
            for (int b = 0; b < 8; ++b) quant16<true>(f[b], inv, X.h[b], X.l[b]);
            sx = scale_of(M);
        }
        // ---------------- stages 1..7: 256 -> 256, ReLU; stage 5 adds the position encoding (four more ring blocks of two output blocks each)
#pragma unroll 1
        for (int st = 1; st <= 7; ++st) {
            const float sxin = sx * (256.f * kappa[st]);
            const int i0 = 8 * st + (st > 5 ? 4 : 0);
            f32x16 f[8];
            float m = 0.f;
            i32x16 tp;                                                                  // block b - 1, dequantised under block b's MFMAs
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const uint4* ws = ring_enter(R, i0 + b);
                if (b == 0) {
                    k_i8<8>(tp, X, ws, R);
                } else {
                    i32x16 t;
                    k_i8_impl<8, true>(t, X, ws, R, f[b - 1], tp, bias + 256 * st + 32 * (b - 1), sxin, m);
                    tp = t;
                }
            }
            dequant16(f[7], tp, sxin, bias + 256 * st + 32 * 7);
            if (st == 5) {
                Enc<4> E;                                                           // (X is dead by now)
                load_enc(E, pw, g, s);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint4* ws = ring_enter(R, 48 + u);
                    k_bf<4, true>(f[2 * u], E, ws, &R, 0);
                    k_bf<4, true>(f[2 * u + 1], E, ws + 4 * kStepU4, &R, 2);
                }
                m = 0.f;                                                                // (the running maximum was taken before the encodings)
#pragma unroll
                for (int b = 0; b < 7; ++b) m = max16<true>(m, f[b]);
            }
            m = max16<true>(m, f[7]);
            const float M = row_max(m), inv = inv_of(M);
#pragma unroll
            for (int b = 0; b < 8; ++b) quant16<true>(f[b], inv, X.h[b], X.l[b]);
            sx = scale_of(M);
            if (st == 5 && !(MODE != WHOLE && a.sigma_only == MODE + 1)) {
                fill_pe_wave(pw, true, a, row0, lane);                                  // the position encoding is done with: direction encoding
            }
        }
        if (MODE == PLAIN && a.sigma_only == 2) {
            // ---------------- the plain head: rows 0..3 of block 68 = output_linear's (r, g, b, sigma)
            i32x16 t;
            f32x16 fo;
            k_i8<8>(t, X, ring_enter(R, 68), R);
            dequant16(fo, t, sx * (256.f * kappa[8]), bias + nm::stage_b_off(8) + 256);
            const float* up = A.consts8 + nm::stage_b_off(8) + 256;                     // the four rows' units
            const int64_t i = row0 + s;
            if (g == 0 && i < a.n)
                reinterpret_cast<float4*>(a.out)[sample_record(a, i)] = make_float4(fo[0] * up[0], fo[1] * up[1], fo[2] * up[2], fo[3] * up[3] * a.sigma_scale);
            R.off = (block_steps(0) + block_steps(1)) * nm::kStepBytes;                 // blocks 0 and 1 of the next tile are in flight: block 2 is next
            continue;
        }
        if (MODE == TRUNK && a.sigma_only == 3) {
            // ---------------- the trunk's end: the alpha row, and the live samples' activations to the colour head's list
            i32x16 t;
            f32x16 fa;
            k_i8<8>(t, X, ring_enter(R, 68), R);
            dequant16(fa, t, sx * (256.f * kappa[8]), bias + nm::stage_b_off(8) + 256);
            const float sigma = fa[0] * u_sigma;
            const float v = sigma * a.sigma_scale;                                      // (row 0 of the block: the g == 0 lane of a sample has it)
            const int64_t i = row0 + s;
            const int64_t rec = g == 0 && i < a.n ? sample_record(a, i) : 0;          // the sample's record in `out`: what the head's list carries
            if (g == 0 && i < a.n) reinterpret_cast<float4*>(a.out)[rec] = make_float4(0.f, 0.f, 0.f, v);
            const unsigned live = (unsigned)__builtin_amdgcn_ballot_w64(g == 0 && i < a.n && !(v <= 0.f));      // bit s: sample s (a NaN is live)
            if (live) {
                int base = 0;
                if (lane == 0) base = atomicAdd(A.live.count, __builtin_popcount(live));
                base = __builtin_amdgcn_readfirstlane(base);
                if ((live >> s) & 1) {
                    const int64_t e = base + __builtin_popcount(live & ((1u << s) - 1u));
                    uint4* dst = A.live.x + g * A.live.cap + e;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        dst[(4 * k) * A.live.cap] = X.h[k];
                        dst[(4 * k + 2) * A.live.cap] = X.l[k];
                    }
                    if (g == 0) { A.live.sx[e] = sx; A.live.idx[e] = (int)rec; }
                }
            }
            // (the list stores, up to 19 per lane, and the atomic queue up BEHIND the copies of the next tile's blocks 0 and 1; the counted wait of the next
            // ring_enter(R, 0) is right only because fill_pe_wave's sample loads at the top of the next tile wait vmcnt(0) first -- as the atomic's
            // return and the exit's scratch reloads already do here: every tile's exit drains the ring's copies in flight, once per tile)
            R.off = (block_steps(0) + block_steps(1)) * nm::kStepBytes;
            continue;
        }
        // ---------------- stage 8: alpha (row 0 of its block; first in the stream) + feature (linear, 256)
        float sigma;
        {
            const float sxin = sx * (256.f * kappa[8]);
            {
                i32x16 t;
                f32x16 fa;
                k_i8<8>(t, X, ring_enter(R, 68), R);
                dequant16(fa, t, sxin, bias + nm::stage_b_off(8) + 256);
                sigma = fa[0] * u_sigma;
            }
            f32x16 f[8];
            float m = 0.f;
#pragma unroll
            for (int b = 0; b < 8; ++b) {                                               // (the riding dequantisation measured no gain here)
                i32x16 t;
                k_i8<8>(t, X, ring_enter(R, 69 + b), R);
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
                const uint4* ws = ring_enter(R, 77 + b);
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
        // ---------------- stage 10: rgb (rows 0..2 of one block), K = 128
        {
            i32x16 t;
            f32x16 fr;
            k_i8<4>(t, X, ring_enter(R, 81), R);
            dequant16(fr, t, sx * (256.f * kappa[10]), bias + nm::stage_b_off(10));
            const int64_t i = row0 + s;
            if (g == 0 && i < a.n)
                reinterpret_cast<float4*>(a.out)[sample_record(a, i)] =
                    make_float4(fr[0] * u_r, fr[1] * u_g, fr[2] * u_b,
                                sigma * a.sigma_scale);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                    // the copy started for a tile that never comes
}

}  // namespace

namespace nm {

int launch_mlp_i8s(const MlpLaunch& L, const void* image8, const float* pts, const float* dirs, const float* origin, const float* direction,
                   const float* z, int64_t n, int S, int in_mode, float sigma_scale, float* out, hipStream_t stream, const MlpChunk* chunk, const LiveList* live) {
    Args8s A;
    MlpArgs& a = A.a;
    a.ray_idx = chunk ? chunk->ray_idx : nullptr;
    a.n_rays_dev = chunk ? chunk->n_rays_dev : nullptr;
    a.s0 = chunk ? chunk->s0 : 0;
    a.S_total = chunk ? chunk->S_total : S;
    a.wpack = nullptr; a.bias = nullptr;
    a.petab = L.petab;
    a.pts = pts; a.dirs = dirs; a.origin = origin; a.direction = direction; a.z = z;
    a.out = out; a.dbg = nullptr; a.prof = nullptr; a.n = n; a.S = S; a.in_mode = in_mode; a.stop_stage = -2; a.sigma_scale = sigma_scale;
    a.sigma_only = L.plain_head ? 2 : live ? 3 : 0;                                     // (PLAIN's and TRUNK's exit after block 68)
    a.save_h = nullptr; a.save_hv = nullptr; a.save_bits = nullptr; a.save_h16 = nullptr; a.save_feat16 = nullptr; a.save_hvbits = nullptr; a.save_x0h = nullptr; a.save_d0h = nullptr;
    a.pos = PeSpec{L.pe_kind, L.pos_nfreq, L.pos_octaves};
    a.dir = PeSpec{L.pe_kind, L.dir_nfreq, L.dir_octaves};
    A.consts8 = L.consts8;
    A.image8 = reinterpret_cast<const uint4*>(image8);
    A.live = live ? *live : LiveList{nullptr, nullptr, nullptr, nullptr, 0};
    const int64_t ntiles = (n + kTile - 1) / kTile;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    const int grid = (int)(ntiles < cus ? ntiles : cus);
    if (L.plain_head) hipLaunchKernelGGL(nerf_mlp_i8s_kernel<PLAIN>, dim3(grid), dim3(kWaves * 64), 0, stream, A);
    else if (live) hipLaunchKernelGGL(nerf_mlp_i8s_kernel<TRUNK>, dim3(grid), dim3(kWaves * 64), 0, stream, A);
    else hipLaunchKernelGGL(nerf_mlp_i8s_kernel<WHOLE>, dim3(grid), dim3(kWaves * 64), 0, stream, A);
    return check_launch("nerf_mlp_i8s_kernel");
}

}  // namespace nm
