// NM_PREC_I8X3, the trunk / colour-head pair of nm_mlp_forward_rays_live (mlp_i8s.hip TRUNK, mlp_i8h.hip) as ONE persistent launch: every workgroup
// shades its own live samples right behind its own trunk tiles.  Same workgroup shape, ring, helpers and LDS plan (mlp_i8as.h); the two tile bodies are
// those kernels', operation for operation, so every record in `out` is bit-identical to the pair's and to the whole-network launch's.
//
//   * Trunk tiles are split statically (tile = blockIdx.x; tile += gridDim.x).  A trunk tile appends its live samples (stored density not <= 0) to a list
//     PRIVATE to the workgroup: kFusedEntries = 768 entries in the pair's [piece][lane half][entry][16 B] layout plus sx and idx, used as a ring.  The
//     number appended so far lives in LDS (one ballot, one LDS atomic add and a prefix count per wave: the return comes back on lgkmcnt, no global
//     atomic, no counter reset, nothing another workgroup ever sees); the number consumed is the same in every wave's registers.
//   * A head tile takes the 256 oldest entries (a multiple of 256 has been consumed before it: its entries never wrap), the last one of a workgroup
//     whatever is left (1..255 entries, clamped as nerf_head_i8s_kernel clamps).  Each entry takes its direction encoding from its own ray (in_mode 3).
//   * What the NEXT tile is must be known before the tile in hand has counted its live samples: the ring copies the next tile's blocks 0 and 1 under
//     the last two blocks of this one.  So it is decided at the top of a tile from what is known there, q = the entries pending, less the 256 a head tile
//     is about to take: a head tile if q >= 256, else the next trunk tile, else (no trunk tile left) a head tile for the remainder -- which is
//     not run if nothing is pending by then.  A trunk tile therefore starts with fewer than 512 entries pending and ends with fewer than 768: the ring.
//     Head tiles of 256 entries run while 256 are pending, whatever the order: a workgroup that lists L samples runs ceil(L / 256) head tiles.
//   * Both stream cuts (mlp_host.hip pack_stream8s_live: trunk | head in one allocation) end in two look-ahead pieces of 8 k-steps: the trunk's tail
//     holds a trunk tile's blocks 0 and 1 padded to 8 steps, the head's blocks 0 and 1 ARE 8 steps.  The ring's copy offset, on reaching the end of the
//     tile in hand (R.edge), goes on at R.next = the one or the other: trunk -> trunk, trunk -> head, head -> head, head -> trunk.
//   * No workgroup waits for another: the only synchronisation is the workgroup barrier.  The entry stores of a trunk tile are handed to the waves that
//     load them in a head tile by a workgroup-scope release / acquire pair around the barrier at the top of every tile.
// Record: profiles/live_fused.md, profiles/i8_encoding_regs.md; DESIGN.md "K4-i8s".
//
// Reference semantics: models/vanilla.py Embedder.forward (:82-92), NeRF.forward (:120-152), Joiner.forward (:162-166).
#include "mlp_i8as.h"

namespace {

constexpr int kTrunkSteps = 8 * 4 + 7 * 8 * 8 + 8 * 4 + 8;   // 520: ring blocks 0..68 of nerf_mlp_i8s_kernel's tile
constexpr int kHeadSteps = 8 * 8 + 4 * 10 + 4;                // 108: blocks 69..81
struct TrunkStream {                                         // blocks 0..68, then the two look-ahead pieces
    static __host__ __device__ constexpr int steps(int i) { return i < 8 ? 4 : 8; }
};
struct HeadStream {                                          // blocks 0..12, then the two look-ahead pieces (its own blocks 0 and 1 as to length)
    static __host__ __device__ constexpr int steps(int i) {
        i = i >= 13 ? i - 13 : i;
        return i < 8 ? 8 : i < 12 ? 10 : 4;
    }
};

struct ArgsF {
    MlpArgs a;                 // the ray form (in_mode 1)
    const float* consts8;
    const char* image;         // the trunk cut, and at head_off the head cut
    int head_off;
    char* list;                // [workgroup] private lists of nm::kFusedListBytes
    int* tiles;                // [workgroup][2] the trunk and the head tiles it ran
};

// RingT (mlp_i8as.h) over two streams: the stream is a template argument of ring_enter, not of the ring, and the copy offset jumps from `edge` to `next`
struct RingF {
    const char* src;
    const uint4* rd;
    unsigned lds0;
    int off, slot;
    int refill, np, nsteps2;
    int edge, next;
};
__device__ __forceinline__ void ring_piece(const RingF& R, int off, int slot, int j) {
    glds16(R.src + off + j * (kWaves * 1024), __builtin_amdgcn_readfirstlane(R.lds0 + slot * (kSlotU4 * 16) + j * (kWaves * 1024)));
}
template <class S>
__device__ __forceinline__ const uint4* ring_enter_f(RingF& R, int i) {
    const int np1 = block_pieces(S::steps(i + 1));
    if (np1 == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if (np1 == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const uint4* cur = R.rd + R.slot * kSlotU4;
    R.refill = R.slot == 0 ? kSlots - 1 : R.slot - 1;
    R.slot = R.slot == kSlots - 1 ? 0 : R.slot + 1;
    R.np = block_pieces(S::steps(i + 2));
    R.nsteps2 = S::steps(i + 2);
    return cur;
}
__device__ __forceinline__ void ring_copy(RingF& R, int j) {
    if (j < R.np) ring_piece(R, R.off, R.refill, j);
    if (j == R.np - 1) {
        R.off += R.nsteps2 * nm::kStepBytes;
        if (R.off == R.edge) R.off = R.next;
    }
}

__global__ __launch_bounds__(kWaves * 64, 2) void nerf_mlp_i8s_fused_kernel(const ArgsF A) {
    __shared__ uint4 lds[kPeU4 + kSlots * kSlotU4 + kBiasU4];
    __shared__ float units[4];                                                          // of sigma, r, g, b
    __shared__ unsigned appended;                                                       // entries this workgroup has listed so far
    const MlpArgs a = A.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, s = lane & 31;
    uint4* pw = lds + w * kPWaveU4;
    RingF R;
    R.src = A.image + lane * 16 + w * 1024;
    R.rd = lds + kPeU4 + lane;
    R.lds0 = (unsigned)(uintptr_t)(lds + kPeU4) + w * 1024;
    R.slot = 0;
    {                                                                                   // the bias table
        float* lb = reinterpret_cast<float*>(lds + kPeU4 + kSlots * kSlotU4);
        for (int i = tid; i < nm::kBiasFloats + 16; i += kWaves * 64) lb[i] = A.consts8[nm::kBiasFloats + i];
    }
    if (tid == 0) appended = 0;
    if (tid < 4) units[tid] = A.consts8[tid == 0 ? nm::stage_b_off(8) + 256 : nm::stage_b_off(10) + tid - 1];
    __syncthreads();
    ring_piece(R, 0, 0, 0);                                                             // blocks 0 and 1 of the first trunk tile (one piece each)
    ring_piece(R, 4 * nm::kStepBytes, 1, 0);
    const float* kappa = reinterpret_cast<const float*>(lds + kPeU4 + kSlots * kSlotU4) + nm::kBiasFloats;
    unsigned bias_lds = (unsigned)(uintptr_t)(lds + kPeU4 + kSlots * kSlotU4) + 16 * g;        // this lane's half of every group of 8
    asm volatile("" : "+v"(bias_lds));
    lds_cfloat* bias = (lds_cfloat*)(uintptr_t)bias_lds;
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    for (int i = lane; i < kPWaveU4; i += 64) pw[i] = make_uint4(0, 0, 0, 0);          // pad slots: finite once
    // this workgroup's list
    char* const mine = A.list + (int64_t)blockIdx.x * nm::kFusedListBytes;
    uint4* const lx = reinterpret_cast<uint4*>(mine);
    float* const lsx = reinterpret_cast<float*>(mine + nm::kFusedEntries * 512);
    int* const lidx = reinterpret_cast<int*>(mine + nm::kFusedEntries * 516);

    int64_t tile = blockIdx.x;                                                          // the next trunk tile (the grid is at most ntiles: there is one)
    unsigned consumed = 0;
    int head = 0, ntrunk = 0, nhead = 0;                                                // head: the tile in hand is a head tile
#pragma unroll 1
    for (;;) {
        // the hand-over of the list: entries stored under the last tile are visible to every wave of the workgroup from here on
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // (read between this barrier and the tile's first ring barrier; the next additions come after the tile's last ring barrier)
        const unsigned pending = (unsigned)__builtin_amdgcn_readfirstlane(__hip_atomic_load(&appended, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) - consumed;
        if (head && pending == 0) break;                                                // (only after the last trunk tile)
        const unsigned ntake = head ? (pending < (unsigned)kTile ? pending : (unsigned)kTile) : 0u;
        const bool more = (head ? tile : tile + gridDim.x) < ntiles;                    // a trunk tile is left after this one
        const int next_head = pending - ntake >= (unsigned)kTile || !more;
        R.off = head ? A.head_off + 16 * nm::kStepBytes : 8 * nm::kStepBytes;           // blocks 0 and 1 are in flight: block 2 is next
        R.edge = head ? A.head_off + kHeadSteps * nm::kStepBytes : kTrunkSteps * nm::kStepBytes;
        R.next = next_head ? A.head_off : kTrunkSteps * nm::kStepBytes;
        asm volatile("" : "+s"(R.off), "+s"(R.edge), "+s"(R.next));                     // (constants would become one copy address per piece, kept across tiles)
        if (!head) {
            // ================ a trunk tile: nerf_mlp_i8s_kernel<TRUNK>'s, the list apart
            const int64_t row0 = tile * kTile + w * kRows;                              // this wave's first sample (rows past n: clamped)
            fill_pe_wave(pw, false, a, row0, lane);
            X8 X;
            float sx;
            // ---------------- stage 0: encodings only (split bf16), ReLU
            {
                f32x16 f[8];
                float m = 0.f;
                Enc<4> E;
                load_enc(E, pw, g, s);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const uint4* ws = ring_enter_f<TrunkStream>(R, b);
                    bias16(f[b], bias + nm::stage_b_off(0) + 32 * b);
                    k_bf<4, true>(f[b], E, ws, &R);
                    m = max16<true>(m, f[b]);
                }
                const float M = row_max(m), inv = inv_of(M);
#pragma unroll
                for (int b = 0; b < 8; ++b) quant16<true>(f[b], inv, X.h[b], X.l[b]);
                sx = scale_of(M);
            }
            // ---------------- stages 1..7: 256 -> 256, ReLU; stage 5 adds the position encoding
#pragma unroll 1
            for (int st = 1; st <= 7; ++st) {
                const float sxin = sx * (256.f * kappa[st]);
                const int i0 = 8 * st + (st > 5 ? 4 : 0);
                f32x16 f[8];
                float m = 0.f;
                i32x16 tp;
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const uint4* ws = ring_enter_f<TrunkStream>(R, i0 + b);
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
                        const uint4* ws = ring_enter_f<TrunkStream>(R, 48 + u);
                        k_bf<4, true>(f[2 * u], E, ws, &R, 0);
                        k_bf<4, true>(f[2 * u + 1], E, ws + 4 * kStepU4, &R, 2);
                    }
                    m = 0.f;
#pragma unroll
                    for (int b = 0; b < 7; ++b) m = max16<true>(m, f[b]);
                }
                m = max16<true>(m, f[7]);
                const float M = row_max(m), inv = inv_of(M);
#pragma unroll
                for (int b = 0; b < 8; ++b) quant16<true>(f[b], inv, X.h[b], X.l[b]);
                sx = scale_of(M);
            }
            // ---------------- the alpha row, and the live samples' activations to this workgroup's list
            {
                i32x16 t;
                f32x16 fa;
                k_i8<8>(t, X, ring_enter_f<TrunkStream>(R, 68), R);
                dequant16(fa, t, sx * (256.f * kappa[8]), bias + nm::stage_b_off(8) + 256);
                const float sigma = fa[0] * units[0];                                    // (the output units are read from LDS where they are used: held in
                                                                                        // registers across a tile they are spilled, and a reload waits vmcnt(0))
                const float v = sigma * a.sigma_scale;
                int sb = s, gb = g;                                                     // (likewise the lane's bit masks and its list address)
                asm volatile("" : "+v"(sb), "+v"(gb));
                const int64_t i = row0 + s;
                if (g == 0 && i < a.n) reinterpret_cast<float4*>(a.out)[i] = make_float4(0.f, 0.f, 0.f, v);
                const unsigned live = (unsigned)__builtin_amdgcn_ballot_w64(g == 0 && i < a.n && !(v <= 0.f));      // bit s: sample s (a NaN is live)
                if (live) {
                    unsigned base = 0;
                    if (lane == 0) base = __hip_atomic_fetch_add(&appended, (unsigned)__builtin_popcount(live), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    base = (unsigned)__builtin_amdgcn_readfirstlane(base);
                    if ((live >> sb) & 1) {
                        const unsigned e = (base + __builtin_popcount(live & ((1u << sb) - 1u))) % (unsigned)nm::kFusedEntries;
                        uint4* dst = lx + gb * nm::kFusedEntries + e;
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            dst[(4 * k) * nm::kFusedEntries] = X.h[k];
                            dst[(4 * k + 2) * nm::kFusedEntries] = X.l[k];
                        }
                        if (g == 0) { lsx[e] = sx; lidx[e] = (int)i; }
                    }
                }
            }
            tile += gridDim.x;
            ++ntrunk;
        } else {
            // ================ a head tile: nerf_head_i8s_kernel's, on entries [consumed, consumed + ntake) of this workgroup's list
            const unsigned e0 = consumed % (unsigned)nm::kFusedEntries;                 // (a multiple of 256: the tile's entries do not wrap)
            MlpArgs ah = a;                                                             // in_mode 3 over the tile's entries
            ah.in_mode = 3;
            ah.ray_idx = lidx + e0;
            ah.n = ntake;
            ah.s0 = 0;
            ah.S_total = a.S;
            const int64_t row0 = w * kRows;
            int e = w * kRows + s;
            const bool listed = e < (int)ntake;
            if (!listed) e = (int)ntake - 1;
            X8 X;
            {
                const uint4* src = lx + g * nm::kFusedEntries + e0 + e;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    X.h[k] = src[(4 * k) * nm::kFusedEntries];
                    X.l[k] = src[(4 * k + 2) * nm::kFusedEntries];
                }
            }
            float sx = lsx[e0 + e];
            int rec = lidx[e0 + e];
            fill_pe_wave(pw, true, ah, row0, lane);                                     // the direction encoding of each entry's own ray
            asm volatile("" : "+v"(rec));                                               // (landed HERE, with the rest: read only under the store's mask at the tile's end, the
                                                                                        // load stays pending for the compiler on the path round it, into the next trunk tile,
                                                                                        // whose stage loop then waits vmcnt(0) -- for the ring's copies too -- once per stage)
            // ---------------- stage 8: feature (linear, 256)
            {
                const float sxin = sx * (256.f * kappa[8]);
                f32x16 f[8];
                float m = 0.f;
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    i32x16 t;
                    k_i8<8>(t, X, ring_enter_f<HeadStream>(R, b), R);
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
                    const uint4* ws = ring_enter_f<HeadStream>(R, 8 + b);
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
            // ---------------- stage 10: rgb (rows 0..2 of one block), K = 128; the density of the record is the trunk tile's
            {
                i32x16 t;
                f32x16 fr;
                k_i8<4>(t, X, ring_enter_f<HeadStream>(R, 12), R);
                dequant16(fr, t, sx * (256.f * kappa[10]), bias + nm::stage_b_off(10));
                if (g == 0 && listed) {
                    float* o = a.out + (int64_t)rec * 4;
                    o[0] = fr[0] * units[1]; o[1] = fr[1] * units[2]; o[2] = fr[2] * units[3];
                }
            }
            consumed += ntake;
            ++nhead;
        }
        head = next_head;
    }
    if (tid == 0) { A.tiles[2 * blockIdx.x] = ntrunk; A.tiles[2 * blockIdx.x + 1] = nhead; }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                    // the copies started for a tile that never comes
}

}  // namespace

namespace nm {

int launch_mlp_i8f(const MlpLaunch& L, const void* trunk8, int head_off, const float* origin, const float* direction, const float* z, int64_t n, int S,
                   float sigma_scale, float* out, void* workspace, hipStream_t stream) {
    ArgsF A;
    MlpArgs& a = A.a;
    a.ray_idx = nullptr; a.n_rays_dev = nullptr; a.s0 = 0; a.S_total = S;
    a.wpack = nullptr; a.bias = nullptr;
    a.petab = L.petab;
    a.pts = nullptr; a.dirs = nullptr; a.origin = origin; a.direction = direction; a.z = z;
    a.out = out; a.dbg = nullptr; a.prof = nullptr; a.n = n; a.S = S; a.in_mode = 1; a.stop_stage = -2; a.sigma_scale = sigma_scale;
    a.sigma_only = 0;
    a.save_h = nullptr; a.save_hv = nullptr; a.save_bits = nullptr; a.save_h16 = nullptr; a.save_feat16 = nullptr; a.save_hvbits = nullptr; a.save_x0h = nullptr; a.save_d0h = nullptr;
    a.pos = PeSpec{L.pe_kind, L.pos_nfreq, L.pos_octaves};
    a.dir = PeSpec{L.pe_kind, L.dir_nfreq, L.dir_octaves};
    A.consts8 = L.consts8;
    A.image = static_cast<const char*>(trunk8);
    A.head_off = head_off;
    const int64_t groups = fused_groups(n);                                             // what the workspace is sized for
    A.list = static_cast<char*>(workspace);
    A.tiles = reinterpret_cast<int*>(A.list + groups * kFusedListBytes);
    int dev = 0, cus = kFusedMaxGroups;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    const int grid = (int)(groups < cus ? groups : cus);
    hipLaunchKernelGGL(nerf_mlp_i8s_fused_kernel, dim3(grid), dim3(kWaves * 64), 0, stream, A);
    return check_launch("nerf_mlp_i8s_fused_kernel");
}

}  // namespace nm
