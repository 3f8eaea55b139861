// Shared device helpers of the activation-stationary i8x3 kernels (mlp_i8s.hip and its colour-head companion mlp_i8h.hip: 8 waves x 32 samples; round 4's mlp_i8t.hip, removed in round 5: 4 waves x two
// 32-sample sub-tiles): encodings of a wave's rows, the resident activation fragments, LDS-DMA, de- and requantisation -- one definition,
// so that the kernels run the same arithmetic instruction for instruction (they must agree bit for bit).
#pragma once
#include "mlp_device.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef __attribute__((ext_vector_type(2))) short i16x2;
typedef __attribute__((address_space(3))) const float lds_cfloat;      // (an LDS address is 32 bits and fits a ds_read's base register)
typedef __attribute__((ext_vector_type(4))) float vf4;
typedef __attribute__((address_space(3))) const vf4 lds_cvf4;

constexpr int kRows = 32;                                    // samples of one MFMA column block = of one (sub-)tile of a wave
struct Args8s {
    MlpArgs a;
    const float* consts8;      // units (kBiasFloats) | biases in those units (kBiasFloats) | kappa (16)
    const uint4* image8;       // the stream (mlp_host.hip pack_stream8s): [ring block][step][hi | lo][64 lanes][16 B] in block_steps() order
    nm::LiveList live;         // the trunk / colour-head pair only (mlp_launch.h)
};

__device__ __forceinline__ i32x4 as_i32x4(uint4 v) { return __builtin_bit_cast(i32x4, v); }

// ---- encodings of this wave's 32 rows (octave recurrence, mlp_device.h fill_pe_fast, wave-private layout)
//   F16: the NM_PREC_FP16X3 form (fp16 parts of 32 v; the general path clamps like split8<false, true>, the octave path has |v| <= max(1, |x|))
template <bool F16 = false>
__device__ __forceinline__ void fill_pe_wave(uint4* pw, bool is_dir, const MlpArgs& a, int64_t base_row, int lane) {
    const PeSpec spec = is_dir ? a.dir : a.pos;
    const float* tab = a.petab + (is_dir ? 96 : 0);
    unsigned short* hi = reinterpret_cast<unsigned short*>(pw);
    auto put = [&](int row, int p, float v, bool clamp = false) {
        const int off = ((p >> 3) * (2 * kRows) + row) * 8 + (p & 7);
        if (F16) {
            float sv = v * kF16ActScale;
            if (clamp) sv = __builtin_amdgcn_fmed3f(sv, -65504.f, 65504.f);
            const _Float16 hb = (_Float16)sv;
            const _Float16 lb = (_Float16)(sv - (float)hb);
            hi[off] = __builtin_bit_cast(unsigned short, hb);
            hi[off + kRows * 8] = __builtin_bit_cast(unsigned short, lb);
            return;
        }
        const bf16x2 hb = __builtin_convertvector((f32x2){v, 0.f}, bf16x2);
        const f32x2 hf = __builtin_convertvector(hb, f32x2);
        const bf16x2 lb = __builtin_convertvector((f32x2){v - hf.x, 0.f}, bf16x2);
        hi[off] = (unsigned short)(__builtin_bit_cast(unsigned, hb) & 0xffffu);
        hi[off + kRows * 8] = (unsigned short)(__builtin_bit_cast(unsigned, lb) & 0xffffu);
    };
    if (spec.octaves) {
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {
            const int j = 2 * round + (lane >> 5), row = lane & 31;
            if (j > 2) break;
            int64_t i = base_row + row;
            if (i >= a.n) i = a.n - 1;
            float x0, x1, x2;
            sample_input(a, i, is_dir, x0, x1, x2);
            const float xj = j == 0 ? x0 : (j == 1 ? x1 : x2);
            const float a0 = spec.kind == NM_PE_POSENC ? xj * tab[0] : fmaf(x2, tab[3 * j + 2], fmaf(x1, tab[3 * j + 1], x0 * tab[3 * j]));
            put(row, j, xj);
            double sn, cs;
            sincos_f64((double)a0, sn, cs);
            const int n3 = 3 * spec.nfreq;
            for (int b = 0; b < spec.nfreq; ++b) {
                if (spec.kind == NM_PE_POSENC) { put(row, 3 + 6 * b + j, (float)sn); put(row, 3 + 6 * b + 3 + j, (float)cs); }
                else { put(row, 3 + 3 * b + j, (float)sn); put(row, 3 + n3 + 3 * b + j, (float)cs); }
                const double s2 = 2.0 * sn * cs, c2 = 1.0 - 2.0 * sn * sn;
                sn = s2; cs = c2;
            }
        }
    } else {
        const int nchunks = is_dir ? 4 : nm::kPeChunks;
        for (int item = lane; item < nchunks * kRows; item += 64) {
            const int c = item >> 5, row = item & 31;
            int64_t i = base_row + row;
            if (i >= a.n) i = a.n - 1;
            float x0, x1, x2;
            sample_input(a, i, is_dir, x0, x1, x2);
#pragma unroll
            for (int e = 0; e < 8; ++e) put(row, 8 * c + e, pe_feature(8 * c + e, x0, x1, x2, spec, tab), true);
        }
    }
}

struct X8 {
    uint4 h[8], l[8];          // the wave's activations: k-step t = feature block t of the producing stage, hi / lo limbs
};

__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// (bias_blk: the block's 32 biases + 4 * g, this lane's half of every group of 8)
__device__ __forceinline__ void bias16(f32x16& f, lds_cfloat* bias_blk) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const vf4 bs = *(lds_cvf4*)(bias_blk + 8 * q);
        f[4 * q] = bs.x; f[4 * q + 1] = bs.y; f[4 * q + 2] = bs.z; f[4 * q + 3] = bs.w;
    }
}
__device__ __forceinline__ void dequant16(f32x16& f, const i32x16& t, float sx256, lds_cfloat* bias_blk) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const vf4 bs = *(lds_cvf4*)(bias_blk + 8 * q);
        const float bsv[4] = {bs.x, bs.y, bs.z, bs.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) f[4 * q + j] = fmaf((float)t[4 * q + j], sx256, bsv[j]);
    }
}
template <bool RELU>
__device__ __forceinline__ float max16(float m, const f32x16& f) {
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, RELU ? f[r] : fabsf(f[r]));
    return m;
}
__device__ __forceinline__ float row_max(float m) {                  // the two lane halves of a sample hold different features
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    const u32x2 sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    return fmaxf(__uint_as_float(sw.x), __uint_as_float(sw.y));
}
// one block's 16 outputs of this lane -> the next stage's k-step fragment (two balanced int8 limbs); nerf_mlp_i8w_kernel's quant_storew
template <bool RELU>
__device__ __forceinline__ void quant16(const f32x16& f, float inv, uint4& xh, uint4& xl) {
    i16x2 P[8], Y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float y0 = f[2 * i] * inv, y1 = f[2 * i + 1] * inv;
        if (RELU) {
            y0 = __builtin_amdgcn_fmed3f(y0, 0.f, 1.f);
            y1 = __builtin_amdgcn_fmed3f(y1, 0.f, 1.f);
        }
        const i16x2 p = __builtin_amdgcn_cvt_pknorm_i16(y0, y1);
        P[i] = p;
        Y[i] = p + (i16x2){128, 128};
    }
    unsigned lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo[k] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, P[2 * k + 1]), __builtin_bit_cast(unsigned, P[2 * k]), 0x06040200u);
        hi[k] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, Y[2 * k + 1]), __builtin_bit_cast(unsigned, Y[2 * k]), 0x07050301u);
    }
    xh = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    xl = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}
__device__ __forceinline__ float inv_of(float M) { return M > 0.f ? ((float)nm::kFixedMax / 32767.f) * __builtin_amdgcn_rcpf(M) : 0.f; }
__device__ __forceinline__ float scale_of(float M) { return M > 0.f ? M * (1.f / (float)nm::kFixedMax) : 1.f; }

// ---- the workgroup shape, its LDS plan and the weight ring shared by the kernels built on these helpers (mlp_i8s.hip, mlp_i8h.hip)
constexpr int kWaves = 8;                        // 8 waves x 32 samples = 256 samples per workgroup, one workgroup per CU
constexpr int kTile = kWaves * kRows;
// LDS: the encodings of each wave's 32 rows, wave-private: [wave][8 chunks][hi: 32 rows | lo: 32 rows][16 B] = 8 KB per wave
constexpr int kPWaveU4 = nm::kPeChunks * 2 * kRows;          // 512 uint4
constexpr int kPeU4 = kWaves * kPWaveU4;
// the weight ring: kSlots slots of one ring block (at most 10 k-steps of 2 KB; sized for 12)
constexpr int kStepU4 = nm::kStepBytes / 16;
constexpr int kSlotU4 = 12 * kStepU4;
constexpr int kSlots = 3;                                    // the block being multiplied + two being copied
constexpr int kBiasU4 = (nm::kBiasFloats + 16 + 3) / 4;      // the bias table and kappa, resident in LDS (a global load per block would sit in the same
                                                             // in-order VMEM queue as the copies and force them to land early)
__host__ __device__ constexpr int block_pieces(int nsteps) { return (2 * nsteps + kWaves - 1) / kWaves; }   // 1 KB pieces per wave

// ---- the weight ring.  Producer side: every wave copies its share (1 KB pieces i = w, w + 8, ..) of the block TWO ahead; consumer side:
// all waves read every fragment of the current block.  Hand-over, once per block: each wave waits until its own pieces of the block it is
// about to enter have landed (counted vmcnt: the pieces of the block after it stay in flight -- issue to landing is about 1 us, longer
// than a block), then the barrier makes everybody's pieces visible and proves that nobody still reads the slot that is refilled next.
// The only other VMEM operations of nerf_mlp_i8s_kernel<WHOLE / PLAIN> are the sample loads at the top of a tile and the 16-byte store at its end (the
// compiler waits vmcnt(0) for the former: two copies land early, once per tile).  <TRUNK> adds its list stores and one returning atomic at the end of
// a tile, the head kernel its list loads at the top and three 4-byte stores at the end: extra operations in the queue only make a counted wait
// stricter (the ring's pieces stay in order among themselves), and each of these tiles still begins with loads the compiler waits vmcnt(0) for.
// S: the stream being walked -- S::steps(i), the k-steps of its flat block i (i up to two past the end: the look-ahead), and S::kBytes,
// where it wraps
template <class S>
struct RingT {
    const char* src;           // image + lane * 16 + w * 1024
    const uint4* rd;           // ring + lane
    unsigned lds0;             // LDS byte address of slot 0 + w * 1024
    int off;                   // image offset of the block to copy next
    int slot;                  // slot of the block to enter next
    int refill, np, nsteps2;   // the copy in progress: slot, pieces per wave, k-steps of the block
};
// this wave's piece j of the block at R.off -> slot (a 10-step block is padded to 3 pieces: the excess lands in the unused tail of the slot)
template <class S>
__device__ __forceinline__ void ring_piece(const RingT<S>& R, int off, int slot, int j) {
    glds16(R.src + off + j * (kWaves * 1024), __builtin_amdgcn_readfirstlane(R.lds0 + slot * (kSlotU4 * 16) + j * (kWaves * 1024)));
}
template <class S>
__device__ __forceinline__ void ring_advance(RingT<S>& R, int nsteps) {
    R.off += nsteps * nm::kStepBytes;
    if (R.off == S::kBytes) R.off = 0;
}
// enter flat block i of the tile; returns this lane's view of block i.  The copy of block i + 2 (into the slot block i - 1 has just given
// up) is issued from inside the k-loop (ring_copy after k-steps 0, 2, 4): the texture path takes one 1 KB piece at a time, and eight
// waves issuing theirs right after the barrier would all start their MFMAs late.
template <class S>
__device__ __forceinline__ const uint4* ring_enter(RingT<S>& R, int i) {
    const int np1 = block_pieces(S::steps(i + 1));
    if (np1 == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if (np1 == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const uint4* cur = R.rd + R.slot * kSlotU4;
    R.refill = R.slot == 0 ? kSlots - 1 : R.slot - 1;                  // the slot of block i - 1 = of block i + 2
    R.slot = R.slot == kSlots - 1 ? 0 : R.slot + 1;
    R.np = block_pieces(S::steps(i + 2));
    R.nsteps2 = S::steps(i + 2);
    return cur;
}
template <class S>
__device__ __forceinline__ void ring_copy(RingT<S>& R, int j) {
    if (j < R.np) ring_piece(R, R.off, R.refill, j);
    if (j == R.np - 1) ring_advance(R, R.nsteps2);
}
struct W8 {
    uint4 h, l;
};

// NSTEPS limb k-steps of one output block: t = 256 * sum(hi.hi) + sum(hi.lo + lo.hi), exact, in two int32 accumulators (two dependency
// chains; every weight fragment read from LDS once).  Between the k-steps rides the dequantisation of the PREVIOUS block (PEND), two
// values per step: in lock-step with its SIMD partner a wave would otherwise do it while nobody uses the matrix pipe.
// PEND: fp = the previous block's outputs (written here, two per MFMA of the first pass), tp = its accumulators, bias_blk = its biases
// (this lane's half of every group of 8), m = the running row maximum
template <int NSTEPS, bool PEND, bool RELU = true, class Ring>
__device__ __forceinline__ void k_i8_impl(i32x16& t, const X8& X, const uint4* ws, Ring& R, f32x16& fp, const i32x16& tp, lds_cfloat* bias_blk,
                                          float sx256, float& m) {
    i32x16 ah, ac;
#pragma unroll
    for (int r = 0; r < 16; ++r) { ah[r] = 0; ac[r] = 0; }
    W8 w[2];
    w[0].h = ws[0]; w[0].l = ws[64];
    w[1].h = ws[kStepU4]; w[1].l = ws[kStepU4 + 64];
#pragma unroll
    for (int s = 0; s < NSTEPS; ++s) {
        const uint4 wh = w[s & 1].h, wl = w[s & 1].l;
        ac = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_i32x4(wh), as_i32x4(X.l[s]), ac, 0, 0, 0);
        ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_i32x4(wh), as_i32x4(X.h[s]), ah, 0, 0, 0);      // (between the two links of the cross-term
        ac = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_i32x4(wl), as_i32x4(X.h[s]), ac, 0, 0, 0);      // chain: -2.5 % at steady state)
        if (s + 2 < NSTEPS) { w[s & 1].h = ws[(s + 2) * kStepU4]; w[s & 1].l = ws[(s + 2) * kStepU4 + 64]; }
        if (s == 0 || s == 2 || s == 4) ring_copy(R, s >> 1);
        if (PEND) {
            const int r = 2 * s;
            const float b0 = bias_blk[8 * (r >> 2) + (r & 3)], b1 = bias_blk[8 * (r >> 2) + (r & 3) + 1];
            const float f0 = fmaf((float)tp[r], sx256, b0), f1 = fmaf((float)tp[r + 1], sx256, b1);
            fp[r] = f0;
            fp[r + 1] = f1;
            m = RELU ? fmaxf(m, fmaxf(f0, f1)) : fmaxf(m, fmaxf(fabsf(f0), fabsf(f1)));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = (ah[r] << 8) + ac[r];
}
template <int NSTEPS, class Ring>
__device__ __forceinline__ void k_i8(i32x16& t, const X8& X, const uint4* ws, Ring& R) {
    f32x16 nf;
    float nm_ = 0.f;
    k_i8_impl<NSTEPS, false>(t, X, ws, R, nf, t, nullptr, 0.f, nm_);
}
struct NoRing {};
__device__ __forceinline__ void ring_copy(NoRing&, int) {}
// The wave's own encoding fragments of NSTEPS k-steps (chunks 2 t + g of its rows in pw), hi / lo parts.  They depend on the lane and the k-step only,
// not on the output block: a stage reads them ONCE, in front of its first block, and every block's k_bf takes them from registers (read inside k_bf
// they were read again per block -- the ring's barriers keep the compiler from merging the reads -- 8 times in stage 0 and in the skip).
// pw was written by this wave's fill_pe_wave: a wave's LDS operations execute in order, and the compiler may not lift these reads over those writes.
template <int NSTEPS>
struct Enc {
    uint4 h[NSTEPS], l[NSTEPS];
};
template <int NSTEPS>
__device__ __forceinline__ void load_enc(Enc<NSTEPS>& E, const uint4* pw, int g, int s) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int t = 0; t < NSTEPS; ++t) {
        E.h[t] = pw[(2 * t + g) * (2 * kRows) + s];
        E.l[t] = pw[(2 * t + g) * (2 * kRows) + kRows + s];
    }
}
// NSTEPS split-bf16 k-steps over the wave's encoding rows, accumulated into f
template <int NSTEPS, bool COPY = false, class Ring = NoRing>
__device__ __forceinline__ void k_bf(f32x16& f, const Enc<NSTEPS>& E, const uint4* ws, Ring* R = nullptr, int j0 = 0) {
#pragma unroll
    for (int t = 0; t < NSTEPS; ++t) {
        if (COPY && (t == 1 || t == 3)) ring_copy(*R, j0 + (t >> 1));
        const uint4 wh = ws[t * kStepU4], wl = ws[t * kStepU4 + 64];
        f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(wh), as_bf16x8(E.l[t]), f, 0, 0, 0);
        f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(wl), as_bf16x8(E.h[t]), f, 0, 0, 0);
        f = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(wh), as_bf16x8(E.h[t]), f, 0, 0, 0);
    }
}

}  // namespace
