// One ray's alpha compositing (reference utils/render_utils.py:69-105) as device code shared by every kernel that composites: the kernels of
// ray_ops.hip and the wide merge of merge_wide.hip go through this one body, so they all produce the same bits.  Include after common.h
// (wave_sum); build with -ffp-contract=off like every file here.
#pragma once
#include "common.h"

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

struct CompositeSums {
    float r, g, b, d, a;
};
// One ray's compositing (render_utils.py:85-100), the wave's lanes across its S samples in chunks of 64.  raw_at(s) / z_at(s): the
// s-th record and depth of the list (global memory, or a merged list staged in LDS); w_out(s, w): called with every weight.  Every
// kernel that composites goes through this one body, so they all produce the same bits.
template <class RawAt, class ZAt, class WOut>
__device__ __forceinline__ CompositeSums composite_ray(int S, float dnorm, int lane, const float* noise_row, RawAt raw_at, ZAt z_at, WOut w_out) {
    double t_carry = 1.0;
    float sr = 0.f, sg = 0.f, sb = 0.f, sd = 0.f, sa = 0.f;
    for (int c0 = 0; c0 < S; c0 += 64) {
        const int s = c0 + lane;
        const bool valid = s < S;
        float w = 0.f, f = 1.f;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        float z = 0.f;
        if (valid) {
            q = raw_at(s);
            z = z_at(s);
            float dist = (s + 1 < S) ? (z_at(s + 1) - z) : 1e10f;       // render_utils.py:85-86
            dist = dist * dnorm;
            float sigma = q.w;
            if (noise_row) sigma = sigma + noise_row[s];               // render_utils.py:93-94
            const float alpha = 1.f - expf(-fmaxf(sigma, 0.f) * dist);  // render_utils.py:81
            w = alpha;
            f = 1.f - alpha + 1e-10f;                                   // render_utils.py:95
        }
        // transmittance: running product in f64, rounded to f32 per entry -- order independent, and what torch's
        // CPU cumprod computes for f32 inputs (the weights feed the inverse-CDF step function)
        double incl = (double)f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double t = __shfl_up(incl, o, 64);
            if (lane >= o) incl *= t;
        }
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0;
        w = w * (float)(t_carry * excl);
        t_carry = t_carry * __shfl(incl, 63, 64);
        if (valid) {
            w_out(s, w);
            sr += w * sigmoidf_(q.x);                                   // render_utils.py:90, 96
            sg += w * sigmoidf_(q.y);
            sb += w * sigmoidf_(q.z);
            sd += w * z;                                                // render_utils.py:98
            sa += w;                                                    // render_utils.py:100
        }
    }
    CompositeSums c;
    c.r = wave_sum(sr); c.g = wave_sum(sg); c.b = wave_sum(sb); c.d = wave_sum(sd); c.a = wave_sum(sa);
    return c;
}
__device__ __forceinline__ void composite_store(CompositeSums c, int white_bkg, int64_t r, float* rgb, float* disp, float* acc, float* depth) {
    if (white_bkg) {                                                    // render_utils.py:102-103
        const float bg = 1.f - c.a;
        c.r = c.r + bg; c.g = c.g + bg; c.b = c.b + bg;
    }
    rgb[r * 3 + 0] = c.r; rgb[r * 3 + 1] = c.g; rgb[r * 3 + 2] = c.b;
    depth[r] = c.d;
    acc[r] = c.a;
    if (disp) {
        const float q = c.d / c.a;                                      // NaN when acc == 0, as torch.max propagates it
        const float m = (q != q) ? q : fmaxf(1e-10f, q);                // render_utils.py:99
        disp[r] = 1.f / m;
    }
}
