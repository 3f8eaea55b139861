// A texture atlas from per-face colour lattices -- include/neuman_hip.h 'mesh atlas', rules A1-A5.  The reference has no such step; it is what
// lets a lattice-coloured mesh (mesh_lattice.hip) leave the project as an OBJ with one image (neuman_hip/mesh_export.py).  Two faces share a
// block of (R+4) x (R+1) texels: the even face's nodes sit at (i1, i2), the odd face's under the point reflection (x, y) -> (R+3-x, R-y), and
// the two diagonals between them are gutters whose values make a viewer's bilinear filter the linear blend of rule L3 in the cells on the
// hypotenuse.  tests/helpers/mesh_atlas_ref.py restates A1-A5 in numpy.
//
//   pack    one thread per texel, gather form: the texel finds its block, its face and its local coordinates, and reads one node (a node
//           texel, the corner gutter), three nodes (a gutter texel) or nothing (+0.0).  A wave's lanes take consecutive texels of a row, so
//           its 12-byte stores are contiguous.  No memset, no atomic, no read-back; W H <= 2^28, so the grid covers the atlas without a loop.
//   sample  one thread per point, grid-stride in 64 bits: rule L3's cell, then the four texels around it; every read lies in the face's own
//           half block whatever the barycentrics.  No read-back.
#include "mesh_device.h"

namespace {

using namespace nm_mesh;

constexpr int kMaxR = 64;
constexpr int kMaxSide = 16384;                               // W and H of an atlas
constexpr unsigned kMaxBlocks = 1u << 20;                     // the grid of the sampler's grid-stride loop

struct Atlas {                                                // rule A1
    int W, H, nbx, R;
    int64_t F, P;
};

// A1 by integer arithmetic only; false when the atlas would be wider or higher than kMaxSide.  1 <= F, 1 <= R <= kMaxR.
bool atlas_of(int64_t F, int R, Atlas* a) {
    const int64_t BW = R + 4, BH = R + 1, P = F / 2 + F % 2;
    if (P > (int64_t)kMaxSide * kMaxSide) return false;       // (more blocks than texels: also keeps P BH inside 64 bits)
    int64_t n = 1;
    while (n * n * BW < P * BH) {
        if (++n * BW > kMaxSide) return false;
    }
    const int64_t nby = (P + n - 1) / n;
    if (n * BW > kMaxSide || nby * BH > kMaxSide) return false;
    *a = Atlas{(int)(n * BW), (int)(nby * BH), (int)n, R, F, P};
    return true;
}

// L1: where node (i1, i2) is stored
__device__ __forceinline__ int node_at(int R, int i1, int i2) { return i2 * (R + 1) - i2 * (i2 - 1) / 2 + i1; }

__global__ void __launch_bounds__(kThreads) atlas_pack_kernel(const float* __restrict__ face_colours, Atlas a, float* __restrict__ atlas) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (int64_t)a.W * a.H) return;
    const int R = a.R, BW = R + 4, BH = R + 1, S = (R + 1) * (R + 2) / 2;
    const int Y = (int)(t / a.W), X = (int)(t - (int64_t)Y * a.W);
    const int bx = X / BW, by = Y / BH;
    int x = X - bx * BW, y = Y - by * BH;
    const int64_t p = (int64_t)by * a.nbx + bx;
    int64_t f = 2 * p;
    if (x + y >= R + 2) {                                      // A2: the upper face's gutter and nodes, seen in its own coordinates
        ++f;
        x = R + 3 - x;
        y = R - y;
    }
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;                        // a block past the last, the upper half of a lone lower face
    if (p < a.P && f < a.F) {
        const float* nodes = face_colours + f * S * 3;
        if (x + y <= R || x == R + 1) {                        // a node, or the corner gutter texel (R+1, 0): a copy of node (R, 0)
            const float* n = nodes + 3 * node_at(R, x == R + 1 ? R : x, y);
            c0 = n[0], c1 = n[1], c2 = n[2];
        } else {                                               // a gutter texel: what makes t00 - t10 - t01 + t11 vanish in its cell
            const float *r = nodes + 3 * node_at(R, x, y - 1), *u = nodes + 3 * node_at(R, x - 1, y), *d = nodes + 3 * node_at(R, x - 1, y - 1);
            c0 = (r[0] + u[0]) - d[0], c1 = (r[1] + u[1]) - d[1], c2 = (r[2] + u[2]) - d[2];
        }
    }
    float* o = atlas + t * 3;
    o[0] = c0, o[1] = c1, o[2] = c2;
}

__global__ void __launch_bounds__(kThreads) atlas_sample_kernel(const float* __restrict__ atlas, Atlas a, const int32_t* __restrict__ face_id,
                                                                const float* __restrict__ bary, int64_t n, float* __restrict__ out) {
    const int R = a.R, BW = R + 4, BH = R + 1;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += stride) {
        const int32_t f = face_id[t];
        float c[3] = {0.f, 0.f, 0.f};
        if (in_range(f, a.F)) {
            const float u1 = bary[3 * t + 1] * (float)R, u2 = bary[3 * t + 2] * (float)R;
            const int i1 = (int)fminf(fmaxf(floorf(u1), 0.f), (float)(R - 1));             // L3's cell: clamped as a float, a NaN counts as 0
            const int i2 = (int)fminf(fmaxf(floorf(u2), 0.f), (float)(R - 1 - i1));
            const float f1 = u1 - (float)i1, f2 = u2 - (float)i2, g1 = 1.f - f1, g2 = 1.f - f2;
            const float w00 = g1 * g2, w10 = f1 * g2, w01 = g1 * f2, w11 = f1 * f2;
            const int p = f >> 1, bx = p % a.nbx, by = p / a.nbx;
            // texel (i1, i2) of the half block and the steps to (i1+1, .) and (., i2+1): reflected for an odd face
            const int x = bx * BW + (f & 1 ? R + 3 - i1 : i1), y = by * BH + (f & 1 ? R - i2 : i2);
            const int64_t dx = f & 1 ? -3 : 3, dy = (f & 1 ? -3 : 3) * (int64_t)a.W;
            const float* t00 = atlas + ((int64_t)y * a.W + x) * 3;
            const float *t10 = t00 + dx, *t01 = t00 + dy, *t11 = t01 + dx;
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = (w00 * t00[k] + w10 * t10[k]) + (w01 * t01[k] + w11 * t11[k]);
        }
        float* o = out + 3 * t;
        o[0] = c[0], o[1] = c[1], o[2] = c[2];
    }
}

}  // namespace

extern "C" {

int nm_mesh_atlas_size(int64_t F, int R, int* W, int* H, int* nbx) {
    NM_REQUIRE(W && H && nbx, "nm_mesh_atlas_size: null pointer");
    NM_REQUIRE(R >= 1 && R <= kMaxR, "nm_mesh_atlas_size: R = %d (1 <= R <= %d)", R, kMaxR);
    NM_REQUIRE(F >= 1, "nm_mesh_atlas_size: F = %lld faces (F >= 1)", (long long)F);
    Atlas a;
    NM_REQUIRE(atlas_of(F, R, &a), "nm_mesh_atlas_size: the atlas of F = %lld faces at R = %d is wider or higher than %d texels", (long long)F, R, kMaxSide);
    *W = a.W, *H = a.H, *nbx = a.nbx;
    return NM_OK;
}

int nm_mesh_atlas_pack(const float* face_colours, int64_t F, int R, float* atlas, nm_stream_t stream) {
    NM_REQUIRE(face_colours && atlas, "nm_mesh_atlas_pack: null pointer");
    NM_REQUIRE(R >= 1 && R <= kMaxR, "nm_mesh_atlas_pack: R = %d (1 <= R <= %d)", R, kMaxR);
    NM_REQUIRE(F >= 1, "nm_mesh_atlas_pack: F = %lld faces (F >= 1)", (long long)F);
    Atlas a;
    NM_REQUIRE(atlas_of(F, R, &a), "nm_mesh_atlas_pack: the atlas of F = %lld faces at R = %d is wider or higher than %d texels", (long long)F, R, kMaxSide);
    hipLaunchKernelGGL(atlas_pack_kernel, dim3(blocks_for((int64_t)a.W * a.H)), dim3(kThreads), 0, nm::as_stream(stream), face_colours, a, atlas);
    return nm::check_launch("nm_mesh_atlas_pack: kernel");
}

int nm_mesh_atlas_sample(const float* atlas, int64_t F, int R, const int32_t* face_id, const float* bary, int64_t n, float* out, nm_stream_t stream) {
    NM_REQUIRE(atlas && face_id && bary && out, "nm_mesh_atlas_sample: null pointer");
    NM_REQUIRE(R >= 1 && R <= kMaxR, "nm_mesh_atlas_sample: R = %d (1 <= R <= %d)", R, kMaxR);
    NM_REQUIRE(F >= 1, "nm_mesh_atlas_sample: F = %lld faces (F >= 1)", (long long)F);
    NM_REQUIRE(n >= 1, "nm_mesh_atlas_sample: n = %lld points (n >= 1)", (long long)n);
    Atlas a;
    NM_REQUIRE(atlas_of(F, R, &a), "nm_mesh_atlas_sample: the atlas of F = %lld faces at R = %d is wider or higher than %d texels", (long long)F, R, kMaxSide);
    const int64_t blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(atlas_sample_kernel, dim3((unsigned)(blocks < (int64_t)kMaxBlocks ? blocks : (int64_t)kMaxBlocks)), dim3(kThreads), 0,
                       nm::as_stream(stream), atlas, a, face_id, bary, n, out);
    return nm::check_launch("nm_mesh_atlas_sample: kernel");
}

}  // extern "C"
