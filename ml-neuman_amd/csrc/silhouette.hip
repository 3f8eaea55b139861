// Soft silhouette of a triangle mesh and its gradient to the vertices -- reference preprocess/optimize_smpl.py:84-102 (silhouette_renderer_from_pinhole_cam:
// pytorch3d's MeshRasterizer with blur_radius = log(1/1e-4 - 1) sigma and 100 faces per pixel under SoftSilhouetteShader) and :249-252 (the
// silhouette term of optimize_smpl's loss and its backward).  pytorch3d is absent: include/neuman_hip.h 'soft silhouette' writes the contract out
// (rules S1-S6 on top of the rasteriser's rules 1-2), tests/helpers/silhouette_ref.py restates it in float64.
//
// forward
//   vertex pass    the rasteriser's (raster_device.h), without normals
//   face setup     one thread per face: reject as the rasteriser does, else the screen box grown by R_px = sqrt(blur_radius) min(W, H) / 2, in tiles
//   binning        one wave per tile scans the F boxes in face order, 64 at a time: ballot + popcount count the tile's faces, an exclusive scan
//                  sizes the lists exactly, and the same scan of the boxes fills them -- every list is in ASCENDING FACE ORDER, with no atomics
//   blend          one 256-lane workgroup per tile, one pixel per lane: the list goes through LDS 256 faces at a time and every lane multiplies
//                  its candidates' q_k into a register in list order (S6: the product has one order, so alpha and keep are the same bits every run)
// backward (recomputes S1-S2 from verts; only keep[H,W] is carried over from the forward)
//   face pass      one 256-lane workgroup per face walks the face's grown box clipped to the image in 16 x 16 steps: each lane sums its pixels' six
//                  screen-space partials in walk order, the wave sums in a fixed butterfly, the four waves in a fixed order -> g_face[F,3,2]
//   vertex pass    one thread per vertex gathers its faces through the vertex -> face table (ascending face order) and applies the
//                  projection's Jacobian in float64 -> g_verts[V,3]
// No float atomic anywhere: no two threads ever add into the same float.
// batch (nm_raster_silhouette_batch / _backward_batch: B frames of a sequence, one topology and image size, each its own vertices and camera)
//   every pass above is one launch over all frames, the frame a grid dimension (blockIdx.y); the per-thread work is the one-frame kernel's
//   own __device__ body on frame b's slice of the arrays, so frame b's outputs are the one-frame entries' bits; the (frame, tile) lists lie
//   end to end behind 64-bit offsets (a batch can pass 2^31 entries), scanned by one workgroup; one 16-byte read-back per call
#include "raster_device.h"

namespace {

using namespace nm_rast;

struct Soft {
    float sigma, blur;       // S3's sigma, S2's blur_radius (NDC units squared)
    float s2;                // (2 / min(W, H))^2: squared pixels -> squared NDC units (pytorch3d maps the shorter side to [-1, 1])
    float rpx;               // sqrt(blur) min(W, H) / 2: the reach of a face beyond its edges, in pixels
};

// rule 2's rejection and the pixels a face can reach: its screen box grown by rpx and one pixel of slack, clipped to the image.
// false: the face contributes nowhere.  (A NaN fails the first comparison.)
__device__ __forceinline__ bool grown_box(const float4 a, const float4 b, const float4 c, float rpx, int W, int H, int4& px) {
    const float area = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
    if (!(a.w > 0.f && b.w > 0.f && c.w > 0.f && area != 0.f)) return false;
    float c0 = floorf(fminf(fminf(a.x, b.x), c.x) - rpx) - 1.f, c1 = floorf(fmaxf(fmaxf(a.x, b.x), c.x) + rpx) + 1.f;
    float r0 = floorf(fminf(fminf(a.y, b.y), c.y) - rpx) - 1.f, r1 = floorf(fmaxf(fmaxf(a.y, b.y), c.y) + rpx) + 1.f;
    if (!(c0 <= c1 && r0 <= r1 && c1 >= 0.f && r1 >= 0.f && c0 <= (float)(W - 1) && r0 <= (float)(H - 1))) return false;
    c0 = fmaxf(c0, 0.f); c1 = fminf(c1, (float)(W - 1));
    r0 = fmaxf(r0, 0.f); r1 = fminf(r1, (float)(H - 1));
    px = make_int4((int)c0, (int)r0, (int)c1, (int)r1);
    return true;
}

// S1 for one edge a -> b, both translated by the pixel centre: foot parameter t, foot (qx, qy), squared distance m
__device__ __forceinline__ void segment(float ax, float ay, float bx, float by, float& m, float& t, float& qx, float& qy) {
    const float ex = bx - ax, ey = by - ay;
    t = fminf(fmaxf(-(ax * ex + ay * ey) / (ex * ex + ey * ey), 0.f), 1.f);
    qx = ax + t * ex;
    qy = ay + t * ey;
    m = qx * qx + qy * qy;
}

// S1 for one face and one pixel centre: inside (the rasteriser's coverage test) and the nearest of the edges 0: v0 v1, 1: v1 v2, 2: v2 v0
// (the first of equals), in squared pixels
__device__ __forceinline__ bool nearest_edge(const float4 r0, const float4 r1, float px, float py, float& m, int& edge, float& t, float& qx, float& qy) {
    float w0, w1, w2;
    edge_functions(r0, r1, px, py, w0, w1, w2);
    const float ax = r0.x - px, ay = r0.y - py, bx = r0.z - px, by = r0.w - py, cx = r1.x - px, cy = r1.y - py;
    float m1, t1, x1, y1, m2, t2, x2, y2;
    segment(ax, ay, bx, by, m, t, qx, qy);
    segment(bx, by, cx, cy, m1, t1, x1, y1);
    segment(cx, cy, ax, ay, m2, t2, x2, y2);
    edge = 0;
    if (m1 < m) { m = m1; t = t1; qx = x1; qy = y1; edge = 1; }
    if (m2 < m) { m = m2; t = t2; qx = x2; qy = y2; edge = 2; }
    return covers(w0, w1, w2);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// rec[f] = two float4: (x0, y0, x1, y1), (x2, y2, -, -); box[f] = tiles (tx0, ty0, tx1, ty1), tx0 > tx1 for a rejected face
__device__ __forceinline__ void face_setup(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, int f, int W, int H, float rpx,
                                           float4* __restrict__ rec, int4* __restrict__ box) {
    const float4 a = vscr[faces[3 * f]], b = vscr[faces[3 * f + 1]], c = vscr[faces[3 * f + 2]];
    int4 px;
    if (!grown_box(a, b, c, rpx, W, H, px)) { box[f] = make_int4(1, 1, 0, 0); return; }
    box[f] = make_int4(px.x / kTile, px.y / kTile, px.z / kTile, px.w / kTile);
    rec[2 * f] = make_float4(a.x, a.y, b.x, b.y);
    rec[2 * f + 1] = make_float4(c.x, c.y, 0.f, 0.f);
}

__global__ void sil_face_kernel(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, int F, int W, int H, float rpx,
                                float4* __restrict__ rec, int4* __restrict__ box) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) face_setup(vscr, faces, f, W, H, rpx, rec, box);
}

// one wave per tile over the F boxes in face order.  kFill = false: count[tile]; true: list[offset[tile] ...] = the tile's faces, ascending
// (the positions come from the same boxes the counts came from, so they stay below offset[tile + 1])
template <bool kFill>
__global__ void __launch_bounds__(256) sil_bin_kernel(const int4* __restrict__ box, int F, int TX, int T, int32_t* __restrict__ count,
                                                      const int32_t* __restrict__ offset, int32_t* __restrict__ list) {
    const int lane = threadIdx.x & 63, tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= T) return;
    const int tx = tile % TX, ty = tile / TX;
    int run = kFill ? offset[tile] : 0;
    const int end = kFill ? offset[tile + 1] : 0;
    for (int base = 0; base < F; base += 64) {
        const int f = base + lane;
        bool hit = false;
        if (f < F) {
            const int4 b = box[f];
            hit = b.x <= tx && tx <= b.z && b.y <= ty && ty <= b.w;
        }
        const unsigned long long mask = __ballot(hit);
        if (kFill && hit) {
            const int at = run + __popcll(mask & ((1ull << lane) - 1ull));
            if (at < end) list[at] = f;
        }
        run += __popcll(mask);
    }
    if (!kFill && lane == 0) count[tile] = run;
}

// one tile of one frame: list[begin .. end) are its faces in ascending order, rec / alpha / keep / n_cand the frame's own; s_rec [2 kBatch] in LDS
__device__ __forceinline__ void tile_blend(const float4* __restrict__ rec, const int32_t* __restrict__ list, int64_t begin, int64_t end, int tile, int W, int H,
                                           int TX, const Soft& so, float* __restrict__ alpha, float* __restrict__ keep, int32_t* __restrict__ n_cand,
                                           float4* s_rec) {
    const int lane = threadIdx.x;
    const int col = (tile % TX) * kTile + (lane % kTile), row = (tile / TX) * kTile + (lane / kTile);
    const float px = (float)col + 0.5f, py = (float)row + 0.5f;
    float prod = 1.f;
    int cand = 0;
    for (int64_t base = begin; base < end; base += kBatch) {
        const int n = (int)(end - base < (int64_t)kBatch ? end - base : (int64_t)kBatch);
        __syncthreads();                                       // the previous batch has been read
        if (lane < n) {
            const int f = list[base + lane];
            s_rec[2 * lane] = rec[2 * f];
            s_rec[2 * lane + 1] = rec[2 * f + 1];
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            float m, t, qx, qy;
            int edge;
            const bool in = nearest_edge(s_rec[2 * j], s_rec[2 * j + 1], px, py, m, edge, t, qx, qy);
            m *= so.s2;
            if (in || m < so.blur) {                           // S2
                prod *= 1.f / (1.f + expf((in ? m : -m) / so.sigma));      // S3: q = 1 / (1 + exp(-d / sigma)), d = -m inside
                ++cand;
            }
        }
    }
    if (col >= W || row >= H) return;
    const int64_t p = (int64_t)row * W + col;
    alpha[p] = 1.f - prod;
    keep[p] = prod;
    if (n_cand) n_cand[p] = cand;
}

__global__ void __launch_bounds__(kBatch) sil_tile_kernel(const float4* __restrict__ rec, const int32_t* __restrict__ offset, const int32_t* __restrict__ list,
                                                         int W, int H, int TX, Soft so, float* __restrict__ alpha, float* __restrict__ keep,
                                                         int32_t* __restrict__ n_cand) {
    __shared__ float4 s_rec[2 * kBatch];
    const int tile = blockIdx.x;
    tile_blend(rec, list, offset[tile], offset[tile + 1], tile, W, H, TX, so, alpha, keep, n_cand, s_rec);
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// one face of one frame by one 256-lane workgroup: vscr / keep / g_alpha / g_face the frame's own; s_part in LDS
__device__ __forceinline__ void bwd_face(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, int f, int W, int H, const Soft& so,
                                         const float* __restrict__ keep, const float* __restrict__ g_alpha, float* __restrict__ g_face, float (*s_part)[6]) {
    const int lane = threadIdx.x;
    const float4 a = vscr[faces[3 * f]], b = vscr[faces[3 * f + 1]], c = vscr[faces[3 * f + 2]];
    int4 box;
    if (!grown_box(a, b, c, so.rpx, W, H, box)) {              // (the same for the whole workgroup)
        if (lane < 6) g_face[6 * f + lane] = 0.f;
        return;
    }
    const float4 r0 = make_float4(a.x, a.y, b.x, b.y), r1 = make_float4(c.x, c.y, 0.f, 0.f);
    const int lx = lane % kTile, ly = lane / kTile;
    float g0x = 0.f, g0y = 0.f, g1x = 0.f, g1y = 0.f, g2x = 0.f, g2y = 0.f;
    for (int rb = box.y; rb <= box.w; rb += kTile)
        for (int cb = box.x; cb <= box.z; cb += kTile) {
            const int col = cb + lx, row = rb + ly;
            if (col > box.z || row > box.w) continue;
            const int64_t p = (int64_t)row * W + col;
            const float k = keep[p], ga = g_alpha[p];
            if (ga * k == 0.f) continue;                       // w = 0: nothing to add
            float m, t, qx, qy;
            int edge;
            const bool in = nearest_edge(r0, r1, (float)col + 0.5f, (float)row + 0.5f, m, edge, t, qx, qy);
            m *= so.s2;
            if (!(in || m < so.blur)) continue;
            const float e = expf((in ? m : -m) / so.sigma);
            const float omq = isinf(e) ? 1.f : e / (1.f + e);  // 1 - q_k without the cancellation
            const float w = ga * k / so.sigma * omq;           // S5: -g_alpha d alpha / d d_k
            // d d_k / d m_k = -1 inside, +1 outside; m_k = s2 |foot|^2; d |foot|^2 / d (edge start, edge end) = 2 foot (1 - t, t)
            const float s = (in ? w : -w) * so.s2 * 2.f;
            const float wa = s * (1.f - t), wb = s * t;
            const float u0 = edge == 0 ? wa : (edge == 2 ? wb : 0.f);
            const float u1 = edge == 1 ? wa : (edge == 0 ? wb : 0.f);
            const float u2 = edge == 2 ? wa : (edge == 1 ? wb : 0.f);
            g0x += u0 * qx; g0y += u0 * qy;
            g1x += u1 * qx; g1y += u1 * qy;
            g2x += u2 * qx; g2y += u2 * qy;
        }
    const float part[6] = {wave_sum(g0x), wave_sum(g0y), wave_sum(g1x), wave_sum(g1y), wave_sum(g2x), wave_sum(g2y)};
    if ((lane & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) s_part[lane >> 6][i] = part[i];
    }
    __syncthreads();
    if (lane < 6) g_face[6 * f + lane] = ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
}

__global__ void __launch_bounds__(256) sil_bwd_face_kernel(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, int W, int H, Soft so,
                                                           const float* __restrict__ keep, const float* __restrict__ g_alpha, float* __restrict__ g_face) {
    __shared__ float s_part[4][6];
    bwd_face(vscr, faces, blockIdx.x, W, H, so, keep, g_alpha, g_face, s_part);
}

__device__ __forceinline__ void bwd_vertex(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ adj_off,
                                           const int32_t* __restrict__ adj, int v, const Cam& cam, const float* __restrict__ g_face,
                                           float* __restrict__ g_verts) {
    double gu = 0.0, gv = 0.0;
    const int lo = adj_off[v], hi = adj_off[v + 1];
    for (int k = lo; k < hi; ++k) {
        const int f = adj[k];
        if (k > lo && adj[k - 1] == f) continue;               // a face that names the vertex twice is listed twice: all its corners were taken at the first
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (faces[3 * f + i] == v) { gu += g_face[6 * f + 2 * i]; gv += g_face[6 * f + 2 * i + 1]; }
    }
    const double x = verts[3 * v], y = verts[3 * v + 1], z = verts[3 * v + 2];
    const double xc = ((cam.w2c[0] * x + cam.w2c[1] * y) + cam.w2c[2] * z) + cam.w2c[3];
    const double yc = ((cam.w2c[4] * x + cam.w2c[5] * y) + cam.w2c[6] * z) + cam.w2c[7];
    const double zc = ((cam.w2c[8] * x + cam.w2c[9] * y) + cam.w2c[10] * z) + cam.w2c[11];
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (zc > 0.0) {                                            // (behind the camera plane every face of the vertex was dropped: its sums are zero)
        const double iz = 1.0 / zc;
        gx = gu * cam.fx * iz;                                 // u = fx xc / zc + cx, v = fy yc / zc + cy
        gy = gv * cam.fy * iz;
        gz = -(gu * cam.fx * xc + gv * cam.fy * yc) * iz * iz;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) g_verts[3 * v + j] = (float)((cam.w2c[j] * gx + cam.w2c[4 + j] * gy) + cam.w2c[8 + j] * gz);
}

__global__ void sil_bwd_vertex_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ adj_off,
                                      const int32_t* __restrict__ adj, int V, Cam cam, const float* __restrict__ g_face, float* __restrict__ g_verts) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V) bwd_vertex(verts, faces, adj_off, adj, v, cam, g_face, g_verts);
}

// ---- the batch: B frames of one topology and one image size, the frame a grid dimension (blockIdx.y) -------------------------------------
// Every kernel below is the one-frame kernel's body (the __device__ functions above) on frame b's slice of the arrays, so frame b's alpha,
// keep, n_cand and g_verts are the one-frame entries' bits.  The camera comes from device memory: w2c [B,4,4] (rows 0-2 are used), intr
// [B,4] = (fx, fy, cx, cy).  A frame with a non-finite entry in either gets no candidates (every screen vertex is (0, 0, 0, 0): w = 0 drops
// the face) and a zero gradient.
__device__ __forceinline__ bool load_cam(const double* __restrict__ w2c, const double* __restrict__ intr, int b, Cam& cam) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double x = w2c[16 * (size_t)b + i];
        ok = ok && isfinite(x);
        if (i < 12) cam.w2c[i] = x;
    }
    cam.fx = intr[4 * (size_t)b]; cam.fy = intr[4 * (size_t)b + 1]; cam.cx = intr[4 * (size_t)b + 2]; cam.cy = intr[4 * (size_t)b + 3];
    return ok && isfinite(cam.fx) && isfinite(cam.fy) && isfinite(cam.cx) && isfinite(cam.cy);
}

__global__ void sil_vertex_batch_kernel(const float* __restrict__ verts, const double* __restrict__ w2c, const double* __restrict__ intr, int V,
                                        float4* __restrict__ vscr) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= V) return;
    Cam cam;
    const bool ok = load_cam(w2c, intr, b, cam);
    vscr[(size_t)b * V + v] = ok ? project_vertex(verts + (size_t)b * V * 3, v, cam) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void sil_face_batch_kernel(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, int F, int V, int W, int H, float rpx,
                                      float4* __restrict__ rec, int4* __restrict__ box) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f < F) face_setup(vscr + (size_t)b * V, faces, f, W, H, rpx, rec + (size_t)b * F * 2, box + (size_t)b * F);
}

// sil_bin_kernel per (frame, tile): counts and 64-bit offsets are indexed b * T + tile, so a frame's lists lie end to end, each ascending
template <bool kFill>
__global__ void __launch_bounds__(256) sil_bin_batch_kernel(const int4* __restrict__ box, int F, int TX, int T, int32_t* __restrict__ count,
                                                            const int64_t* __restrict__ offset, int32_t* __restrict__ list) {
    const int lane = threadIdx.x & 63, tile = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (tile >= T) return;
    const int4* bx = box + (size_t)b * F;
    const int64_t g = (int64_t)b * T + tile;
    const int tx = tile % TX, ty = tile / TX;
    int64_t run = kFill ? offset[g] : 0;
    const int64_t end = kFill ? offset[g + 1] : 0;
    for (int base = 0; base < F; base += 64) {
        const int f = base + lane;
        bool hit = false;
        if (f < F) {
            const int4 q = bx[f];
            hit = q.x <= tx && tx <= q.z && q.y <= ty && ty <= q.w;
        }
        const unsigned long long mask = __ballot(hit);
        if (kFill && hit) {
            const int64_t at = run + __popcll(mask & ((1ull << lane) - 1ull));
            if (at < end) list[at] = f;
        }
        run += __popcll(mask);
    }
    if (!kFill && lane == 0) count[g] = (int32_t)run;
}

// exclusive scan of the n = B T counts by one workgroup into 64-bit offsets: offset[0 .. n], offset[n] the total; offset[n + 1] = 1 + the
// first frame whose camera has a non-finite entry, 0 if none -- the two words the host reads back
__global__ void __launch_bounds__(1024) sil_scan_batch_kernel(const int32_t* __restrict__ count, int64_t n, const double* __restrict__ w2c,
                                                              const double* __restrict__ intr, int B, int64_t* __restrict__ offset) {
    __shared__ int64_t part[1024];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = B;
    const int64_t per = (n + 1023) / 1024, lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 1024) {
        Cam cam;
        if (!load_cam(w2c, intr, b, cam)) atomicMin(&s_bad, b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < 1024; ++i) { const int64_t t = part[i]; part[i] = run; run += t; }
        offset[n] = run;
        offset[n + 1] = s_bad < B ? s_bad + 1 : 0;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { offset[i] = run; run += count[i]; }
}

__global__ void __launch_bounds__(kBatch) sil_tile_batch_kernel(const float4* __restrict__ rec, const int64_t* __restrict__ offset,
                                                               const int32_t* __restrict__ list, int F, int W, int H, int TX, int T, Soft so,
                                                               float* __restrict__ alpha, float* __restrict__ keep, int32_t* __restrict__ n_cand) {
    __shared__ float4 s_rec[2 * kBatch];
    const int tile = blockIdx.x, b = blockIdx.y;
    const int64_t g = (int64_t)b * T + tile;
    const size_t px = (size_t)b * W * H;
    tile_blend(rec + (size_t)b * F * 2, list, offset[g], offset[g + 1], tile, W, H, TX, so, alpha + px, keep + px, n_cand ? n_cand + px : nullptr, s_rec);
}

__global__ void __launch_bounds__(256) sil_bwd_face_batch_kernel(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, int F, int V, int W,
                                                                 int H, Soft so, const float* __restrict__ keep, const float* __restrict__ g_alpha,
                                                                 float* __restrict__ g_face) {
    __shared__ float s_part[4][6];
    const int b = blockIdx.y;
    const size_t px = (size_t)b * W * H;
    bwd_face(vscr + (size_t)b * V, faces, blockIdx.x, W, H, so, keep + px, g_alpha + px, g_face + (size_t)b * F * 6, s_part);
}

__global__ void sil_bwd_vertex_batch_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ adj_off,
                                            const int32_t* __restrict__ adj, int F, int V, const double* __restrict__ w2c,
                                            const double* __restrict__ intr, const float* __restrict__ g_face, float* __restrict__ g_verts) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= V) return;
    Cam cam;
    float* g = g_verts + (size_t)b * V * 3;
    if (load_cam(w2c, intr, b, cam)) bwd_vertex(verts + (size_t)b * V * 3, faces, adj_off, adj, v, cam, g_face + (size_t)b * F * 6, g);
    else g[3 * v] = g[3 * v + 1] = g[3 * v + 2] = 0.f;
}

// the batch's scratch: per-frame screen vertices, face records and boxes for B frames, counts and offsets for B T tiles; both only grow
int reserve_batch(nm_raster_s* h, int B, int T) {
    int rc = NM_OK;
    if (B > h->batch_cap) {
        void* old[] = {h->d_bvscr, h->d_brec, h->d_bbox};
        for (void* p : old)
            if (p) (void)hipFree(p);
        h->d_bvscr = nullptr; h->d_brec = nullptr; h->d_bbox = nullptr; h->batch_cap = 0;
        if ((rc = nm::check_hip(hipMalloc(&h->d_bvscr, (size_t)B * h->V * sizeof(float4)), "silhouette batch: hipMalloc(screen vertices)"))) return rc;
        if ((rc = nm::check_hip(hipMalloc(&h->d_brec, (size_t)B * h->F * 2 * sizeof(float4)), "silhouette batch: hipMalloc(records)"))) return rc;
        if ((rc = nm::check_hip(hipMalloc(&h->d_bbox, (size_t)B * h->F * sizeof(int4)), "silhouette batch: hipMalloc(boxes)"))) return rc;
        h->batch_cap = B;
    }
    const int64_t n = (int64_t)B * T;
    if (n > h->btiles_cap) {
        if (h->d_bcount) (void)hipFree(h->d_bcount);
        if (h->d_boffset) (void)hipFree(h->d_boffset);
        h->d_bcount = nullptr; h->d_boffset = nullptr; h->btiles_cap = 0;
        if ((rc = nm::check_hip(hipMalloc(&h->d_bcount, (size_t)n * 4), "silhouette batch: hipMalloc(counts)"))) return rc;
        if ((rc = nm::check_hip(hipMalloc(&h->d_boffset, (size_t)(n + 2) * 8), "silhouette batch: hipMalloc(offsets)"))) return rc;
        h->btiles_cap = n;
    }
    return NM_OK;
}

Soft make_soft(double sigma, double blur_radius, int W, int H) {
    const double half = 0.5 * (double)(W < H ? W : H);
    Soft so;
    so.sigma = (float)sigma;
    so.blur = (float)blur_radius;
    so.s2 = (float)(1.0 / (half * half));
    so.rpx = (float)(sqrt(blur_radius) * half);
    return so;
}

}  // namespace

extern "C" {

#define NM_SOFT_ARGS(who)                                                                                                            \
    NM_REQUIRE(sigma > 0.0 && isfinite(sigma) && (float)sigma > 0.f, who ": sigma must be finite and > 0 (got %g)", sigma);          \
    NM_REQUIRE(blur_radius >= 0.0 && isfinite(blur_radius), who ": blur_radius must be finite and >= 0 (got %g)", blur_radius)

int nm_raster_silhouette(nm_raster_t h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W, int H, double sigma,
                         double blur_radius, float* alpha, float* keep, int32_t* n_cand, nm_stream_t stream) {
    NM_RASTER_ARGS("nm_raster_silhouette");
    NM_REQUIRE(alpha && keep, "nm_raster_silhouette: null output");
    NM_SOFT_ARGS("nm_raster_silhouette");
    hipStream_t st = nm::as_stream(stream);
    const int TX = (W + kTile - 1) / kTile, TY = (H + kTile - 1) / kTile, T = TX * TY;
    int rc = NM_OK;
    if ((rc = reserve_tiles(h, T))) return rc;
    int32_t *count = h->d_tiles, *offset = count + T, *cursor = offset + T + 1;
    const Cam cam = make_cam(w2c, fx, fy, cx, cy);
    const Soft so = make_soft(sigma, blur_radius, W, H);
    hipLaunchKernelGGL(raster_vertex_kernel, dim3((h->V + 255) / 256), dim3(256), 0, st, verts, h->d_faces, h->d_adj_off, h->d_adj, h->V, cam, 0, h->d_vscr,
                       h->d_vnrm);
    hipLaunchKernelGGL(sil_face_kernel, dim3((h->F + 255) / 256), dim3(256), 0, st, h->d_vscr, h->d_faces, h->F, W, H, so.rpx, h->d_rec, h->d_box);
    hipLaunchKernelGGL(sil_bin_kernel<false>, dim3((T + 3) / 4), dim3(256), 0, st, h->d_box, h->F, TX, T, count, offset, (int32_t*)nullptr);
    hipLaunchKernelGGL(raster_scan_kernel, dim3(1), dim3(256), 0, st, count, T, offset, cursor);
    if ((rc = nm::check_launch("silhouette setup kernels"))) return rc;
    // the one read-back, as in the rasteriser: the lists' total length, so that their buffer is sized exactly
    int32_t total = 0;
    if ((rc = nm::check_hip(hipMemcpyAsync(&total, offset + T, 4, hipMemcpyDeviceToHost, st), "silhouette: read total"))) return rc;
    if ((rc = nm::check_hip(hipStreamSynchronize(st), "silhouette: sync"))) return rc;
    if (total < 0) { nm::set_error("nm_raster_silhouette: the tile lists overflow 2^31 entries"); return NM_ERR_UNSUPPORTED; }
    if ((rc = reserve_lists(h, total))) return rc;
    if (total > 0) hipLaunchKernelGGL(sil_bin_kernel<true>, dim3((T + 3) / 4), dim3(256), 0, st, h->d_box, h->F, TX, T, count, offset, h->d_list);
    hipLaunchKernelGGL(sil_tile_kernel, dim3(T), dim3(kBatch), 0, st, h->d_rec, offset, h->d_list, W, H, TX, so, alpha, keep, n_cand);
    return nm::check_launch("sil_tile_kernel");
}

int nm_raster_silhouette_backward(nm_raster_t h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W, int H,
                                  double sigma, double blur_radius, const float* keep, const float* g_alpha, float* g_verts, nm_stream_t stream) {
    NM_RASTER_ARGS("nm_raster_silhouette_backward");
    NM_REQUIRE(keep && g_alpha && g_verts, "nm_raster_silhouette_backward: null keep, g_alpha or g_verts");
    NM_SOFT_ARGS("nm_raster_silhouette_backward");
    hipStream_t st = nm::as_stream(stream);
    int rc = NM_OK;
    if (!h->d_gface && (rc = nm::check_hip(hipMalloc(&h->d_gface, (size_t)h->F * 6 * sizeof(float)), "nm_raster_silhouette_backward: hipMalloc(g_face)"))) return rc;
    const Cam cam = make_cam(w2c, fx, fy, cx, cy);
    const Soft so = make_soft(sigma, blur_radius, W, H);
    hipLaunchKernelGGL(raster_vertex_kernel, dim3((h->V + 255) / 256), dim3(256), 0, st, verts, h->d_faces, h->d_adj_off, h->d_adj, h->V, cam, 0, h->d_vscr,
                       h->d_vnrm);
    hipLaunchKernelGGL(sil_bwd_face_kernel, dim3(h->F), dim3(256), 0, st, h->d_vscr, h->d_faces, W, H, so, keep, g_alpha, h->d_gface);
    hipLaunchKernelGGL(sil_bwd_vertex_kernel, dim3((h->V + 255) / 256), dim3(256), 0, st, verts, h->d_faces, h->d_adj_off, h->d_adj, h->V, cam, h->d_gface,
                       g_verts);
    return nm::check_launch("silhouette backward kernels");
}

#define NM_BATCH_ARGS(who)                                                                                                          \
    NM_REQUIRE(h && verts && w2c && intr, who ": null pointer");                                                                    \
    NM_REQUIRE(B >= 1 && B <= 65535, who ": B = %d frames (1 <= B <= 65535)", B);                                                   \
    NM_REQUIRE(W >= 1 && H >= 1 && (int64_t)W * H <= (1ll << 30), who ": bad image size W=%d H=%d", W, H)

int nm_raster_silhouette_batch(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H, double sigma,
                               double blur_radius, float* alpha, float* keep, int32_t* n_cand, nm_stream_t stream) {
    NM_BATCH_ARGS("nm_raster_silhouette_batch");
    NM_REQUIRE(alpha && keep, "nm_raster_silhouette_batch: null output");
    NM_SOFT_ARGS("nm_raster_silhouette_batch");
    hipStream_t st = nm::as_stream(stream);
    const int TX = (W + kTile - 1) / kTile, TY = (H + kTile - 1) / kTile, T = TX * TY;
    const int64_t n = (int64_t)B * T;
    int rc = NM_OK;
    if ((rc = reserve_batch(h, B, T))) return rc;
    const Soft so = make_soft(sigma, blur_radius, W, H);
    hipLaunchKernelGGL(sil_vertex_batch_kernel, dim3((h->V + 255) / 256, B), dim3(256), 0, st, verts, w2c, intr, h->V, h->d_bvscr);
    hipLaunchKernelGGL(sil_face_batch_kernel, dim3((h->F + 255) / 256, B), dim3(256), 0, st, h->d_bvscr, h->d_faces, h->F, h->V, W, H, so.rpx, h->d_brec,
                       h->d_bbox);
    hipLaunchKernelGGL(sil_bin_batch_kernel<false>, dim3((T + 3) / 4, B), dim3(256), 0, st, h->d_bbox, h->F, TX, T, h->d_bcount, (const int64_t*)nullptr,
                       (int32_t*)nullptr);
    hipLaunchKernelGGL(sil_scan_batch_kernel, dim3(1), dim3(1024), 0, st, h->d_bcount, n, w2c, intr, B, h->d_boffset);
    if ((rc = nm::check_launch("silhouette batch setup kernels"))) return rc;
    // the one read-back of the call: the lists' total length (64-bit: a batch can pass 2^31 entries) and the bad-camera word beside it
    int64_t back[2] = {0, 0};
    if ((rc = nm::check_hip(hipMemcpyAsync(back, h->d_boffset + n, 16, hipMemcpyDeviceToHost, st), "silhouette batch: read total"))) return rc;
    if ((rc = nm::check_hip(hipStreamSynchronize(st), "silhouette batch: sync"))) return rc;
    const int64_t total = back[0];
    if (total < 0 || total > (int64_t)B * T * h->F) { nm::set_error("nm_raster_silhouette_batch: bad list total %lld", (long long)total); return NM_ERR_UNSUPPORTED; }
    if ((rc = reserve_lists(h, total))) return rc;
    if (total > 0)
        hipLaunchKernelGGL(sil_bin_batch_kernel<true>, dim3((T + 3) / 4, B), dim3(256), 0, st, h->d_bbox, h->F, TX, T, h->d_bcount, h->d_boffset, h->d_list);
    hipLaunchKernelGGL(sil_tile_batch_kernel, dim3(T, B), dim3(kBatch), 0, st, h->d_brec, h->d_boffset, h->d_list, h->F, W, H, TX, T, so, alpha, keep, n_cand);
    if ((rc = nm::check_launch("sil_tile_batch_kernel"))) return rc;
    // (the bad frame's outputs are defined all the same: it had no candidates, so alpha 0 and keep 1)
    NM_REQUIRE(back[1] == 0, "nm_raster_silhouette_batch: a non-finite w2c or intrinsic entry in frame %lld", (long long)(back[1] - 1));
    return NM_OK;
}

int nm_raster_silhouette_backward_batch(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H, double sigma,
                                        double blur_radius, const float* keep, const float* g_alpha, float* g_verts, nm_stream_t stream) {
    NM_BATCH_ARGS("nm_raster_silhouette_backward_batch");
    NM_REQUIRE(keep && g_alpha && g_verts, "nm_raster_silhouette_backward_batch: null keep, g_alpha or g_verts");
    NM_SOFT_ARGS("nm_raster_silhouette_backward_batch");
    hipStream_t st = nm::as_stream(stream);
    const int TX = (W + kTile - 1) / kTile, TY = (H + kTile - 1) / kTile;
    int rc = NM_OK;
    if ((rc = reserve_batch(h, B, TX * TY))) return rc;
    if (B > h->gface_cap) {
        if (h->d_bgface) (void)hipFree(h->d_bgface);
        h->d_bgface = nullptr; h->gface_cap = 0;
        if ((rc = nm::check_hip(hipMalloc(&h->d_bgface, (size_t)B * h->F * 6 * sizeof(float)), "nm_raster_silhouette_backward_batch: hipMalloc(g_face)"))) return rc;
        h->gface_cap = B;
    }
    const Soft so = make_soft(sigma, blur_radius, W, H);
    hipLaunchKernelGGL(sil_vertex_batch_kernel, dim3((h->V + 255) / 256, B), dim3(256), 0, st, verts, w2c, intr, h->V, h->d_bvscr);
    hipLaunchKernelGGL(sil_bwd_face_batch_kernel, dim3(h->F, B), dim3(256), 0, st, h->d_bvscr, h->d_faces, h->F, h->V, W, H, so, keep, g_alpha, h->d_bgface);
    hipLaunchKernelGGL(sil_bwd_vertex_batch_kernel, dim3((h->V + 255) / 256, B), dim3(256), 0, st, verts, h->d_faces, h->d_adj_off, h->d_adj, h->F, h->V, w2c,
                       intr, h->d_bgface, g_verts);
    return nm::check_launch("silhouette batch backward kernels");
}

}  // extern "C"
