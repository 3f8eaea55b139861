// What the mesh rasteriser (raster.hip), its batched form with colour (raster_frames.hip) and the soft silhouette (silhouette.hip) share: the
// handle, the camera, the float64 vertex pass, the exclusive scan of the per-tile counts, the edge functions that decide coverage and the
// rasterisers' depth test.  Both files work on one nm_raster_t, so a pixel is
// "inside" a face for the silhouette exactly when the rasteriser covers it.  Include after common.h.
#pragma once
#include "common.h"

#include <math.h>

namespace nm_rast {

constexpr int kTile = 16;                    // pixels per tile side; kTile * kTile lanes per workgroup
constexpr int kBatch = kTile * kTile;        // faces staged through LDS at a time
constexpr float kNormEps = 1e-6f;            // torch.nn.functional.normalize's eps as pytorch3d calls it: x / max(|x|, eps)

struct Cam {
    double w2c[12];                          // row-major [3][4]
    double fx, fy, cx, cy;
};

inline Cam make_cam(const double* w2c, double fx, double fy, double cx, double cy) {
    Cam cam;
    for (int i = 0; i < 12; ++i) cam.w2c[i] = w2c[i];
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy;
    return cam;
}

// ---- vertex pass ----------------------------------------------------------------------------------------------------------------------
// rule 1 for one vertex: (u, v, 1/z, z); the one-frame and the batched passes both go through here, so they round alike
__device__ __forceinline__ float4 project_vertex(const float* __restrict__ verts, int v, const Cam& cam) {
    const double x = verts[3 * v], y = verts[3 * v + 1], z = verts[3 * v + 2];
    const double xc = ((cam.w2c[0] * x + cam.w2c[1] * y) + cam.w2c[2] * z) + cam.w2c[3];
    const double yc = ((cam.w2c[4] * x + cam.w2c[5] * y) + cam.w2c[6] * z) + cam.w2c[7];
    const double zc = ((cam.w2c[8] * x + cam.w2c[9] * y) + cam.w2c[10] * z) + cam.w2c[11];
    // a vertex at or behind the camera plane drops its faces whole (face setup reads the sign of .w); its screen position is never used
    const bool front = zc > 0.0;
    const double iz = front ? 1.0 / zc : 0.0;
    return make_float4(front ? (float)(cam.fx * xc * iz + cam.cx) : 0.f, front ? (float)(cam.fy * yc * iz + cam.cy) : 0.f, (float)iz, (float)zc);
}

static __global__ void raster_vertex_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ adj_off,
                                            const int32_t* __restrict__ adj, int V, Cam cam, int want_normals, float4* __restrict__ vscr,
                                            float* __restrict__ vnrm) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    vscr[v] = project_vertex(verts, v, cam);
    if (!want_normals) return;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    for (int k = adj_off[v]; k < adj_off[v + 1]; ++k) {
        const int f = adj[k];
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        const double ax = (double)verts[3 * i1] - verts[3 * i0], ay = (double)verts[3 * i1 + 1] - verts[3 * i0 + 1], az = (double)verts[3 * i1 + 2] - verts[3 * i0 + 2];
        const double bx = (double)verts[3 * i2] - verts[3 * i0], by = (double)verts[3 * i2 + 1] - verts[3 * i0 + 1], bz = (double)verts[3 * i2 + 2] - verts[3 * i0 + 2];
        nx += ay * bz - az * by;
        ny += az * bx - ax * bz;
        nz += ax * by - ay * bx;
    }
    const double len = fmax(sqrt((nx * nx + ny * ny) + nz * nz), (double)kNormEps);
    vnrm[3 * v] = (float)(nx / len);
    vnrm[3 * v + 1] = (float)(ny / len);
    vnrm[3 * v + 2] = (float)(nz / len);
}

// exclusive scan of the T tile counts by one workgroup: offset[0 .. T], offset[T] the total; cursor = offset[0 .. T-1] for the fill
static __global__ void raster_scan_kernel(const int32_t* __restrict__ count, int T, int32_t* __restrict__ offset, int32_t* __restrict__ cursor) {
    __shared__ int part[256];
    const int per = (T + 255) / 256, lo = threadIdx.x * per, hi = min(lo + per, T);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int t = part[i]; part[i] = run; run += t; }
        offset[T] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) { offset[i] = run; cursor[i] = run; run += count[i]; }
}

// the three edge functions of the pixel centre, on vertices translated by it: w0 pairs (v1, v2), w1 (v2, v0), w2 (v0, v1)
__device__ __forceinline__ void edge_functions(const float4 r0, const float4 r1, float px, float py, float& w0, float& w1, float& w2) {
    const float ax = r0.x - px, ay = r0.y - py, bx = r0.z - px, by = r0.w - py, cx = r1.x - px, cy = r1.y - py;
    w0 = bx * cy - by * cx;
    w1 = cx * ay - cy * ax;
    w2 = ax * by - ay * bx;
}

// rule 2's coverage test on those edge functions
__device__ __forceinline__ bool covers(float w0, float w1, float w2) {
    const float s = (w0 + w1) + w2;
    return (s > 0.f && w0 >= 0.f && w1 >= 0.f && w2 >= 0.f) || (s < 0.f && w0 <= 0.f && w1 <= 0.f && w2 <= 0.f);
}

// rule 2's rejection and the 16 x 16-pixel tiles a face can cover: (tx0, ty0, tx1, ty1), tx0 > tx1 for a face that covers nothing.  a, b, c
// are its screen vertices (u, v, 1/z, z).  The screen box clipped to the image is conservative for rule 2 (a covered pixel's centre lies
// inside the closed box); a NaN fails the first comparison
__device__ __forceinline__ int4 tile_box(const float4 a, const float4 b, const float4 c, int W, int H) {
    int4 bx = make_int4(1, 1, 0, 0);
    const float area = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
    if (a.w > 0.f && b.w > 0.f && c.w > 0.f && area != 0.f) {
        float c0 = floorf(fminf(fminf(a.x, b.x), c.x)), c1 = floorf(fmaxf(fmaxf(a.x, b.x), c.x));
        float r0 = floorf(fminf(fminf(a.y, b.y), c.y)), r1 = floorf(fmaxf(fmaxf(a.y, b.y), c.y));
        if (c0 <= c1 && r0 <= r1 && c1 >= 0.f && r1 >= 0.f && c0 <= (float)(W - 1) && r0 <= (float)(H - 1)) {
            c0 = fmaxf(c0, 0.f); c1 = fminf(c1, (float)(W - 1));
            r0 = fmaxf(r0, 0.f); r1 = fminf(r1, (float)(H - 1));
            bx = make_int4((int)c0 / kTile, (int)r0 / kTile, (int)c1 / kTile, (int)r1 / kTile);
        }
    }
    return bx;
}

// rules 2 and 3 for one face and one pixel centre: r0 = (x0, y0, x1, y1), r1 = (x2, y2, 1/z0, 1/z1), iz2 = 1/z2.  Where the face covers the
// pixel, its perspective-correct depth enters the pixel's (z, face id) minimum
__device__ __forceinline__ void depth_test(const float4 r0, const float4 r1, float iz2, float px, float py, int f, float& zmin, int& fmin) {
    float w0, w1, w2;
    edge_functions(r0, r1, px, py, w0, w1, w2);
    if (!covers(w0, w1, w2)) return;
    const float s = (w0 + w1) + w2;
    const float z = s / ((w0 * r1.z + w1 * r1.w) + w2 * iz2);
    if (z < zmin || (z == zmin && f < fmin)) { zmin = z; fmin = f; }
}

// rule 3's b' of the winning face at the pixel centre
__device__ __forceinline__ void winner_bary(const float4 r0, const float4 r1, float iz2, float px, float py, float& b0, float& b1, float& b2) {
    float w0, w1, w2;
    edge_functions(r0, r1, px, py, w0, w1, w2);
    const float q0 = w0 * r1.z, q1 = w1 * r1.w, q2 = w2 * iz2;
    const float q = (q0 + q1) + q2;
    b0 = q0 / q; b1 = q1 / q; b2 = q2 / q;
}

// x / max(|x|, kNormEps)
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
    const float len = fmaxf(sqrtf((x * x + y * y) + z * z), kNormEps);
    x /= len; y /= len; z /= len;
}

// ---- colour lattice ('mesh lattice', rules L1 and L3) -----------------------------------------------------------------------------------
// L1: where node (i1, i2) of a lattice of resolution R is stored: rows by i2, row i2 has R + 1 - i2 entries
__device__ __forceinline__ int lattice_node(int R, int i1, int i2) { return i2 * (R + 1) - i2 * (i2 - 1) / 2 + i1; }

// L3: the colour of a face's lattice (nodes [S,3]) at the barycentrics (., b1, b2).  The cell index is clamped while it is still a float: a
// NaN falls into cell 0, and every node read lies inside the face's S nodes whatever b1 and b2 are
__device__ __forceinline__ void lattice_colour(const float* __restrict__ nodes, int R, float b1, float b2, float c[3]) {
    const float u1 = b1 * (float)R, u2 = b2 * (float)R;
    const int i1 = (int)fminf(fmaxf(floorf(u1), 0.f), (float)(R - 1));
    const int i2 = (int)fminf(fmaxf(floorf(u2), 0.f), (float)(R - 1 - i1));
    const float f1 = u1 - (float)i1, f2 = u2 - (float)i2;
    const bool upper = f1 + f2 > 1.f && i1 + i2 < R - 1;      // the hypotenuse cell has no upper half
    const float wa = upper ? (f1 + f2) - 1.f : (1.f - f1) - f2, wb = upper ? 1.f - f1 : f1, wc = upper ? 1.f - f2 : f2;
    const float* na = nodes + 3 * lattice_node(R, upper ? i1 + 1 : i1, upper ? i2 + 1 : i2);
    const float* nb = nodes + 3 * lattice_node(R, upper ? i1 : i1 + 1, upper ? i2 + 1 : i2);
    const float* nc = nodes + 3 * lattice_node(R, upper ? i1 + 1 : i1, upper ? i2 : i2 + 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (wa * na[k] + wb * nb[k]) + wc * nc[k];
}

// ---- lattice pyramid ('mesh mip', rules M2 and M3) --------------------------------------------------------------------------------------
// where level l's block of a pyramid of resolution R0 starts, in nodes per face: S(R0 >> k) summed over the finer levels k < l
__device__ __forceinline__ int pyramid_nodes_before(int R0, int l) {
    int n = 0;
    for (int k = 0; k < l; ++k) n += ((R0 >> k) + 1) * ((R0 >> k) + 2) / 2;
    return n;
}

// M2: the level of a face from its screen vertices r0 = (x0, y0, x1, y1), r1 = (x2, y2, ., .) and the blend t towards the next coarser
// one.  rho is the number of level-0 nodes per pixel across the face's narrowest extent (twice its area over its longest edge).  A NaN rho
// fails the loop's comparison and fmaxf returns its other operand for it: l = 0, t = 0; an infinite one walks to the coarsest level
__device__ __forceinline__ int lattice_level(const float4 r0, const float4 r1, int R0, int levels, float lod_scale, float& t) {
    const float ax = r0.z - r0.x, ay = r0.w - r0.y;           // d01
    const float bx = r1.x - r0.x, by = r1.y - r0.y;           // d02
    const float cx = r1.x - r0.z, cy = r1.y - r0.w;           // d12
    const float e2 = fmaxf(fmaxf(ax * ax + ay * ay, bx * bx + by * by), cx * cx + cy * cy);
    const float cr = fabsf(ax * by - ay * bx);
    float rho = lod_scale * (float)R0 * sqrtf(e2) / cr;
    int l = 0;
    while (rho >= 2.f && l < levels - 1) { rho *= 0.5f; ++l; }
    t = l < levels - 1 ? fminf(fmaxf(rho - 1.f, 0.f), 1.f) : 0.f;
    return l;
}

// M3: the colour of face f of a pyramid [levels][F,S(R0 >> l),3] at level l and the barycentrics (., b1, b2), blended by t towards level
// l + 1; t == 0 reads one level and gives lattice_colour's own bits on it
__device__ __forceinline__ void pyramid_colour(const float* __restrict__ pyramid, int F, int f, int R0, int l, float t, float b1, float b2, float c[3]) {
    const int R = R0 >> l, S = (R + 1) * (R + 2) / 2;
    const float* level = pyramid + 3 * ((size_t)F * pyramid_nodes_before(R0, l));
    lattice_colour(level + 3 * ((size_t)f * S), R, b1, b2, c);
    if (t > 0.f) {
        const int Rc = R >> 1;
        float d[3];
        lattice_colour(level + 3 * ((size_t)F * S) + 3 * ((size_t)f * ((Rc + 1) * (Rc + 2) / 2)), Rc, b1, b2, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = c[k] + t * (d[k] - c[k]);
    }
}

}  // namespace nm_rast

struct nm_raster_s {
    int F, V;
    int32_t* d_faces;        // [F,3]
    int32_t* d_adj_off;      // [V+1] vertex -> faces, CSR, ascending face id inside a vertex
    int32_t* d_adj;          // [3F]
    float4* d_vscr;          // [V] (u, v, 1/z, z)
    float* d_vnrm;           // [V,3]
    float4* d_rec;           // [F][3]
    int4* d_box;             // [F]
    int32_t* d_tiles;        // count [T], offset [T+1], cursor [T]: grown to the largest image seen
    int tiles_cap;
    int32_t* d_list;         // the tiles' face lists, end to end: grown to the largest total seen
    int64_t list_cap;
    float* d_gface;          // [F,3,2] the silhouette's screen-space gradient per face corner: made by the first backward call
    // the batched silhouette's scratch (silhouette.hip), apart from the one-frame passes': grown to the largest batch / image seen
    int batch_cap;           // frames the three per-frame arrays hold
    float4* d_bvscr;         // [B,V]
    float4* d_brec;          // [B,F,2]
    int4* d_bbox;            // [B,F]
    int64_t btiles_cap;      // B * T entries
    int32_t* d_bcount;       // [B*T]
    int64_t* d_boffset;      // [B*T+1] | {total, first bad frame + 1}: 64-bit, a batch's lists can pass 2^31 entries
    int gface_cap;           // frames d_bgface holds
    float* d_bgface;         // [B,F,3,2]: made by the first batched backward call
    // nm_raster_frames' scratch (raster_frames.hip), apart from both of the above: grown to the largest batch / image seen
    int frames_cap;          // frames d_fvscr holds
    float4* d_fvscr;         // [B,V]
    int64_t ftiles_cap;      // B * T entries
    int32_t* d_fcount;       // [B*T] the count pass's counts, then the fill pass's cursors
    int64_t* d_foffset;      // [B*T+1] | {total, first bad frame + 1}
};

namespace nm_rast {

// the tile scratch of an image of T tiles and the face lists of `total` entries: both only ever grow
inline int reserve_tiles(nm_raster_s* h, int T) {
    if (T <= h->tiles_cap) return NM_OK;
    if (h->d_tiles) (void)hipFree(h->d_tiles);
    h->d_tiles = nullptr; h->tiles_cap = 0;
    if (int rc = nm::check_hip(hipMalloc(&h->d_tiles, (size_t)(3 * T + 1) * 4), "raster: hipMalloc(tiles)")) return rc;
    h->tiles_cap = T;
    return NM_OK;
}

inline int reserve_lists(nm_raster_s* h, int64_t total) {
    if (total <= h->list_cap) return NM_OK;
    if (h->d_list) (void)hipFree(h->d_list);
    h->d_list = nullptr; h->list_cap = 0;
    if (int rc = nm::check_hip(hipMalloc(&h->d_list, (size_t)total * 4), "raster: hipMalloc(lists)")) return rc;
    h->list_cap = total;
    return NM_OK;
}

}  // namespace nm_rast

#define NM_RASTER_ARGS(who)                                                                                                         \
    NM_REQUIRE(h && verts && w2c, who ": null pointer");                                                                            \
    NM_REQUIRE(W >= 1 && H >= 1 && (int64_t)W * H <= (1ll << 30), who ": bad image size W=%d H=%d", W, H);                          \
    NM_REQUIRE(fx == fx && fy == fy && cx == cx && cy == cy, who ": NaN intrinsics")
