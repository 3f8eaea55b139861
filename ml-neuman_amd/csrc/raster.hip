// Triangle-mesh rasteriser: the body's per-pixel face id, depth and barycentrics, its Phong-shaded overlay and the byte select onto a
// photograph -- reference utils/render_utils.py:464-501 (phong_renderer_from_pinhole_cam + overlay_smpl, which sit on pytorch3d's
// MeshRasterizer with blur_radius 0, one face per pixel, and HardPhongShader).  pytorch3d is not vendored by the reference and is absent
// here: include/neuman_hip.h writes the contract out (plain pinhole projection, pixel centres, barycentrics >= 0, nearest perspective-correct
// depth, lower face index on an exact tie, per-pixel Phong in world space); tests/helpers/raster_ref.py restates it in float64.
//
//   vertex pass    one thread per vertex, in float64: camera-space position, screen position, 1/z; the area-weighted vertex normal is the sum of
//                  cross(v1-v0, v2-v0) over the vertex's faces, gathered through a vertex -> face table in ascending face order (no atomics: the
//                  normals are the same bits on every run)
//   face setup     one thread per face: reject (a vertex at z <= 0, zero screen area, box off the image), else the 16 x 16-pixel tiles
//                  its screen box, clipped to the image, touches; count per tile (integer atomics) -> exclusive scan -> fill (integer atomics on a cursor)
//   raster + shade one 256-thread workgroup per tile, one pixel per lane: the tile's list goes through LDS 256 faces at a time, every lane keeps
//                  its (z, face) minimum in registers, and after the last batch recomputes the winner's barycentrics, shades and writes
//
// The order inside a tile's list is whatever the atomics made it; the minimum over (z, face id) does not depend on it.  The edge functions are
// evaluated on vertices translated by the pixel centre (products of differences, no fmaf: cross(b, c) = -cross(c, b) exactly, so the two faces
// of a shared edge never both reject a pixel), which keeps sub-pixel triangles well conditioned.
#include "raster_device.h"

#include <string.h>

#include <vector>

namespace {

using namespace nm_rast;                     // the handle, the camera, the vertex pass, the scan and the edge functions: raster_device.h

struct Shade {
    float light[3], centre[3];               // world space
};

// ---- face setup and binning -----------------------------------------------------------------------------------------------------------
// rec[f] = three float4: (x0, y0, x1, y1), (x2, y2, 1/z0, 1/z1), (1/z2, -, -, -); box[f] = tiles (tx0, ty0, tx1, ty1), tx0 > tx1 for a rejected face
__global__ void raster_face_kernel(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, int F, int W, int H, int TX,
                                   float4* __restrict__ rec, int4* __restrict__ box, int32_t* __restrict__ count) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float4 a = vscr[faces[3 * f]], b = vscr[faces[3 * f + 1]], c = vscr[faces[3 * f + 2]];
    const int4 bx = tile_box(a, b, c, W, H);
    box[f] = bx;
    if (bx.x > bx.z) return;
    rec[3 * f] = make_float4(a.x, a.y, b.x, b.y);
    rec[3 * f + 1] = make_float4(c.x, c.y, a.z, b.z);
    rec[3 * f + 2] = make_float4(c.z, 0.f, 0.f, 0.f);
    for (int ty = bx.y; ty <= bx.w; ++ty)
        for (int tx = bx.x; tx <= bx.z; ++tx) atomicAdd(&count[ty * TX + tx], 1);
}

__global__ void raster_fill_kernel(const int4* __restrict__ box, int F, int TX, int32_t* __restrict__ cursor, int32_t* __restrict__ list, int cap) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int4 bx = box[f];
    for (int ty = bx.y; ty <= bx.w; ++ty)
        for (int tx = bx.x; tx <= bx.z; ++tx) {
            const int at = atomicAdd(&cursor[ty * TX + tx], 1);
            if (at < cap) list[at] = f;                        // (always: the counts came from the same boxes)
        }
}

// ---- raster and shade -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBatch) raster_tile_kernel(const float4* __restrict__ rec, const int32_t* __restrict__ offset, const int32_t* __restrict__ list,
                                                            const int32_t* __restrict__ faces, const float* __restrict__ verts,
                                                            const float* __restrict__ vnrm, int W, int H, int TX, Shade sh, int32_t* __restrict__ face_id,
                                                            float* __restrict__ zbuf, float* __restrict__ bary, float4* __restrict__ rgba) {
    __shared__ float4 s_rec[3 * kBatch];
    __shared__ int s_face[kBatch];
    const int tile = blockIdx.x, lane = threadIdx.x;
    const int col = (tile % TX) * kTile + (lane % kTile), row = (tile / TX) * kTile + (lane / kTile);
    const float px = (float)col + 0.5f, py = (float)row + 0.5f;
    const int begin = offset[tile], end = offset[tile + 1];
    float zmin = INFINITY;
    int fmin = -1;
    for (int base = begin; base < end; base += kBatch) {
        const int n = min(kBatch, end - base);
        __syncthreads();                                       // the previous batch has been read
        if (lane < n) {
            const int f = list[base + lane];
            s_face[lane] = f;
            s_rec[3 * lane] = rec[3 * f];
            s_rec[3 * lane + 1] = rec[3 * f + 1];
            s_rec[3 * lane + 2] = rec[3 * f + 2];
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) depth_test(s_rec[3 * j], s_rec[3 * j + 1], s_rec[3 * j + 2].x, px, py, s_face[j], zmin, fmin);
    }
    if (col >= W || row >= H) return;
    const int64_t p = (int64_t)row * W + col;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    if (fmin >= 0) winner_bary(rec[3 * fmin], rec[3 * fmin + 1], rec[3 * fmin + 2].x, px, py, b0, b1, b2);
    if (face_id) face_id[p] = fmin;
    if (zbuf) zbuf[p] = zmin;
    if (bary) { bary[3 * p] = b0; bary[3 * p + 1] = b1; bary[3 * p + 2] = b2; }
    if (!rgba) return;
    if (fmin < 0) { rgba[p] = make_float4(1.f, 1.f, 1.f, 0.f); return; }
    const int i0 = faces[3 * fmin], i1 = faces[3 * fmin + 1], i2 = faces[3 * fmin + 2];
    float n[3], x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        n[k] = (b0 * vnrm[3 * i0 + k] + b1 * vnrm[3 * i1 + k]) + b2 * vnrm[3 * i2 + k];
        x[k] = (b0 * verts[3 * i0 + k] + b1 * verts[3 * i1 + k]) + b2 * verts[3 * i2 + k];
    }
    normalize3(n[0], n[1], n[2]);
    float l[3] = {sh.light[0] - x[0], sh.light[1] - x[1], sh.light[2] - x[2]};
    float w[3] = {sh.centre[0] - x[0], sh.centre[1] - x[1], sh.centre[2] - x[2]};
    normalize3(l[0], l[1], l[2]);
    normalize3(w[0], w[1], w[2]);
    const float nl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
    float spec = 0.f;
    if (nl > 0.f) {
        const float k2 = 2.f * nl;
        float a = fmaxf(((k2 * n[0] - l[0]) * w[0] + (k2 * n[1] - l[1]) * w[1]) + (k2 * n[2] - l[2]) * w[2], 0.f);
#pragma unroll
        for (int k = 0; k < 6; ++k) a *= a;                    // shininess 64 = six squarings
        spec = 0.2f * a;
    }
    const float c = (0.5f + 0.3f * fmaxf(nl, 0.f)) + spec;
    rgba[p] = make_float4(c, c, c, 1.f);
}

// rule 5: Image.alpha_composite with alpha 0 or 255 is a select; the byte is np.uint8(colour * 255), a truncation
__global__ void overlay_rgba8_kernel(const float4* __restrict__ rgba, const uint8_t* __restrict__ image, uint8_t* __restrict__ out, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float4 c = rgba[p];
    const bool on = c.w > 0.f;
    const float v[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * p + k] = on ? (uint8_t)fminf(fmaxf(v[k] * 255.f, 0.f), 255.f) : image[3 * p + k];
}

}  // namespace

namespace {

int raster_run(const char* who, nm_raster_s* h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W, int H,
               int32_t* face_id, float* zbuf, float* bary, const double* light, float4* rgba, hipStream_t st) {
    const int TX = (W + kTile - 1) / kTile, TY = (H + kTile - 1) / kTile, T = TX * TY;
    int rc = NM_OK;
    if ((rc = reserve_tiles(h, T))) return rc;
    int32_t *count = h->d_tiles, *offset = count + T, *cursor = offset + T + 1;
    const Cam cam = make_cam(w2c, fx, fy, cx, cy);
    Shade sh = {};
    if (rgba) {
        for (int k = 0; k < 3; ++k) {
            sh.light[k] = (float)light[k];
            sh.centre[k] = (float)-(w2c[k] * w2c[3] + w2c[4 + k] * w2c[7] + w2c[8 + k] * w2c[11]);      // C = -R^T t
        }
    }
    if ((rc = nm::check_hip(hipMemsetAsync(count, 0, (size_t)T * 4, st), "raster: memset(counts)"))) return rc;
    hipLaunchKernelGGL(raster_vertex_kernel, dim3((h->V + 255) / 256), dim3(256), 0, st, verts, h->d_faces, h->d_adj_off, h->d_adj, h->V, cam, rgba ? 1 : 0,
                       h->d_vscr, h->d_vnrm);
    hipLaunchKernelGGL(raster_face_kernel, dim3((h->F + 255) / 256), dim3(256), 0, st, h->d_vscr, h->d_faces, h->F, W, H, TX, h->d_rec, h->d_box, count);
    hipLaunchKernelGGL(raster_scan_kernel, dim3(1), dim3(256), 0, st, count, T, offset, cursor);
    if ((rc = nm::check_launch("raster setup kernels"))) return rc;
    // the one read-back: the lists' total length, so that their buffer is sized exactly and never by a guess
    int32_t total = 0;
    if ((rc = nm::check_hip(hipMemcpyAsync(&total, offset + T, 4, hipMemcpyDeviceToHost, st), "raster: read total"))) return rc;
    if ((rc = nm::check_hip(hipStreamSynchronize(st), "raster: sync"))) return rc;
    if (total < 0) { nm::set_error("%s: the tile lists overflow 2^31 entries", who); return NM_ERR_UNSUPPORTED; }
    if ((rc = reserve_lists(h, total))) return rc;
    if (total > 0) hipLaunchKernelGGL(raster_fill_kernel, dim3((h->F + 255) / 256), dim3(256), 0, st, h->d_box, h->F, TX, cursor, h->d_list, total);
    hipLaunchKernelGGL(raster_tile_kernel, dim3(T), dim3(kBatch), 0, st, h->d_rec, offset, h->d_list, h->d_faces, verts, h->d_vnrm, W, H, TX, sh, face_id, zbuf,
                       bary, rgba);
    return nm::check_launch("raster_tile_kernel");
}

}  // namespace

extern "C" {

int nm_raster_destroy(nm_raster_t h) {
    if (!h) return NM_OK;
    void* bufs[] = {h->d_faces, h->d_adj_off, h->d_adj, h->d_vscr, h->d_vnrm, h->d_rec, h->d_box, h->d_tiles, h->d_list, h->d_gface, h->d_bvscr,
                    h->d_brec, h->d_bbox, h->d_bcount, h->d_boffset, h->d_bgface, h->d_fvscr, h->d_fcount, h->d_foffset};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete h;
    return NM_OK;
}

int nm_raster_create(const int32_t* faces, int F, int V, nm_raster_t* out) {
    NM_REQUIRE(faces && out, "nm_raster_create: null pointer");
    NM_REQUIRE(V >= 1 && F >= 1 && F <= (1 << 24), "nm_raster_create: bad sizes V=%d F=%d", V, F);
    for (int64_t i = 0; i < 3ll * F; ++i)
        NM_REQUIRE(faces[i] >= 0 && faces[i] < V, "nm_raster_create: face %lld names vertex %d of %d", (long long)(i / 3), faces[i], V);
    // vertex -> faces, counting sort by vertex: faces are visited in ascending order, so every vertex's run is ascending too
    std::vector<int32_t> off((size_t)V + 1, 0), adj((size_t)3 * F);
    for (int64_t i = 0; i < 3ll * F; ++i) ++off[faces[i] + 1];
    for (int v = 0; v < V; ++v) off[v + 1] += off[v];
    {
        std::vector<int32_t> at(off.begin(), off.end() - 1);
        for (int f = 0; f < F; ++f)
            for (int k = 0; k < 3; ++k) adj[at[faces[3 * f + k]]++] = f;
    }
    nm_raster_s* h = new nm_raster_s();
    memset(h, 0, sizeof(*h));
    h->F = F; h->V = V;
    int rc = NM_OK;
#define NM_TRY(expr, what) if (!rc) rc = nm::check_hip((expr), what)
    NM_TRY(hipMalloc(&h->d_faces, (size_t)F * 12), "nm_raster_create: hipMalloc(faces)");
    NM_TRY(hipMalloc(&h->d_adj_off, ((size_t)V + 1) * 4), "nm_raster_create: hipMalloc(adjacency offsets)");
    NM_TRY(hipMalloc(&h->d_adj, (size_t)F * 12), "nm_raster_create: hipMalloc(adjacency)");
    NM_TRY(hipMalloc(&h->d_vscr, (size_t)V * sizeof(float4)), "nm_raster_create: hipMalloc(screen vertices)");
    NM_TRY(hipMalloc(&h->d_vnrm, (size_t)V * 12), "nm_raster_create: hipMalloc(normals)");
    NM_TRY(hipMalloc(&h->d_rec, (size_t)F * 3 * sizeof(float4)), "nm_raster_create: hipMalloc(records)");
    NM_TRY(hipMalloc(&h->d_box, (size_t)F * sizeof(int4)), "nm_raster_create: hipMalloc(boxes)");
    NM_TRY(hipMemcpy(h->d_faces, faces, (size_t)F * 12, hipMemcpyHostToDevice), "nm_raster_create: copy faces");
    NM_TRY(hipMemcpy(h->d_adj_off, off.data(), ((size_t)V + 1) * 4, hipMemcpyHostToDevice), "nm_raster_create: copy adjacency offsets");
    NM_TRY(hipMemcpy(h->d_adj, adj.data(), (size_t)F * 12, hipMemcpyHostToDevice), "nm_raster_create: copy adjacency");
#undef NM_TRY
    if (rc) { nm_raster_destroy(h); return rc; }
    *out = h;
    return NM_OK;
}

int nm_raster_mesh(nm_raster_t h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W, int H, int32_t* face_id,
                   float* zbuf, float* bary, nm_stream_t stream) {
    NM_RASTER_ARGS("nm_raster_mesh");
    NM_REQUIRE(face_id && zbuf, "nm_raster_mesh: null output");
    return raster_run("nm_raster_mesh", h, verts, w2c, fx, fy, cx, cy, W, H, face_id, zbuf, bary, nullptr, nullptr, nm::as_stream(stream));
}

int nm_raster_phong(nm_raster_t h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W, int H, int32_t* face_id,
                    float* zbuf, float* bary, const double* light, float* rgba, nm_stream_t stream) {
    NM_RASTER_ARGS("nm_raster_phong");
    NM_REQUIRE(light && rgba, "nm_raster_phong: null light or rgba");
    NM_REQUIRE((reinterpret_cast<uintptr_t>(rgba) & 15) == 0, "nm_raster_phong: rgba must be 16-byte aligned");
    return raster_run("nm_raster_phong", h, verts, w2c, fx, fy, cx, cy, W, H, face_id, zbuf, bary, light, reinterpret_cast<float4*>(rgba), nm::as_stream(stream));
}

int nm_overlay_rgba8(const float* rgba, const uint8_t* image, uint8_t* out, int64_t n, nm_stream_t stream) {
    NM_REQUIRE(n >= 1, "nm_overlay_rgba8: no pixels (n=%lld)", (long long)n);
    NM_REQUIRE(rgba && image && out, "nm_overlay_rgba8: null pointer");
    NM_REQUIRE((reinterpret_cast<uintptr_t>(rgba) & 15) == 0, "nm_overlay_rgba8: rgba must be 16-byte aligned");
    hipLaunchKernelGGL(overlay_rgba8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nm::as_stream(stream), reinterpret_cast<const float4*>(rgba), image, out, n);
    return nm::check_launch("overlay_rgba8_kernel");
}

}  // extern "C"
