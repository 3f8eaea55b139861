// The frames of an animated mesh as images: the mesh rasteriser (raster.hip) over B frames of one topology in one call, with per-vertex colours,
// a diffuse light on SUPPLIED per-frame normals, a depth test against a background and byte egress -- include/neuman_hip.h 'mesh frames', rules
// F1-F7 on top of the rasteriser's rules 1-3.  The reference has no such step; it is what shows the mesh that mesh_extract made and mesh_pose
// animated.  tests/helpers/raster_frames_ref.py restates F2-F5 in float64 on top of tests/helpers/raster_ref.py.
//
//   vertex pass    one thread per (frame, vertex): raster_device.h's project_vertex on the frame's camera, read from device memory; a frame whose
//                  camera has a non-finite entry gets (0, 0, 0, 0) everywhere, which drops every face of it
//   count          one thread per (frame, face): tile_box (rule 2's rejection, the tiles the screen box touches), one integer atomic per tile
//   scan           one workgroup: 64-bit exclusive offsets of the B T counts, their total and the bad-camera word beside it (the call's one
//                  read-back); the counts are cleared on the way out and serve as the fill's cursors
//   fill           the count pass again (the boxes are recomputed, not stored), writing the face into its tiles' lists
//   raster + shade one 256-thread workgroup per (frame, tile), one pixel per lane: the list goes through LDS 256 faces at a time, gathered from the
//                  frame's screen vertices; every lane keeps its (z, face) minimum in registers (raster_device.h's depth_test, the one-frame
//                  kernel's), recomputes the winner's barycentrics (winner_bary), blends colours, lights, tests against bg_z and stores bytes
//
// No per-frame face records or boxes are kept: a record is nine of the twelve floats of the face's three screen vertices, so the tile kernel
// reads those instead, and frame b's depth test sees the bits the one-frame kernel sees.  Scratch is 16 V bytes per frame, not 16 V + 64 F.
// The order inside a (frame, tile) list is whatever the atomics made it; the minimum over (z, face id) does not depend on it.
//
// nm_raster_frames_lattice is the same call with rule F2 replaced by F2': the colour comes from the winning face's colour lattice ('mesh
// lattice', rule L3; raster_device.h's lattice_colour) at the winner's barycentrics.  frames_tile_kernel is one body with the colour source as
// a template argument; every other kernel and the host code serve both entries.  The lattice stays [F,S,3] as the caller made it: a pixel
// reads three nodes of 12 bytes inside its face's 12 S bytes, neighbouring pixels of a face read the same or neighbouring nodes, so a wave's
// nine loads fall into a few cache lines that the tile's other waves and the next frames' tiles find in L2.
//
// nm_raster_frames_lattice_mip is the same call again with rule F2'' ('mesh mip', rules M2 and M3; raster_device.h's lattice_level and
// pyramid_colour): the colour comes from a pyramid of the lattice (mesh_lattice.hip), at a level chosen per frame and face from the winner's
// three screen vertices -- the ones the depth test read -- and blended towards the next coarser level.  The colour source is a three-valued
// template argument; a pixel reads three nodes of one level or of two.
#include "raster_device.h"

namespace {

using namespace nm_rast;

constexpr int kScanThreads = 1024;           // the one workgroup of frames_scan_kernel

struct Frames {
    int B, V, F, W, H, TX, T;
    int lit;                                 // normals and light were given
    int R;                                   // the colour lattice's resolution (level 0's for a pyramid), else 0
    int levels;                              // the pyramid's levels (frames_tile_kernel<kPyramid>), else 0
    float lod_scale;                         // rule M2's factor
    float light[3];                          // world space
};

// frame b's camera from device memory: w2c [B,4,4] (rows 0-2 are used), intr [B,4] = (fx, fy, cx, cy); false: a non-finite entry
__device__ __forceinline__ bool frame_cam(const double* __restrict__ w2c, const double* __restrict__ intr, int b, Cam& cam) {
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

__global__ void frames_vertex_kernel(const float* __restrict__ verts, const double* __restrict__ w2c, const double* __restrict__ intr, int V,
                                     float4* __restrict__ vscr) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (v >= V) return;
    Cam cam;
    const bool ok = frame_cam(w2c, intr, b, cam);
    vscr[(size_t)b * V + v] = ok ? project_vertex(verts + (size_t)b * V * 3, v, cam) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// kFill = false: count[b T + tile] += 1 for every tile of the face's box; true: the same walk, list[offset[b T + tile] + cursor++] = f (the
// positions come from the boxes the counts came from, so they stay below the next tile's offset and below `total`)
template <bool kFill>
__global__ void frames_bin_kernel(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, Frames fr, int32_t* __restrict__ count,
                                  const int64_t* __restrict__ offset, int32_t* __restrict__ list, int64_t total) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (f >= fr.F) return;
    const float4* vs = vscr + (size_t)b * fr.V;
    const int4 bx = tile_box(vs[faces[3 * f]], vs[faces[3 * f + 1]], vs[faces[3 * f + 2]], fr.W, fr.H);
    for (int ty = bx.y; ty <= bx.w; ++ty)
        for (int tx = bx.x; tx <= bx.z; ++tx) {
            const int64_t g = (int64_t)b * fr.T + ty * fr.TX + tx;
            const int at = atomicAdd(&count[g], 1);
            if (kFill) {
                const int64_t to = offset[g] + at;
                if (to < total) list[to] = f;
            }
        }
}

// exclusive scan of the n = B T counts by one workgroup into 64-bit offsets: offset[0 .. n], offset[n] the total; offset[n + 1] = 1 + the first
// frame whose camera has a non-finite entry, 0 if none -- the two words the host reads back.  count[] leaves as zeros: the fill's cursors
__global__ void __launch_bounds__(kScanThreads) frames_scan_kernel(int32_t* __restrict__ count, int64_t n, const double* __restrict__ w2c,
                                                                   const double* __restrict__ intr, int B, int64_t* __restrict__ offset) {
    __shared__ int64_t part[kScanThreads];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = B;
    const int64_t per = (n + kScanThreads - 1) / kScanThreads, lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += kScanThreads) {
        Cam cam;
        if (!frame_cam(w2c, intr, b, cam)) atomicMin(&s_bad, b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < kScanThreads; ++i) { const int64_t t = part[i]; part[i] = run; run += t; }
        offset[n] = run;
        offset[n + 1] = s_bad < B ? s_bad + 1 : 0;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) { offset[i] = run; run += count[i]; count[i] = 0; }
}

// a face's record as raster.hip keeps it, from the frame's screen vertices: (x0, y0, x1, y1), (x2, y2, 1/z0, 1/z1), 1/z2
__device__ __forceinline__ void face_record(const float4* __restrict__ vs, const int32_t* __restrict__ faces, int f, float4& r0, float4& r1, float& iz2) {
    const float4 a = vs[faces[3 * f]], b = vs[faces[3 * f + 1]], c = vs[faces[3 * f + 2]];
    r0 = make_float4(a.x, a.y, b.x, b.y);
    r1 = make_float4(c.x, c.y, a.z, b.z);
    iz2 = c.z;
}

// rule F5's byte: truncation; fmaxf returns its other operand for a NaN, so a NaN gives 0
__device__ __forceinline__ uint8_t colour_byte(float c) { return (uint8_t)fminf(fmaxf(c * 255.f, 0.f), 255.f); }

// the colour source.  kVertex: `colours` is [V,3], rule F2 (null: white); kLattice: `colours` is the faces' lattice [F,S,3] of resolution
// fr.R, rule F2'; kPyramid: `colours` is that lattice's pyramid of fr.levels levels, rule F2''
enum Source { kVertex = 0, kLattice = 1, kPyramid = 2 };

template <int kSource>
__global__ void __launch_bounds__(kBatch) frames_tile_kernel(const float4* __restrict__ vscr, const int32_t* __restrict__ faces, const int64_t* __restrict__ offset,
                                                            const int32_t* __restrict__ list, const float* __restrict__ verts,
                                                            const float* __restrict__ colours, const float* __restrict__ normals, Frames fr,
                                                            const uint8_t* __restrict__ bg, const float* __restrict__ bg_z, uint8_t* __restrict__ out,
                                                            int32_t* __restrict__ face_id, float* __restrict__ zbuf, float* __restrict__ bary) {
    __shared__ float4 s_r0[kBatch], s_r1[kBatch];
    __shared__ float s_iz2[kBatch];
    __shared__ int s_face[kBatch];
    const int tile = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const float4* vs = vscr + (size_t)b * fr.V;
    const int col = (tile % fr.TX) * kTile + (lane % kTile), row = (tile / fr.TX) * kTile + (lane / kTile);
    const float px = (float)col + 0.5f, py = (float)row + 0.5f;
    const int64_t g = (int64_t)b * fr.T + tile;
    const int64_t begin = offset[g], end = offset[g + 1];
    float zmin = INFINITY;
    int fmin = -1;
    for (int64_t base = begin; base < end; base += kBatch) {
        const int n = (int)(end - base < (int64_t)kBatch ? end - base : (int64_t)kBatch);
        __syncthreads();                                       // the previous batch has been read
        if (lane < n) {
            const int f = list[base + lane];
            s_face[lane] = f;
            face_record(vs, faces, f, s_r0[lane], s_r1[lane], s_iz2[lane]);
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) depth_test(s_r0[j], s_r1[j], s_iz2[j], px, py, s_face[j], zmin, fmin);
    }
    if (col >= fr.W || row >= fr.H) return;
    const size_t p = (size_t)b * fr.W * fr.H + (size_t)row * fr.W + col;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    float4 r0, r1;                                             // the winner's record: kPyramid reads its screen vertices again below
    if (fmin >= 0) {
        float iz2;
        face_record(vs, faces, fmin, r0, r1, iz2);
        winner_bary(r0, r1, iz2, px, py, b0, b1, b2);
    }
    if (face_id) face_id[p] = fmin;
    if (zbuf) zbuf[p] = zmin;
    if (bary) { bary[3 * p] = b0; bary[3 * p + 1] = b1; bary[3 * p + 2] = b2; }
    // F4: the comparison is strict and false for a NaN
    if (fmin < 0 || (bg_z && !(zmin < bg_z[p]))) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * p + k] = bg ? bg[3 * p + k] : (uint8_t)255;
        return;
    }
    const int i0 = faces[3 * fmin], i1 = faces[3 * fmin + 1], i2 = faces[3 * fmin + 2];
    float c[3] = {1.f, 1.f, 1.f};                               // F2: no colours is white itself, not a blend of ones
    if (kSource == kPyramid) {                                 // F2'': rule M2's level of this frame's face, rule M3 at the winner's b'
        float t;
        const int l = lattice_level(r0, r1, fr.R, fr.levels, fr.lod_scale, t);
        pyramid_colour(colours, fr.F, fmin, fr.R, l, t, b1, b2, c);
    } else if (kSource == kLattice) {                          // F2': rule L3 at the winner's b'
        lattice_colour(colours + (size_t)fmin * (size_t)(3 * ((fr.R + 1) * (fr.R + 2) / 2)), fr.R, b1, b2, c);
    } else if (colours) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (b0 * colours[3 * i0 + k] + b1 * colours[3 * i1 + k]) + b2 * colours[3 * i2 + k];
    }
    if (fr.lit) {                                              // F3: rule 4's n, p and l on the supplied normals
        const float* vw = verts + (size_t)b * fr.V * 3;
        const float* nw = normals + (size_t)b * fr.V * 3;
        float n[3], l[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            n[k] = (b0 * nw[3 * i0 + k] + b1 * nw[3 * i1 + k]) + b2 * nw[3 * i2 + k];
            l[k] = fr.light[k] - ((b0 * vw[3 * i0 + k] + b1 * vw[3 * i1 + k]) + b2 * vw[3 * i2 + k]);
        }
        normalize3(n[0], n[1], n[2]);
        normalize3(l[0], l[1], l[2]);
        const float nl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2];
        const float shade = 0.5f + 0.5f * fmaxf(nl, 0.f);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] *= shade;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * p + k] = colour_byte(c[k]);
}

// the call's scratch: screen vertices for B frames, counts and offsets for B T tiles; both only grow
int reserve_frames(nm_raster_s* h, int B, int T) {
    int rc = NM_OK;
    if (B > h->frames_cap) {
        if (h->d_fvscr) (void)hipFree(h->d_fvscr);
        h->d_fvscr = nullptr; h->frames_cap = 0;
        if ((rc = nm::check_hip(hipMalloc(&h->d_fvscr, (size_t)B * h->V * sizeof(float4)), "nm_raster_frames: hipMalloc(screen vertices)"))) return rc;
        h->frames_cap = B;
    }
    const int64_t n = (int64_t)B * T;
    if (n > h->ftiles_cap) {
        if (h->d_fcount) (void)hipFree(h->d_fcount);
        if (h->d_foffset) (void)hipFree(h->d_foffset);
        h->d_fcount = nullptr; h->d_foffset = nullptr; h->ftiles_cap = 0;
        if ((rc = nm::check_hip(hipMalloc(&h->d_fcount, (size_t)n * 4), "nm_raster_frames: hipMalloc(counts)"))) return rc;
        if ((rc = nm::check_hip(hipMalloc(&h->d_foffset, (size_t)(n + 2) * 8), "nm_raster_frames: hipMalloc(offsets)"))) return rc;
        h->ftiles_cap = n;
    }
    return NM_OK;
}

// the three entries: R = 0 is nm_raster_frames (colours [V,3], nullable), R >= 1 and levels = 0 nm_raster_frames_lattice (colours [F,S,3]),
// levels >= 1 nm_raster_frames_lattice_mip (colours the pyramid of a lattice of resolution R)
int raster_frames(const char* who, nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H, const float* colours, int R,
                  int levels, float lod_scale, const float* normals, const double* light, const uint8_t* bg, const float* bg_z, uint8_t* out, int32_t* face_id, float* zbuf,
                  float* bary, nm_stream_t stream) {
    NM_REQUIRE(B >= 1 && B <= 65535, "%s: B = %d frames (1 <= B <= 65535)", who, B);
    NM_REQUIRE(W >= 1 && H >= 1 && (int64_t)W * H <= (1ll << 30), "%s: bad image size W=%d H=%d", who, W, H);
    NM_REQUIRE((normals != nullptr) == (light != nullptr), "%s: normals and light go together (normals %s, light %s)", who, normals ? "given" : "null",
               light ? "given" : "null");
    NM_REQUIRE(!light || (isfinite(light[0]) && isfinite(light[1]) && isfinite(light[2])), "%s: a non-finite light", who);
    hipStream_t st = nm::as_stream(stream);
    Frames fr = {};
    fr.B = B; fr.V = h->V; fr.F = h->F; fr.W = W; fr.H = H;
    fr.TX = (W + kTile - 1) / kTile;
    fr.T = fr.TX * ((H + kTile - 1) / kTile);
    fr.lit = normals ? 1 : 0;
    fr.R = R;
    fr.levels = levels;
    fr.lod_scale = lod_scale;
    for (int k = 0; k < 3; ++k) fr.light[k] = light ? (float)light[k] : 0.f;
    const int64_t n = (int64_t)B * fr.T;
    int rc = NM_OK;
    if ((rc = reserve_frames(h, B, fr.T))) return rc;
    const dim3 per_vertex((h->V + 255) / 256, B), per_face((h->F + 255) / 256, B);
    if ((rc = nm::check_hip(hipMemsetAsync(h->d_fcount, 0, (size_t)n * 4, st), "nm_raster_frames: memset(counts)"))) return rc;
    hipLaunchKernelGGL(frames_vertex_kernel, per_vertex, dim3(256), 0, st, verts, w2c, intr, h->V, h->d_fvscr);
    hipLaunchKernelGGL(frames_bin_kernel<false>, per_face, dim3(256), 0, st, h->d_fvscr, h->d_faces, fr, h->d_fcount, (const int64_t*)nullptr, (int32_t*)nullptr,
                       (int64_t)0);
    hipLaunchKernelGGL(frames_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, h->d_fcount, n, w2c, intr, B, h->d_foffset);
    if ((rc = nm::check_launch("nm_raster_frames: setup kernels"))) return rc;
    // the one read-back of the call: the lists' total length (64-bit: a batch can pass 2^31 entries) and the bad-camera word beside it
    int64_t back[2] = {0, 0};
    if ((rc = nm::check_hip(hipMemcpyAsync(back, h->d_foffset + n, 16, hipMemcpyDeviceToHost, st), "nm_raster_frames: read total"))) return rc;
    if ((rc = nm::check_hip(hipStreamSynchronize(st), "nm_raster_frames: sync"))) return rc;
    const int64_t total = back[0];
    if (total < 0 || (total + n - 1) / n > h->F) {                 // (total > n F, without the product)
        nm::set_error("%s: bad list total %lld", who, (long long)total); return NM_ERR_UNSUPPORTED; }
    if ((rc = reserve_lists(h, total))) return rc;
    if (total > 0) hipLaunchKernelGGL(frames_bin_kernel<true>, per_face, dim3(256), 0, st, h->d_fvscr, h->d_faces, fr, h->d_fcount, h->d_foffset, h->d_list, total);
    if (levels > 0)
        hipLaunchKernelGGL(frames_tile_kernel<kPyramid>, dim3(fr.T, B), dim3(kBatch), 0, st, h->d_fvscr, h->d_faces, h->d_foffset, h->d_list, verts, colours, normals, fr,
                           bg, bg_z, out, face_id, zbuf, bary);
    else if (R > 0)
        hipLaunchKernelGGL(frames_tile_kernel<kLattice>, dim3(fr.T, B), dim3(kBatch), 0, st, h->d_fvscr, h->d_faces, h->d_foffset, h->d_list, verts, colours, normals, fr,
                           bg, bg_z, out, face_id, zbuf, bary);
    else
        hipLaunchKernelGGL(frames_tile_kernel<kVertex>, dim3(fr.T, B), dim3(kBatch), 0, st, h->d_fvscr, h->d_faces, h->d_foffset, h->d_list, verts, colours, normals, fr,
                           bg, bg_z, out, face_id, zbuf, bary);
    if ((rc = nm::check_launch("nm_raster_frames: frames_tile_kernel"))) return rc;
    // (the bad frame's outputs are defined all the same: its lists are empty, so face_id -1, zbuf +inf and out the background)
    NM_REQUIRE(back[1] == 0, "%s: a non-finite w2c or intrinsic entry in frame %lld", who, (long long)(back[1] - 1));
    return NM_OK;
}

}  // namespace

extern "C" {

int nm_raster_frames(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H, const float* colours,
                     const float* normals, const double* light, const uint8_t* bg, const float* bg_z, uint8_t* out, int32_t* face_id, float* zbuf,
                     float* bary, nm_stream_t stream) {
    NM_REQUIRE(h && verts && w2c && intr && out, "nm_raster_frames: null pointer");
    return raster_frames("nm_raster_frames", h, verts, w2c, intr, B, W, H, colours, 0, 0, 0.f, normals, light, bg, bg_z, out, face_id, zbuf, bary, stream);
}

int nm_raster_frames_lattice(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H, const float* face_colours,
                             int R, const float* normals, const double* light, const uint8_t* bg, const float* bg_z, uint8_t* out, int32_t* face_id,
                             float* zbuf, float* bary, nm_stream_t stream) {
    NM_REQUIRE(h && verts && w2c && intr && out && face_colours, "nm_raster_frames_lattice: null pointer");
    NM_REQUIRE(R >= 1 && R <= 64, "nm_raster_frames_lattice: R = %d (1 <= R <= 64)", R);
    return raster_frames("nm_raster_frames_lattice", h, verts, w2c, intr, B, W, H, face_colours, R, 0, 0.f, normals, light, bg, bg_z, out, face_id, zbuf, bary, stream);
}

int nm_raster_frames_lattice_mip(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H, const float* pyramid, int R0,
                                 int levels, float lod_scale, const float* normals, const double* light, const uint8_t* bg, const float* bg_z, uint8_t* out,
                                 int32_t* face_id, float* zbuf, float* bary, nm_stream_t stream) {
    NM_REQUIRE(h && verts && w2c && intr && out && pyramid, "nm_raster_frames_lattice_mip: null pointer");
    NM_REQUIRE(R0 >= 1 && R0 <= 64, "nm_raster_frames_lattice_mip: R0 = %d (1 <= R0 <= 64)", R0);
    NM_REQUIRE(levels >= 1 && levels <= 7 && (R0 & ((1 << (levels - 1)) - 1)) == 0, "nm_raster_frames_lattice_mip: levels = %d (>= 1, and 2^(levels-1) divides R0 = %d)",
               levels, R0);
    NM_REQUIRE(isfinite(lod_scale) && lod_scale >= 0.f, "nm_raster_frames_lattice_mip: lod_scale = %g (finite, >= 0)", (double)lod_scale);
    return raster_frames("nm_raster_frames_lattice_mip", h, verts, w2c, intr, B, W, H, pyramid, R0, levels, lod_scale, normals, light, bg, bg_z, out, face_id, zbuf,
                         bary, stream);
}

}  // extern "C"
