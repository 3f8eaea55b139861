// Per-face colour lattices ("mesh colours"): the nodes of a regular barycentric grid of resolution R on every face of an indexed triangle mesh,
// filled from per-vertex rows -- include/neuman_hip.h 'mesh lattice', rules L1 and L2.  The reference has no such step; it is what lets a
// thinned mesh (mesh_simplify.hip) carry more colour samples than it has vertices.  The same kernel makes the nodes' positions from the
// vertices, their normals from the vertex normals (neuman_hip/mesh_texture.py evaluates a net there) and a lattice from per-vertex colours.
// Rule L3, the lookup, lives in raster_device.h beside the rasteriser that reads it (raster_frames.hip).  tests/helpers/mesh_lattice_ref.py
// restates L1-L3 in numpy.
//
//   one thread per (face, node), grid-stride over the F S nodes in 64 bits: the node's row i2 is found by walking the rows' lengths (at most
//   R steps), the three weights are (float)i_k / (float)R, and the thread writes its node's w columns.  The thread of a face's node 0
//   range-checks the face (mesh_device.h's invalid-face words); a face that fails is never dereferenced and none of its nodes is written.
//
// The pyramid of a lattice ('mesh mip', rule M1): level l has resolution R0 >> l while 2^l divides R0, coarse node (i1, i2) sits on fine node
// (2 i1, 2 i2), and its value is the transpose of linear prolongation on the triangular lattice -- restricted to the edge for an edge node, a copy
// for a corner, so that two faces that agree on a shared edge at level 0 agree on it at every level.  raster_frames.hip reads the pyramid
// (nm_raster_frames_lattice_mip); tests/helpers/mesh_mip_ref.py restates M1-M3 in numpy.
//
//   one launch per level, one thread per (face, coarse node), grid-stride as above: the thread finds its (i1, i2), reads one, three or seven
//   nodes of the finer level inside its own face's block and writes its node's w columns once.  No read-back: nothing is range-checked on
//   the device, since no index comes from memory.
#include "mesh_device.h"

namespace {

using namespace nm_mesh;

constexpr int kMaxR = 64;
constexpr unsigned kMaxBlocks = 1u << 20;                     // the grid of the grid-stride loop

__global__ void __launch_bounds__(kThreads) lattice_rows_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, const float* __restrict__ rows,
                                                                int w, int R, float* __restrict__ out, int64_t* __restrict__ hdr) {
    const int S = (R + 1) * (R + 2) / 2;
    const int64_t n = F * S, stride = (int64_t)gridDim.x * kThreads;
    const float fr = (float)R;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += stride) {
        const int64_t f = t / S;
        const int s = (int)(t - f * S);
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (!(in_range(a, V) && in_range(b, V) && in_range(c, V))) {
            if (s == 0) record_invalid_face(hdr, f);
            continue;
        }
        int i2 = 0, i1 = s;                                    // L1: row i2 has R + 1 - i2 entries
        while (i1 >= R + 1 - i2) { i1 -= R + 1 - i2; ++i2; }
        const float w0 = (float)(R - i1 - i2) / fr, w1 = (float)i1 / fr, w2 = (float)i2 / fr;
        const float *r0 = rows + (int64_t)a * w, *r1 = rows + (int64_t)b * w, *r2 = rows + (int64_t)c * w;
        float* o = out + t * w;
        for (int k = 0; k < w; ++k) o[k] = (w0 * r0[k] + w1 * r1[k]) + w2 * r2[k];                     // L2
    }
}

// S(R) summed over the levels before level l: where level l's block starts, in nodes per face
inline int64_t nodes_before(int R0, int l) {
    int64_t n = 0;
    for (int k = 0; k < l; ++k) n += ((R0 >> k) + 1) * ((R0 >> k) + 2) / 2;
    return n;
}

// the levels R0 allows: 1 + the trailing zero bits of R0
inline int levels_of(int R0) {
    int n = 1;
    while (!(R0 & 1)) { R0 >>= 1; ++n; }
    return n;
}

// M1: fine [F,S(2 R),w] -> coarse [F,S(R),w]
__global__ void __launch_bounds__(kThreads) lattice_reduce_kernel(const float* __restrict__ fine, int64_t F, int R, int w, float* __restrict__ coarse) {
    const int S = (R + 1) * (R + 2) / 2, Rf = 2 * R, Sf = (Rf + 1) * (Rf + 2) / 2;
    const int64_t n = F * S, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += stride) {
        const int64_t f = t / S;
        const int s = (int)(t - f * S);
        int i2 = 0, i1 = s;                                    // L1, as lattice_rows_kernel walks it
        while (i1 >= R + 1 - i2) { i1 -= R + 1 - i2; ++i2; }
        const int i0 = R - i1 - i2, j1 = 2 * i1, j2 = 2 * i2;
        const float* src = fine + f * Sf * w;
        auto at = [&](int a1, int a2) { return src + (int64_t)(a2 * (Rf + 1) - a2 * (a2 - 1) / 2 + a1) * w; };
        const float* c = at(j1, j2);
        float* o = coarse + t * w;
        const int zeros = (i0 == 0) + (i1 == 0) + (i2 == 0);
        if (zeros >= 2) {                                      // a corner: the fine node itself
            for (int k = 0; k < w; ++k) o[k] = c[k];
        } else if (zeros == 1) {                               // an edge node: the two fine neighbours along that edge, the smaller i1 (i2 on i1 = 0) first
            const float* a = i1 == 0 ? at(0, j2 - 1) : i2 == 0 ? at(j1 - 1, 0) : at(j1 - 1, j2 + 1);
            const float* b = i1 == 0 ? at(0, j2 + 1) : i2 == 0 ? at(j1 + 1, 0) : at(j1 + 1, j2 - 1);
            for (int k = 0; k < w; ++k) o[k] = 0.5f * c[k] + 0.25f * (a[k] + b[k]);
        } else {                                               // interior: all six fine neighbours exist
            const float *n0 = at(j1 + 1, j2), *n1 = at(j1, j2 + 1), *n2 = at(j1 - 1, j2 + 1), *n3 = at(j1 - 1, j2), *n4 = at(j1, j2 - 1), *n5 = at(j1 + 1, j2 - 1);
            for (int k = 0; k < w; ++k) o[k] = 0.25f * c[k] + 0.125f * (((((n0[k] + n1[k]) + n2[k]) + n3[k]) + n4[k]) + n5[k]);
        }
    }
}

}  // namespace

extern "C" {

int nm_mesh_lattice_rows(const int32_t* faces, int64_t F, int64_t V, const float* rows, int w, int R, float* out, nm_stream_t stream) {
    NM_REQUIRE(faces && rows && out, "nm_mesh_lattice_rows: null pointer");
    NM_REQUIRE(w >= 1, "nm_mesh_lattice_rows: w = %d columns (w >= 1)", w);
    NM_REQUIRE(R >= 1 && R <= kMaxR, "nm_mesh_lattice_rows: R = %d (1 <= R <= %d)", R, kMaxR);
    NM_REQUIRE(F >= 1 && V >= 1 && mesh_ok(V, F), "nm_mesh_lattice_rows: F = %lld faces over V = %lld vertices (1 <= V < 2^31, 1 <= 3 F < 2^31)",
               (long long)F, (long long)V);
    hipStream_t st = nm::as_stream(stream);
    int64_t* hdr = nullptr;                                    // the call's own 64 bytes: the entry takes no workspace
    int rc = NM_OK;
    if ((rc = nm::check_hip(hipMalloc(&hdr, (size_t)kHeaderBytes), "nm_mesh_lattice_rows: hipMalloc(header)"))) return rc;
    const int64_t n = F * ((R + 1) * (R + 2) / 2), blocks = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(reset_header_kernel, dim3(1), dim3(kThreads), 0, st, hdr);
    hipLaunchKernelGGL(lattice_rows_kernel, dim3((unsigned)(blocks < (int64_t)kMaxBlocks ? blocks : (int64_t)kMaxBlocks)), dim3(kThreads), 0, st, faces, F, V,
                       rows, w, R, out, hdr);
    int64_t head[3] = {0, 0, 0};
    if (!(rc = nm::check_launch("nm_mesh_lattice_rows: kernels"))) rc = read_header("nm_mesh_lattice_rows", hdr, head, 3, V, st);
    (void)hipFree(hdr);
    return rc;
}

int nm_mesh_lattice_pyramid_size(int R0, int levels, int64_t* nodes_per_face_total) {
    NM_REQUIRE(nodes_per_face_total, "nm_mesh_lattice_pyramid_size: null pointer");
    NM_REQUIRE(R0 >= 1 && R0 <= kMaxR, "nm_mesh_lattice_pyramid_size: R0 = %d (1 <= R0 <= %d)", R0, kMaxR);
    NM_REQUIRE(levels >= 1 && levels <= levels_of(R0), "nm_mesh_lattice_pyramid_size: levels = %d (R0 = %d allows 1 .. %d)", levels, R0, levels_of(R0));
    *nodes_per_face_total = nodes_before(R0, levels);
    return NM_OK;
}

int nm_mesh_lattice_pyramid(const float* lattice, int64_t F, int R0, int levels, int w, float* out, nm_stream_t stream) {
    NM_REQUIRE(lattice && out, "nm_mesh_lattice_pyramid: null pointer");
    NM_REQUIRE(w >= 1 && w <= 64, "nm_mesh_lattice_pyramid: w = %d columns (1 <= w <= 64)", w);
    NM_REQUIRE(R0 >= 1 && R0 <= kMaxR, "nm_mesh_lattice_pyramid: R0 = %d (1 <= R0 <= %d)", R0, kMaxR);
    NM_REQUIRE(levels >= 1 && levels <= levels_of(R0), "nm_mesh_lattice_pyramid: levels = %d (R0 = %d allows 1 .. %d)", levels, R0, levels_of(R0));
    NM_REQUIRE(F >= 1 && mesh_ok(1, F), "nm_mesh_lattice_pyramid: F = %lld faces (1 <= 3 F < 2^31)", (long long)F);
    hipStream_t st = nm::as_stream(stream);
    int rc = NM_OK;
    // level 0 is the input byte for byte; lattice == out is the in-place form, whose level 0 is already there
    if (lattice != out && (rc = nm::check_hip(hipMemcpyAsync(out, lattice, (size_t)(F * nodes_before(R0, 1) * w) * sizeof(float), hipMemcpyDeviceToDevice, st),
                                              "nm_mesh_lattice_pyramid: copy(level 0)")))
        return rc;
    for (int l = 1; l < levels; ++l) {
        const int R = R0 >> l;
        const int64_t n = F * ((R + 1) * (R + 2) / 2), blocks = (n + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(lattice_reduce_kernel, dim3((unsigned)(blocks < (int64_t)kMaxBlocks ? blocks : (int64_t)kMaxBlocks)), dim3(kThreads), 0, st,
                           out + F * nodes_before(R0, l - 1) * w, F, R, w, out + F * nodes_before(R0, l) * w);
    }
    return nm::check_launch("nm_mesh_lattice_pyramid: kernels");
}

}  // extern "C"
