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

}  // extern "C"
