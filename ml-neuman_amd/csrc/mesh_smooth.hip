// Smoothing of an indexed triangle mesh: the vertex -> incident faces adjacency, Taubin lambda|mu steps over it, and vertex normals from the mesh's
// own faces -- include/neuman_hip.h 'mesh smooth' writes the contract out (rules S1-S5); tests/helpers/mesh_smooth_ref.py restates it in numpy.
// What isosurface.hip extracts from a learned density is rippled at the scale of a grid cell; neuman_hip/mesh_smooth.py (adjacency, smooth_mesh,
// vertex_normals) smooths it without touching `faces`, and gives every posed frame of neuman_hip/mesh_pose.py the normals of its own geometry.
//
//   adjacency    count: every face range-checked BEFORE anything is indexed (invalid faces counted, their lowest index kept), a proper face adds
//                one to each of its three vertices' counters.  scan: mesh_device.h's span_rank_kernel over the counters and span_scan_kernel
//                over the spans' sums, then a launch here adds the span's offset: inc_off, and a copy of it as the fill's cursors.
//                fill: a proper face takes a slot of each of its vertices' lists through an integer atomicAdd on the cursor, so a list's ORDER
//                depends on the interleaving; finish: a thread per vertex sorts its list in place (insertion up to kSortInThread entries, heap
//                sort beyond: O(k log k), no second buffer), which makes the lists a function of the mesh alone.  The boundary flag comes from the
//                same sort: the 2k neighbour ids of a vertex's k faces, sorted; an id that occurs exactly once is an edge with one face.
//                Every launch after the first reads the invalid count and does nothing when it is not zero.
//   smooth       a thread per (vertex, column): one lane's loop over the list in list order, float64, Jacobi -- all steps of a call are launches
//                on one stream ping-ponging between `out` and `scratch`, no read-back.
//   normals      a thread per (frame, vertex), the frame a grid dimension: the sum of the incident faces' cross products in list order.
//
// Workspace: 4 bytes per vertex (counter, then cursor) + 24 bytes per face (six neighbour ids) + 16 bytes per kSpan vertices + 64.
#include "common.h"
#include "mesh_device.h"

#include <cmath>

namespace {

using namespace nm_mesh;                                      // the sizes, the header's protocol, the scan, the sort, the checks: mesh_device.h

enum { kHdrIncident = 0 };                                    // int64 word of the header beside kHdrInvalid and kHdrFirstInvalid

// ---- workspace --------------------------------------------------------------------------------------------------------------------------
struct Layout {
    int64_t vspans;
    int64_t off_sum, off_off, off_cursor, off_nbr, bytes;
};

inline Layout layout_of(int64_t V, int64_t F) {
    Layout L;
    L.vspans = spans_of(V);
    L.off_sum = kHeaderBytes;
    L.off_off = L.off_sum + L.vspans * 8;
    L.off_cursor = up16(L.off_off + L.vspans * 8);
    L.off_nbr = up16(L.off_cursor + V * 4);
    L.bytes = up16(L.off_nbr + F * 24);
    return L;
}

struct Work {
    int64_t* hdr;                                             // kHdr*
    int64_t *sum, *off;                                       // [vspans] the spans' sums and their exclusive scan
    int32_t* cursor;                                          // [V] proper faces naming the vertex; after the scan the fill's next free slot
    int32_t* nbr;                                             // [6F] per vertex (at 2 inc_off[v]) the neighbour ids of its faces
};

inline Work work_of(void* ws, const Layout& L) {
    char* b = static_cast<char*>(ws);
    Work w;
    w.hdr = reinterpret_cast<int64_t*>(b);
    w.sum = reinterpret_cast<int64_t*>(b + L.off_sum);
    w.off = reinterpret_cast<int64_t*>(b + L.off_off);
    w.cursor = reinterpret_cast<int32_t*>(b + L.off_cursor);
    w.nbr = reinterpret_cast<int32_t*>(b + L.off_nbr);
    return w;
}

// ---- adjacency --------------------------------------------------------------------------------------------------------------------------
// rule S1: the range check comes before any use of an index; only a proper face counts.  `count` was zeroed by the call.
__global__ void __launch_bounds__(kThreads) ms_count_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, int32_t* count, int64_t* hdr) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!(in_range(a, V) && in_range(b, V) && in_range(c, V))) {
        record_invalid_face(hdr, f);
        return;
    }
    if (a == b || a == c || b == c) return;
    atomicAdd(count + a, 1);
    atomicAdd(count + b, 1);
    atomicAdd(count + c, 1);
}

// after span_rank_kernel and span_scan_kernel: the in-span offset + the span's offset -> inc_off, and a copy as the fill's cursor
__global__ void __launch_bounds__(kThreads) ms_offset_kernel(int64_t V, int32_t* __restrict__ inc_off, int32_t* __restrict__ cursor,
                                                             const int64_t* __restrict__ span_off, const int64_t* __restrict__ hdr) {
    if (hdr[kHdrInvalid] != 0) return;
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const int32_t at = (int32_t)(span_off[v / kSpan] + inc_off[v]);
    inc_off[v] = at;
    cursor[v] = at;
}

// a proper face takes the next free slot of each of its three vertices (every face is valid here); the slot's number depends on the
// interleaving, the SET of a list's entries does not
__global__ void __launch_bounds__(kThreads) ms_fill_kernel(const int32_t* __restrict__ faces, int64_t F, int32_t* cursor, int32_t* __restrict__ inc,
                                                          const int64_t* __restrict__ hdr) {
    if (hdr[kHdrInvalid] != 0) return;
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a == b || a == c || b == c) return;
    const int32_t v[3] = {a, b, c};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t at = atomicAdd(cursor + v[k], 1);
        if (at >= 0 && at < 3 * F) inc[at] = (int32_t)f;
    }
}

// rule S2: the list in ascending face index; boundary[v] = some neighbour shares exactly one proper face with v
__global__ void __launch_bounds__(kThreads) ms_finish_kernel(const int32_t* __restrict__ faces, int64_t V, const int32_t* __restrict__ inc_off, int32_t* inc,
                                                            int32_t* nbr, uint8_t* __restrict__ boundary, const int64_t* __restrict__ hdr) {
    if (hdr[kHdrInvalid] != 0) return;
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const int32_t lo = inc_off[v];
    const int k = inc_off[v + 1] - lo;
    sort_segment(inc + lo, k);
    if (!boundary) return;
    int32_t* mine = nbr + 2 * (int64_t)lo;
    for (int i = 0; i < k; ++i) {
        const int64_t f = inc[lo + i];
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        mine[2 * i] = a == (int32_t)v ? b : a;                 // the two vertices of the face that are not v
        mine[2 * i + 1] = c == (int32_t)v ? b : c;
    }
    sort_segment(mine, 2 * k);
    bool open = false;
    for (int i = 0; i < 2 * k;) {
        const int32_t u = mine[i];
        int j = i + 1;
        while (j < 2 * k && mine[j] == u) ++j;
        open = open || j - i == 1;
        i = j;
    }
    boundary[v] = open ? 1 : 0;
}

// ---- smooth -----------------------------------------------------------------------------------------------------------------------------
// rule S3, one thread per (vertex, column).  An offset, a face index or a vertex index out of range is never followed: the entry is skipped,
// and a vertex none of whose entries can be followed keeps its bits.
__global__ void __launch_bounds__(kThreads) ms_step_kernel(const float* __restrict__ x, int width, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                                          const int32_t* __restrict__ inc_off, const int32_t* __restrict__ inc,
                                                          const uint8_t* __restrict__ hold, float t, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= V * width) return;
    const int64_t v = e / width;
    const int col = (int)(e - v * width);
    const float own = x[e];
    float result = own;
    const int64_t lo = inc_off[v], hi = inc_off[v + 1];
    if (!(hold && hold[v] != 0) && lo >= 0 && hi <= 3 * F && lo < hi) {
        double s = 0.0;
        int64_t k = 0;
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t f = inc[i];
            if (!in_range(f, F)) continue;
            const int32_t a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
            int32_t p, q;                                      // the face rotated so that v comes first: (v, p, q)
            if ((int64_t)a == v) { p = b; q = c; }
            else if ((int64_t)b == v) { p = c; q = a; }
            else if ((int64_t)c == v) { p = a; q = b; }
            else continue;
            if (!in_range(p, V) || !in_range(q, V)) continue;
            s = (s + (double)x[(int64_t)p * width + col]) + (double)x[(int64_t)q * width + col];
            ++k;
        }
        if (k > 0) {
            const double m = s / (double)(2 * k);
            const double d = m - (double)own;
            result = (float)((double)own + (double)t * d);
        }
    }
    out[e] = result;
}

// ---- normals ----------------------------------------------------------------------------------------------------------------------------
// rule S5, one thread per (frame, vertex); frames beyond the grid's second dimension are taken in strides of it
__global__ void __launch_bounds__(kThreads) ms_normals_kernel(const float* __restrict__ verts, int64_t B, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                                             const int32_t* __restrict__ inc_off, const int32_t* __restrict__ inc,
                                                             float* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    int64_t lo = inc_off[v], hi = inc_off[v + 1];
    if (lo < 0 || hi > 3 * F) hi = lo;
    for (int64_t frame = blockIdx.y; frame < B; frame += gridDim.y) {
        const float* x = verts + frame * V * 3;
        double nx = 0.0, ny = 0.0, nz = 0.0;
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t f = inc[i];
            if (!in_range(f, F)) continue;
            const int32_t a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
            if (!in_range(a, V) || !in_range(b, V) || !in_range(c, V)) continue;
            const double ax = x[3 * (int64_t)a], ay = x[3 * (int64_t)a + 1], az = x[3 * (int64_t)a + 2];
            const double ux = (double)x[3 * (int64_t)b] - ax, uy = (double)x[3 * (int64_t)b + 1] - ay, uz = (double)x[3 * (int64_t)b + 2] - az;
            const double wx = (double)x[3 * (int64_t)c] - ax, wy = (double)x[3 * (int64_t)c + 1] - ay, wz = (double)x[3 * (int64_t)c + 2] - az;
            nx += uy * wz - uz * wy;
            ny += uz * wx - ux * wz;
            nz += ux * wy - uy * wx;
        }
        const double l2 = (nx * nx + ny * ny) + nz * nz;
        float* o = normals + (frame * V + v) * 3;
        if (l2 > 0.0 && l2 <= 1.7976931348623157e308) {        // finite and positive (a NaN compares false)
            const double l = sqrt(l2);
            o[0] = (float)(nx / l);
            o[1] = (float)(ny / l);
            o[2] = (float)(nz / l);
        } else {
            o[0] = 0.f;
            o[1] = 0.f;
            o[2] = 0.f;
        }
    }
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------------
#define NM_MS_MESH(who)                                                                                                                      \
    NM_REQUIRE(mesh_ok(V, F), who ": V = %lld, F = %lld: V and 3 F must be in [0, 2^31)", (long long)V, (long long)F);                      \
    NM_REQUIRE(faces || F == 0, who ": null faces")
#define NM_MS_LISTS(who)                                                                                                                     \
    NM_REQUIRE(inc_off, who ": null inc_off");                                                                                               \
    NM_REQUIRE(inc || F == 0, who ": null inc")

}  // namespace

extern "C" {

int64_t nm_mesh_adjacency_workspace_bytes(int64_t V, int64_t F) {
    if (!mesh_ok(V, F)) {
        nm::set_error("nm_mesh_adjacency_workspace_bytes: V = %lld, F = %lld: V and 3 F must be in [0, 2^31)", (long long)V, (long long)F);
        return NM_ERR_ARG;
    }
    return layout_of(V, F).bytes;
}

int nm_mesh_adjacency(const int32_t* faces, int64_t F, int64_t V, int32_t* inc_off, int32_t* inc, uint8_t* boundary, void* workspace,
                      int64_t workspace_bytes, int64_t* n_incident, nm_stream_t stream) {
    NM_MS_MESH("nm_mesh_adjacency");
    NM_MS_LISTS("nm_mesh_adjacency");
    NM_REQUIRE(n_incident, "nm_mesh_adjacency: null count pointer");
    const Layout L = layout_of(V, F);
    NM_MESH_WORKSPACE("nm_mesh_adjacency", L.bytes);
    const Work w = work_of(workspace, L);
    hipStream_t st = nm::as_stream(stream);
    int rc = NM_OK;
    if (V > 0 && (rc = nm::check_hip(hipMemsetAsync(w.cursor, 0, (size_t)V * 4, st), "nm_mesh_adjacency: clear counters"))) return rc;
    hipLaunchKernelGGL(reset_header_kernel, dim3(1), dim3(64), 0, st, w.hdr);
    if (F > 0) hipLaunchKernelGGL(ms_count_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, faces, F, V, w.cursor, w.hdr);
    if (V > 0)
        hipLaunchKernelGGL(span_rank_kernel<Counters>, dim3((unsigned)L.vspans), dim3(kThreads), 0, st, Counters{w.cursor}, V, inc_off, 0, w.sum, w.hdr + kHdrInvalid);
    hipLaunchKernelGGL(span_scan_kernel, dim3(1), dim3(kThreads), 0, st, w.sum, L.vspans, w.off, w.hdr + kHdrIncident, inc_off + V, w.hdr + kHdrInvalid);
    if (V > 0) {
        hipLaunchKernelGGL(ms_offset_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, V, inc_off, w.cursor, w.off, w.hdr);
        if (F > 0) hipLaunchKernelGGL(ms_fill_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, faces, F, w.cursor, inc, w.hdr);
        hipLaunchKernelGGL(ms_finish_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, faces, V, inc_off, inc, w.nbr, boundary, w.hdr);
    }
    if ((rc = nm::check_launch("mesh adjacency kernels"))) return rc;
    int64_t head[3] = {0, 0, 0};                               // the one read-back: {n_incident, n_invalid, first_invalid}
    if ((rc = read_header("nm_mesh_adjacency", w.hdr, head, 3, V, st))) return rc;
    *n_incident = head[kHdrIncident];
    return NM_OK;
}

int nm_mesh_smooth(const float* rows, int width, int64_t V, const int32_t* faces, int64_t F, const int32_t* inc_off, const int32_t* inc,
                   const uint8_t* hold, float lambda, float mu, int iterations, float* out, float* scratch, nm_stream_t stream) {
    NM_MS_MESH("nm_mesh_smooth");
    NM_REQUIRE(width >= 1 && width <= 64, "nm_mesh_smooth: width = %d must be in 1..64", width);
    NM_REQUIRE(iterations >= 0, "nm_mesh_smooth: iterations = %d must be >= 0", iterations);
    NM_REQUIRE(std::isfinite(lambda) && std::isfinite(mu), "nm_mesh_smooth: lambda = %g, mu = %g: both must be finite", (double)lambda, (double)mu);
    if (V == 0) return NM_OK;
    NM_MS_LISTS("nm_mesh_smooth");
    NM_REQUIRE(rows && out && scratch, "nm_mesh_smooth: null rows, out or scratch");
    const int64_t n = V * width, bytes = n * 4;
    NM_REQUIRE(!overlap(rows, bytes, out, bytes) && !overlap(rows, bytes, scratch, bytes) && !overlap(out, bytes, scratch, bytes),
               "nm_mesh_smooth: rows, out and scratch must be three distinct buffers of V x width floats");
    hipStream_t st = nm::as_stream(stream);
    const int steps = mu != 0.f ? 2 : 1;
    if (iterations == 0) return nm::check_hip(hipMemcpyAsync(out, rows, (size_t)bytes, hipMemcpyDeviceToDevice, st), "nm_mesh_smooth: copy");
    const int64_t total = (int64_t)iterations * steps;
    const float* src = rows;
    for (int64_t j = 0; j < total; ++j) {
        float* dst = ((total - 1 - j) & 1) ? scratch : out;   // by parity, so that the last step writes `out`
        const float t = (steps == 2 && (j & 1)) ? mu : lambda;
        hipLaunchKernelGGL(ms_step_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, src, width, V, faces, F, inc_off, inc, hold, t, dst);
        src = dst;
    }
    return nm::check_launch("mesh smoothing kernels");
}

int nm_mesh_vertex_normals(const float* verts, int64_t B, int64_t V, const int32_t* faces, int64_t F, const int32_t* inc_off, const int32_t* inc,
                           float* normals, nm_stream_t stream) {
    NM_MS_MESH("nm_mesh_vertex_normals");
    NM_REQUIRE(B >= 1 && B < (1ll << 31) && B * V < (1ll << 31), "nm_mesh_vertex_normals: B = %lld, V = %lld: B >= 1 and B V < 2^31", (long long)B,
               (long long)V);
    if (V == 0) return NM_OK;
    NM_MS_LISTS("nm_mesh_vertex_normals");
    NM_REQUIRE(verts && normals, "nm_mesh_vertex_normals: null verts or normals");
    NM_REQUIRE(!overlap(verts, B * V * 12, normals, B * V * 12), "nm_mesh_vertex_normals: verts and normals must be distinct buffers");
    const unsigned frames = (unsigned)(B < 65535 ? B : 65535);
    hipLaunchKernelGGL(ms_normals_kernel, dim3(blocks_for(V), frames), dim3(kThreads), 0, nm::as_stream(stream), verts, B, V, faces, F, inc_off, inc, normals);
    return nm::check_launch("mesh vertex normals kernel");
}

}  // extern "C"
