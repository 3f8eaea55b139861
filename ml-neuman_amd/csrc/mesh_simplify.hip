// Simplification of an indexed triangle mesh by vertex clustering on a uniform grid (Rossignac-Borrel), the cluster's vertex placed at the
// minimiser of the area^2-weighted plane quadrics of the faces around its members (Lindstrom's out-of-core simplification), else at the
// members' mean -- include/neuman_hip.h 'mesh simplify' writes the contract out (rules Q1-Q9); tests/helpers/mesh_simplify_ref.py restates it
// in numpy.  What isosurface.hip extracts has the size its grid dictates; neuman_hip/mesh_simplify.py (simplify_mesh) thins it before it is
// bound, posed and drawn.
//
//   count        cells: a thread per vertex, the cell of rule Q2 (-1: a coordinate that is not finite).  mark: every face range-checked BEFORE
//                anything is indexed (invalid faces counted, their lowest index kept); a candidate stores 1 into its three cells' flags.
//                The three rankings (used cells -> cluster ids, clusters' member counts -> the member lists' offsets, kept faces -> output
//                rows) share mesh_device.h's scan: span_rank_kernel over a span of kSpan counters, span_scan_kernel over the spans' sums in 64
//                bits, the consumer adds the span's offset.  members: count per cluster -> scan -> fill through an integer
//                atomicAdd on the cursor -> a sort of every cluster's segment in place by one lane (insertion up to kSortInThread entries,
//                heap sort beyond), which makes the lists a function of the mesh alone.  duplicates: an open-addressing table of face
//                indices, 2 slots per face; a slot's key is the rotated triple of the face it holds, claimed by compare-and-swap and lowered
//                by atomicMin, so every key's slot ends with the key's lowest face under every interleaving; a candidate is kept iff it
//                finds itself there.  Every launch after mark reads the invalid count and does nothing when it is not zero.
//   fill         a thread per cluster: the mean, then (quadric) A and b over the members' incident faces in list order, all in one lane's
//                loop in float64; a thread per face writes the kept faces.  rows: a thread per (cluster, column), rule Q5.
//
// Workspace: 16 bytes per vertex (cell, cursor, offset, member) + 12 bytes per face (rank, two table slots) + 4 bytes per cell (flag, then
// rank) + 16 bytes per kSpan vertices, faces and cells + 68.
#include "common.h"
#include "mesh_device.h"

#include <cmath>

namespace {

using namespace nm_mesh;                                      // the sizes, the header's protocol, the scan, the sort, the checks, the records: mesh_device.h

constexpr int kSlotsPerFace = 2;                              // the duplicate table: slots per input face (at most half of them are ever taken)

enum { kHdrClusters = 0, kHdrFacesOut = 3, kHdrMembers = 4 };      // int64 words of the header beside kHdrInvalid and kHdrFirstInvalid
enum { kPlaceMean = 0, kPlaceQuadric = 1 };

struct Grid {                                                 // rule Q2
    double lo[3], h;
    int n[3];
};

// ---- workspace --------------------------------------------------------------------------------------------------------------------------
struct Layout {
    int64_t cells, cspans, vspans, fspans, slots;
    int64_t off_csum, off_coff, off_vsum, off_voff, off_fsum, off_foff, off_vcell, off_cursor, off_moff, off_mem, off_crank, off_frank, off_table, bytes;
};

inline Layout layout_of(int64_t V, int64_t F, int64_t cells) {
    Layout L;
    L.cells = cells;
    L.cspans = spans_of(cells);
    L.vspans = spans_of(V);
    L.fspans = spans_of(F);
    L.slots = kSlotsPerFace * F;
    L.off_csum = kHeaderBytes;
    L.off_coff = L.off_csum + L.cspans * 8;
    L.off_vsum = L.off_coff + L.cspans * 8;
    L.off_voff = L.off_vsum + L.vspans * 8;
    L.off_fsum = L.off_voff + L.vspans * 8;
    L.off_foff = L.off_fsum + L.fspans * 8;
    L.off_vcell = up16(L.off_foff + L.fspans * 8);
    L.off_cursor = up16(L.off_vcell + V * 4);
    L.off_moff = up16(L.off_cursor + V * 4);
    L.off_mem = up16(L.off_moff + (V + 1) * 4);
    L.off_crank = up16(L.off_mem + V * 4);
    L.off_frank = up16(L.off_crank + cells * 4);
    L.off_table = up16(L.off_frank + F * 4);
    L.bytes = up16(L.off_table + L.slots * 4);
    return L;
}

struct Work {
    int64_t* hdr;                                             // kHdr*
    int64_t *csum, *coff, *vsum, *voff, *fsum, *foff;         // [spans] the spans' sums and their exclusive scan: cells, clusters, faces
    int32_t* vcell;                                           // [V] the vertex's linear cell index, -1 for a vertex that is not finite
    int32_t* cursor;                                          // [V] by cluster id: the member count; after the scan the fill's next free slot
    int32_t* moff;                                            // [V+1] by cluster id: where the cluster's members start in `mem` (entries past K: the total)
    int32_t* mem;                                             // [V] the members, cluster after cluster, ascending inside a cluster
    int32_t* crank;                                           // [cells] 1 for a used cell; after the scan its in-span rank, -1 for an unused cell
    int32_t* frank;                                           // [F] 1 for a kept face; after the scan its in-span rank, -1 for any other face
    int32_t* table;                                           // [slots] the lowest face of the slot's rotated triple, -1 for a free slot
    int64_t V, F, slots;
    Grid g;
};

inline Work work_of(const void* ws, const Layout& L, int64_t V, int64_t F, const Grid& g) {
    char* b = static_cast<char*>(const_cast<void*>(ws));
    Work w;
    w.hdr = reinterpret_cast<int64_t*>(b);
    w.csum = reinterpret_cast<int64_t*>(b + L.off_csum);
    w.coff = reinterpret_cast<int64_t*>(b + L.off_coff);
    w.vsum = reinterpret_cast<int64_t*>(b + L.off_vsum);
    w.voff = reinterpret_cast<int64_t*>(b + L.off_voff);
    w.fsum = reinterpret_cast<int64_t*>(b + L.off_fsum);
    w.foff = reinterpret_cast<int64_t*>(b + L.off_foff);
    w.vcell = reinterpret_cast<int32_t*>(b + L.off_vcell);
    w.cursor = reinterpret_cast<int32_t*>(b + L.off_cursor);
    w.moff = reinterpret_cast<int32_t*>(b + L.off_moff);
    w.mem = reinterpret_cast<int32_t*>(b + L.off_mem);
    w.crank = reinterpret_cast<int32_t*>(b + L.off_crank);
    w.frank = reinterpret_cast<int32_t*>(b + L.off_frank);
    w.table = reinterpret_cast<int32_t*>(b + L.off_table);
    w.V = V;
    w.F = F;
    w.slots = L.slots;
    w.g = g;
    return w;
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }             // (a NaN compares false)
__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

// ---- cells and candidates ---------------------------------------------------------------------------------------------------------------
// rule Q2: floor((x - lo) / h) in float64, clamped while still a double (a far vertex must not overflow the conversion)
__global__ void __launch_bounds__(kThreads) sx_cell_kernel(const float* __restrict__ verts, int64_t V, Grid g, int32_t* __restrict__ vcell) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    int64_t c[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = verts[3 * v + a];
        finite = finite && finite_f(x);
        double t = floor(((double)x - g.lo[a]) / g.h);
        const double top = (double)(g.n[a] - 1);
        t = t >= 0.0 ? t : 0.0;                                // (a NaN lands on 0; the vertex is dropped below)
        t = t <= top ? t : top;
        c[a] = (int64_t)t;
    }
    vcell[v] = finite ? (int32_t)((c[2] * g.n[1] + c[1]) * g.n[0] + c[0]) : -1;
}

// rule Q3 on a VALID face: its three cells, and whether it is a candidate (three finite vertices in three pairwise distinct cells -- a face
// that is not proper cannot be one)
__device__ __forceinline__ bool candidate_cells(const int32_t* __restrict__ vcell, int32_t a, int32_t b, int32_t c, int32_t cell[3]) {
    cell[0] = vcell[a];
    cell[1] = vcell[b];
    cell[2] = vcell[c];
    return cell[0] >= 0 && cell[1] >= 0 && cell[2] >= 0 && cell[0] != cell[1] && cell[0] != cell[2] && cell[1] != cell[2];
}

// rule Q1: the range check comes before any use of an index.  `used` was zeroed by the call; the stores race with equal values.
__global__ void __launch_bounds__(kThreads) sx_mark_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ vcell,
                                                           int64_t cells, int32_t* used, int64_t* hdr) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!(in_range(a, V) && in_range(b, V) && in_range(c, V))) {
        record_invalid_face(hdr, f);
        return;
    }
    int32_t cell[3];
    if (!candidate_cells(vcell, a, b, c, cell)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if ((int64_t)cell[k] < cells) used[cell[k]] = 1;
}

// ---- clusters and members ---------------------------------------------------------------------------------------------------------------
// rule Q3: the rank of the vertex's cell among the used cells, -1 for an unused cell or a vertex that is not finite
__device__ __forceinline__ int32_t cluster_of(const Work& w, int32_t v) {
    const int32_t c = w.vcell[v];
    if (c < 0) return -1;
    const int32_t r = w.crank[c];
    return r < 0 ? -1 : (int32_t)(w.coff[c / kSpan] + r);
}

// `count` (the cursors) was zeroed by the call; a cluster id is below K <= V
__global__ void __launch_bounds__(kThreads) sx_cluster_kernel(Work w, int32_t* __restrict__ vert_cluster) {
    if (w.hdr[kHdrInvalid] != 0) return;
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= w.V) return;
    const int32_t k = cluster_of(w, (int32_t)v);
    vert_cluster[v] = k;
    if (in_range(k, w.V)) atomicAdd(w.cursor + k, 1);
}

__global__ void __launch_bounds__(kThreads) sx_offset_kernel(Work w) {
    if (w.hdr[kHdrInvalid] != 0) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= w.V) return;
    const int32_t at = (int32_t)(w.voff[i / kSpan] + w.moff[i]);
    w.moff[i] = at;
    w.cursor[i] = at;
}

// a member takes the next free slot of its cluster; the slot's number depends on the interleaving, the SET of a list's entries does not
__global__ void __launch_bounds__(kThreads) sx_member_kernel(Work w) {
    if (w.hdr[kHdrInvalid] != 0) return;
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= w.V) return;
    const int32_t k = cluster_of(w, (int32_t)v);
    if (!in_range(k, w.V)) return;
    const int64_t at = atomicAdd(w.cursor + k, 1);
    if (at >= 0 && at < w.V) w.mem[at] = (int32_t)v;
}

// rule Q4: a cluster's members in ascending vertex index (entries past K have empty segments)
__global__ void __launch_bounds__(kThreads) sx_sort_kernel(Work w) {
    if (w.hdr[kHdrInvalid] != 0) return;
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= w.V) return;
    const int64_t lo = w.moff[k], hi = w.moff[k + 1];
    if (lo < 0 || hi > w.V || hi - lo < 2) return;
    sort_segment(w.mem + lo, (int)(hi - lo));
}

// ---- duplicates -------------------------------------------------------------------------------------------------------------------------
// rule Q7: the candidate's corners as cluster ids, rotated so that the smallest comes first (they are pairwise distinct); false for a face
// that is no candidate.  Every face is valid here.
__device__ __forceinline__ bool rotated_triple(const Work& w, const int32_t* __restrict__ faces, int64_t f, int32_t t[3]) {
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!(in_range(a, w.V) && in_range(b, w.V) && in_range(c, w.V))) return false;
    int32_t cell[3];
    if (!candidate_cells(w.vcell, a, b, c, cell)) return false;
    const int32_t p = cluster_of(w, a), q = cluster_of(w, b), r = cluster_of(w, c);
    if (p < 0 || q < 0 || r < 0) return false;                 // (a candidate's cells are used)
    if (p < q && p < r) { t[0] = p; t[1] = q; t[2] = r; }
    else if (q < r) { t[0] = q; t[1] = r; t[2] = p; }
    else { t[0] = r; t[1] = p; t[2] = q; }
    return true;
}

__device__ __forceinline__ int64_t first_slot(const int32_t t[3], int64_t slots) {
    unsigned long long h = (unsigned long long)(unsigned)t[0] * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h = (h + (unsigned)t[1]) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    h = (h + (unsigned)t[2]) * 0x94D049BB133111EBull;
    h ^= h >> 31;
    return (int64_t)(h % (unsigned long long)slots);
}

__device__ __forceinline__ bool same_triple(const int32_t s[3], const int32_t t[3]) { return s[0] == t[0] && s[1] == t[1] && s[2] == t[2]; }

// A free slot is claimed by compare-and-swap; a slot taken by a face of the same triple is lowered by atomicMin; a slot of another triple is
// passed.  Whatever face holds a slot, the slot's triple never changes, so each triple's slot ends with the triple's lowest face.  At most F of
// the 2 F slots are ever taken: the walk ends.
__global__ void __launch_bounds__(kThreads) sx_insert_kernel(Work w, const int32_t* __restrict__ faces) {
    if (w.hdr[kHdrInvalid] != 0) return;
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= w.F) return;
    int32_t t[3], s[3];
    if (!rotated_triple(w, faces, f, t)) return;
    int64_t slot = first_slot(t, w.slots);
    for (int64_t probe = 0; probe < w.slots; ++probe) {
        const int32_t seen = atomicCAS(w.table + slot, -1, (int32_t)f);
        if (seen == -1) return;
        if (!in_range(seen, w.F) || !rotated_triple(w, faces, seen, s)) return;      // (never: the table holds candidates only)
        if (same_triple(s, t)) {
            atomicMin(w.table + slot, (int32_t)f);
            return;
        }
        slot = slot + 1 == w.slots ? 0 : slot + 1;
    }
}

// a candidate is kept iff the slot of its triple holds the candidate itself: no candidate of a lower index has the same rotated triple
__global__ void __launch_bounds__(kThreads) sx_keep_kernel(Work w, const int32_t* __restrict__ faces) {
    if (w.hdr[kHdrInvalid] != 0) return;
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= w.F) return;
    int32_t t[3], s[3];
    int keep = 0;
    if (rotated_triple(w, faces, f, t)) {
        int64_t slot = first_slot(t, w.slots);
        for (int64_t probe = 0; probe < w.slots; ++probe) {
            const int32_t seen = w.table[slot];
            if (!in_range(seen, w.F) || !rotated_triple(w, faces, seen, s)) break;
            if (same_triple(s, t)) {
                keep = seen == (int32_t)f;
                break;
            }
            slot = slot + 1 == w.slots ? 0 : slot + 1;
        }
    }
    w.frank[f] = keep;
}

// ---- fill -------------------------------------------------------------------------------------------------------------------------------
// rules Q5 and Q6, a thread per cluster.  The counts the caller sized the outputs with must be the header's: a stale workspace writes nothing.
// An offset, a member, a face index or a vertex index out of range is never followed: the entry is skipped.
__global__ void __launch_bounds__(kThreads) sx_place_kernel(Work w, const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ inc_off, const int32_t* __restrict__ inc, int placement,
                                                            int64_t n_clusters, int64_t n_faces_out, float* __restrict__ verts_out) {
    if (w.hdr[kHdrClusters] != n_clusters || w.hdr[kHdrFacesOut] != n_faces_out) return;
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n_clusters || k >= w.V) return;
    int64_t lo = w.moff[k], hi = w.moff[k + 1];
    if (lo < 0 || hi > w.V || lo > hi) hi = lo;
    double m[3];
    const double count = (double)(hi - lo);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double s = 0.0;
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t v = w.mem[i];
            if (in_range(v, w.V)) s = s + (double)verts[3 * (int64_t)v + a];
        }
        m[a] = s / count;
    }
    double p[3] = {m[0], m[1], m[2]};
    if (placement == kPlaceQuadric && lo < hi) {
        double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t v = w.mem[i];
            if (!in_range(v, w.V)) continue;
            const int64_t jlo = inc_off[v], jhi = inc_off[v + 1];
            if (jlo < 0 || jhi > 3 * w.F || jlo > jhi) continue;
            for (int64_t j = jlo; j < jhi; ++j) {
                const int32_t f = inc[j];
                if (!in_range(f, w.F)) continue;
                const int32_t a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
                if (!in_range(a, w.V) || !in_range(b, w.V) || !in_range(c, w.V)) continue;
                const double ax = verts[3 * (int64_t)a], ay = verts[3 * (int64_t)a + 1], az = verts[3 * (int64_t)a + 2];
                const double ux = (double)verts[3 * (int64_t)b] - ax, uy = (double)verts[3 * (int64_t)b + 1] - ay, uz = (double)verts[3 * (int64_t)b + 2] - az;
                const double wx = (double)verts[3 * (int64_t)c] - ax, wy = (double)verts[3 * (int64_t)c + 1] - ay, wz = (double)verts[3 * (int64_t)c + 2] - az;
                const double n0 = uy * wz - uz * wy, n1 = uz * wx - ux * wz, n2 = ux * wy - uy * wx;
                const double e0 = ax - m[0], e1 = ay - m[1], e2 = az - m[2];
                const double t = (n0 * e0 + n1 * e1) + n2 * e2;
                A00 += n0 * n0;
                A01 += n0 * n1;
                A02 += n0 * n2;
                A11 += n1 * n1;
                A12 += n1 * n2;
                A22 += n2 * n2;
                b0 += n0 * t;
                b1 += n1 * t;
                b2 += n2 * t;
            }
        }
        const double reg = ((A00 + A11) + A22) * 0.0009765625;  // 2^-10
        A00 += reg;
        A11 += reg;
        A22 += reg;
        const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
        const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
        const double det = (A00 * c00 + A01 * c01) + A02 * c02;
        const double y0 = ((c00 * b0 + c01 * b1) + c02 * b2) / det;
        const double y1 = ((c01 * b0 + c11 * b1) + c12 * b2) / det;
        const double y2 = ((c02 * b0 + c12 * b1) + c22 * b2) / det;
        const double q[3] = {m[0] + y0, m[1] + y1, m[2] + y2};
        bool ok = det > 0.0 && finite_d(det) && finite_d(q[0]) && finite_d(q[1]) && finite_d(q[2]);
        const int32_t first = w.mem[lo];
        int64_t cell = in_range(first, w.V) ? w.vcell[first] : -1;
        ok = ok && cell >= 0;
        const int64_t c3[3] = {cell % w.g.n[0], (cell / w.g.n[0]) % w.g.n[1], cell / ((int64_t)w.g.n[0] * w.g.n[1])};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double box_lo = w.g.lo[a] + (double)c3[a] * w.g.h, box_hi = w.g.lo[a] + (double)(c3[a] + 1) * w.g.h;
            ok = ok && box_lo <= q[a] && q[a] <= box_hi;
        }
        if (ok) {
            p[0] = q[0];
            p[1] = q[1];
            p[2] = q[2];
        }
    }
    verts_out[3 * k] = (float)p[0];
    verts_out[3 * k + 1] = (float)p[1];
    verts_out[3 * k + 2] = (float)p[2];
}

// rule Q7: the kept faces in ascending input order, each as its rotated triple
__global__ void __launch_bounds__(kThreads) sx_faces_kernel(Work w, const int32_t* __restrict__ faces, int64_t n_clusters, int64_t n_faces_out,
                                                            int32_t* __restrict__ faces_out, int32_t* __restrict__ face_src) {
    if (w.hdr[kHdrClusters] != n_clusters || w.hdr[kHdrFacesOut] != n_faces_out) return;
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= w.F) return;
    const int32_t r = w.frank[f];
    if (r < 0) return;
    const int64_t at = w.foff[f / kSpan] + r;
    int32_t t[3];
    if (at < 0 || at >= n_faces_out || !rotated_triple(w, faces, f, t)) return;
    faces_out[3 * at] = t[0];
    faces_out[3 * at + 1] = t[1];
    faces_out[3 * at + 2] = t[2];
    if (face_src) face_src[at] = (int32_t)f;
}

// rule Q5, a thread per (cluster, column)
__global__ void __launch_bounds__(kThreads) sx_rows_kernel(Work w, const float* __restrict__ rows, int width, int64_t n_clusters, float* __restrict__ out) {
    if (w.hdr[kHdrClusters] != n_clusters) return;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_clusters * width) return;
    const int64_t k = e / width;
    const int col = (int)(e - k * width);
    if (k >= w.V) return;
    int64_t lo = w.moff[k], hi = w.moff[k + 1];
    if (lo < 0 || hi > w.V || lo > hi) hi = lo;
    double s = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t v = w.mem[i];
        if (in_range(v, w.V)) s = s + (double)rows[(int64_t)v * width + col];
    }
    out[e] = (float)(s / (double)(hi - lo));
}

// What nm_mesh_simplify_count left in a workspace, for the fill and the rows entry to compare their counts with, without a read-back (rule Q8)
struct Record {
    const void* workspace;
    int64_t V, F, cells, n_clusters, n_faces_out;
};
Remembered<Record> g_records;

// ---- argument checks --------------------------------------------------------------------------------------------------------------------
inline bool dims_ok(int nx, int ny, int nz) { return nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny < (1ll << 31) && (int64_t)nx * ny * nz < (1ll << 31); }
inline bool grid_ok(const float* lo, float h, int nx, int ny, int nz) {
    return lo && std::isfinite(lo[0]) && std::isfinite(lo[1]) && std::isfinite(lo[2]) && std::isfinite(h) && h > 0.f && dims_ok(nx, ny, nz);
}

inline Grid grid_of(const float* lo, float h, int nx, int ny, int nz) {
    Grid g;
    for (int a = 0; a < 3; ++a) g.lo[a] = (double)lo[a];
    g.h = (double)h;
    g.n[0] = nx;
    g.n[1] = ny;
    g.n[2] = nz;
    return g;
}

#define NM_SX_MESH(who)                                                                                                                      \
    NM_REQUIRE(mesh_ok(V, F), who ": V = %lld, F = %lld: V and 3 F must be in [0, 2^31)", (long long)V, (long long)F);                      \
    NM_REQUIRE(faces || F == 0, who ": null faces");                                                                                         \
    NM_REQUIRE(verts || V == 0, who ": null verts")
#define NM_SX_GRID(who)                                                                                                                      \
    NM_REQUIRE(grid_ok(lo, h, nx, ny, nz), who ": bad grid: lo must be three finite floats, h finite and > 0 (h = %g), dims >= 1 with fewer " \
               "than 2^31 cells (%d x %d x %d)", (double)h, nx, ny, nz)

}  // namespace

extern "C" {

int64_t nm_mesh_simplify_workspace_bytes(int64_t V, int64_t F, int nx, int ny, int nz) {
    if (!mesh_ok(V, F) || !dims_ok(nx, ny, nz)) {
        nm::set_error("nm_mesh_simplify_workspace_bytes: V = %lld, F = %lld, dims %d x %d x %d: V, 3 F and the cell count must be in [0, 2^31), every dim >= 1",
                      (long long)V, (long long)F, nx, ny, nz);
        return NM_ERR_ARG;
    }
    return layout_of(V, F, (int64_t)nx * ny * nz).bytes;
}

int nm_mesh_simplify_count(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo, float h, int nx, int ny, int nz,
                           int32_t* vert_cluster, void* workspace, int64_t workspace_bytes, int64_t* n_clusters, int64_t* n_faces_out,
                           nm_stream_t stream) {
    NM_SX_MESH("nm_mesh_simplify_count");
    NM_SX_GRID("nm_mesh_simplify_count");
    NM_REQUIRE(vert_cluster || V == 0, "nm_mesh_simplify_count: null vert_cluster");
    NM_REQUIRE(n_clusters && n_faces_out, "nm_mesh_simplify_count: null count pointer");
    const Layout L = layout_of(V, F, (int64_t)nx * ny * nz);
    NM_MESH_WORKSPACE("nm_mesh_simplify_count", L.bytes);
    {
        const Range outs[2] = {{vert_cluster, V * 4}, {workspace, L.bytes}}, ins[2] = {{verts, V * 12}, {faces, F * 12}};
        NM_REQUIRE(!any_overlap(outs, 2, ins, 2), "nm_mesh_simplify_count: verts, faces, vert_cluster and the workspace must not overlap");
    }
    g_records.forget(workspace);
    const Work w = work_of(workspace, L, V, F, grid_of(lo, h, nx, ny, nz));
    hipStream_t st = nm::as_stream(stream);
    int rc = NM_OK;
    if ((rc = nm::check_hip(hipMemsetAsync(w.crank, 0, (size_t)L.cells * 4, st), "nm_mesh_simplify_count: clear cell flags"))) return rc;
    if (V > 0 && (rc = nm::check_hip(hipMemsetAsync(w.cursor, 0, (size_t)V * 4, st), "nm_mesh_simplify_count: clear counters"))) return rc;
    if (F > 0 && (rc = nm::check_hip(hipMemsetAsync(w.table, 0xFF, (size_t)L.slots * 4, st), "nm_mesh_simplify_count: clear table"))) return rc;
    hipLaunchKernelGGL(reset_header_kernel, dim3(1), dim3(64), 0, st, w.hdr);
    if (V > 0) hipLaunchKernelGGL(sx_cell_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, verts, V, w.g, w.vcell);
    if (F > 0) hipLaunchKernelGGL(sx_mark_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, faces, F, V, w.vcell, L.cells, w.crank, w.hdr);
    const int64_t* const invalid = w.hdr + kHdrInvalid;       // every scan launch is skipped when this word is not zero
    hipLaunchKernelGGL(span_rank_kernel<Counters>, dim3((unsigned)L.cspans), dim3(kThreads), 0, st, Counters{w.crank}, L.cells, w.crank, 1, w.csum, invalid);
    hipLaunchKernelGGL(span_scan_kernel, dim3(1), dim3(kThreads), 0, st, w.csum, L.cspans, w.coff, w.hdr + kHdrClusters, nullptr, invalid);
    if (V > 0) {
        hipLaunchKernelGGL(sx_cluster_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, w, vert_cluster);
        hipLaunchKernelGGL(span_rank_kernel<Counters>, dim3((unsigned)L.vspans), dim3(kThreads), 0, st, Counters{w.cursor}, V, w.moff, 0, w.vsum, invalid);
        hipLaunchKernelGGL(span_scan_kernel, dim3(1), dim3(kThreads), 0, st, w.vsum, L.vspans, w.voff, w.hdr + kHdrMembers, w.moff + V, invalid);
        hipLaunchKernelGGL(sx_offset_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, w);
        hipLaunchKernelGGL(sx_member_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, w);
        hipLaunchKernelGGL(sx_sort_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, w);
    }
    if (F > 0 && V > 0) {
        hipLaunchKernelGGL(sx_insert_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, w, faces);
        hipLaunchKernelGGL(sx_keep_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, w, faces);
        hipLaunchKernelGGL(span_rank_kernel<Counters>, dim3((unsigned)L.fspans), dim3(kThreads), 0, st, Counters{w.frank}, F, w.frank, 1, w.fsum, invalid);
        hipLaunchKernelGGL(span_scan_kernel, dim3(1), dim3(kThreads), 0, st, w.fsum, L.fspans, w.foff, w.hdr + kHdrFacesOut, nullptr, invalid);
    }
    if ((rc = nm::check_launch("mesh simplify count kernels"))) return rc;
    int64_t head[4] = {0, 0, 0, 0};                            // the one read-back: {K, n_invalid, first_invalid, F'}
    if ((rc = read_header("nm_mesh_simplify_count", w.hdr, head, 4, V, st))) return rc;
    g_records.remember(Record{workspace, V, F, L.cells, head[kHdrClusters], head[kHdrFacesOut]});
    *n_clusters = head[kHdrClusters];
    *n_faces_out = head[kHdrFacesOut];
    return NM_OK;
}

int nm_mesh_simplify_fill(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo, float h, int nx, int ny, int nz,
                          int placement, const int32_t* inc_off, const int32_t* inc, const void* workspace, int64_t workspace_bytes,
                          float* verts_out, int32_t* faces_out, int32_t* face_src, int64_t n_clusters, int64_t n_faces_out, nm_stream_t stream) {
    NM_SX_MESH("nm_mesh_simplify_fill");
    NM_SX_GRID("nm_mesh_simplify_fill");
    NM_REQUIRE(placement == kPlaceMean || placement == kPlaceQuadric, "nm_mesh_simplify_fill: placement = %d is neither 0 (mean) nor 1 (quadric)", placement);
    NM_REQUIRE(placement != kPlaceQuadric || (inc_off && (inc || F == 0)), "nm_mesh_simplify_fill: quadric placement needs inc_off and inc of nm_mesh_adjacency");
    const Layout L = layout_of(V, F, (int64_t)nx * ny * nz);
    NM_MESH_WORKSPACE("nm_mesh_simplify_fill", L.bytes);
    NM_REQUIRE(count_ok(n_clusters) && count_ok(n_faces_out), "nm_mesh_simplify_fill: bad counts %lld, %lld", (long long)n_clusters, (long long)n_faces_out);
    NM_REQUIRE((verts_out || n_clusters == 0) && (faces_out || n_faces_out == 0), "nm_mesh_simplify_fill: null output");      // (an empty tensor's pointer is null)
    {
        const Range outs[3] = {{verts_out, n_clusters * 12}, {faces_out, n_faces_out * 12}, {face_src, n_faces_out * 4}};
        const Range ins[5] = {{verts, V * 12}, {faces, F * 12}, {workspace, L.bytes}, {inc_off, placement == kPlaceQuadric ? (V + 1) * 4 : 0},
                              {inc, placement == kPlaceQuadric ? 3 * F * 4 : 0}};
        NM_REQUIRE(!any_overlap(outs, 3, ins, 5), "nm_mesh_simplify_fill: the outputs must not overlap each other, the mesh, the lists or the workspace");
    }
    Record r;
    NM_REQUIRE(g_records.recall(workspace, &r) && r.V == V && r.F == F && r.cells == L.cells,
               "nm_mesh_simplify_fill: the workspace holds no count of this mesh and grid (run nm_mesh_simplify_count on it first)");
    NM_REQUIRE(r.n_clusters == n_clusters && r.n_faces_out == n_faces_out,
               "nm_mesh_simplify_fill: counts %lld clusters, %lld faces; nm_mesh_simplify_count left %lld, %lld in the workspace", (long long)n_clusters,
               (long long)n_faces_out, (long long)r.n_clusters, (long long)r.n_faces_out);
    if (n_clusters == 0) return NM_OK;
    const Work w = work_of(workspace, L, V, F, grid_of(lo, h, nx, ny, nz));
    hipStream_t st = nm::as_stream(stream);
    hipLaunchKernelGGL(sx_place_kernel, dim3(blocks_for(n_clusters)), dim3(kThreads), 0, st, w, verts, faces, inc_off, inc, placement, n_clusters, n_faces_out,
                       verts_out);
    if (n_faces_out > 0)
        hipLaunchKernelGGL(sx_faces_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, w, faces, n_clusters, n_faces_out, faces_out, face_src);
    return nm::check_launch("mesh simplify fill kernels");
}

int nm_mesh_simplify_rows(const float* rows, int width, int64_t V, int64_t F, int nx, int ny, int nz, const void* workspace, int64_t workspace_bytes,
                          float* out, int64_t n_clusters, nm_stream_t stream) {
    NM_REQUIRE(mesh_ok(V, F), "nm_mesh_simplify_rows: V = %lld, F = %lld: V and 3 F must be in [0, 2^31)", (long long)V, (long long)F);
    NM_REQUIRE(dims_ok(nx, ny, nz), "nm_mesh_simplify_rows: bad grid: dims >= 1 with fewer than 2^31 cells (%d x %d x %d)", nx, ny, nz);
    NM_REQUIRE(width >= 1 && width <= 64, "nm_mesh_simplify_rows: width = %d must be in 1..64", width);
    NM_REQUIRE(rows || V == 0, "nm_mesh_simplify_rows: null rows");
    const Layout L = layout_of(V, F, (int64_t)nx * ny * nz);
    NM_MESH_WORKSPACE("nm_mesh_simplify_rows", L.bytes);
    NM_REQUIRE(count_ok(n_clusters) && n_clusters * width < (1ll << 31), "nm_mesh_simplify_rows: bad count %lld (n_clusters x width must be below 2^31)",
               (long long)n_clusters);
    NM_REQUIRE(out || n_clusters == 0, "nm_mesh_simplify_rows: null output");
    {
        const Range outs[1] = {{out, n_clusters * width * 4}}, ins[2] = {{rows, V * width * 4}, {workspace, L.bytes}};
        NM_REQUIRE(!any_overlap(outs, 1, ins, 2), "nm_mesh_simplify_rows: out must not overlap rows or the workspace");
    }
    Record r;
    NM_REQUIRE(g_records.recall(workspace, &r) && r.V == V && r.F == F && r.cells == L.cells,
               "nm_mesh_simplify_rows: the workspace holds no count of this mesh and grid (run nm_mesh_simplify_count on it first)");
    NM_REQUIRE(r.n_clusters == n_clusters, "nm_mesh_simplify_rows: %lld clusters; nm_mesh_simplify_count left %lld in the workspace", (long long)n_clusters,
               (long long)r.n_clusters);
    if (n_clusters == 0) return NM_OK;
    Grid g = {};
    g.n[0] = nx;
    g.n[1] = ny;
    g.n[2] = nz;
    const Work w = work_of(workspace, L, V, F, g);
    hipLaunchKernelGGL(sx_rows_kernel, dim3(blocks_for(n_clusters * width)), dim3(kThreads), 0, nm::as_stream(stream), w, rows, width, n_clusters, out);
    return nm::check_launch("mesh simplify rows kernel");
}

}  // extern "C"
