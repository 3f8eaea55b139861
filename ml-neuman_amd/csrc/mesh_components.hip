// Clean-up of an indexed triangle mesh: its connected components, their sizes and boxes, and the mesh compacted to a chosen subset of them --
// include/neuman_hip.h 'mesh components' writes the contract out (rules C1-C7); tests/helpers/mesh_components_ref.py restates it in numpy.
// What isosurface.hip extracts from a learned density is the body plus small closed blobs wherever sigma crosses the level in empty space;
// neuman_hip/mesh_extract.py (components, select_components, clean_mesh) drops them with these entry points.
//
//   label        init + validate: parent[v] = v, every face range-checked BEFORE anything is indexed (invalid faces counted, their lowest index
//                kept), referenced vertices marked.  hook: a thread per face unites (a, b) and (a, c) in a lock-free union-find -- roots found
//                with path halving, the larger root linked under the smaller by compare-and-swap, retried from the new roots when another
//                thread's link won.  A parent only ever decreases, so the root of a class ends as its smallest vertex under every interleaving
//                (C3, C7).  flatten: every vertex points at its root.  Every launch after the first reads the invalid count and does nothing
//                when it is not zero.
//   rank         the three rankings (roots -> component ids, kept vertices -> new indices, kept faces -> output rows) are mesh_device.h's:
//                span_rank_kernel over a flag per item, span_scan_kernel over the spans' sums, a last launch here adds the span's offset.
//   statistics   integer atomicAdd per vertex and per face; the boxes by atomicMin / atomicMax on the order-preserving integer image of a
//                float, decoded in place by a last launch.  No float is ever added atomically.  The lanes of a wave that share a label are
//                combined before the atomic (one body holds nearly every vertex: 10.5 ms without, profiles/mesh_components.md).
//
// Workspace: 9 bytes per vertex (parent, rank, referenced flag) + 4 bytes per face (rank) + 16 bytes per kSpan vertices and per kSpan faces + 64.
#include "common.h"
#include "mesh_device.h"

namespace {

using namespace nm_mesh;                                      // the sizes, the header's protocol, the ranking, the checks: mesh_device.h

constexpr int kCombine = 8;                                   // statistics: lanes of one label in a wave, from which their boxes are reduced by shuffles

#define NM_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

enum { kHdrComponents = 0, kHdrVertsOut = 3, kHdrFacesOut = 4 };      // int64 words of the header beside kHdrInvalid and kHdrFirstInvalid

// ---- workspace --------------------------------------------------------------------------------------------------------------------------
struct Layout {
    int64_t vspans, fspans;
    int64_t off_vsum, off_voff, off_fsum, off_foff, off_parent, off_rank, off_frank, off_ref, bytes;
};

inline Layout layout_of(int64_t V, int64_t F) {
    Layout L;
    L.vspans = spans_of(V);
    L.fspans = spans_of(F);
    L.off_vsum = kHeaderBytes;
    L.off_voff = L.off_vsum + L.vspans * 8;
    L.off_fsum = L.off_voff + L.vspans * 8;
    L.off_foff = L.off_fsum + L.fspans * 8;
    L.off_parent = up16(L.off_foff + L.fspans * 8);
    L.off_rank = up16(L.off_parent + V * 4);
    L.off_frank = up16(L.off_rank + V * 4);
    L.off_ref = up16(L.off_frank + F * 4);
    L.bytes = up16(L.off_ref + V);
    return L;
}

struct Work {
    int64_t* hdr;                                             // kHdr*
    int64_t *vsum, *voff, *fsum, *foff;                       // [spans] the spans' sums and their exclusive scan
    int32_t* parent;                                          // [V] union-find; after flatten the root
    int32_t* rank;                                            // [V] in-span rank of a root (label) | new index of a kept vertex, -1 (select)
    int32_t* frank;                                           // [F] output row of a kept face, -1
    uint8_t* ref;                                             // [V] some face names the vertex
};

inline Work work_of(void* ws, const Layout& L) {
    char* b = static_cast<char*>(ws);
    Work w;
    w.hdr = reinterpret_cast<int64_t*>(b);
    w.vsum = reinterpret_cast<int64_t*>(b + L.off_vsum);
    w.voff = reinterpret_cast<int64_t*>(b + L.off_voff);
    w.fsum = reinterpret_cast<int64_t*>(b + L.off_fsum);
    w.foff = reinterpret_cast<int64_t*>(b + L.off_foff);
    w.parent = reinterpret_cast<int32_t*>(b + L.off_parent);
    w.rank = reinterpret_cast<int32_t*>(b + L.off_rank);
    w.frank = reinterpret_cast<int32_t*>(b + L.off_frank);
    w.ref = reinterpret_cast<uint8_t*>(b + L.off_ref);
    return w;
}

// ---- label ------------------------------------------------------------------------------------------------------------------------------
// rule C1: the range check comes before any use of an index.  `ref` was zeroed by the call.
__global__ void __launch_bounds__(kThreads) mc_init_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, int32_t* __restrict__ parent,
                                                           uint8_t* __restrict__ ref, int64_t* __restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < V) parent[i] = (int32_t)i;
    if (i >= F) return;
    const int32_t a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
    if (in_range(a, V) && in_range(b, V) && in_range(c, V)) {
        ref[a] = 1; ref[b] = 1; ref[c] = 1;                   // (racing stores of the same byte value)
    } else {
        record_invalid_face(hdr, i);
    }
}

// every read of `parent` that can race with a link is a relaxed atomic load at agent scope: no value stays in a register across a retry
__device__ __forceinline__ int32_t load_parent(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, NM_RLX_AGENT);
}

// the root of x, halving the path on the way: parent[x] < x for every vertex that is not a root, so the walk ends; a halving store is an
// atomicMin, so a parent never increases
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
    int32_t p = load_parent(parent, x);
    while (p != x) {
        const int32_t g = load_parent(parent, p);
        if (g != p) __hip_atomic_fetch_min(parent + x, g, NM_RLX_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// A compare-and-swap links a ROOT (parent[hi] == hi) under a smaller root; when it fails another thread's link of `hi` succeeded, and the
// retry starts from the parent that link left: the loop needs no bound and waits for nobody.
__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
    while (true) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        a = lo;
        b = seen;
    }
}

__global__ void __launch_bounds__(kThreads) mc_hook_kernel(const int32_t* __restrict__ faces, int64_t F, int32_t* parent, const int64_t* __restrict__ hdr) {
    if (hdr[kHdrInvalid] != 0) return;
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a != b) unite(parent, a, b);
    if (a != c) unite(parent, a, c);
}

__global__ void __launch_bounds__(kThreads) mc_flatten_kernel(int64_t V, int32_t* parent, const int64_t* __restrict__ hdr) {
    if (hdr[kHdrInvalid] != 0) return;
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    int32_t x = (int32_t)v, p = load_parent(parent, x);
    while (p != x) { x = p; p = load_parent(parent, x); }      // a root stays one in this launch: nothing links any more
    __hip_atomic_store(parent + v, x, NM_RLX_AGENT);
}

// ---- rank -------------------------------------------------------------------------------------------------------------------------------
// the sources of mesh_device.h's span_rank_kernel: count(i) is 1 for a flagged item, and with mark_empty the rank of any other reads -1
struct IsRoot {                                               // rule C3: a representative is a referenced vertex that is its own root
    const int32_t* parent;
    const uint8_t* ref;
    __device__ int count(int64_t v) const { return ref[v] != 0 && parent[v] == (int32_t)v; }
};

// rule C3: the id of a component is the rank of its root among the roots; a face has the label of its first vertex
__global__ void __launch_bounds__(kThreads) mc_label_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ parent,
                                                            const uint8_t* __restrict__ ref, const int32_t* __restrict__ rank,
                                                            const int64_t* __restrict__ voff, const int64_t* __restrict__ hdr,
                                                            int32_t* __restrict__ vert_label, int32_t* __restrict__ face_label) {
    if (hdr[kHdrInvalid] != 0) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < V) {
        const int32_t r = parent[i];
        vert_label[i] = ref[i] ? (int32_t)(voff[r / kSpan] + rank[r]) : -1;
    }
    if (face_label && i < F) {
        const int32_t r = parent[faces[3 * i]];                // (every face is valid here)
        face_label[i] = (int32_t)(voff[r / kSpan] + rank[r]);
    }
}

// ---- statistics -------------------------------------------------------------------------------------------------------------------------
// the order-preserving integer image of a float: a < b as floats iff image(a) < image(b) as unsigned (-0 below +0)
__device__ __forceinline__ unsigned float_image(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float image_float(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__global__ void __launch_bounds__(kThreads) mc_stats_init_kernel(int64_t C, int32_t* __restrict__ comp_verts, int32_t* __restrict__ comp_faces,
                                                                 unsigned* __restrict__ box) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    comp_verts[c] = 0;
    comp_faces[c] = 0;
    if (box) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            box[6 * c + a] = float_image(INFINITY);
            box[6 * c + 3 + a] = float_image(-INFINITY);
        }
    }
}

__global__ void __launch_bounds__(kThreads) mc_stats_verts_kernel(int64_t V, const int32_t* __restrict__ vert_label, const float* __restrict__ verts, int64_t C,
                                                                  int32_t* comp_verts, unsigned* box) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t l = v < V ? vert_label[v] : -1;
    const bool valid = l >= 0 && (int64_t)l < C;
    unsigned lo[3], hi[3];                                     // the images of the usable coordinates, else the neutral elements of min and max
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = (valid && box) ? verts[3 * v + a] : NAN;
        const bool usable = x == x;                            // rule C4: a NaN is skipped
        lo[a] = usable ? float_image(x) : 0xffffffffu;
        hi[a] = usable ? float_image(x) : 0u;
    }
    // Neighbouring vertices mostly share a label (one body, a few floaters): the lanes of a wave that do are combined first, and one lane
    // issues the atomics -- sums, minima and maxima of integers, so the result is the same.  The loop is uniform over the wave.
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t ll = __shfl(l, leader, 64);
        const bool mine = valid && l == ll;
        const unsigned long long group = __ballot(mine);
        todo &= ~group;
        if (lane == leader) atomicAdd(comp_verts + ll, __popcll(group));
        if (!box) continue;
        if (__popcll(group) >= kCombine) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                unsigned mn = mine ? lo[a] : 0xffffffffu, mx = mine ? hi[a] : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned tn = __shfl_xor(mn, o, 64), tx = __shfl_xor(mx, o, 64);
                    mn = tn < mn ? tn : mn;
                    mx = tx > mx ? tx : mx;
                }
                if (lane == leader) {
                    atomicMin(box + 6 * (int64_t)ll + a, mn);
                    atomicMax(box + 6 * (int64_t)ll + 3 + a, mx);
                }
            }
        } else if (mine) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(box + 6 * (int64_t)ll + a, lo[a]);
                atomicMax(box + 6 * (int64_t)ll + 3 + a, hi[a]);
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads) mc_stats_faces_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ vert_label,
                                                                  int64_t C, int32_t* comp_faces) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t a = f < F ? faces[3 * f] : -1;
    const int32_t l = in_range(a, V) ? vert_label[a] : -1;
    const bool valid = l >= 0 && (int64_t)l < C;
    unsigned long long todo = __ballot(valid);                 // as in the vertex pass: one add per label and wave
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t ll = __shfl(l, leader, 64);
        const unsigned long long group = __ballot(valid && l == ll);
        todo &= ~group;
        if (lane == leader) atomicAdd(comp_faces + ll, __popcll(group));
    }
}

__global__ void __launch_bounds__(kThreads) mc_stats_decode_kernel(int64_t n, unsigned* __restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) reinterpret_cast<float*>(box)[i] = image_float(box[i]);
}

// ---- selection --------------------------------------------------------------------------------------------------------------------------
struct Kept {                                                 // rule C5; a label outside [0, C) keeps nothing
    const int32_t* vert_label;
    const uint8_t* keep;
    int64_t C;
    __device__ bool vertex(int64_t v) const {
        const int32_t l = vert_label[v];
        return l >= 0 && (int64_t)l < C && keep[l] != 0;
    }
};

struct KeptVertex {
    Kept k;
    __device__ int count(int64_t v) const { return k.vertex(v); }
};

struct KeptFace {                                             // a face has the label of its first vertex; an index out of range is never followed
    Kept k;
    const int32_t* faces;
    int64_t V;
    __device__ int count(int64_t f) const {
        const int32_t a = faces[3 * f];
        return in_range(a, V) && k.vertex(a);
    }
};

// the fill launch of the two rankings: in-span rank + the span's offset, in place
__global__ void __launch_bounds__(kThreads) mc_select_offset_kernel(int64_t V, int64_t F, int32_t* __restrict__ rank, int32_t* __restrict__ frank,
                                                                    const int64_t* __restrict__ voff, const int64_t* __restrict__ foff) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < V && rank[i] >= 0) rank[i] = (int32_t)(voff[i / kSpan] + rank[i]);
    if (i < F && frank[i] >= 0) frank[i] = (int32_t)(foff[i / kSpan] + frank[i]);
}

// the counts the caller sized the outputs with must be the header's: a stale workspace writes nothing
__global__ void __launch_bounds__(kThreads) mc_select_fill_kernel(const int32_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ rank,
                                                                  const int32_t* __restrict__ frank, const int64_t* __restrict__ hdr, int64_t n_verts_out,
                                                                  int64_t n_faces_out, int32_t* __restrict__ vert_src, int32_t* __restrict__ faces_out) {
    if (hdr[kHdrVertsOut] != n_verts_out || hdr[kHdrFacesOut] != n_faces_out) return;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < V) {
        const int32_t at = rank[i];
        if (at >= 0 && (int64_t)at < n_verts_out) vert_src[at] = (int32_t)i;
    }
    if (i < F) {
        const int32_t at = frank[i];
        if (at >= 0 && (int64_t)at < n_faces_out) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int32_t old = faces[3 * i + k];
                faces_out[3 * (int64_t)at + k] = in_range(old, V) ? rank[old] : -1;      // (-1: only with labels no nm_mesh_components wrote)
            }
        }
    }
}

// What nm_mesh_select_count left in a workspace, for nm_mesh_select_fill to compare its counts with, without a read-back (rule C6)
struct Selection {
    const void* workspace;
    int64_t V, F, n_verts_out, n_faces_out;
};
Remembered<Selection> g_selections;

// ---- argument checks --------------------------------------------------------------------------------------------------------------------
#define NM_MC_SIZES(who)                                                                                                                     \
    NM_REQUIRE(count_ok(V) && count_ok(F), who ": V = %lld, F = %lld: both must be in [0, 2^31)", (long long)V, (long long)F);              \
    NM_REQUIRE(faces || F == 0, who ": null faces")
#define NM_MC_LABELS(who)                                                                                                                    \
    NM_REQUIRE(vert_label || V == 0, who ": null vert_label");                                                                               \
    NM_REQUIRE(count_ok(C), who ": C = %lld must be in [0, 2^31)", (long long)C)

}  // namespace

extern "C" {

int64_t nm_mesh_components_workspace_bytes(int64_t V, int64_t F) {
    if (!count_ok(V) || !count_ok(F)) {
        nm::set_error("nm_mesh_components_workspace_bytes: V = %lld, F = %lld: both must be in [0, 2^31)", (long long)V, (long long)F);
        return NM_ERR_ARG;
    }
    return layout_of(V, F).bytes;
}

int nm_mesh_components(const int32_t* faces, int64_t F, int64_t V, int32_t* vert_label, int32_t* face_label, void* workspace,
                       int64_t workspace_bytes, int64_t* n_components, nm_stream_t stream) {
    NM_MC_SIZES("nm_mesh_components");
    NM_REQUIRE(vert_label || V == 0, "nm_mesh_components: null vert_label");
    NM_REQUIRE(n_components, "nm_mesh_components: null count pointer");
    NM_MESH_WORKSPACE("nm_mesh_components", layout_of(V, F).bytes);
    g_selections.forget(workspace);                               // the arrays of a selection are overwritten
    if (V == 0 && F == 0) {
        *n_components = 0;
        return NM_OK;
    }
    const Layout L = layout_of(V, F);
    const Work w = work_of(workspace, L);
    hipStream_t st = nm::as_stream(stream);
    int rc = NM_OK;
    if (V > 0 && (rc = nm::check_hip(hipMemsetAsync(w.ref, 0, (size_t)V, st), "nm_mesh_components: clear flags"))) return rc;
    hipLaunchKernelGGL(reset_header_kernel, dim3(1), dim3(64), 0, st, w.hdr);
    hipLaunchKernelGGL(mc_init_kernel, dim3(blocks_for(V > F ? V : F)), dim3(kThreads), 0, st, faces, F, V, w.parent, w.ref, w.hdr);
    if (V > 0 && F > 0) {
        hipLaunchKernelGGL(mc_hook_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, faces, F, w.parent, w.hdr);
        hipLaunchKernelGGL(mc_flatten_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, V, w.parent, w.hdr);
    }
    if (V > 0) {
        hipLaunchKernelGGL(span_rank_kernel<IsRoot>, dim3((unsigned)L.vspans), dim3(kThreads), 0, st, IsRoot{w.parent, w.ref}, V, w.rank, 1, w.vsum,
                           w.hdr + kHdrInvalid);
        hipLaunchKernelGGL(span_scan_kernel, dim3(1), dim3(kThreads), 0, st, w.vsum, L.vspans, w.voff, w.hdr + kHdrComponents, nullptr,
                           w.hdr + kHdrInvalid);
        hipLaunchKernelGGL(mc_label_kernel, dim3(blocks_for(V > F ? V : F)), dim3(kThreads), 0, st, faces, F, V, w.parent, w.ref, w.rank, w.voff, w.hdr,
                           vert_label, face_label);
    }
    if ((rc = nm::check_launch("mesh component kernels"))) return rc;
    int64_t head[3] = {0, 0, 0};                               // the one read-back: {n_components, n_invalid, first_invalid}
    if ((rc = read_header("nm_mesh_components", w.hdr, head, 3, V, st))) return rc;
    *n_components = head[kHdrComponents];
    return NM_OK;
}

int nm_mesh_component_stats(const int32_t* faces, int64_t F, int64_t V, const int32_t* vert_label, const float* verts, int64_t C, int32_t* comp_verts,
                            int32_t* comp_faces, float* comp_box, nm_stream_t stream) {
    NM_MC_SIZES("nm_mesh_component_stats");
    NM_MC_LABELS("nm_mesh_component_stats");
    NM_REQUIRE((comp_verts && comp_faces) || C == 0, "nm_mesh_component_stats: null output");
    NM_REQUIRE(verts || !comp_box, "nm_mesh_component_stats: comp_box needs verts");
    if (C == 0) return NM_OK;
    hipStream_t st = nm::as_stream(stream);
    unsigned* box = reinterpret_cast<unsigned*>(comp_box);    // the integer images until the last launch
    hipLaunchKernelGGL(mc_stats_init_kernel, dim3(blocks_for(C)), dim3(kThreads), 0, st, C, comp_verts, comp_faces, box);
    if (V > 0) hipLaunchKernelGGL(mc_stats_verts_kernel, dim3(blocks_for(V)), dim3(kThreads), 0, st, V, vert_label, verts, C, comp_verts, box);
    if (F > 0 && V > 0) hipLaunchKernelGGL(mc_stats_faces_kernel, dim3(blocks_for(F)), dim3(kThreads), 0, st, faces, F, V, vert_label, C, comp_faces);
    if (box) hipLaunchKernelGGL(mc_stats_decode_kernel, dim3(blocks_for(6 * C)), dim3(kThreads), 0, st, 6 * C, box);
    return nm::check_launch("mesh component statistics kernels");
}

int nm_mesh_select_count(const int32_t* faces, int64_t F, int64_t V, const int32_t* vert_label, const uint8_t* keep, int64_t C, void* workspace,
                         int64_t workspace_bytes, int64_t* n_verts_out, int64_t* n_faces_out, nm_stream_t stream) {
    NM_MC_SIZES("nm_mesh_select_count");
    NM_MC_LABELS("nm_mesh_select_count");
    NM_REQUIRE(keep || C == 0, "nm_mesh_select_count: null keep");
    NM_REQUIRE(n_verts_out && n_faces_out, "nm_mesh_select_count: null count pointer");
    NM_MESH_WORKSPACE("nm_mesh_select_count", layout_of(V, F).bytes);
    g_selections.forget(workspace);
    const Layout L = layout_of(V, F);
    const Work w = work_of(workspace, L);
    hipStream_t st = nm::as_stream(stream);
    int rc = NM_OK;
    int64_t counts[2] = {0, 0};
    if (V > 0) {
        const Kept k = {vert_label, keep, C};
        hipLaunchKernelGGL(reset_header_kernel, dim3(1), dim3(64), 0, st, w.hdr);
        hipLaunchKernelGGL(span_rank_kernel<KeptVertex>, dim3((unsigned)L.vspans), dim3(kThreads), 0, st, KeptVertex{k}, V, w.rank, 1, w.vsum, nullptr);
        hipLaunchKernelGGL(span_scan_kernel, dim3(1), dim3(kThreads), 0, st, w.vsum, L.vspans, w.voff, w.hdr + kHdrVertsOut, nullptr, nullptr);
        if (F > 0) {
            hipLaunchKernelGGL(span_rank_kernel<KeptFace>, dim3((unsigned)L.fspans), dim3(kThreads), 0, st, KeptFace{k, faces, V}, F, w.frank, 1, w.fsum, nullptr);
            hipLaunchKernelGGL(span_scan_kernel, dim3(1), dim3(kThreads), 0, st, w.fsum, L.fspans, w.foff, w.hdr + kHdrFacesOut, nullptr, nullptr);
        }
        hipLaunchKernelGGL(mc_select_offset_kernel, dim3(blocks_for(V > F ? V : F)), dim3(kThreads), 0, st, V, F, w.rank, w.frank, w.voff, w.foff);
        if ((rc = nm::check_launch("mesh selection count kernels"))) return rc;
        if ((rc = nm::check_hip(hipMemcpyAsync(counts, w.hdr + kHdrVertsOut, 16, hipMemcpyDeviceToHost, st), "nm_mesh_select_count: read counts"))) return rc;
        if ((rc = nm::check_hip(hipStreamSynchronize(st), "nm_mesh_select_count: sync"))) return rc;     // the one read-back
    }
    g_selections.remember(Selection{workspace, V, F, counts[0], counts[1]});
    *n_verts_out = counts[0];
    *n_faces_out = counts[1];
    return NM_OK;
}

int nm_mesh_select_fill(const int32_t* faces, int64_t F, int64_t V, const int32_t* vert_label, const uint8_t* keep, int64_t C, const void* workspace,
                        int64_t workspace_bytes, int32_t* vert_src, int32_t* faces_out, int64_t n_verts_out, int64_t n_faces_out, nm_stream_t stream) {
    NM_MC_SIZES("nm_mesh_select_fill");
    NM_MC_LABELS("nm_mesh_select_fill");
    NM_REQUIRE(keep || C == 0, "nm_mesh_select_fill: null keep");
    NM_MESH_WORKSPACE("nm_mesh_select_fill", layout_of(V, F).bytes);
    NM_REQUIRE(count_ok(n_verts_out) && count_ok(n_faces_out), "nm_mesh_select_fill: bad counts %lld, %lld", (long long)n_verts_out, (long long)n_faces_out);
    NM_REQUIRE((vert_src || n_verts_out == 0) && (faces_out || n_faces_out == 0), "nm_mesh_select_fill: null output");      // (an empty tensor's pointer is null)
    Selection s;
    NM_REQUIRE(g_selections.recall(workspace, &s) && s.V == V && s.F == F,
               "nm_mesh_select_fill: the workspace holds no selection of this mesh (run nm_mesh_select_count on it first)");
    NM_REQUIRE(s.n_verts_out == n_verts_out && s.n_faces_out == n_faces_out,
               "nm_mesh_select_fill: counts %lld vertices, %lld faces; nm_mesh_select_count left %lld, %lld in the workspace", (long long)n_verts_out,
               (long long)n_faces_out, (long long)s.n_verts_out, (long long)s.n_faces_out);
    if (n_verts_out == 0) return NM_OK;
    const Layout L = layout_of(V, F);
    const Work w = work_of(const_cast<void*>(workspace), L);
    hipLaunchKernelGGL(mc_select_fill_kernel, dim3(blocks_for(V > F ? V : F)), dim3(kThreads), 0, nm::as_stream(stream), faces, F, V, w.rank, w.frank, w.hdr,
                       n_verts_out, n_faces_out, vert_src, faces_out);
    return nm::check_launch("mesh selection fill kernel");
}

}  // extern "C"
