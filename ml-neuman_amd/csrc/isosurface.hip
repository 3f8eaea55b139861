// Isosurface of a scalar field on a regular grid as an indexed triangle mesh: marching tetrahedra on the Kuhn (Freudenthal) split of every
// cell -- include/neuman_hip.h 'isosurface' writes the contract out (rules M1-M7); tests/helpers/isosurface_ref.py restates it in numpy.
// The reference has no such step: this is what turns a trained density (neuman_hip/mesh_extract.py) into geometry.
//
//   classify     one 256-thread workgroup per brick of kBrick^3 grid vertices: the inside bits of the brick and of a one-vertex halo toward the
//                higher indices go to LDS once (the field is read here and, densely, nowhere else); every vertex then gets one byte of
//                crossed-edge flags (its seven edges toward higher indices) and one byte with the face count of the cell it anchors
//   scan         words of eight vertices: a workgroup counts kScanSpan vertices' flags (64-bit popcount) and faces, scans them (shuffles
//                inside a wave, LDS across the four waves) and keeps the in-span prefix of every word as two uint16; the spans' totals are
//                scanned in 64 bits by one workgroup, raster_device.h's scheme -- nothing is atomic, every run gives the same bits
//   read-back    the two 64-bit totals, 16 bytes: nm_isosurface_count's one synchronisation
//   fill         vertices: one thread per grid vertex with a crossed edge; faces: one thread per cell with a face.  An edge's mesh vertex
//                index is a rank query: span offset + word prefix + popcount of the flag bits below it
//
// Workspace: 2 bytes per grid vertex (flags, face counts) + 4 bytes per eight (prefixes) + 32 bytes per kScanSpan (span sums and offsets).
#include "common.h"

#include <math.h>

#include <cmath>

namespace {

constexpr int kBrick = 16;                                    // grid vertices per brick edge (each anchors a cell and owns seven edges)
constexpr int kHalo = kBrick + 1;                             // staged per axis: the brick and the next vertex
constexpr int kThreads = 256;
constexpr int kWord = 8;                                      // grid vertices per 64-bit word of flag bytes
constexpr int kScanSpan = 2048;                               // grid vertices one workgroup of the scan covers (kThreads words)
constexpr int64_t kHeaderBytes = 64;                          // {n_verts, n_faces} int64, padded
static_assert(kScanSpan == kThreads * kWord, "a thread of the scan takes one word");
static_assert(kScanSpan * 12 < 65536, "the in-span prefixes are uint16: 7 edges and 12 faces per vertex at most");

// ---- the tables, built from rule M3 / M5 ------------------------------------------------------------------------------------------------
// corner c of tetrahedron t as an offset mask (bit 0 x, bit 1 y, bit 2 z): 0, e_a, e_a + e_b, (1,1,1), permutations (a, b, c) in lexicographic order
struct TetTable {
    unsigned char corner[6][4];
    unsigned char odd[6];                                     // the permutation's parity = the sign of det(P1 - P0, P2 - P0, P3 - P0)
};

constexpr TetTable make_tets() {
    TetTable t = {};
    int n = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            if (b == a) continue;
            const int c = 3 - a - b;
            t.corner[n][0] = 0;
            t.corner[n][1] = (unsigned char)(1 << a);
            t.corner[n][2] = (unsigned char)((1 << a) | (1 << b));
            t.corner[n][3] = 7;
            t.odd[n] = (unsigned char)(((a > b) + (a > c) + (b > c)) & 1);
            ++n;
        }
    return t;
}

// one of the 16 inside patterns of a tetrahedron (bit c = corner c inside): bits 0-1 the triangle count, then six 4-bit fields, the three
// edges (p << 2 | q, corners p < q) of triangle 0 and of triangle 1, counter-clockwise seen from outside for an EVEN tetrahedron
constexpr unsigned tet_case(int mask) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int c = 0; c < 4; ++c) {
        if ((mask >> c) & 1) in[ni++] = c;
        else out[no++] = c;
    }
    if (ni == 0 || ni == 4) return 0u;
    int perm[4] = {0, 0, 0, 0};
    for (int i = 0; i < ni; ++i) perm[i] = in[i];
    for (int i = 0; i < no; ++i) perm[ni + i] = out[i];
    int inv = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j) inv += perm[i] > perm[j];
    int e[6] = {0, 0, 0, 0, 0, 0};
    auto edge = [](int a, int b) { return a < b ? (a << 2 | b) : (b << 2 | a); };
    int count = 1;
    if (ni == 1) {
        e[0] = edge(in[0], out[0]); e[1] = edge(in[0], out[1]); e[2] = edge(in[0], out[2]);
    } else if (ni == 3) {
        e[0] = edge(in[0], out[0]); e[1] = edge(in[1], out[0]); e[2] = edge(in[2], out[0]);
    } else {
        // the quad (AC, AD, BD, BC), A < B inside, C < D outside, cut along AC - BD
        count = 2;
        e[0] = edge(in[0], out[0]); e[1] = edge(in[0], out[1]); e[2] = edge(in[1], out[1]);
        e[3] = edge(in[0], out[0]); e[4] = edge(in[1], out[1]); e[5] = edge(in[1], out[0]);
    }
    if (inv & 1) {                                            // an odd arrangement of (inside..., outside...): the mirror image
        int t = e[1]; e[1] = e[2]; e[2] = t;
        t = e[4]; e[4] = e[5]; e[5] = t;
    }
    unsigned r = (unsigned)count;
    for (int i = 0; i < 6; ++i) r |= (unsigned)e[i] << (2 + 4 * i);
    return r;
}

__constant__ TetTable d_tets = make_tets();
__constant__ unsigned d_case[16] = {tet_case(0), tet_case(1), tet_case(2), tet_case(3), tet_case(4), tet_case(5), tet_case(6), tet_case(7),
                                    tet_case(8), tet_case(9), tet_case(10), tet_case(11), tet_case(12), tet_case(13), tet_case(14), tet_case(15)};

struct Grid {
    int nx, ny, nz;
    float lo[3], h[3];
    float level;
};

// ---- workspace --------------------------------------------------------------------------------------------------------------------------
struct Layout {
    int64_t n, words, spans;                                  // grid vertices, words of kWord, spans of kScanSpan
    int64_t off_span_off, off_span_sum, off_pre, off_flags, off_fcnt, bytes;
};

inline Layout layout_of(int nx, int ny, int nz) {
    Layout L;
    L.n = (int64_t)nx * ny * nz;
    L.words = (L.n + kWord - 1) / kWord;
    L.spans = (L.words + kThreads - 1) / kThreads;
    L.off_span_off = kHeaderBytes;
    L.off_span_sum = L.off_span_off + L.spans * 16;
    L.off_pre = L.off_span_sum + L.spans * 16;
    L.off_flags = (L.off_pre + L.words * 4 + 15) / 16 * 16;
    L.off_fcnt = L.off_flags + L.words * kWord;
    L.bytes = L.off_fcnt + L.words * kWord;
    return L;
}

struct Work {
    int64_t* counts;                                          // {n_verts, n_faces}
    int64_t* span_off;                                        // [spans][2] exclusive
    int64_t* span_sum;                                        // [spans][2]
    uint32_t* pre;                                            // [words] in-span exclusive prefix: vertices | faces << 16
    uint8_t* flags;                                           // [8 words] bit d = the edge in direction d is crossed
    uint8_t* fcnt;                                            // [8 words] faces of the cell anchored here
};

inline Work work_of(void* ws, const Layout& L) {
    char* b = static_cast<char*>(ws);
    Work w;
    w.counts = reinterpret_cast<int64_t*>(b);
    w.span_off = reinterpret_cast<int64_t*>(b + L.off_span_off);
    w.span_sum = reinterpret_cast<int64_t*>(b + L.off_span_sum);
    w.pre = reinterpret_cast<uint32_t*>(b + L.off_pre);
    w.flags = reinterpret_cast<uint8_t*>(b + L.off_flags);
    w.fcnt = reinterpret_cast<uint8_t*>(b + L.off_fcnt);
    return w;
}

// ---- classify ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int faces_of_cube(unsigned cube) {
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        int k = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) k += (cube >> d_tets.corner[t][c]) & 1u;
        n += (k == 2) ? 2 : ((k == 1 || k == 3) ? 1 : 0);
    }
    return n;
}

__global__ void __launch_bounds__(kThreads) iso_classify_kernel(const float* __restrict__ field, int nx, int ny, int nz, float level, int bricks_x,
                                                                int bricks_y, uint8_t* __restrict__ flags, uint8_t* __restrict__ fcnt) {
    __shared__ uint8_t s_in[kHalo * kHalo * kHalo];
    const int b = blockIdx.x;
    const int x0 = (b % bricks_x) * kBrick, y0 = ((b / bricks_x) % bricks_y) * kBrick, z0 = (b / (bricks_x * bricks_y)) * kBrick;
    // every load of the thread is issued before the first is used: the staging costs one memory latency, not kStage of them
    constexpr int kStaged = kHalo * kHalo * kHalo, kStage = (kStaged + kThreads - 1) / kThreads;
    float val[kStage];
#pragma unroll
    for (int r = 0; r < kStage; ++r) {
        const int s = threadIdx.x + r * kThreads;
        const int x = x0 + s % kHalo, y = y0 + (s / kHalo) % kHalo, z = z0 + s / (kHalo * kHalo);
        val[r] = (s < kStaged && x < nx && y < ny && z < nz) ? field[((int64_t)z * ny + y) * nx + x] : -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < kStage; ++r) {
        const int s = threadIdx.x + r * kThreads;
        if (s < kStaged) s_in[s] = val[r] > level ? 1 : 0;     // rule M2: a NaN compares false (and so does what lies beyond the grid)
    }
    __syncthreads();
    const int lx = threadIdx.x % kBrick, ly = threadIdx.x / kBrick;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= nx || y >= ny) return;
    for (int lz = 0; lz < kBrick; ++lz) {
        const int z = z0 + lz;
        if (z >= nz) break;
        const int s = (lz * kHalo + ly) * kHalo + lx;
        unsigned cube = 0;                                     // bit m = the vertex at offset mask m is inside (0 beyond the grid)
#pragma unroll
        for (int m = 0; m < 8; ++m) cube |= (unsigned)s_in[s + (m & 1) + ((m >> 1) & 1) * kHalo + (m >> 2) * kHalo * kHalo] << m;
        const unsigned there = (x + 1 < nx ? 1u : 0u) | (y + 1 < ny ? 2u : 0u) | (z + 1 < nz ? 4u : 0u);
        unsigned fl = 0;
#pragma unroll
        for (int m = 1; m < 8; ++m)
            if ((m & there) == (unsigned)m && (((cube >> m) ^ cube) & 1u)) fl |= 1u << (m - 1);
        const int64_t v = ((int64_t)z * ny + y) * nx + x;
        flags[v] = (uint8_t)fl;
        fcnt[v] = (uint8_t)((there == 7u && cube != 0u && cube != 255u) ? faces_of_cube(cube) : 0);
    }
}

// ---- scan -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_scan_add_int(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// the bytes of a word that belong to grid vertices below `n_valid` of its eight
__device__ __forceinline__ uint64_t low_bytes(int n_valid) { return n_valid >= 8 ? ~0ull : ((1ull << (8 * n_valid)) - 1ull); }
__device__ __forceinline__ int byte_sum(uint64_t w) { return (int)((w * 0x0101010101010101ull) >> 56); }      // bytes <= 12: no carry

__global__ void __launch_bounds__(kThreads) iso_span_kernel(const uint64_t* __restrict__ flags, const uint64_t* __restrict__ fcnt, int64_t n, int64_t words,
                                                            uint32_t* __restrict__ pre, int64_t* __restrict__ span_sum) {
    __shared__ int s_v[kThreads / 64], s_f[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int cv = 0, cf = 0;
    if (g < words) {
        const int64_t left = n - g * kWord;
        const uint64_t keep = low_bytes(left >= 8 ? 8 : (int)left);
        cv = __popcll(flags[g] & keep);
        cf = byte_sum(fcnt[g] & keep);
    }
    const int iv = wave_scan_add_int(cv, lane), jf = wave_scan_add_int(cf, lane);
    if (lane == 63) { s_v[wave] = iv; s_f[wave] = jf; }
    __syncthreads();
    int bv = 0, bf = 0;
    for (int w = 0; w < wave; ++w) { bv += s_v[w]; bf += s_f[w]; }
    if (g < words) pre[g] = (uint32_t)(bv + iv - cv) | ((uint32_t)(bf + jf - cf) << 16);
    if (threadIdx.x == kThreads - 1) {
        span_sum[2 * (int64_t)blockIdx.x] = bv + iv;
        span_sum[2 * (int64_t)blockIdx.x + 1] = bf + jf;
    }
}

// exclusive scan of the spans' sums by one workgroup (raster_device.h's raster_scan_kernel, 64-bit and two columns): totals -> counts
__global__ void __launch_bounds__(kThreads) iso_scan_kernel(const int64_t* __restrict__ span_sum, int64_t spans, int64_t* __restrict__ span_off,
                                                            int64_t* __restrict__ counts) {
    __shared__ int64_t part[kThreads][2];
    const int64_t per = (spans + kThreads - 1) / kThreads, lo = threadIdx.x * per, hi = lo + per < spans ? lo + per : spans;
    int64_t sv = 0, sf = 0;
    for (int64_t i = lo; i < hi; ++i) { sv += span_sum[2 * i]; sf += span_sum[2 * i + 1]; }
    part[threadIdx.x][0] = sv;
    part[threadIdx.x][1] = sf;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t rv = 0, rf = 0;
        for (int i = 0; i < kThreads; ++i) {
            const int64_t tv = part[i][0], tf = part[i][1];
            part[i][0] = rv; part[i][1] = rf;
            rv += tv; rf += tf;
        }
        counts[0] = rv;
        counts[1] = rf;
    }
    __syncthreads();
    int64_t rv = part[threadIdx.x][0], rf = part[threadIdx.x][1];
    for (int64_t i = lo; i < hi; ++i) {
        span_off[2 * i] = rv; span_off[2 * i + 1] = rf;
        rv += span_sum[2 * i]; rf += span_sum[2 * i + 1];
    }
}

// ---- fill -------------------------------------------------------------------------------------------------------------------------------
struct Rank {
    const int64_t* span_off;
    const uint32_t* pre;
    const uint64_t* flags;
    const uint64_t* fcnt;
};

// rule M4: the rank of edge (v, d) among the crossed edges in ascending edge id
__device__ __forceinline__ int64_t vertex_rank(const Rank& r, int64_t v, int d) {
    const int64_t g = v / kWord;
    const int sh = (int)(v % kWord) * 8;
    const uint64_t w = r.flags[g];
    const unsigned own = (unsigned)(w >> sh) & 0xffu;
    return r.span_off[2 * (g / kThreads)] + (int64_t)(r.pre[g] & 0xffffu) + __popcll(w & ((1ull << sh) - 1ull)) + __popc(own & ((1u << d) - 1u));
}

__device__ __forceinline__ int64_t face_base(const Rank& r, int64_t v) {
    const int64_t g = v / kWord;
    const int sh = (int)(v % kWord) * 8;
    return r.span_off[2 * (g / kThreads) + 1] + (int64_t)(r.pre[g] >> 16) + byte_sum(r.fcnt[g] & ((1ull << sh) - 1ull));
}

// rule M6's gradient at grid vertex (x, y, z): central differences, one-sided at the box faces
__device__ __forceinline__ void gradient_at(const float* __restrict__ f, const Grid& G, int x, int y, int z, float* g) {
    const int64_t sx = 1, sy = G.nx, sz = (int64_t)G.nx * G.ny;
    const int64_t v = (int64_t)z * sz + (int64_t)y * sy + x;
    const int c[3] = {x, y, z}, n[3] = {G.nx, G.ny, G.nz};
    const int64_t s[3] = {sx, sy, sz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const bool lo = c[a] > 0, hi = c[a] + 1 < n[a];
        const float up = f[hi ? v + s[a] : v], dn = f[lo ? v - s[a] : v];
        g[a] = (up - dn) / ((lo && hi) ? 2.f * G.h[a] : G.h[a]);
    }
}

// the mesh vertices on the crossed edges `fl` of grid vertex v, the first of them of rank `first`
__device__ __forceinline__ void fill_vertex(const float* __restrict__ field, const Grid& G, int64_t v, unsigned fl, int64_t first, float* __restrict__ verts,
                                            float* __restrict__ normals, int64_t cap_verts) {
    const int x = (int)(v % G.nx), y = (int)((v / G.nx) % G.ny), z = (int)(v / ((int64_t)G.nx * G.ny));
    const unsigned there = (x + 1 < G.nx ? 1u : 0u) | (y + 1 < G.ny ? 2u : 0u) | (z + 1 < G.nz ? 4u : 0u);
    const float fa = field[v];
    const int ca[3] = {x, y, z};
    float pa[3], ga[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) pa[a] = fmaf((float)ca[a], G.h[a], G.lo[a]);
    if (normals) gradient_at(field, G, x, y, z, ga);
    int k = 0;
    for (int d = 0; d < 7; ++d) {
        if (!((fl >> d) & 1u)) continue;
        const int64_t at = first + k++;
        const int m = d + 1;
        // (never on a workspace nm_isosurface_count filled for this grid and level: the entry point compared the capacities with the counts)
        if (at < 0 || at >= cap_verts || (m & there) != (unsigned)m) return;
        const int cb[3] = {x + (m & 1), y + ((m >> 1) & 1), z + (m >> 2)};
        const float fb = field[((int64_t)cb[2] * G.ny + cb[1]) * G.nx + cb[0]];
        float t = (G.level - fa) / (fb - fa);                // IEEE division: hipcc rounds f32 / and sqrtf correctly unless told otherwise
        if (!(t >= 0.f && t <= 1.f)) t = 0.5f;                 // an endpoint that is NaN or infinite
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float pb = fmaf((float)cb[a], G.h[a], G.lo[a]);
            verts[3 * at + a] = fmaf(t, pb - pa[a], pa[a]);
        }
        if (!normals) continue;
        float gb[3], g[3];
        gradient_at(field, G, cb[0], cb[1], cb[2], gb);
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] = fmaf(t, gb[a] - ga[a], ga[a]);
        const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        const bool ok = len > 0.f && len < INFINITY;           // a NaN fails both
#pragma unroll
        for (int a = 0; a < 3; ++a) normals[3 * at + a] = ok ? -g[a] / len : 0.f;
    }
}

__global__ void __launch_bounds__(kThreads) iso_fill_verts_kernel(const float* __restrict__ field, Grid G, Rank r, int64_t n, float* __restrict__ verts,
                                                                  float* __restrict__ normals, int64_t cap_verts) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    const unsigned fl = reinterpret_cast<const uint8_t*>(r.flags)[v];
    if (fl) fill_vertex(field, G, v, fl, vertex_rank(r, v, 0), verts, normals, cap_verts);
}

// the faces of the cell anchored at grid vertex v (which has some, so x + 1 < nx, y + 1 < ny, z + 1 < nz: classify counted a cell), from face `at` on
__device__ __forceinline__ void fill_cell(const float* __restrict__ field, const Grid& G, const Rank& r, int64_t v, int64_t at, int32_t* __restrict__ faces,
                                          int64_t cap_faces) {
    const int64_t sy = G.nx, sz = (int64_t)G.nx * G.ny;
    if (v % G.nx + 1 >= G.nx || (v / G.nx) % G.ny + 1 >= G.ny || v / sz + 1 >= G.nz) return;      // (never, as in the vertex pass)
    unsigned cube = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) cube |= (field[v + (m & 1) + ((m >> 1) & 1) * sy + (m >> 2) * sz] > G.level ? 1u : 0u) << m;
    for (int t = 0; t < 6; ++t) {
        unsigned in4 = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) in4 |= ((cube >> d_tets.corner[t][c]) & 1u) << c;
        const unsigned rec = d_case[in4];
        const int count = (int)(rec & 3u);
        for (int k = 0; k < count; ++k, ++at) {
            if (at < 0 || at >= cap_faces) return;             // (never, as above)
            int32_t idx[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const unsigned pq = (rec >> (2 + 4 * (3 * k + e))) & 15u;
                const int mp = d_tets.corner[t][pq >> 2], mq = d_tets.corner[t][pq & 3u];
                idx[e] = (int32_t)vertex_rank(r, v + (mp & 1) + ((mp >> 1) & 1) * sy + (mp >> 2) * sz, (mq ^ mp) - 1);
            }
            const bool flip = d_tets.odd[t] != 0;              // rule M5: orientation from the case and the tetrahedron's parity alone
            faces[3 * at] = idx[0];
            faces[3 * at + 1] = flip ? idx[2] : idx[1];
            faces[3 * at + 2] = flip ? idx[1] : idx[2];
        }
    }
}

// (a thread per word of eight vertices, walking its non-empty bytes, was measured too: 1.2 to 2.4 times slower -- profiles/isosurface.md)
__global__ void __launch_bounds__(kThreads) iso_fill_faces_kernel(const float* __restrict__ field, Grid G, Rank r, int64_t n, int32_t* __restrict__ faces,
                                                                  int64_t cap_faces) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    if (reinterpret_cast<const uint8_t*>(r.fcnt)[v]) fill_cell(field, G, r, v, face_base(r, v), faces, cap_faces);
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------------
inline bool dims_ok(int nx, int ny, int nz) { return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < (1ll << 31); }

#define NM_ISO_ARGS(who)                                                                                                                     \
    NM_REQUIRE(field && aabb && workspace, who ": null pointer");                                                                            \
    NM_REQUIRE(dims_ok(nx, ny, nz), who ": bad grid %d x %d x %d (every dim >= 2, fewer than 2^31 vertices)", nx, ny, nz);                  \
    for (int a = 0; a < 3; ++a)                                                                                                              \
        NM_REQUIRE(std::isfinite(aabb[a]) && std::isfinite(aabb[3 + a]) && aabb[a] < aabb[3 + a] && std::isfinite(aabb[3 + a] - aabb[a]),                  \
                   who ": the box must be finite with lo < hi on every axis (axis %d: %g, %g)", a, (double)aabb[a], (double)aabb[3 + a]);   \
    NM_REQUIRE(std::isfinite(level), who ": level must be finite");                                                                               \
    NM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, who ": workspace must be 16-byte aligned");                              \
    NM_REQUIRE(workspace_bytes >= layout_of(nx, ny, nz).bytes, who ": workspace of %lld bytes, %lld needed", (long long)workspace_bytes,    \
               (long long)layout_of(nx, ny, nz).bytes)

inline Grid grid_of(int nx, int ny, int nz, const float* aabb, float level) {
    Grid G;
    G.nx = nx; G.ny = ny; G.nz = nz;
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        G.lo[a] = aabb[a];
        const float extent = aabb[3 + a] - aabb[a];           // rule M1: float32 at every step
        G.h[a] = extent / (float)(n[a] - 1);
    }
    G.level = level;
    return G;
}

}  // namespace

extern "C" {

int64_t nm_isosurface_workspace_bytes(int nx, int ny, int nz) {
    if (!dims_ok(nx, ny, nz)) {
        nm::set_error("nm_isosurface_workspace_bytes: bad grid %d x %d x %d (every dim >= 2, fewer than 2^31 vertices)", nx, ny, nz);
        return NM_ERR_ARG;
    }
    return layout_of(nx, ny, nz).bytes;
}

int nm_isosurface_count(const float* field, int nx, int ny, int nz, const float* aabb, float level, void* workspace, int64_t workspace_bytes,
                        int64_t* n_verts, int64_t* n_faces, nm_stream_t stream) {
    NM_ISO_ARGS("nm_isosurface_count");
    NM_REQUIRE(n_verts && n_faces, "nm_isosurface_count: null count pointer");
    const Layout L = layout_of(nx, ny, nz);
    const Work w = work_of(workspace, L);
    hipStream_t st = nm::as_stream(stream);
    const int bx = (nx + kBrick - 1) / kBrick, by = (ny + kBrick - 1) / kBrick, bz = (nz + kBrick - 1) / kBrick;
    const int64_t bricks = (int64_t)bx * by * bz;
    NM_REQUIRE(bricks < (1ll << 31), "nm_isosurface_count: %lld bricks, too many for one launch", (long long)bricks);
    hipLaunchKernelGGL(iso_classify_kernel, dim3((unsigned)bricks), dim3(kThreads), 0, st, field, nx, ny, nz, level, bx, by, w.flags, w.fcnt);
    hipLaunchKernelGGL(iso_span_kernel, dim3((unsigned)L.spans), dim3(kThreads), 0, st, reinterpret_cast<const uint64_t*>(w.flags),
                       reinterpret_cast<const uint64_t*>(w.fcnt), L.n, L.words, w.pre, w.span_sum);
    hipLaunchKernelGGL(iso_scan_kernel, dim3(1), dim3(kThreads), 0, st, w.span_sum, L.spans, w.span_off, w.counts);
    int rc = NM_OK;
    if ((rc = nm::check_launch("isosurface count kernels"))) return rc;
    int64_t counts[2] = {0, 0};                                // the one read-back
    if ((rc = nm::check_hip(hipMemcpyAsync(counts, w.counts, 16, hipMemcpyDeviceToHost, st), "nm_isosurface_count: read counts"))) return rc;
    if ((rc = nm::check_hip(hipStreamSynchronize(st), "nm_isosurface_count: sync"))) return rc;
    *n_verts = counts[0];
    *n_faces = counts[1];
    return NM_OK;
}

int nm_isosurface_fill(const float* field, int nx, int ny, int nz, const float* aabb, float level, const void* workspace, int64_t workspace_bytes,
                       float* verts, float* normals, int32_t* faces, int64_t cap_verts, int64_t cap_faces, nm_stream_t stream) {
    NM_ISO_ARGS("nm_isosurface_fill");
    NM_REQUIRE(cap_verts >= 0 && cap_faces >= 0, "nm_isosurface_fill: negative capacity");
    NM_REQUIRE((verts || cap_verts == 0) && (faces || cap_faces == 0), "nm_isosurface_fill: null output");      // (an empty tensor's pointer is null)
    const Layout L = layout_of(nx, ny, nz);
    const Work w = work_of(const_cast<void*>(workspace), L);
    hipStream_t st = nm::as_stream(stream);
    int rc = NM_OK;
    int64_t counts[2] = {0, 0};
    if ((rc = nm::check_hip(hipMemcpyAsync(counts, w.counts, 16, hipMemcpyDeviceToHost, st), "nm_isosurface_fill: read counts"))) return rc;
    if ((rc = nm::check_hip(hipStreamSynchronize(st), "nm_isosurface_fill: sync"))) return rc;
    NM_REQUIRE(counts[0] >= 0 && counts[1] >= 0 && counts[0] <= 7 * L.n && counts[1] <= 12 * L.n,
               "nm_isosurface_fill: the workspace holds no counts of this grid (run nm_isosurface_count on it first)");
    NM_REQUIRE(cap_verts >= counts[0] && cap_faces >= counts[1], "nm_isosurface_fill: capacity %lld vertices, %lld faces; the mesh has %lld, %lld",
               (long long)cap_verts, (long long)cap_faces, (long long)counts[0], (long long)counts[1]);
    if (counts[0] >= (1ll << 31) || counts[1] >= (1ll << 31)) {
        nm::set_error("nm_isosurface_fill: %lld vertices, %lld faces: face indices are int32", (long long)counts[0], (long long)counts[1]);
        return NM_ERR_UNSUPPORTED;
    }
    if (counts[0] == 0) return NM_OK;
    const Grid G = grid_of(nx, ny, nz, aabb, level);
    const Rank r = {w.span_off, w.pre, reinterpret_cast<const uint64_t*>(w.flags), reinterpret_cast<const uint64_t*>(w.fcnt)};
    const unsigned blocks = (unsigned)((L.n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(iso_fill_verts_kernel, dim3(blocks), dim3(kThreads), 0, st, field, G, r, L.n, verts, normals, cap_verts);
    if (counts[1] > 0) hipLaunchKernelGGL(iso_fill_faces_kernel, dim3(blocks), dim3(kThreads), 0, st, field, G, r, L.n, faces, cap_faces);
    return nm::check_launch("isosurface fill kernels");
}

}  // extern "C"
