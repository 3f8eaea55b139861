// An extracted mesh animated by the body it was bound to: per vertex and frame the barycentric blend of three per-vertex transforms of the
// body, applied to the canonical point and (by the cofactor matrix) to the canonical normal -- include/neuman_hip.h 'mesh pose' writes the
// contract out (rules P1-P6); tests/helpers/mesh_pose_ref.py restates it in numpy.  It is the blend of the observation -> canonical warp
// (warp.hip; reference utils/ray_utils.py:56-58) run forwards, without the inverse.  neuman_hip/mesh_pose.py (bind_mesh, pose_mesh,
// pose_mesh_frames) is the Python surface.
//
//   one thread per vertex, the frame in grid.y: the binding row (36 bytes) and the canonical point are read once per (frame, vertex), the three
//   rows of the frame's transform table are gathered with 16-byte loads (rows 0-2 only: rule P3 never reads row 3), everything after that is
//   float64 arithmetic in registers, and the thread stores 12 or 24 bytes.  Nothing is shared between threads: no LDS, no workspace, no float
//   atomic; the one atomic is the integer count of rule P5.
//
// -ffp-contract=off (build.py) and no fma() here: every product and every sum below is rounded on its own, in the association the header states.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxFrames = 65535;                             // the frame is grid.y

// rows 0-2 of one 4x4, as float64 whatever the table holds (a float32 converts exactly)
struct Rows {
    double m[12];
};

__device__ __forceinline__ Rows load_rows(const double* __restrict__ row) {
    Rows r;
    const double2* p = reinterpret_cast<const double2*>(row);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double2 v = p[k];
        r.m[2 * k] = v.x;
        r.m[2 * k + 1] = v.y;
    }
    return r;
}

__device__ __forceinline__ Rows load_rows(const float* __restrict__ row) {
    Rows r;
    const float4* p = reinterpret_cast<const float4*>(row);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 v = p[k];
        r.m[4 * k] = (double)v.x;
        r.m[4 * k + 1] = (double)v.y;
        r.m[4 * k + 2] = (double)v.z;
        r.m[4 * k + 3] = (double)v.w;
    }
    return r;
}

__device__ __forceinline__ bool row_ok(int32_t i, int64_t t_rows) { return i >= 0 && (int64_t)i < t_rows; }

// rule P4: cross(a, b), each component two products and one subtraction
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

template <typename TT, bool kNormals>
__global__ void __launch_bounds__(kThreads) mesh_pose_kernel(const TT* __restrict__ T, int64_t t_rows, const int32_t* __restrict__ tri,
                                                             const float* __restrict__ bary, int per_frame_binding, const float* __restrict__ pts,
                                                             const float* __restrict__ normals, int64_t N, float* __restrict__ out_pts,
                                                             float* __restrict__ out_normals, int32_t* n_invalid) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int64_t b = blockIdx.y;
    const int64_t bind = ((per_frame_binding ? b * N : 0) + i) * 3;       // rule P1: every offset in 64 bits
    const int64_t out = (b * N + i) * 3;
    const int32_t t0 = tri[bind], t1 = tri[bind + 1], t2 = tri[bind + 2];
    // rule P5: the range check comes before any use of an index
    if (!(row_ok(t0, t_rows) && row_ok(t1, t_rows) && row_ok(t2, t_rows))) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            out_pts[out + r] = NAN;
            if (kNormals) out_normals[out + r] = NAN;
        }
        if (n_invalid) atomicAdd(n_invalid, 1);
        return;
    }
    const TT* table = T + b * t_rows * 16;
    const Rows A = load_rows(table + (int64_t)t0 * 16), B = load_rows(table + (int64_t)t1 * 16), C = load_rows(table + (int64_t)t2 * 16);
    const double b0 = (double)bary[bind], b1 = (double)bary[bind + 1], b2 = (double)bary[bind + 2];
    double M[12];                                             // rule P2
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = (b0 * A.m[k] + b1 * B.m[k]) + b2 * C.m[k];
    const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r)                               // rule P3
        out_pts[out + r] = (float)(((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3]);
    if (kNormals) {                                           // rule P4
        const double n0 = (double)normals[3 * i], n1 = (double)normals[3 * i + 1], n2 = (double)normals[3 * i + 2];
        double cof[3][3];
        cross3(M + 4, M + 8, cof[0]);
        cross3(M + 8, M, cof[1]);
        cross3(M, M + 4, cof[2]);
        double n[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) n[r] = (cof[r][0] * n0 + cof[r][1] * n1) + cof[r][2] * n2;
        const double s = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        const bool usable = s != 0.0 && isfinite(s);
        const double len = sqrt(s);
#pragma unroll
        for (int r = 0; r < 3; ++r) out_normals[out + r] = usable ? (float)(n[r] / len) : 0.f;
    }
}

template <typename TT>
void launch(const void* T, int64_t t_rows, int B, const int32_t* tri, const float* bary, int per_frame_binding, const float* pts, const float* normals,
            int64_t N, float* out_pts, float* out_normals, int32_t* n_invalid, hipStream_t st) {
    const dim3 grid((unsigned)((N + kThreads - 1) / kThreads), (unsigned)B);
    const TT* t = static_cast<const TT*>(T);
    if (normals)
        hipLaunchKernelGGL((mesh_pose_kernel<TT, true>), grid, dim3(kThreads), 0, st, t, t_rows, tri, bary, per_frame_binding, pts, normals, N, out_pts,
                           out_normals, n_invalid);
    else
        hipLaunchKernelGGL((mesh_pose_kernel<TT, false>), grid, dim3(kThreads), 0, st, t, t_rows, tri, bary, per_frame_binding, pts, normals, N, out_pts,
                           out_normals, n_invalid);
}

}  // namespace

extern "C" {

int nm_mesh_pose_batch(const void* T, int t_f64, int64_t t_rows, int B, const int32_t* tri, const float* bary, int per_frame_binding, const float* pts,
                       const float* normals, int64_t N, float* out_pts, float* out_normals, int32_t* n_invalid, nm_stream_t stream) {
    NM_REQUIRE(B >= 1 && B <= kMaxFrames, "nm_mesh_pose_batch: B = %d must be in [1, %d]", B, kMaxFrames);
    NM_REQUIRE(N >= 0 && N < (1ll << 31), "nm_mesh_pose_batch: N = %lld must be in [0, 2^31)", (long long)N);
    NM_REQUIRE(t_rows >= 1 && t_rows < (1ll << 31), "nm_mesh_pose_batch: t_rows = %lld must be in [1, 2^31)", (long long)t_rows);
    NM_REQUIRE(t_f64 == 0 || t_f64 == 1, "nm_mesh_pose_batch: t_f64 = %d must be 0 or 1", t_f64);
    NM_REQUIRE(per_frame_binding == 0 || per_frame_binding == 1, "nm_mesh_pose_batch: per_frame_binding = %d must be 0 or 1", per_frame_binding);
    NM_REQUIRE((normals == nullptr) == (out_normals == nullptr), "nm_mesh_pose_batch: normals and out_normals go together (%s is null)",
               normals ? "out_normals" : "normals");
    if (N == 0) return NM_OK;
    NM_REQUIRE(T && tri && bary && pts && out_pts, "nm_mesh_pose_batch: null %s", !T ? "T" : !tri ? "tri" : !bary ? "bary" : !pts ? "pts" : "out_pts");
    NM_REQUIRE((reinterpret_cast<uintptr_t>(T) & 15) == 0, "nm_mesh_pose_batch: T must be 16-byte aligned");
    hipStream_t st = nm::as_stream(stream);
    if (t_f64)
        launch<double>(T, t_rows, B, tri, bary, per_frame_binding, pts, normals, N, out_pts, out_normals, n_invalid, st);
    else
        launch<float>(T, t_rows, B, tri, bary, per_frame_binding, pts, normals, N, out_pts, out_normals, n_invalid, st);
    return nm::check_launch("mesh pose kernel");
}

}  // extern "C"
