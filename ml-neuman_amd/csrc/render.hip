// Sequenced per-ray entry points (SURVEY 8b's proposed ABI: nm_render_rays_bkg / _human, nm_merge_composite): ONE C call per pass of the
// reference's renderers, the kernels of the pass enqueued back to back on the caller's stream -- no host synchronisation inside, no
// hidden allocation (every intermediate lives in the caller's workspace or output arrays), same kernels and therefore the same bits
// as the step-by-step entry points.  Reference: utils/render_utils.py:131-151 / 287-297 (two-pass background), :213-229 / 320-329
// (human pass of already compacted hit rays), :330-345 / 441-456 (merge + composite).
#include "common.h"
#include <string>

namespace {
inline int64_t align4(int64_t n) { return (n + 3) & ~int64_t(3); }        // keep every sub-array 16-byte aligned

// The pass of a call whose output is composited and nothing else, in its two forms: the whole-network launch (lw == nullptr: what the plain
// entries enqueue), or the trunk / colour-head pair on live samples only (the *_live entries: nm_mlp_forward_*_live).  The passes of one call
// use the workspace one after another.
struct LiveWs {
    void* ws; int64_t bytes; int64_t chunk;
};
int shade_rays(const LiveWs* lw, nm_mlp_t m, const float* o, const float* d, const float* z, int64_t R, int S, int prec, float scale, float* out, nm_stream_t st) {
    return lw ? nm_mlp_forward_rays_live(m, o, d, z, R, S, prec, scale, out, lw->ws, lw->bytes, lw->chunk, st) : nm_mlp_forward_rays(m, o, d, z, R, S, prec, scale, out, st);
}
int shade_points(const LiveWs* lw, nm_mlp_t m, const float* pts, const float* dirs, int64_t n, int prec, float scale, float* out, nm_stream_t st) {
    return lw ? nm_mlp_forward_live(m, pts, dirs, n, prec, scale, out, lw->ws, lw->bytes, lw->chunk, st) : nm_mlp_forward(m, pts, dirs, n, prec, scale, out, st);
}
int shade_samples(const LiveWs* lw, nm_mlp_t m, const float* o, const float* d, const float* z, int64_t R, int S, const int32_t* idx, const int32_t* n_dev, int prec,
                  float scale, float* out, nm_stream_t st) {
    return lw ? nm_mlp_forward_samples_live(m, o, d, z, R, S, idx, n_dev, R * S, prec, scale, out, lw->ws, lw->bytes, lw->chunk, st)
              : nm_mlp_forward_samples(m, o, d, z, R, S, idx, n_dev, R * S, prec, scale, out, st);
}
int shade_listed(const LiveWs* lw, nm_mlp_t m, const float* pts, const float* dirs, int64_t n, const int32_t* idx, const int32_t* n_dev, int prec, float scale,
                 float* out, nm_stream_t st) {
    return lw ? nm_mlp_forward_listed_live(m, pts, dirs, n, idx, n_dev, n, prec, scale, out, lw->ws, lw->bytes, lw->chunk, st)
              : nm_mlp_forward_listed(m, pts, dirs, n, idx, n_dev, n, prec, scale, out, st);
}
}  // namespace

// what a *_live entry checks of its live workspace before anything is enqueued: a composited pass of n samples (S_ray to a ray) at precision prec
#define NM_LIVE_WS_REQUIRE(who, prec, n, S_ray)                                                                                                     \
    NM_REQUIRE((reinterpret_cast<uintptr_t>(live_ws) & 15) == 0, who ": live_ws must be 16-byte aligned");                                          \
    NM_REQUIRE(chunk_samples <= 0 || chunk_samples >= (S_ray), who ": chunk_samples holds no whole ray of %d samples", (int)(S_ray));               \
    NM_REQUIRE((prec) != NM_PREC_I8X3 || (n) <= 0 || (live_ws && live_ws_bytes >= nm_mlp_live_workspace_bytes(n, chunk_samples)),                   \
               who ": live workspace of %lld bytes, %lld needed", (long long)live_ws_bytes, (long long)nm_mlp_live_workspace_bytes(n, chunk_samples))

extern "C" {

int64_t nm_render_rays_bkg_workspace_floats(int64_t R, int S, int N) {
    // coarse z [R,S] | coarse raw [R,S,4] | coarse weights [R,S] | per-ray scratch of the coarse composite [R,6]
    return N > 0 ? align4(R * S) + align4(R * S * 4) + align4(R * S) + align4(R * 6) : align4(R * 6);
}

static int render_rays_bkg(const LiveWs* lw, nm_mlp_t coarse, nm_mlp_t fine, const float* origin, const float* direction, const float* near, const float* far,
                           int64_t R, int S, int N, const float* t_vals, const float* u, int white_bkg, int precision_coarse, int precision_fine,
                           float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, nm_stream_t stream) {
    const char* who = lw ? "nm_render_rays_bkg_live" : "nm_render_rays_bkg";       // (one body, two entries: errors name the one that was called)
    NM_REQUIRE(R == 0 || (coarse && origin && direction && near && far && t_vals && workspace && raw_out && z_out), "%s: null pointer", who);
    NM_REQUIRE(R >= 0 && S >= 1 && N >= 0 && (N == 0) == (fine == nullptr), "%s: a fine net and N > 0 importance samples go together (S=%d N=%d)", who, S, N);
    NM_REQUIRE(N == 0 || u, "%s: u [N] is missing", who);
    if (R == 0) return NM_OK;
    int rc;
    float* scratch = workspace + (N > 0 ? align4(R * S) + align4(R * S * 4) + align4(R * S) : 0);      // [R,6]
    if (!fine) {                                                  // one pass: its output is what is composited
        if ((rc = nm_ray_to_samples(origin, direction, near, far, R, S, t_vals, 0, nullptr, nullptr, nullptr, z_out, stream))) return rc;
        if ((rc = shade_rays(lw, coarse, origin, direction, z_out, R, S, precision_coarse, 1.f, raw_out, stream))) return rc;
    } else {
        float* zc = workspace;
        float* rawc = zc + align4(R * S);
        float* wc = rawc + align4(R * S * 4);
        // (scratch: rgb [R,3] | disp | acc | depth of the coarse composite, discarded as the reference discards them, :139-141)
        if ((rc = nm_ray_to_samples(origin, direction, near, far, R, S, t_vals, 0, nullptr, nullptr, nullptr, zc, stream))) return rc;
        if ((rc = nm_mlp_sigma_rays(coarse, origin, direction, zc, R, S, precision_coarse, 1.f, rawc, stream))) return rc;
        // (the coarse composite's colours are discarded, as the reference discards them, :139-141: ONE kernel from sigma to the samples)
        (void)wc;
        if ((rc = nm_importance_from_raw(rawc, zc, direction, R, S, u, N, z_out, nullptr, stream))) return rc;
        if ((rc = shade_rays(lw, fine, origin, direction, z_out, R, S + N, precision_fine, 1.f, raw_out, stream))) return rc;
    }
    if (rgb) {
        NM_REQUIRE(depth && acc, "%s: rgb, depth and acc go together", who);
        if ((rc = nm_composite(raw_out, z_out, direction, R, S + N, white_bkg, nullptr, rgb, scratch + 3 * R, acc, nullptr, depth, stream))) return rc;
    }
    return NM_OK;
}

int nm_render_rays_bkg(nm_mlp_t coarse, nm_mlp_t fine, const float* origin, const float* direction, const float* near, const float* far,
                       int64_t R, int S, int N, const float* t_vals, const float* u, int white_bkg, int precision_coarse, int precision_fine,
                       float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, nm_stream_t stream) {
    return render_rays_bkg(nullptr, coarse, fine, origin, direction, near, far, R, S, N, t_vals, u, white_bkg, precision_coarse, precision_fine, workspace, raw_out,
                           z_out, rgb, depth, acc, stream);
}

int nm_render_rays_bkg_live(nm_mlp_t coarse, nm_mlp_t fine, const float* origin, const float* direction, const float* near, const float* far,
                            int64_t R, int S, int N, const float* t_vals, const float* u, int white_bkg, int precision_coarse, int precision_fine,
                            float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, void* live_ws, int64_t live_ws_bytes,
                            int64_t chunk_samples, nm_stream_t stream) {
    NM_REQUIRE(S >= 1 && N >= 0, "nm_render_rays_bkg_live: bad sizes");
    NM_LIVE_WS_REQUIRE("nm_render_rays_bkg_live", fine ? precision_fine : precision_coarse, R * (int64_t)(S + N), S + N);
    const LiveWs lw{live_ws, live_ws_bytes, chunk_samples};
    return render_rays_bkg(&lw, coarse, fine, origin, direction, near, far, R, S, N, t_vals, u, white_bkg, precision_coarse, precision_fine, workspace, raw_out,
                           z_out, rgb, depth, acc, stream);
}

int64_t nm_render_rays_human_workspace_floats(int64_t R, int S, int posed) {
    // posed: observation-space points [R,S,3] | canonical points | canonical directions;  + disp [R]
    return (posed ? 3 * align4(R * S * 3) : 0) + align4(R);
}

static int render_rays_human(const LiveWs* lw, nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* origin, const float* direction, const float* near,
                             const float* far, int64_t R, int S, const float* t_vals, int white_bkg, float sigma_scale, int precision,
                             float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, nm_stream_t stream) {
    const char* who = lw ? "nm_render_rays_human_live" : "nm_render_rays_human";       // (one body, two entries: errors name the one that was called)
    NM_REQUIRE(R == 0 || (human && origin && direction && near && far && t_vals && workspace && raw_out && z_out), "%s: null pointer", who);
    NM_REQUIRE(R >= 0 && S >= 1 && (mesh == nullptr) == (T == nullptr), "%s: a posed mesh and its transforms go together", who);
    if (R == 0) return NM_OK;
    int rc;
    float* disp = workspace + (mesh ? 3 * align4(R * S * 3) : 0);
    if (!mesh) {                                                  // canonical render (render_can=True, :213-216): the camera ray is the view direction
        if ((rc = nm_ray_to_samples(origin, direction, near, far, R, S, t_vals, 0, nullptr, nullptr, nullptr, z_out, stream))) return rc;
        if ((rc = shade_rays(lw, human, origin, direction, z_out, R, S, precision, sigma_scale, raw_out, stream))) return rc;
    } else {                                                      // posed: warp the samples, directions = differences of warped points (:217-227)
        float* pts = workspace;
        float* can_pts = pts + align4(R * S * 3);
        float* can_dirs = can_pts + align4(R * S * 3);
        if ((rc = nm_ray_to_samples(origin, direction, near, far, R, S, t_vals, 0, nullptr, pts, nullptr, z_out, stream))) return rc;
        if ((rc = nm_warp_to_canonical(mesh, pts, R, S, T, can_pts, can_dirs, nullptr, stream))) return rc;
        if ((rc = shade_points(lw, human, can_pts, can_dirs, R * S, precision, sigma_scale, raw_out, stream))) return rc;
    }
    if (rgb) {
        NM_REQUIRE(depth && acc, "%s: rgb, depth and acc go together", who);
        if ((rc = nm_composite(raw_out, z_out, direction, R, S, white_bkg, nullptr, rgb, disp, acc, nullptr, depth, stream))) return rc;
    }
    return NM_OK;
}

int nm_render_rays_human(nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* origin, const float* direction, const float* near,
                         const float* far, int64_t R, int S, const float* t_vals, int white_bkg, float sigma_scale, int precision,
                         float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, nm_stream_t stream) {
    return render_rays_human(nullptr, human, mesh, T, origin, direction, near, far, R, S, t_vals, white_bkg, sigma_scale, precision, workspace, raw_out, z_out, rgb,
                             depth, acc, stream);
}

int nm_render_rays_human_live(nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* origin, const float* direction, const float* near,
                              const float* far, int64_t R, int S, const float* t_vals, int white_bkg, float sigma_scale, int precision,
                              float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, void* live_ws, int64_t live_ws_bytes,
                              int64_t chunk_samples, nm_stream_t stream) {
    NM_REQUIRE(S >= 1, "nm_render_rays_human_live: bad sizes");
    NM_LIVE_WS_REQUIRE("nm_render_rays_human_live", precision, R * (int64_t)S, S);
    const LiveWs lw{live_ws, live_ws_bytes, chunk_samples};
    return render_rays_human(&lw, human, mesh, T, origin, direction, near, far, R, S, t_vals, white_bkg, sigma_scale, precision, workspace, raw_out, z_out, rgb,
                             depth, acc, stream);
}

// K11b: the human pass with occupancy-grid empty-space skipping (occupancy.hip).  The workspace starts with nm_render_rays_human's layout
// (posed: points | canonical points | canonical directions; disp), then the kept list and the compaction's scratch.
int64_t nm_render_rays_human_occ_workspace_floats(int64_t R, int S, int posed) {
    return nm_render_rays_human_workspace_floats(R, S, posed) + align4(R * S) + align4(nm_occ_compact_workspace_ints(R * S));
}

static int render_rays_human_occ(const LiveWs* lw, nm_mlp_t human, nm_mesh_t mesh, const double* T, const uint32_t* bits, int res, const float* aabb,
                                 const float* origin, const float* direction, const float* near, const float* far, int64_t R, int S, const float* t_vals,
                                 int white_bkg, float sigma_scale, int precision, float* workspace, float* raw_out, float* z_out, int32_t* counts, float* rgb,
                                 float* depth, float* acc, nm_stream_t stream) {
    const char* who = lw ? "nm_render_rays_human_occ_live" : "nm_render_rays_human_occ";       // (one body, two entries: errors name the one that was called)
    NM_REQUIRE(bits && aabb && counts, "%s: null pointer", who);
    NM_REQUIRE(R == 0 || (human && origin && direction && near && far && t_vals && workspace && raw_out && z_out), "%s: null pointer", who);
    NM_REQUIRE(R >= 0 && S >= 1 && (mesh == nullptr) == (T == nullptr), "%s: a posed mesh and its transforms go together", who);
    NM_REQUIRE(R * (int64_t)S < (1ll << 31), "%s: too many samples (R=%lld S=%d)", who, (long long)R, S);
    hipStream_t st = nm::as_stream(stream);
    int rc;
    if (R == 0) return nm::check_hip(hipMemsetAsync(counts, 0, 8, st), (std::string(who) + ": counts").c_str());
    // a skipped sample keeps raw = 0: alpha 0, weight 0 -- what relu(sigma) = 0 gives
    if ((rc = nm::check_hip(hipMemsetAsync(raw_out, 0, (size_t)(R * S) * 16, st), (std::string(who) + ": raw").c_str()))) return rc;
    const int64_t base = nm_render_rays_human_workspace_floats(R, S, mesh != nullptr);
    float* disp = workspace + (mesh ? 3 * align4(R * S * 3) : 0);
    int32_t* idx = reinterpret_cast<int32_t*>(workspace + base);
    int32_t* cws = idx + align4(R * S);
    if (!mesh) {                                                  // canonical: the grid is tested on o + d z itself (in_mode 3)
        if ((rc = nm_ray_to_samples(origin, direction, near, far, R, S, t_vals, 0, nullptr, nullptr, nullptr, z_out, stream))) return rc;
        if ((rc = nm_occ_compact_samples(bits, res, aabb, origin, direction, z_out, R, S, idx, counts, cws, stream))) return rc;
        if ((rc = shade_samples(lw, human, origin, direction, z_out, R, S, idx, counts, precision, sigma_scale, raw_out, stream))) return rc;
    } else {                                                      // posed: the grid lives in canonical space -- tested on the WARPED points (in_mode 4)
        float* pts = workspace;
        float* can_pts = pts + align4(R * S * 3);
        float* can_dirs = can_pts + align4(R * S * 3);
        if ((rc = nm_ray_to_samples(origin, direction, near, far, R, S, t_vals, 0, nullptr, pts, nullptr, z_out, stream))) return rc;
        if ((rc = nm_warp_to_canonical(mesh, pts, R, S, T, can_pts, can_dirs, nullptr, stream))) return rc;
        if ((rc = nm_occ_compact_points(bits, res, aabb, can_pts, R * S, idx, counts, cws, stream))) return rc;
        if ((rc = shade_listed(lw, human, can_pts, can_dirs, R * S, idx, counts, precision, sigma_scale, raw_out, stream))) return rc;
    }
    if (rgb) {
        NM_REQUIRE(depth && acc, "%s: rgb, depth and acc go together", who);
        if ((rc = nm_composite(raw_out, z_out, direction, R, S, white_bkg, nullptr, rgb, disp, acc, nullptr, depth, stream))) return rc;
    }
    return NM_OK;
}

int nm_render_rays_human_occ(nm_mlp_t human, nm_mesh_t mesh, const double* T, const uint32_t* bits, int res, const float* aabb, const float* origin,
                             const float* direction, const float* near, const float* far, int64_t R, int S, const float* t_vals, int white_bkg,
                             float sigma_scale, int precision, float* workspace, float* raw_out, float* z_out, int32_t* counts, float* rgb, float* depth,
                             float* acc, nm_stream_t stream) {
    return render_rays_human_occ(nullptr, human, mesh, T, bits, res, aabb, origin, direction, near, far, R, S, t_vals, white_bkg, sigma_scale, precision, workspace,
                                 raw_out, z_out, counts, rgb, depth, acc, stream);
}

int nm_render_rays_human_occ_live(nm_mlp_t human, nm_mesh_t mesh, const double* T, const uint32_t* bits, int res, const float* aabb, const float* origin,
                                  const float* direction, const float* near, const float* far, int64_t R, int S, const float* t_vals, int white_bkg,
                                  float sigma_scale, int precision, float* workspace, float* raw_out, float* z_out, int32_t* counts, float* rgb, float* depth,
                                  float* acc, void* live_ws, int64_t live_ws_bytes, int64_t chunk_samples, nm_stream_t stream) {
    NM_REQUIRE(S >= 1, "nm_render_rays_human_occ_live: bad sizes");
    NM_LIVE_WS_REQUIRE("nm_render_rays_human_occ_live", precision, R * (int64_t)S, S);
    const LiveWs lw{live_ws, live_ws_bytes, chunk_samples};
    return render_rays_human_occ(&lw, human, mesh, T, bits, res, aabb, origin, direction, near, far, R, S, t_vals, white_bkg, sigma_scale, precision, workspace,
                                 raw_out, z_out, counts, rgb, depth, acc, stream);
}

// (the merged list lives in LDS now: nothing is needed; kept for callers that size a workspace)
int64_t nm_merge_composite_workspace_floats(int64_t R, int Sa, int Sb) { (void)R; (void)Sa; (void)Sb; return 4; }

int nm_merge_composite(const float* za, const float* rawa, int Sa, const float* zb, const float* rawb, int Sb, int64_t R, const float* rays_d,
                       int white_bkg, float* workspace, float* rgb, float* depth, float* acc, nm_stream_t stream) {
    (void)workspace;
    NM_REQUIRE(R == 0 || (za && rawa && zb && rawb && rays_d && rgb && depth && acc), "nm_merge_composite: null pointer");
    if (R == 0) return NM_OK;
    const float* zs[2] = {za, zb};
    const float* raws[2] = {rawa, rawb};
    const int Ss[2] = {Sa, Sb};
    return nm_merge_composite_lists(2, zs, raws, nullptr, Ss, R, rays_d, white_bkg, rgb, depth, acc, stream);
}

// ---- render_hybrid_nerf's per-batch body (utils/render_utils.py:287-353) as one call: two-pass background for every ray and its
// composite (what a ray that misses the body keeps, :303-311), near / far against the posed body, compaction of the hit rays (the one
// host read of the call: their count -- the reference's boolean-mask indexing implies the same), human pass of the hit rays, merged
// composite (:330-345) and the human-only accumulation (:345-350) scattered back.  Built from the entry points above and below: same
// kernels, same bits as calling them one by one (tests/test_hip_fused.py).
namespace {
struct HybridWs {
    float *near_b, *far_b, *bkg_ws, *raw_b, *z_b, *near_h, *far_h, *ho, *hd, *hn, *hf, *bz, *braw, *h_raw, *h_z, *human_ws, *merge_ws, *rgb_h, *depth_h, *acc_h,
        *scratch;
    int32_t *hit, *counts, *cws;
    int64_t total;
};
inline HybridWs hybrid_layout(float* base, int64_t R, int S, int N, int Sh) {
    HybridWs w;
    int64_t o = 0;
    auto take = [&](int64_t n) { float* p = base ? base + o : nullptr; o += align4(n); return p; };
    const int Sb = S + N;
    w.near_b = take(R); w.far_b = take(R);
    w.bkg_ws = take(nm_render_rays_bkg_workspace_floats(R, S, N));
    w.raw_b = take(R * Sb * 4); w.z_b = take(R * Sb);
    w.near_h = take(R); w.far_h = take(R);
    w.hit = reinterpret_cast<int32_t*>(take(R)); w.counts = reinterpret_cast<int32_t*>(take(4));
    w.cws = reinterpret_cast<int32_t*>(take(nm_compact_workspace_ints(R)));
    w.ho = take(R * 3); w.hd = take(R * 3); w.hn = take(R); w.hf = take(R);
    w.bz = nullptr; w.braw = nullptr;                             // (the merge reads the background rows in place)
    w.h_raw = take(R * Sh * 4); w.h_z = take(R * Sh);
    w.human_ws = take(nm_render_rays_human_workspace_floats(R, Sh, 1));
    w.merge_ws = nullptr;
    w.rgb_h = take(R * 3); w.depth_h = take(R); w.acc_h = take(R); w.scratch = take(R * 6);
    w.total = o;
    return w;
}
}  // namespace

int64_t nm_render_rays_hybrid_workspace_floats(int64_t R, int S, int N, int S_human) { return hybrid_layout(nullptr, R, S, N, S_human).total; }

static int render_rays_hybrid(const LiveWs* lw, nm_mlp_t coarse, nm_mlp_t fine, nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* verts, int V,
                              double geo_threshold, const float* origin, const float* direction, int64_t R, float bkg_near, float bkg_far, int S, int N,
                              int S_human, const float* t_vals, const float* u, const float* t_vals_human, int white_bkg, int precision_coarse,
                              int precision_fine, int precision_human, float* workspace, float* rgb, float* depth, float* acc, nm_stream_t stream) {
    const char* who = lw ? "nm_render_rays_hybrid_live" : "nm_render_rays_hybrid";       // (one body, two entries: errors name the one that was called)
    NM_REQUIRE(R == 0 || (coarse && human && mesh && T && verts && origin && direction && t_vals && t_vals_human && workspace && rgb && depth && acc),
               "%s: null pointer", who);
    NM_REQUIRE(R >= 0 && S >= 1 && N >= 0 && S_human >= 2 && V >= 1, "%s: bad sizes", who);
    if (R == 0) return NM_OK;
    hipStream_t st = nm::as_stream(stream);
    const HybridWs w = hybrid_layout(workspace, R, S, N, S_human);
    const int Sb = S + N;
    int rc;
    union { float f; uint32_t u; } nb{bkg_near}, fb{bkg_far};
    if ((rc = nm::check_hip(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.near_b), (int)nb.u, (size_t)R, st), (std::string(who) + ": near").c_str()))) return rc;
    if ((rc = nm::check_hip(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.far_b), (int)fb.u, (size_t)R, st), (std::string(who) + ": far").c_str()))) return rc;
    // every ray: the background-only composite; acc is forced to 0 where the body is missed (:311)
    if ((rc = render_rays_bkg(lw, coarse, fine, origin, direction, w.near_b, w.far_b, R, S, N, t_vals, u, white_bkg, precision_coarse, precision_fine, w.bkg_ws,
                              w.raw_b, w.z_b, rgb, depth, acc, stream))) return rc;
    if ((rc = nm::check_hip(hipMemsetAsync(acc, 0, (size_t)R * 4, st), (std::string(who) + ": acc").c_str()))) return rc;
    if ((rc = nm_near_far(origin, direction, R, verts, V, geo_threshold, w.near_h, w.far_h, stream))) return rc;
    if ((rc = nm_compact_hits(w.near_h, w.far_h, R, w.hit, nullptr, w.counts, w.cws, stream))) return rc;
    int32_t n_hit = 0;
    if ((rc = nm::check_hip(hipMemcpyAsync(&n_hit, w.counts, 4, hipMemcpyDeviceToHost, st), (std::string(who) + ": hit count").c_str()))) return rc;
    if ((rc = nm::check_hip(hipStreamSynchronize(st), (std::string(who) + ": hit count").c_str()))) return rc;
    if (n_hit == 0) return NM_OK;
    // the hit rays: overwritten by the merged human + background composite (:313-353)
    if ((rc = nm_gather_rows(origin, w.hit, nullptr, n_hit, 3, w.ho, stream))) return rc;
    if ((rc = nm_gather_rows(direction, w.hit, nullptr, n_hit, 3, w.hd, stream))) return rc;
    if ((rc = nm_gather_rows(w.near_h, w.hit, nullptr, n_hit, 1, w.hn, stream))) return rc;
    if ((rc = nm_gather_rows(w.far_h, w.hit, nullptr, n_hit, 1, w.hf, stream))) return rc;
    if ((rc = render_rays_human(lw, human, mesh, T, w.ho, w.hd, w.hn, w.hf, n_hit, S_human, t_vals_human, white_bkg, 1.f, precision_human, w.human_ws, w.h_raw,
                                w.h_z, nullptr, nullptr, nullptr, stream))) return rc;
    {                                                                 // merged composite: the background lists of the hit rays read in place
        const float* zs[2] = {w.z_b, w.h_z};
        const float* raws[2] = {w.raw_b, w.h_raw};
        const int32_t* rows[2] = {w.hit, nullptr};
        const int Ss[2] = {Sb, S_human};
        if ((rc = nm_merge_composite_lists(2, zs, raws, rows, Ss, n_hit, w.hd, white_bkg, w.rgb_h, w.depth_h, w.acc_h, stream))) return rc;
    }
    if ((rc = nm_composite(w.h_raw, w.h_z, w.hd, n_hit, S_human, white_bkg, nullptr, w.scratch, w.scratch + 3 * (int64_t)n_hit, w.acc_h, nullptr,
                           w.scratch + 5 * (int64_t)n_hit, stream))) return rc;                     // the human-only accumulation (:345-350)
    if ((rc = nm_scatter_rows(w.rgb_h, w.hit, nullptr, n_hit, 3, rgb, stream))) return rc;
    if ((rc = nm_scatter_rows(w.depth_h, w.hit, nullptr, n_hit, 1, depth, stream))) return rc;
    return nm_scatter_rows(w.acc_h, w.hit, nullptr, n_hit, 1, acc, stream);
}

int nm_render_rays_hybrid(nm_mlp_t coarse, nm_mlp_t fine, nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* verts, int V,
                          double geo_threshold, const float* origin, const float* direction, int64_t R, float bkg_near, float bkg_far, int S, int N,
                          int S_human, const float* t_vals, const float* u, const float* t_vals_human, int white_bkg, int precision_coarse,
                          int precision_fine, int precision_human, float* workspace, float* rgb, float* depth, float* acc, nm_stream_t stream) {
    return render_rays_hybrid(nullptr, coarse, fine, human, mesh, T, verts, V, geo_threshold, origin, direction, R, bkg_near, bkg_far, S, N, S_human, t_vals, u,
                              t_vals_human, white_bkg, precision_coarse, precision_fine, precision_human, workspace, rgb, depth, acc, stream);
}

int nm_render_rays_hybrid_live(nm_mlp_t coarse, nm_mlp_t fine, nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* verts, int V,
                               double geo_threshold, const float* origin, const float* direction, int64_t R, float bkg_near, float bkg_far, int S, int N,
                               int S_human, const float* t_vals, const float* u, const float* t_vals_human, int white_bkg, int precision_coarse,
                               int precision_fine, int precision_human, float* workspace, float* rgb, float* depth, float* acc, void* live_ws,
                               int64_t live_ws_bytes, int64_t chunk_samples, nm_stream_t stream) {
    NM_REQUIRE(S >= 1 && N >= 0 && S_human >= 2, "nm_render_rays_hybrid_live: bad sizes");
    NM_LIVE_WS_REQUIRE("nm_render_rays_hybrid_live", fine ? precision_fine : precision_coarse, R * (int64_t)(S + N), S + N);      // the two composited passes
    NM_LIVE_WS_REQUIRE("nm_render_rays_hybrid_live", precision_human, R * (int64_t)S_human, S_human);                              // share live_ws
    const LiveWs lw{live_ws, live_ws_bytes, chunk_samples};
    return render_rays_hybrid(&lw, coarse, fine, human, mesh, T, verts, V, geo_threshold, origin, direction, R, bkg_near, bkg_far, S, N, S_human, t_vals, u,
                              t_vals_human, white_bkg, precision_coarse, precision_fine, precision_human, workspace, rgb, depth, acc, stream);
}

// ---- render_hybrid_nerf_multi_persons' per-batch body (utils/render_utils.py:390-456) for A actors as one call: two-pass background of every
// ray (:396-402), under the mixed precision policy the re-evaluation of every ray's LAST background sample (precision_last != 0: the sample
// whose interval ends on an actor's placeholder, host mirror render_multi_rays), then per actor near / far against its posed body,
// compaction of the hit rays (ONE host read per actor: their count -- the reference's boolean-mask indexing implies the same), the human
// pass of the hit rays into COMPACT [n_hit + 1, S_human] arrays whose last row is the zero-density placeholder at far_z (:405-419) and a
// row index for every ray, and ONE merge + composite kernel over the 1 + A lists (:441-456): nm_merge_composite_lists up to three actors,
// nm_merge_composite_lists_wide beyond.  Built from the entry points above (and two row kernels of its own): same kernels, same bits as
// calling them one by one.
namespace {
// dst[i * dst_stride + c] = src[i * src_stride + c], c < width: a column block of one row-major array into another
__global__ __launch_bounds__(256) void strided_rows_kernel(const float* __restrict__ src, int64_t src_stride, float* __restrict__ dst, int64_t dst_stride,
                                                           int width, int64_t n) {
    const int64_t total = n * width;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / width;
        const int c = (int)(t - i * width);
        dst[i * dst_stride + c] = src[i * src_stride + c];
    }
}

// rows[hit[i]] = i: the compact row of every hit ray (the others keep what the caller filled in: the placeholder row)
__global__ __launch_bounds__(256) void hit_rows_kernel(const int32_t* __restrict__ hit, int64_t n_hit, int32_t* __restrict__ rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_hit; i += (int64_t)gridDim.x * blockDim.x) rows[hit[i]] = (int32_t)i;
}

inline int rows_grid(int64_t items) {
    const int64_t b = (items + 255) / 256;
    return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}
int copy_strided_rows(const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int width, int64_t n, nm_stream_t stream) {
    if (n <= 0) return NM_OK;
    hipLaunchKernelGGL(strided_rows_kernel, dim3(rows_grid(n * width)), dim3(256), 0, nm::as_stream(stream), src, src_stride, dst, dst_stride, width, n);
    return nm::check_launch("strided_rows_kernel");
}
int fill_hit_rows(const int32_t* hit, int64_t n_hit, int32_t* rows, nm_stream_t stream) {
    if (n_hit <= 0) return NM_OK;
    hipLaunchKernelGGL(hit_rows_kernel, dim3(rows_grid(n_hit)), dim3(256), 0, nm::as_stream(stream), hit, n_hit, rows);
    return nm::check_launch("hit_rows_kernel");
}

struct MultiWs {
    float *near_b, *far_b, *bkg_ws, *raw_b, *z_b, *z_last, *raw_last, *near_h, *far_h, *ho, *hd, *hn, *hf, *human_ws, *acc, *actors;
    int32_t *hit, *counts, *cws;
    int64_t raw_a, z_a, rows_a, per_actor, total;                 // an actor's block at actors + a * per_actor: raw | z | rows
};
inline MultiWs multi_layout(float* base, int64_t R, int S, int N, int Sh, int A) {
    MultiWs w;
    int64_t o = 0;
    auto take = [&](int64_t n) { float* p = base ? base + o : nullptr; o += align4(n); return p; };
    const int Sb = S + N;
    w.near_b = take(R); w.far_b = take(R);
    w.bkg_ws = take(nm_render_rays_bkg_workspace_floats(R, S, N));
    w.raw_b = take(R * Sb * 4); w.z_b = take(R * Sb);
    w.z_last = take(R); w.raw_last = take(R * 4);
    w.near_h = take(R); w.far_h = take(R);
    w.hit = reinterpret_cast<int32_t*>(take(R)); w.counts = reinterpret_cast<int32_t*>(take(4));
    w.cws = reinterpret_cast<int32_t*>(take(nm_compact_workspace_ints(R)));
    w.ho = take(R * 3); w.hd = take(R * 3); w.hn = take(R); w.hf = take(R);
    w.human_ws = take(nm_render_rays_human_workspace_floats(R, Sh, 1));
    w.acc = take(R);
    w.raw_a = 0;                                                  // (every ray may hit every actor: n_hit + 1 <= R + 1 rows)
    w.z_a = w.raw_a + align4((R + 1) * Sh * 4);
    w.rows_a = w.z_a + align4((R + 1) * Sh);
    w.per_actor = w.rows_a + align4(R);
    w.actors = base ? base + o : nullptr;
    o += (int64_t)A * w.per_actor;
    w.total = o;
    return w;
}
}  // namespace

int64_t nm_render_rays_multi_workspace_floats(int64_t R, int S, int N, int S_human, int A) {
    return multi_layout(nullptr, R < 0 ? 0 : R, S, N, S_human, A < 0 ? 0 : A).total;
}

static int render_rays_multi(const LiveWs* lw, nm_mlp_t coarse, nm_mlp_t fine, int A, const nm_mlp_t* humans, const nm_mesh_t* meshes, const double* const* T,
                             const float* const* verts, const int* V, double geo_threshold, const float* origin, const float* direction, int64_t R,
                             float bkg_near, float bkg_far, int S, int N, int S_human, const float* t_vals, const float* u, const float* t_vals_human,
                             const float* far_z, int white_bkg, int precision_coarse, int precision_fine, int precision_last, int precision_human,
                             float* workspace, float* rgb, float* depth, nm_stream_t stream) {
    const char* who = lw ? "nm_render_rays_multi_live" : "nm_render_rays_multi";       // (one body, two entries: errors name the one that was called)
    NM_REQUIRE(R >= 0 && S >= 1 && N >= 0 && S_human >= 2 && A >= 0 && A < 32, "%s: bad sizes (S=%d N=%d S_human=%d actors=%d, at most 31)", who, S, N, S_human, A);
    NM_REQUIRE(R == 0 || (coarse && origin && direction && t_vals && workspace && rgb && depth), "%s: null pointer", who);
    NM_REQUIRE(A == 0 || (humans && meshes && T && verts && V), "%s: null actor arrays", who);
    NM_REQUIRE(R == 0 || A == 0 || (t_vals_human && far_z), "%s: null pointer", who);
    for (int a = 0; a < A; ++a) NM_REQUIRE(R == 0 || (humans[a] && meshes[a] && T[a] && verts[a] && V[a] >= 1), "%s: actor %d has a null pointer or no vertices", who, a);
    const int Sb = S + N;
    const int64_t St = (int64_t)Sb + (int64_t)A * S_human;
    if (A <= 3) NM_REQUIRE(St * 12 <= 64 * 1024, "%s: %lld merged samples exceed what nm_merge_composite_lists stages", who, (long long)St);
    else NM_REQUIRE(St <= nm::wide_merge_max_samples(), "%s: %lld merged samples, nm_merge_composite_lists_wide stages at most %d", who, (long long)St,
                    nm::wide_merge_max_samples());
    if (R == 0) return NM_OK;
    hipStream_t st = nm::as_stream(stream);
    const MultiWs w = multi_layout(workspace, R, S, N, S_human, A);
    int rc;
    union { float f; uint32_t u; } nb{bkg_near}, fb{bkg_far};
    if ((rc = nm::check_hip(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.near_b), (int)nb.u, (size_t)R, st), (std::string(who) + ": near").c_str()))) return rc;
    if ((rc = nm::check_hip(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.far_b), (int)fb.u, (size_t)R, st), (std::string(who) + ": far").c_str()))) return rc;
    if ((rc = render_rays_bkg(lw, coarse, fine, origin, direction, w.near_b, w.far_b, R, S, N, t_vals, u, white_bkg, precision_coarse, precision_fine, w.bkg_ws,
                              w.raw_b, w.z_b, nullptr, nullptr, nullptr, stream))) return rc;
    if (precision_last) {                                         // z[:, -1:] -> forward_rays -> raw[:, -1, :]
        if ((rc = copy_strided_rows(w.z_b + (Sb - 1), Sb, w.z_last, 1, 1, R, stream))) return rc;
        if ((rc = nm_mlp_forward_rays(fine ? fine : coarse, origin, direction, w.z_last, R, 1, precision_last, 1.f, w.raw_last, stream))) return rc;
        if ((rc = copy_strided_rows(w.raw_last, 4, w.raw_b + (int64_t)(Sb - 1) * 4, (int64_t)Sb * 4, 4, R, stream))) return rc;
    }
    const float* zs[32];
    const float* raws[32];
    const int32_t* rows[32];
    int Ss[32];
    zs[0] = w.z_b; raws[0] = w.raw_b; rows[0] = nullptr; Ss[0] = Sb;
    for (int a = 0; a < A; ++a) {
        float* h_raw = w.actors + a * w.per_actor + w.raw_a;
        float* h_z = w.actors + a * w.per_actor + w.z_a;
        int32_t* h_rows = reinterpret_cast<int32_t*>(w.actors + a * w.per_actor + w.rows_a);
        if ((rc = nm_near_far(origin, direction, R, verts[a], V[a], geo_threshold, w.near_h, w.far_h, stream))) return rc;
        if ((rc = nm_compact_hits(w.near_h, w.far_h, R, w.hit, nullptr, w.counts, w.cws, stream))) return rc;
        int32_t n_hit = 0;
        if ((rc = nm::check_hip(hipMemcpyAsync(&n_hit, w.counts, 4, hipMemcpyDeviceToHost, st), (std::string(who) + ": hit count").c_str()))) return rc;
        if ((rc = nm::check_hip(hipStreamSynchronize(st), (std::string(who) + ": hit count").c_str()))) return rc;
        NM_REQUIRE(n_hit >= 0 && n_hit <= R, "%s: actor %d: hit count %d of %lld rays", who, a, (int)n_hit, (long long)R);
        // the placeholder row behind the hit rays' rows, and every ray pointing at it until it is found among the hits
        if ((rc = nm::check_hip(hipMemcpyAsync(h_z + (int64_t)n_hit * S_human, far_z, (size_t)S_human * 4, hipMemcpyDeviceToDevice, st),
                                (std::string(who) + ": placeholder z").c_str()))) return rc;
        if ((rc = nm::check_hip(hipMemsetAsync(h_raw + (int64_t)n_hit * S_human * 4, 0, (size_t)S_human * 16, st), (std::string(who) + ": placeholder raw").c_str())))
            return rc;
        if ((rc = nm::check_hip(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h_rows), (int)n_hit, (size_t)R, st), (std::string(who) + ": rows").c_str()))) return rc;
        if (n_hit > 0) {
            if ((rc = nm_gather_rows(origin, w.hit, nullptr, n_hit, 3, w.ho, stream))) return rc;
            if ((rc = nm_gather_rows(direction, w.hit, nullptr, n_hit, 3, w.hd, stream))) return rc;
            if ((rc = nm_gather_rows(w.near_h, w.hit, nullptr, n_hit, 1, w.hn, stream))) return rc;
            if ((rc = nm_gather_rows(w.far_h, w.hit, nullptr, n_hit, 1, w.hf, stream))) return rc;
            if ((rc = render_rays_human(lw, humans[a], meshes[a], T[a], w.ho, w.hd, w.hn, w.hf, n_hit, S_human, t_vals_human, white_bkg, 1.f, precision_human,
                                        w.human_ws, h_raw, h_z, nullptr, nullptr, nullptr, stream))) return rc;
            if ((rc = fill_hit_rows(w.hit, n_hit, h_rows, stream))) return rc;
        }
        zs[1 + a] = h_z; raws[1 + a] = h_raw; rows[1 + a] = h_rows; Ss[1 + a] = S_human;
    }
    if (A <= 3) return nm_merge_composite_lists(1 + A, zs, raws, rows, Ss, R, direction, white_bkg, rgb, depth, w.acc, stream);
    return nm_merge_composite_lists_wide(1 + A, zs, raws, rows, Ss, R, direction, white_bkg, rgb, depth, w.acc, stream);
}

int nm_render_rays_multi(nm_mlp_t coarse, nm_mlp_t fine, int A, const nm_mlp_t* humans, const nm_mesh_t* meshes, const double* const* T,
                         const float* const* verts, const int* V, double geo_threshold, const float* origin, const float* direction, int64_t R,
                         float bkg_near, float bkg_far, int S, int N, int S_human, const float* t_vals, const float* u, const float* t_vals_human,
                         const float* far_z, int white_bkg, int precision_coarse, int precision_fine, int precision_last, int precision_human,
                         float* workspace, float* rgb, float* depth, nm_stream_t stream) {
    return render_rays_multi(nullptr, coarse, fine, A, humans, meshes, T, verts, V, geo_threshold, origin, direction, R, bkg_near, bkg_far, S, N, S_human, t_vals, u,
                             t_vals_human, far_z, white_bkg, precision_coarse, precision_fine, precision_last, precision_human, workspace, rgb, depth, stream);
}

int nm_render_rays_multi_live(nm_mlp_t coarse, nm_mlp_t fine, int A, const nm_mlp_t* humans, const nm_mesh_t* meshes, const double* const* T,
                              const float* const* verts, const int* V, double geo_threshold, const float* origin, const float* direction, int64_t R,
                              float bkg_near, float bkg_far, int S, int N, int S_human, const float* t_vals, const float* u, const float* t_vals_human,
                              const float* far_z, int white_bkg, int precision_coarse, int precision_fine, int precision_last, int precision_human,
                              float* workspace, float* rgb, float* depth, void* live_ws, int64_t live_ws_bytes, int64_t chunk_samples, nm_stream_t stream) {
    NM_REQUIRE(S >= 1 && N >= 0 && S_human >= 2, "nm_render_rays_multi_live: bad sizes");
    NM_LIVE_WS_REQUIRE("nm_render_rays_multi_live", fine ? precision_fine : precision_coarse, R * (int64_t)(S + N), S + N);      // the composited passes
    if (A > 0) { NM_LIVE_WS_REQUIRE("nm_render_rays_multi_live", precision_human, R * (int64_t)S_human, S_human); }              // share live_ws
    const LiveWs lw{live_ws, live_ws_bytes, chunk_samples};
    return render_rays_multi(&lw, coarse, fine, A, humans, meshes, T, verts, V, geo_threshold, origin, direction, R, bkg_near, bkg_far, S, N, S_human, t_vals, u,
                             t_vals_human, far_z, white_bkg, precision_coarse, precision_fine, precision_last, precision_human, workspace, rgb, depth, stream);
}

}  // extern "C"
