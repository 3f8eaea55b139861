/*
 * neuman_hip.h -- C ABI of libneuman_hip.so: the NeuMan ray-march hot path on MI355X (gfx950).
 *
 * The reference (apple/ml-neuman) has no FFI seam: its hot path is the Python function level of
 * utils/ray_utils.py, utils/render_utils.py and models/vanilla.py.  This header IS the seam a
 * maintainer binds underneath those functions (ctypes stub: INTEGRATION.md).  Each entry point names
 * the reference lines it replaces.
 *
 * Conventions
 *   - every function returns 0 (NM_OK) or a negative NM_ERR_* code; nm_last_error() returns a
 *     thread-local human readable message for the last failure on the calling thread;
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensor.data_ptr()) unless the
 *     parameter name starts with host_;  all tensors are dense, row-major, float32 / int32;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); kernels
 *     are enqueued on it and the call returns without synchronising;
 *   - no hidden allocation except inside the opaque nm_mlp_t handle; no global mutable state;
 *   - there is NO CPU fallback: without a HIP device the compute entry points fail with NM_ERR_HIP.
 */
#ifndef NEUMAN_HIP_H
#define NEUMAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NM_OK 0
#define NM_ERR_ARG (-1)         /* bad argument (null pointer, size, unsupported shape) */
#define NM_ERR_HIP (-2)         /* HIP runtime error (message carries hipGetErrorString) */
#define NM_ERR_UNSUPPORTED (-3) /* valid request this build does not implement */

#define NM_ABI_VERSION 1

typedef void* nm_stream_t;

/* precision of the MLP contraction (nm_mlp_forward*) */
#define NM_PREC_FP32 0   /* exact-f32 FMA chains on the vector ALU: slow validation path            */
#define NM_PREC_BF16X3 1 /* split-bf16 (hi+lo) x3 MFMA, f32 accumulate: the parity-grade default     */
#define NM_PREC_BF16 2   /* single bf16 MFMA, f32 accumulate: fast, NOT parity grade     */
#define NM_PREC_I8X3 3   /* hidden layers as per-row-scaled int16 = two int8 limbs on the i8 MFMA (hh + hl + lh, exact
                            int32 accumulate), encodings on split bf16: composited colours within 2e-5 of f32 on identical
                            samples -- parity grade for passes that are only composited (the host's default policy uses it
                            there), NOT for a pass whose weights place importance samples */
#define NM_PREC_FP16X3 4 /* split-fp16 (hi+lo, 11+11 significand bits) x3 MFMA, f32 accumulate, exact power-of-two operand
                            scalings: float32-class results (sigma within ~2e-6 of an f64 evaluation, as an f32 sgemm is)
                            at the bf16x3 price -- the arithmetic of a pass whose weights place importance samples      */

/* positional-encoding kinds (reference models/vanilla.py:44-79) */
#define NM_PE_POSENC 0 /* [x, sin(f0 x), cos(f0 x), sin(f1 x), ...]   vanilla.py:60-79,92 */
#define NM_PE_ROTATE 1 /* [x, sin(x B^T), cos(x B^T)]                 vanilla.py:44-58,83-89 */

int nm_version(void);
const char* nm_last_error(void);
/* number of visible HIP devices (0 when none): lets a host fail loudly before any compute call */
int nm_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * a4  ray_to_samples -- reference utils/ray_utils.py:96-135
 *   z = near*(1-t) + far*t  (or the lindisp form, :113-114); optional stratified jitter with a
 *   caller-drawn, already clipped t_rand[R,S] (:116-129); pts = o + d*z (:131); dirs = d repeated.
 *   t_vals[S] is the caller's torch.linspace(0,1,S) so both sides consume identical t.
 *   pts [R,S,3] and dirs [R,S,3] are optional (NULL = do not materialise).
 * ------------------------------------------------------------------------------------------- */
int nm_ray_to_samples(const float* origin, const float* direction, const float* near, const float* far,
                      int64_t R, int S, const float* t_vals, int lindisp, const float* t_rand,
                      float* pts, float* dirs, float* z_vals, nm_stream_t stream);

/* pts[i,s,:] = origin[i,:] + direction[i,:] * z[i,s]; dirs likewise (ray_utils.py:153-156). */
int nm_z_to_points(const float* origin, const float* direction, const float* z_vals, int64_t R, int S,
                   float* pts, float* dirs, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a5  raw2outputs -- reference utils/render_utils.py:69-105
 *   raw [R,S,4] = (r,g,b,sigma), z [R,S], rays_d [R,3]; noise [R,S] optional (the caller's
 *   torch.randn * raw_noise_std, :91-93).  Outputs: rgb [R,3], disp [R], acc [R], weights [R,S]
 *   (optional), depth [R].  One wavefront per ray, transmittance by a wave prefix product.
 * ------------------------------------------------------------------------------------------- */
int nm_composite(const float* raw, const float* z_vals, const float* rays_d, int64_t R, int S, int white_bkg,
                 const float* noise, float* rgb, float* disp, float* acc, float* weights, float* depth,
                 nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a6  sample_pdf (det=True) -- reference utils/ray_utils.py:164-194
 *   bins [R,B], weights [R,B-1], u [N] (caller's torch.linspace(0,1,N)) -> samples [R,N]
 * a7  ray_to_importance_samples -- reference utils/ray_utils.py:138-160
 *   z [R,S], weights [R,S] (as returned by raw2outputs) -> z_out [R,S+N] sorted (including_old)
 *   or [R,N] (not including_old).  Mid-points, weights[1:-1] slicing and the sort are fused.
 * ------------------------------------------------------------------------------------------- */
int nm_sample_pdf(const float* bins, const float* weights, int64_t R, int B, const float* u, int N,
                  float* samples, nm_stream_t stream);
int nm_importance_z(const float* z_vals, const float* weights, int64_t R, int S, const float* u, int N,
                    int including_old, float* z_out, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a2  geometry_guided_near_far -- reference utils/ray_utils.py:197-233
 *   near = min_v(z0 - dz), far = max_v(z0 + dz), dz = sqrt(tau^2 - (|v-o|^2 - z0^2)), NaN -> +-inf.
 * a3  hit-ray compaction -- reference utils/render_utils.py:199-212 (boolean-mask indexing)
 *   hit_idx receives the indices of rays with near < far in ascending order, miss_idx (optional)
 *   the others; counts[0] = n_hit, counts[1] = n_miss (device int32[2]).  Wave ballot + prefix sum.
 *   workspace: device int32, at least nm_compact_workspace_ints(R) entries.
 * ------------------------------------------------------------------------------------------- */
int nm_near_far(const float* origin, const float* direction, int64_t R, const float* verts, int V, double geo_threshold,
                float* near, float* far, nm_stream_t stream);
int64_t nm_compact_workspace_ints(int64_t R);
int nm_compact_hits(const float* near, const float* far, int64_t R, int32_t* hit_idx, int32_t* miss_idx,
                    int32_t* counts, int32_t* workspace, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a8/a9/a10  Joiner.forward = Embedder x2 + NeRF.forward -- reference models/vanilla.py:82-92,120-152,162-166
 *
 *   The net is the reference's default: depth 8, width 256, skip after layer 4, use_viewdirs
 *   (options/options.py:52-57), pos PE -> 63 features, dir PE -> 27 features.
 *   host_params: 24 HOST pointers to float32 arrays in the reference state_dict order
 *     nerf.pts_linears.{0..7}.{weight,bias}, nerf.views_linears.0.{weight,bias},
 *     nerf.feature_linear.{weight,bias}, nerf.alpha_linear.{weight,bias}, nerf.rgb_linear.{weight,bias}
 *   (weights are [out,in] row-major as torch.nn.Linear stores them).
 *   pe tables: posenc -> host_pos_tab[n_freqs] = the f32 frequency bands; rotate ->
 *   host_pos_tab[3*n_freqs*3] = Embedder.bvals ([3N,3] row-major).
 *   nm_mlp_create packs the weights into MFMA fragment order (split bf16 hi/lo) and uploads them;
 *   the handle owns that device memory.  A handle is immutable: rebuild it after the weights change.
 * ------------------------------------------------------------------------------------------- */
typedef struct nm_mlp_s* nm_mlp_t;

typedef struct nm_mlp_desc {
    int32_t depth;        /* 8 */
    int32_t width;        /* 256 */
    int32_t skip;         /* 4: cat([x_pe, h]) after pts_linears[4] */
    int32_t pe_kind;      /* NM_PE_POSENC / NM_PE_ROTATE, used for both inputs (vanilla.py:216,225) */
    int32_t pos_n_freqs;  /* 10 */
    int32_t dir_n_freqs;  /* 4 */
    int32_t plain_head;   /* 0: the use_viewdirs=True net (alpha / feature / views / rgb heads, vanilla.py:112-115, 133-144);
                             1: use_viewdirs=False (`--specular_can no`, models/human_nerf.py:28): one output_linear 256 -> 4 =
                             (r, g, b, sigma) on the eighth layer (vanilla.py:116-117, 145), view directions ignored.  host_params
                             then holds the 16 pts_linears tensors followed by output_linear.weight [4,256] and .bias [4] (the other
                             entries are not read).  NM_PREC_I8X3: the whole-network launch only (nerf_mlp_i8s_kernel<true>: output_linear's rows
                             in the alpha block, the tile ends there); no stage-by-stage or density-only i8 form. */
} nm_mlp_desc;

int64_t nm_mlp_pack_bytes(const nm_mlp_desc* desc);
/* host-only: write the packed weight image (what nm_mlp_create uploads) into host_out. */
int nm_mlp_pack(const nm_mlp_desc* desc, const float* const* host_params, void* host_out);
/* host-only: the NM_PREC_FP16X3 image -- same size and fragment layout, split fp16 of W * 2^8, biases * 2^13 (the exact
 * power-of-two scalings that keep both parts of every operand inside fp16's normal range; csrc/mlp.hip). */
int nm_mlp_pack_f16(const nm_mlp_desc* desc, const float* const* host_params, void* host_out);
/* host-only: the NM_PREC_I8X3 image by stage and block (limb fragments | pad | per-feature units | biases in those
 * units | one scalar per stage); nm_mlp_create uploads its fragments re-ordered into per-wave streams. */
int64_t nm_mlp_pack_i8_bytes(const nm_mlp_desc* desc);
int nm_mlp_pack_i8(const nm_mlp_desc* desc, const float* const* host_params, void* host_out);
/* host-only: the limb fragments of that image as the activation-stationary kernel streams them (what nm_mlp_create uploads for it):
 * k-steps of 2 KB in consumption order -- stage 0; stages 1-7, stage 5's four encoding steps per block behind its eight i8 blocks;
 * stage 8 with the alpha block first; stage 9; stage 10 -- followed by 8 KB of zeros (the ring copies whole 1 KB pieces: a 10-step block is rounded up). */
int64_t nm_mlp_pack_i8s_bytes(const nm_mlp_desc* desc);
int nm_mlp_pack_i8s(const nm_mlp_desc* desc, const float* const* host_params, void* host_out);
/* host-only: the two cuts of that stream that nm_mlp_forward_rays_live's launches walk (not the plain-head net).  Trunk: steps [0, 520) -- through the
 * alpha block -- then the next tile's first two ring blocks, 4 steps each padded with zeros to 8 (the ring looks two blocks ahead), then 8 KB of zeros.
 * Head: steps [520, 628), then 8 KB of zeros. */
int64_t nm_mlp_pack_i8s_trunk_bytes(const nm_mlp_desc* desc);
int64_t nm_mlp_pack_i8s_head_bytes(const nm_mlp_desc* desc);
int nm_mlp_pack_i8s_live(const nm_mlp_desc* desc, const float* const* host_params, void* host_trunk_out, void* host_head_out);
int nm_mlp_create(const nm_mlp_desc* desc, const float* const* host_params, const float* host_pos_tab,
                  const float* host_dir_tab, nm_mlp_t* out);
int nm_mlp_destroy(nm_mlp_t mlp);

/* out[i,:] = NeRF(PE(pts[i]), PE(dirs[i])) * (1,1,1,sigma_scale);  pts/dirs [n,3], out [n,4].
 * sigma_scale carries `out[..., -1] *= interval_comp` (render_utils.py:229); pass 1.0 otherwise. */
int nm_mlp_forward(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n, int precision,
                   float sigma_scale, float* out, nm_stream_t stream);
/* The forward of a TRAINING step (reference trainers/vanilla_nerf_trainer.py:66, 79: `self.coarse_net(pts, dirs)` with grad):
 * nm_mlp_forward in split-fp16 x3 (float32 class) that also keeps what the backward pass reads -- save_h [9][n][256] = the outputs of
 * pts_linears 0..7 after their ReLU, then feature_linear's (models/vanilla.py:125-138); save_hv [n][128] = views_linears[0]'s after its
 * ReLU (:140-142) -- written from the kernel's epilogues, so a tile's activations never return from HBM between layers.
 * nm_mlp_refresh_f16 rewrites the handle's split-fp16 weight image from DEVICE-resident parameters (24 device pointers, reference
 * state_dict order) in three small kernels: what nm_mlp_create packs on the host, bit for bit, for weights an optimiser changes every
 * iteration.  The plain-head net: 18 tensors (the trunk's 16, output_linear's weight [4][256] and bias [4]). */
int nm_mlp_refresh_f16(nm_mlp_t mlp, const float* const* dev_params, nm_stream_t stream);
int nm_mlp_forward_save(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n, float* save_h, float* save_hv,
                        float* out, nm_stream_t stream);
/* ... and, with save_bits [8][n][8] != NULL, one bit per trunk activation (> 0): word f >> 5 of (layer, sample) holds output f = 32 w + 8 q + 4 g + j
 * of pts_linears[layer] at bit 16 g + 15 - (4 q + j) (the producing kernel's register order) -- all the backward-data chain needs of them (1/32 of the bytes). */
int nm_mlp_forward_save_bits(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n, float* save_h, float* save_hv,
                             uint32_t* save_bits, float* out, nm_stream_t stream);
/* The backward-data chain of the trunk in a TRAINING step (autograd's adjoint of models/vanilla.py:126-134 inside
 * trainers/vanilla_nerf_trainer.py:45-96 / human_nerf_trainer.py:382-446 `loss.backward()`), one kernel with a 128-sample tile's dZ kept on
 * chip between the layers (split-bf16 x3 products, as nm_gemm_bf16x3):
 *     dZ_{i-1} = (dZ_i W_i[:, hidden columns]) * (H_{i-1} > 0),   bias gradient of layer i-1 = column sums of dZ_{i-1},   i = 7 .. 1.
 * Two forms: from dz_top [n][256] = dZ_7 (d_feat = d_raw = NULL): dz_out [7][n][256] = dZ_6 .. dZ_0, bias_grads [7][256];
 * or from d_feat [n][256] (gradient of feature_linear's output) and d_raw [n][4] (column 3: d sigma), the first stage forming
 *     dZ_7 = (d_feat W_feature + d sigma w_alpha) * (H_7 > 0)                                             (models/vanilla.py:133-134)
 * itself: dz_out [8][n][256] = dZ_7 .. dZ_0, bias_grads [8][256].  acts = nm_mlp_forward_save's save_h, relu_bits = nm_mlp_forward_save_bits'
 * save_bits (either may be NULL; the bits are read when given); dev_params = the 24 DEVICE pointers of nm_mlp_refresh_f16 (the weights are
 * repacked, transposed, from their live values in the call); workspace of nm_mlp_backward_chain_workspace_floats(n) floats.  The weight
 * gradients are the caller's products of dz_out with the saved activations (nm_gemm_*). */
int64_t nm_mlp_backward_chain_workspace_floats(int64_t n);
int nm_mlp_backward_chain(nm_mlp_t mlp, const float* const* dev_params, const float* dz_top, const float* d_feat, const float* d_raw,
                          const float* acts, const uint32_t* relu_bits, int64_t n, float* dz_out, float* bias_grads, float* workspace,
                          int64_t workspace_floats, nm_stream_t stream);
/* The 16-bit form of the two calls above (round 5): what a training step keeps between its forward and backward pass -- the reference's autograd
 * keeps every layer's float32 output (models/vanilla.py:126-141 under trainers/vanilla_nerf_trainer.py:45-96) -- is stored as fp16 wherever it is only
 * an operand of a weight-gradient product (a sum over all samples: the 2^-12 roundings of independent samples average out):
 *   nm_mlp_forward_save16: save_h16 [8][n][256] = fp16 of 32 x (output of pts_linears[l], after ReLU) -- the very hi part the next layer's MFMA reads --
 *     in K-SLOT ORDER: 16-byte chunk c, element e of a row holds feature 32 (c >> 2) + 8 (2 ((c >> 1) & 1) + (e >> 2)) + 4 (c & 1) + (e & 3)
 *     (mlp_layout.h slot_feature: the order the producing lanes hold them); feature_linear's output as save_feat [n][256] float32 and / or save_feat16
 *     [n][256] fp16 (x 32, k-slot order) (one of them required); save_hv [n][128] float32; save_bits [8][n][8] required; save_hvbits (nullable) [n][4]:
 *     the signs of the views layer's output, word f >> 5, bit order as save_bits; save_x0h / save_d0h (nullable) [n][64] fp16: the encoded position /
 *     direction exactly as the kernel holds them (32 x value, natural order, zero beyond the encoding; the direction's column 63 holds 1 -- what
 *     nm_pe_encode16 would give, without the extra launches).
 *   nm_mlp_backward_chain16: from d_feat / d_raw as nm_mlp_backward_chain's second form; dz16 [8][n][256] = fp16 of s x dZ_7 .. dZ_0 in k-slot order,
 *     dfeat16 (nullable) [n][256] = s x d_feat likewise, s = the power of two that puts *amax into [2, 4) (amax: a device scalar >= the largest magnitude
 *     entering the chain, nm_absmax; values beyond fp16's range saturate); dz32_layer5 / dz32_layer0 (nullable): float32 copies, natural order, of the
 *     two layers whose input-gradient products still want one; bias_grads [8][256] from the unrounded values.
 *   nm_mlp_backward_net16: the WHOLE backward-data pass of the net from d_raw [n][4] in one kernel -- autograd's adjoint of models/vanilla.py:133-145 too:
 *         d_hv = (d_rgb W_rgb) * (hv > 0)      d_feat = d_hv W_views[:, :256]      dZ_7 = (d_feat W_feature + d sigma w_alpha) * (H_7 > 0)  ...
 *     with the tile's d_hv and d_feat kept on chip.  amax >= max |d_raw| (the scale has 2^13 of headroom for growth through the layers).  Outputs as
 *     above plus dhv16 [n][128] (fp16 of s x d_hv, k-slot order of a 128-wide row: the views layer's weight-gradient operand), dhv32 (nullable) [n][128]
 *     float32 natural order (for the view-direction gradient); bias_grads [9][256]: rows 0..7 = layers 7..0, row 8 = feature_linear's.
 *     d_feat_add (nullable) [n][256] float32: a gradient that reaches feature_linear's output from elsewhere -- a second evaluation of the views head on the
 *     same features with other view directions (human_nerf_trainer.py:280-290 asks the net about the SAME points twice) -- added to the kernel's d_feat.
 *   Workspace of nm_mlp_backward_chain_workspace_floats(n) floats each.  The consumers: nm_wgrad16, nm_wgrad_alpha16 below (section "training"). */
int nm_mlp_forward_save16(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n, uint16_t* save_h16, float* save_feat, uint16_t* save_feat16,
                          float* save_hv, uint32_t* save_bits, uint32_t* save_hvbits, uint16_t* save_x0h, uint16_t* save_d0h, float* out,
                          nm_stream_t stream);
int nm_mlp_backward_chain16(nm_mlp_t mlp, const float* const* dev_params, const float* d_feat, const float* d_raw, const uint32_t* relu_bits,
                            int64_t n, const float* amax, uint16_t* dz16, uint16_t* dfeat16, float* dz32_layer5, float* dz32_layer0,
                            float* bias_grads, float* workspace, int64_t workspace_floats, nm_stream_t stream);
/* ... of the plain-head net (use_viewdirs=False: output_linear [4][256] straight off layer 7; nm_mlp_forward_save16 then keeps save_h16 / save_bits /
 * save_x0h only and dev_params are 18 tensors: the trunk's 16, output_linear's weight padded to [4][256] and bias [4]): dZ_7 = (d_out W_out) * (H_7 > 0)
 * from d_out [n][4], then the trunk; dz16 [8][n][256], bias_grads [8][256] = layers 7 .. 0.  What the offset nets of the human trainer run on
 * (models/vanilla.py:169-205, 3 outputs: a zero fourth row) once their constant time input is folded into the biases (neuman_hip/train.py). */
int nm_mlp_backward_plain16(nm_mlp_t mlp, const float* const* dev_params, const float* d_out, const uint32_t* relu_bits, int64_t n, const float* amax,
                            uint16_t* dz16, float* dz32_layer5, float* dz32_layer0, float* bias_grads, float* workspace, int64_t workspace_floats,
                            nm_stream_t stream);
int nm_mlp_backward_net16(nm_mlp_t mlp, const float* const* dev_params, const float* d_raw, const float* d_feat_add, const uint32_t* relu_bits,
                          const uint32_t* hv_bits, int64_t n, const float* amax, uint16_t* dz16, uint16_t* dfeat16, uint16_t* dhv16, float* dz32_layer5, float* dz32_layer0,
                          float* dhv32, float* bias_grads, float* workspace, int64_t workspace_floats, nm_stream_t stream);
/* Same with ray_to_samples' point construction fused: sample (r,s) is at origin[r] + direction[r]*z[r,s]
 * with view direction direction[r] (ray_utils.py:131-132); out [R,S,4]. */
int nm_mlp_forward_rays(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals,
                        int64_t R, int S, int precision, float sigma_scale, float* out, nm_stream_t stream);
/* nm_mlp_forward_rays for a pass whose output is composited and nothing else (raw2outputs: alpha = 1 - exp(-relu(sigma) dist)): a sample whose
 * stored density sigma * sigma_scale is <= 0 has weight exactly 0, so its colour is never seen -- it is returned as (0, 0, 0) and the colour head
 * (feature_linear, views_linears, rgb_linear: 17 % of the MACs) is evaluated on the other samples only.  Their records, and every density, are
 * BIT-IDENTICAL to nm_mlp_forward_rays'; all records are finite.  NM_PREC_I8X3 with the view-dependent head; any other precision, the plain-head
 * net and NEUMAN_I8_KERNEL=w run nm_mlp_forward_rays itself.  The rays are walked in chunks of chunk_samples samples (whole rays; <= 0:
 * NM_LIVE_CHUNK_SAMPLES); per chunk a counter reset, a trunk launch that lists the live samples with their activations (520 B each) in
 * `workspace`, and a head launch sized on the device from that list -- no host synchronisation.  workspace (16-byte aligned):
 * nm_mlp_forward_rays_live_workspace_bytes(R, S, chunk_samples) bytes = one chunk with every sample live.  Where that workspace is large enough the
 * whole call is ONE launch instead (nm_mlp_forward_rays_fused below: same records, no chunks). */
#define NM_LIVE_CHUNK_SAMPLES (1 << 21)
int64_t nm_mlp_forward_rays_live_workspace_bytes(int64_t R, int S, int64_t chunk_samples);
int nm_mlp_forward_rays_live(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int64_t R, int S, int precision,
                             float sigma_scale, float* out, void* workspace, int64_t workspace_bytes, int64_t chunk_samples, nm_stream_t stream);
/* The pair as ONE persistent launch (csrc/mlp_i8f.hip): every workgroup lists the live samples of its own trunk tiles in a ring of 768 entries of its
 * own and runs colour-head tiles on them between its trunk tiles -- no chunks, no global counter, no reset; every record bit-identical to the pair's.
 * nm_mlp_forward_rays_live takes it for a call with R * S < 2^31 whose workspace (sized as above) also holds
 * nm_mlp_live_fused_workspace_bytes(R * S) bytes = min(ceil(n / 256), 256) lists of 768 * 520 B and two int32 per list (rounded up to 256 B), which is
 * every call of frame size; NEUMAN_LIVE_FUSED=0 keeps the pair for every call, =1 takes the fused launch, unset: NM_LIVE_FUSED_DEFAULT.
 * nm_mlp_forward_rays_fused runs the fused launch itself, on a workspace of at least that size, whatever the switch says (an error for the plain-head
 * net and under NEUMAN_I8_KERNEL=w: there is no such kernel).  After the call the workspace's last block holds, per workgroup, the trunk tiles and the
 * head tiles it ran (int32 [groups][2] at byte groups * 768 * 520, groups = min(ceil(n / 256), 256); the launch takes min(groups, CUs) workgroups). */
#define NM_LIVE_FUSED_DEFAULT 1
int64_t nm_mlp_live_fused_workspace_bytes(int64_t n);
int nm_mlp_forward_rays_fused(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int64_t R, int S, float sigma_scale,
                              float* out, void* workspace, int64_t workspace_bytes, nm_stream_t stream);
/* Density only, for a pass whose colours the caller discards -- the coarse pass of a two-pass render: the reference
 * composites it (render_utils.py:139) and keeps nothing but the weights that place the importance samples (:141), which
 * depend on sigma alone.  Same arguments as nm_mlp_forward_rays; out [R,S,4] receives (0, 0, 0, sigma * sigma_scale) with
 * sigma BIT-IDENTICAL to nm_mlp_forward_rays' (same instruction sequence for the alpha row); feature_linear,
 * views_linears and rgb_linear -- 17 % of the MACs -- are not evaluated.  NM_PREC_BF16X3 / NM_PREC_BF16; the other
 * precisions evaluate everything and return the colours too. */
int nm_mlp_sigma_rays(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals,
                      int64_t R, int S, int precision, float sigma_scale, float* out, nm_stream_t stream);
/* Front-to-back marching with early ray termination (the north star's "wavefront ballot / prefix-sum for early termination
 * and sample compaction ... MLP over the compacted (rays x samples) batch"; the reference evaluates every sample,
 * utils/render_utils.py:139-151).  One chunk of the pass: samples s0 .. s0+S-1 of the rays listed in ray_idx [n_rays]
 * (int32, compacted list of live rays; when n_rays_dev is non-null the list's length is read from the device and n_rays
 * is only its upper bound, so no host synchronisation separates the chunks).  origin / direction [R,3], z_vals
 * [R,S_total], out [R,S_total,4]: only the listed rays' records of this chunk are written (pre-zeroed records of samples
 * never evaluated composite with weight exactly 0).  NM_PREC_FP32 is not available in this form. */
int nm_mlp_forward_ray_chunk(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int S_total,
                             const int32_t* ray_idx, const int32_t* n_rays_dev, int64_t n_rays, int s0, int S, int precision,
                             float sigma_scale, float* out, nm_stream_t stream);
/* The same chunk, density only (nm_mlp_sigma_rays' arithmetic: sigma bit-identical, colours 0) -- the march of a COARSE pass, whose
 * colours the reference composites and discards (render_utils.py:139-141). */
int nm_mlp_sigma_ray_chunk(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int S_total,
                           const int32_t* ray_idx, const int32_t* n_rays_dev, int64_t n_rays, int s0, int S, int precision,
                           float sigma_scale, float* out, nm_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * K11  occupancy-grid empty-space skipping for the background passes -- reference utils/render_utils.py:131-151, 287-297 (which
 * evaluate every sample).  A skipped sample keeps raw = 0: alpha = 0 and weight 0 in raw2outputs, exactly what a sample with
 * relu(sigma) = 0 gets.  Grid: res^3 bits (res 4..256, a multiple of 4) over the box aabb = host float[6] (lo x y z, hi x y z);
 * cell (i, j, k) along (x, y, z) is bit c = (k res + j) res + i of word c >> 5.  Every buffer is the caller's.
 *
 * nm_occ_probe_offset: offset in [0, 1) along `axis` of probe k inside every cell (a sub-cell lattice of m^3 >= probes slots with a
 *   seeded jitter); the probe of cell (i, j, k) is lo + (float(i) + offset) * ((hi - lo) / res) per axis, in float32.
 * nm_occ_build: cell value = max sigma of the net (density-only launch, `precision`) over its probes; a cell is occupied when a cell
 *   within `dilate` of it per axis has a value > sigma_threshold (>= 0).  workspace: nm_occ_build_workspace_floats(res, probes)
 *   floats (16-byte aligned); bits: res^3 / 32 words.
 * nm_occ_compact_samples: sample_idx [R*S] receives the ascending flat indices r*S + s of the samples of rays origin + direction *
 *   z_vals [R,S] (the point built as the MLP launches build it) whose cell is occupied or that lie outside the box; counts[0] =
 *   their number, counts[1] = the skipped (device int32[2]).  workspace: nm_occ_compact_workspace_ints(R*S) int32.
 * nm_occ_compact_ray_chunk: nm_occ_compact_samples for one chunk of a front-to-back march (nm_mlp_forward_ray_chunk's arguments): the
 *   live rays are n = n_rays_dev ? clamp(*n_rays_dev, 0, n_rays) : n_rays, read on the device (n_rays only sizes the launch); candidate
 *   j in [0, n*S) is sample s = s0 + j % S of ray r = ray_idx ? ray_idx[j / S] : j / S (entries of ray_idx at or past n are never read;
 *   without ray_idx n_rays <= R).  sample_idx [n_rays*S] receives the flat indices r * S_total + s of the candidates whose cell is
 *   occupied or that lie outside the box -- the same test on the same point, so the same decision as nm_occ_compact_samples' -- in
 *   candidate order (ascending when ray_idx is); counts = (kept, n*S - kept).  What nm_mlp_forward_samples, nm_mlp_sigma_samples and
 *   nm_mlp_forward_samples_live take.  0 <= s0, 1 <= S, s0 + S <= S_total; R * S_total and n_rays * S below 2^31; n_rays == 0 writes
 *   counts = (0, 0).  workspace: nm_occ_compact_workspace_ints(n_rays * S) int32.  No host synchronisation, no allocation.
 * nm_mlp_forward_samples / nm_mlp_sigma_samples: nm_mlp_forward_rays / nm_mlp_sigma_rays on the listed samples only (in_mode 3):
 *   the first *n_dev entries of sample_idx (n_dev nullable: n_max entries; n_max = the list's upper bound) are evaluated and written
 *   into out[r, s] [R,S,4]; nothing else of out is touched.  Bit-identical to the matching records of the every-sample launch.
 *   NM_PREC_FP32 is not available in this form.
 * ------------------------------------------------------------------------------------------- */
float nm_occ_probe_offset(int probes, int seed, int k, int axis);
int64_t nm_occ_build_workspace_floats(int res, int probes);
int nm_occ_build(nm_mlp_t mlp, const float* aabb, int res, int probes, int dilate, float sigma_threshold, int seed, int precision,
                 float* workspace, int64_t workspace_floats, uint32_t* bits, nm_stream_t stream);
int64_t nm_occ_compact_workspace_ints(int64_t n_samples);
int nm_occ_compact_samples(const uint32_t* bits, int res, const float* aabb, const float* origin, const float* direction, const float* z_vals,
                           int64_t R, int S, int32_t* sample_idx, int32_t* counts, int32_t* workspace, nm_stream_t stream);
int nm_occ_compact_ray_chunk(const uint32_t* bits, int res, const float* aabb, const float* origin, const float* direction, const float* z_vals,
                             int64_t R, int S_total, const int32_t* ray_idx, const int32_t* n_rays_dev, int64_t n_rays, int s0, int S,
                             int32_t* sample_idx, int32_t* counts, int32_t* workspace, nm_stream_t stream);
int nm_mlp_forward_samples(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int64_t R, int S,
                           const int32_t* sample_idx, const int32_t* n_dev, int64_t n_max, int precision, float sigma_scale, float* out,
                           nm_stream_t stream);
int nm_mlp_sigma_samples(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int64_t R, int S,
                         const int32_t* sample_idx, const int32_t* n_dev, int64_t n_max, int precision, float sigma_scale, float* out,
                         nm_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * K11b  occupancy-grid empty-space skipping for the human passes -- reference utils/render_utils.py:213-229, 320-329 (every sample).
 * Same grid, box and skipped-sample convention as K11 above; a human net's grid lives in CANONICAL space.
 *
 * nm_occ_compact_points: point_idx [n] receives the ascending indices k of the points pts [n,3] whose cell is occupied or that lie
 *   outside the box; counts[0] = their number, counts[1] = the skipped (device int32[2]).  The cell test and the scan of
 *   nm_occ_compact_samples.  workspace: nm_occ_compact_workspace_ints(n) int32.
 * nm_mlp_forward_listed: nm_mlp_forward on the listed points only (in_mode 4): launch entry i evaluates point k = point_idx[i] (pts[k],
 *   dirs[k]) and writes out[k] [n_points,4]; the first *n_dev entries (n_dev nullable: n_max) are evaluated, nothing else of out is
 *   touched.  Bit-identical to the matching rows of nm_mlp_forward.  NM_PREC_FP32 is not available in this form.
 * nm_render_rays_human_occ: nm_render_rays_human with the grid (bits, res, aabb).  raw_out [R,S,4] is zeroed, then: mesh == NULL
 *   (canonical render) -> nm_occ_compact_samples on o + d z and nm_mlp_forward_samples; else sample -> nm_warp_to_canonical ->
 *   nm_occ_compact_points on the canonical points -> nm_mlp_forward_listed.  counts (device int32[2]) = (evaluated, skipped)
 *   samples.  workspace: nm_render_rays_human_occ_workspace_floats(R, S, posed) floats; it begins with nm_render_rays_human's layout.
 *   No host synchronisation, no allocation.  (Declared with the fused passes below.)
 * ------------------------------------------------------------------------------------------- */
int nm_occ_compact_points(const uint32_t* bits, int res, const float* aabb, const float* pts, int64_t n, int32_t* point_idx, int32_t* counts,
                          int32_t* workspace, nm_stream_t stream);
int nm_mlp_forward_listed(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n_points, const int32_t* point_idx, const int32_t* n_dev,
                          int64_t n_max, int precision, float sigma_scale, float* out, nm_stream_t stream);
/* The colour head on live samples only (nm_mlp_forward_rays_live above) for the other input forms -- for a caller whose records are composited and
 * nothing else: raw2outputs (utils/render_utils.py:85-95), alone or behind a sorted merge (:330-345, 441-456), reads a colour only as
 * weight * sigmoid(colour), and the weight of an interval, a merged one included, is exactly 0 when the stored density is <= 0.
 *   nm_mlp_forward_live            = nm_mlp_forward            (points and their own directions;         models/vanilla.py:162-166)
 *   nm_mlp_forward_listed_live     = nm_mlp_forward_listed     (the listed points, each with dirs[k];    utils/render_utils.py:213-229)
 *   nm_mlp_forward_samples_live    = nm_mlp_forward_samples    (the listed samples of rays;              utils/render_utils.py:139-151)
 *   nm_mlp_forward_ray_chunk_live  = nm_mlp_forward_ray_chunk  (samples s0 .. s0+S-1 of the listed rays; utils/render_utils.py:139-151)
 * Each takes its sibling's arguments, then workspace, workspace_bytes, chunk_samples before stream, and writes what the sibling writes except that
 * the colour of a listed record whose stored density sigma * sigma_scale is <= 0 is (0, 0, 0): every density and every other listed record is
 * BIT-IDENTICAL to the sibling's, every written value is finite, records that are not listed are not touched.  NM_PREC_I8X3 with the
 * view-dependent head; any other precision, the plain-head net and NEUMAN_I8_KERNEL=w run the sibling itself.  The input is walked in pieces of
 * at most chunk_samples entries (<= 0: NM_LIVE_CHUNK_SAMPLES; for nm_mlp_forward_ray_chunk_live a piece is a whole number of listed rays, so
 * chunk_samples must be at least S): per piece a counter reset, a trunk launch and a head launch.  Where the list's length lives on the device
 * (n_dev, n_rays_dev), piece p covers clamp(*n_dev - p * piece, 0, piece) entries: one small kernel computes these into the workspace before the
 * first trunk launch, and an empty piece launches over a count of 0.  No host synchronisation, no allocation.  out and workspace must be
 * 16-byte aligned; with NM_PREC_I8X3 the workspace holds nm_mlp_live_workspace_bytes(n_max, chunk_samples) bytes (n_max = n, n_max, or
 * n_rays * S) whichever net is behind the handle: one piece with every entry live, 520 B per entry with the piece = min(n_max, chunk_samples)
 * rounded up to 256, plus the counters.  These argument errors are reported before the handle is looked at and before anything is enqueued.
 * out of nm_mlp_forward_ray_chunk_live holds fewer than 2^31 records (the list carries a record as int32). */
int64_t nm_mlp_live_workspace_bytes(int64_t n_max, int64_t chunk_samples);
int nm_mlp_forward_live(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n, int precision, float sigma_scale, float* out, void* workspace,
                        int64_t workspace_bytes, int64_t chunk_samples, nm_stream_t stream);
int nm_mlp_forward_listed_live(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n_points, const int32_t* point_idx, const int32_t* n_dev,
                               int64_t n_max, int precision, float sigma_scale, float* out, void* workspace, int64_t workspace_bytes,
                               int64_t chunk_samples, nm_stream_t stream);
int nm_mlp_forward_samples_live(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int64_t R, int S,
                                const int32_t* sample_idx, const int32_t* n_dev, int64_t n_max, int precision, float sigma_scale, float* out,
                                void* workspace, int64_t workspace_bytes, int64_t chunk_samples, nm_stream_t stream);
int nm_mlp_forward_ray_chunk_live(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int S_total,
                                  const int32_t* ray_idx, const int32_t* n_rays_dev, int64_t n_rays, int s0, int S, int precision,
                                  float sigma_scale, float* out, void* workspace, int64_t workspace_bytes, int64_t chunk_samples,
                                  nm_stream_t stream);
/* T[r] *= prod_{i in chunk} (1 - alpha_i + 1e-10) for the listed rays (ray_idx nullable = rays 0..n_rays-1): the
 * transmittance factors of raw2outputs (render_utils.py:85-95) over samples s0 .. s0+S-1 of raw [R,S_total,4]; rays whose T
 * falls below the caller's epsilon are dropped by nm_compact_hits(eps, T). */
int nm_transmittance_chunk(const float* raw, const float* z_vals, const float* rays_d, const int32_t* ray_idx, const int32_t* n_rays_dev,
                           int64_t n_rays, int s0, int S, int S_total, float* T, nm_stream_t stream);
/* The same with the samples' z INTERVALS given (dz [R,S_total], before the multiplication by |rays_d|): a list that will be merged
 * with other lists before it is composited (render_utils.py:330-345, 441-456) -- the interval behind a sample then ends at its
 * successor in the merged order, and the transmittance the early-termination cut is decided on is the merged list's. */
int nm_transmittance_chunk_dz(const float* raw, const float* dz, const float* rays_d, const int32_t* ray_idx, const int32_t* n_rays_dev,
                              int64_t n_rays, int s0, int S, int S_total, float* T, nm_stream_t stream);
/* One marched pass of one net as ONE call (the reference evaluates every sample: utils/render_utils.py:139-151, 294-297): the chunks above,
 * front to back in uniform chunks of `chunk` samples (the last may be shorter), and between two chunks -- on the device, over the rays of the
 * live list only, in three launches (transmittance + count, single-block scan, write) -- what a host loop does with nm_transmittance_chunk*
 * and nm_compact_hits:
 *   1. T[r] *= prod (1 - alpha_i + 1e-10) over the chunk (render_utils.py:85-95), nm_transmittance_chunk's arithmetic bit for bit; with
 *      dz [R,S_total] nm_transmittance_chunk_dz's (the samples' intervals in a merged list, :330-345);
 *   2. with an occluder, T_eff = T[r] * (z_vals[r, s_next] >= occ_z_far[r] ? occ_T[r] : 1), one float32 multiply (s_next: the next chunk's
 *      first sample): the list will be merged with one that lies in front of occ_z_far and lets occ_T through (:330-345, 441-456);
 *   3. the ray stays iff eps < T_eff (a NaN drops it); the next list is ascending.
 * eps <= 0: no boundary runs and every sample is evaluated (the records of nm_mlp_forward_rays / nm_mlp_sigma_rays); none runs after the last
 * chunk.  raw_out [R,S_total,4] is zeroed here first: a sample never evaluated keeps raw = 0, weight exactly 0 in nm_composite.  sigma_only:
 * nm_mlp_sigma_ray_chunk instead of nm_mlp_forward_ray_chunk.  stats (nullable, device int64[2]) receives (samples the network ran on, 0).
 * workspace: workspace_floats >= nm_march_pass_workspace_floats(R) floats, 16-byte aligned like raw_out.  NM_PREC_FP32 has no chunked form.
 * No host synchronisation, no allocation, no copy to the host; argument errors are reported before anything is enqueued. */
int64_t nm_march_pass_workspace_floats(int64_t R);
int nm_march_pass(nm_mlp_t mlp, const float* origin, const float* direction, const float* z_vals, int64_t R, int S_total, int chunk, float eps,
                  int sigma_only, int precision, float sigma_scale, const float* dz, const float* occ_z_far, const float* occ_T, float* workspace,
                  int64_t workspace_floats, float* raw_out, int64_t* stats, nm_stream_t stream);
/* Debug: the density-only NM_PREC_FP16X3 activation-stationary kernel (csrc/mlp_f16t.hip) on n points (out [n,4] = (0, 0, 0, sigma)), plus the
 * activations of its first tile after `stage` (0..7): state [128 samples][256] float32 in natural feature order (hi + lo parts, unscaled). */
int nm_mlp_sigma_f16t_debug(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n, int stage, float* state, float* out, nm_stream_t stream);
/* Debug: stop after `stage` and write that stage's activations as f32 [n, width_of_stage]:
 *   -1 -> position PE (64 wide, col 63 = 0);  0..7 -> relu(pts_linears[i]) (256);
 *    8 -> feature_linear output (256);  9 -> relu(views_linears[0]) (128). */
int nm_mlp_forward_debug(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n, int precision,
                         int stage, float* hidden, nm_stream_t stream);
/* Profiling build of the NM_PREC_BF16X3 or NM_PREC_I8X3 kernel: same result in `out`, plus per-wave s_memtime
 * totals in cycles[(workgroup*8 + wave)*8 + bucket]; cycles must hold 64 * min(#CUs, ceil(n/128)) uint64.
 *   bf16x3 buckets: {0 PE, 1 k-loops, 2 wait before epilogue, 3 epilogue, 4 wait after epilogue, 5 tile tail}
 *   i8x3 buckets:   {0 PE fill, 1 k-loops, 2 end barrier of an M slot, 3 epilogue part 1, 4 its middle barrier,
 *                    5 epilogue part 2, 6 end barrier of an E slot, 7 rest}  (csrc/mlp.hip) */
int nm_mlp_forward_profile(nm_mlp_t mlp, const float* pts, const float* dirs, int64_t n, int precision, float* out,
                           uint64_t* cycles, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a11  warp_samples_to_canonical -- reference utils/ray_utils.py:48-66
 *   closest point on the posed mesh (replaces igl.point_mesh_squared_distance, :53), barycentrics
 *   (:55), blended per-vertex transform T (f64, [>=V,4,4]), 4x4 inverse, canonical point, and
 *   finite-difference canonical directions along each ray (:62-64).
 *
 *   nm_mesh_create builds, once per posed mesh (per frame and actor), an exact search structure on the
 *   device: triangle records in Morton order and an implicit 4-ary tree of child boxes over them
 *   (NM_SEARCH_TREE).  verts [V,3] f32 and faces [F,3] int32 are DEVICE pointers and are copied into the
 *   handle; F <= 2^24.  NM_SEARCH_ALL makes the query loop over every triangle instead (diagnostics and
 *   tests: both modes return bit-identical results, ties between equidistant triangles going to the lowest
 *   face id).  The call synchronises the stream once (non-finite vertices are an error).
 *   nm_mesh_update: the SAME topology with moved vertices (verts [V,3], device) -- what a training iteration has (the posed SMPL mesh of
 *   human_nerf_trainer.py:262-271 after every optimiser step): the tree, and on the next nm_signed_distance the normals, are rebuilt into the handle's
 *   buffers; no allocation, no read-back, no synchronisation (a non-finite vertex is NOT reported here: the queries then fall back to the
 *   all-triangles loop point by point).
 *   nm_warp_to_canonical: pts [R,S,3] f32, T [*,16] f64 -> can_pts, can_dirs [R,S,3] f32,
 *   closest [R,S,3] f32 (optional).
 * ------------------------------------------------------------------------------------------- */
#define NM_SEARCH_TREE 0
#define NM_SEARCH_ALL 1
#define NM_SEARCH_TREE_WIDE 2 /* the tree search with the stack layout of meshes beyond 65,536 nodes (tests) */
typedef struct nm_mesh_s* nm_mesh_t;
int nm_mesh_create(const float* verts, int V, const int32_t* faces, int F, int search, nm_mesh_t* out,
                   nm_stream_t stream);
int nm_mesh_update(nm_mesh_t mesh, const float* verts, nm_stream_t stream);
int nm_mesh_destroy(nm_mesh_t mesh);
/* tree levels, node count and device bytes of a built mesh (diagnostics) */
int nm_mesh_info(nm_mesh_t mesh, int32_t* levels, int64_t* nodes, int64_t* bytes);
int nm_warp_to_canonical(nm_mesh_t mesh, const float* pts, int64_t R, int S, const double* T, float* can_pts,
                         float* can_dirs, float* closest, nm_stream_t stream);
/* igl.signed_distance(P, V, F) -- reference utils/ray_utils.py:70, trainers/human_nerf_trainer.py:310, 326: for pts [N,3]
 * the distance to the mesh signed by the angle-weighted pseudonormal of the closest feature (negative inside a closed,
 * outward-oriented mesh), the closest face (the caller's id; lowest id on ties) and the closest point.  The pseudonormal
 * table is built by the first call on a mesh (synchronises once). */
int nm_signed_distance(nm_mesh_t mesh, const float* pts, int64_t N, float* sdist, int32_t* face, float* closest,
                       nm_stream_t stream);

/* The differentiable warp of the human trainer (utils/ray_utils.py:85-93 + trainers/human_nerf_trainer.py:262-266), per sample i of N:
 *   can[i] = inv( sum_k bary[i][k] T[tri[i][k]] ) [pts[i]; 1]     T [V,4,4] f32, tri [N,3] int32 vertex ids, bary / pts / can [N,3] f32
 * forward and backward as one kernel each.  backward: g_can [N,3] -> g_T [V,4,4] (cleared here, then float atomics: the summation
 * order over a vertex's samples is not fixed) and g_bary [N,3]; the points carry no gradient (the trainer detaches them). */
int nm_warp_apply_forward(const float* T, const int32_t* tri, const float* bary, const float* pts, int64_t N, float* can, nm_stream_t stream);
int nm_warp_apply_backward(const float* T, const int32_t* tri, const float* bary, const float* pts, const float* g_can, int64_t N, int64_t V,
                           float* g_T, float* g_bary, nm_stream_t stream);
/* The barycentric coordinates the warp blends with (utils/ray_utils.py:72-84), per sample i of N, of the closest point closest[i] (a constant:
 * the reference gets it from igl as numpy) in the triangle tri[i] of verts [V,3]:  bary [N,3] = (u, v, 1 - u - v), the reference's float32
 * cross / dot / divide sequence -- and their adjoint, g_bary [N,3] -> g_verts [V,3] (cleared here, then float atomics), which is what carries
 * the loss to the SMPL parameters through the posed vertices (trainers/human_nerf_trainer.py:241-278). */
int nm_bary_forward(const float* verts, const int32_t* tri, const float* closest, int64_t N, float* bary, nm_stream_t stream);
int nm_bary_backward(const float* verts, const int32_t* tri, const float* closest, const float* g_bary, int64_t N, int64_t V, float* g_verts,
                     nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a12  SMPL linear blend skinning, batched over frames -- reference models/smpl.py:266-360 (lbs),
 *   :407-438 (batch_rodrigues), :454-505 (batch_rigid_transform), :109-216 (SMPL.verts_transformations /
 *   forward); callers data_io/neuman_helper.py:288-330 (read_smpls) and models/human_nerf.py:92-122
 *   (HumanNeRF.vertex_forward).
 *
 *   nm_smpl_create copies the model to the device.  HOST pointers, float32 as the reference registers them
 *   (smpl.py:74-107): v_template [V,3], shapedirs [V,3,NB], j_regressor [J,V], parents [J] (parents[0]
 *   ignored, parents[j] < j), lbs_weights [V,J], da_pose [J*3] (the canonical pose: neuman_helper.py:294-299).
 *   J <= 64, 1 <= NB <= 32 (a model without shape directions is refused: every entry takes a betas array).
 *   nm_smpl_frames, per frame b of B (DEVICE pointers): poses [B,J*3] f32, betas [B,NB] f32,
 *   alignments [B,4,4] f64 = the matrix whose TRANSPOSE the reference applies (read_smpls' temp_alignment,
 *   vertex_forward's alignments[idx]).  Rows 0..V-1 are vertices, rows V..V+J-1 the joints
 *   (concat_joints=True):
 *     T_out      [B,V+J,4,4] f64  T_da2scene = S(scale) align^T T_t2pose inv(T_t2da)
 *     world_out  [B,V+J,3]   f32  T_da2scene [da-pose point; 1]   (world_verts | joints_3d)
 *     static_out [B,V+J,3]   f32  the da-pose points              (static_vert | static_joints_3d)
 *   precise = 1: read_smpls' arithmetic (float32 up to T_da2pose, float64 after); precise = 0:
 *   vertex_forward's (float32 throughout; T_out then holds float32 values).
 *   The first call with a larger B than any before allocates workspace (synchronises).
 * ------------------------------------------------------------------------------------------- */
typedef struct nm_smpl_s* nm_smpl_t;
int nm_smpl_create(const float* v_template, const float* shapedirs, const float* j_regressor, const int32_t* parents,
                   const float* lbs_weights, const float* da_pose, int V, int J, int NB, nm_smpl_t* out);
int nm_smpl_destroy(nm_smpl_t smpl);
/* The differentiable form of ONE frame -- HumanNeRF.vertex_forward under autograd in the human trainer (models/human_nerf.py:92-122
 * over models/smpl.py:266-360; SURVEY 8f-1: gradients of the loss with respect to the frame's pose, shape and alignment), float32
 * throughout like the reference.  DEVICE pointers: pose [J*3], beta [NB] f32, alignment [4,4] f64 (its TRANSPOSE is applied),
 * da_pose [J*3] f32 or null (= the handle's).  workspace: nm_smpl_vertex_workspace_floats() floats.
 *   forward:  world_out [V,3], T_out [V,4,4] f32 (T_da2scene of the vertices; two launches)
 *   backward: upstream g_world [V,3] and / or g_T [V,4,4] (null = zero) -> g_pose [J*3], g_beta [NB], g_align [4,4] (gradient with
 *             respect to `alignment` as passed).  Six launches, every reduction in a fixed order (no float atomics): run to run
 *             bit-identical.  Nothing is kept between the two calls: backward recomputes the joints. */
int64_t nm_smpl_vertex_workspace_floats(nm_smpl_t smpl);
int nm_smpl_vertex_forward(nm_smpl_t smpl, const float* pose, const float* beta, const double* alignment, double scale, const float* da_pose,
                           float* workspace, float* world_out, float* T_out, nm_stream_t stream);
int nm_smpl_vertex_backward(nm_smpl_t smpl, const float* pose, const float* beta, const double* alignment, double scale, const float* da_pose,
                            const float* g_world, const float* g_T, float* workspace, float* g_pose, float* g_beta, float* g_align,
                            nm_stream_t stream);
/* The same for B frames at once -- what a sequence's pose refinement needs (preprocess/optimize_smpl.py:259-295 refines every capture of a
 * video; the frames are independent problems of one body model).  DEVICE pointers: poses [B,J*3], betas [B,NB] f32, alignments [B,4,4] f64,
 * da_pose [J*3] f32 or null (one canonical pose for all frames).  The frame is a grid dimension of the one-frame kernels: three launches
 * forward, seven backward (eight with g_joints), whatever B is.
 *   forward:  world_out [B,V,3]; joints_out [B,J,3] = the world joints of the reference's vertext_forward (preprocess/optimize_smpl.py:105-130):
 *             D(scale) align^T A_j [J_j; 1] with A_j the pose chain's joint transform and J_j the rest joint, float32; T_out [B,V,4,4] or null.
 *   backward: g_world [B,V,3], g_joints [B,J,3], g_T [B,V,4,4], each nullable (= zero) but not all three -> g_pose [B,J*3], g_beta [B,NB],
 *             g_align [B,4,4], written, not accumulated.
 *   With g_joints null, frame b's world_out, g_pose, g_beta and g_align are the SAME BITS as the one-frame entries give on frame b's
 *   inputs, whatever B is and wherever b sits: the same kernels run on the frame's slice.  joints_out and the terms g_joints adds are
 *   float32 sums in a fixed order (run to run bit-identical).
 *   workspace: nm_smpl_vertex_batch_workspace_floats(smpl, B) floats, the caller's: B x (38 J + 27 V + 24 J + 3 J + 48 ceil(V / 256)
 *   + 15 J + 16) + 64; about 0.75 MB per frame for SMPL (V 6890, J 24).  No hidden allocation.
 *   NM_ERR_ARG for a null pointer, B < 1 or B > 65535, or no upstream gradient. */
int64_t nm_smpl_vertex_batch_workspace_floats(nm_smpl_t smpl, int B);
int nm_smpl_vertex_forward_batch(nm_smpl_t smpl, const float* poses, const float* betas, const double* alignments, double scale,
                                 const float* da_pose, int B, float* workspace, float* world_out, float* joints_out, float* T_out,
                                 nm_stream_t stream);
int nm_smpl_vertex_backward_batch(nm_smpl_t smpl, const float* poses, const float* betas, const double* alignments, double scale,
                                  const float* da_pose, int B, const float* g_world, const float* g_joints, const float* g_T, float* workspace,
                                  float* g_pose, float* g_beta, float* g_align, nm_stream_t stream);
int nm_smpl_frames(nm_smpl_t smpl, const float* poses, const float* betas, const double* alignments, int B, double scale,
                   int precise, double* T_out, float* world_out, float* static_out, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused per-ray passes (nm_render_rays_bkg / nm_render_rays_human / merge + composite): ONE call per pass of the
 * reference's renderers -- utils/render_utils.py:131-151 / 287-297 (two-pass background), :213-229 / 320-329 (human pass of
 * compacted hit rays), :330-345 / 441-456 (merge + composite) -- the pass's kernels enqueued back to back on `stream`: no host
 * synchronisation inside, no hidden allocation (intermediates in the caller's `workspace`, sized by the *_workspace_floats
 * queries), the same kernels as the step-by-step entry points and therefore the same bits.
 *
 *   nm_render_rays_bkg   origin / direction [R,3], near / far [R], t_vals [S] and u [N] = the caller's torch.linspace(0,1,.);
 *       fine == NULL and N == 0: one pass (S samples); else coarse density pass -> compositing weights -> importance samples ->
 *       fine pass on S + N samples.  raw_out [R,S+N,4] and z_out [R,S+N] always; rgb [R,3] / depth [R] / acc [R] when rgb != NULL
 *       (hybrid renderers composite later, after merging).  precision_*: NM_PREC_* of each pass.
 *   nm_render_rays_human   already compacted hit rays with their per-ray near / far; mesh == NULL (and T == NULL): canonical
 *       render (camera-ray directions); else ray_to_samples -> nm_warp_to_canonical(mesh, T) -> network on the warped points and
 *       finite-difference directions.  sigma_scale = interval_comp (:229).
 *   nm_merge_composite   nm_merge_sorted + nm_composite of the merged list (disp discarded).
 * ------------------------------------------------------------------------------------------- */
int64_t nm_render_rays_bkg_workspace_floats(int64_t R, int S, int N);
int nm_render_rays_bkg(nm_mlp_t coarse, nm_mlp_t fine, const float* origin, const float* direction, const float* near, const float* far,
                       int64_t R, int S, int N, const float* t_vals, const float* u, int white_bkg, int precision_coarse, int precision_fine,
                       float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, nm_stream_t stream);
/* nm_render_rays_bkg with its passes marched (nm_march_pass above; utils/render_utils.py:131-151 / 287-297 evaluate every sample).  Two nets:
 * sample -> density-only march of the coarse net at eps_coarse (on its own transmittance: where the importance samples go) ->
 * nm_importance_from_raw -> march of the fine net at eps -> nm_composite when rgb != NULL.  One net: sample -> march at eps -> composite.
 * chunk: samples per chunk of both marches.  stats (nullable, device int64[4]): (evaluated, 0) of the composited pass, then of the coarse pass
 * (zeros with one net).  workspace: workspace_floats >= nm_render_rays_bkg_march_workspace_floats(R, S, N) floats, 16-byte aligned. */
int64_t nm_render_rays_bkg_march_workspace_floats(int64_t R, int S, int N);
int nm_render_rays_bkg_march(nm_mlp_t coarse, nm_mlp_t fine, const float* origin, const float* direction, const float* near, const float* far,
                             int64_t R, int S, int N, const float* t_vals, const float* u, int white_bkg, int precision_coarse, int precision_fine,
                             float eps, float eps_coarse, int chunk, float* workspace, int64_t workspace_floats, float* raw_out, float* z_out,
                             float* rgb, float* depth, float* acc, int64_t* stats, nm_stream_t stream);
int64_t nm_render_rays_human_workspace_floats(int64_t R, int S, int posed);
int nm_render_rays_human(nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* origin, const float* direction, const float* near,
                         const float* far, int64_t R, int S, const float* t_vals, int white_bkg, float sigma_scale, int precision,
                         float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, nm_stream_t stream);
/* K11b: nm_render_rays_human with an occupancy grid -- see the K11b block above */
int64_t nm_render_rays_human_occ_workspace_floats(int64_t R, int S, int posed);
int nm_render_rays_human_occ(nm_mlp_t human, nm_mesh_t mesh, const double* T, const uint32_t* bits, int res, const float* aabb, const float* origin,
                             const float* direction, const float* near, const float* far, int64_t R, int S, const float* t_vals, int white_bkg,
                             float sigma_scale, int precision, float* workspace, float* raw_out, float* z_out, int32_t* counts, float* rgb, float* depth,
                             float* acc, nm_stream_t stream);
/* render_hybrid_nerf's per-batch body (utils/render_utils.py:287-353; SURVEY 8b nm_render_rays_hybrid) as one call: two-pass background
 * of every ray (scalar bkg_near / bkg_far) and its composite, near / far against the posed body `verts` [V,3] (geo_threshold), compaction
 * of the hit rays (ONE host read: their count), human pass of the hit rays through `mesh` / `T`, merged composite and the human-only
 * accumulation scattered back -> rgb [R,3], depth [R], acc [R] (0 where the body is missed).  t_vals [S], u [N], t_vals_human
 * [S_human] = the caller's torch.linspace(0, 1, .).  Same kernels, same bits as the separate calls. */
int64_t nm_render_rays_hybrid_workspace_floats(int64_t R, int S, int N, int S_human);
int nm_render_rays_hybrid(nm_mlp_t coarse, nm_mlp_t fine, nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* verts, int V,
                          double geo_threshold, const float* origin, const float* direction, int64_t R, float bkg_near, float bkg_far, int S, int N,
                          int S_human, const float* t_vals, const float* u, const float* t_vals_human, int white_bkg, int precision_coarse,
                          int precision_fine, int precision_human, float* workspace, float* rgb, float* depth, float* acc, nm_stream_t stream);
/* The four calls above with the pass that is COMPOSITED -- the single or the fine background pass (utils/render_utils.py:148-151, 294-297), the
 * human pass (:213-229, 320-329) -- run as nm_mlp_forward_rays_live / nm_mlp_forward_live / nm_mlp_forward_samples_live /
 * nm_mlp_forward_listed_live: for a caller whose raw_out reaches raw2outputs (:85-95), alone or behind a sorted merge (:330-345, 441-456), and
 * nothing else.  raw_out differs from the sibling's only in the colours of samples whose stored density is <= 0, which are 0; rgb, depth and acc
 * are BIT-IDENTICAL.  The coarse pass of a two-pass background still runs nm_mlp_sigma_rays.  Each takes its sibling's arguments, then
 * live_ws (16-byte aligned), live_ws_bytes, chunk_samples (<= 0: NM_LIVE_CHUNK_SAMPLES; at least one ray's samples): the passes of one call use
 * live_ws one after another, so it holds nm_mlp_live_workspace_bytes(n, chunk_samples) bytes for the largest composited pass of the call that
 * runs in NM_PREC_I8X3 -- n = R (S + N), R S, or for nm_render_rays_hybrid_live the larger of R (S + N) and R S_human.  These are checked
 * before anything is enqueued.  The plain entries enqueue exactly what they did before these existed (one body serves both). */
int nm_render_rays_bkg_live(nm_mlp_t coarse, nm_mlp_t fine, const float* origin, const float* direction, const float* near, const float* far,
                            int64_t R, int S, int N, const float* t_vals, const float* u, int white_bkg, int precision_coarse, int precision_fine,
                            float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, void* live_ws,
                            int64_t live_ws_bytes, int64_t chunk_samples, nm_stream_t stream);
int nm_render_rays_human_live(nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* origin, const float* direction, const float* near,
                              const float* far, int64_t R, int S, const float* t_vals, int white_bkg, float sigma_scale, int precision,
                              float* workspace, float* raw_out, float* z_out, float* rgb, float* depth, float* acc, void* live_ws,
                              int64_t live_ws_bytes, int64_t chunk_samples, nm_stream_t stream);
int nm_render_rays_human_occ_live(nm_mlp_t human, nm_mesh_t mesh, const double* T, const uint32_t* bits, int res, const float* aabb,
                                  const float* origin, const float* direction, const float* near, const float* far, int64_t R, int S,
                                  const float* t_vals, int white_bkg, float sigma_scale, int precision, float* workspace, float* raw_out,
                                  float* z_out, int32_t* counts, float* rgb, float* depth, float* acc, void* live_ws, int64_t live_ws_bytes,
                                  int64_t chunk_samples, nm_stream_t stream);
int nm_render_rays_hybrid_live(nm_mlp_t coarse, nm_mlp_t fine, nm_mlp_t human, nm_mesh_t mesh, const double* T, const float* verts, int V,
                               double geo_threshold, const float* origin, const float* direction, int64_t R, float bkg_near, float bkg_far, int S,
                               int N, int S_human, const float* t_vals, const float* u, const float* t_vals_human, int white_bkg,
                               int precision_coarse, int precision_fine, int precision_human, float* workspace, float* rgb, float* depth,
                               float* acc, void* live_ws, int64_t live_ws_bytes, int64_t chunk_samples, nm_stream_t stream);
/* ONE KERNEL for the merge + composite tail of the hybrid renderers (utils/render_utils.py:330-345, 441-456): k <= 4 sorted lists per
 * ray (z[l] [.,S[l]], raw[l] [.,S[l],4]; rows[l] nullable: list l's arrays are indexed by rows[l][ray] -- e.g. the background arrays of
 * ALL rays read in place for the hit rays) -> the merged order (ties: the earlier list first, exactly what nm_merge_sorted applied list
 * by list gives) -> raw2outputs' sums.  The merged list lives in LDS only; bit-identical to nm_merge_sorted (+ ...) + nm_composite.
 * z / raw / rows / S are HOST arrays of k entries. */
int nm_merge_composite_lists(int k, const float* const* z, const float* const* raw, const int32_t* const* rows, const int* S, int64_t R,
                             const float* rays_d, int white_bkg, float* rgb, float* depth, float* acc, nm_stream_t stream);
/* nm_merge_composite_lists for 1 <= k <= 32 lists (K7c; utils/render_utils.py:441-456 with any number of actors: the background list and one
 * list per actor): the same arguments and contract -- z / raw / rows / S HOST arrays of k entries, rows[l] nullable, ties: the earlier list
 * first -- in a kernel of its own (csrc/merge_wide.hip: per-list state in LDS tables, not in unrolled registers).  Bit-identical to
 * nm_merge_sorted list by list + nm_composite, and for k <= 4 to nm_merge_composite_lists.  The merged list lives in LDS only: at most 8014
 * merged samples per ray (e.g. 320 + 31 x 192 = 6272); more, or k outside 1 .. 32, is refused with NM_ERR_ARG before anything is launched. */
int nm_merge_composite_lists_wide(int k, const float* const* z, const float* const* raw, const int32_t* const* rows, const int* S, int64_t R,
                                  const float* rays_d, int white_bkg, float* rgb, float* depth, float* acc, nm_stream_t stream);
/* nm_merge_composite_lists_wide WITH per-list layers (K7d, csrc/merge_layers.hip): the same arguments and contract, the same rgb / depth / acc
 * bit for bit, and for every list l the sums over ITS samples of what the totals sum over all, with the weight w a sample has in the merged list
 * (the other lists' occlusion resolved; ties: the earlier list first): layer_acc [R,k] = sum w, layer_rgb [R,k,3] = sum w sigmoid(rgb) --
 * premultiplied, never with a white background added --, layer_depth [R,k] = sum w z (nullable).  So sum_l layer_rgb_l + white_bkg (1 - sum_l
 * layer_acc_l) is rgb up to the rounding of the sums.  Deterministic (no atomics); the sums are formed as the totals are, so for k = 1 the layer
 * equals the totals bit for bit.  At most nm_merge_composite_layers_max_samples(k) merged samples per ray (8014 for every 1 <= k <= 32, 0 for any
 * other k); more, or k outside 1 .. 32, is refused with NM_ERR_ARG before anything is launched.  No allocation, no synchronisation. */
int nm_merge_composite_layers_max_samples(int k);
int nm_merge_composite_layers(int k, const float* const* z, const float* const* raw, const int32_t* const* rows, const int* S, int64_t R,
                              const float* rays_d, int white_bkg, float* rgb, float* depth, float* acc, float* layer_rgb, float* layer_depth,
                              float* layer_acc, nm_stream_t stream);
/* render_hybrid_nerf_multi_persons' per-batch body (utils/render_utils.py:390-456) for A >= 0 actors as one call: two-pass background of
 * every ray (scalar bkg_near / bkg_far, :396-402); when precision_last != 0 the LAST background sample of every ray evaluated once more by
 * the composited net at that NM_PREC_* (nm_mlp_forward_rays on z[:, -1:]; what the host mirror's mixed-precision policy does for the one
 * sample whose interval ends on a placeholder; 0: not done); per actor a: near / far against verts[a] [V[a],3] (geo_threshold, :405-407),
 * compaction of the hit rays -- ONE host read per actor: their count n_hit (the reference's boolean-mask indexing implies the same) --, the
 * human pass of the hit rays through humans[a] / meshes[a] / T[a] into compact [n_hit + 1, S_human] arrays whose last row is the
 * zero-density placeholder at far_z [S_human] (= the caller's torch.linspace(2 far, 3 far, S_human), :418-419), and a row index for every
 * ray; then ONE merge + composite of the 1 + A lists (:441-456): nm_merge_composite_lists up to three actors, nm_merge_composite_lists_wide
 * beyond -> rgb [R,3], depth [R].  humans / meshes / T / verts / V are HOST arrays of A entries (an actor may appear several times);
 * t_vals [S], u [N], t_vals_human [S_human] = the caller's torch.linspace(0, 1, .).  All memory is the caller's workspace
 * (nm_render_rays_multi_workspace_floats(R, S, N, S_human, A) floats: every ray may hit every actor).  A == 0 (background only), R == 0
 * and an actor nobody hits are ordinary cases.  Shapes the merge cannot stage are refused before anything is enqueued.  Same kernels, same
 * bits as the separate calls.  nm_render_rays_multi_live: as the *_live calls above -- the fine (or single) background pass and the human
 * passes evaluate the colour head on their live samples only; live_ws holds the larger of R (S + N) and R S_human samples; rgb and depth
 * are bit-identical. */
int64_t nm_render_rays_multi_workspace_floats(int64_t R, int S, int N, int S_human, int A);
int nm_render_rays_multi(nm_mlp_t coarse, nm_mlp_t fine, int A, const nm_mlp_t* humans, const nm_mesh_t* meshes, const double* const* T,
                         const float* const* verts, const int* V, double geo_threshold, const float* origin, const float* direction, int64_t R,
                         float bkg_near, float bkg_far, int S, int N, int S_human, const float* t_vals, const float* u, const float* t_vals_human,
                         const float* far_z, int white_bkg, int precision_coarse, int precision_fine, int precision_last, int precision_human,
                         float* workspace, float* rgb, float* depth, nm_stream_t stream);
int nm_render_rays_multi_live(nm_mlp_t coarse, nm_mlp_t fine, int A, const nm_mlp_t* humans, const nm_mesh_t* meshes, const double* const* T,
                              const float* const* verts, const int* V, double geo_threshold, const float* origin, const float* direction, int64_t R,
                              float bkg_near, float bkg_far, int S, int N, int S_human, const float* t_vals, const float* u, const float* t_vals_human,
                              const float* far_z, int white_bkg, int precision_coarse, int precision_fine, int precision_last, int precision_human,
                              float* workspace, float* rgb, float* depth, void* live_ws, int64_t live_ws_bytes, int64_t chunk_samples,
                              nm_stream_t stream);
/* ONE KERNEL for the coarse tail of a two-pass render (utils/render_utils.py:139-147; ray_utils.py:138-194): the compositing weights of
 * raw [R,S,4] (raw2outputs), their inverse-CDF samples at u [N] and the sorted merge with z_vals -> z_out [R,S+N]; sigma is read once,
 * the weights are written only when weights_out [R,S] != NULL.  Bit-identical to nm_composite + nm_importance_z. */
int nm_importance_from_raw(const float* raw, const float* z_vals, const float* rays_d, int64_t R, int S, const float* u, int N, float* z_out,
                           float* weights_out, nm_stream_t stream);
/* The intervals the samples of k <= 32 sorted lists per ray (z[l] [R,S[l]]; its own limit, not nm_merge_composite_lists' 4: nothing is staged in LDS) will be composited with ONCE MERGED: for every sample the distance
 * to its successor in the stable merged order (ties: the earlier list first -- nm_merge_sorted's order, the reference's sort(cat(...)),
 * utils/render_utils.py:330-337, 441-448), 1e10 for the last sample of the merged list (:86) -> dz[l] [R,S[l]].  What an early-termination
 * cut is decided on before the lists are merged.  z / S / dz are HOST arrays of k entries. */
int nm_merged_intervals(int k, const float* const* z, const int* S, int64_t R, float* const* dz, nm_stream_t stream);
int64_t nm_merge_composite_workspace_floats(int64_t R, int Sa, int Sb);
int nm_merge_composite(const float* za, const float* rawa, int Sa, const float* zb, const float* rawb, int Sb, int64_t R, const float* rays_d,
                       int white_bkg, float* workspace, float* rgb, float* depth, float* acc, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a13  sorted merge of sample lists -- reference utils/render_utils.py:330-337, 441-448
 *   Two lists per ray, each already sorted in z: (za [R,Sa], rawa [R,Sa,4]) and (zb, rawb).
 *   Writes z_out [R,Sa+Sb] sorted and raw_out [R,Sa+Sb,4] gathered in the same order
 *   (== torch.sort(cat(z)) + the three-index gather).  Apply repeatedly for k lists.
 * ------------------------------------------------------------------------------------------- */
int nm_merge_sorted(const float* za, const float* rawa, int Sa, const float* zb, const float* rawb, int Sb,
                    int64_t R, float* z_out, float* raw_out, nm_stream_t stream);

/* row gather / scatter of per-ray records (boolean-mask indexing of render_utils.py:206-212, 231-233):
 *   dst[i, :] = src[idx[i], :]  for i < n (gather)   |   dst[idx[i], :] = src[i, :] (scatter)
 * n is read from the device (counts pointer) so the host never synchronises on the hit count. */
int nm_gather_rows(const float* src, const int32_t* idx, const int32_t* n_dev, int64_t n_max, int width,
                   float* dst, nm_stream_t stream);
int nm_scatter_rows(const float* src, const int32_t* idx, const int32_t* n_dev, int64_t n_max, int width,
                    float* dst, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * a1  shot_rays / shot_all_rays on the device -- reference utils/ray_utils.py:23-38 via
 *     geometry/pcd_projector.py:85-120 (pcd_2d_to_pcd_3d) and :209-227 (integer pixel grid, no +0.5)
 *   pixel (x, y) at depth 1 -> K^-1 [x,y,1] -> camera-to-world (4x4) -> / w, all in f64, then
 *     mode 0 (shot_all_rays, :32-38): dir = (p - centre) / |p - centre| in f64, cast to f32
 *     mode 1 (shot_rays, :23-29):     p is cast to f32 first (:25), then the same (numpy promotes to an f64 centre)
 *     mode 2 (shot_rays, f32 pose):   as the reference's own CameraPose (f32 matrix from f32 quaternions,
 *                                     cameras/camera_pose.py:29-45) makes numpy do it: subtraction, norm and division in f32
 *   xy: device int32 [n,2] pixel coordinates, or NULL = the full grid of `width` columns in
 *   row-major order (render_utils.py:185).  inv_intrinsic (3x3) and cam2world (4x4) are HOST f64
 *   row-major matrices (25 by-value parameters, like the reference's numpy arrays); the centre is
 *   cam2world[:3,3] (cameras/camera_pose.py:94-95).  origin [n,3] (centre repeated), direction [n,3].
 * ------------------------------------------------------------------------------------------- */
int nm_shot_rays(const int32_t* xy, int64_t n, int width, int mode, const double* inv_intrinsic,
                 const double* cam2world, float* origin, float* direction, nm_stream_t stream);

/* The same for a training batch whose rays come from many captures at once -- reference
 *   datasets/background_rays.py:47-101 and datasets/human_rays.py:133-209 call shot_rays once per
 *   capture inside a host loop; here ray i uses camera cam_id[i] of a DEVICE table cams [n_cams][25]
 *   of f64 (K^-1 row-major, then cam2world row-major), so a batch is one launch whatever the number
 *   of captures it touches.  mode 1 / 2 as above (there is no full-grid form).  cam_id out of range
 *   is clamped.  xy device int32 [n,2]; origin, direction [n,3].                                  */
int nm_shot_rays_cams(const int32_t* xy, const int32_t* cam_id, int64_t n, int mode, const double* cams,
                      int n_cams, float* origin, float* direction, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * frame egress -- reference render_test_views.py:83-88, render_360.py:77-81 (imageio.imsave of the
 *   renderer's f32 [H,W,3] frame) and render_test_views.py:35 (PSNR of the uint8 frames).
 *   imageio is a conda dependency (environment.yml:22, unpinned), not vendored: nm_frame_to_uint8
 *   restates its published float -> uint8 rule (v2 image_as_uint: clip to [0,1], x*255 + 0.499999999,
 *   truncate; -inf gives 0, +inf 255, and a NaN gives 0, as rule F5 of the mesh frames has it).
 *   nm_ssd_u8 returns the exact integer sum of squared differences of two uint8 arrays;
 *   PSNR = 10 log10(255^2 * n / ssd) is skimage.metrics.peak_signal_noise_ratio (environment.yml:30)
 *   for uint8 inputs.  ssd: device uint64[1].
 * ------------------------------------------------------------------------------------------- */
int nm_frame_to_uint8(const float* src, int64_t n, uint8_t* dst, nm_stream_t stream);
/* A premultiplied layer of nm_merge_composite_layers (layer_rgb [n,3], layer_acc [n]) as straight-alpha RGBA bytes [n,4], what a PNG stores:
 * colour = clamp(rgb / acc, 0, 1) as an f32 quotient, 0 where acc <= 0; alpha = clamp(acc, 0, 1); each channel by nm_frame_to_uint8's rule.
 * rgba 4-byte aligned. */
int nm_layers_to_rgba8(const float* layer_rgb, const float* layer_acc, int64_t n, uint8_t* rgba, nm_stream_t stream);
int nm_ssd_u8(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* ssd, nm_stream_t stream);
/* skimage.metrics.structural_similarity(pred, gt, multichannel=True) as render_test_views.py:33 calls it, for uint8 [H,W,C]
 * images: 7x7 uniform window, K1 0.01, K2 0.03, data range 255, sample covariance, mean over the image cropped by 3 pixels
 * and over channels.  ssim: device double[1]; workspace: device double[NM_SSIM_WORKSPACE_DOUBLES]. */
#define NM_SSIM_WORKSPACE_DOUBLES 4096
int nm_ssim_u8(const uint8_t* a, const uint8_t* b, int H, int W, int C, double* ssim, double* workspace, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh rasteriser -- reference utils/render_utils.py:464-501 (phong_renderer_from_pinhole_cam,
 *   overlay_smpl) and trainers/human_nerf_trainer.py:478-481 (the SMPL overlay of validate()).
 *   The reference sits on pytorch3d 0.6.2 (environment.yml, not vendored, absent here):
 *   RasterizationSettings(blur_radius=0, faces_per_pixel=1), PerspectiveCameras(in_ndc=False),
 *   HardPhongShader, PointLights(location=(2,2,-2)), white vertices, default Materials / BlendParams;
 *   with R = R_w2c^T, T = t_w2c, principal point (W - cx, H - cy) and the rot90(k=2) of :497 its
 *   conventions cancel to the plain pinhole model stated here.  Parity with pytorch3d itself is NOT
 *   pinned by a golden; tests/helpers/raster_ref.py restates this contract in float64.
 *     1 projection  Xc = R Xw + t (w2c: HOST f64 [3][4] row-major), u = fx Xc.x / Xc.z + cx, v = fy Xc.y / Xc.z + cy;
 *                   pixel (row r, column c) is sampled at (c + 0.5, r + 0.5).
 *     2 coverage    the three screen-space barycentrics of the pixel centre all >= 0 (no top-left rule, no back-face
 *                   culling); faces of zero screen area are skipped; a face with a vertex at Xc.z <= 0 is dropped
 *                   WHOLE (a choice of this library: it is not clipped against the near plane).
 *     3 visibility  b_i' = (b_i / z_i) / sum_j (b_j / z_j), z = 1 / sum_i (b_i / z_i); the nearest z wins, the lower face
 *                   index on an exact tie -- the result does not depend on binning or scheduling order.
 *     4 shading     per pixel, world space: vertex normal = normalize(sum over the vertex's faces of cross(v1 - v0, v2 - v0)),
 *                   n = normalize(sum b_i' n_i), p = sum b_i' v_i, l = normalize(light - p), w = normalize(C - p) with C the
 *                   camera centre (normalize(x) = x / max(|x|, 1e-6)); colour = 0.5 + 0.3 max(n.l, 0)
 *                   + 0.2 [n.l > 0] max((2 (n.l) n - l).w, 0)^64 on the three channels, alpha 1; uncovered pixels (1, 1, 1, 0).
 *     5 overlay     covered pixels take uint8(colour * 255) (truncated, as np.uint8 does at :498), all others keep the image's
 *                   byte (Image.alpha_composite with alpha in {0, 255} is a select).
 *   nm_raster_create: faces HOST int32 [F,3] (every index is checked against V before any device work); the handle owns the
 *     topology, the vertex -> face table of the normals and the scratch of the passes, which grows to the largest image seen.
 *     Calls on one handle must be issued on one stream at a time.  The tile lists are sized exactly, from a scan of the per-tile
 *     counts: one 4-byte read-back (a stream synchronise) per call.
 *   nm_raster_mesh: verts DEVICE f32 [V,3] (world); face_id [H,W] int32, -1 where nothing covers; zbuf [H,W] f32, +inf there;
 *     bary [H,W,3] f32 (b', zeros there), nullable.
 *   nm_raster_phong: the same pass plus rule 4: light HOST f64 [3] (world), rgba DEVICE f32 [H,W,4], 16-byte aligned;
 *     face_id, zbuf and bary are all nullable here.
 *   nm_overlay_rgba8: rule 5 over n pixels: rgba [n,4] f32 (16-byte aligned), image and out uint8 [n,3] (two buffers).
 *   NM_ERR_ARG for a null pointer, W * H = 0, F = 0 or an index out of range.
 * ------------------------------------------------------------------------------------------- */
typedef struct nm_raster_s* nm_raster_t;
int nm_raster_create(const int32_t* faces, int F, int V, nm_raster_t* out);
int nm_raster_destroy(nm_raster_t h);
int nm_raster_mesh(nm_raster_t h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W, int H,
                   int32_t* face_id, float* zbuf, float* bary, nm_stream_t stream);
int nm_raster_phong(nm_raster_t h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W, int H,
                    int32_t* face_id, float* zbuf, float* bary, const double* light, float* rgba, nm_stream_t stream);
int nm_overlay_rgba8(const float* rgba, const uint8_t* image, uint8_t* out, int64_t n, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * soft silhouette -- reference preprocess/optimize_smpl.py:84-102 (silhouette_renderer_from_pinhole_cam:
 *   MeshRasterizer(blur_radius = log(1/1e-4 - 1) sigma, faces_per_pixel = 100) under
 *   SoftSilhouetteShader(BlendParams(sigma = 1e-4))) and :249-252 (the silhouette term of optimize_smpl
 *   and its backward to the vertices).  pytorch3d is absent, so parity with it is NOT pinned by a golden,
 *   as for the rasteriser; tests/helpers/silhouette_ref.py restates this contract in float64.  The
 *   reference's principal point (W - cx, H - cy) and its rot90(k=2) of :250 cancel to the plain pinhole
 *   image, as they do for the overlay.  The rasteriser's rules 1 and 2 hold unchanged (float64 pinhole
 *   projection, pixel centres at (c + 0.5, r + 0.5), a face with a vertex at z <= 0 or of zero screen
 *   area dropped whole); on top of them:
 *     S1 distance    for pixel centre c and face k, m_k = the smallest of the squared distances from c to the three edge
 *                    segments (foot parameter t = clamp(dot(c - a, b - a) / |b - a|^2, 0, 1)), in NDC units:
 *                    m_k = m_pixels (2 / min(W, H))^2 (pytorch3d maps the shorter image side to [-1, 1]); inside_k is
 *                    rule 2's coverage test; d_k = -m_k if inside_k, else +m_k.
 *     S2 candidates  face k contributes to the pixel iff inside_k or m_k < blur_radius (strict).
 *     S3 blend       q_k = 1 / (1 + exp(-d_k / sigma)) (= 1 - p_k, evaluated directly); keep = prod_k q_k over the
 *                    candidates; alpha = 1 - keep; a pixel without candidates has keep 1, alpha 0.
 *     S4 no K cap    EVERY candidate counts.  pytorch3d keeps the faces_per_pixel = 100 nearest in depth; this library
 *                    does not, and the two coincide wherever a pixel has <= 100 candidates: n_cand [H,W] int32
 *                    (nullable) returns the count per pixel so that a caller can tell.  Depth plays no other role.
 *     S5 gradient    the candidate set and inside_k are constants; d alpha / d d_k = -(1 - q_k) keep / sigma;
 *                    d d_k / d(screen vertices) is that of the winning segment's squared distance (at a clamped foot it
 *                    goes to that endpoint only), chained through rule 1 to the world-space vertices in float64.
 *                    keep is SAVED by the forward and read by the backward, never recomputed as 1 - alpha.
 *     S6 same bits   alpha, keep and g_verts are the same bits on every run: no float atomics; the product of S3 runs in
 *                    ascending face id, the sums of S5 in a fixed order.
 *   nm_raster_silhouette: verts DEVICE f32 [V,3] (world); alpha, keep DEVICE f32 [H,W]; n_cand DEVICE int32 [H,W] or null.
 *     One 4-byte read-back per call, as nm_raster_mesh.  It shares the handle's scratch with the rasteriser: calls on one
 *     handle go on one stream at a time.
 *   nm_raster_silhouette_backward: recomputes S1-S2 from verts (the same verts, camera, sigma and blur_radius as the
 *     forward); keep DEVICE f32 [H,W] from the forward, g_alpha DEVICE f32 [H,W] = d loss / d alpha, g_verts DEVICE f32
 *     [V,3] (written, not accumulated).  No read-back.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) for a null pointer, W * H = 0, NaN intrinsics, sigma not finite
 *   or <= 0, blur_radius not finite or < 0 -- all checked before any device work.
 * ------------------------------------------------------------------------------------------- */
int nm_raster_silhouette(nm_raster_t h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W, int H,
                         double sigma, double blur_radius, float* alpha, float* keep, int32_t* n_cand, nm_stream_t stream);
int nm_raster_silhouette_backward(nm_raster_t h, const float* verts, const double* w2c, double fx, double fy, double cx, double cy, int W,
                                  int H, double sigma, double blur_radius, const float* keep, const float* g_alpha, float* g_verts,
                                  nm_stream_t stream);
/* The soft silhouette of B frames at once: one topology (the handle's) and one image size, each frame with its own vertices and camera.
 *   Every array is a DEVICE pointer: verts [B,V,3] f32, w2c [B,4,4] f64 (row-major world-to-camera; rows 0-2 are used), intr [B,4] f64
 *   (fx, fy, cx, cy); alpha, keep [B,H,W] f32, n_cand [B,H,W] int32 or null; backward: keep, g_alpha [B,H,W], g_verts [B,V,3] written,
 *   not accumulated.
 *   Rules S1-S6 hold unchanged, per frame, and frame b's alpha, keep, n_cand and g_verts are the SAME BITS as the one-frame entries give
 *   on frame b's inputs, whatever B is and wherever b sits in the batch: the kernels are the one-frame kernels' bodies with the frame as
 *   a grid dimension, every (frame, tile) list in ascending face order, no float atomics, the same summation orders.
 *   Launches: forward six (vertex pass, face setup, count, scan, fill, blend), backward three, whatever B is.  The forward makes ONE
 *   16-byte read-back per call (the lists' total length and the bad-camera word), the backward none.
 *   List offsets are 64-bit: a batch's lists can pass 2^31 entries (some 630 candidates per pixel were measured on single frames).
 *   Scratch, owned by the handle and grown to the largest batch seen (apart from the one-frame passes' scratch):
 *     per frame  16 V + 48 F bytes (screen vertices, face records, boxes) + 12 ceil(W / 16) ceil(H / 16) (counts, offsets)
 *                + 24 F once a backward has run (per-corner gradients): 0.81 MB, then 1.14 MB, for the 13 776-face body at 1280 x 720
 *     per call   4 bytes per list entry (sum over the frames' tiles of the faces whose grown box touches the tile)
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work for a null pointer, B < 1 (or > 65535), W * H = 0,
 *   sigma not finite or <= 0, blur_radius not finite or < 0.  A non-finite entry of a frame's w2c or intr is found on the device and
 *   reported through the same read-back: the call returns NM_ERR_ARG naming the first such frame, after writing every frame's outputs
 *   (such a frame has no candidates: alpha 0, keep 1; its g_verts are 0). */
int nm_raster_silhouette_batch(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H, double sigma,
                               double blur_radius, float* alpha, float* keep, int32_t* n_cand, nm_stream_t stream);
int nm_raster_silhouette_backward_batch(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H,
                                        double sigma, double blur_radius, const float* keep, const float* g_alpha, float* g_verts,
                                        nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh frames -- the frames of an animated mesh as images, B frames in one call (csrc/raster_frames.hip).  The reference has
 *   no such step: it is what shows the mesh that the isosurface section extracts and the mesh pose section animates, as a
 *   preview that costs a fraction of one volume-rendered frame.  One topology (the handle's) and one image size; each frame
 *   has its own vertices, normals and camera.  tests/helpers/raster_frames_ref.py restates F2-F5 in float64 on top of
 *   tests/helpers/raster_ref.py.
 *     F1 geometry    per frame, rules 1-3 of the mesh rasteriser hold unchanged, and frame b's face_id, zbuf and bary are the
 *                    SAME BITS as nm_raster_mesh gives on frame b's vertices and camera, whatever B is and wherever b sits in
 *                    the batch: the same projection, edge functions, coverage test, (z, face id) minimum and barycentric
 *                    recomputation (csrc/raster_device.h has one copy of each).  These three outputs report the mesh alone:
 *                    F4 does not touch them.
 *     F2 colour      at a covered pixel, per channel in float32 without fused multiply-add: c = (b0' c0 + b1' c1) + b2' c2, the
 *                    c_i the winning face's vertex colours.  colours == null is white: c = 1 exactly, not a blend of ones.
 *     F3 light       with normals: n = normalize((b0' n0 + b1' n1) + b2' n2) on the SUPPLIED normals of the winning face's
 *                    vertices (the handle's normal table is not read), p = (b0' v0 + b1' v1) + b2' v2, l = normalize(light - p),
 *                    normalize(x) = x / max(|x|, 1e-6) as in rule 4; c *= 0.5 + 0.5 max(n.l, 0), n.l = (n0 l0 + n1 l1) + n2 l2.
 *                    There is no specular term: an avatar's colours already carry the look.  Without normals c is unlit.
 *     F4 occlusion   a covered pixel shows the mesh iff bg_z is null or z < bg_z[p] (z = zbuf[p], camera-space depth).  The
 *                    comparison is strict: a NaN bg_z hides the mesh, +inf never does.
 *     F5 bytes       a pixel that shows the mesh writes (uint8_t)fminf(fmaxf(c * 255, 0), 255) per channel: rule 5's truncation,
 *                    and a NaN gives 0.  Every other pixel takes bg's bytes, or 255, 255, 255 when bg is null.
 *     F6 launches    five launches and one memset whatever B is (vertex pass, count, scan, fill, raster + shade; the fill is
 *                    skipped when nothing is covered), and ONE 16-byte read-back per call: the lists' total length and the
 *                    bad-camera word, as in the batched silhouette.  List offsets are 64-bit.  A frame whose w2c or intr
 *                    holds a non-finite entry is found on the device: it covers nothing (face_id -1, zbuf +inf, out = the
 *                    background), and the call returns NM_ERR_ARG naming the first such frame AFTER every frame's outputs
 *                    are written.
 *     F7 same bits   every output is a function of the inputs alone and byte-identical from run to run: no float atomics; the
 *                    order in which the integer atomics leave a (frame, tile) list shows in no output, since the minimum over
 *                    (z, face id) does not depend on it.
 *   Every array is a DEVICE pointer except light: verts [B,V,3] f32 (world); w2c [B,4,4] f64 and intr [B,4] f64 as
 *   nm_raster_silhouette_batch reads them; colours [V,3] f32, ONE set for all frames, nullable; normals [B,V,3] f32 (world),
 *   nullable; light HOST f64 [3] (world), given iff normals is; bg [B,H,W,3] uint8, nullable; bg_z [B,H,W] f32 (camera-space
 *   z), nullable; out [B,H,W,3] uint8; face_id [B,H,W] int32, zbuf [B,H,W] f32 and bary [B,H,W,3] f32 each nullable.
 *   Scratch, owned by the handle and only ever grown (apart from the one-frame passes' and the batched silhouette's; the
 *   lists share the handle's list buffer, so calls on one handle go on one stream at a time):
 *     per frame  16 V bytes (screen vertices) + 12 ceil(W / 16) ceil(H / 16) (counts, offsets); no per-frame face records or
 *                boxes are kept: the raster pass reads a face through its three screen vertices
 *     per call   4 bytes per list entry (sum over the frames' tiles of the faces whose screen box touches the tile) + 16
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work for: a null handle, verts, w2c, intr or out;
 *   B < 1 or B > 65535; W * H = 0 or W * H > 2^30; normals without light or light without normals; a non-finite light.
 * ------------------------------------------------------------------------------------------- */
int nm_raster_frames(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H, const float* colours,
                     const float* normals, const double* light, const uint8_t* bg, const float* bg_z, uint8_t* out, int32_t* face_id,
                     float* zbuf, float* bary, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh lattice -- per-face colour lattices ("mesh colours": colour nodes on a regular barycentric grid of every face; no UV
 *   atlas, no seams, no packing) and the frame rasteriser that shades from them (csrc/mesh_lattice.hip, csrc/raster_device.h,
 *   csrc/raster_frames.hip).  The reference has no such step.  A thinned mesh ('mesh simplify') keeps its shape but carries
 *   one colour per vertex, so the look is sampled as sparsely as the geometry; a lattice holds more colour samples than the
 *   mesh has vertices.  It belongs to the canonical mesh: baked once (neuman_hip/mesh_texture.py), it serves every frame of
 *   every posed sequence.  tests/helpers/mesh_lattice_ref.py restates L1-L3 in numpy.
 *   Every product, sum, difference and quotient below is a float32 operation rounded on its own, no fused multiply-add.
 *     L1 nodes     resolution R, 1 <= R <= 64, the same for every face.  A face has S = (R+1)(R+2)/2 nodes (i1, i2) with
 *                  i1, i2 >= 0, i1 + i2 <= R and i0 = R - i1 - i2; node (i1, i2) is stored at
 *                  s = i2 (R+1) - i2 (i2-1)/2 + i1: rows run by i2, and row i2 has R + 1 - i2 entries.  The corners are the
 *                  nodes (0, 0), (R, 0) and (0, R) of the face's vertices 0, 1 and 2.
 *     L2 node rows nm_mesh_lattice_rows: out[f,s,:] = (w0 r0 + w1 r1) + w2 r2 with w_k = (float)i_k / (float)R (a correctly
 *                  rounded division) and r_k the rows of face f's three vertices in `rows` [V,w], any w >= 1.  With the
 *                  vertices as rows it gives the nodes' positions, with the vertex normals their (unnormalised) normals,
 *                  with per-vertex colours a lattice that F2' shades as F2 shades the colours, up to rounding.  faces [F,3]
 *                  DEVICE int32, rows [V,w] and out [F,S,w] DEVICE f32, sizes as int64_t, 1 <= V < 2^31, 1 <= 3 F < 2^31;
 *                  every offset into out is 64-bit.  A face that names an index outside [0, V) is found on the device, is
 *                  never dereferenced and none of its nodes is written; the entry then returns NM_ERR_ARG and nm_last_error()
 *                  gives the number of such faces and the lowest such face index (rule C1's words).  One 24-byte read-back (a
 *                  stream synchronise); the 64 bytes those words live in are allocated and freed by the call.
 *     L3 lookup    at a point of face f with barycentrics (b0, b1, b2):  u1 = b1 (float)R, u2 = b2 (float)R;
 *                  i1 = clamp(floorf(u1), 0, R-1), i2 = clamp(floorf(u2), 0, R-1-i1), as integers (a NaN counts as 0);
 *                  f1 = u1 - i1, f2 = u2 - i2.  The UPPER sub-triangle of cell (i1, i2) is used iff f1 + f2 > 1 and
 *                  i1 + i2 < R - 1 (a cell on the hypotenuse has no upper half, and a sum a rounding above 1 stays in
 *                  the lower one): nodes a, b, c = (i1+1, i2+1), (i1, i2+1), (i1+1, i2) with weights
 *                  ((f1 + f2) - 1, 1 - f1, 1 - f2).  Otherwise the LOWER one: nodes (i1, i2), (i1+1, i2), (i1, i2+1) with
 *                  weights ((1 - f1) - f2, f1, f2).  Per channel c = (wa ca + wb cb) + wc cc.  The interpolant is
 *                  piecewise linear and continuous over the face, so a few ulps of disagreement about the sub-triangle
 *                  move the colour by a few ulps.  Every node read lies inside face f's S nodes whatever the barycentrics.
 *     F2' colour   nm_raster_frames_lattice is nm_raster_frames with rule F2 replaced by L3 on face_colours [F,S,3] DEVICE
 *                  f32 at the winning face and its b' (b1', b2').  Rules F1 and F3-F7 of 'mesh frames' hold word for word:
 *                  face_id, zbuf and bary are the same bits as nm_raster_frames gives, the launches and the single 16-byte
 *                  read-back are the same, and so is the handle's scratch; the lattice is the caller's (12 S F bytes).
 *   Not here ('mesh atlas' exports to OBJ, 'mesh mip' filters under minification: with rule F2' alone a face far smaller
 *   than a pixel shows one cell's blend, as a vertex-coloured face shows one point of its blend): a resolution that varies
 *   from face to face.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work: nm_mesh_lattice_rows for a null pointer,
 *   w < 1, R outside [1, 64], F < 1, V < 1 or a count of 2^31 or more; nm_raster_frames_lattice for everything
 *   nm_raster_frames refuses, a null face_colours and R outside [1, 64].
 * ------------------------------------------------------------------------------------------- */
int nm_mesh_lattice_rows(const int32_t* faces, int64_t F, int64_t V, const float* rows, int w, int R, float* out, nm_stream_t stream);
int nm_raster_frames_lattice(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H,
                             const float* face_colours, int R, const float* normals, const double* light, const uint8_t* bg, const float* bg_z,
                             uint8_t* out, int32_t* face_id, float* zbuf, float* bary, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh mip -- a pyramid of the colour lattices of 'mesh lattice' and the frame rasteriser that filters with it under
 *   minification (csrc/mesh_lattice.hip, csrc/raster_device.h, csrc/raster_frames.hip).  The reference has no such step.
 *   One R serves the whole mesh, so short faces are over-resolved, and a far camera draws faces two or three pixels wide whose
 *   R = 8 lattice has nine nodes along an edge; rule L3 point-samples that lattice at the pixel centre, which shows as moire
 *   within a frame and as shimmer from frame to frame.  tests/helpers/mesh_mip_ref.py restates M1-M3 in numpy.  As in 'mesh
 *   lattice' every product, sum, difference and quotient is a float32 operation rounded on its own, no fused multiply-add;
 *   sqrtf is the correctly rounded one.
 *     M1 pyramid   a lattice [F,S(R0),w] has levels l = 0 .. with resolution R_l = R0 >> l while 2^l divides R0: at most
 *                  1 + (the trailing zero bits of R0) levels -- 4 for R0 = 8, 1 for an odd R0, 7 for R0 = 64.  The pyramid
 *                  is one f32 buffer, level-major: level l is a contiguous [F,S(R_l),w] block after the blocks of the finer
 *                  levels, level 0 the input byte for byte.  nm_mesh_lattice_pyramid_size (HOST only) gives the sum of
 *                  S(R_l) over the levels, so the buffer holds F w times that many floats.  Coarse node (i1, i2) of level
 *                  l+1 sits on fine node (2 i1, 2 i2) of level l, value c, and is
 *                    a corner (two of i0, i1, i2 zero)    c, copied;
 *                    an edge node (exactly one zero)      0.5 c + 0.25 (a + b), a and b the two fine neighbours along that
 *                                                         edge, a the one with the smaller i1 (on the edge i1 = 0: the
 *                                                         smaller i2);
 *                    interior                             0.25 c + 0.125 (((((n0 + n1) + n2) + n3) + n4) + n5) over the six
 *                                                         fine neighbours at (+1,0), (0,+1), (-1,+1), (-1,0), (0,-1), (+1,-1)
 *                                                         in (i1, i2), which all exist.
 *                  These weights are the transpose of linear prolongation on the triangular lattice (restricted to the edge
 *                  on an edge): a linear lattice stays linear at every level.  Edge and corner values depend on nodes of
 *                  that edge alone, so two faces whose shared-edge nodes agree at level 0 agree there at every level: no
 *                  seam is added.  nm_mesh_lattice_pyramid: lattice and out DEVICE f32; lattice == out is the in-place form
 *                  (level 0 is already in out), otherwise the two must not overlap and level 0 is copied on the stream.
 *                  One launch per coarser level, one thread per coarse node, every node written once; no read-back, no
 *                  workspace.  1 <= w <= 64.
 *     M2 level     one value per frame and face, computed at the pixel from the winner's screen vertices (x0,y0), (x1,y1),
 *                  (x2,y2) (rule 1's u, v as floats): d01 = v1 - v0, d02 = v2 - v0, d12 = v2 - v1;
 *                  e2 = max(max(|d01|^2, |d02|^2), |d12|^2) with |d|^2 = dx dx + dy dy; cr = |d01.x d02.y - d01.y d02.x|;
 *                  rho = ((lod_scale (float)R0) sqrtf(e2)) / cr: the level-0 nodes per pixel across the face's narrowest
 *                  extent under an affine approximation (perspective inside a face is ignored).  l = 0; while rho >= 2 and
 *                  l < levels - 1: rho *= 0.5, ++l.  t = (l < levels - 1) ? fminf(fmaxf(rho - 1, 0), 1) : 0.  A NaN rho gives
 *                  l = 0, t = 0 (fmaxf returns its other operand); an infinite one the coarsest level.
 *     M3 colour    c = L3 on level l of face f at (b1', b2'); if t > 0, c = c + t (L3 on level l+1 - c) per channel.  With
 *                  t == 0 the second lookup is skipped and c is L3's own bits on that level.
 *     F2'' colour  nm_raster_frames_lattice_mip is nm_raster_frames_lattice with rule F2' replaced by M2 and M3 on pyramid
 *                  [levels][F,S(R_l),3].  Rules F1 and F3-F7 hold word for word: the same geometry bits, launches, single
 *                  16-byte read-back and scratch.  lod_scale = 0 is nm_raster_frames_lattice on level 0; a huge one is
 *                  nm_raster_frames_lattice on the coarsest level.
 *   Not here: filtering the corner nodes across the faces around a vertex (they stay point samples, as per-vertex colours
 *   are); a level that varies inside a face, anisotropic filtering; atlas padding for mip-mapping viewers; a per-face R.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work: a null pointer, R0 outside [1, 64], levels
 *   < 1 or more than R0 allows, w outside [1, 64], F < 1 or 3 F >= 2^31; nm_raster_frames_lattice_mip for everything
 *   nm_raster_frames refuses, a null pyramid and a lod_scale that is negative or not finite.
 * ------------------------------------------------------------------------------------------- */
int nm_mesh_lattice_pyramid_size(int R0, int levels, int64_t* nodes_per_face_total);
int nm_mesh_lattice_pyramid(const float* lattice, int64_t F, int R0, int levels, int w, float* out, nm_stream_t stream);
int nm_raster_frames_lattice_mip(nm_raster_t h, const float* verts, const double* w2c, const double* intr, int B, int W, int H,
                                 const float* pyramid, int R0, int levels, float lod_scale, const float* normals, const double* light,
                                 const uint8_t* bg, const float* bg_z, uint8_t* out, int32_t* face_id, float* zbuf, float* bary,
                                 nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh atlas -- a texture atlas packed from the colour lattices of 'mesh lattice', so that a lattice-coloured mesh can leave
 *   the project as an OBJ with one image (csrc/mesh_atlas.hip, neuman_hip/mesh_export.py).  The reference has no such step.
 *   Two faces share a block of texels; the nodes of a face are texels, and the gutter between the two faces is filled so
 *   that a viewer's bilinear filter shows rule L3's blend in the cells on the hypotenuse.
 *   tests/helpers/mesh_atlas_ref.py restates A1-A5 in numpy.  As in 'mesh lattice' every product, sum and difference is a
 *   float32 operation rounded on its own, no fused multiply-add; every offset is 64-bit.  S = (R+1)(R+2)/2 and node
 *   (i1, i2) sits at the index rule L1 gives it.
 *     A1 size      nm_mesh_atlas_size, HOST only, no device work.  A block is BW = R+4 texels wide and BH = R+1 high; faces
 *                  2p and 2p+1 share block p, P = ceil(F/2) blocks.  nbx = the smallest n >= 1 with n n BW >= P BH (integer
 *                  arithmetic only: the atlas is about square), nby = ceil(P / nbx), W = nbx BW, H = nby BH.  Block p starts
 *                  at x0 = (p mod nbx) BW, y0 = (p div nbx) BH.  E.g. (F, R) = (13776, 8) gives 864 x 864 with nbx = 72,
 *                  (600, 8) 180 x 180, (10, 5) 18 x 18, (1, 1) 5 x 2.
 *     A2 texels    in block-local (x, y), 0 <= x < BW, 0 <= y < BH: node (i1, i2) of the even ("lower") face sits at
 *                  (i1, i2); the odd ("upper") face is the same picture under the point reflection (x, y) -> (R+3-x, R-y).
 *                  Lower nodes have x + y <= R, upper nodes x + y >= R+3; the diagonals x + y = R+1 and x + y = R+2 are the
 *                  lower and the upper face's gutters.  Every texel of a block belongs to exactly one of the four sets.
 *     A3 values    nm_mesh_atlas_pack: face_colours [F,S,3] -> atlas [H,W,3], both DEVICE f32, row 0 first.  One thread per
 *                  texel, gather form: every texel of the atlas is written exactly once; no memset, no atomic, no
 *                  read-back.  In a face's own (unreflected) local coordinates: a node texel is a bit copy of its node; a
 *                  gutter texel (x, y) with x + y = R+1 and 1 <= x <= R is (c(x, y-1) + c(x-1, y)) - c(x-1, y-1); the
 *                  gutter texel (R+1, 0) is a copy of node (R, 0); the upper half of the last block when F is odd and the
 *                  blocks p >= P of the last row are +0.0.  A NaN node gives a NaN texel and a NaN in each gutter texel
 *                  computed from it, nothing else.  The values are not clamped: the byte egress (nm_frame_to_uint8) clamps.
 *     A4 uv        corner k of face f is node (0, 0), (R, 0) or (0, R); its texture coordinate is the centre of that node's
 *                  texel (X, Y): u = (X + 0.5) / W, v = 1 - (Y + 0.5) / H in float64 (image row 0 is the top row, as OBJ
 *                  viewers expect).  No two faces share a coordinate.  No entry point: neuman_hip.mesh_export.atlas_uvs.
 *     A5 sample    nm_mesh_atlas_sample: what a viewer with bilinear filtering shows at a point of face f with barycentrics
 *                  (b0, b1, b2).  The cell is L3's: u1 = b1 (float)R, u2 = b2 (float)R; i1 = clamp(floorf(u1), 0, R-1),
 *                  i2 = clamp(floorf(u2), 0, R-1-i1) (a NaN counts as 0); f1 = u1 - i1, f2 = u2 - i2.  Per channel
 *                  c = ((1-f1)(1-f2) t00 + f1 (1-f2) t10) + ((1-f1) f2 t01 + f1 f2 t11), each weight ONE product of two
 *                  rounded factors, t_ab the texel at local (i1+a, i2+b) of the face's half block (reflected for an odd
 *                  face).  face_id [n] DEVICE int32, bary [n,3] and out [n,3] DEVICE f32: exactly the face_id and bary
 *                  nm_raster_frames returns, so a textured view is that call followed by this one.  A face_id outside
 *                  [0, F) gives (0, 0, 0) and reads nothing; whatever the barycentrics, every read lies inside the face's
 *                  own half block.  One thread per point, no read-back.
 *   Derived: at a node's barycentrics the sample is the node.  With D = t00 - t10 - t01 + t11 the sample is L3's value plus
 *   f1 f2 D in a cell's lower sub-triangle and plus (1-f1)(1-f2) D in its upper one, at most |D| / 4 in magnitude; in a
 *   cell on the hypotenuse A3's gutter makes D vanish (up to its own rounding), so there the sample is L3's value.
 *   Not here: a textured colour source inside nm_raster_frames; padding for mip-mapped viewers; glTF.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work: a null pointer, F < 1, R outside
 *   [1, 64], W or H above 16384 (e.g. F = 2^20 at R = 64), and for nm_mesh_atlas_sample n < 1.
 * ------------------------------------------------------------------------------------------- */
int nm_mesh_atlas_size(int64_t F, int R, int* W, int* H, int* nbx);
int nm_mesh_atlas_pack(const float* face_colours, int64_t F, int R, float* atlas, nm_stream_t stream);
int nm_mesh_atlas_sample(const float* atlas, int64_t F, int R, const int32_t* face_id, const float* bary, int64_t n, float* out,
                         nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * isosurface -- a scalar field on a regular grid as an indexed triangle mesh (csrc/isosurface.hip).  The reference has
 *   no such step; it is what turns a trained density into geometry (neuman_hip/mesh_extract.py).  Marching tetrahedra
 *   on the Kuhn (Freudenthal) split of every cell: no 256-case table and no ambiguous case; the 16 cases of a
 *   tetrahedron are built in code from rule M5.  tests/helpers/isosurface_ref.py restates the rules in numpy.
 *     M1 grid      field f[nz][ny][nx] DEVICE f32 at the vertices of a regular grid over aabb = HOST float[6] (lo x y z,
 *                  hi x y z); (nx-1)(ny-1)(nz-1) cells; the dims are independent, each >= 2, nx ny nz < 2^31.  Vertex
 *                  (i, j, k) has linear index v = (k ny + j) nx + i and position p = fmaf(i, h, lo) per axis with
 *                  h = (hi - lo) / (n - 1), every step in float32.
 *     M2 inside    a vertex is inside iff f > level; a NaN is outside.  No NaN or Inf reaches an output.
 *     M3 split     a cell is six tetrahedra, one per permutation (a, b, c) of the axes in lexicographic order, with
 *                  corners v0, v0 + e_a, v0 + e_a + e_b, v0 + (1,1,1) in that order (corners 0..3).  The split is the same
 *                  in every cell, so neighbours agree on shared faces and the surface is watertight by construction.
 *     M4 vertices  every mesh vertex lies on one of the seven edges leaving a grid vertex toward higher indices: direction
 *                  d = m - 1 for the offset mask m = 1..7 (bit 0 +x, bit 1 +y, bit 2 +z: x, y, xy, z, xz, yz, xyz).  Edge id
 *                  = 7 v + d.  An edge is crossed iff its endpoints differ in M2.  The mesh vertex index is the rank of
 *                  its edge among the crossed edges in ascending edge id (count -> scan -> fill, no atomics: the same
 *                  bits on every run).  Position: from the lower-index endpoint a toward b, per axis,
 *                  t = (level - fa) / (fb - fa) as an IEEE float32 division, p = fmaf(t, pb - pa, pa); where t is not
 *                  in [0, 1] (an endpoint is NaN or infinite) t = 0.5.
 *     M5 faces     a tetrahedron with 1 or 3 inside corners gives one triangle, on the three edges that join the lone
 *                  corner L to the others X < Y < Z: (LX, LY, LZ).  With 2 inside corners A < B and outside C < D it gives two:
 *                  the quad (AC, AD, BD, BC) cut along the diagonal from AC -- the edge at (lowest inside, lowest
 *                  outside) -- to the opposite edge BD: (AC, AD, BD), (AC, BD, BC).  The last two vertices of every triangle are
 *                  swapped iff [the corner list (inside ascending, then outside ascending) is an odd permutation of 0..3] xor
 *                  [(a, b, c) is an odd permutation]: orientation comes from the case and the tetrahedron's parity, never
 *                  from computed geometry, so triangles of zero area (grid values equal to level) are wound consistently too.
 *                  Counter-clockwise vertices: the normal points from inside to outside.  Output order: cells in
 *                  (k, j, i) order, then tetrahedron 0..5, then triangle 0..1; offsets from a scan.
 *     M6 normals   per mesh vertex: -g / |g|, g = fmaf(t, gb - ga, ga) per axis from the gradients at the edge's endpoints
 *                  with M4's t; gradient per axis = (f[i+1] - f[i-1]) / (2 h), at a box face (f[1] - f[0]) / h resp.
 *                  (f[n-1] - f[n-2]) / h; |g| = sqrt((gx gx + gy gy) + gz gz).  |g| zero or not finite gives (0, 0, 0).
 *     M7 sizes     counts are 64-bit on the device.  nm_isosurface_count reports n_verts and n_faces to the host in ONE
 *                  16-byte read-back (a stream synchronise) and nothing else; nm_isosurface_fill reads the same 16 bytes
 *                  back from the workspace and refuses capacities smaller than the counts.
 *   workspace: DEVICE, 16-byte aligned, nm_isosurface_workspace_bytes(nx, ny, nz) bytes = 2.5 bytes per grid vertex (one byte of
 *     crossed-edge flags, one byte of the anchored cell's face count, two uint16 prefix counts per eight vertices) + 32 bytes
 *     per 2048 vertices (the scan's spans) + 64: no index is stored per edge; a vertex index is recovered by a rank query.
 *     nm_isosurface_count fills it; nm_isosurface_fill takes it with the same field, dims and level and writes verts [n_verts,3]
 *     f32, normals [n_verts,3] f32 (nullable) and faces [n_faces,3] int32.  A mesh of 2^31 vertices or faces or more is
 *     counted but not filled (NM_ERR_UNSUPPORTED).  With n_verts = 0 the fill launches nothing; an output of capacity 0 may be null.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work for a null pointer, a dim < 2 or 2^31
 *   vertices, a box that is not finite or not lo < hi on every axis, a level that is not finite, a workspace that is
 *   misaligned or short.
 * ------------------------------------------------------------------------------------------- */
int64_t nm_isosurface_workspace_bytes(int nx, int ny, int nz);
int nm_isosurface_count(const float* field, int nx, int ny, int nz, const float* aabb, float level, void* workspace, int64_t workspace_bytes,
                        int64_t* n_verts, int64_t* n_faces, nm_stream_t stream);
int nm_isosurface_fill(const float* field, int nx, int ny, int nz, const float* aabb, float level, const void* workspace,
                       int64_t workspace_bytes, float* verts, float* normals, int32_t* faces, int64_t cap_verts, int64_t cap_faces,
                       nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh components -- clean-up of an indexed triangle mesh (csrc/mesh_components.hip): its connected components, their
 *   sizes and boxes, and the mesh compacted to a chosen subset of them.  A learned density thresholded at any level is the
 *   body plus small closed blobs in empty space; this is what drops them (neuman_hip/mesh_extract.py: components,
 *   select_components, clean_mesh).  tests/helpers/mesh_components_ref.py restates the rules in numpy.
 *     C1 mesh      faces [F,3] DEVICE int32 over V vertices, 0 <= V, F < 2^31 (passed as int64_t).  A face that names an
 *                  index outside [0, V) is invalid: it is counted and never dereferenced.  With any invalid face
 *                  nm_mesh_components returns NM_ERR_ARG, nm_last_error() gives their number and the lowest invalid face
 *                  index, and nothing outside the caller's buffers has been written.  (The other three entry points take
 *                  labels, so they never follow an index or a label that is out of range: such a face or vertex counts
 *                  nowhere and is kept nowhere.)
 *     C2 connect   two vertices are connected if some face names both (vertex connectivity: what a welded marching-
 *                  tetrahedra mesh shares); components are the classes of that relation among the REFERENCED vertices.
 *                  Degenerate faces ((a,a,b), (a,a,a)) and repeated faces count like any other.  A vertex that no face
 *                  names has label -1 and belongs to no component.
 *     C3 labels    a component's representative is its smallest vertex index; its id is the rank of the representative
 *                  among all representatives in ascending order, 0 .. C-1.  vert_label [V] int32; face_label [F] int32
 *                  (nullable) = the label of the face's first vertex.
 *     C4 stats     comp_verts [C], comp_faces [C] int32; with verts [V,3] f32 given, comp_box [C,6] f32 (lo x y z, hi x y z)
 *                  over the component's vertices in the order -inf < ... < -0 < +0 < ... < +inf; a NaN coordinate is
 *                  skipped, an axis with no usable coordinate reads +inf, -inf.  verts == NULL requires comp_box == NULL.
 *     C5 select    keep [C] DEVICE uint8.  A vertex is kept iff its label is >= 0 and keep[label] != 0; a face is kept iff
 *                  its label (its first vertex's) is kept.  A kept vertex's new index is its rank among the kept vertices in
 *                  ascending old index; kept faces stay in their old order with their indices remapped.  vert_src
 *                  [n_verts_out] int32 (new -> old) is exactly the idx nm_gather_rows takes; faces_out [n_faces_out,3]
 *                  int32.  Keeping everything on a mesh without unreferenced vertices reproduces it byte for byte;
 *                  keeping nothing gives two empty outputs.
 *     C6 reads     nm_mesh_components reports {n_components, n_invalid, first_invalid} in ONE 24-byte read-back (a stream
 *                  synchronise); nm_mesh_select_count {n_verts_out, n_faces_out} in one of 16 bytes.
 *                  nm_mesh_component_stats and nm_mesh_select_fill read nothing back and do not synchronise:
 *                  nm_mesh_select_count leaves its totals in the workspace AND remembers them on the host under the
 *                  workspace's address (the 64 most recent workspaces; any later nm_mesh_components or
 *                  nm_mesh_select_count on that workspace replaces the record); nm_mesh_select_fill compares its counts
 *                  with that record on the host, and its kernel with the workspace's header.
 *     C7 determinism  every output is a function of the inputs alone, byte-identical from run to run, and vert_label
 *                  does not change when the rows of faces are permuted: labelling is a lock-free union-find in which the
 *                  larger root is linked under the smaller by compare-and-swap, so a class's root ends as its smallest
 *                  vertex under every interleaving; the rankings are count -> scan -> fill.  Only integer atomics whose
 *                  result is order-independent are used (compare-and-swap, min, max, add), the boxes through the order-
 *                  preserving integer image of a float; nothing adds floats atomically.
 *   workspace: DEVICE, 16-byte aligned, nm_mesh_components_workspace_bytes(V, F) bytes = 9 bytes per vertex (parent and rank,
 *     4 bytes each, one flag byte) + 4 bytes per face (its rank) + 16 bytes per 1024 vertices and per 1024 faces (the scans'
 *     spans) + 64 and padding below 64: linear in V and F, under 16 V + 8 F + 256.  The same size serves nm_mesh_components
 *     and the selection pair, which may share one buffer (labels and statistics are outputs, not workspace).
 *     nm_mesh_select_count fills it; nm_mesh_select_fill takes it with the same faces, V, F, labels and keep.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work for a null pointer (an array of no rows may
 *   be null), a count that is negative or >= 2^31, a workspace that is misaligned or short, comp_box without verts,
 *   n_verts_out / n_faces_out other than what nm_mesh_select_count left for this workspace.
 * ------------------------------------------------------------------------------------------- */
int64_t nm_mesh_components_workspace_bytes(int64_t V, int64_t F);
int nm_mesh_components(const int32_t* faces, int64_t F, int64_t V, int32_t* vert_label, int32_t* face_label /* nullable */, void* workspace,
                       int64_t workspace_bytes, int64_t* n_components, nm_stream_t stream);
int nm_mesh_component_stats(const int32_t* faces, int64_t F, int64_t V, const int32_t* vert_label, const float* verts /* nullable */, int64_t C,
                            int32_t* comp_verts, int32_t* comp_faces, float* comp_box /* nullable */, nm_stream_t stream);
int nm_mesh_select_count(const int32_t* faces, int64_t F, int64_t V, const int32_t* vert_label, const uint8_t* keep, int64_t C, void* workspace,
                         int64_t workspace_bytes, int64_t* n_verts_out, int64_t* n_faces_out, nm_stream_t stream);
int nm_mesh_select_fill(const int32_t* faces, int64_t F, int64_t V, const int32_t* vert_label, const uint8_t* keep, int64_t C,
                        const void* workspace, int64_t workspace_bytes, int32_t* vert_src, int32_t* faces_out, int64_t n_verts_out,
                        int64_t n_faces_out, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh pose -- a canonical-space mesh animated by the body it is bound to (csrc/mesh_pose.hip): per vertex and frame the
 *   barycentric blend of three of the body's per-vertex transforms, applied to the canonical point and normal.  It is the blend
 *   of section a11's warp -- reference utils/ray_utils.py:56-58, `T_interp = (T[faces[f]] * bary[..., None, None]).sum(axis=1)` --
 *   run FORWARDS: the reference inverts the blend to take an observed sample to canonical space (:58), this applies it as it is
 *   to take a canonical vertex to the scene, for every frame of a sequence in one launch.  neuman_hip/mesh_pose.py (bind_mesh,
 *   pose_mesh, pose_mesh_frames) binds an extracted mesh (section 'isosurface', 'mesh components') and poses it;
 *   tests/helpers/mesh_pose_ref.py restates the rules in numpy.
 *     P1 inputs    all pointers are DEVICE pointers.  T [B, t_rows, 4, 4] row-major canonical -> scene transforms, 16-byte aligned:
 *                  t_f64 = 1: float64, what nm_smpl_frames writes (t_rows = V + J); t_f64 = 0: float32, what
 *                  nm_smpl_vertex_forward_batch's T_out is (t_rows = V).  tri [N,3] int32 row indices into a frame's table,
 *                  bary [N,3] f32; with per_frame_binding = 1 both are [B,N,3].  pts, normals [N,3] f32: the canonical mesh,
 *                  shared by all frames.  out_pts, out_normals [B,N,3] f32.  1 <= B <= 65535 (the frame is a grid dimension, as in
 *                  the batched SMPL entries), 0 <= N < 2^31, 1 <= t_rows < 2^31.  N = 0 returns NM_OK without a launch.  Every
 *                  offset into [B,N,3] and [B,t_rows,16] is computed in 64 bits.
 *     P2 blend     per vertex i and frame b, in float64 (a float32 input converts exactly), elementwise over the entries of rows
 *                  0-2 in this association, no fused multiply-add:   M = (b0 T[t0] + b1 T[t1]) + b2 T[t2]
 *     P3 point     p_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3 for r = 0, 1, 2 in float64, rounded once to float32.  Row 3 of a
 *                  transform is never read: the reference likewise takes [:, :3, 0] without dividing.
 *     P4 normal    with normals given: A = the upper 3x3 of M; its cofactor matrix C row by row = cross(A_row1, A_row2),
 *                  cross(A_row2, A_row0), cross(A_row0, A_row1), with cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0),
 *                  each component two products and one subtraction;  n'_r = (C_r0 n0 + C_r1 n1) + C_r2 n2;
 *                  s = (n'0^2 + n'1^2) + n'2^2;  the output is n' / sqrt(s), rounded once to float32, and (0, 0, 0) if s is zero or
 *                  not finite.  This is the normal the transformed faces' winding gives, reflections included.
 *     P5 invalid   a vertex any of whose three indices lies outside [0, t_rows) is never dereferenced: its output point, and its
 *                  output normal if present, is NaN in every frame (with per_frame_binding = 1: in the frames where its indices
 *                  are bad), and *n_invalid (DEVICE int32, nullable, zeroed by the caller) is increased by one per such
 *                  (frame, vertex) through an integer atomic add: the sum does not depend on order.  The entry reads nothing
 *                  back and does not synchronise.
 *     P6 determinism  every output element is a function of the inputs alone, the same bits from run to run, and frame b of a
 *                  B-frame call is the same bits as a one-frame call on frame b's slice.  One thread per vertex and frame: no
 *                  float atomics, no workspace, no hidden allocation.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work for a null required pointer with N > 0,
 *   out_normals without normals or the reverse, B, N or t_rows out of range, t_f64 or per_frame_binding other than 0 or 1, a T
 *   that is not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int nm_mesh_pose_batch(const void* T, int t_f64, int64_t t_rows, int B, const int32_t* tri, const float* bary, int per_frame_binding,
                       const float* pts, const float* normals /* nullable */, int64_t N, float* out_pts,
                       float* out_normals /* nullable iff normals is */, int32_t* n_invalid /* nullable, DEVICE, caller-zeroed */,
                       nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh smooth -- topology-preserving smoothing of an indexed triangle mesh (csrc/mesh_smooth.hip): the vertex -> incident
 *   faces adjacency, Taubin lambda|mu steps over it, and vertex normals from the mesh's own faces.  A learned density is
 *   noisy: what section 'isosurface' extracts is rippled at the scale of a grid cell.  The smoothing moves vertices only, so
 *   `faces` stays byte for byte and every later stage ('mesh components', 'mesh pose', the rasteriser) takes the result
 *   unchanged; the normals serve any mesh whose vertices have moved, a posed frame included (neuman_hip/mesh_smooth.py:
 *   adjacency, smooth_mesh, vertex_normals).  tests/helpers/mesh_smooth_ref.py restates the rules in numpy.
 *   Every product, sum and quotient below is a float64 operation rounded on its own, in the association stated, no fused
 *   multiply-add; a float32 input converts exactly.
 *     S1 mesh      faces [F,3] DEVICE int32 over V vertices, sizes passed as int64_t, 0 <= V < 2^31, 0 <= 3 F < 2^31.  A face
 *                  that names an index outside [0, V) is invalid: it is counted and never dereferenced.  With any invalid face
 *                  nm_mesh_adjacency returns NM_ERR_ARG, nm_last_error() gives their number and the lowest invalid face index
 *                  (rule C1's behaviour), and nothing outside the caller's buffers has been written.  A valid face is PROPER
 *                  if its three indices are pairwise distinct; only proper faces enter the adjacency: a degenerate face joins
 *                  no list and contributes to nothing.  Repeated faces count as often as they occur.
 *     S2 adjacency inc_off [V+1] int32, inc [3 F] int32 (allocated at the bound; the first n_incident = 3 x the number of
 *                  proper faces entries are written).  inc[inc_off[v] .. inc_off[v+1]) holds the proper faces that name v in
 *                  ascending face index; a vertex no proper face names has an empty list.  boundary [V] uint8 (nullable):
 *                  boundary[v] = 1 iff there is a vertex u such that exactly one proper face names both u and v (an edge
 *                  with one face; an edge with three or more is no boundary), else 0.  nm_mesh_adjacency reports
 *                  {n_incident, n_invalid, first_invalid} in ONE 24-byte read-back (a stream synchronise) and nothing else.
 *                  The lists are built count -> scan -> fill through an integer atomic cursor -> a sort of every vertex's
 *                  segment in place by its lane: insertion sort up to 32 entries, heap sort (O(k log k), no second buffer)
 *                  beyond, so no vertex costs time quadratic in its valence past that threshold.  The boundary flag comes from
 *                  the sorted neighbour ids of the vertex's faces (two per face): an id that occurs exactly once.
 *     S3 step      rows x [V,w] float32, 1 <= w <= 64 (positions: w = 3; colours or any attribute go through the same call),
 *                  factor t.  For a vertex v with k = inc_off[v+1] - inc_off[v] > 0 and hold[v] == 0 (hold [V] uint8,
 *                  nullable = all zero), per column:  s = 0;  for each incident face in list order, rotated so that v comes
 *                  first, (v, p, q):  s = (s + x[p]) + x[q];  m = s / (2 k);  d = m - x[v];  x'[v] = (float)(x[v] + t d).
 *                  This is the umbrella operator with each neighbour weighted by the faces it shares with v (on a closed
 *                  manifold the uniform umbrella).  The sum is left to right as written: one lane's loop, never a tree.  A
 *                  vertex with k = 0 or hold[v] != 0 keeps its bits.  A step reads only the previous step's rows (Jacobi).
 *     S4 schedule  iterations = n >= 0; an iteration is a step with lambda, then a step with mu if mu != 0 (mu == 0: plain
 *                  Laplacian smoothing).  All steps run in one call, ping-ponging between out and the caller's scratch (both
 *                  [V,w]); the buffer the first step writes is chosen by parity so that the last step writes out.  n = 0
 *                  copies rows to out byte for byte.  No read-back, no synchronise.  Taubin's pair lambda = 0.5, mu = -0.53
 *                  has the pass-band 1/lambda + 1/mu ~ 0.11 and does not shrink the body.
 *     S5 normals   verts [B,V,3] float32, B >= 1, B V < 2^31, the frame a grid dimension: all B frames in one launch.  For
 *                  frame b and vertex v:  n = 0;  for each incident face f = (a, b, c) in list order and in STORED vertex order,
 *                  u = x[b] - x[a], w = x[c] - x[a]:  n += cross(u, w) component-wise, cross(u, w) = (u1 w2 - u2 w1,
 *                  u2 w0 - u0 w2, u0 w1 - u1 w0), each component two products and one difference;  l2 = (nx nx + ny ny) + nz nz;
 *                  normals[b,v] = (float)(n / sqrt(l2)), and (0, 0, 0) if l2 is not finite or not > 0 or the list is empty.
 *                  Area-weighted; outward for the counter-clockwise faces nm_isosurface_fill makes.  Frame b of a B-frame call
 *                  is the same bits as a one-frame call on frame b.  No read-back.
 *     S6 determinism  every output is a function of the inputs alone, byte-identical from run to run, and boundary does not
 *                  change when the rows of faces are permuted.  Only integer atomics whose result is order-independent are used
 *                  (add); the one order-dependent intermediate, a list's order after the fill, is removed by the sort.  Nothing
 *                  adds floats atomically.
 *   nm_mesh_smooth and nm_mesh_vertex_normals trust inc_off / inc only as far as nm_mesh_adjacency made them for the same
 *   faces, V, F; they still never follow an offset, a face index or a vertex index that is out of range, nor a face that does
 *   not name the vertex (smooth): such an entry is skipped, and a vertex none of whose entries is followed keeps its bits.
 *   workspace: DEVICE, 16-byte aligned, nm_mesh_adjacency_workspace_bytes(V, F) bytes = 4 bytes per vertex (its counter, then
 *     the fill's cursor) + 24 bytes per face (six neighbour ids) + 16 bytes per 1024 vertices (the scan's spans) + 64 and
 *     padding below 32: linear in V and F, under 8 V + 24 F + 256.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work for a null pointer (an array of no rows may
 *   be null; inc_off never has no rows), V or 3 F negative or >= 2^31, B < 1 or B V >= 2^31, width outside 1..64,
 *   iterations < 0, lambda or mu not finite, a workspace that is misaligned or short, rows / out / scratch (or verts /
 *   normals) that overlap.
 * ------------------------------------------------------------------------------------------- */
int64_t nm_mesh_adjacency_workspace_bytes(int64_t V, int64_t F);
int nm_mesh_adjacency(const int32_t* faces, int64_t F, int64_t V, int32_t* inc_off, int32_t* inc, uint8_t* boundary /* nullable */,
                      void* workspace, int64_t workspace_bytes, int64_t* n_incident, nm_stream_t stream);
int nm_mesh_smooth(const float* rows, int width, int64_t V, const int32_t* faces, int64_t F, const int32_t* inc_off, const int32_t* inc,
                   const uint8_t* hold /* nullable */, float lambda, float mu, int iterations, float* out, float* scratch,
                   nm_stream_t stream);
int nm_mesh_vertex_normals(const float* verts, int64_t B, int64_t V, const int32_t* faces, int64_t F, const int32_t* inc_off,
                           const int32_t* inc, float* normals, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mesh simplify -- an indexed triangle mesh thinned by vertex clustering on a uniform grid (csrc/mesh_simplify.hip), in the
 *   style of Rossignac-Borrel: all vertices of a grid cell become one, and a face survives if its corners fall into three
 *   different cells.  The cell's vertex is placed at the minimiser of the area^2-weighted plane quadrics of the faces around
 *   the cell's members (Lindstrom's out-of-core simplification), which keeps sharp edges and corners where a mean rounds
 *   them off; it falls back to the members' mean.  What section 'isosurface' extracts has the size its grid dictates, not the
 *   size binding, posing and drawing a sequence need (neuman_hip/mesh_simplify.py: simplify_mesh).
 *   tests/helpers/mesh_simplify_ref.py restates the rules in numpy.
 *   Every product, sum and quotient below is a float64 operation rounded on its own, in the association stated, no fused
 *   multiply-add; a float32 input converts exactly.
 *     Q1 mesh      as S1: faces [F,3] DEVICE int32 over V vertices, sizes passed as int64_t, 0 <= V < 2^31, 0 <= 3 F < 2^31.  A
 *                  face that names an index outside [0, V) is invalid: it is counted and never dereferenced.  With any invalid
 *                  face nm_mesh_simplify_count returns NM_ERR_ARG, nm_last_error() gives their number and the lowest invalid
 *                  face index, and nothing outside the caller's buffers has been written (vert_cluster is then unspecified).
 *                  A valid face is PROPER if its three indices are pairwise distinct.  verts [V,3] DEVICE float32; a vertex with
 *                  a coordinate that is not finite belongs to no cell: its label is -1 and no face naming it is a candidate.
 *     Q2 grid      HOST arguments: the origin lo[3] (float32, finite), the cell edge h (float32, finite, > 0), the dims
 *                  nx, ny, nz >= 1 with nx ny nz < 2^31.  The cell of a finite vertex per axis is
 *                  c_i = floor(((double)x_i - (double)lo_i) / (double)h) clamped to [0, n_i - 1] (a vertex outside the grid
 *                  belongs to the nearest border cell); its linear index is (c2 ny + c1) nx + c0.
 *     Q3 clusters  a face is a CANDIDATE iff it is valid and proper, its three vertices are finite and they lie in three
 *                  pairwise distinct cells.  A cell is USED iff some candidate names a vertex in it (the flag is set with a plain
 *                  store of 1 by every such candidate: the racing stores write the same value).  A cluster's id is the rank of
 *                  its cell among the used cells in ascending linear index, 0 .. K-1.  vert_cluster [V] int32 = the cluster id
 *                  of the vertex's cell, -1 for a vertex in an unused cell or one that is not finite.  So the output has no
 *                  vertex that no output face names, and a floater that collapses into one cell disappears whole.
 *     Q4 members   the members of cluster k are ALL finite vertices in its cell (named by a candidate or not), in ascending
 *                  vertex index; every sum below runs over them in that order, left to right, in one lane's loop.  The lists are
 *                  built count -> scan -> fill through an integer atomic cursor -> a sort of every cluster's segment in place by
 *                  its lane: insertion sort up to 32 entries, heap sort (O(k log k), no second buffer) beyond -- a coarse cell
 *                  holds hundreds of vertices.
 *     Q5 mean      per column of rows x [V,w] float32, 1 <= w <= 64:  s = 0;  s = s + x[v] over the members;  m = s / count;
 *                  the output is (float)m.  Positions under placement `mean`, colours and any other attribute go through this
 *                  one rule (nm_mesh_simplify_rows; the fill computes the positions itself).
 *     Q6 quadric   needs inc_off / inc of nm_mesh_adjacency for the INPUT mesh, trusted as far as section 'mesh smooth' trusts
 *                  them: an offset, a face index or a vertex index out of range is never followed, such an entry is skipped.
 *                  m = the float64 mean of Q5 of the positions, unrounded.  A (symmetric, six entries) and b start at zero.  For
 *                  each member v ascending and each face of v's list in list order, with its STORED corners (a, b, c):
 *                  u = x[b] - x[a], w = x[c] - x[a];  n = cross(u, w) as S5 writes it;  e = x[a] - m;
 *                  t = (n0 e0 + n1 e1) + n2 e2;  A_ij += n_i n_j for i <= j;  b_i += n_i t.  A face with j corners in the
 *                  cluster is met j times and counts j times.  Then reg = ((A00 + A11) + A22) 2^-10 is added to A00, A11, A22;
 *                  c00 = A11 A22 - A12 A12, c01 = A02 A12 - A01 A22, c02 = A01 A12 - A02 A11, c11 = A00 A22 - A02 A02,
 *                  c12 = A01 A02 - A00 A12, c22 = A00 A11 - A01 A01;  det = (A00 c00 + A01 c01) + A02 c02;
 *                  y_i = ((c_i0 b0 + c_i1 b1) + c_i2 b2) / det (c symmetric);  p = m + y.  The output is (float)p iff det is
 *                  finite and > 0, p is finite and lo_i + c_i h <= p_i <= lo_i + (c_i + 1) h on every axis (float64, c_i the
 *                  cluster's cell, each product rounded on its own); otherwise it is (float)m.  The regulariser makes a flat
 *                  or straight neighbourhood solvable and slides its vertex towards the mean along the flat directions; the
 *                  in-cell test keeps a runaway solution from leaving its cell.
 *     Q7 faces     a candidate's corners are mapped through vert_cluster and rotated cyclically so that the smallest id comes
 *                  first, which keeps the orientation.  A candidate f is dropped iff a candidate g < f has the same rotated
 *                  triple; two faces over the same three clusters with OPPOSITE orientation have different triples and both
 *                  stay (a sheet thinner than a cell keeps its two sides).  Kept faces come out in ascending input face index:
 *                  faces_out [F',3] int32, face_src [F'] int32 (nullable) = new -> old face index.  The duplicates are found
 *                  in an open-addressing table of 2 F slots of face indices: a free slot is claimed by compare-and-swap, a slot
 *                  of the same triple lowered by an integer atomicMin, so a triple's slot ends with its lowest face.
 *     Q8 calls     nm_mesh_simplify_count writes vert_cluster and reports {K, F', n_invalid, first_invalid} in ONE 32-byte
 *                  read-back (a stream synchronise) and nothing else.  nm_mesh_simplify_fill writes verts_out [K,3], faces_out
 *                  and face_src, placement 0 = mean or 1 = quadric; nm_mesh_simplify_rows averages rows [V,w] to out [K,w] by
 *                  Q5.  Neither reads anything back nor synchronises: the count leaves its totals in the workspace AND
 *                  remembers them on the host under the workspace's address (the 64 most recent workspaces, as C6), and both
 *                  refuse a V, F, cell count, n_clusters or n_faces_out other than those.  K = 0 launches nothing (then F' = 0
 *                  too), and an output of capacity 0 may be null.
 *     Q9 determinism  every output is a function of the inputs alone, byte-identical from run to run.  Under a permutation of
 *                  the rows of faces vert_cluster, K, the mean-placed vertices, the averaged rows and the SET of kept rotated
 *                  triples do not change; quadric placement may move in its last bits, because its sums follow the lists'
 *                  order, which is face order.  Only integer atomics whose result is order-independent are used (add,
 *                  compare-and-swap of a free slot, min); the one order-dependent intermediate, a member list's order after the
 *                  fill, is removed by the sort.  Nothing adds floats atomically.
 *   workspace: DEVICE, 16-byte aligned, nm_mesh_simplify_workspace_bytes(V, F, nx, ny, nz) bytes = 16 bytes per vertex (cell,
 *     cursor, offset, member) + 12 bytes per face (its rank, two table slots) + 4 bytes per cell (flag, then rank) + 16 bytes
 *     per 1024 vertices, per 1024 faces and per 1024 cells (the scans' spans) + 68 and padding below 128: linear in V, F and
 *     the cell count.  nm_mesh_simplify_count fills it; the other two entries take it with the same V, F and dims.
 *   NM_ERR_ARG (with the entry's name in nm_last_error()) before any device work for a null required pointer (an array of no
 *   rows may be null), V or 3 F negative or >= 2^31, a bad grid (lo or h not finite, h <= 0, a dim < 1, 2^31 cells or more),
 *   width outside 1..64, an unknown placement, quadric placement without inc_off / inc, a workspace that is misaligned or
 *   short, buffers that overlap (an output with another output, an input or the workspace), counts other than the count
 *   phase left.
 * ------------------------------------------------------------------------------------------- */
int64_t nm_mesh_simplify_workspace_bytes(int64_t V, int64_t F, int nx, int ny, int nz);
int nm_mesh_simplify_count(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo /* HOST [3] */, float h, int nx,
                           int ny, int nz, int32_t* vert_cluster, void* workspace, int64_t workspace_bytes, int64_t* n_clusters,
                           int64_t* n_faces_out, nm_stream_t stream);
int nm_mesh_simplify_fill(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* lo /* HOST [3] */, float h, int nx,
                          int ny, int nz, int placement, const int32_t* inc_off /* nullable unless quadric */,
                          const int32_t* inc /* nullable unless quadric */, const void* workspace, int64_t workspace_bytes, float* verts_out,
                          int32_t* faces_out, int32_t* face_src /* nullable */, int64_t n_clusters, int64_t n_faces_out,
                          nm_stream_t stream);
int nm_mesh_simplify_rows(const float* rows, int width, int64_t V, int64_t F, int nx, int ny, int nz, const void* workspace,
                          int64_t workspace_bytes, float* out, int64_t n_clusters, nm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SURVEY 8f-1 (first slice): device primitives of a training step of the background NeRF --
 *   reference trainers/vanilla_nerf_trainer.py:45-96 (forward with grad) + torch autograd's backward
 *   of models/vanilla.py:120-152 and utils/render_utils.py:69-105.  The layer loop is host code
 *   (neuman_hip/train.py), as the reference's is Python.
 *
 *   nm_gemm_f32: C[M,N] = op(A) op(B) in float32 on the f32 MFMA (true f32 products and accumulation);
 *   nm_gemm_bf16x3 below is the faster, slightly less exact form (NEUMAN_TRAIN_GEMM=bf16x3).
 *     a_kmajor = 0: A is an [M,K] row-major array (lda);  1: A is stored [K,M] (its transpose is multiplied)
 *     b_kmajor = 1: B is a [K,N] row-major array (ldb);   0: B is stored [N,K] (nn.Linear's weight layout)
 *     forward      Z  = A  W^T      (0, 0)        backward-data     dA = dZ W      (0, 1)
 *     backward-weights  dW = dZ^T A  (1, 1): split over K with a deterministic second pass when M*N is
 *     small and K large; needs nm_gemm_workspace_floats(M,N,K) floats of workspace and allows no flag
 *     but ACCUMULATE.
 *     flags: ACCUMULATE  C += ...;  BIAS  + bias[col];  RELU  max(.,0);  MASK  zero where mask[row,col] <= 0
 *     (applied in that order).  M, N, K, lda, ldb multiples of 4 (pad with zeros), A and B 16-byte aligned.
 *   nm_pe_encode: models/vanilla.py:60-92 stand-alone: x [n,dims] (dims 3, or 4 = point + time for the offset net,
 *     vanilla.py:180-188) -> out [n,ld], dims (1 + 2 n_freqs) features then
 *     zeros; table = the n_freqs bands (posenc) or the [3 n_freqs, 3] projection (rotate), device f32.
 *   nm_composite_backward: d loss / d raw [R,S,4] through raw2outputs given the gradients of rgb_map [R,3],
 *     acc_map [R], depth_map [R], weights [R,S] (each nullable = zero); disp_map's gradient is not supported.
 *     d_raw must be 8-byte aligned (refused otherwise: the records double as f64 scratch); with raw and d_raw 16-byte
 *     aligned and S <= 1024 a wave takes a ray, otherwise a lane does.
 * ------------------------------------------------------------------------------------------- */
#define NM_GEMM_ACCUMULATE 1
#define NM_GEMM_BIAS 2
#define NM_GEMM_RELU 4
#define NM_GEMM_MASK 8
#define NM_GEMM_COLSUM 16   /* also write the column sums of the stored output, per band of 64 rows, to workspace [ceil(M/64)][N]
                              (deterministic; the bias gradient of the layer below is the sum of the bands: nm_colsum on them).  Not
                              with a split-K product; needs the 16-byte aligned output layout (ldc % 4 == 0) */
int64_t nm_gemm_workspace_floats(int M, int N, int K);
int nm_gemm_f32(int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                int ldc, const float* bias, const float* mask, int ldmask, int flags, float* workspace,
                int64_t workspace_floats, nm_stream_t stream);
/* the same product with each float32 operand split into bf16 hi + lo and hi*hi + hi*lo + lo*hi accumulated in float32 on the
 * bf16 MFMA (2^-17 relative per product; what the rendering kernels call bf16x3).  Same arguments, same rules. */
int nm_gemm_bf16x3(int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                   int ldc, const float* bias, const float* mask, int ldmask, int flags, float* workspace,
                   int64_t workspace_floats, nm_stream_t stream);
/* and split into fp16 hi + lo on the fp16 MFMA (11 + 11 significand bits: float32 class, what the rendering kernels call fp16x3).
 * Operands are taken as they are (no scaling): parts below fp16's normal range lose at most 2^-25 absolutely, magnitudes beyond
 * 65504 saturate -- meant for the forward products (activations and weights of O(1)); gradients, whose magnitudes are unbounded
 * below, belong on nm_gemm_bf16x3 or nm_gemm_f32.  Same arguments, same rules. */
int nm_gemm_fp16x3(int a_kmajor, int b_kmajor, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                   int ldc, const float* bias, const float* mask, int ldmask, int flags, float* workspace,
                   int64_t workspace_floats, nm_stream_t stream);
int nm_pe_encode(const float* x, int64_t n, int dims, int kind, int n_freqs, const float* table, float* out, int ld,
                 nm_stream_t stream);
/* nm_pe_encode with the output as fp16 of 32 x value (an operand of nm_wgrad16; ld a multiple of 8, out 16-byte aligned).  ones_col >= 0 (a padding
 * column of the row): that column holds 1 (x 32) -- the product with it is the column sum of the other operand, i.e. the layer's bias gradient */
int nm_pe_encode16(const float* x, int64_t n, int dims, int kind, int n_freqs, const float* table, uint16_t* out, int ld, int ones_col,
                   nm_stream_t stream);
/* *out_max = max(*out_max, max |x[i]|), i < count: device scalar, updated atomically (zero it first); x 16-byte aligned */
int nm_absmax(const float* x, int64_t count, float* out_max, nm_stream_t stream);
/* Backward-weights from 16-bit operands, nprod <= 8 products of one n in ONE launch (+ one deterministic reduction):
 *     dW_p [p_cols][q_cols] = (1 / (32 s)) sum_n dz16_p[n][:]^T act16_p[n][:]          (s from *amax as in nm_mlp_backward_chain16)
 * dz16_p [n][p_cols] fp16 in k-slot order, p_cols = 256 (a trunk layer, feature_linear) or 128 (the views layer: dhv16); q_cols == 256: act16_p
 * [n][256] fp16 in k-slot order (nm_mlp_forward_save16's save_h16[l] / save_feat16); q_cols <= 64: act16_p [n][64] fp16 in natural order
 * (nm_pe_encode16, zero beyond the encoding).  dW_p in the natural [out][in] order of nn.Linear, row stride ldw[p] (so the hidden columns of the skip
 * layer land inside its [256][319] gradient).  One fp16 MFMA per product, 1 KB per sample and 256 x 256 product.  dz16 / act16 / dW / ldw: HOST arrays
 * of nprod entries. */
int64_t nm_wgrad16_workspace_floats(int nprod, int64_t n, int p_cols, int q_cols);
int nm_wgrad16(int nprod, int p_cols, int q_cols, const uint16_t* const* dz16, const uint16_t* const* act16, float* const* dW, const int* ldw,
               int64_t n, const float* amax, float* workspace, int64_t workspace_floats, nm_stream_t stream);
/* The 4-row heads of a step in one pass over d_raw [n][4], save_h16[7] and save_hv [n][128]: out[0..255] = alpha_linear's weight gradient
 * sum_n d_raw[n][3] H7[n][:], out[256..639] = rgb_linear's [3][128] = sum_n d_raw[n][k] hv[n][:], out[640..643] = the column sums of d_raw (rgb_linear's and
 * alpha_linear's bias gradients); *amax (nullable, a zeroed device scalar) = max |d_raw|: the scale source of nm_mlp_backward_net16 from the same read */
int64_t nm_wgrad_heads16_workspace_floats(int64_t n);
int nm_wgrad_heads16(const float* d_raw, const uint16_t* h16_7, const float* hv, int64_t n, float* out644, float* amax, float* workspace,
                     int64_t workspace_floats, nm_stream_t stream);
/* ... and of the plain-head net: out[0..1023] = output_linear's [4][256] = sum_n d_out[n][k] H7[n][:], out[1024..1027] = the column sums of d_out; amax as above */
int64_t nm_wgrad_out16_workspace_floats(int64_t n);
int nm_wgrad_out16(const float* d_out, const uint16_t* h16_7, int64_t n, float* out1028, float* amax, float* workspace, int64_t workspace_floats,
                   nm_stream_t stream);
/* alpha_linear's weight gradient out[256] = sum_n d_raw[n][3] H7[n][:] from save_h16[7] (x 32, k-slot order) */
int64_t nm_wgrad_alpha16_workspace_floats(int64_t n);
int nm_wgrad_alpha16(const float* d_raw, const uint16_t* h16, int64_t n, float* out, float* workspace, int64_t workspace_floats,
                     nm_stream_t stream);
/* out[W] = column sums of X [n,W] (row stride ld): the bias gradients; bands of 256 rows summed in order (deterministic) */
int64_t nm_colsum_workspace_floats(int64_t n, int W);
int nm_colsum(const float* X, int64_t n, int W, int ld, float* out, float* workspace, int64_t workspace_floats, nm_stream_t stream);
/* adjoint of nm_pe_encode: g [n,ld] = gradient of the encoded features -> dx [n,3] */
int nm_pe_backward(const float* x, int64_t n, int dims, int kind, int n_freqs, const float* table, const float* g, int ld,
                   float* dx, nm_stream_t stream);
int nm_composite_backward(const float* raw, const float* z_vals, const float* rays_d, int64_t R, int S, int white_bkg,
                          const float* g_rgb, const float* g_acc, const float* g_depth, const float* g_weights,
                          float* d_raw, nm_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * The scalar regularisers of the human trainer's loss (trainers/human_nerf_trainer.py:280-380) as single passes: the VALUE of a term and its
 * GRADIENT with respect to the network outputs it reads, in one kernel + one deterministic finalisation (csrc/loss.hip) -- torch's elementwise
 * algebra takes 10-25 launches per term and as many again in autograd's backward pass.  raw arrays are [n][4] = (r, g, b, sigma) rows, 16-byte
 * aligned; `loss` is one device float; workspace: nm_loss_workspace_doubles() doubles.
 *   nm_loss_bimodal: mean_i(-log(e^-|y_i| + e^-|1 - y_i|) + offset), y = clamp(x, 0, 1) when clamp01 (:368-379 with HARD_SURFACE_OFFSET); dx [n]
 *   nm_loss_pair_mse: scale * mse between two raw outputs: mode 0 over sigmoid(rgb) (the colour-range term, :280-290), mode 1 over tanh(relu(sigma))
 *                     (the symmetry term, :292-304); da_raw / db_raw [n][4]
 *   nm_loss_shape: the SMPL shape prior (:305-343): w_smpl * mean_{dist_h < 0}((1 - occ(pred))^2) + w_dummy * (mean_{dist_d < 0}((1 - occ(dummy))^2)
 *                  + mean_{dist_d > 0}(|occ(dummy) * (|dist_d| * outside_factor)^exponent|)), occ = 1 - exp(-relu(sigma)), empty selections count as 1;
 *                  nd = 0: the first term alone; norm3: three device floats, left holding weight / max(count, 1) of the three selections.
 * Gradients are autograd's on these formulas in float32, kinks included: relu passes nothing at sigma <= 0, clamp passes inside the closed interval,
 * abs has slope 0 at 0 -- so the outside term's gradient is exactly 0 wherever occ(dummy) * (|dist_d| * outside_factor)^exponent is 0 in float32
 * (sigma below about 3e-8).  A NaN density reaches the value of every term that reads it; a NaN distance is in no selection.  Columns a term does
 * not read get gradient 0 whatever they hold.  The result is the same bits on every run, whatever the workspace held before. */
int64_t nm_loss_workspace_doubles(void);
int nm_loss_bimodal(const float* x, int64_t n, int clamp01, float offset, float* loss, float* dx, double* workspace, nm_stream_t stream);
int nm_loss_pair_mse(int mode, const float* a_raw, const float* b_raw, int64_t n, float scale, float* loss, float* da_raw, float* db_raw,
                     double* workspace, nm_stream_t stream);
int nm_loss_shape(const float* pred_raw, const float* dist_h, int64_t nh, const float* dummy_raw, const float* dist_d, int64_t nd, float w_smpl,
                  float w_dummy, float outside_factor, float exponent, float* loss, float* d_pred_raw, float* d_dummy_raw, double* workspace,
                  float* norm3, nm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NEUMAN_HIP_H */
