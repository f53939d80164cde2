// Host-side launch interface of the hot-path kernels (internal to libmde_hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace mde {

typedef _Float16 h16;

// How the A operand (rows = output pixels / tokens, K contiguous) is formed.
enum AMode : int {
  A_DENSE = 0,    // A[m*lda + k], row-major f16
  A_CONV3 = 1,    // implicit im2col of a 3x3 pad-1 conv over an NHWC f16 map
  A_CONV3_UP = 2  // same, over bilinear(align_corners=True)-upsampled NHWC map
};

// What the epilogue does with acc[m][n] (fp32).
enum EMode : int {
  E_STORE = 0,   // out16[m*ldo+n] = act(acc + bias[n]) (+ res0 + res1)
  E_QKV = 1,     // scatter to head-major q (pre-scaled), k and transposed v
  E_RESID = 2,   // x32[m*ldo+n] += ls[n] * (acc + bias[n])
  E_PATCH = 3,   // x32[(b*T+tok0+p)*ldo+n] = acc + bias[n] + pos[p*ldo+n]
  E_CONVT = 4,   // ConvTranspose(k=s) pixel-shuffle store into NHWC f16
  E_HEAD = 5,    // relu(acc+bias(+pe)) . w2 + b2 -> sigmoid*max | relu | exp -> fp32 map
  E_PARTIAL = 6  // split-K slice s (blockIdx.y, XCD-remapped): x32[s*M*ldo + m*ldo + n] = acc (split paths only)
};

enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2 };

struct GemmParams {
  int amode = A_DENSE, emode = E_STORE;
  int M = 0, N = 0, K = 0;
  const h16* A = nullptr; int lda = 0;
  const h16* W = nullptr; int ldw = 0;  // weights [Npad][ldw], ldw % 64 == 0
  // conv geometry: source NHWC map [cb][ch][cw][cc]; output map [cb][oh][ow]
  int cb = 0, ch = 0, cw = 0, cc = 0;
  int uh = 0, uw = 0;  // virtual (upsampled) input size, A_CONV3_UP
  int oh = 0, ow = 0, stride = 1;
  int relu_in = 0;
  // epilogue
  const float* bias = nullptr; int act = ACT_NONE;
  h16* out16 = nullptr; int ldo = 0;
  const h16* res0 = nullptr; const h16* res1 = nullptr;
  // E_STORE residual options: res0_relu -> add relu(res0) (VGGT's in-place
  // ReLU residual units); res0_rows > 0 -> res0 is a table of res0_rows rows
  // repeated over m (row m % res0_rows: a per-image positional embedding)
  int res0_relu = 0; int res0_rows = 0;
  // res1_up (switch "resize_fold"): res1 is the bilinear (align_corners)
  // upsample of res1_up [cb][res1_uh][res1_uw][N] to the output map [cb][oh][ow]
  // (3x3 conv problems, ldo == N).  The direct conv reads it through that
  // upsample in its epilogue; every other path first writes the upsample into
  // res1 (launch_gemm), so res1 must be a buffer of the output's shape either way
  const h16* res1_up = nullptr; int res1_uh = 0, res1_uw = 0;
  // a 64 -> 64 1x1 conv folded behind a 3x3 conv (switch "outconv_fold": the
  // DPT fusion blocks' out_conv behind rcu2's second conv): pw_out [M][ldo] =
  // f16(pw_w . f16(conv epilogue) + pw_bias), pw_w = [64][pw_ldw] dense-GEMM
  // weights; out16 is then not written.  Only the persistent conv runs it --
  // set the fields when conv_folds_pointwise(p) says so, any other route
  // rejects them
  const h16* pw_w = nullptr; int pw_ldw = 0; const float* pw_bias = nullptr; h16* pw_out = nullptr;
  float* x32 = nullptr; const float* ls = nullptr;
  // f16 residual stream: when set, E_RESID / E_PATCH update / write xh
  // [m][ldo] f16 instead of x32 (DA-V2 engines with an f16 residual)
  h16* xh = nullptr;
  // E_QKV
  h16 *q = nullptr, *k = nullptr, *vt = nullptr;
  int T = 0, Tpad = 0, heads = 0; float qscale = 1.0f;
  // E_PATCH: patch rows start at token tok0 of each sequence (1 = after cls)
  const float* pos = nullptr; int npatch = 0; int tok0 = 1;
  // E_CONVT
  int s = 0, cout = 0, ih = 0, iw = 0;
  // E_HEAD: head_metric 0 ReLU, 1 max_depth * sigmoid, 2 exp; hpe (optional)
  // = f16 [hpe_pix][32] added to the hidden layer before its ReLU at pixel
  // m % hpe_pix (VGGT: the folded conv of the UV positional embedding)
  const float* w2 = nullptr; float b2 = 0.f; int head_metric = 1; float max_depth = 1.f;
  float* out32 = nullptr;
  const h16* hpe = nullptr; int hpe_pix = 0;
  // E_RESID split-K (small M, long K): splitk > 1 and partial = fp32
  // workspace [splitk][M][N]; the K range is cut into splitk slices whose
  // partial sums are added in slice order by a second kernel (deterministic)
  int splitk = 1; float* partial = nullptr;
  // E_STORE split-K (dense and 3x3-conv problems whose tile grid leaves most
  // of the chip idle: small batches, the DPT's 19^2 / 37^2 maps): when
  // partial_cap > 0 the launcher picks the slice count itself, bounded by
  // partial_cap fp32 elements of `partial`
  size_t partial_cap = 0;
  // Fused split-K (switch "splitk_fused"): with tile_cnt set (tile_cnt_cap
  // zero-initialised arrival counters, left zero by every launch) both split
  // paths above run as ONE launch whose last-arriving slice per tile adds the
  // slices' slots -- S x tiles x BM x BN fp32 in `partial`, at most slot_cap
  // elements -- in slice order and runs the epilogue; otherwise, or when the
  // slots do not fit, the slices + reduce-kernel form
  int* tile_cnt = nullptr; int tile_cnt_cap = 0; size_t slot_cap = 0;
  // LayerNorm folded across a GEMM boundary (DA-V2 f16-residual engines):
  //  * producer (E_RESID / E_PATCH over xh, and the split-K reduce): lnst_out
  //    = fp32 [lnst_ns][lnst_rows][2] -- per 32-column slice and token row
  //    (slice-major: a load of 16 consecutive rows is one 128-B line), the
  //    sum of the f16 values written and their squared deviations from the
  //    slice mean (M2; merged with Chan et al.'s formula, no E[x^2] - mean^2);
  //  * consumer (the next qkv / fc1, A = the raw f16 residual rows, W = W * gamma,
  //    bias = b + W beta): lnst_in = those partials, lnc1[n] = sum_k W[n][k]
  //    -> acc := rstd_m * (acc - mean_m * lnc1[n]) before the epilogue.
  float* lnst_out = nullptr;
  const float* lnst_in = nullptr; const float* lnc1 = nullptr;
  int lnst_ns = 0, lnst_rows = 0; float ln_eps = 1e-6f;
  // A_DENSE row skip (the DPT projects reading the residual stream through
  // the tap LayerNorm fold): a_tok > 1 -> GEMM row m reads A row (and LN
  // partial row) (m / (a_tok - 1)) * a_tok + 1 + m % (a_tok - 1), i.e. every
  // sequence's first (cls) row is skipped
  int a_tok = 0;
};

// Exact-fp32 encoder GEMM (fp32.hip; precision "fp32" engines): C = A W^T
// with fp32 A [M][lda] (lda % 4 == 0, 16-B aligned) and fp32 W [Npad][ldw]
// (ldw % 32 == 0, zero-padded), v_mfma_f32_16x16x4_f32.  emode:
//   E_STORE  out32 (fp32) or out16 (f16) [m*ldo + n] = act(acc + bias)
//   E_QKV    q (scaled by qscale) / k / v fp32 [B*heads][Tpad][64] rows
//   E_RESID  x32[m*ldo + n] += ls[n] * (acc + bias[n])
//   E_PATCH  x32[(b*T + 1 + p)*ldo + n] = acc + bias[n] + pos[p*ldo + n]
struct Gemm32Params {
  int emode = E_STORE;
  int amode = A_DENSE;  // A_DENSE or A_CONV3 (implicit im2col of a 3x3 pad-1 conv over an fp32 NHWC map)
  int M = 0, N = 0, K = 0;
  const float* A = nullptr; int lda = 0;
  const float* W = nullptr; int ldw = 0;
  const float* bias = nullptr; int act = ACT_NONE;
  float* out32 = nullptr; h16* out16 = nullptr; int ldo = 0;
  float* x32 = nullptr; const float* ls = nullptr;
  float *q = nullptr, *k = nullptr, *v = nullptr; int T = 0, Tpad = 0, heads = 0; float qscale = 1.f;
  const float* pos = nullptr; int npatch = 0;
  // A_CONV3: input map [cb][ch][cw][cc] (cc % 4 == 0), output [cb][oh][ow],
  // K = 9 cc in (ky, kx, c) order; relu_in: ReLU applied to the A operand
  int cb = 0, ch = 0, cw = 0, cc = 0, stride = 1, oh = 0, ow = 0, relu_in = 0;
  // E_STORE: out = act(acc + bias) + res0 + res1 (fp32 maps laid out like out32)
  const float* res0 = nullptr; const float* res1 = nullptr;
  // E_CONVT (ConvTranspose k = s): rows = input pixels [cb][ih][iw], column
  // n = (dy s + dx) cout + co -> out32 pixel (s iy + dy, s ix + dx), channel co
  // (stride ldo), + bias[co]
  int s = 0, cout = 0, ih = 0, iw = 0;
};
hipError_t launch_gemm32(const Gemm32Params& p, hipStream_t st);
// fp32 NHWC bilinear resize, align_corners=True ([B][ih][iw][C] -> [B][oh][ow][C], C % 4 == 0)
hipError_t launch_resize32(const float* in, float* out, int B, int ih, int iw, int C, int oh, int ow, hipStream_t st);
// DPT head tail over an fp32 hidden map hid [M][32] (already ReLU'd): out[m] =
// act(sum_c w2[c] hid[m][c] + b2), act = ReLU (relative), sigmoid * max_depth
// (metric, 1), exp (2) -- output_conv2's last 1x1 conv and activation
hipError_t launch_head32(const float* hid, const float* w2, float b2, int M, int metric, float max_depth, float* out,
                         hipStream_t st);
// fp32 attention over q (pre-scaled by dh^-0.5 * log2 e) / k / v fp32
// [B*H][Tpad][64] rows -> o fp32 [B*T][ldo], head h in columns 64h .. 64h+63
hipError_t launch_attention32(const float* q, const float* k, const float* v, float* o, int B, int H, int T,
                              int Tpad, int ldo, hipStream_t st);
// which of its two shapes the calling thread's last launch_attention32 launched
// (fp32.hip decides once and launches from it; mde_debug_last_attention32_route)
struct Attn32Route {
  int key_groups = 0;  // 4: attn32_kernel<4>, one 32-query block per workgroup; 1: attn32_kernel<1>,
                       // four blocks over all keys; 0: nothing launched (yet, empty or rejected)
  int nqb = 0;         // query blocks per (sequence, head)
};
const Attn32Route& attention32_last_route();


// x32[m*ldo+n] += ls[n] * (sum_{s<S} P[s][m][n] + bias[n]), slices summed in
// order (elementwise.hip): the second half of the E_RESID split-K path
hipError_t launch_splitk_resid(const float* P, int S, int M, int N, const float* bias, const float* ls, float* x32,
                               h16* xh, int ldo, hipStream_t st, float* lnst_out = nullptr);  // lnst_out rows = M

// out16 = E_STORE epilogue of (sum_{s<S} P[s][m][n]) (elementwise.hip): the
// second half of the E_STORE split-K path
hipError_t launch_splitk_store(const float* P, int S, const GemmParams& p, hipStream_t st);

// routes p (gemm_route.h: validation and the choice of kernel) and launches it
hipError_t launch_gemm(const GemmParams& p, hipStream_t st);

// Direct 3x3 conv with an LDS halo patch (conv.hip); launch_gemm routes
// A_CONV3 / A_CONV3_UP problems here when conv_direct_supported().
bool conv_direct_supported(const GemmParams& p);
// the direct conv takes p's res1 through GemmParams::res1_up (conv.hip)
bool conv3_takes_res1_up(const GemmParams& p);
hipError_t launch_conv3(const GemmParams& p, hipStream_t st);
// the kernel launch_conv3 launches for p (conv.hip; policy only, no device
// call): launch_conv3 acts on it and gemm_route records it (GemmRoute::conv)
enum ConvKernel : int {
  CONV_K_NONE = 0,        // not a direct-conv route
  CONV_K_CONV3,           // conv3_kernel on the map itself
  CONV_K_CONV3_UP,        // conv3_kernel, four-tap upsampling loader (A_CONV3_UP)
  CONV_K_UPCONV,          // upconv_kernel, one tile per workgroup
  CONV_K_UPCONV_PERSIST,  // upconv_kernel, persistent grid
  CONV_K_CONV64P          // the persistent 64-channel conv
};
int conv3_kernel_choice(const GemmParams& p);
// the persistent 64-channel conv (conv.hip) takes p and would run a following
// 1x1 (GemmParams::pw_*) on its tiles
bool conv64p_folds_pointwise(const GemmParams& p);
// launch_gemm routes p to that kernel with the fold available (gemm.hip): the
// caller may then attach the 1x1 (pw_*) instead of launching it
bool conv_folds_pointwise(const GemmParams& p);

// A-stationary panel GEMM (gemm_panel.hip) for K = 384 token-major E_STORE /
// E_QKV problems at large batch (the ViT-S fc1 and qkv); launch_gemm routes there when
// panel_gemm_eligible() (switch "panel").
bool panel_gemm_eligible(const GemmParams& p);
// compute units of the current device (cached)
int cu_count();
hipError_t launch_panel_gemm(const GemmParams& p, hipStream_t st);

// 256x256 phase-pipelined dense GEMM (gemm256.hip) for large token-major
// problems; launch_gemm routes there when gemm256_eligible() (switch "gemm256").
bool gemm256_eligible(const GemmParams& p);
hipError_t launch_gemm256(const GemmParams& p, hipStream_t st);

// ws (optional, attention_split_ws_bytes): fp32 workspace for the split-KV
// path the launcher takes on grids too small to fill the chip (batch 1)
// cfg (optional) = "<waves>[s<split>][g<groups>][r<ring>][q2]" ("8", "4s2",
// "4g2", ...): forces a workgroup shape / split for tests and tuning; nullptr
// or "" = the launch policy.
hipError_t launch_attention(const h16* q, const h16* k, const h16* vt, h16* o, int B, int H, int T,
                            int Tpad, int ldo, hipStream_t st, float* ws = nullptr, size_t ws_bytes = 0,
                            const char* cfg = nullptr);
size_t attention_split_ws_bytes(int B, int H, int T);
// What launch_attention launches for a problem (attention.hip attention_route
// decides: policy or cfg, and every fall-back -- key groups that do not fit
// the key tiles, a split that collapses or whose workspace is too small;
// launch_attention launches from the decision and keeps a copy per thread for
// the tests, mde_debug_last_attention_route in include/mde.h).
// A rejected call (hipErrorInvalidValue) resets the record like an empty one.
enum AttnKernel : int {
  ATTN_K_NONE = 0,  // nothing launched yet on this thread, or an empty problem
  ATTN_K_MFMA32,    // attn_fwd_kernel (v_mfma_f32_32x32x16_f16)
  ATTN_K_MFMA16     // attn16_fwd_kernel (v_mfma_f32_16x16x32_f16)
};
struct AttnRoute {
  int kernel = ATTN_K_NONE;
  int nw = 0;      // waves per workgroup
  int groups = 1;  // key groups inside the workgroup (1 = none)
  int split = 1;   // key splits over gridDim.z actually launched (1 = none: no combine launch)
  int tiles = 0;   // key tiles per split (split > 1)
  int ring = 2;    // K / V^T ring depth
  int qs = 1;      // 32-query sub-tiles per wave
  int tail = 0;    // MFMA16: the attn_tail switch handed to the kernel; else 0
  int nqb = 0;     // query blocks per (sequence, head): gridDim.x
  int nkt = 0;     // 64-key tiles
};
const AttnRoute& attention_last_route();

// x (fp32) or xh (f16) residual rows -> LayerNorm -> f16 y
hipError_t launch_layernorm(const float* x, h16* y, const float* g, const float* b, int rows, int D,
                            float eps, int T, int skip_cls, hipStream_t st, const h16* xh = nullptr);

// P32 (exact-fp32 engines): the patch rows as fp32 into P32 instead of f16 into P
hipError_t launch_patch_prep_u8(const unsigned char* img, h16* P, float* X, const float* cls_pos, int B, int H, int W,
                                int ph, int pw, int T, int D, float scale, const float* mean3, const float* std3,
                                hipStream_t st, h16* Xh = nullptr, float* lnst = nullptr,
                                const float* cls_st = nullptr, float* P32 = nullptr);
hipError_t launch_depth_postprocess(const float* in, int B, int ih, int iw, float* out, int oh, int ow, float lo,
                                    float hi, hipStream_t st);
// preprocess.hip: cv2's uint8 INTER_LINEAR stretch of [B][sh][pitch] 3-channel rows; lut == nullptr:
// dst uint8 NHWC [B][oh][ow][3]; else dst float NCHW [B][3][oh][ow] = lut[c][value] (lut float[3][256])
hipError_t launch_resize_u8(const unsigned char* src, int B, int sh, int sw, int pitch, int swap_rb, const float* lut,
                            void* dst, int oh, int ow, hipStream_t st);
// depth_pro_photo.hip: Depth Pro's pre-process (uint8 [B][sh][pitch] photo -> lut[u], torch bilinear
// align_corners=False -> float NCHW [B][3][oh][ow]; lut float[256]) and post-process (inverse depth
// [B][ih][iw] * ow / f, the same bilinear to [B][oh][ow], 1 / clamp(., 1e-4, 1e4); f from fov_deg [B]
// when non-null, else f_px; f_px_out [B] optional).  No argument checks here: the ABI wrappers in
// ops_abi.hip hold the only copy of the limits
hipError_t launch_dp_preprocess(const unsigned char* src, int B, int sh, int sw, int pitch, int swap_rb,
                                const float* lut, float* dst, int oh, int ow, hipStream_t st);
hipError_t launch_dp_postprocess(const float* inv, int B, int ih, int iw, const float* fov_deg, float f_px,
                                 float* f_px_out, float* out, int oh, int ow, hipStream_t st);
// The cloud source of launch_point_cloud, launch_depth_mesh and launch_cloud_view: fp32 depth [B][h][w]
// sampled at every step-th pixel on both axes, an optional photo [B][h][pitch] (3 bytes per pixel, its
// channels reversed when swap_rb) and the pinhole camera -- fx = fy = f_px_dev[b] when f_px_dev is given,
// else the host's fx, fy; cx, cy.  The fields are the mde_op_* arguments of the same names.
struct CloudSource {
  const float* depth;
  int B, h, w, step;
  const unsigned char* photo;
  int pitch, swap_rb;
  const float* f_px_dev;
  float fx, fy, cx, cy;
};
// point_cloud.hip: pinhole unprojection of fp32 depth [B][h][w] (every step-th pixel on both axes) into
// packed PLY vertex records (float x, y, z [+ uchar r, g, b from photo [B][h][pitch]]), organized or
// compacted to z in [z_lo, z_hi]; counts int[B]; ws = point_cloud_ws_bytes() of scratch (compact only).
// Enqueues one (organized) or three (compact) kernels, nothing else.  No argument checks here: the ABI
// wrapper in ops_abi.hip holds the only copy of the limits
size_t point_cloud_ws_bytes(int B, int h, int w, int step);
hipError_t launch_point_cloud(const CloudSource& src, int compact, float z_lo, float z_hi, void* records, int* counts,
                              void* ws, hipStream_t st);
// depth_mesh.hip: the same grid, camera and vertex records as launch_point_cloud, after the depth-edge
// filter (include/mde.h, mde_op_depth_mesh): the vertices the kept quads use (faces != 0) or the clean
// samples (faces == 0), compacted, and two 13-byte PLY face entries per kept quad; vertex_counts, face_counts
// int[B]; ws = depth_mesh_ws_bytes() of 4-byte aligned scratch.  Enqueues six kernels (four without
// faces), nothing else.  No argument checks here: the ABI wrapper in ops_abi.hip holds the only copy of
// the limits
size_t depth_mesh_ws_bytes(int B, int h, int w, int step);
hipError_t launch_depth_mesh(const CloudSource& src, float z_lo, float z_hi, float edge_rtol, float edge_atol,
                             int faces, void* vertices, int* vertex_counts, void* face_records, int* face_counts,
                             void* ws, hipStream_t st);
// depth_eval.hip: fp32 prediction and ground truth [B][h][w] and a uint8 mask -> double out[B][16]
// (include/mde.h, mde_op_depth_eval: fit status and parameters, the metrics, the orientation);
// ws = depth_eval_ws_bytes() of 8-byte aligned scratch.  Enqueues four kernels, nothing else.  No
// argument checks here: the ABI wrapper in ops_abi.hip holds the only copy of the limits
size_t depth_eval_ws_bytes(int B, int h, int w);
hipError_t launch_depth_eval(const float* pred, const float* gt, const unsigned char* mask, int B, int h, int w,
                             int policy, int pred_is_inverse, int fit_finite_only, float max_depth, double* out,
                             void* ws, hipStream_t st);
// depth_colorize.hip: fp32 map [B][h][w] -> uint8 picture [B][h][w][3] through a 257-entry colour
// table (include/mde.h, mde_op_depth_colorize: inverse_auto, minmax_u8 or a fixed axis); range_out
// float[B][2] optional; ws = depth_colorize_ws_bytes() of 4-byte aligned scratch (modes 0 and 1).
// Enqueues at most four kernels, nothing else.  No argument checks here: the ABI wrapper in
// ops_abi.hip holds the only copy of the limits
size_t depth_colorize_ws_bytes(int B, int h, int w);
hipError_t launch_depth_colorize(const float* map, int B, int h, int w, int mode, int map_is_inverse, double denom_eps,
                                 double vmin, double vmax, const unsigned char* lut257x3, int swap_rb,
                                 unsigned char* out, float* range_out, void* ws, hipStream_t st);
// the same colour pass on an axis read from device memory (include/mde.h, mde_op_depth_colorize_ranged):
// image b is drawn on range[b * range_stride], range[b * range_stride + 1].  One or two kernels
hipError_t launch_depth_colorize_ranged(const float* map, int B, int h, int w, int positive_only, int reciprocal,
                                        const double* range, int range_stride, const unsigned char* lut257x3,
                                        int swap_rb, unsigned char* out, hipStream_t st);
// depth_quantiles.hip: np.percentile (method linear) of the valid pixels of fp32 maps [B][h][w] by radix
// select -> double out[rows][8] (include/mde.h, mde_op_depth_quantiles: counts, min, max, up to three
// quantiles, the display range); q_percent is read on the host; ws = depth_quantiles_ws_bytes() of
// 8-byte aligned scratch.  Enqueues eleven kernels, nothing else.  No argument checks
// here: the ABI wrapper in ops_abi.hip holds the only copy of the limits
size_t depth_quantiles_ws_bytes(int B, int h, int w);
hipError_t launch_depth_quantiles(const float* map, int B, int h, int w, int positive_only, int reciprocal,
                                  int pooled, int sample_cap, const double* q_percent, int nq, double* out, void* ws,
                                  hipStream_t st);
// cloud_view.hip: an orthographic, z-buffered picture uint8 [B][out_h][out_w][3] of the cloud that
// launch_point_cloud would pack (the same CloudSource), seen from the angles whose
// cosines and sines the caller gives (include/mde.h, mde_op_cloud_view); view_out double[B][8]: the
// counts, the centre, the span and the scale; view_in non-null: a fixed camera, no selection.  ws =
// cloud_view_ws_bytes() of 8-byte aligned scratch.  Enqueues kernels (and launch_depth_quantiles, 1 + B
// times, without view_in), nothing else.  No argument checks here: the ABI wrapper in ops_abi.hip holds
// the only copy of the limits
size_t cloud_view_ws_bytes(int B, int h, int w, int step, int out_h, int out_w);
hipError_t launch_cloud_view(const CloudSource& src, double cos_a, double sin_a, double cos_e, double sin_e,
                             const double* view_in, const int bg_rgb[3], int out_swap_rb, unsigned char* out,
                             int out_h, int out_w, double* view_out, void* ws, hipStream_t st);
// preprocess_cubic.hip: cv2's uint8 INTER_CUBIC of [B][sh][pitch] 3-channel rows seen through a virtual
// constant border of pad_* pixels (include/mde.h, mde_op_resize_cubic_u8; pad_rgb in output channel
// order); lut == nullptr: dst uint8 NHWC [B][oh][ow][3]; else dst float NCHW [B][3][oh][ow] =
// lut[c][value] (lut float[3][256]).  launch_crop_f32: the window [y0, y0 + ch) x [x0, x0 + cw) of fp32
// maps [B][h][w] -> [B][ch][cw].  One kernel each.  No argument checks here: the ABI wrappers in
// ops_abi.hip hold the only copy of the limits
hipError_t launch_resize_cubic_u8(const unsigned char* src, int B, int sh, int sw, int pitch, int swap_rb,
                                  int pad_top, int pad_bottom, int pad_left, int pad_right, const int pad_rgb[3],
                                  const float* lut, void* dst, int oh, int ow, hipStream_t st);
hipError_t launch_crop_f32(const float* src, int B, int h, int w, int y0, int x0, int ch, int cw, float* dst,
                           hipStream_t st);
// preprocess_cubic.hip: cv2's scalar float INTER_CUBIC of the photo / 255 in T = float (wide == 0) or
// double, then (x - mean) / std in float64, rounded once to float32 NCHW [B][3][oh][ow] (include/mde.h,
// mde_op_resize_cubic_f_norm); lut: device T[256], mean / stdv in output channel order.  One kernel
hipError_t launch_resize_cubic_f_norm(const unsigned char* src, int B, int sh, int sw, int pitch, int swap_rb,
                                      int wide, const void* lut, const double mean[3], const double stdv[3],
                                      float* dst, int oh, int ow, hipStream_t st);
hipError_t launch_patch_prep(const float* img, h16* P, float* X, const float* cls_pos, int B, int H,
                             int W, int ph, int pw, int T, int D, hipStream_t st, h16* Xh = nullptr,
                             float* lnst = nullptr, const float* cls_st = nullptr, float* P32 = nullptr);
// fp32 rows -> LayerNorm -> fp32 rows (exact-fp32 engines)
// (T, skip_cls = 1: the cls row of every T-row sequence dropped, the patch
// rows written as the [B*(T-1)][D] NHWC token map -- the taps' final norm)
hipError_t launch_layernorm32(const float* x, float* y, const float* g, const float* b, int rows, int D, float eps,
                              hipStream_t st, int T = 1, int skip_cls = 0);

hipError_t launch_resize(const h16* in, h16* out, int B, int ih, int iw, int C, int oh, int ow,
                         hipStream_t st);

// ---- Depth Pro (depth_pro_ops.hip) ----
// Pyramid levels of the patch encoder input, high-res first: sequences
// l in [first[i], first[i+1]) are the n[i] x n[i] patches of level i
// (row-major), taken with `stride` from the image downsampled by f[i].
struct DpPyramid {
  int nlev = 0, nseq = 0;  // nseq = patches per image
  int first[3] = {0, 0, 0}, n[3] = {0, 0, 0}, stride[3] = {0, 0, 0}, f[3] = {1, 1, 1};
};
// One merged level map: patches (base + r*n + c) of every image, G x G
// tokens each (row 0 of each sequence = cls, dropped), interior edges
// trimmed by pad -> [B][n G - 2 (n-1) pad]^2 NHWC.
struct DpMerge {
  int B = 0, n = 1, G = 0, pad = 0, base = 0, T = 0;
};
hipError_t launch_dp_patch_prep(const float* img, h16* P, int B, int S, int G, const DpPyramid& pyr,
                                hipStream_t st);
hipError_t launch_cls_rows(float* X, const float* cls, int nseq, int T, int D, hipStream_t st);
// g == nullptr: plain fp32 -> f16 copy (raw hook features); else LayerNorm(g, b)
hipError_t launch_merge_tokens(const float* x, h16* y, const float* g, const float* b, int D, const DpMerge& m,
                               float eps, hipStream_t st);
hipError_t launch_fov_final(const h16* in, const float* w, float bias, int K, int B, float* out, hipStream_t st);

// ---- VGGT (vggt_ops.hip) ----
// Token geometry of the q/k rows one qk_norm_rope launch covers: T tokens per
// sequence (rows padded to Tpad), P tokens per frame (T = S * P for global
// attention), the first npre of each frame special (RoPE position (0, 0)),
// the rest a grid gw wide at positions (row + 1, col + 1).
struct RopeGeom {
  int T = 0, Tpad = 0, P = 1, npre = 0, gw = 1;
  float qscale = 1.f, eps = 1e-5f;
};
// special-token rows [0, npre) of every sequence from pre[sets][npre][D]
// (sets 2: set 0 for the first frame of each batch item, 1 for the others)
hipError_t launch_prefix_rows(float* X, const float* pre, int nseq, int T, int npre, int D, int frames, int sets,
                              hipStream_t st);
hipError_t launch_rows_layernorm(float* X, const float* g, const float* b, int nseq, int T, int row0, int D, float eps,
                                 hipStream_t st);
hipError_t launch_qk_norm_rope(h16* q, h16* k, const float* qg, const float* qb, const float* kg, const float* kb,
                               const float* rope_cos, const float* rope_sin, int BH, const RopeGeom& geo,
                               hipStream_t st);
hipError_t launch_tap_concat_ln(const float* xa, const float* xb, h16* y, const float* g, const float* b, int nseq,
                                int T, int npre, int D, float eps, hipStream_t st);

// ---- a run-time value as a template argument ----
// f(std::integral_constant<int, x>) for x in [0, N); any other x is an invalid argument
template <int N, class F>
hipError_t with_constant(int x, F&& f) {
  if constexpr (N == 0) return hipErrorInvalidValue;
  else return x == N - 1 ? f(std::integral_constant<int, N - 1>{}) : with_constant<N - 1>(x, f);
}
// The wave-per-row kernels give each lane PER = D / 64 columns of a row:
// f(std::integral_constant<int, PER>) for the PER of the launcher's list PERS
// with D == 64 PER; any other width is an invalid argument (nothing launched)
template <int PER, int... PERS, class F>
hipError_t with_row_per(int D, F&& f) {
  if (D == 64 * PER) return f(std::integral_constant<int, PER>{});
  if constexpr (sizeof...(PERS) > 0) return with_row_per<PERS...>(D, f);
  else return hipErrorInvalidValue;
}

}  // namespace mde
