// libmde_hip op-level C ABI (include/mde.h mde_op_*): one kernel launch per
// entry point, for the parity tests and tools.  Host code only: argument
// validation here, launch parameters through the builders the engines use
// (gemm_params.h), kernels and dispatch policy in the launchers.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "engine_internal.h"
#include "gemm_route.h"

using namespace mde;

extern "C" {

// ---- kernel-level entry points ------------------------------------------------
// a launcher's result as the ABI status: hipErrorInvalidValue is the
// launchers' "bad shape / argument", anything else a HIP failure
static int op_status(hipError_t e, const char* what) {
  if (e == hipErrorInvalidValue) return fail(MDE_ERR_ARG, std::string(what) + ": invalid shape/argument");
  if (e != hipSuccess) return hip_fail(e, what);
  return MDE_OK;
}
#define OP_RET(call, what) return op_status((call), what)

int mde_debug_last_gemm_route(char* buf, size_t n) {
  static const char* const kKind[] = {"none", "tile", "split_store", "split_resid", "conv_direct", "panel", "gemm256"};
  static const char* const kConv[] = {"none", "conv3", "conv3_up", "upconv", "upconv_persist", "conv64p"};
  const GemmRoute& r = gemm_last_route();
  if (!buf) return fail(MDE_ERR_ARG, "mde_debug_last_gemm_route: null buffer");
  int len;
  if (r.kind == ROUTE_TILE || r.kind == ROUTE_SPLIT_STORE || r.kind == ROUTE_SPLIT_RESID)
    len = snprintf(buf, n, "kind=%s bm=%d bn=%d wm=%d wn=%d bk=%d stages=%d slices=%d fused=%d resize_first=%d",
                   kKind[r.kind], r.bm, r.bn, r.wm, r.wn, r.bk, r.stages, r.slices, r.fused, r.resize_first);
  else if (r.kind == ROUTE_CONV_DIRECT)
    len = snprintf(buf, n, "kind=%s conv=%s resize_first=%d", kKind[r.kind],
                   kConv[r.conv >= 0 && r.conv <= CONV_K_CONV64P ? r.conv : 0], r.resize_first);
  else
    len = snprintf(buf, n, "kind=%s", kKind[r.kind >= 0 && r.kind <= ROUTE_GEMM256 ? r.kind : 0]);
  if (len < 0 || (size_t)len >= n) return fail(MDE_ERR_ARG, "mde_debug_last_gemm_route: buffer too small");
  return MDE_OK;
}

int mde_debug_last_attention_route(char* buf, size_t n) {
  static const char* const kKernel[] = {"none", "mfma32", "mfma16"};
  const AttnRoute& r = attention_last_route();
  if (!buf) return fail(MDE_ERR_ARG, "mde_debug_last_attention_route: null buffer");
  int len;
  if (r.kernel == ATTN_K_MFMA32 || r.kernel == ATTN_K_MFMA16)
    len = snprintf(buf, n, "kernel=%s nw=%d groups=%d split=%d tiles=%d ring=%d qs=%d tail=%d nqb=%d nkt=%d",
                   kKernel[r.kernel], r.nw, r.groups, r.split, r.tiles, r.ring, r.qs, r.tail, r.nqb, r.nkt);
  else
    len = snprintf(buf, n, "kernel=%s", kKernel[0]);
  if (len < 0 || (size_t)len >= n) return fail(MDE_ERR_ARG, "mde_debug_last_attention_route: buffer too small");
  return MDE_OK;
}

int mde_debug_last_attention32_route(char* buf, size_t n) {
  const Attn32Route& r = attention32_last_route();
  if (!buf) return fail(MDE_ERR_ARG, "mde_debug_last_attention32_route: null buffer");
  const int len = r.key_groups ? snprintf(buf, n, "kernel=fp32 key_groups=%d nqb=%d", r.key_groups, r.nqb)
                               : snprintf(buf, n, "kernel=none");
  if (len < 0 || (size_t)len >= n) return fail(MDE_ERR_ARG, "mde_debug_last_attention32_route: buffer too small");
  return MDE_OK;
}

int mde_op_patch_prep_u8(const unsigned char* img, int batch, int h, int w, float scale, const float* mean3,
                         const float* std3, void* patches, void* st) {
  if (!img || !mean3 || !std3 || !patches || batch < 1 || h % 14 || w % 14 || h < 14 || w < 14)
    return fail(MDE_ERR_ARG, "mde_op_patch_prep_u8: bad argument (h, w multiples of 14)");
  OP_RET(launch_patch_prep_u8(img, (h16*)patches, nullptr, nullptr, batch, h, w, h / 14, w / 14, 1, 0, scale, mean3,
                              std3, (hipStream_t)st),
         "patch_prep_u8");
}

int mde_op_depth_postprocess(const float* depth, int batch, int ih, int iw, float* out, int oh, int ow, float lo,
                             float hi, void* st) {
  if (!depth || !out || batch < 1 || ih < 1 || iw < 1 || oh < 1 || ow < 1)
    return fail(MDE_ERR_ARG, "mde_op_depth_postprocess: bad argument");
  OP_RET(launch_depth_postprocess(depth, batch, ih, iw, out, oh, ow, lo, hi, (hipStream_t)st), "depth_postprocess");
}

namespace {
const char* resize_u8_arg_error(const void* src, const void* dst, int batch, int sh, int sw, int pitch, int oh,
                                int ow) {
  if (!src || !dst) return "null pointer";
  if (batch < 1 || sh < 1 || sw < 1 || oh < 1 || ow < 1) return "batch and sizes must be positive";
  if (pitch < 3 * (long long)sw) return "pitch < 3 * sw";
  return nullptr;
}
}  // namespace

int mde_op_resize_u8(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                     unsigned char* dst_u8, int oh, int ow, void* st) {
  if (const char* why = resize_u8_arg_error(src, dst_u8, batch, sh, sw, pitch, oh, ow))
    return fail(MDE_ERR_ARG, std::string("mde_op_resize_u8: ") + why);
  OP_RET(launch_resize_u8(src, batch, sh, sw, pitch, swap_rb, nullptr, dst_u8, oh, ow, (hipStream_t)st),
         "mde_op_resize_u8");
}

int mde_op_resize_u8_norm(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                          const float* lut3x256, float* dst_f32_nchw, int oh, int ow, void* st) {
  const char* why = resize_u8_arg_error(src, dst_f32_nchw, batch, sh, sw, pitch, oh, ow);
  if (!why && !lut3x256) why = "null pointer";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_resize_u8_norm: ") + why);
  OP_RET(launch_resize_u8(src, batch, sh, sw, pitch, swap_rb, lut3x256, dst_f32_nchw, oh, ow, (hipStream_t)st),
         "mde_op_resize_u8_norm");
}

namespace {
// the Depth Pro photo ops index a plane with an int and put the batch on grid.y
const char* dp_photo_geometry_error(int batch, int sh, int sw, int oh, int ow) {
  if (batch < 1 || sh < 1 || sw < 1 || oh < 1 || ow < 1) return "batch and sizes must be positive";
  const long long lim = 0x7fffffffLL - 256;
  if ((long long)sh * sw >= lim || (long long)oh * ow >= lim) return "a plane of 2^31 - 256 elements or more";
  if (batch > 65535) return "batch > 65535";
  return nullptr;
}
}  // namespace

int mde_op_dp_preprocess(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                         const float* lut256, float* dst_f32_nchw, int oh, int ow, void* st) {
  const char* why = dp_photo_geometry_error(batch, sh, sw, oh, ow);
  if (!src || !lut256 || !dst_f32_nchw) why = "null pointer";
  if (!why && pitch < 3 * (long long)sw) why = "pitch < 3 * sw";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_dp_preprocess: ") + why);
  OP_RET(launch_dp_preprocess(src, batch, sh, sw, pitch, swap_rb, lut256, dst_f32_nchw, oh, ow, (hipStream_t)st),
         "mde_op_dp_preprocess");
}

int mde_op_dp_postprocess(const float* inv, int batch, int ih, int iw, const float* fov_deg, float f_px,
                          float* f_px_out, float* depth, int oh, int ow, void* st) {
  const char* why = (!inv || !depth) ? "null pointer" : dp_photo_geometry_error(batch, ih, iw, oh, ow);
  if (!why && !fov_deg && !(f_px > 0.f)) why = "fov_deg is null and f_px <= 0";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_dp_postprocess: ") + why);
  OP_RET(launch_dp_postprocess(inv, batch, ih, iw, fov_deg, f_px, f_px_out, depth, oh, ow, (hipStream_t)st),
         "mde_op_dp_postprocess");
}

namespace {
// sampled grid of the point-cloud op; returns why it is unusable, else nullptr and the grid's size
const char* point_cloud_geometry_error(int batch, int h, int w, int step, long long* plane) {
  if (batch < 1 || h < 1 || w < 1) return "batch and sizes must be positive";
  if (step < 1) return "step must be positive";
  *plane = (long long)((h + (long long)step - 1) / step) * ((w + (long long)step - 1) / step);
  if ((long long)h * w >= 0x7fffffffLL - 256 || *plane >= 0x7fffffffLL - 256)
    return "a plane of 2^31 - 256 elements or more";
  if (batch > 65535) return "batch > 65535";
  return nullptr;
}

// why a cloud source is unusable, in the order the three ops report it, else nullptr and the sampled
// plane's size: a null depth, the geometry, the photo's pitch, the focal length, the centre
const char* cloud_source_error(const CloudSource& s, long long* plane) {
  if (!s.depth) return "null pointer";
  if (const char* why = point_cloud_geometry_error(s.B, s.h, s.w, s.step, plane)) return why;
  if (s.photo && s.pitch < 3 * (long long)s.w) return "pitch < 3 * w";
  if (!s.f_px_dev && !(s.fx > 0.f && s.fy > 0.f)) return "f_px_dev is null and fx <= 0 or fy <= 0";
  if (!(s.cx == s.cx && s.cy == s.cy)) return "cx or cy is NaN";
  return nullptr;
}

// batch <= 65535, plane < 2^31, a record of 15 bytes at most: no overflow in 64 bits
unsigned long long vertex_bytes(const CloudSource& s, long long plane) {
  return (unsigned long long)s.B * plane * (s.photo ? 15 : 12);
}
}  // namespace

size_t mde_op_point_cloud_ws_bytes(int batch, int h, int w, int step) {
  long long plane = 0;
  if (point_cloud_geometry_error(batch, h, w, step, &plane)) return 0;
  return point_cloud_ws_bytes(batch, h, w, step);
}

int mde_op_point_cloud(const float* depth, int batch, int h, int w, int step, const unsigned char* photo, int pitch,
                       int swap_rb, const float* f_px_dev, float fx, float fy, float cx, float cy, int compact,
                       float z_lo, float z_hi, void* records, size_t records_bytes, int* counts, void* ws,
                       size_t ws_bytes, void* st) {
  const CloudSource src = {depth, batch, h, w, step, photo, pitch, swap_rb, f_px_dev, fx, fy, cx, cy};
  long long plane = 0;
  const char* why = (!records || !counts) ? "null pointer" : cloud_source_error(src, &plane);
  if (!why && records_bytes < vertex_bytes(src, plane)) why = "records_bytes < batch * hs * ws * record size";
  if (!why && compact) {
    if (!(z_lo <= z_hi)) why = "z_lo > z_hi (or NaN)";
    else if (!ws || ws_bytes < point_cloud_ws_bytes(batch, h, w, step))
      why = "compact mode needs ws of mde_op_point_cloud_ws_bytes()";
  }
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_point_cloud: ") + why);
  OP_RET(launch_point_cloud(src, compact, z_lo, z_hi, records, counts, ws, (hipStream_t)st), "mde_op_point_cloud");
}

size_t mde_op_depth_mesh_ws_bytes(int batch, int h, int w, int step) {
  long long plane = 0;
  if (point_cloud_geometry_error(batch, h, w, step, &plane)) return 0;
  return depth_mesh_ws_bytes(batch, h, w, step);
}

int mde_op_depth_mesh(const float* depth, int batch, int h, int w, int step, const unsigned char* photo, int pitch,
                      int swap_rb, const float* f_px_dev, float fx, float fy, float cx, float cy, float z_lo,
                      float z_hi, float edge_rtol, float edge_atol, int faces, void* vertices, size_t vertices_bytes,
                      int* vertex_counts, void* face_records, size_t faces_bytes, int* face_counts, void* ws,
                      size_t ws_bytes, void* st) {
  const CloudSource src = {depth, batch, h, w, step, photo, pitch, swap_rb, f_px_dev, fx, fy, cx, cy};
  long long plane = 0;
  const char* why = (!vertices || !vertex_counts) ? "null pointer" : cloud_source_error(src, &plane);
  if (!why && vertices_bytes < vertex_bytes(src, plane)) why = "vertices_bytes < batch * hs * ws * record size";
  if (!why && !(z_lo <= z_hi)) why = "z_lo > z_hi (or NaN)";
  if (!why && !(edge_rtol >= 0.f && edge_atol >= 0.f)) why = "edge_rtol or edge_atol is negative or NaN";
  if (!why && faces) {
    // triangles of one image: < 2 * plane, no overflow in 64 bits; batch <= 65535 and 13 bytes each neither
    const long long tri = 2 * ((h + (long long)step - 1) / step - 1) * ((w + (long long)step - 1) / step - 1);
    if (!face_records || !face_counts) why = "faces with a null face_records or face_counts";
    else if (tri >= 0x7fffffffLL - 256) why = "faces: 2 * (hs - 1) * (ws - 1) of 2^31 - 256 or more";
    else if (faces_bytes < (unsigned long long)batch * tri * 13)
      why = "faces_bytes < batch * 2 * (hs - 1) * (ws - 1) * 13";
  }
  if (!why && (!ws || ws_bytes < depth_mesh_ws_bytes(batch, h, w, step)))
    why = "needs ws of mde_op_depth_mesh_ws_bytes()";
  if (!why && (reinterpret_cast<uintptr_t>(ws) & 3)) why = "ws must be 4-byte aligned";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_depth_mesh: ") + why);
  OP_RET(launch_depth_mesh(src, z_lo, z_hi, edge_rtol, edge_atol, faces, vertices, vertex_counts, face_records,
                           face_counts, ws, (hipStream_t)st),
         "mde_op_depth_mesh");
}

namespace {
// what mde_op_cloud_view_ws_bytes can judge: the point-cloud op's geometry, the picture, and the limits of
// the selection (three planes per image on grid.y; an image's two planes pooled in one quantile call)
const char* cloud_view_geometry_error(int batch, int h, int w, int step, int out_h, int out_w) {
  long long plane = 0;
  if (const char* why = point_cloud_geometry_error(batch, h, w, step, &plane)) return why;
  if (out_h < 1 || out_w < 1) return "the picture's sizes must be positive";
  if ((long long)out_h * out_w >= 0x7fffffffLL - 256) return "a picture of 2^31 - 256 pixels or more";
  if (plane >= 0x40000000LL - 128) return "a sampled grid of 2^30 - 128 samples or more";
  if (batch > 21845) return "batch > 21845";
  return nullptr;
}
}  // namespace

size_t mde_op_cloud_view_ws_bytes(int batch, int h, int w, int step, int out_h, int out_w) {
  if (cloud_view_geometry_error(batch, h, w, step, out_h, out_w)) return 0;
  return cloud_view_ws_bytes(batch, h, w, step, out_h, out_w);
}

int mde_op_cloud_view(const float* depth, int batch, int h, int w, int step, const unsigned char* photo, int pitch,
                      int swap_rb, const float* f_px_dev, float fx, float fy, float cx, float cy, double cos_a,
                      double sin_a, double cos_e, double sin_e, const double* view_in, const int* bg_rgb,
                      int out_swap_rb, unsigned char* out_u8, int out_h, int out_w, double* view_out, void* ws,
                      size_t ws_bytes, void* st) {
  const CloudSource src = {depth, batch, h, w, step, photo, pitch, swap_rb, f_px_dev, fx, fy, cx, cy};
  long long plane = 0;
  // the view's stricter limits speak after the shared geometry and before the rest of the source: the
  // geometry is judged here first and passes again inside cloud_source_error
  const char* why = (!depth || !out_u8 || !view_out || !bg_rgb)
                        ? "null pointer"
                        : cloud_view_geometry_error(batch, h, w, step, out_h, out_w);
  if (!why) why = cloud_source_error(src, &plane);
  for (double t : {cos_a, sin_a, cos_e, sin_e})
    if (!why && !(t - t == 0.0)) why = "a NaN or infinite trig value";
  for (int c = 0; !why && c < 3; ++c)
    if (bg_rgb[c] < 0 || bg_rgb[c] > 255) why = "background colour outside 0..255";
  if (!why && (!ws || ws_bytes < cloud_view_ws_bytes(batch, h, w, step, out_h, out_w)))
    why = "needs ws of mde_op_cloud_view_ws_bytes()";
  if (!why && ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(view_in) |
                reinterpret_cast<uintptr_t>(view_out)) & 7))
    why = "ws, view_in and view_out must be 8-byte aligned";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_cloud_view: ") + why);
  OP_RET(launch_cloud_view(src, cos_a, sin_a, cos_e, sin_e, view_in, bg_rgb, out_swap_rb != 0, out_u8, out_h, out_w,
                           view_out, ws, (hipStream_t)st),
         "mde_op_cloud_view");
}

namespace {
const char* depth_eval_geometry_error(int batch, int h, int w) {
  if (batch < 1 || h < 1 || w < 1) return "batch and sizes must be positive";
  if ((long long)h * w >= 0x80000000LL - 256) return "a plane of 2^31 - 256 pixels or more";
  if (batch > 65535) return "batch > 65535";
  return nullptr;
}
}  // namespace

size_t mde_op_depth_eval_ws_bytes(int batch, int h, int w) {
  if (depth_eval_geometry_error(batch, h, w)) return 0;
  return depth_eval_ws_bytes(batch, h, w);
}

int mde_op_depth_eval(const float* pred, const float* gt, const unsigned char* mask, int batch, int h, int w,
                      int policy, int pred_is_inverse, int fit_finite_only, float max_depth, double* out, void* ws,
                      size_t ws_bytes, void* st) {
  const char* why = (!pred || !gt || !mask || !out) ? "null pointer" : depth_eval_geometry_error(batch, h, w);
  if (!why && (policy < 0 || policy > 2)) why = "policy must be 0 (none), 1 (scale) or 2 (scale_shift)";
  if (!why && !(max_depth == max_depth)) why = "max_depth is NaN";
  if (!why && (!ws || ws_bytes < depth_eval_ws_bytes(batch, h, w)))
    why = "needs ws of mde_op_depth_eval_ws_bytes()";
  if (!why && ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(out)) & 7))
    why = "out and ws must be 8-byte aligned";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_depth_eval: ") + why);
  OP_RET(launch_depth_eval(pred, gt, mask, batch, h, w, policy, pred_is_inverse != 0, fit_finite_only != 0, max_depth,
                           out, ws, (hipStream_t)st),
         "mde_op_depth_eval");
}

size_t mde_op_depth_colorize_ws_bytes(int batch, int h, int w) {
  if (depth_eval_geometry_error(batch, h, w)) return 0;  // the same limits: unsigned pixel index, grid.y
  return depth_colorize_ws_bytes(batch, h, w);
}

int mde_op_depth_colorize(const float* map, int batch, int h, int w, int mode, int map_is_inverse, double denom_eps,
                          double vmin, double vmax, const unsigned char* lut257x3, int swap_rb, unsigned char* out_u8,
                          float* range_out, void* ws, size_t ws_bytes, void* st) {
  const char* why = (!map || !out_u8 || !lut257x3) ? "null pointer" : depth_eval_geometry_error(batch, h, w);
  if (!why && (mode < 0 || mode > 2)) why = "mode must be 0 (inverse_auto), 1 (minmax_u8) or 2 (fixed)";
  if (!why && !(denom_eps == denom_eps)) why = "denom_eps is NaN";
  if (!why && mode == 2 && !(vmin == vmin && vmax == vmax)) why = "vmin or vmax is NaN";
  if (!why && mode != 2) {
    if (!ws || ws_bytes < depth_colorize_ws_bytes(batch, h, w))
      why = "modes 0 and 1 need ws of mde_op_depth_colorize_ws_bytes()";
    else if (reinterpret_cast<uintptr_t>(ws) & 3)
      why = "ws must be 4-byte aligned";
  }
  if (!why && range_out && (reinterpret_cast<uintptr_t>(range_out) & 3)) why = "range_out must be 4-byte aligned";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_depth_colorize: ") + why);
  OP_RET(launch_depth_colorize(map, batch, h, w, mode, map_is_inverse != 0, denom_eps, vmin, vmax, lut257x3,
                               swap_rb != 0, out_u8, range_out, ws, (hipStream_t)st),
         "mde_op_depth_colorize");
}

int mde_op_depth_colorize_ranged(const float* map, int batch, int h, int w, int positive_only, int reciprocal,
                                 const double* range_dev, int range_stride, const unsigned char* lut257x3,
                                 int swap_rb, unsigned char* out_u8, void* st) {
  const char* why = (!map || !out_u8 || !lut257x3 || !range_dev) ? "null pointer"
                                                                  : depth_eval_geometry_error(batch, h, w);
  if (!why && range_stride < 0) why = "range_stride is negative";
  if (!why && (reinterpret_cast<uintptr_t>(range_dev) & 7)) why = "range_dev must be 8-byte aligned";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_depth_colorize_ranged: ") + why);
  OP_RET(launch_depth_colorize_ranged(map, batch, h, w, positive_only != 0, reciprocal != 0, range_dev, range_stride,
                                      lut257x3, swap_rb != 0, out_u8, (hipStream_t)st),
         "mde_op_depth_colorize_ranged");
}

size_t mde_op_depth_quantiles_ws_bytes(int batch, int h, int w) {
  if (depth_eval_geometry_error(batch, h, w)) return 0;  // the same limits: unsigned pixel index, grid.y
  return depth_quantiles_ws_bytes(batch, h, w);
}

int mde_op_depth_quantiles(const float* map, int batch, int h, int w, int positive_only, int reciprocal, int pooled,
                           int sample_cap, const double* q_percent, int nq, double* out, void* ws, size_t ws_bytes,
                           void* st) {
  const char* why = (!map || !q_percent || !out) ? "null pointer" : depth_eval_geometry_error(batch, h, w);
  if (!why && (nq < 1 || nq > 3)) why = "nq must be 1, 2 or 3";
  for (int i = 0; !why && i < nq; ++i)
    if (!(q_percent[i] >= 0.0 && q_percent[i] <= 100.0)) why = "a q_percent outside [0, 100] (or NaN)";
  if (!why && sample_cap < 0) why = "sample_cap is negative";
  // batch <= 65535 and a plane below 2^31: the product fits 64 bits
  if (!why && pooled && (long long)batch * h * w >= 0x80000000LL - 256)
    why = "pooled: batch * h * w of 2^31 - 256 or more";
  if (!why && (!ws || ws_bytes < depth_quantiles_ws_bytes(batch, h, w)))
    why = "needs ws of mde_op_depth_quantiles_ws_bytes()";
  if (!why && ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(out)) & 7))
    why = "out and ws must be 8-byte aligned";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_depth_quantiles: ") + why);
  OP_RET(launch_depth_quantiles(map, batch, h, w, positive_only != 0, reciprocal != 0, pooled != 0, sample_cap,
                                q_percent, nq, out, ws, (hipStream_t)st),
         "mde_op_depth_quantiles");
}

namespace {
// the cubic resize indexes the source, the virtual (padded) and the destination plane with an int
// and puts the batch on grid.y
const char* resize_cubic_arg_error(const void* src, const void* dst, int batch, int sh, int sw, int pitch,
                                   int pad_top, int pad_bottom, int pad_left, int pad_right, int c0, int c1, int c2,
                                   int oh, int ow) {
  if (!src || !dst) return "null pointer";
  if (batch < 1 || sh < 1 || sw < 1 || oh < 1 || ow < 1) return "batch and sizes must be positive";
  if (pitch < 3 * (long long)sw) return "pitch < 3 * sw";
  if (pad_top < 0 || pad_bottom < 0 || pad_left < 0 || pad_right < 0) return "negative pad";
  if ((c0 | c1 | c2) < 0 || c0 > 255 || c1 > 255 || c2 > 255) return "pad colour outside 0..255";
  const long long lim = 0x7fffffffLL - 256;
  const long long ph = (long long)pad_top + sh + pad_bottom, pw = (long long)pad_left + sw + pad_right;
  // ph and pw are tested alone first: below 2^31 each, their product cannot overflow 64 bits
  if ((long long)sh * sw >= lim || ph >= lim || pw >= lim || ph * pw >= lim || (long long)oh * ow >= lim)
    return "a plane of 2^31 - 256 elements or more";
  if (batch > 65535) return "batch > 65535";
  return nullptr;
}
}  // namespace

int mde_op_resize_cubic_u8(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb, int pad_top,
                           int pad_bottom, int pad_left, int pad_right, int pad_c0, int pad_c1, int pad_c2,
                           unsigned char* dst_u8, int oh, int ow, void* st) {
  if (const char* why = resize_cubic_arg_error(src, dst_u8, batch, sh, sw, pitch, pad_top, pad_bottom, pad_left,
                                               pad_right, pad_c0, pad_c1, pad_c2, oh, ow))
    return fail(MDE_ERR_ARG, std::string("mde_op_resize_cubic_u8: ") + why);
  const int pad_rgb[3] = {pad_c0, pad_c1, pad_c2};
  OP_RET(launch_resize_cubic_u8(src, batch, sh, sw, pitch, swap_rb, pad_top, pad_bottom, pad_left, pad_right, pad_rgb,
                                nullptr, dst_u8, oh, ow, (hipStream_t)st),
         "mde_op_resize_cubic_u8");
}

int mde_op_resize_cubic_u8_norm(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb,
                                int pad_top, int pad_bottom, int pad_left, int pad_right, int pad_c0, int pad_c1,
                                int pad_c2, const float* lut3x256, float* dst_f32_nchw, int oh, int ow, void* st) {
  const char* why = resize_cubic_arg_error(src, dst_f32_nchw, batch, sh, sw, pitch, pad_top, pad_bottom, pad_left,
                                           pad_right, pad_c0, pad_c1, pad_c2, oh, ow);
  if (!why && !lut3x256) why = "null pointer";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_resize_cubic_u8_norm: ") + why);
  const int pad_rgb[3] = {pad_c0, pad_c1, pad_c2};
  OP_RET(launch_resize_cubic_u8(src, batch, sh, sw, pitch, swap_rb, pad_top, pad_bottom, pad_left, pad_right, pad_rgb,
                                lut3x256, dst_f32_nchw, oh, ow, (hipStream_t)st),
         "mde_op_resize_cubic_u8_norm");
}

int mde_op_resize_cubic_f_norm(const unsigned char* src, int batch, int sh, int sw, int pitch, int swap_rb, int wide,
                               const void* scale_lut, double mean0, double mean1, double mean2, double std0,
                               double std1, double std2, float* dst, int oh, int ow, void* st) {
  const char* why = resize_cubic_arg_error(src, dst, batch, sh, sw, pitch, 0, 0, 0, 0, 0, 0, 0, oh, ow);
  if (!why && !scale_lut) why = "null pointer";
  if (!why && wide != 0 && wide != 1) why = "wide must be 0 (float) or 1 (double)";
  if (!why && (reinterpret_cast<uintptr_t>(scale_lut) & (wide ? 7 : 3))) why = "scale_lut is not aligned to its type";
  if (!why && (reinterpret_cast<uintptr_t>(dst) & 3)) why = "dst must be 4-byte aligned";
  if (!why && !(mean0 == mean0 && mean1 == mean1 && mean2 == mean2)) why = "a NaN mean";
  for (double s : {std0, std1, std2})
    if (!why && (s == 0.0 || s != s)) why = "a zero or NaN std";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_resize_cubic_f_norm: ") + why);
  const double mean[3] = {mean0, mean1, mean2}, stdv[3] = {std0, std1, std2};
  OP_RET(launch_resize_cubic_f_norm(src, batch, sh, sw, pitch, swap_rb, wide, scale_lut, mean, stdv, dst, oh, ow,
                                    (hipStream_t)st),
         "mde_op_resize_cubic_f_norm");
}

int mde_op_crop_f32(const float* src, int batch, int h, int w, int y0, int x0, int ch, int cw, float* dst, void* st) {
  const char* why = nullptr;
  if (!src || !dst) why = "null pointer";
  else if (batch < 1 || h < 1 || w < 1 || ch < 1 || cw < 1) why = "batch and sizes must be positive";
  else if (y0 < 0 || x0 < 0 || (long long)y0 + ch > h || (long long)x0 + cw > w)
    why = "the window is not inside [0, h) x [0, w)";
  else if ((long long)h * w >= 0x7fffffffLL - 256) why = "a plane of 2^31 - 256 elements or more";
  else if (batch > 65535) why = "batch > 65535";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_crop_f32: ") + why);
  OP_RET(launch_crop_f32(src, batch, h, w, y0, x0, ch, cw, dst, (hipStream_t)st), "mde_op_crop_f32");
}

int mde_op_dp_pyramid_patches(const float* img, int batch, int size, void* patches, void* st) {
  if (!img || !patches || batch < 1 || size != 1536) return fail(MDE_ERR_ARG, "mde_op_dp_pyramid_patches: bad argument");
  DpPyramid pyr;
  pyr.nlev = 3;
  const int f[3] = {1, 2, 4}, n[3] = {5, 3, 1}, stride[3] = {288, 192, 384};
  int first = 0;
  for (int i = 0; i < 3; ++i) {
    pyr.first[i] = first;
    pyr.n[i] = n[i];
    pyr.stride[i] = stride[i];
    pyr.f[i] = f[i];
    first += n[i] * n[i];
  }
  pyr.nseq = first;
  OP_RET(launch_dp_patch_prep(img, (h16*)patches, batch, size, 24, pyr, (hipStream_t)st), "dp_pyramid_patches");
}

int mde_op_merge_tokens(const float* x32, int batch, int tokens, int dim, int n, int g, int pad, int base,
                        const float* gamma, const float* beta, float eps, void* out, void* st) {
  if (!x32 || !out || batch < 1 || (gamma == nullptr) != (beta == nullptr))
    return fail(MDE_ERR_ARG, "mde_op_merge_tokens: bad argument");
  DpMerge m;
  m.B = batch;
  m.n = n;
  m.G = g;
  m.pad = pad;
  m.base = base;
  m.T = tokens;
  OP_RET(launch_merge_tokens(x32, (h16*)out, gamma, beta, dim, m, eps, (hipStream_t)st), "merge_tokens");
}

int mde_op_qk_norm_rope(void* q, void* k, const float* qg, const float* qb, const float* kg, const float* kb, int bh,
                        int tokens, int tokens_pad, int frame_tokens, int npre, int grid_w, const float* rope_cos,
                        const float* rope_sin, float q_scale, float eps, void* st) {
  if (!q || !k || !qg || !qb || !kg || !kb || !rope_cos || !rope_sin) return fail(MDE_ERR_ARG, "null argument");
  RopeGeom geo;
  geo.T = tokens;
  geo.Tpad = tokens_pad;
  geo.P = frame_tokens;
  geo.npre = npre;
  geo.gw = grid_w;
  geo.qscale = q_scale;
  geo.eps = eps;
  OP_RET(launch_qk_norm_rope((h16*)q, (h16*)k, qg, qb, kg, kb, rope_cos, rope_sin, bh, geo, (hipStream_t)st),
         "qk_norm_rope");
}

int mde_op_tap_concat_ln(const float* xa, const float* xb, int nseq, int tokens, int npre, int dim, const float* g,
                         const float* b, float eps, void* out, void* st) {
  if (!xa || !xb || !g || !b || !out || nseq < 0) return fail(MDE_ERR_ARG, "null argument");
  OP_RET(launch_tap_concat_ln(xa, xb, (h16*)out, g, b, nseq, tokens, npre, dim, eps, (hipStream_t)st),
         "tap_concat_ln");
}

int mde_op_layernorm_f16(const void* x, void* y, const float* g, const float* b, int rows, int dim, float eps,
                         int tokens, int skip_cls, void* st) {
  if (!x || !y || !g || !b) return fail(MDE_ERR_ARG, "null argument");
  if (skip_cls && tokens < 2) return fail(MDE_ERR_ARG, "skip_cls needs tokens >= 2");
  OP_RET(launch_layernorm(nullptr, (h16*)y, g, b, rows, dim, eps, tokens > 0 ? tokens : 1, skip_cls, (hipStream_t)st,
                          (const h16*)x),
         "layernorm_f16");
}

int mde_op_layernorm(const float* x, void* y, const float* g, const float* b, int rows, int dim, float eps,
                     int tokens, int skip_cls, void* st) {
  if (!x || !y || !g || !b) return fail(MDE_ERR_ARG, "null argument");
  if (skip_cls && tokens < 2) return fail(MDE_ERR_ARG, "skip_cls needs tokens >= 2");
  OP_RET(launch_layernorm(x, (h16*)y, g, b, rows, dim, eps, tokens > 0 ? tokens : 1, skip_cls, (hipStream_t)st),
         "layernorm");
}

namespace {
// fused split-K operands (GemmParams::tile_cnt): the slots live in ws, and
// every 64^2 tile of the problem has a counter (the 128^2 grids are smaller)
const char* fused_split_error(const float* ws, size_t ws_floats, const int* tile_cnt, int tile_cnt_cap,
                              size_t slot_floats, int m, int n) {
  if (!tile_cnt) return nullptr;
  if (!ws || slot_floats > ws_floats) return "fused split-K: slot_floats exceeds the workspace";
  const long long t64 = (long long)((m + 63) / 64) * ((n + 63) / 64);
  if (tile_cnt_cap < t64) return "fused split-K: fewer counters than 64^2 tiles";
  return nullptr;
}

// E_STORE split-K operands of the *_ws / *_res entry points; reports the slice count
void set_store_split(GemmParams& g, float* ws, size_t ws_floats, int* slices, int* tile_cnt, int tile_cnt_cap,
                     size_t slot_floats) {
  g.partial = ws;
  g.partial_cap = ws_floats;
  g.tile_cnt = tile_cnt;
  g.tile_cnt_cap = tile_cnt_cap;
  g.slot_cap = slot_floats;
  if (slices) *slices = gemm_store_split_slices(g);
}

// mde_op_linear_res and its subsets mde_op_linear_ws, mde_op_linear (the options they lack off)
int linear_store(const char* what, const void* a, int lda, const void* wt, int ldw, int m, int n, int k,
                 const float* bias, int act, const void* res0, int res0_rows, int res0_relu, const void* res1,
                 void* out, int ldo, float* ws, size_t ws_floats, int* slices, int* tile_cnt, int tile_cnt_cap,
                 size_t slot_floats, void* st) {
  if (!a || !wt || !out || (!ws && ws_floats)) return fail(MDE_ERR_ARG, "null argument");
  if (res0_rows < 0 || ((res0_rows > 0 || res0_relu) && !res0)) return fail(MDE_ERR_ARG, "res0 options without res0");
  if (const char* why = fused_split_error(ws, ws_floats, tile_cnt, tile_cnt_cap, slot_floats, m, n))
    return fail(MDE_ERR_ARG, why);
  GemmParams g = gemm_dense((const h16*)a, lda, (const h16*)wt, ldw, m, n, k);
  g.bias = bias;
  g.act = act;
  g.res0 = (const h16*)res0;
  g.res0_rows = res0_rows;
  g.res0_relu = res0_relu ? 1 : 0;
  g.res1 = (const h16*)res1;
  g.out16 = (h16*)out;
  g.ldo = ldo;
  set_store_split(g, ws, ws_floats, slices, tile_cnt, tile_cnt_cap, slot_floats);
  return op_status(launch_gemm(g, (hipStream_t)st), what);
}

// mde_op_conv3x3_res and its subsets mde_op_conv3x3_ws, mde_op_conv3x3
int conv3x3_store(const char* what, const void* in, int batch, int h, int w, int cin, const void* wt, int ldw,
                  int cout, int stride, int relu_in, const float* bias, int act, const void* res0, int res0_relu,
                  const void* res1, const void* res1_up, int res1_uh, int res1_uw, void* out, float* ws,
                  size_t ws_floats, int* slices, int* tile_cnt, int tile_cnt_cap, size_t slot_floats, void* st) {
  if (!in || !wt || !out || (!ws && ws_floats)) return fail(MDE_ERR_ARG, "null argument");
  if (stride != 1 && stride != 2) return fail(MDE_ERR_ARG, "stride must be 1 or 2");
  if (res0_relu && !res0) return fail(MDE_ERR_ARG, "res0_relu without res0");
  if (res1_up && !res1) return fail(MDE_ERR_ARG, "res1_up needs res1 (a buffer of the output's shape)");
  GemmParams g = gemm_conv3((const h16*)in, batch, h, w, cin, (const h16*)wt, ldw, cout, stride);
  if (const char* why = fused_split_error(ws, ws_floats, tile_cnt, tile_cnt_cap, slot_floats, g.M, g.N))
    return fail(MDE_ERR_ARG, why);
  g.relu_in = relu_in;
  g.bias = bias;
  g.act = act;
  g.res0 = (const h16*)res0;
  g.res0_relu = res0_relu ? 1 : 0;
  g.res1 = (const h16*)res1;
  g.res1_up = (const h16*)res1_up;
  g.res1_uh = res1_uh;
  g.res1_uw = res1_uw;
  g.out16 = (h16*)out;
  set_store_split(g, ws, ws_floats, slices, tile_cnt, tile_cnt_cap, slot_floats);
  return op_status(launch_gemm(g, (hipStream_t)st), what);
}
}  // namespace

int mde_op_linear(const void* a, int lda, const void* w, int ldw, int m, int n, int k, const float* bias, int act,
                  void* out, int ldo, void* st) {
  return linear_store("linear", a, lda, w, ldw, m, n, k, bias, act, nullptr, 0, 0, nullptr, out, ldo, nullptr, 0,
                      nullptr, nullptr, 0, 0, st);
}

int mde_op_linear_residual(const void* a, int lda, const void* w, int ldw, int m, int n, int k, const float* bias,
                           const float* ls, float* x32, int ldx, void* st) {
  if (!a || !w || !bias || !ls || !x32) return fail(MDE_ERR_ARG, "null argument");
  GemmParams g = gemm_dense((const h16*)a, lda, (const h16*)w, ldw, m, n, k);
  set_resid(g, bias, ls, x32, nullptr, ldx);
  OP_RET(launch_gemm(g, (hipStream_t)st), "linear_residual");
}

// E_QKV geometry: V^T stores key t at vt_pos(t), which swaps bits 2 and 3 of
// t, so a row of tokens_pad keys holds whole 16-key groups only when
// tokens_pad % 16 == 0 (otherwise the last group's keys land in the next row)
static const char* qkv_geometry_error(int batch, int tokens, int heads, int tokens_pad) {
  if (batch <= 0 || tokens <= 0 || heads <= 0) return "batch, tokens and heads must be > 0";
  if (tokens_pad < tokens) return "tokens_pad < tokens";
  if (tokens_pad % 16) return "tokens_pad % 16 != 0 (V^T key permutation works on 16-key groups)";
  return nullptr;
}

int mde_op_qkv(const void* a, const void* w, int ldw, const float* bias, int batch, int tokens, int heads,
               int tokens_pad, float qscale, void* q, void* k, void* vt, void* st) {
  if (!a || !w || !bias || !q || !k || !vt) return fail(MDE_ERR_ARG, "null argument");
  if (const char* why = qkv_geometry_error(batch, tokens, heads, tokens_pad)) return fail(MDE_ERR_ARG, why);
  const int D = heads * 64;
  GemmParams g = gemm_dense((const h16*)a, D, (const h16*)w, ldw, batch * tokens, 3 * D, D);
  g.bias = bias;
  set_qkv(g, (h16*)q, (h16*)k, (h16*)vt, tokens, tokens_pad, heads, qscale);
  OP_RET(launch_gemm(g, (hipStream_t)st), "qkv");
}

int mde_op_linear_residual_f16(const void* a, int lda, const void* w, int ldw, int m, int n, int k, const float* bias,
                               const float* ls, void* xh, int ldx, float* ln_partials, void* st) {
  if (!a || !w || !bias || !ls || !xh) return fail(MDE_ERR_ARG, "null argument");
  if (ln_partials && (n & 31)) return fail(MDE_ERR_ARG, "ln_partials need n % 32 == 0");
  GemmParams g = gemm_dense((const h16*)a, lda, (const h16*)w, ldw, m, n, k);
  set_resid(g, bias, ls, nullptr, (h16*)xh, ldx);
  set_ln_producer(g, ln_partials, m);
  OP_RET(launch_gemm(g, (hipStream_t)st), "linear_residual_f16");
}

namespace {
// mde_op_linear_lnfold_tok (a_tok = tokens: every sequence's cls row skipped)
// and its subset mde_op_linear_lnfold (a_tok = 0, lnst_rows = m)
int linear_lnfold(const char* what, const void* x, const float* ln_partials, float eps, const void* wg, int ldw,
                  const float* c1, const float* c2, int m, int n, int k, int act, void* out, int ldo, int lnst_rows,
                  int a_tok, void* st) {
  GemmParams g = gemm_dense((const h16*)x, k, (const h16*)wg, ldw, m, n, k);
  g.act = act;
  g.out16 = (h16*)out;
  g.ldo = ldo;
  set_ln_consumer(g, ln_partials, c1, c2, lnst_rows, eps);
  g.a_tok = a_tok;
  return op_status(launch_gemm(g, (hipStream_t)st), what);
}
}  // namespace

int mde_op_linear_lnfold(const void* x, const float* ln_partials, float eps, const void* wg, int ldw, const float* c1,
                         const float* c2, int m, int n, int k, int act, void* out, int ldo, void* st) {
  if (!x || !ln_partials || !wg || !c1 || !c2 || !out) return fail(MDE_ERR_ARG, "null argument");
  if (k & 31) return fail(MDE_ERR_ARG, "k % 32 != 0");
  return linear_lnfold("linear_lnfold", x, ln_partials, eps, wg, ldw, c1, c2, m, n, k, act, out, ldo, m, 0, st);
}

int mde_op_qkv_lnfold(const void* x, const float* ln_partials, float eps, const void* wg, int ldw, const float* c1,
                      const float* c2, int batch, int tokens, int heads, int tokens_pad, float qscale, void* q, void* k,
                      void* vt, void* st) {
  if (!x || !ln_partials || !wg || !c1 || !c2 || !q || !k || !vt) return fail(MDE_ERR_ARG, "null argument");
  if (const char* why = qkv_geometry_error(batch, tokens, heads, tokens_pad)) return fail(MDE_ERR_ARG, why);
  const int D = heads * 64;
  GemmParams g = gemm_dense((const h16*)x, D, (const h16*)wg, ldw, batch * tokens, 3 * D, D);
  set_qkv(g, (h16*)q, (h16*)k, (h16*)vt, tokens, tokens_pad, heads, qscale);
  set_ln_consumer(g, ln_partials, c1, c2, g.M, eps);
  OP_RET(launch_gemm(g, (hipStream_t)st), "qkv_lnfold");
}

int mde_op_attention(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int tokens,
                     int tokens_pad, int ldo, void* st) {
  if (!q || !k || !vt || !o) return fail(MDE_ERR_ARG, "null argument");
  OP_RET(launch_attention((const h16*)q, (const h16*)k, (const h16*)vt, (h16*)o, batch, heads, tokens, tokens_pad,
                          ldo, (hipStream_t)st),
         "attention");
}

int mde_op_attention_ws(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int tokens,
                        int tokens_pad, int ldo, void* ws, size_t ws_bytes, void* st) {
  if (!q || !k || !vt || !o || (!ws && ws_bytes)) return fail(MDE_ERR_ARG, "null argument");
  OP_RET(launch_attention((const h16*)q, (const h16*)k, (const h16*)vt, (h16*)o, batch, heads, tokens, tokens_pad,
                          ldo, (hipStream_t)st, (float*)ws, ws_bytes),
         "attention_ws");
}

int mde_op_attention_cfg(const void* q, const void* k, const void* vt, void* o, int batch, int heads, int tokens,
                         int tokens_pad, int ldo, const char* cfg, void* ws, size_t ws_bytes, void* st) {
  if (!q || !k || !vt || !o || (!ws && ws_bytes)) return fail(MDE_ERR_ARG, "null argument");
  OP_RET(launch_attention((const h16*)q, (const h16*)k, (const h16*)vt, (h16*)o, batch, heads, tokens, tokens_pad,
                          ldo, (hipStream_t)st, (float*)ws, ws_bytes, cfg),
         "attention_cfg");
}

size_t mde_op_attention_ws_bytes(int batch, int heads, int tokens) {
  return batch > 0 && heads > 0 && tokens > 0 ? attention_split_ws_bytes(batch, heads, tokens) : 0;
}

int mde_op_linear32(const float* a, int lda, const float* w, int ldw, int m, int n, int k, const float* bias, int act,
                    float* out, int ldo, void* st) {
  if (!a || !w || !out) return fail(MDE_ERR_ARG, "null argument");
  Gemm32Params g;
  g.A = a;
  g.lda = lda;
  g.W = w;
  g.ldw = ldw;
  g.M = m;
  g.N = n;
  g.K = k;
  g.bias = bias;
  g.act = act;
  g.out32 = out;
  g.ldo = ldo;
  OP_RET(launch_gemm32(g, (hipStream_t)st), "linear32");
}

int mde_op_conv3x3_32(const float* in, int batch, int h, int w, int cin, const float* wt, int ldw, int cout,
                      int stride, int relu_in, const float* bias, int act, const float* res0, const float* res1,
                      float* out, void* st) {
  if (!in || !wt || !out) return fail(MDE_ERR_ARG, "null argument");
  if (stride != 1 && stride != 2) return fail(MDE_ERR_ARG, "stride must be 1 or 2");
  if (batch <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return fail(MDE_ERR_ARG, "bad shape");
  Gemm32Params g;
  g.amode = A_CONV3;
  g.emode = E_STORE;
  g.A = in;
  g.cb = batch;
  g.ch = h;
  g.cw = w;
  g.cc = cin;
  g.stride = stride;
  g.oh = (h - 1) / stride + 1;
  g.ow = (w - 1) / stride + 1;
  g.W = wt;
  g.ldw = ldw;
  g.M = batch * g.oh * g.ow;
  g.N = cout;
  g.K = 9 * cin;
  g.relu_in = relu_in;
  g.bias = bias;
  g.act = act;
  g.res0 = res0;
  g.res1 = res1;
  g.out32 = out;
  g.ldo = cout;
  OP_RET(launch_gemm32(g, (hipStream_t)st), "conv3x3_32");
}

int mde_op_conv_transpose32(const float* in, int batch, int h, int w, int cin, const float* wt, int ldw, int cout,
                            int stride, const float* bias, float* out, void* st) {
  if (!in || !wt || !out) return fail(MDE_ERR_ARG, "null argument");
  if (batch <= 0 || h <= 0 || w <= 0 || stride < 1) return fail(MDE_ERR_ARG, "bad shape");
  Gemm32Params g;
  g.emode = E_CONVT;
  g.A = in;
  g.lda = cin;
  g.W = wt;
  g.ldw = ldw;
  g.M = batch * h * w;
  g.N = stride * stride * cout;
  g.K = cin;
  g.bias = bias;
  g.out32 = out;
  g.ldo = cout;
  g.s = stride;
  g.cout = cout;
  g.cb = batch;
  g.ih = h;
  g.iw = w;
  OP_RET(launch_gemm32(g, (hipStream_t)st), "conv_transpose32");
}

int mde_op_resize32(const float* in, int batch, int h, int w, int c, int oh, int ow, float* out, void* st) {
  if (!in || !out) return fail(MDE_ERR_ARG, "null argument");
  OP_RET(launch_resize32(in, out, batch, h, w, c, oh, ow, (hipStream_t)st), "resize32");
}

int mde_op_linear_residual32(const float* a, int lda, const float* w, int ldw, int m, int n, int k,
                             const float* bias, const float* ls, float* x32, int ldx, void* st) {
  if (!a || !w || !ls || !x32) return fail(MDE_ERR_ARG, "null argument");
  Gemm32Params g;
  g.emode = E_RESID;
  g.A = a;
  g.lda = lda;
  g.W = w;
  g.ldw = ldw;
  g.M = m;
  g.N = n;
  g.K = k;
  g.bias = bias;
  g.ls = ls;
  g.x32 = x32;
  g.ldo = ldx;
  OP_RET(launch_gemm32(g, (hipStream_t)st), "linear_residual32");
}

int mde_op_qkv32(const float* a, const float* w, int ldw, const float* bias, int batch, int tokens, int heads,
                 int tokens_pad, float q_scale, float* q, float* k, float* v, void* st) {
  if (!a || !w || !q || !k || !v) return fail(MDE_ERR_ARG, "null argument");
  Gemm32Params g;
  g.emode = E_QKV;
  g.A = a;
  g.lda = heads * 64;
  g.W = w;
  g.ldw = ldw;
  g.M = batch * tokens;
  g.N = 3 * heads * 64;
  g.K = heads * 64;
  g.bias = bias;
  g.q = q;
  g.k = k;
  g.v = v;
  g.T = tokens;
  g.Tpad = tokens_pad;
  g.heads = heads;
  g.qscale = q_scale;
  OP_RET(launch_gemm32(g, (hipStream_t)st), "qkv32");
}

int mde_op_attention32(const float* q, const float* k, const float* v, float* o, int batch, int heads, int tokens,
                       int tokens_pad, int ldo, void* st) {
  if (!q || !k || !v || !o) return fail(MDE_ERR_ARG, "null argument");
  OP_RET(launch_attention32(q, k, v, o, batch, heads, tokens, tokens_pad, ldo, (hipStream_t)st), "attention32");
}

int mde_op_patch_embed(const float* img, int batch, int h, int w, const void* wt, int ldw, const float* bias,
                       const float* pos_patch, const float* cls_pos, int dim, void* scratch, float* x32, void* st) {
  if (!img || !wt || !bias || !pos_patch || !cls_pos || !scratch || !x32) return fail(MDE_ERR_ARG, "null argument");
  if (h % 14 || w % 14) return fail(MDE_ERR_ARG, "image size must be a multiple of 14");
  const int ph = h / 14, pw = w / 14, T = ph * pw + 1;
  hipError_t e = launch_patch_prep(img, (h16*)scratch, x32, cls_pos, batch, h, w, ph, pw, T, dim, (hipStream_t)st);
  if (e != hipSuccess) return hip_fail(e, "patch_prep");
  GemmParams g = gemm_dense((const h16*)scratch, 672, (const h16*)wt, ldw, batch * ph * pw, dim, 672);
  g.emode = E_PATCH;
  g.bias = bias;
  g.x32 = x32;
  g.ldo = dim;
  g.T = T;
  g.pos = pos_patch;
  g.npatch = ph * pw;
  OP_RET(launch_gemm(g, (hipStream_t)st), "patch_embed");
}

int mde_op_conv3x3(const void* in, int batch, int h, int w, int cin, const void* wt, int ldw, int cout, int stride,
                   int relu_in, const float* bias, int act, const void* res0, const void* res1, void* out,
                   void* st) {
  return conv3x3_store("conv3x3", in, batch, h, w, cin, wt, ldw, cout, stride, relu_in, bias, act, res0, 0, res1,
                       nullptr, 0, 0, out, nullptr, 0, nullptr, nullptr, 0, 0, st);
}

int mde_op_conv3x3_ws(const void* in, int batch, int h, int w, int cin, const void* wt, int ldw, int cout, int stride,
                      int relu_in, const float* bias, int act, const void* res0, const void* res1, void* out,
                      float* ws, size_t ws_floats, int* slices, void* st) {
  return conv3x3_store("conv3x3_ws", in, batch, h, w, cin, wt, ldw, cout, stride, relu_in, bias, act, res0, 0, res1,
                       nullptr, 0, 0, out, ws, ws_floats, slices, nullptr, 0, 0, st);
}

int mde_op_linear_ws(const void* a, int lda, const void* wt, int ldw, int m, int n, int k, const float* bias, int act,
                     void* out, int ldo, float* ws, size_t ws_floats, int* slices, void* st) {
  return linear_store("linear_ws", a, lda, wt, ldw, m, n, k, bias, act, nullptr, 0, 0, nullptr, out, ldo, ws,
                      ws_floats, slices, nullptr, 0, 0, st);
}

int mde_op_conv3x3_up(const void* in, int batch, int sh, int sw, int cin, int uh, int uw, const void* wt, int ldw,
                      int cout, const float* bias, int act, void* out, void* st) {
  if (!in || !wt || !out) return fail(MDE_ERR_ARG, "null argument");
  GemmParams g = gemm_conv3_up((const h16*)in, batch, sh, sw, cin, uh, uw, (const h16*)wt, ldw, cout);
  g.bias = bias;
  g.act = act;
  g.out16 = (h16*)out;
  g.ldo = cout;
  OP_RET(launch_gemm(g, (hipStream_t)st), "conv3x3_up");
}

namespace {
// mde_op_conv_transpose_ld and its subset mde_op_conv_transpose (ldo = cout)
int conv_transpose(const char* what, const void* in, int batch, int h, int w, int cin, const void* wt, int ldw,
                   int cout, int stride, const float* bias, void* out, int ldo, void* st) {
  if (!in || !wt || !bias || !out) return fail(MDE_ERR_ARG, "null argument");
  GemmParams g = gemm_convt((const h16*)in, batch, h, w, cin, (const h16*)wt, ldw, cout, stride, (h16*)out, ldo);
  g.bias = bias;
  return op_status(launch_gemm(g, (hipStream_t)st), what);
}
}  // namespace

int mde_op_conv_transpose(const void* in, int batch, int h, int w, int cin, const void* wt, int ldw, int cout,
                          int stride, const float* bias, void* out, void* st) {
  return conv_transpose("conv_transpose", in, batch, h, w, cin, wt, ldw, cout, stride, bias, out, cout, st);
}

int mde_op_resize_bilinear(const void* in, int batch, int ih, int iw, int c, int oh, int ow, void* out, void* st) {
  if (!in || !out) return fail(MDE_ERR_ARG, "null argument");
  OP_RET(launch_resize((const h16*)in, (h16*)out, batch, ih, iw, c, oh, ow, (hipStream_t)st), "resize_bilinear");
}

namespace {
// mde_op_depth_head_pe and its subset mde_op_depth_head (no hpe)
int depth_head(const char* what, const void* in, int batch, int sh, int sw, int cin, int uh, int uw, const void* wt,
               int ldw, const float* bias, const float* w2, float b2, int metric, float max_depth, const void* hpe,
               int hpe_pix, float* out, void* st) {
  if (!in || !wt || !bias || !w2 || !out) return fail(MDE_ERR_ARG, "null argument");
  if (hpe && hpe_pix < 1) return fail(MDE_ERR_ARG, "hpe needs hpe_pix >= 1");
  GemmParams g = gemm_conv3_up((const h16*)in, batch, sh, sw, cin, uh, uw, (const h16*)wt, ldw, 32);
  g.bias = bias;
  set_head(g, w2, b2, metric, max_depth, (const h16*)hpe, hpe ? hpe_pix : 0, out);
  return op_status(launch_gemm(g, (hipStream_t)st), what);
}
}  // namespace

int mde_op_depth_head(const void* in, int batch, int sh, int sw, int cin, int uh, int uw, const void* wt, int ldw,
                      const float* bias, const float* w2, float b2, int metric, float max_depth, float* out,
                      void* st) {
  return depth_head("depth_head", in, batch, sh, sw, cin, uh, uw, wt, ldw, bias, w2, b2, metric, max_depth, nullptr, 0,
                    out, st);
}

// ---- the GemmParams options only the engine graphs set, one wrapper each ----
// (no kernel code and no policy here: launch_gemm picks the route as it does
// for the engines; tests/test_gpu_ops_engine_paths.py)
int mde_op_linear_res(const void* a, int lda, const void* wt, int ldw, int m, int n, int k, const float* bias, int act,
                      const void* res0, int res0_rows, int res0_relu, const void* res1, void* out, int ldo, float* ws,
                      size_t ws_floats, int* slices, int* tile_cnt, int tile_cnt_cap, size_t slot_floats, void* st) {
  return linear_store("linear_res", a, lda, wt, ldw, m, n, k, bias, act, res0, res0_rows, res0_relu, res1, out, ldo,
                      ws, ws_floats, slices, tile_cnt, tile_cnt_cap, slot_floats, st);
}

int mde_op_conv3x3_res(const void* in, int batch, int h, int w, int cin, const void* wt, int ldw, int cout, int stride,
                       int relu_in, const float* bias, int act, const void* res0, int res0_relu, const void* res1,
                       const void* res1_up, int res1_uh, int res1_uw, void* out, float* ws, size_t ws_floats,
                       int* slices, int* tile_cnt, int tile_cnt_cap, size_t slot_floats, void* st) {
  return conv3x3_store("conv3x3_res", in, batch, h, w, cin, wt, ldw, cout, stride, relu_in, bias, act, res0, res0_relu,
                       res1, res1_up, res1_uh, res1_uw, out, ws, ws_floats, slices, tile_cnt, tile_cnt_cap,
                       slot_floats, st);
}

int mde_op_linear_lnfold_tok(const void* x, const float* ln_partials, float eps, const void* wg, int ldw,
                             const float* c1, const float* c2, int seqs, int tokens, int n, int k, int act, void* out,
                             int ldo, void* st) {
  if (!x || !ln_partials || !wg || !c1 || !c2 || !out) return fail(MDE_ERR_ARG, "null argument");
  if (k & 31) return fail(MDE_ERR_ARG, "k % 32 != 0");
  if (seqs < 1 || tokens < 2) return fail(MDE_ERR_ARG, "seqs >= 1 and tokens >= 2 (a cls row and at least one more)");
  return linear_lnfold("linear_lnfold_tok", x, ln_partials, eps, wg, ldw, c1, c2, seqs * (tokens - 1), n, k, act, out,
                       ldo, seqs * tokens, tokens, st);
}

int mde_op_depth_head_pe(const void* in, int batch, int sh, int sw, int cin, int uh, int uw, const void* wt, int ldw,
                         const float* bias, const float* w2, float b2, int metric, float max_depth, const void* hpe,
                         int hpe_pix, float* out, void* st) {
  return depth_head("depth_head_pe", in, batch, sh, sw, cin, uh, uw, wt, ldw, bias, w2, b2, metric, max_depth, hpe,
                    hpe_pix, out, st);
}

int mde_op_conv_transpose_ld(const void* in, int batch, int h, int w, int cin, const void* wt, int ldw, int cout,
                             int stride, const float* bias, void* out, int ldo, void* st) {
  return conv_transpose("conv_transpose_ld", in, batch, h, w, cin, wt, ldw, cout, stride, bias, out, ldo, st);
}

int mde_op_linear_residual_split(const void* a, int lda, const void* wt, int ldw, int m, int n, int k,
                                 const float* bias, const float* ls, float* x32, void* xh, int ldx, float* ln_partials,
                                 int splitk, float* ws, size_t ws_floats, int* tile_cnt, int tile_cnt_cap,
                                 size_t slot_floats, void* st) {
  if (!a || !wt || !bias || !ls || (!x32 == !xh) || (!ws && ws_floats))
    return fail(MDE_ERR_ARG, "null argument (one of x32 / xh)");
  if (ln_partials && (!xh || (n & 31))) return fail(MDE_ERR_ARG, "ln_partials need xh and n % 32 == 0");
  if (m < 0 || n < 0 || splitk < 0) return fail(MDE_ERR_ARG, "negative size");
  // the 128^2 route cuts K into 4 slices whatever splitk says
  if (splitk > 1 && (!ws || ws_floats / (size_t)(splitk > 4 ? splitk : 4) < (size_t)m * (size_t)n))
    return fail(MDE_ERR_ARG, "ws must hold max(splitk, 4) * m * n floats");
  if (const char* why = fused_split_error(ws, ws_floats, tile_cnt, tile_cnt_cap, slot_floats, m, n))
    return fail(MDE_ERR_ARG, why);
  GemmParams g = gemm_dense((const h16*)a, lda, (const h16*)wt, ldw, m, n, k);
  set_resid(g, bias, ls, x32, (h16*)xh, ldx);
  if (ln_partials) set_ln_producer(g, ln_partials, m);
  if (splitk > 1) set_resid_splitk(g, ws, splitk, slot_floats, tile_cnt, tile_cnt_cap);
  OP_RET(launch_gemm(g, (hipStream_t)st), "linear_residual_split");
}

// ---- ABI 12: the row / head / patch-embed kernels only the engine graphs reached, one wrapper each ----
// (no kernel code and no policy here; tests/test_gpu_rows.py, tests/test_gpu_engine_rows.py)
namespace {
// a [nseq][tokens][dim] stream addressed by a kernel with one thread per element or per row
const char* stream_rows_error(int nseq, int tokens, int dim) {
  if (nseq < 1 || tokens < 1 || dim < 1) return "nseq, tokens and dim must be positive";
  if ((long long)nseq * tokens >= 0x7fffffffLL / 4) return "nseq * tokens of 2^29 or more";
  return nullptr;
}
}  // namespace

int mde_op_layernorm32(const float* x, float* y, const float* g, const float* b, int rows, int dim, float eps,
                       int tokens, int skip_cls, void* st) {
  if (!x || !y || !g || !b) return fail(MDE_ERR_ARG, "mde_op_layernorm32: null argument");
  if (rows < 0) return fail(MDE_ERR_ARG, "mde_op_layernorm32: negative rows");
  if (skip_cls && tokens < 2) return fail(MDE_ERR_ARG, "mde_op_layernorm32: skip_cls needs tokens >= 2");
  if (skip_cls && rows % tokens) return fail(MDE_ERR_ARG, "mde_op_layernorm32: skip_cls needs rows % tokens == 0");
  OP_RET(launch_layernorm32(x, y, g, b, rows, dim, eps, (hipStream_t)st, tokens > 0 ? tokens : 1, skip_cls),
         "mde_op_layernorm32");
}

int mde_op_rows_layernorm(float* x, const float* g, const float* b, int nseq, int tokens, int row0, int dim, float eps,
                          void* st) {
  const char* why = (!x || !g || !b) ? "null argument" : stream_rows_error(nseq, tokens, dim);
  if (!why && (row0 < 0 || row0 >= tokens)) why = "row0 outside [0, tokens)";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_rows_layernorm: ") + why);
  OP_RET(launch_rows_layernorm(x, g, b, nseq, tokens, row0, dim, eps, (hipStream_t)st), "mde_op_rows_layernorm");
}

int mde_op_prefix_rows(float* x, const float* pre, int nseq, int tokens, int npre, int dim, int frames, int sets,
                       void* st) {
  const char* why = (!x || !pre) ? "null argument" : stream_rows_error(nseq, tokens, dim);
  if (!why && (npre < 1 || npre > tokens)) why = "npre outside [1, tokens]";
  if (!why && (dim & 3)) why = "dim % 4 != 0";
  if (!why && sets != 1 && sets != 2) why = "sets must be 1 or 2";
  if (!why && frames < 1) why = "frames must be positive";
  if (!why && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(pre)) & 15))
    why = "x and pre must be 16-byte aligned";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_prefix_rows: ") + why);
  OP_RET(launch_prefix_rows(x, pre, nseq, tokens, npre, dim, frames, sets, (hipStream_t)st), "mde_op_prefix_rows");
}

int mde_op_cls_rows(float* x, const float* cls, int nseq, int tokens, int dim, void* st) {
  const char* why = (!x || !cls) ? "null argument" : stream_rows_error(nseq, tokens, dim);
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_cls_rows: ") + why);
  OP_RET(launch_cls_rows(x, cls, nseq, tokens, dim, (hipStream_t)st), "mde_op_cls_rows");
}

int mde_op_fov_final(const void* in_f16, const float* w, float bias, int k, int batch, float* out, void* st) {
  if (!in_f16 || !w || !out) return fail(MDE_ERR_ARG, "mde_op_fov_final: null argument");
  if (k < 1 || batch < 1) return fail(MDE_ERR_ARG, "mde_op_fov_final: k and batch must be positive");
  OP_RET(launch_fov_final((const h16*)in_f16, w, bias, k, batch, out, (hipStream_t)st), "mde_op_fov_final");
}

int mde_op_head32(const float* hid, const float* w2, float b2, int m, int metric, float max_depth, float* out,
                  void* st) {
  if (!hid || !w2 || !out) return fail(MDE_ERR_ARG, "mde_op_head32: null argument");
  if (m < 1) return fail(MDE_ERR_ARG, "mde_op_head32: m must be positive");
  if (metric < 0 || metric > 2) return fail(MDE_ERR_ARG, "mde_op_head32: metric must be 0 (ReLU), 1 (sigmoid) or 2 (exp)");
  if (reinterpret_cast<uintptr_t>(hid) & 15) return fail(MDE_ERR_ARG, "mde_op_head32: hid must be 16-byte aligned");
  OP_RET(launch_head32(hid, w2, b2, m, metric, max_depth, out, (hipStream_t)st), "mde_op_head32");
}

int mde_op_patch_embed_stream(const float* img, int batch, int h, int w, const void* wt, int ldw, const float* bias,
                              const float* pos_patch, const float* cls_pos, int dim, int tokens, int tok0,
                              void* scratch, float* x32, void* xh, float* ln_partials, const float* cls_st,
                              void* st) {
  const char* why = nullptr;
  const int ph = h / 14, pw = w / 14;
  if (!img || !wt || !bias || !pos_patch || !scratch) why = "null argument";
  else if (!x32 == !xh) why = "exactly one of x32 / xh_f16";
  else if (batch < 1 || ph < 1 || pw < 1 || dim < 1) why = "batch and dim positive, h and w at least 14";
  else if (tok0 < 0 || (long long)tok0 + (long long)ph * pw > tokens) why = "tok0 + patches exceeds tokens";
  else if (cls_pos && tok0 < 1) why = "a cls row needs tok0 >= 1";
  else if ((ln_partials || cls_st) && !(xh && ln_partials && cls_st && cls_pos))
    why = "ln_partials and cls_st come together, with xh_f16 and cls_pos";
  else if (ln_partials && (dim & 31)) why = "ln_partials need dim % 32 == 0";
  if (why) return fail(MDE_ERR_ARG, std::string("mde_op_patch_embed_stream: ") + why);
  // cls_pos null: no cls row (rows [0, tok0) of every sequence belong to another kernel)
  hipError_t e = launch_patch_prep(img, (h16*)scratch, cls_pos ? x32 : nullptr, cls_pos, batch, h, w, ph, pw, tokens,
                                   dim, (hipStream_t)st, cls_pos ? (h16*)xh : nullptr, ln_partials, cls_st);
  if (e != hipSuccess) return op_status(e, "mde_op_patch_embed_stream (patch_prep)");
  GemmParams g = gemm_dense((const h16*)scratch, 672, (const h16*)wt, ldw, batch * ph * pw, dim, 672);
  g.emode = E_PATCH;
  g.bias = bias;
  g.x32 = x32;
  g.xh = (h16*)xh;
  g.ldo = dim;
  g.T = tokens;
  g.tok0 = tok0;
  g.pos = pos_patch;
  g.npatch = ph * pw;
  if (ln_partials) set_ln_producer(g, ln_partials, batch * tokens);
  OP_RET(launch_gemm(g, (hipStream_t)st), "mde_op_patch_embed_stream");
}

int mde_op_patch_embed32(const float* img, int batch, int h, int w, const float* wt, int ldw, const float* bias,
                         const float* pos_patch, const float* cls_pos, int dim, float* scratch32, float* x32,
                         void* st) {
  const int ph = h / 14, pw = w / 14;
  if (!img || !wt || !bias || !pos_patch || !cls_pos || !scratch32 || !x32)
    return fail(MDE_ERR_ARG, "mde_op_patch_embed32: null argument");
  if (batch < 1 || ph < 1 || pw < 1 || dim < 1)
    return fail(MDE_ERR_ARG, "mde_op_patch_embed32: batch and dim positive, h and w at least 14");
  const int T = ph * pw + 1;
  hipError_t e = launch_patch_prep(img, nullptr, x32, cls_pos, batch, h, w, ph, pw, T, dim, (hipStream_t)st, nullptr,
                                   nullptr, nullptr, scratch32);
  if (e != hipSuccess) return op_status(e, "mde_op_patch_embed32 (patch_prep)");
  Gemm32Params g;
  g.emode = E_PATCH;
  g.A = scratch32;
  g.lda = 672;
  g.W = wt;
  g.ldw = ldw;
  g.M = batch * ph * pw;
  g.N = dim;
  g.K = 672;
  g.bias = bias;
  g.x32 = x32;
  g.ldo = dim;
  g.T = T;
  g.pos = pos_patch;
  g.npatch = ph * pw;
  OP_RET(launch_gemm32(g, (hipStream_t)st), "mde_op_patch_embed32");
}

}  // extern "C"
