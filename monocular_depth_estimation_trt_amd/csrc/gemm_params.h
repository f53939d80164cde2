// GemmParams builders: the one place the host code assembles the launch
// parameters of launch_gemm's operand and epilogue modes.  The forward
// schedules (engine.hip, depth_pro.hip, vggt.hip, through Runner) and the
// op-level ABI wrappers (ops_abi.hip) both build through these, so the parity
// tests of the ops check the assembly the engines run.  Plain pointers and
// ints only: nothing here knows of Runner or weight names.
#pragma once
#include "mde_ops.h"

namespace mde {

// dh^-0.5 * log2(e) for 64-wide heads: attention scores in log2 units
constexpr float kQScale = 0.125f * 1.4426950408889634f;

inline GemmParams gemm_dense(const h16* A, int lda, const h16* W, int ldw, int M, int N, int K) {
  GemmParams g;
  g.amode = A_DENSE;
  g.A = A;
  g.lda = lda;
  g.W = W;
  g.ldw = ldw;
  g.M = M;
  g.N = N;
  g.K = K;
  return g;
}

// 3x3 pad-1 conv over NHWC map [B][h][w][cin] -> [B][oh][ow][cout]
inline GemmParams gemm_conv3(const h16* in, int B, int h, int w, int cin, const h16* W, int ldw, int cout,
                             int stride) {
  GemmParams g;
  g.amode = A_CONV3;
  g.A = in;
  g.cb = B;
  g.ch = h;
  g.cw = w;
  g.cc = cin;
  g.stride = stride;
  g.oh = (h - 1) / stride + 1;
  g.ow = (w - 1) / stride + 1;
  g.W = W;
  g.ldw = ldw;
  g.M = B * g.oh * g.ow;
  g.N = cout;
  g.K = 9 * cin;
  g.ldo = cout;
  return g;
}

// the same conv over the bilinear (align_corners) upsample of [B][sh][sw][cin]
// to uh x uw, formed in the loader; the caller sets the epilogue (and ldo)
inline GemmParams gemm_conv3_up(const h16* in, int B, int sh, int sw, int cin, int uh, int uw, const h16* W, int ldw,
                                int cout) {
  GemmParams g;
  g.amode = A_CONV3_UP;
  g.A = in;
  g.cb = B;
  g.ch = sh;
  g.cw = sw;
  g.cc = cin;
  g.uh = uh;
  g.uw = uw;
  g.oh = uh;
  g.ow = uw;
  g.stride = 1;
  g.W = W;
  g.ldw = ldw;
  g.M = B * uh * uw;
  g.N = cout;
  g.K = 9 * cin;
  return g;
}

// ConvTranspose(k = s) of an NHWC map as a GEMM with a pixel-shuffle
// epilogue; ldo = channel stride of the output map (concat slots, padding)
inline GemmParams gemm_convt(const h16* in, int B, int h, int w, int cin, const h16* W, int ldw, int cout, int s,
                             h16* out, int ldo) {
  GemmParams g = gemm_dense(in, cin, W, ldw, B * h * w, s * s * cout, cin);
  g.emode = E_CONVT;
  g.out16 = out;
  g.s = s;
  g.cout = cout;
  g.ldo = ldo;
  g.ih = h;
  g.iw = w;
  return g;
}

inline void set_qkv(GemmParams& g, h16* q, h16* k, h16* vt, int T, int Tpad, int heads, float qscale) {
  g.emode = E_QKV;
  g.q = q;
  g.k = k;
  g.vt = vt;
  g.T = T;
  g.Tpad = Tpad;
  g.heads = heads;
  g.qscale = qscale;
}

// one of x32 / xh is the residual stream
inline void set_resid(GemmParams& g, const float* bias, const float* ls, float* x32, h16* xh, int ldo) {
  g.emode = E_RESID;
  g.bias = bias;
  g.ls = ls;
  g.x32 = x32;
  g.xh = xh;
  g.ldo = ldo;
}

// LayerNorm folded across the GEMM boundary (GemmParams::lnst_in): A = the raw
// f16 residual rows, W = W * gamma, c1 / c2 the folded column sums and bias,
// partials = the producers' row partials over `rows` rows
inline void set_ln_consumer(GemmParams& g, const float* partials, const float* c1, const float* c2, int rows,
                            float eps) {
  g.lnst_in = partials;
  g.lnc1 = c1;
  g.bias = c2;
  g.lnst_ns = g.K / 32;
  g.lnst_rows = rows;
  g.ln_eps = eps;
}

inline void set_ln_producer(GemmParams& g, float* partials, int rows) {
  g.lnst_out = partials;
  g.lnst_ns = g.N / 32;
  g.lnst_rows = rows;
}

inline void set_head(GemmParams& g, const float* w2, float b2, int metric, float max_depth, const h16* hpe,
                     int hpe_pix, float* out32) {
  g.emode = E_HEAD;
  g.w2 = w2;
  g.b2 = b2;
  g.head_metric = metric;
  g.max_depth = max_depth;
  g.hpe = hpe;
  g.hpe_pix = hpe_pix;
  g.out32 = out32;
}

inline void set_resid_splitk(GemmParams& g, float* ws, int slices, size_t slot_cap, int* tile_cnt, int tile_cnt_cap) {
  g.partial = ws;
  g.splitk = slices;
  g.slot_cap = slot_cap;
  g.tile_cnt = tile_cnt;
  g.tile_cnt_cap = tile_cnt_cap;
}

}  // namespace mde
