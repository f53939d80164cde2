// VGGT's device preprocess and crop: OpenCV's 8-bit, 3-channel INTER_CUBIC resize
// (`cv2.resize(padded_u8, (ow, oh), interpolation=cv2.INTER_CUBIC)` after the
// `cv2.copyMakeBorder(BORDER_CONSTANT)` of reference core/preprocess.py:
// resize_square_pad), restated from OpenCV's published scalar fixed-point
// algorithm, reading the border as a virtual one (no padded copy), with the
// BGR->RGB swap and the /255 of core/preprocess.py:scale folded into the store;
// and the content-box crop of the depth map (models/vggt/onnx2trt.py:131).
//
// Contract (the same text as include/mde.h; monocular_depth_estimation_trt_amd/
// preprocess.py:resize_cubic_u8 is the independent numpy restatement the tests
// hold this kernel to, bit for bit):
//
//   virtual source: ph = pad_top + sh + pad_bottom rows by pw = pad_left + sw +
//     pad_right columns; pixel (y, x) is the photo's pixel (y - pad_top,
//     x - pad_left) where that lies inside the photo, the pad colour elsewhere
//   per axis (dst outputs from src = pw or ph inputs), the same on both axes; no
//   fraction is zeroed at a border
//     scale = 1.0 / ((double)dst / (double)src)        float64; NOT src / dst
//     f     = (float)((d + 0.5) * scale - 0.5)         float64, rounded once to float32
//     s     = floor(f);  x = f - s                     float32
//     taps  = s - 1, s, s + 1, s + 2, each clamped to [0, src - 1] of the VIRTUAL image
//   coefficients, float32, every operation rounded separately in this order,
//   never fused; A = -0.75f (5A, 8A, 4A, A + 2, A + 3 are exact)
//     x1 = x + 1
//     c0 = ((A*x1 - 5*A)*x1 + 8*A)*x1 - 4*A
//     c1 = (((A + 2)*x - (A + 3))*x)*x + 1
//     g  = 1 - x
//     c2 = (((A + 2)*g - (A + 3))*g)*g + 1
//     c3 = ((1 - c0) - c1) - c2
//     k_i = rint(c_i * 2048.f)      half to even; the four need not sum to 2048
//                                   (2047..2049 occur)
//   horizontal pass, exact integers, no shift
//     H = sum_i S[tap_i] * a_i
//   vertical pass
//     V = sum_j H_j * b_j;  out = clamp((V + (1 << 21)) >> 22, 0, 255)   arithmetic shift
//   swap_rb != 0: output channel c reads source channel 2 - c; the pad colour
//   is given in OUTPUT channel order (the reference pads after its BGR->RGB)
//
// int32 holds V: sum_i |c_i| is largest at x = 0.5, where the coefficients are
// -0.09375, 0.59375, 0.59375, -0.09375, so 1.375; each k_i is within 0.5 of
// 2048 c_i, so sum_i |k_i| <= 2816 + 2, and
//   |V| + 2^21 <= 255 * 2818^2 + 2^21 = 2 027 095 772 < 2^31 = 2 147 483 648.
//
// Rounding discipline: as in preprocess.hip -- coordinates and coefficients are
// computed in the kernel from a `scale` the host computed as a double, one
// rounded operation per step.  With this toolchain's headers the _rn forms are
// the plain operators, so what forbids contracting any a * b + c above into an
// fma is -ffp-contract=off (_build.PER_FILE) and the pragma below.
//
// Thread mapping: one thread produces one output pixel, all three channels;
// consecutive lanes are consecutive output columns of one row.  A pixel has
// 4 x 4 taps of 3 bytes.  At the 3024 -> 518 ratio (5.84 source pixels per
// output) neighbouring outputs share no tap: lane l reads 12 contiguous bytes
// at byte offset ~17.5 l of each of its four rows, so a wave touches about
// 1.1 KB of a row and uses two thirds of it, and a tile in LDS would stage bytes
// that no second thread reads.  The rows a wave reads are the same four for all
// its lanes (one output row), so every 128-B line fetched is used by the lanes
// around it and comes from L2 at most once per output row.
// Loads: byte loads (global_load_ubyte), for preprocess.hip's reasons -- the
// taps sit at byte offsets 3 x + c of rows with an arbitrary pitch, and no load
// may touch a byte outside [0, 3 sw) of a row.  A tap in the border loads the
// photo's nearest pixel (index clamped, always inside the photo) and selects the
// pad colour afterwards: no divergent branch and no address formed from a
// border coordinate.  48 byte loads and 3 bytes or 3 floats stored per thread;
// 268 324 threads at 518^2.
//
// resize_cubic_f_norm_kernel<T>: the DA-V2 family's native profile, the
// reference's keep-ratio cubic resize of the FLOAT image (core/preprocess.py:
// scale, then ResizeStep("keep_ratio", interp="cubic"), then standardize), read
// straight from the uint8 photo.  The same positions, taps and float32
// coefficients as above (coef4), kept as float32 instead of rounded to 1 / 2048;
// samples T(u) / T(255) from a host-made table; both passes in T = float or
// double, one rounding per product and per sum, left to right; no clamp; then
// (V - mean) / std in float64 and one rounding to float32.  The contract is in
// include/mde.h at mde_op_resize_cubic_f_norm; preprocess.py:resize_cubic_float
// is the numpy restatement the tests hold it to, bit for bit.  Same thread
// mapping and byte loads as the 8-bit kernel, no image tile in LDS: at
// 3024 -> 700 neighbouring outputs share no tap; at ratios near 1 (640 -> 700)
// they share three of four columns and all four rows, and those repeats hit L1
// / L2 (a wave's 64 outputs of one row touch about 4 x 190 contiguous bytes).
// The table is the one thing every thread reads 48 times, so it alone goes to
// LDS (1 or 2 KB per block).
//
// crop_f32_kernel: one thread per destination element, a strided row copy.

#include <hip/hip_runtime.h>

#include "mde_ops.h"

#pragma clang fp contract(off)

namespace mde {
namespace {

struct Coef4 {
  int s;       // first tap, s - 1 of the contract, unclamped
  float c[4];  // float32 weights
};

// position, taps and coefficients of output index d: what the 8-bit and the float resize share
__device__ __forceinline__ Coef4 coef4(int d, double scale) {
  const double pos = __dadd_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), -0.5);
  const float f = __double2float_rn(pos);
  const float fl = floorf(f);
  const float x = __fsub_rn(f, fl);
  constexpr float A = -0.75f;
  Coef4 t;
  const float x1 = __fadd_rn(x, 1.f);
  t.c[0] = __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(A, x1), 5 * A), x1), 8 * A), x1), 4 * A);
  t.c[1] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(A + 2, x), A + 3), x), x), 1.f);
  const float g = __fsub_rn(1.f, x);
  t.c[2] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(A + 2, g), A + 3), g), g), 1.f);
  t.c[3] = __fsub_rn(__fsub_rn(__fsub_rn(1.f, t.c[0]), t.c[1]), t.c[2]);
  t.s = (int)fl - 1;
  return t;
}

struct Tap4 {
  int s;     // first tap, s - 1 of the contract, unclamped
  int k[4];  // 11-bit fixed-point weights
};

__device__ __forceinline__ Tap4 tap4(int d, double scale) {
  const Coef4 q = coef4(d, scale);
  Tap4 t;
  t.s = q.s;
#pragma unroll
  for (int i = 0; i < 4; ++i) t.k[i] = __float2int_rn(__fmul_rn(q.c[i], 2048.f));
  return t;
}

struct CubicGeom {
  int sh, sw, pitch;
  int pad_top, pad_left;
  int ph, pw;  // the virtual image
  int pad[3];  // pad colour in SOURCE channel order
  double scale_y, scale_x;
};

// NORM = false: dst uint8 NHWC [B][oh][ow][3]; true: dst float NCHW [B][3][oh][ow] = lut[c][value]
template <bool NORM>
__global__ void __launch_bounds__(256)
resize_cubic_u8_kernel(const unsigned char* __restrict__ src, CubicGeom g, int swap_rb,
                       const float* __restrict__ lut, void* __restrict__ dst, int oh, int ow) {
  const int plane = oh * ow;  // the ABI wrapper keeps it below 2^31 - 256
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int b = (int)blockIdx.y;
  if (r >= plane) return;
  const int oy = r / ow, ox = r - oy * ow;
  const unsigned char* img = src + (size_t)b * g.sh * g.pitch;
  const Tap4 tx = tap4(ox, g.scale_x);
  const Tap4 ty = tap4(oy, g.scale_y);

  int off[4];     // byte offset of the tap's pixel in a photo row (clamped into the photo)
  bool in_x[4];   // the tap's virtual column lies inside the photo
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int x = min(max(tx.s + i, 0), g.pw - 1) - g.pad_left;
    in_x[i] = x >= 0 && x < g.sw;
    off[i] = 3 * min(max(x, 0), g.sw - 1);
  }
  int v[3] = {0, 0, 0};  // in source channel order
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = min(max(ty.s + j, 0), g.ph - 1) - g.pad_top;
    const bool in_y = y >= 0 && y < g.sh;
    const unsigned char* row = img + (size_t)min(max(y, 0), g.sh - 1) * g.pitch;
    int h[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int s = (int)row[off[i] + c];
        h[c] += ((in_y && in_x[i]) ? s : g.pad[c]) * tx.k[i];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] += h[c] * ty.k[j];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = min(max((v[c] + (1 << 21)) >> 22, 0), 255);
  if (swap_rb) {
    const int t = v[0];
    v[0] = v[2];
    v[2] = t;
  }
  if constexpr (NORM) {
    float* o = reinterpret_cast<float*>(dst) + (size_t)b * 3 * plane + r;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * plane] = lut[c * 256 + v[c]];
  } else {
    unsigned char* o = reinterpret_cast<unsigned char*>(dst) + ((size_t)b * plane + r) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned char)v[c];
  }
}

struct CubicFGeom {
  int sh, sw, pitch;
  double scale_y, scale_x;
  double mean[3], std[3];  // in SOURCE channel order
};

// The DA-V2 family's native profile (include/mde.h, mde_op_resize_cubic_f_norm): cv2's scalar float
// INTER_CUBIC of the photo after its division by 255, working type T, then the standardise in float64
// and one rounding to float32.  T(u) / T(255) comes from a 256-entry table the host made; the block
// copies it to LDS once (one entry per thread), so the 48 lookups of a thread are LDS reads and the
// vector memory path carries the byte taps alone.
template <typename T>
__global__ void __launch_bounds__(256)
resize_cubic_f_norm_kernel(const unsigned char* __restrict__ src, CubicFGeom g, int swap_rb,
                           const T* __restrict__ lut, float* __restrict__ dst, int oh, int ow) {
  __shared__ T lut_s[256];
  lut_s[threadIdx.x] = lut[threadIdx.x];  // blockDim.x == 256
  __syncthreads();
  const int plane = oh * ow;  // the ABI wrapper keeps it below 2^31 - 256
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int b = (int)blockIdx.y;
  if (r >= plane) return;  // after the only barrier
  const int oy = r / ow, ox = r - oy * ow;
  const unsigned char* img = src + (size_t)b * g.sh * g.pitch;
  const Coef4 tx = coef4(ox, g.scale_x);
  const Coef4 ty = coef4(oy, g.scale_y);

  int off[4];  // byte offset of the tap's pixel in a row, clamped into the photo
#pragma unroll
  for (int i = 0; i < 4; ++i) off[i] = 3 * min(max(tx.s + i, 0), g.sw - 1);
  T v[3];  // in source channel order
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned char* row = img + (size_t)min(max(ty.s + j, 0), g.sh - 1) * g.pitch;
    const T bj = (T)ty.c[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // H = ((S0 a0 + S1 a1) + S2 a2) + S3 a3, each product and sum rounded once in T
      T h = lut_s[row[off[0] + c]] * (T)tx.c[0];
      h = h + lut_s[row[off[1] + c]] * (T)tx.c[1];
      h = h + lut_s[row[off[2] + c]] * (T)tx.c[2];
      h = h + lut_s[row[off[3] + c]] * (T)tx.c[3];
      // V = ((H0 b0 + H1 b1) + H2 b2) + H3 b3, the same discipline
      const T p = h * bj;
      v[c] = j == 0 ? p : v[c] + p;
    }
  }
  float* o = dst + (size_t)b * 3 * plane + r;
#pragma unroll
  for (int c = 0; c < 3; ++c)  // source channel c is output channel 2 - c under swap_rb
    o[(size_t)(swap_rb ? 2 - c : c) * plane] =
        __double2float_rn(__ddiv_rn(__dsub_rn((double)v[c], g.mean[c]), g.std[c]));
}

__global__ void __launch_bounds__(256)
crop_f32_kernel(const float* __restrict__ src, int h, int w, int y0, int x0, int ch, int cw,
                float* __restrict__ dst) {
  const int plane = ch * cw;  // <= h * w, which the ABI wrapper keeps below 2^31 - 256
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int b = (int)blockIdx.y;
  if (r >= plane) return;
  const int y = r / cw, x = r - y * cw;
  dst[(size_t)b * plane + r] = src[((size_t)b * h + (y0 + y)) * w + (x0 + x)];
}

}  // namespace

hipError_t launch_resize_cubic_u8(const unsigned char* src, int B, int sh, int sw, int pitch, int swap_rb,
                                  int pad_top, int pad_bottom, int pad_left, int pad_right, const int pad_rgb[3],
                                  const float* lut, void* dst, int oh, int ow, hipStream_t st) {
  CubicGeom g;
  g.sh = sh;
  g.sw = sw;
  g.pitch = pitch;
  g.pad_top = pad_top;
  g.pad_left = pad_left;
  g.ph = pad_top + sh + pad_bottom;
  g.pw = pad_left + sw + pad_right;
  for (int c = 0; c < 3; ++c) g.pad[c] = pad_rgb[swap_rb ? 2 - c : c];
  // cv2: scale = 1.0 / inv_scale with inv_scale = (double)dst / src (two divisions, not src / dst)
  g.scale_x = 1.0 / ((double)ow / (double)g.pw);
  g.scale_y = 1.0 / ((double)oh / (double)g.ph);
  const long long plane = (long long)oh * ow;
  const dim3 grid((unsigned)((plane + 255) / 256), (unsigned)B), block(256);
  if (lut)
    hipLaunchKernelGGL(resize_cubic_u8_kernel<true>, grid, block, 0, st, src, g, swap_rb, lut, dst, oh, ow);
  else
    hipLaunchKernelGGL(resize_cubic_u8_kernel<false>, grid, block, 0, st, src, g, swap_rb, lut, dst, oh, ow);
  return hipGetLastError();
}

hipError_t launch_resize_cubic_f_norm(const unsigned char* src, int B, int sh, int sw, int pitch, int swap_rb,
                                      int wide, const void* lut, const double mean[3], const double stdv[3],
                                      float* dst, int oh, int ow, hipStream_t st) {
  CubicFGeom g;
  g.sh = sh;
  g.sw = sw;
  g.pitch = pitch;
  g.scale_x = 1.0 / ((double)ow / (double)sw);
  g.scale_y = 1.0 / ((double)oh / (double)sh);
  for (int c = 0; c < 3; ++c) {  // given in output channel order
    g.mean[swap_rb ? 2 - c : c] = mean[c];
    g.std[swap_rb ? 2 - c : c] = stdv[c];
  }
  const long long plane = (long long)oh * ow;
  const dim3 grid((unsigned)((plane + 255) / 256), (unsigned)B), block(256);
  if (wide)
    hipLaunchKernelGGL(resize_cubic_f_norm_kernel<double>, grid, block, 0, st, src, g, swap_rb,
                       static_cast<const double*>(lut), dst, oh, ow);
  else
    hipLaunchKernelGGL(resize_cubic_f_norm_kernel<float>, grid, block, 0, st, src, g, swap_rb,
                       static_cast<const float*>(lut), dst, oh, ow);
  return hipGetLastError();
}

hipError_t launch_crop_f32(const float* src, int B, int h, int w, int y0, int x0, int ch, int cw, float* dst,
                           hipStream_t st) {
  const long long plane = (long long)ch * cw;
  const dim3 grid((unsigned)((plane + 255) / 256), (unsigned)B), block(256);
  hipLaunchKernelGGL(crop_f32_kernel, grid, block, 0, st, src, h, w, y0, x0, ch, cw, dst);
  return hipGetLastError();
}

}  // namespace mde
