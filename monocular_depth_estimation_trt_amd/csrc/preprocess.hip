// Device preprocess: OpenCV's 8-bit, 3-channel INTER_LINEAR resize
// (`cv2.resize(img_u8, (ow, oh), interpolation=cv2.INTER_LINEAR)`, the stretch of
// reference core/preprocess.py:resize_stretch), restated from OpenCV's published
// fixed-point algorithm, with the BGR->RGB swap and the /255 + standardise of
// core/preprocess.py:scale/standardize folded into the store.
//
// Contract (the same text as include/mde.h; monocular_depth_estimation_trt_amd/
// preprocess.py:resize_linear_u8 is the independent numpy restatement the tests
// hold this kernel to, bit for bit):
//
//   per axis (dst outputs from src inputs)
//     scale = 1.0 / ((double)dst / (double)src)        float64; NOT src / dst
//     f     = (float)((d + 0.5) * scale - 0.5)         float64, rounded once to float32
//     s     = floor(f);  f -= s                        float32
//   horizontal axis only
//     s <  0         -> s = 0,         f = 0
//     s >= src_w - 1 -> s = src_w - 1, f = 0
//     second tap     = min(s + 1, src_w - 1)
//   vertical axis
//     f is not changed at the borders; both tap rows s and s + 1 are clamped
//     to [0, src_h - 1]
//   coefficients, per axis (two separately rounded float32 products, half to
//   even; they need not sum to 2048)
//     c0 = rint((1.f - f) * 2048.f),  c1 = rint(f * 2048.f)
//   horizontal pass, exact integers
//     H = S[s] * a0 + S[s1] * a1
//   vertical pass
//     out = (((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16) + 2) >> 2   (always 0..255)
//   special case: src_w == 2 dst_w AND src_h == 2 dst_h takes cv2's area path,
//     out = (s00 + s01 + s10 + s11 + 2) >> 2 over the 2x2 block
//     (a 2x ratio on one axis only stays on the linear path)
//
// Rounding discipline: the coordinates and coefficients are computed in the
// kernel, from a `scale` the host computed as a double, with one explicitly
// rounded operation per step (__dadd_rn, __dmul_rn, __fsub_rn, __fmul_rn,
// __float2int_rn).  In-kernel rather than host-built tables because the op
// must only enqueue on the caller's stream (hipGraph capture): tables would
// need an allocation and an upload per shape, or a cache with a lifetime, for
// six fp64 operations a thread.  With this toolchain's headers the _rn forms
// are the plain operators, so what actually forbids the (d + 0.5) * scale - 0.5
// -> fma contraction is that this file is compiled with -ffp-contract=off
// (_build.PER_FILE) and carries the pragma below; nothing else in the
// arithmetic can be reassociated (no fast-math flags in the build).
//
// Loads: the taps sit at byte offsets 3 s + c of rows with an arbitrary pitch,
// so they are byte-granular and unaligned.  Byte loads (global_load_ubyte):
// neighbouring lanes' taps fall into the same or the next 64-B line, which the
// texture path serves from L1/L2 once fetched, and no load can touch a byte
// outside [0, 3 src_w) of a row -- dword loads plus shifts would need two
// dwords per straddling tap and a guard for the last bytes of the image
// (nothing may be read past pitch * src_h).  The kernel reads at most 12
// source bytes and writes 3 bytes or 3 floats per thread; it is bound by
// launch and latency, not by load width (device preprocess).
//
// One thread produces one output pixel, all three channels.

#include <hip/hip_runtime.h>

#include "mde_ops.h"

#pragma clang fp contract(off)

namespace mde {
namespace {

struct Tap {
  int s0, s1;  // source indices of the two taps
  int c0, c1;  // 11-bit fixed-point weights
};

// source coordinate of output index d, as (floor, float32 fraction)
__device__ __forceinline__ void coord(int d, double scale, int& s, float& f) {
  const double x = __dadd_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), -0.5);
  f = __double2float_rn(x);
  const float fl = floorf(f);
  s = (int)fl;
  f = __fsub_rn(f, fl);
}

__device__ __forceinline__ void coeffs(float f, int& c0, int& c1) {
  c0 = __float2int_rn(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
  c1 = __float2int_rn(__fmul_rn(f, 2048.f));
}

__device__ __forceinline__ Tap tap_x(int d, double scale, int sw) {
  int s;
  float f;
  coord(d, scale, s, f);
  if (s < 0) {
    s = 0;
    f = 0.f;
  }
  if (s >= sw - 1) {
    s = sw - 1;
    f = 0.f;
  }
  Tap t;
  t.s0 = s;
  t.s1 = min(s + 1, sw - 1);
  coeffs(f, t.c0, t.c1);
  return t;
}

__device__ __forceinline__ Tap tap_y(int d, double scale, int sh) {
  int s;
  float f;
  coord(d, scale, s, f);
  Tap t;
  t.s0 = min(max(s, 0), sh - 1);
  t.s1 = min(max(s + 1, 0), sh - 1);
  coeffs(f, t.c0, t.c1);
  return t;
}

// NORM = false: dst uint8 NHWC [B][oh][ow][3]; true: dst float NCHW [B][3][oh][ow] = lut[c][value]
template <bool NORM>
__global__ void __launch_bounds__(256)
resize_u8_kernel(const unsigned char* __restrict__ src, int sh, int sw, int pitch, int swap_rb,
                 double scale_y, double scale_x, int area2, const float* __restrict__ lut,
                 void* __restrict__ dst, int oh, int ow) {
  const int plane = oh * ow;  // the launcher keeps it below 2^31 - 256
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int b = (int)blockIdx.y;
  if (r >= plane) return;
  const int oy = r / ow, ox = r - oy * ow;
  const unsigned char* img = src + (size_t)b * sh * pitch;

  int v[3];  // in source channel order
  if (area2) {
    const unsigned char* p0 = img + (size_t)(2 * oy) * pitch + 6 * ox;
    const unsigned char* p1 = p0 + pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ((int)p0[c] + (int)p0[3 + c] + (int)p1[c] + (int)p1[3 + c] + 2) >> 2;
  } else {
    const Tap tx = tap_x(ox, scale_x, sw);
    const Tap ty = tap_y(oy, scale_y, sh);
    const unsigned char* r0 = img + (size_t)ty.s0 * pitch;
    const unsigned char* r1 = img + (size_t)ty.s1 * pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int h0 = (int)r0[3 * tx.s0 + c] * tx.c0 + (int)r0[3 * tx.s1 + c] * tx.c1;
      const int h1 = (int)r1[3 * tx.s0 + c] * tx.c0 + (int)r1[3 * tx.s1 + c] * tx.c1;
      v[c] = (((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
    }
  }
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

}  // namespace

hipError_t launch_resize_u8(const unsigned char* src, int B, int sh, int sw, int pitch, int swap_rb, const float* lut,
                            void* dst, int oh, int ow, hipStream_t st) {
  if (B < 1 || sh < 1 || sw < 1 || oh < 1 || ow < 1 || pitch < 3 * (long long)sw) return hipErrorInvalidValue;
  const long long plane = (long long)oh * ow;
  if (plane > 0x7fffffffLL - 256 || B > 65535) return hipErrorInvalidValue;  // int pixel index; grid.y = batch
  // cv2: scale = 1.0 / inv_scale with inv_scale = (double)dst / src (two divisions, not src / dst)
  const double scale_x = 1.0 / ((double)ow / (double)sw);
  const double scale_y = 1.0 / ((double)oh / (double)sh);
  const int area2 = (sw == 2 * (long long)ow && sh == 2 * (long long)oh) ? 1 : 0;
  const dim3 grid((unsigned)((plane + 255) / 256), (unsigned)B), block(256);
  if (lut)
    hipLaunchKernelGGL(resize_u8_kernel<true>, grid, block, 0, st, src, sh, sw, pitch, swap_rb, scale_y, scale_x,
                       area2, lut, dst, oh, ow);
  else
    hipLaunchKernelGGL(resize_u8_kernel<false>, grid, block, 0, st, src, sh, sw, pitch, swap_rb, scale_y, scale_x,
                       area2, lut, dst, oh, ow);
  return hipGetLastError();
}

}  // namespace mde
