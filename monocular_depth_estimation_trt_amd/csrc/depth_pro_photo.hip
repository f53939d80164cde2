// Depth Pro photo path: the two ends of reference models/depth_pro/onnx2trt.py
// around the engine, on the device.
//
//   dp_preprocess_kernel   :56-74   ToTensor + Normalize(0.5, 0.5) + F.interpolate(bilinear,
//                                   align_corners=False) of a uint8 photo into the engine's
//                                   float32 NCHW "input" binding
//   dp_postprocess_kernel  :118-134 focal length from fov_deg (or given), inverse depth * W / f,
//                                   bilinear (align_corners=False) to the photo's size,
//                                   depth = 1 / clamp(., 1e-4, 1e4)
//
// Contract (the same text as include/mde.h; preprocess.py:resize_bilinear_f32 and
// postprocess.py:depth_pro_postprocess_np are the numpy restatements the tests hold these
// kernels to, bit for bit):
//
//   value of a pixel byte u:  lut[u], a device float[256] the caller passes
//                             (host builds it as ((float32(u) / 255f) - 0.5f) / 0.5f, all float32)
//   per axis (dst outputs from src inputs), every operation rounded to float32 separately, never fused:
//     scale = (float)src / (float)dst
//     x  = scale * ((float)d + 0.5f) - 0.5f;   x = max(x, 0)
//     i0 = min((int)x, src - 1);  i1 = min(i0 + 1, src - 1)
//     l1 = clamp(x - (float)i0, 0, 1);  l0 = 1 - l1
//   out = b0 * (a0 * v00 + a1 * v01) + b1 * (a0 * v10 + a1 * v11)     (a: horizontal, b: vertical)
//
//   post-process:
//     f  = fov_deg ? (0.5f * ow) / tanf(0.5f * (fov_deg[b] * (pi/180))) : f_px
//     k  = (float)ow / f
//     tap value = inv * k                 (rounded, before blending - the reference scales, then resizes)
//     m  = the same bilinear as above, [ih][iw] -> [oh][ow]
//     depth = 1.0f / min(max(m, 1e-4f), 1e4f)        (IEEE division; the build has no fast-math)
//     a NaN m stays NaN, as in torch.clamp (the clamp is two comparisons, not fminf / fmaxf)
//
// Rounding discipline: as in preprocess.hip -- the coordinates and weights are computed in the
// kernel from a `scale` the host divided in float32, one rounded operation per step; the file
// is compiled with -ffp-contract=off (_build.PER_FILE) and carries the pragma below, and no
// fast-math flag is in the build, so nothing is fused or reassociated and the division is
// hipcc's default correctly rounded one.
//
// Pre-process: one thread per output pixel, all three channels; byte loads for the reasons
// given in preprocess.hip (unaligned 3-byte taps, nothing read outside [0, 3 sw) of a row),
// then 12 LUT reads that hit a 1 KiB table.
//
// Post-process: bound by its writes (27 MB for a 2268 x 3024 photo against a 9.4 MB source
// that stays in L2, so the source is read with plain loads and not staged in LDS).  One
// thread produces four consecutive x of one row -- the vertical taps once, the four results
// in one 16-byte store when every row starts 16-byte aligned (ow % 4 == 0 and an aligned
// base; a wave then writes 1 KiB contiguous per instruction), scalar stores otherwise and
// for the tail of a row.  The focal length is wave-uniform: thread 0 of a block computes it
// (one tanf per block rather than per thread) and hands k over through one LDS float.

#include <hip/hip_runtime.h>

#include "mde_ops.h"

#pragma clang fp contract(off)

namespace mde {
namespace {

struct Lin {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Lin axis(int d, float scale, int src) {
  float x = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)d, 0.5f)), 0.5f);
  x = fmaxf(x, 0.f);
  Lin t;
  t.i0 = min((int)x, src - 1);
  t.i1 = min(t.i0 + 1, src - 1);
  t.l1 = fminf(fmaxf(__fsub_rn(x, (float)t.i0), 0.f), 1.f);
  t.l0 = __fsub_rn(1.f, t.l1);
  return t;
}

__device__ __forceinline__ float blend(const Lin& a, const Lin& b, float v00, float v01, float v10, float v11) {
  const float top = __fadd_rn(__fmul_rn(a.l0, v00), __fmul_rn(a.l1, v01));
  const float bot = __fadd_rn(__fmul_rn(a.l0, v10), __fmul_rn(a.l1, v11));
  return __fadd_rn(__fmul_rn(b.l0, top), __fmul_rn(b.l1, bot));
}

__global__ void __launch_bounds__(256)
dp_preprocess_kernel(const unsigned char* __restrict__ src, int sh, int sw, int pitch, int swap_rb, float scale_y,
                     float scale_x, const float* __restrict__ lut, float* __restrict__ dst, int oh, int ow) {
  const int plane = oh * ow;  // the ABI wrapper keeps it below 2^31 - 256
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int b = (int)blockIdx.y;
  if (r >= plane) return;
  const int oy = r / ow, ox = r - oy * ow;
  const Lin tx = axis(ox, scale_x, sw);
  const Lin ty = axis(oy, scale_y, sh);
  const unsigned char* img = src + (size_t)b * sh * pitch;
  const unsigned char* r0 = img + (size_t)ty.i0 * pitch;
  const unsigned char* r1 = img + (size_t)ty.i1 * pitch;
  float* o = dst + (size_t)b * 3 * plane + r;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sc = swap_rb ? 2 - c : c;  // source channel of output channel c
    const float v = blend(tx, ty, lut[r0[3 * tx.i0 + sc]], lut[r0[3 * tx.i1 + sc]], lut[r1[3 * tx.i0 + sc]],
                          lut[r1[3 * tx.i1 + sc]]);
    o[(size_t)c * plane] = v;
  }
}

// VEC: every row of `out` starts 16-byte aligned and ow % 4 == 0
template <bool VEC>
__global__ void __launch_bounds__(256)
dp_postprocess_kernel(const float* __restrict__ inv, int ih, int iw, float scale_y, float scale_x,
                      const float* __restrict__ fov_deg, float f_px, float* __restrict__ f_px_out,
                      float* __restrict__ out, int oh, int ow, int groups) {
  __shared__ float s_k;
  const int b = (int)blockIdx.y;
  if (threadIdx.x == 0) {
    float f = f_px;
    if (fov_deg) {
      const float rad = __fmul_rn(fov_deg[b], 0.017453292519943295f);  // float32(pi / 180), torch.deg2rad
      f = __fdiv_rn(__fmul_rn(0.5f, (float)ow), tanf(__fmul_rn(0.5f, rad)));
    }
    if (f_px_out && blockIdx.x == 0) f_px_out[b] = f;
    s_k = __fdiv_rn((float)ow, f);
  }
  __syncthreads();
  const float k = s_k;
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);  // (row, group of 4 columns)
  if (r >= oh * groups) return;  // oh * groups <= oh * ow: below 2^31 - 256
  const int oy = r / groups, x0 = (r - oy * groups) * 4;
  const Lin ty = axis(oy, scale_y, ih);
  const float* img = inv + (size_t)b * ih * iw;
  const float* r0 = img + (size_t)ty.i0 * iw;
  const float* r1 = img + (size_t)ty.i1 * iw;
  float d[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = min(x0 + j, ow - 1);  // past the row's end: a valid tap, never stored
    const Lin tx = axis(ox, scale_x, iw);
    const float m = blend(tx, ty, __fmul_rn(r0[tx.i0], k), __fmul_rn(r0[tx.i1], k), __fmul_rn(r1[tx.i0], k),
                          __fmul_rn(r1[tx.i1], k));
    // torch.clamp, not fminf(fmaxf()): the comparisons are false for a NaN, which so stays NaN
    const float cl = m < 1e-4f ? 1e-4f : (m > 1e4f ? 1e4f : m);
    d[j] = __fdiv_rn(1.0f, cl);
  }
  float* o = out + (size_t)b * oh * ow + (size_t)oy * ow + x0;
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(o) = make_float4(d[0], d[1], d[2], d[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < ow) o[j] = d[j];
  }
}

}  // namespace

// The launchers check nothing: their one caller each, the ABI wrapper in engine.hip, has
// refused null pointers, non-positive sizes, pitch < 3 sw, planes of 2^31 - 256 elements or
// more (int pixel index in the kernels), batch > 65535 (grid.y) and a missing focal length
// before it gets here.
hipError_t launch_dp_preprocess(const unsigned char* src, int B, int sh, int sw, int pitch, int swap_rb,
                                const float* lut, float* dst, int oh, int ow, hipStream_t st) {
  const float scale_y = (float)sh / (float)oh, scale_x = (float)sw / (float)ow;
  const long long plane = (long long)oh * ow;
  const dim3 grid((unsigned)((plane + 255) / 256), (unsigned)B), block(256);
  hipLaunchKernelGGL(dp_preprocess_kernel, grid, block, 0, st, src, sh, sw, pitch, swap_rb, scale_y, scale_x, lut, dst,
                     oh, ow);
  return hipGetLastError();
}

hipError_t launch_dp_postprocess(const float* inv, int B, int ih, int iw, const float* fov_deg, float f_px,
                                 float* f_px_out, float* out, int oh, int ow, hipStream_t st) {
  const float scale_y = (float)ih / (float)oh, scale_x = (float)iw / (float)ow;
  const int groups = (ow + 3) / 4;
  const long long n = (long long)oh * groups;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)B), block(256);
  const bool vec = (ow % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
  if (vec)
    hipLaunchKernelGGL(dp_postprocess_kernel<true>, grid, block, 0, st, inv, ih, iw, scale_y, scale_x, fov_deg, f_px,
                       f_px_out, out, oh, ow, groups);
  else
    hipLaunchKernelGGL(dp_postprocess_kernel<false>, grid, block, 0, st, inv, ih, iw, scale_y, scale_x, fov_deg, f_px,
                       f_px_out, out, oh, ow, groups);
  return hipGetLastError();
}

}  // namespace mde
