// Colour frames: the closing lines of the reference drivers (models/depth_pro/onnx2trt.py:156-168,
// models/depth_anything_v2/onnx2trt.py:131-150, models/vggt/onnx2trt.py:122-142, core/viz.py:colorize),
// on the device.  A depth map at the photo's size (what depth_postprocess / dp_postprocess leave in
// device memory) becomes a uint8 [h][w][3] picture through a 257-entry colour table; 3 bytes per pixel
// come back instead of 4.
//
// Contract: include/mde.h, mde_op_depth_colorize (visualize.py:colorize_np is the numpy restatement the
// tests hold these kernels to, byte for byte).  Modes 0 and 1 are float32 with one rounding per
// operation, mode 2 is float64 -- -ffp-contract=off for the file (_build.PER_FILE) and the pragma
// below, IEEE division spelled out, no fast-math flag in the build.
//
// Structure.  Modes 0 and 1 range every image on its own, so they take three launches, mode 2 one:
//   dc_range_partials   a workgroup of 256 threads owns MDE_DEPTH_COLORIZE_TILE = 4096 consecutive
//                       pixels of one image and writes the min and max of its finite values to ws
//   dc_range_finalize   one workgroup per image folds the partials and writes {lo, d} to ws and
//                       {lo, hi} to range_out
//   dc_color            the table look-up, below
// mde_op_depth_colorize_ranged is the colour pass as template mode 3: mode 2's float64 lines on an axis
// that each image reads from device memory (the rows of mde_op_depth_quantiles), one or two launches.
// Min and max do not depend on the order they are taken in, no workgroup waits on another's writes and
// there are no floating-point atomics: the same bytes on every run.
//
// The colour pass works on the flat pixel index g = b * h * w + p, so that a batch is one stream of
// 4-byte reads and 3-byte writes.  A thread takes 16 consecutive pixels: four 16-byte loads, three
// 16-byte stores (a dword store costs about six times, a short store twelve times the dwordx4 time per
// byte).  The first group starts at pixel `head`, the one offset in 0..15 at which the output address
// is 16-byte aligned (3 * head = -out mod 16, 3 * 11 = 1 mod 16); the vector path is taken when the
// map's address is aligned there too, else every pixel takes the scalar path, as the `head` pixels
// before the first group and the fewer than 16 after the last do.  A group that runs over an image's
// end reloads {lo, d} at the pixel where the next image starts.  The table sits in LDS as 257 dwords
// (R, G, B or B, G, R in the low three bytes): one ds_read_b32 per pixel at an index that neighbours
// mostly share, and the twelve output dwords are shifts and ors of sixteen of them.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mde.h"
#include "mde_ops.h"

#pragma clang fp contract(off)

namespace mde {
namespace {

constexpr int kThreads = 256;                  // 4 waves of 64
constexpr int kPasses = 4;                     // float4 loads per thread in the range pass
constexpr int kTile = kThreads * 4 * kPasses;  // pixels per workgroup in the range pass
constexpr int kGroup = 16;                     // pixels per thread in the colour pass
constexpr int kLut = 257;                      // 256 colours and the bad colour
constexpr unsigned kMaxBlocks = 1u << 20;      // the colour pass strides over what is beyond

static_assert(kTile == MDE_DEPTH_COLORIZE_TILE, "the tile is part of the contract (include/mde.h)");

__device__ __forceinline__ bool finite_f(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

// what is ranged: inverse depth in mode 0, the map itself in mode 1
__device__ __forceinline__ float ranged_value(float x, int mode, int inverse) {
  return (mode == 0 && !inverse) ? __fdiv_rn(1.0f, x) : x;
}

// min and max over the workgroup; valid in thread 0.  s: 2 * (kThreads / 64) floats of LDS
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* s) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const float a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  const int t = (int)threadIdx.x;
  if ((t & 63) == 0) s[2 * (t >> 6)] = mn, s[2 * (t >> 6) + 1] = mx;
  __syncthreads();
  if (t == 0) {
    for (int k = 1; k < kThreads / 64; ++k) {
      mn = s[2 * k] < mn ? s[2 * k] : mn;
      mx = s[2 * k + 1] > mx ? s[2 * k + 1] : mx;
    }
  }
}

// part[b][tile] = {min, max} of the tile's finite values; {+inf, -inf} when it has none
__global__ void __launch_bounds__(kThreads)
dc_range_partials(const float* __restrict__ map, unsigned plane, int tiles, int mode, int inverse,
                  float* __restrict__ part) {
  __shared__ float s[2 * (kThreads / 64)];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const float* im = map + (size_t)b * plane;
  const bool vec = (reinterpret_cast<uintptr_t>(im) & 15) == 0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
    // unsigned: the last tile's indices run up to kTile - 1 past the plane, which is below 2^31 - 256
    const unsigned i0 = blockIdx.x * (unsigned)kTile + (unsigned)(pass * kThreads * 4 + t * 4);
    float x[4];
    bool in[4];
    if (vec && i0 + 4u <= plane) {
      const float4 q = *reinterpret_cast<const float4*>(im + i0);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
      in[0] = in[1] = in[2] = in[3] = true;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        in[j] = i0 + (unsigned)j < plane;
        x[j] = in[j] ? im[i0 + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = ranged_value(x[j], mode, inverse);
      if (in[j] && finite_f(v)) {
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
      }
    }
  }
  block_minmax(mn, mx, s);
  if (t == 0) {
    float* o = part + ((size_t)b * tiles + blockIdx.x) * 2;
    o[0] = mn, o[1] = mx;
  }
}

// params[b] = {lo, d}, range_out[b] = {lo, hi}.  d_both: mode 0's denominator when both ends clip
__global__ void __launch_bounds__(kThreads)
dc_range_finalize(const float* __restrict__ part, int tiles, int mode, float eps, float d_both,
                  float* __restrict__ params, float* __restrict__ range_out) {
  __shared__ float s[2 * (kThreads / 64)];
  const int b = (int)blockIdx.x;
  const float* p = part + (size_t)b * tiles * 2;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int i = (int)threadIdx.x; i < tiles; i += kThreads) {
    mn = p[2 * i] < mn ? p[2 * i] : mn;
    mx = p[2 * i + 1] > mx ? p[2 * i + 1] : mx;
  }
  block_minmax(mn, mx, s);
  if (threadIdx.x != 0) return;
  float lo, hi, d;
  if (mn > mx) {  // no finite value at all
    lo = hi = d = __builtin_nanf("");
  } else if (mode == 0) {
    const float c = (float)(1.0 / 250);
    lo = mn > c ? mn : c;
    hi = mx < 10.0f ? mx : 10.0f;
    d = (mx > 10.0f && mn <= c) ? d_both : __fadd_rn(__fsub_rn(hi, lo), eps);
  } else {
    lo = mn, hi = mx;
    d = __fsub_rn(mx, mn);
  }
  params[2 * b] = lo, params[2 * b + 1] = d;
  if (range_out) range_out[2 * b] = lo, range_out[2 * b + 1] = hi;
}

// mode 2 ranges nothing: the given axis, as it was used
__global__ void dc_range_fixed(float lo, float hi, int B, float* __restrict__ range_out) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b < B) range_out[2 * b] = lo, range_out[2 * b + 1] = hi;
}

struct ColorArgs {
  const float* map;
  unsigned char* out;
  const unsigned char* lut;  // uchar[257][3], R, G, B
  const float* params;       // {lo, d} per image (modes 0 and 1)
  unsigned plane;
  int inverse, swap_rb;
  double vmin, den;          // mode 2: t = (x - vmin) / den
  const double* range;       // mode 3 (ranged): image b's {vmin, vmax} at range[b * range_stride]
  int range_stride, positive_only, reciprocal;
};

// mode 3's axis of image b, with mode 2's rule for an empty one
__device__ __forceinline__ void ranged_axis(const ColorArgs& a, long long b, double& vmin, double& den) {
  const double* r = a.range + b * a.range_stride;
  double vmax = r[1];
  vmin = r[0];
  if (vmax <= vmin) vmax = vmin + 1e-6;
  den = vmax - vmin;
}

// the table index of one pixel; lo, d: this image's (modes 0 and 1); vmin, den: the axis (modes 2 and 3)
template <int MODE>
__device__ __forceinline__ int pixel_index(float x, float lo, float d, double vmin, double den, const ColorArgs& a) {
  if (MODE >= 2) {
    if (!finite_f(x)) return 256;
    double y = (double)x;
    if (MODE == 3) {
      if (a.positive_only && !(x > 0.f)) return 256;
      if (a.reciprocal) y = 1.0 / y;
    }
    double t = (y - vmin) / den;
    if (t != t) return 256;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const int i = (int)(t * 256.0);
    return i > 255 ? 255 : i;
  }
  const float top = MODE == 0 ? 256.0f : 255.0f;
  const float v = ranged_value(x, MODE, a.inverse);
  const float t = __fmul_rn(__fdiv_rn(__fsub_rn(v, lo), d), top);
  if (t != t) return 256;
  if (t < 0.f) return 0;
  if (t >= top) return 255;
  return (int)t;
}

// s_lut[i] = the three bytes of entry i in output order, low byte first
__device__ __forceinline__ void load_lut(const ColorArgs& a, unsigned* s_lut) {
  for (int i = (int)threadIdx.x; i < kLut; i += (int)blockDim.x) {
    const unsigned r = a.lut[3 * i], g = a.lut[3 * i + 1], b = a.lut[3 * i + 2];
    s_lut[i] = a.swap_rb ? (b | (g << 8) | (r << 16)) : (r | (g << 8) | (b << 16));
  }
  __syncthreads();
}

// groups [0, ngroups) of 16 pixels from flat pixel `head`: map + head and out + 3 * head are 16-byte
// aligned, head + 16 * ngroups <= batch * plane
template <int MODE>
__global__ void __launch_bounds__(kThreads)
dc_color(ColorArgs a, long long head, long long ngroups) {
  __shared__ unsigned s_lut[kLut];
  load_lut(a, s_lut);
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long grp = (long long)blockIdx.x * kThreads + threadIdx.x; grp < ngroups; grp += stride) {
    const long long g0 = head + grp * kGroup;
    const float4* src = reinterpret_cast<const float4*>(a.map + g0);
    float x[kGroup];
#pragma unroll
    for (int k = 0; k < kGroup / 4; ++k) {
      const float4 q = src[k];
      x[4 * k] = q.x, x[4 * k + 1] = q.y, x[4 * k + 2] = q.z, x[4 * k + 3] = q.w;
    }
    long long b = g0 / a.plane;
    unsigned p = (unsigned)(g0 - b * a.plane);
    float lo = 0.f, d = 0.f;
    double vmin = a.vmin, den = a.den;
    if (MODE < 2) lo = a.params[2 * b], d = a.params[2 * b + 1];
    if (MODE == 3) ranged_axis(a, b, vmin, den);
    unsigned c[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      if (MODE != 2 && p == a.plane) {  // the next image starts inside the group
        p = 0, ++b;
        if (MODE < 2) lo = a.params[2 * b], d = a.params[2 * b + 1];
        if (MODE == 3) ranged_axis(a, b, vmin, den);
      }
      c[j] = s_lut[pixel_index<MODE>(x[j], lo, d, vmin, den, a)];
      ++p;
    }
    uint4* dst = reinterpret_cast<uint4*>(a.out + 3 * g0);
    unsigned w[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w[3 * q] = c[4 * q] | (c[4 * q + 1] << 24);
      w[3 * q + 1] = (c[4 * q + 1] >> 8) | (c[4 * q + 2] << 16);
      w[3 * q + 2] = (c[4 * q + 2] >> 16) | (c[4 * q + 3] << 8);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
  }
}

// flat pixels [s0, s0 + n0) and [s1, s1 + n1), one at a time
template <int MODE>
__global__ void __launch_bounds__(kThreads)
dc_color_scalar(ColorArgs a, long long s0, long long n0, long long s1, long long n1) {
  __shared__ unsigned s_lut[kLut];
  load_lut(a, s_lut);
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n0 + n1; i += stride) {
    const long long g = i < n0 ? s0 + i : s1 + (i - n0);
    float lo = 0.f, d = 0.f;
    double vmin = a.vmin, den = a.den;
    if (MODE != 2) {
      const long long b = g / a.plane;
      if (MODE < 2) lo = a.params[2 * b], d = a.params[2 * b + 1];
      if (MODE == 3) ranged_axis(a, b, vmin, den);
    }
    const unsigned c = s_lut[pixel_index<MODE>(a.map[g], lo, d, vmin, den, a)];
    unsigned char* o = a.out + 3 * g;
    o[0] = (unsigned char)c, o[1] = (unsigned char)(c >> 8), o[2] = (unsigned char)(c >> 16);
  }
}

unsigned blocks_for(long long n) {
  const long long need = (n + kThreads - 1) / kThreads;
  return (unsigned)(need < (long long)kMaxBlocks ? need : (long long)kMaxBlocks);
}

template <int MODE>
void launch_color(const ColorArgs& a, long long total, hipStream_t st) {
  // the one pixel offset in 0..15 at which out + 3 * head is 16-byte aligned
  const long long head = (long long)(((16 - (reinterpret_cast<uintptr_t>(a.out) & 15)) * 11) & 15);
  const bool vec = ((reinterpret_cast<uintptr_t>(a.map) + 4 * (uintptr_t)head) & 15) == 0 && total >= head + kGroup;
  if (!vec) {
    hipLaunchKernelGGL(dc_color_scalar<MODE>, dim3(blocks_for(total)), dim3(kThreads), 0, st, a, 0LL, total, 0LL, 0LL);
    return;
  }
  const long long ngroups = (total - head) / kGroup;
  const long long tail = head + ngroups * kGroup;
  hipLaunchKernelGGL(dc_color<MODE>, dim3(blocks_for(ngroups)), dim3(kThreads), 0, st, a, head, ngroups);
  if (head + (total - tail) > 0)
    hipLaunchKernelGGL(dc_color_scalar<MODE>, dim3(1), dim3(kThreads), 0, st, a, 0LL, head, tail, total - tail);
}

int tiles_of(int h, int w) { return (int)(((long long)h * w + kTile - 1) / kTile); }

}  // namespace

size_t depth_colorize_ws_bytes(int B, int h, int w) {
  return ((size_t)B * tiles_of(h, w) * 2 + (size_t)B * 2) * sizeof(float);
}

// Checks nothing: the one caller, mde_op_depth_colorize in ops_abi.hip, has refused null pointers,
// non-positive sizes, a mode outside 0..2, NaN denom_eps or bounds, a plane of 2^31 - 256 pixels or
// more (unsigned pixel index plus a tile), batch > 65535 (grid.y) and a short or misaligned workspace.
hipError_t launch_depth_colorize(const float* map, int B, int h, int w, int mode, int map_is_inverse, double denom_eps,
                                 double vmin, double vmax, const unsigned char* lut, int swap_rb, unsigned char* out,
                                 float* range_out, void* ws, hipStream_t st) {
  ColorArgs a;
  a.map = map, a.out = out, a.lut = lut, a.params = nullptr;
  a.plane = (unsigned)h * (unsigned)w;
  a.inverse = map_is_inverse, a.swap_rb = swap_rb;
  a.vmin = 0.0, a.den = 1.0;
  a.range = nullptr, a.range_stride = 0, a.positive_only = 0, a.reciprocal = 0;
  const long long total = (long long)B * a.plane;
  if (mode == 2) {
    if (vmax <= vmin) vmax = vmin + 1e-6;
    a.vmin = vmin, a.den = vmax - vmin;
    if (range_out)
      hipLaunchKernelGGL(dc_range_fixed, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                         (float)vmin, (float)vmax, B, range_out);
    launch_color<2>(a, total, st);
    return hipGetLastError();
  }
  const int tiles = tiles_of(h, w);
  float* part = static_cast<float*>(ws);
  float* params = part + (size_t)B * tiles * 2;
  a.params = params;
  const float d_both = (float)(10.0 - 1.0 / 250 + denom_eps);  // summed in double, one rounding
  hipLaunchKernelGGL(dc_range_partials, dim3((unsigned)tiles, (unsigned)B), dim3(kThreads), 0, st, map, a.plane, tiles,
                     mode, map_is_inverse, part);
  hipLaunchKernelGGL(dc_range_finalize, dim3((unsigned)B), dim3(kThreads), 0, st, part, tiles, mode, (float)denom_eps,
                     d_both, params, range_out);
  if (mode == 0)
    launch_color<0>(a, total, st);
  else
    launch_color<1>(a, total, st);
  return hipGetLastError();
}

// Checks nothing: the one caller, mde_op_depth_colorize_ranged in ops_abi.hip, has refused null pointers,
// non-positive sizes, a negative range_stride, a misaligned range, a plane of 2^31 - 256 pixels or more
// and batch > 65535.
hipError_t launch_depth_colorize_ranged(const float* map, int B, int h, int w, int positive_only, int reciprocal,
                                        const double* range, int range_stride, const unsigned char* lut, int swap_rb,
                                        unsigned char* out, hipStream_t st) {
  ColorArgs a;
  a.map = map, a.out = out, a.lut = lut, a.params = nullptr;
  a.plane = (unsigned)h * (unsigned)w;
  a.inverse = 0, a.swap_rb = swap_rb;
  a.vmin = 0.0, a.den = 1.0;
  a.range = range, a.range_stride = range_stride, a.positive_only = positive_only, a.reciprocal = reciprocal;
  launch_color<3>(a, (long long)B * a.plane, st);
  return hipGetLastError();
}

}  // namespace mde
