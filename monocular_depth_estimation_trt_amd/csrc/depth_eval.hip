// Depth evaluation: the per-image call sequence of reference tools/evaluate_gt.py:555-583 over
// core/gt.py (orientation :125-149, align :31-91, metrics :94-122), on the device.  A predicted depth
// map at the photo's size (what depth_postprocess / dp_postprocess leave in device memory) is scored
// against measured ground truth and a validity mask; 16 doubles per image come back.
//
// Contract: include/mde.h, mde_op_depth_eval (evaluate.py:score_np is the numpy float64 restatement
// the tests hold these kernels to).  Every per-pixel operation is float64 with one rounding per
// operation -- -ffp-contract=off for the file (_build.PER_FILE) and the pragma below, no fast-math
// flag in the build: x * s + t rounds twice, as numpy does.
//
// Structure.  A workgroup of 128 threads (2 waves) owns MDE_DEPTH_EVAL_TILE = 1024 consecutive pixels
// of one image, whatever the grid or the card; thread t takes pixels 4t .. 4t + 3 and 512 + 4t ..
// 512 + 4t + 3 of the tile (one float4 of each map and one dword of the mask per pass: a wave reads 1 KiB
// contiguous per load).  Four launches on the stream, no host read in between:
//   de_fit_partials      ws fit[b][tile][12]  = the tile's sums for the orientation and the fit
//   de_fit_finalize      one workgroup per image adds the partials in a fixed order, writes status,
//                        n_fit, scale, shift, orientation, n_mask to out[b] (and zeros to out[b][13..15])
//   de_metric_partials   reads status, scale, shift from out[b]; ws met[b][tile][8] = metric sums
//   de_metric_finalize   one workgroup per image: n, abs_rel, rmse, log10, delta1..3 to out[b]
// No workgroup ever waits on memory another workgroup writes (the order between the steps is the
// stream's) and there are no floating-point atomics: the order of every addition is fixed by the
// pixel's index alone, so the 128 bytes per image are the same on every run and every card.
//
// Order of additions.  In a thread: its 8 pixels in index order.  In a wave: a DPP butterfly inside
// each row of 16 lanes (quad_perm xor 1, xor 2, row_half_mirror, row_mirror -- IEEE addition is
// commutative, so every lane of the row ends with the same bits), the four row sums to LDS.  In the
// workgroup: thread k adds the rows' values of sum k in row order.  In the finalising workgroup: thread
// t adds tiles t, t + 256, ... in order, then the same row butterfly and the 16 rows in order.
//
// The pixel count per thread: fp64 VALU issues a wave64 operation in 4 cycles here, a 64-bit DPP move
// is two 32-bit ones, so the row butterfly of the fit launch's 12 sums plus the LDS step is about 270
// issue slots per wave.  At
// 8 pixels per lane the fit's arithmetic (two IEEE divisions per pixel under scale_shift) is of the
// same order, the metric kernel's (three divisions, two log10) several times that; 4 pixels per lane
// would leave the fit launch reduction-bound, 16 would give a 768 x 1024 map fewer workgroups than
// the chip has CUs.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mde.h"
#include "mde_ops.h"

#pragma clang fp contract(off)

namespace mde {
namespace {

constexpr int kThreads = 128;                 // 2 waves of 64
constexpr int kPasses = 2;                    // float4 loads per map and thread
constexpr int kTile = kThreads * 4 * kPasses; // pixels per workgroup
constexpr int kFinThreads = 256;              // the finalising workgroup
constexpr int kFitSums = 12;                  // doubles per tile in ws, listed below
constexpr int kMetSums = 8;                   // doubles per tile in ws, listed below

static_assert(kTile == MDE_DEPTH_EVAL_TILE, "the tile is part of the contract (include/mde.h)");
static_assert(kThreads % 64 == 0 && kFinThreads % 64 == 0, "the row butterfly is over whole wave64s");

// fit[b][tile][.]: 0 n_o, 1 Sa, 2 Sb, 3 Saa, 4 Sbb, 5 Sab (orientation: a = pred, b = gt over m && finite(pred))
//                  6 n_fit, 7..10 the fit's sums (scale: Spg, Spp; scale_shift: Sx, Sy, Sxx, Sxy), 11 n_mask (m)
// met[b][tile][.]: 0 n, 1 S|p-g|/g, 2 S(p-g)^2, 3 S|log10 p - log10 g|, 4..6 counts ratio < 1.25^k, 7 = 0
// counts are exact in a double (a plane has fewer than 2^31 pixels)

template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// the sum of v over the 16 lanes of this lane's DPP row, the same bits in all 16; whole waves only
__device__ __forceinline__ double row_sum(double v) {
  v += dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp<0x141>(v);  // row_half_mirror: the other quad of the 8
  v += dpp<0x140>(v);  // row_mirror: the other 8 of the 16
  return v;
}

// sums v[0 .. N) over the workgroup of THREADS threads in the fixed order above; thread k < N returns
// sum k, the others 0.  s_rows: N * (THREADS / 16) doubles of LDS, free to reuse after the call.
template <int N, int THREADS>
__device__ __forceinline__ double block_sum(const double (&v)[N], double* s_rows) {
  constexpr int kRows = THREADS / 16;
  const int t = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double r = row_sum(v[k]);
    if ((t & 15) == 0) s_rows[k * kRows + (t >> 4)] = r;
  }
  __syncthreads();
  double s = 0.0;
  if (t < N) {
    s = s_rows[t * kRows];
    for (int r = 1; r < kRows; ++r) s += s_rows[t * kRows + r];
  }
  __syncthreads();
  return s;
}

struct Quad {
  float p[4], g[4];
  bool m[4];  // mask != 0, false past the image's end
};

// pixels i0 .. i0 + 3 of one image (i0 a multiple of 4; unsigned: the last tile's indices run up to
// kTile - 1 past the plane, which the wrapper keeps below 2^31 - 256).  vec: the three image bases
// are aligned for a 16-byte / 4-byte access at every multiple of 4.
__device__ __forceinline__ Quad load_quad(const float* __restrict__ pred, const float* __restrict__ gt,
                                          const unsigned char* __restrict__ mask, unsigned i0, unsigned plane,
                                          bool vec) {
  Quad q;
  if (vec && i0 + 4u <= plane) {
    const float4 p = *reinterpret_cast<const float4*>(pred + i0);
    const float4 g = *reinterpret_cast<const float4*>(gt + i0);
    const unsigned m = *reinterpret_cast<const unsigned*>(mask + i0);
    q.p[0] = p.x, q.p[1] = p.y, q.p[2] = p.z, q.p[3] = p.w;
    q.g[0] = g.x, q.g[1] = g.y, q.g[2] = g.z, q.g[3] = g.w;
#pragma unroll
    for (int j = 0; j < 4; ++j) q.m[j] = ((m >> (8 * j)) & 0xffu) != 0u;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = i0 + (unsigned)j < plane;
      q.p[j] = in ? pred[i0 + j] : 0.f;
      q.g[j] = in ? gt[i0 + j] : 0.f;
      q.m[j] = in && mask[i0 + j] != 0;
    }
  }
  return q;
}

__device__ __forceinline__ bool finite_f(float x) { return __builtin_fabsf(x) < __builtin_inff(); }
__device__ __forceinline__ bool finite_d(double x) { return __builtin_fabs(x) < __builtin_inf(); }

struct Image {
  const float* pred;
  const float* gt;
  const unsigned char* mask;
  bool vec;
};

__device__ __forceinline__ Image image_of(const float* pred, const float* gt, const unsigned char* mask, int b,
                                          unsigned plane) {
  Image im;
  im.pred = pred + (size_t)b * plane;
  im.gt = gt + (size_t)b * plane;
  im.mask = mask + (size_t)b * plane;
  im.vec = ((reinterpret_cast<uintptr_t>(im.pred) | reinterpret_cast<uintptr_t>(im.gt)) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(im.mask) & 3) == 0;
  return im;
}

__global__ void __launch_bounds__(kThreads)
de_fit_partials(const float* __restrict__ pred, const float* __restrict__ gt, const unsigned char* __restrict__ mask,
                unsigned plane, int tiles, int policy, int inverse, int finite_only, double* __restrict__ fit) {
  __shared__ double s_rows[kFitSums * (kThreads / 16)];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const Image im = image_of(pred, gt, mask, b, plane);
  double v[kFitSums];
#pragma unroll
  for (int k = 0; k < kFitSums; ++k) v[k] = 0.0;
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
    const unsigned i0 = blockIdx.x * (unsigned)kTile + (unsigned)(pass * kThreads * 4 + t * 4);
    const Quad q = load_quad(im.pred, im.gt, im.mask, i0, plane, im.vec);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool m = q.m[j] && q.g[j] > 0.f;
      const bool fin = finite_f(q.p[j]);
      const double a = (double)q.p[j], g = (double)q.g[j];
      if (m) v[11] += 1.0;
      if (m && fin) {
        v[0] += 1.0;
        v[1] += a;
        v[2] += g;
        v[3] += a * a;
        v[4] += g * g;
        v[5] += a * g;
      }
      if (policy == 1) {
        if (m && (fin || !finite_only)) {
          v[6] += 1.0;
          v[7] += a * g;
          v[8] += a * a;
        }
      } else if (policy == 2) {
        if (m && fin && (inverse || q.p[j] > 0.f)) {
          const double x = inverse ? a : 1.0 / a;
          const double y = 1.0 / g;
          v[6] += 1.0;
          v[7] += x;
          v[8] += y;
          v[9] += x * x;
          v[10] += x * y;
        }
      }
    }
  }
  const double s = block_sum<kFitSums, kThreads>(v, s_rows);
  if (t < kFitSums) fit[((size_t)b * tiles + blockIdx.x) * kFitSums + t] = s;
}

// thread t's sum of column k over tiles t, t + kFinThreads, ...
template <int N>
__device__ __forceinline__ void gather_tiles(const double* __restrict__ part, int tiles, double (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.0;
  for (int i = (int)threadIdx.x; i < tiles; i += kFinThreads) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += part[(size_t)i * N + k];
  }
}

__global__ void __launch_bounds__(kFinThreads)
de_fit_finalize(const double* __restrict__ fit, int tiles, int policy, double* __restrict__ out) {
  __shared__ double s_rows[kFitSums * (kFinThreads / 16)];
  __shared__ double s_sum[kFitSums];
  const int b = (int)blockIdx.x, t = (int)threadIdx.x;
  double v[kFitSums];
  gather_tiles<kFitSums>(fit + (size_t)b * tiles * kFitSums, tiles, v);
  const double s = block_sum<kFitSums, kFinThreads>(v, s_rows);
  if (t < kFitSums) s_sum[t] = s;
  __syncthreads();
  if (t != 0) return;
  const double nan = __builtin_nan("");
  double* o = out + (size_t)b * 16;

  // orientation: Pearson in the reference's uncentred form
  double orient = nan;
  const double n = s_sum[0];
  if (n >= 2.0) {
    const double sa = s_sum[1], sb = s_sum[2];
    const double saa = s_sum[3] - sa * sa / n;
    const double sbb = s_sum[4] - sb * sb / n;
    if (!(saa <= 0.0 || sbb <= 0.0)) {
      const double sab = s_sum[5] - sa * sb / n;
      orient = sab / sqrt(saa * sbb);
    }
  }

  double status = 0.0, scale = nan, shift = nan, n_fit = 0.0;
  if (policy != 0) {
    n_fit = s_sum[6];
    if (n_fit < 2.0) {
      status = 1.0;
    } else if (policy == 1) {
      const double spg = s_sum[7], spp = s_sum[8];
      scale = spg / (1e-12 > spp ? 1e-12 : spp);  // Python's max(spp, 1e-12): a NaN spp stays
    } else {
      const double sx = s_sum[7], sy = s_sum[8], sxx = s_sum[9], sxy = s_sum[10];
      const double denom = n_fit * sxx - sx * sx;
      if (__builtin_fabs(denom) < 1e-12) {
        status = 2.0;
      } else {
        scale = (n_fit * sxy - sx * sy) / denom;
        shift = (sy - scale * sx) / n_fit;
      }
    }
  }
  o[0] = status;
  o[1] = n_fit;
  o[2] = scale;
  o[3] = shift;
  o[11] = orient;
  o[12] = s_sum[11];
  o[13] = o[14] = o[15] = 0.0;
}

__global__ void __launch_bounds__(kThreads)
de_metric_partials(const float* __restrict__ pred, const float* __restrict__ gt,
                   const unsigned char* __restrict__ mask, unsigned plane, int tiles, int policy, int inverse,
                   float max_depth, const double* __restrict__ out, double* __restrict__ met) {
  __shared__ double s_rows[kMetSums * (kThreads / 16)];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const Image im = image_of(pred, gt, mask, b, plane);
  const double* o = out + (size_t)b * 16;
  const bool scored = o[0] == 0.0;  // a failed fit scores nothing: the partials are zeros
  const double scale = o[2], shift = o[3];
  const bool limit = max_depth > 0.f;
  double v[kMetSums];
#pragma unroll
  for (int k = 0; k < kMetSums; ++k) v[k] = 0.0;
  if (scored) {
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const unsigned i0 = blockIdx.x * (unsigned)kTile + (unsigned)(pass * kThreads * 4 + t * 4);
      const Quad q = load_quad(im.pred, im.gt, im.mask, i0, plane, im.vec);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double p = (double)q.p[j], g = (double)q.g[j];
        double al;
        if (policy == 0) {
          al = p;
        } else if (policy == 1) {
          al = p * scale;
        } else {
          const double x = inverse ? p : 1.0 / (q.p[j] > 0.f ? p : __builtin_nan(""));
          const double disp = x * scale + shift;
          al = disp > 1e-8 ? 1.0 / disp : __builtin_inf();
        }
        const bool ok = q.m[j] && q.g[j] > 0.f && finite_d(al) && (!limit || q.g[j] <= max_depth);
        if (ok) {
          const double pp = al > 1e-6 ? al : 1e-6;
          const double r1 = pp / g, r2 = g / pp;
          const double ratio = r1 > r2 ? r1 : r2;
          const double d = pp - g;
          v[0] += 1.0;
          v[1] += __builtin_fabs(d) / g;
          v[2] += d * d;
          v[3] += __builtin_fabs(log10(pp) - log10(g));
          if (ratio < 1.25) v[4] += 1.0;
          if (ratio < 1.5625) v[5] += 1.0;
          if (ratio < 1.953125) v[6] += 1.0;
        }
      }
    }
  }
  const double s = block_sum<kMetSums, kThreads>(v, s_rows);
  if (t < kMetSums) met[((size_t)b * tiles + blockIdx.x) * kMetSums + t] = s;
}

__global__ void __launch_bounds__(kFinThreads)
de_metric_finalize(const double* __restrict__ met, int tiles, double* __restrict__ out) {
  __shared__ double s_rows[kMetSums * (kFinThreads / 16)];
  __shared__ double s_sum[kMetSums];
  const int b = (int)blockIdx.x, t = (int)threadIdx.x;
  double v[kMetSums];
  gather_tiles<kMetSums>(met + (size_t)b * tiles * kMetSums, tiles, v);
  const double s = block_sum<kMetSums, kFinThreads>(v, s_rows);
  if (t < kMetSums) s_sum[t] = s;
  __syncthreads();
  if (t != 0) return;
  double* o = out + (size_t)b * 16;
  const double n = s_sum[0];
  o[4] = n;
  if (n == 0.0) {
    const double nan = __builtin_nan("");
    for (int k = 5; k <= 10; ++k) o[k] = nan;
    return;
  }
  o[5] = s_sum[1] / n;
  o[6] = sqrt(s_sum[2] / n);
  o[7] = s_sum[3] / n;
  o[8] = s_sum[4] / n;
  o[9] = s_sum[5] / n;
  o[10] = s_sum[6] / n;
}

}  // namespace

int depth_eval_tiles(int h, int w) { return (int)(((long long)h * w + kTile - 1) / kTile); }

size_t depth_eval_ws_bytes(int B, int h, int w) {
  return (size_t)B * depth_eval_tiles(h, w) * (kFitSums + kMetSums) * sizeof(double);
}

// Checks nothing: the one caller, mde_op_depth_eval in ops_abi.hip, has refused null pointers,
// non-positive sizes, a policy outside 0..2, a plane of 2^31 - 256 pixels or more (unsigned pixel
// index plus a tile), batch > 65535 (grid.y), a NaN max_depth and a short or misaligned workspace.
hipError_t launch_depth_eval(const float* pred, const float* gt, const unsigned char* mask, int B, int h, int w,
                             int policy, int pred_is_inverse, int fit_finite_only, float max_depth, double* out,
                             void* ws, hipStream_t st) {
  const unsigned plane = (unsigned)h * (unsigned)w;
  const int tiles = depth_eval_tiles(h, w);
  double* fit = static_cast<double*>(ws);
  double* met = fit + (size_t)B * tiles * kFitSums;
  const dim3 grid((unsigned)tiles, (unsigned)B), block(kThreads);
  hipLaunchKernelGGL(de_fit_partials, grid, block, 0, st, pred, gt, mask, plane, tiles, policy, pred_is_inverse,
                     fit_finite_only, fit);
  hipLaunchKernelGGL(de_fit_finalize, dim3((unsigned)B), dim3(kFinThreads), 0, st, fit, tiles, policy, out);
  hipLaunchKernelGGL(de_metric_partials, grid, block, 0, st, pred, gt, mask, plane, tiles, policy, pred_is_inverse,
                     max_depth, out, met);
  hipLaunchKernelGGL(de_metric_finalize, dim3((unsigned)B), dim3(kFinThreads), 0, st, met, tiles, out);
  return hipGetLastError();
}

}  // namespace mde
