// Robust display range: the reference's core/viz.py (robust_range, display_ranges, qualitative_display)
// and demo.py:distribution on the device -- np.percentile(method linear) of the valid pixels of a depth
// map, exact, by radix select.
//
// Contract: include/mde.h, mde_op_depth_quantiles (visualize.py:quantiles_np is the numpy restatement the
// tests hold these kernels to, float64 bit for bit).  -ffp-contract=off for the file (_build.PER_FILE)
// and the pragma below: the lerp's multiply and add round separately, as numpy's do.
//
// Selection runs on 32-bit keys whose unsigned order is the order of the SAMPLE, not of the map:
//   plain        the float's bits with the sign flipped (negatives complemented): key order = x order
//   reciprocal   1 / x ascends where x descends inside one sign, the negatives stay below the positives
//                and 1 / 0 = +inf is on top: negatives key |x|, positives 0x80000000 + (0x7f800000 - bits)
// so the k-th smallest sample value is the decoded k-th smallest key, with no mirrored ranks and no count
// of the signs.  -0 is keyed as +0.  float32 -> float64 and the float64 division are monotone, so equal
// keys are equal sample values and the order statistics of the keys are those of the sample.
//
// Structure (ws: hist | state | img | tile counts):
//   dq_count            a workgroup of 256 threads owns MDE_DEPTH_QUANTILES_TILE = 4096 consecutive pixels
//                       of one image and writes how many of them are valid
//   dq_plan             one workgroup per image: exclusive scan of the tile counts in place (a tile's
//                       first valid pixel's rank), n_valid, stride, n_used
//   dq_targets          one workgroup per row: zeroes the row's histograms, then n of the sample and the
//                       up to 8 target ranks (0, n - 1, prev and next of each quantile), one prefix group
//   4 x { dq_digit<P>   8-bit digit P of every used pixel whose key carries a live target's prefix is
//                       counted in an LDS histogram per prefix group (8 x 256 counters = 8 KB, which leaves
//                       the CU's occupancy to the registers), flushed with integer atomics;
//         dq_pick       one workgroup per row finds each target's digit in its group's histogram (staged
//                       in LDS, 32 threads per target), extends the prefixes, regroups equal ones and
//                       zeroes the histograms for the next digit }
//   the last dq_pick decodes the 8 keys and does the float64 lerp and the fallbacks.
// A pixel's rank for the stride test is its tile's base plus its rank in the tile (popcounts of the
// validity bits, a wave scan by shuffles, the wave totals through LDS); it is skipped when stride == 1.
// Integer sums do not depend on their order and there are no floating-point atomics: the same bytes on
// every run and every grid.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mde.h"
#include "mde_ops.h"

#pragma clang fp contract(off)

namespace mde {
namespace {

constexpr int kThreads = 256;                  // 4 waves of 64
constexpr int kWaves = kThreads / 64;
constexpr int kPasses = 4;                     // float4 loads per thread
constexpr int kTile = kThreads * 4 * kPasses;  // pixels per workgroup
constexpr int kTargets = 8;                    // ranks 0 and n - 1, prev and next of three quantiles
constexpr int kBins = 256;                     // 8-bit digits, four of them
constexpr int kHist = kTargets * kBins;        // counters per row
// state[row]: 0 n (sample size), 1 n_valid, 2 groups, 3 targets, then per target 8.. rank inside its
// prefix, 16.. prefix (the key's digits so far), 24.. group; 32.. prefix of each group
constexpr int kState = 40;
constexpr int kImg = 4;                        // img[b]: n_valid, stride, n_used, 0

static_assert(kTile == MDE_DEPTH_QUANTILES_TILE, "the tile is part of the contract (include/mde.h)");

struct Quantiles {
  double p[3];
  int nq;
};

__device__ __forceinline__ bool valid_pixel(float x, int positive_only) {
  return __builtin_fabsf(x) < __builtin_inff() && (!positive_only || x > 0.f);
}

__device__ __forceinline__ unsigned key_of(float x, int reciprocal) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0;  // -0 counts as +0
  if (!reciprocal) return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (u & 0x80000000u) ? (u & 0x7fffffffu) : 0x80000000u + (0x7f800000u - u);
}

// the sample value a key stands for
__device__ __forceinline__ double value_of(unsigned k, int reciprocal) {
  if (!reciprocal) return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  const unsigned u = (k & 0x80000000u) ? 0x7f800000u - (k - 0x80000000u) : (k | 0x80000000u);
  return 1.0 / (double)__uint_as_float(u);
}

// np.percentile's indices (method linear): vi = (n - 1) * q, prev = floor(vi), next = prev + 1, both
// n - 1 when vi >= n - 1; g = vi - floor(vi).  n >= 1
__device__ __forceinline__ void quantile_index(unsigned n, double p, unsigned& prev, unsigned& next, double& g) {
  const double q = p / 100.0;
  const double top = (double)(n - 1);
  const double vi = top * q;
  const double fl = __builtin_floor(vi);
  if (vi >= top) {
    prev = next = n - 1;
  } else {
    prev = (unsigned)fl;
    next = prev + 1;
  }
  g = vi - fl;
}

// this thread's 16 pixels of the tile, pass-major (pixel tile * kTile + pass * 1024 + t * 4 + j sits at
// x[4 * pass + j]); returns the mask of the valid ones, bit 4 * pass + j
__device__ __forceinline__ unsigned load_tile(const float* __restrict__ im, unsigned plane, unsigned tile,
                                              int positive_only, float (&x)[4 * kPasses]) {
  const bool vec = (reinterpret_cast<uintptr_t>(im) & 15) == 0;
  unsigned mask = 0;
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
    // unsigned: the last tile's indices run up to kTile - 1 past the plane, which is below 2^31 - 256
    const unsigned i0 = tile * (unsigned)kTile + (unsigned)(pass * kThreads * 4) + threadIdx.x * 4u;
    if (vec && i0 + 4u <= plane) {
      const float4 q = *reinterpret_cast<const float4*>(im + i0);
      x[4 * pass] = q.x, x[4 * pass + 1] = q.y, x[4 * pass + 2] = q.z, x[4 * pass + 3] = q.w;
#pragma unroll
      for (int j = 0; j < 4; ++j) mask |= (unsigned)valid_pixel(x[4 * pass + j], positive_only) << (4 * pass + j);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = i0 + (unsigned)j < plane;
        x[4 * pass + j] = in ? im[i0 + j] : 0.f;
        mask |= (unsigned)(in && valid_pixel(x[4 * pass + j], positive_only)) << (4 * pass + j);
      }
    }
  }
  return mask;
}

// inclusive scan over the wave
__device__ __forceinline__ unsigned wave_scan(unsigned v) {
  const int lane = (int)threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned n = __shfl_up(v, o);
    if (lane >= o) v += n;
  }
  return v;
}

// base[pass]: how many valid pixels of the tile come before this thread's four of that pass.
// s: kPasses * kWaves counters of LDS.  Every thread of the workgroup calls it
__device__ __forceinline__ void tile_ranks(unsigned mask, unsigned (&base)[kPasses], unsigned* s) {
  const int t = (int)threadIdx.x, wave = t >> 6;
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
    const unsigned c = (unsigned)__popc((mask >> (4 * pass)) & 15u);
    const unsigned inc = wave_scan(c);
    base[pass] = inc - c;
    if ((t & 63) == 63) s[pass * kWaves + wave] = inc;
  }
  __syncthreads();
  unsigned run = 0;
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w == wave) base[pass] += run;
      run += s[pass * kWaves + w];
    }
  }
}

// cnt[b][tile] = valid pixels of the tile
__global__ void __launch_bounds__(kThreads)
dq_count(const float* __restrict__ map, unsigned plane, int tiles, int positive_only, unsigned* __restrict__ cnt) {
  __shared__ unsigned s[kWaves];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  float x[4 * kPasses];
  const unsigned mask = load_tile(map + (size_t)b * plane, plane, blockIdx.x, positive_only, x);
  unsigned c = (unsigned)__popc(mask);
#pragma unroll
  for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
  if ((t & 63) == 0) s[t >> 6] = c;
  __syncthreads();
  if (t == 0) cnt[(size_t)b * tiles + blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// cnt[b][.] becomes its exclusive scan; img[b] = {n_valid, stride, n_used, 0}
__global__ void __launch_bounds__(kThreads)
dq_plan(unsigned* __restrict__ cnt, int tiles, unsigned sample_cap, unsigned* __restrict__ img) {
  __shared__ unsigned s[kWaves];
  const int b = (int)blockIdx.x, t = (int)threadIdx.x, wave = t >> 6;
  unsigned* c = cnt + (size_t)b * tiles;
  unsigned carry = 0;  // the same in every thread
  for (int i0 = 0; i0 < tiles; i0 += kThreads) {
    const int i = i0 + t;
    const unsigned v = i < tiles ? c[i] : 0u;
    const unsigned inc = wave_scan(v);
    if ((t & 63) == 63) s[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) before += s[w];
      all += s[w];
    }
    if (i < tiles) c[i] = carry + before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (t == 0) {
    unsigned stride = 1;
    if (sample_cap > 0 && carry > sample_cap) stride = carry / sample_cap;  // >= 1
    unsigned* o = img + (size_t)b * kImg;
    o[0] = carry, o[1] = stride, o[2] = (carry + stride - 1) / stride, o[3] = 0;
  }
}

// state[row]: the sample's size and the target ranks, one prefix group (none for an empty sample);
// hist[row] = 0, whatever the caller left in ws
__global__ void __launch_bounds__(kThreads)
dq_targets(const unsigned* __restrict__ img, int B, int pooled, Quantiles qs, unsigned* __restrict__ state,
           unsigned* __restrict__ hist) {
  __shared__ unsigned s[2 * kWaves];
  const int row = (int)blockIdx.x, t = (int)threadIdx.x;
  for (int i = t; i < kHist; i += kThreads) hist[(size_t)row * kHist + i] = 0;
  unsigned nv = 0, nu = 0;
  if (pooled) {
    for (int b = t; b < B; b += kThreads) nv += img[(size_t)b * kImg], nu += img[(size_t)b * kImg + 2];
  } else if (t == 0) {
    nv = img[(size_t)row * kImg], nu = img[(size_t)row * kImg + 2];
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) nv += __shfl_xor(nv, o), nu += __shfl_xor(nu, o);
  if ((t & 63) == 0) s[2 * (t >> 6)] = nv, s[2 * (t >> 6) + 1] = nu;
  __syncthreads();
  if (t != 0) return;
  nv = s[0] + s[2] + s[4] + s[6], nu = s[1] + s[3] + s[5] + s[7];
  unsigned* st = state + (size_t)row * kState;
  for (int i = 0; i < kState; ++i) st[i] = 0;
  st[0] = nu, st[1] = nv, st[3] = (unsigned)(2 + 2 * qs.nq);
  if (nu == 0) return;
  st[2] = 1;
  st[8] = 0, st[9] = nu - 1;
  for (int i = 0; i < qs.nq; ++i) {
    unsigned prev, next;
    double g;
    quantile_index(nu, qs.p[i], prev, next, g);
    st[10 + 2 * i] = prev, st[11 + 2 * i] = next;
  }
}

// digit PASS (most significant first) of every used pixel under a live prefix, counted per prefix group
template <int PASS>
__global__ void __launch_bounds__(kThreads)
dq_digit(const float* __restrict__ map, unsigned plane, int tiles, int positive_only, int reciprocal, int pooled,
         const unsigned* __restrict__ tile_base, const unsigned* __restrict__ img,
         const unsigned* __restrict__ state, unsigned* __restrict__ hist) {
  __shared__ unsigned s_hist[kHist];
  __shared__ unsigned s_scan[kPasses * kWaves];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const int row = pooled ? 0 : b;
  const unsigned* st = state + (size_t)row * kState;
  const int groups = (int)st[2];  // the same in every thread
  if (groups == 0) return;
  unsigned gp[kTargets];
#pragma unroll
  for (int g = 0; g < kTargets; ++g) gp[g] = st[32 + g];
  for (int i = t; i < groups * kBins; i += kThreads) s_hist[i] = 0;

  float x[4 * kPasses];
  const unsigned mask = load_tile(map + (size_t)b * plane, plane, blockIdx.x, positive_only, x);
  const unsigned stride = img[(size_t)b * kImg + 1];
  unsigned base[kPasses] = {0, 0, 0, 0};
  if (stride > 1) {
    tile_ranks(mask, base, s_scan);
    const unsigned r0 = tile_base[(size_t)b * tiles + blockIdx.x];
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) base[pass] += r0;
  }
  __syncthreads();

  // equal bins in a row (a smooth map) go to LDS as one add
  int cur = -1;
  unsigned run = 0;
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
    unsigned r = base[pass];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((mask >> (4 * pass + j)) & 1u)) continue;
      const bool used = stride == 1 || r % stride == 0;
      ++r;
      if (!used) continue;
      const unsigned key = key_of(x[4 * pass + j], reciprocal);
      int g = 0;
      if (PASS > 0) {
        const unsigned pre = key >> (32 - 8 * PASS);
        g = -1;
#pragma unroll
        for (int k = 0; k < kTargets; ++k)
          if (k < groups && gp[k] == pre) g = k;
        if (g < 0) continue;
      }
      const int bin = g * kBins + (int)((key >> (24 - 8 * PASS)) & 255u);
      if (bin == cur) {
        ++run;
      } else {
        if (run) atomicAdd(&s_hist[cur], run);
        cur = bin, run = 1;
      }
    }
  }
  if (run) atomicAdd(&s_hist[cur], run);
  __syncthreads();
  unsigned* h = hist + (size_t)row * kHist;
  for (int i = t; i < groups * kBins; i += kThreads) {
    const unsigned c = s_hist[i];
    if (c) atomicAdd(&h[i], c);
  }
}

// after digit `pass`: each target's digit from its group's histogram, the longer prefixes regrouped, the
// histograms zeroed; after the last digit the prefixes are the keys and out[row] is written
__global__ void __launch_bounds__(kThreads)
dq_pick(unsigned* __restrict__ hist, unsigned* __restrict__ state, int pass, int reciprocal, Quantiles qs,
        double* __restrict__ out) {
  __shared__ unsigned s_pre[kTargets], s_rank[kTargets];
  __shared__ unsigned s_h[kHist];
  const int row = (int)blockIdx.x, t = (int)threadIdx.x;
  unsigned* st = state + (size_t)row * kState;
  unsigned* h = hist + (size_t)row * kHist;
  const unsigned n = st[0];
  const int targets = (int)st[3];
  if (t < kTargets) s_pre[t] = 0, s_rank[t] = 0;
  for (int i = t; i < kHist; i += kThreads) s_h[i] = n > 0 ? h[i] : 0u;
  __syncthreads();
  // 32 threads per target, 8 bins per thread: a scan of the 32 sums finds the thread whose bins hold the
  // rank (the counts of a group sum to more than the ranks inside it), and it walks its eight
  const int tg = t >> 5, l = t & 31;
  const bool live = n > 0 && tg < targets;
  const unsigned* hg = s_h + (live ? st[24 + tg] : 0u) * kBins + 8 * l;
  unsigned c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) c += hg[k];
  unsigned inc = c;
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {
    const unsigned v = __shfl_up(inc, o, 32);
    if (l >= o) inc += v;
  }
  if (live) {
    unsigned r = st[8 + tg];
    if (r >= inc - c && r < inc) {
      r -= inc - c;
      unsigned d = 0;
      for (; d < 7; ++d) {
        if (r < hg[d]) break;
        r -= hg[d];
      }
      s_pre[tg] = (st[16 + tg] << 8) | (unsigned)(8 * l) | d;
      s_rank[tg] = r;
    }
  }
  __syncthreads();
  for (int i = t; i < kHist; i += kThreads) h[i] = 0;
  if (t != 0) return;
  if (n > 0) {
    unsigned groups = 0;
    for (int i = 0; i < targets; ++i) {
      st[8 + i] = s_rank[i], st[16 + i] = s_pre[i];
      int same = -1;
      for (int j = 0; j < i && same < 0; ++j)
        if (s_pre[j] == s_pre[i]) same = j;
      if (same >= 0) {
        st[24 + i] = st[24 + same];
      } else {
        st[24 + i] = groups, st[32 + groups] = s_pre[i];
        ++groups;
      }
    }
    st[2] = groups;
  }
  if (pass != 3) return;

  double* o = out + (size_t)row * 8;
  o[0] = (double)st[1], o[1] = (double)n;
  if (n == 0) {
    const double nan = __builtin_nan("");
    o[2] = o[3] = o[4] = o[5] = nan;
    o[6] = 0.0, o[7] = 1.0;
    return;
  }
  const double mn = value_of(s_pre[0], reciprocal), mx = value_of(s_pre[1], reciprocal);
  double qv[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < qs.nq; ++i) {
    unsigned prev, next;
    double g;
    quantile_index(n, qs.p[i], prev, next, g);
    const double a = value_of(s_pre[2 + 2 * i], reciprocal), c = value_of(s_pre[3 + 2 * i], reciprocal);
    const double d = c - a;
    qv[i] = g < 0.5 ? a + d * g : c - d * (1.0 - g);
  }
  o[2] = mn, o[3] = qs.nq == 3 ? qv[2] : mx;
  o[4] = qv[0], o[5] = qv[1];
  double vmin = qv[0], vmax = qv[qs.nq - 1];
  const double inf = __builtin_inf();
  if (!(__builtin_fabs(vmin) < inf) || !(__builtin_fabs(vmax) < inf) || vmax <= vmin) {
    vmin = mn, vmax = mx;
    if (vmax <= vmin) vmax = vmin + 1.0;
  }
  o[6] = vmin, o[7] = vmax;
}

int tiles_of(int h, int w) { return (int)(((long long)h * w + kTile - 1) / kTile); }

}  // namespace

size_t depth_quantiles_ws_bytes(int B, int h, int w) {
  return ((size_t)B * (kHist + kState + kImg) + (size_t)B * tiles_of(h, w)) * sizeof(unsigned);
}

// Checks nothing: the one caller, mde_op_depth_quantiles in ops_abi.hip, has refused null pointers,
// non-positive sizes, nq outside 1..3, a percentage outside [0, 100], a negative sample_cap, a plane (a
// pool, when pooled) of 2^31 - 256 pixels or more (unsigned pixel index plus a tile; 32-bit counters),
// batch > 65535 (grid.y) and a short or misaligned workspace or out.
hipError_t launch_depth_quantiles(const float* map, int B, int h, int w, int positive_only, int reciprocal,
                                  int pooled, int sample_cap, const double* q_percent, int nq, double* out, void* ws,
                                  hipStream_t st) {
  const int rows = pooled ? 1 : B;
  const int tiles = tiles_of(h, w);
  const unsigned plane = (unsigned)h * (unsigned)w;
  unsigned* hist = static_cast<unsigned*>(ws);
  unsigned* state = hist + (size_t)B * kHist;
  unsigned* img = state + (size_t)B * kState;
  unsigned* cnt = img + (size_t)B * kImg;
  Quantiles qs;
  qs.nq = nq;
  for (int i = 0; i < 3; ++i) qs.p[i] = i < nq ? q_percent[i] : 0.0;

  const dim3 grid((unsigned)tiles, (unsigned)B), block(kThreads);
  hipLaunchKernelGGL(dq_count, grid, block, 0, st, map, plane, tiles, positive_only, cnt);
  hipLaunchKernelGGL(dq_plan, dim3((unsigned)B), block, 0, st, cnt, tiles, (unsigned)sample_cap, img);
  hipLaunchKernelGGL(dq_targets, dim3((unsigned)rows), block, 0, st, img, B, pooled, qs, state, hist);
#define MDE_DQ_DIGIT(P)                                                                                       \
  hipLaunchKernelGGL(dq_digit<P>, grid, block, 0, st, map, plane, tiles, positive_only, reciprocal, pooled, cnt, \
                     img, state, hist);                                                                       \
  hipLaunchKernelGGL(dq_pick, dim3((unsigned)rows), block, 0, st, hist, state, P, reciprocal, qs, out)
  MDE_DQ_DIGIT(0);
  MDE_DQ_DIGIT(1);
  MDE_DQ_DIGIT(2);
  MDE_DQ_DIGIT(3);
#undef MDE_DQ_DIGIT
  return hipGetLastError();
}

}  // namespace mde
