// Point-cloud preview: the reference's core/viz.py:render_points (what demo.py:cloud_figure draws for
// every model that has a camera), on the device -- an orthographic, z-buffered splat of the cloud that
// mde_op_point_cloud would pack, seen from (elev, azim), centred on the per-axis median and scaled by the
// 99th percentile of the rotated |x|, |y|, the near point winning each pixel.
//
// Contract: include/mde.h, mde_op_cloud_view (pointcloud.py:render_np is the numpy restatement the tests
// hold these kernels to, the picture byte for byte and the view row bit for bit).  -ffp-contract=off for
// the file (_build.PER_FILE) and cloud_source.h's pragma: every float32 and float64 operation rounds on its own,
// as numpy's do; the grid, the camera and the unprojection are cloud_source.h's, shared with point_cloud.hip.
//
// Structure (ws: z-buffer | quantile rows | workgroup counts | planes | quantile scratch), all on the stream:
//   cv_planes     X, Y, Z of every sample as three float32 planes, NaN where the sample is invalid
//   quantiles     launch_depth_quantiles on the 3 * B planes, p = 50: the centre, exact
//   cv_abs        X, Y, Z again from the depth map; (float)|x1| and (float)|y2| over the X and Y planes
//   quantiles     one pooled call per image over its two planes, p = 99: the span, exact
//     (the four steps above are skipped under view_in: a fixed camera needs no selection)
//   cv_finish     one thread per image: fallbacks, scale, the view row (its two counts come later)
//   cv_clear      the z-buffer to all ones
//   cv_splat      every valid sample inside the picture: one 64-bit atomicMin of
//                 (ordered key of (float)z2) << 32 | sample index on its pixel -- the smallest z2 wins, then
//                 the lowest index; each workgroup writes how many of its samples are valid and inside
//   cv_count      one workgroup per image adds those counts into the view row
//   cv_resolve    one thread per pixel: the winner's photo bytes, or the background
// The only atomic is the integer min, whose result does not depend on the order, and no workgroup waits on
// memory another workgroup writes (the order between the steps is the stream's): the same bytes on every
// run and every grid.
//
// When many samples fall on few pixels the atomics on one address serialise, so cv_splat first reads the
// pixel with a plain load and skips the atomic when its own value cannot win.  A z-buffer entry only ever
// decreases, so a value read earlier (even a stale one from a cache) is never below the final one: a
// sample that is skipped would have lost anyway, and the result is the same.

#include "cloud_source.h"

namespace mde {
namespace {

constexpr int kThreads = 256;  // 4 waves of 64
constexpr int kRow = 8;        // doubles per quantile row and per view row
constexpr unsigned long long kEmpty = ~0ull;

static_assert(kThreads % 64 == 0, "ballots below are over wave64");

struct Trig {
  double cos_a, sin_a, cos_e, sin_e;
};

__device__ __forceinline__ bool finite32(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

// sample s of image b (img its depth map): X, Y, Z as mde_op_point_cloud computes them; whether the sample is
// drawn (the reference's subsample_cloud keep rule), false past the grid's end
__device__ __forceinline__ bool drawn(const float* __restrict__ img, const Geom& g, const Camera& cam, Focal f,
                                      unsigned s, float& X, float& Y, float& Z) {
  int v, u;
  if (!sample_pixel(g, s, v, u)) return false;
  Z = img[(size_t)v * g.w + u];
  unproject_xy(cam, f, v, u, Z, X, Y);
  return finite32(X) && finite32(Y) && finite32(Z) && Z > 0.f;
}

// the order-preserving key of depth_quantiles.hip (plain): -0 counts as +0
__device__ __forceinline__ unsigned key_of(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(kThreads)
cv_planes(const float* __restrict__ depth, Geom g, Camera cam, float* __restrict__ planes) {
  const int b = (int)blockIdx.y;
  const unsigned n = (unsigned)(g.hs * g.ws), s = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (s >= n) return;
  float X, Y, Z;
  const bool ok = drawn(depth + (size_t)b * g.h * g.w, g, cam, cam.focal(b), s, X, Y, Z);
  const float nan = __builtin_nanf("");
  float* p = planes + (size_t)b * 3 * n;
  p[s] = ok ? X : nan;
  p[(size_t)n + s] = ok ? Y : nan;
  p[2 * (size_t)n + s] = ok ? Z : nan;
}

// centre[b * 3 + k][4] is percentile 50 of plane k of image b (NaN when the image has no valid sample,
// and then no sample reads it)
__global__ void __launch_bounds__(kThreads)
cv_abs(const float* __restrict__ depth, Geom g, Camera cam, Trig t, const double* __restrict__ centre,
       float* __restrict__ planes) {
  const int b = (int)blockIdx.y;
  const unsigned n = (unsigned)(g.hs * g.ws), s = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (s >= n) return;
  float X, Y, Z;
  const bool ok = drawn(depth + (size_t)b * g.h * g.w, g, cam, cam.focal(b), s, X, Y, Z);
  float ax = __builtin_nanf(""), ay = ax;
  if (ok) {
    const double* c = centre + (size_t)b * 3 * kRow;
    const double dx = (double)X - c[4], dy = (double)Y - c[kRow + 4], dz = (double)Z - c[2 * kRow + 4];
    const double x1 = t.cos_a * dx + t.sin_a * dz;
    const double z1 = (-t.sin_a) * dx + t.cos_a * dz;
    const double y2 = t.cos_e * dy - t.sin_e * z1;
    ax = (float)__builtin_fabs(x1);
    ay = (float)__builtin_fabs(y2);
  }
  float* p = planes + (size_t)b * 3 * n;
  p[s] = ax;
  p[(size_t)n + s] = ay;
}

// view_out[b] = {0, c0, c1, c2, span, scale, 0, 0}; slots 0 and 6 are cv_resolve's
// (view_in may be view_out itself: a thread reads its row before it writes it)
__global__ void cv_finish(int B, const double* view_in, const double* __restrict__ centre,
                          const double* __restrict__ span_rows, double half_min, double* view_out) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= B) return;
  double c0, c1, c2, span, scale;
  if (view_in) {
    const double* vi = view_in + (size_t)b * kRow;
    c0 = vi[1], c1 = vi[2], c2 = vi[3], span = vi[4], scale = vi[5];
  } else {
    const double* c = centre + (size_t)b * 3 * kRow;
    if (c[0] == 0.0) {  // no valid sample
      c0 = c1 = c2 = 0.0;
      span = 1.0;
    } else {
      c0 = c[4], c1 = c[kRow + 4], c2 = c[2 * kRow + 4];
      span = span_rows[(size_t)b * kRow + 4];
      if (!(__builtin_fabs(span) < __builtin_inf()) || span <= 0.0) span = 1.0;
    }
    scale = half_min / span;
  }
  double* o = view_out + (size_t)b * kRow;
  o[0] = 0.0, o[1] = c0, o[2] = c1, o[3] = c2, o[4] = span, o[5] = scale, o[6] = 0.0, o[7] = 0.0;
}

__global__ void __launch_bounds__(kThreads)
cv_clear(unsigned long long* __restrict__ zbuf, unsigned pixels) {
  const int b = (int)blockIdx.y;
  const unsigned i = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (i < pixels) zbuf[(size_t)b * pixels + i] = kEmpty;
}

__global__ void __launch_bounds__(kThreads)
cv_splat(const float* __restrict__ depth, Geom g, Camera cam, Trig t, const double* __restrict__ view, int out_h,
         int out_w, unsigned long long* __restrict__ zbuf, unsigned* __restrict__ block_counts) {
  __shared__ unsigned s_cnt[2 * (kThreads / 64)];
  const int b = (int)blockIdx.y;
  const unsigned n = (unsigned)(g.hs * g.ws), s = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  bool ok = false, in = false;
  unsigned long long packed = kEmpty;
  unsigned pixel = 0;
  if (s < n) {
    float X, Y, Z;
    ok = drawn(depth + (size_t)b * g.h * g.w, g, cam, cam.focal(b), s, X, Y, Z);
    if (ok) {
      const double* vw = view + (size_t)b * kRow;
      const double scale = vw[5];
      const double dx = (double)X - vw[1], dy = (double)Y - vw[2], dz = (double)Z - vw[3];
      const double x1 = t.cos_a * dx + t.sin_a * dz;
      const double z1 = (-t.sin_a) * dx + t.cos_a * dz;
      const double y2 = t.cos_e * dy - t.sin_e * z1;
      const double z2 = t.sin_e * dy + t.cos_e * z1;
      const double pu = __builtin_rint(x1 * scale + (double)out_w / 2.0);
      const double pv = __builtin_rint(y2 * scale + (double)out_h / 2.0);
      in = pu >= 0.0 && pu < (double)out_w && pv >= 0.0 && pv < (double)out_h;  // a NaN is outside
      if (in) {
        pixel = (unsigned)(int)pv * (unsigned)out_w + (unsigned)(int)pu;  // < out_h * out_w
        packed = ((unsigned long long)key_of((float)z2) << 32) | s;
      }
    }
  }
  if (in) {
    unsigned long long* z = zbuf + (size_t)b * ((size_t)out_h * out_w) + pixel;
    if (packed < *z) atomicMin(z, packed);
  }
  // every thread of the workgroup is here: the ballots are whole.  The workgroup's two counts go to its own
  // slot (a hundred thousand waves adding to one address would serialise there); cv_count adds the slots
  const unsigned long long m_ok = __ballot(ok), m_in = __ballot(in);
  if ((threadIdx.x & 63) == 0) {
    s_cnt[2 * (threadIdx.x >> 6)] = (unsigned)__popcll(m_ok);
    s_cnt[2 * (threadIdx.x >> 6) + 1] = (unsigned)__popcll(m_in);
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned c = 0;
#pragma unroll
    for (int wv = 0; wv < kThreads / 64; ++wv) c += s_cnt[2 * wv + threadIdx.x];
    block_counts[((size_t)b * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = c;
  }
}

// view_out[b][0] = valid samples, view_out[b][6] = samples inside the picture: the sums of cv_splat's slots
// (integers: the order does not matter)
__global__ void __launch_bounds__(kThreads)
cv_count(const unsigned* __restrict__ block_counts, unsigned blocks, double* __restrict__ view_out) {
  __shared__ unsigned s_cnt[2 * (kThreads / 64)];
  const int b = (int)blockIdx.x, t = (int)threadIdx.x;
  const unsigned* c = block_counts + (size_t)b * blocks * 2;
  unsigned ok = 0, in = 0;
  for (unsigned i = (unsigned)t; i < blocks; i += kThreads) ok += c[2 * (size_t)i], in += c[2 * (size_t)i + 1];
#pragma unroll
  for (int o = 32; o; o >>= 1) ok += __shfl_xor(ok, o), in += __shfl_xor(in, o);
  if ((t & 63) == 0) s_cnt[2 * (t >> 6)] = ok, s_cnt[2 * (t >> 6) + 1] = in;
  __syncthreads();
  if (t < 2) {
    unsigned sum = 0;
#pragma unroll
    for (int wv = 0; wv < kThreads / 64; ++wv) sum += s_cnt[2 * wv + t];
    view_out[(size_t)b * kRow + (t ? 6 : 0)] = (double)sum;
  }
}

__global__ void __launch_bounds__(kThreads)
cv_resolve(const unsigned long long* __restrict__ zbuf, Geom g, Camera cam, unsigned pixels, int bg0, int bg1, int bg2,
           int out_swap_rb, unsigned char* __restrict__ out) {
  const int b = (int)blockIdx.y;
  const unsigned i = blockIdx.x * (unsigned)kThreads + threadIdx.x;
  if (i >= pixels) return;
  const unsigned long long p = zbuf[(size_t)b * pixels + i];
  unsigned char r = (unsigned char)bg0, gr = (unsigned char)bg1, bl = (unsigned char)bg2;
  if (p != kEmpty) {
    r = gr = bl = 200;
    if (cam.photo) {
      int v = 0, u = 0;
      sample_pixel(g, (unsigned)(p & 0xffffffffull), v, u);  // the winner is a sample of the grid
      photo_rgb(cam, g, b, v, u, r, gr, bl);
    }
  }
  unsigned char* o = out + ((size_t)b * pixels + i) * 3;
  o[0] = out_swap_rb ? bl : r;
  o[1] = gr;
  o[2] = out_swap_rb ? r : bl;
}

size_t round8(size_t x) { return (x + 7) & ~(size_t)7; }

struct Layout {
  size_t zbuf, rows, counters, planes, quant, total;
};

Layout layout_of(int B, int h, int w, int step, int out_h, int out_w) {
  const Geom g = make_geom(h, w, step);
  const size_t n = (size_t)g.hs * g.ws;
  Layout l;
  l.zbuf = 0;
  l.rows = l.zbuf + (size_t)B * out_h * out_w * sizeof(unsigned long long);
  l.counters = l.rows + (size_t)B * 4 * kRow * sizeof(double);  // three centre rows and one span row per image
  l.planes = l.counters + (size_t)B * ((n + kThreads - 1) / kThreads) * 2 * sizeof(unsigned);  // cv_splat's slots
  l.quant = l.planes + round8((size_t)B * 3 * n * sizeof(float));
  l.total = l.quant + round8(depth_quantiles_ws_bytes(3 * B, g.hs, g.ws));
  return l;
}

}  // namespace

size_t cloud_view_ws_bytes(int B, int h, int w, int step, int out_h, int out_w) {
  return layout_of(B, h, w, step, out_h, out_w).total;
}

// Checks nothing: the one caller, mde_op_cloud_view in ops_abi.hip, has refused null pointers, non-positive
// sizes, a sampled grid of 2^30 - 128 samples or more (two planes pooled in one quantile call), a picture
// of 2^31 - 256 pixels or more, batch > 21845 (three planes per image on grid.y), a short or misaligned
// workspace, misaligned view rows, a missing focal length and non-finite trig values.
hipError_t launch_cloud_view(const CloudSource& src, double cos_a, double sin_a, double cos_e, double sin_e,
                             const double* view_in, const int bg_rgb[3], int out_swap_rb, unsigned char* out,
                             int out_h, int out_w, double* view_out, void* ws, hipStream_t st) {
  const Geom g = make_geom(src.h, src.w, src.step);
  const Camera cam = make_camera(src);
  const Trig t = {cos_a, sin_a, cos_e, sin_e};
  const float* depth = src.depth;
  const int B = src.B;
  const Layout l = layout_of(B, src.h, src.w, src.step, out_h, out_w);
  char* base = static_cast<char*>(ws);
  unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(base + l.zbuf);
  double* centre = reinterpret_cast<double*>(base + l.rows);
  double* span_rows = centre + (size_t)B * 3 * kRow;
  unsigned* block_counts = reinterpret_cast<unsigned*>(base + l.counters);
  float* planes = reinterpret_cast<float*>(base + l.planes);
  void* quant = base + l.quant;
  const size_t n = (size_t)g.hs * g.ws;
  const unsigned pixels = (unsigned)out_h * (unsigned)out_w;
  const dim3 block(kThreads), sgrid((unsigned)((n + kThreads - 1) / kThreads), (unsigned)B),
      pgrid((pixels + kThreads - 1) / kThreads, (unsigned)B);

  if (!view_in) {
    hipLaunchKernelGGL(cv_planes, sgrid, block, 0, st, depth, g, cam, planes);
    const double p50 = 50.0, p99 = 99.0;
    hipError_t e = launch_depth_quantiles(planes, 3 * B, g.hs, g.ws, 0, 0, 0, 0, &p50, 1, centre, quant, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cv_abs, sgrid, block, 0, st, depth, g, cam, t, centre, planes);
    for (int b = 0; b < B; ++b) {  // the pooled mode pools a whole call
      e = launch_depth_quantiles(planes + (size_t)b * 3 * n, 2, g.hs, g.ws, 0, 0, 1, 0, &p99, 1,
                                 span_rows + (size_t)b * kRow, quant, st);
      if (e != hipSuccess) return e;
    }
  }
  const double half_min = 0.46 * (double)(out_h < out_w ? out_h : out_w);
  hipLaunchKernelGGL(cv_finish, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, B, view_in, centre, span_rows,
                     half_min, view_out);
  hipLaunchKernelGGL(cv_clear, pgrid, block, 0, st, zbuf, pixels);
  hipLaunchKernelGGL(cv_splat, sgrid, block, 0, st, depth, g, cam, t, view_out, out_h, out_w, zbuf, block_counts);
  hipLaunchKernelGGL(cv_count, dim3((unsigned)B), block, 0, st, block_counts, sgrid.x, view_out);
  hipLaunchKernelGGL(cv_resolve, pgrid, block, 0, st, zbuf, g, cam, pixels, bg_rgb[0], bg_rgb[1], bg_rgb[2],
                     out_swap_rb, out);
  return hipGetLastError();
}

}  // namespace mde
