// Point clouds: the tail of reference models/depth_pro/onnx2trt_pointcloud.py (:172-184), on the
// device.  Metric depth at the photo's size (what dp_postprocess_kernel / depth_postprocess leave
// in device memory) is unprojected through a pinhole camera, invalid pixels are dropped in
// row-major order and the survivors are packed as PLY binary_little_endian vertex records.
//
// Contract (the same text as include/mde.h; pointcloud.py:unproject_np is the numpy restatement
// the tests hold these kernels to, bit for bit):
//
//   sampled grid: hs = ceil(h / step) by ws = ceil(w / step), sample (i, j) is pixel
//                 (v, u) = (i * step, j * step), z = depth[b][v][u]
//   fx = fy = f_px_dev[b] when f_px_dev is given, else the host floats fx, fy
//   every operation float32 and rounded separately, never fused:
//     xn = ((float)u - cx) / fx          yn = ((float)v - cy) / fy        (IEEE division)
//     X = xn * z,  Y = yn * z,  Z = z
//   colour = photo bytes of pixel (v, u), output order R, G, B after swap_rb (swap_rb != 0: output
//            channel c is source channel 2 - c, the rule of mde_op_resize_u8)
//   record = float X, Y, Z, then uchar R, G, B when a photo is given: 15 bytes (12 without),
//            tightly packed; image b's region starts at byte b * hs * ws * rec
//   organized (compact == 0): every sample is written, record index = sample index (row-major),
//            no range test, a NaN z gives NaN X, Y, Z; counts[b] = hs * ws
//   compact: a sample is kept iff z == z && z >= z_lo && z <= z_hi; the kept records are dense, in
//            row-major sample order; counts[b] = number kept; bytes of the region past counts[b]
//            records are not written
//
// Rounding discipline: as in depth_pro_photo.hip -- __f*_rn per step, -ffp-contract=off for the
// file (_build.PER_FILE) and the pragma below, no fast-math flag in the build.
//
// Structure.  A workgroup of 256 threads owns TILE = 1024 consecutive samples of one image;
// thread t takes samples t, t + 256, t + 512, t + 768 of the tile, so a wave reads 64 consecutive
// floats per load.  A sample's rank among the kept ones of its tile is the number of kept lanes
// below it (one ballot) plus the kept counts of the 16 (pass, wave) segments before its own.
//   organized: pc_write_kernel<false> alone; a tile's first record index is its first sample index.
//   compact, three launches on the stream:
//     pc_count_kernel            tile_count[b][g]  = kept samples of tile g
//     pc_scan_kernel             tile_count[b][g] := exclusive prefix (one workgroup per image,
//                                walking the tiles 256 at a time with a running carry, so any
//                                number of tiles), counts[b] = total
//     pc_write_kernel<true>      evaluates the same keep() again, ranks, writes from the prefix
//   No workgroup ever waits on memory another workgroup writes: the order between the three
//   steps is the stream's.  (A single-pass look-back scan would spin on its predecessors' flags
//   and so rely on them being scheduled; it saves one read of the depth map, which is a quarter
//   of what the records cost to write.)  Integer counts and a fixed order: the result is the
//   same bits on every run.
//
// Store path.  A tile's records are one contiguous byte range [g0, g0 + n * rec) that starts at
// any alignment (rec = 15; and a compacted tile starts wherever its predecessors ended).  The
// records are staged in LDS at byte (g0 & 15) + rank * rec, i.e. with the same alignment modulo 16
// as in global memory; then the 16-byte aligned middle of the range goes out as uint4 LDS loads
// and uint4 global stores (a wave writes 1 KiB contiguous per instruction) and the up to 15 bytes
// before and after it as single-byte stores.  A dword that two tiles share is never read or
// written whole: each tile stores exactly its own bytes.

#include <hip/hip_runtime.h>

#include <type_traits>

#include "mde_ops.h"

#pragma clang fp contract(off)

namespace mde {
namespace {

constexpr int kThreads = 256;                 // 4 waves of 64
constexpr int kPasses = 4;                    // samples per thread
constexpr int kTile = kThreads * kPasses;     // samples per workgroup
constexpr int kSegs = kPasses * (kThreads / 64);
constexpr int kScanThreads = 256;             // pc_scan_kernel's one workgroup per image

static_assert(kThreads % 64 == 0, "ballots below are over wave64");

struct __attribute__((packed)) Rec12 {
  float x, y, z;
};
struct __attribute__((packed)) Rec15 {
  float x, y, z;
  unsigned char r, g, b;
};
static_assert(sizeof(Rec12) == 12 && sizeof(Rec15) == 15, "PLY vertex records are tightly packed");

struct Geom {
  int h, w, step, hs, ws;  // hs * ws < 2^31 - 256 (the ABI wrapper)
};

// the one statement of validity: count and write must agree on every sample
__device__ __forceinline__ bool keep(float z, float z_lo, float z_hi) { return z == z && z >= z_lo && z <= z_hi; }

// sample s of image b -> its pixel; returns false past the grid's end
// (s is unsigned: the last tile's sample indices run up to 1023 past hs * ws, past INT_MAX for the
// largest grids the wrapper lets through)
__device__ __forceinline__ bool sample_pixel(const Geom& g, unsigned s, int& v, int& u) {
  if (s >= (unsigned)(g.hs * g.ws)) return false;
  const int i = (int)(s / (unsigned)g.ws), j = (int)(s - (unsigned)i * (unsigned)g.ws);
  v = i * g.step;
  u = j * g.step;
  return true;
}

__global__ void __launch_bounds__(kThreads)
pc_count_kernel(const float* __restrict__ depth, Geom g, float z_lo, float z_hi, int* __restrict__ tile_count,
                int tiles) {
  __shared__ int s_cnt[kThreads / 64];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const float* img = depth + (size_t)b * g.h * g.w;
  int mine = 0;  // wave-uniform: kept samples of this wave's four segments
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    int v, u;
    bool k = sample_pixel(g, blockIdx.x * (unsigned)kTile + (unsigned)(p * kThreads + t), v, u);
    if (k) k = keep(img[(size_t)v * g.w + u], z_lo, z_hi);
    mine += __popcll(__ballot(k));
  }
  if ((t & 63) == 0) s_cnt[t >> 6] = mine;
  __syncthreads();
  if (t == 0) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) n += s_cnt[i];
    tile_count[(size_t)b * tiles + blockIdx.x] = n;
  }
}

// in place: tile_count[b][.] becomes its exclusive prefix; any number of tiles
__global__ void __launch_bounds__(kScanThreads)
pc_scan_kernel(int* __restrict__ tile_count, int tiles, int* __restrict__ counts) {
  __shared__ int s_wave[kScanThreads / 64];
  const int b = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  int* c = tile_count + (size_t)b * tiles;
  int carry = 0;
  for (int base = 0; base < tiles; base += kScanThreads) {
    const int i = base + t;
    const int own = i < tiles ? c[i] : 0;
    int incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int below = __shfl_up(incl, d);
      if (lane >= d) incl += below;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kScanThreads / 64; ++k) {
      if (k < wave) before += s_wave[k];
      all += s_wave[k];
    }
    if (i < tiles) c[i] = carry + before + incl - own;
    carry += all;
    __syncthreads();  // s_wave is rewritten by the next chunk
  }
  if (t == 0) counts[b] = carry;
}

template <bool COMPACT, bool COLOUR>
__global__ void __launch_bounds__(kThreads)
pc_write_kernel(const float* __restrict__ depth, Geom g, const unsigned char* __restrict__ photo, int pitch,
                int swap_rb, const float* __restrict__ f_px_dev, float fx, float fy, float cx, float cy, float z_lo,
                float z_hi, unsigned char* __restrict__ records, const int* __restrict__ tile_first,
                int* __restrict__ counts, int tiles) {
  using Rec = typename std::conditional<COLOUR, Rec15, Rec12>::type;
  constexpr int rec = (int)sizeof(Rec);
  // the tile's bytes behind up to 15 bytes of alignment shift, in whole uint4
  __shared__ uint4 s_stage[(kTile * rec + 15 + 15) / 16];
  __shared__ int s_cnt[kSegs];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int plane = g.hs * g.ws;
  if (f_px_dev) fx = fy = f_px_dev[b];
  const float* img = depth + (size_t)b * g.h * g.w;

  Rec r[kPasses];
  bool k[kPasses];
  int below[kPasses];  // kept lanes of the same wave and pass below this one
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    int v = 0, u = 0;
    k[p] = sample_pixel(g, blockIdx.x * (unsigned)kTile + (unsigned)(p * kThreads + t), v, u);
    float z = 0.f;
    if (k[p]) {
      z = img[(size_t)v * g.w + u];
      if (COMPACT) k[p] = keep(z, z_lo, z_hi);
    }
    const unsigned long long m = __ballot(k[p]);
    below[p] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[p * (kThreads / 64) + wave] = __popcll(m);
    if (k[p]) {
      const float xn = __fdiv_rn(__fsub_rn((float)u, cx), fx);
      const float yn = __fdiv_rn(__fsub_rn((float)v, cy), fy);
      r[p].x = __fmul_rn(xn, z);
      r[p].y = __fmul_rn(yn, z);
      r[p].z = z;
      if constexpr (COLOUR) {
        const unsigned char* px = photo + ((size_t)b * g.h + v) * pitch + 3 * (size_t)u;
        const unsigned char c0 = px[0], c1 = px[1], c2 = px[2];
        r[p].r = swap_rb ? c2 : c0;
        r[p].g = c1;
        r[p].b = swap_rb ? c0 : c2;
      }
    }
  }
  __syncthreads();

  int n = 0;  // records of this tile
  int before[kPasses];
#pragma unroll
  for (int p = 0; p < kPasses; ++p) before[p] = 0;
#pragma unroll
  for (int s = 0; s < kSegs; ++s) {
    const int c = s_cnt[s];
#pragma unroll
    for (int p = 0; p < kPasses; ++p)
      if (s < p * (kThreads / 64) + wave) before[p] += c;
    n += c;
  }
  // first record of the tile within the image's region
  const int first = COMPACT ? tile_first[(size_t)b * tiles + blockIdx.x] : (int)blockIdx.x * kTile;
  if (!COMPACT && blockIdx.x == 0 && t == 0) counts[b] = plane;

  unsigned char* out = records + ((size_t)b * plane + (size_t)first) * rec;  // g0
  const int shift = (int)(reinterpret_cast<uintptr_t>(out) & 15);
  unsigned char* stage = reinterpret_cast<unsigned char*>(s_stage) + shift;
#pragma unroll
  for (int p = 0; p < kPasses; ++p)
    if (k[p]) *reinterpret_cast<Rec*>(stage + (before[p] + below[p]) * rec) = r[p];  // alignment 1: packed
  __syncthreads();

  const int bytes = n * rec;
  const int head = min(bytes, (16 - shift) & 15);  // up to the first 16-byte boundary
  const int vecs = (bytes - head) >> 4;
  const int tail = bytes - head - (vecs << 4);
  if (t < head) out[t] = stage[t];
  // stage + head and out + head are both 16-byte aligned (when vecs > 0)
  const uint4* lv = reinterpret_cast<const uint4*>(stage + head);
  uint4* gv = reinterpret_cast<uint4*>(out + head);
  for (int i = t; i < vecs; i += kThreads) gv[i] = lv[i];
  const int done = head + (vecs << 4);
  if (t < tail) out[done + t] = stage[done + t];
}

}  // namespace

int point_cloud_tiles(int h, int w, int step) {
  const long long hs = (h + step - 1) / step, ws = (w + step - 1) / step;
  return (int)((hs * ws + kTile - 1) / kTile);
}

size_t point_cloud_ws_bytes(int B, int h, int w, int step) {
  return (size_t)B * point_cloud_tiles(h, w, step) * sizeof(int);
}

// Checks nothing: the one caller, mde_op_point_cloud in ops_abi.hip, has refused null pointers,
// non-positive sizes, a sampled grid of 2^31 - 256 samples or more (int sample index), batch >
// 65535 (grid.y), a short records buffer or workspace and a missing focal length.
hipError_t launch_point_cloud(const float* depth, int B, int h, int w, int step, const unsigned char* photo, int pitch,
                              int swap_rb, const float* f_px_dev, float fx, float fy, float cx, float cy, int compact,
                              float z_lo, float z_hi, void* records, int* counts, void* ws, hipStream_t st) {
  Geom g;
  g.h = h, g.w = w, g.step = step;
  g.hs = (h + step - 1) / step, g.ws = (w + step - 1) / step;
  const int tiles = point_cloud_tiles(h, w, step);
  const dim3 grid((unsigned)tiles, (unsigned)B), block(kThreads);
  int* tile_count = static_cast<int*>(ws);
  unsigned char* rec = static_cast<unsigned char*>(records);
#define PC_WRITE(COMPACT, COLOUR)                                                                                  \
  hipLaunchKernelGGL((pc_write_kernel<COMPACT, COLOUR>), grid, block, 0, st, depth, g, photo, pitch, swap_rb,      \
                     f_px_dev, fx, fy, cx, cy, z_lo, z_hi, rec, tile_count, counts, tiles)
  if (!compact) {
    if (photo) PC_WRITE(false, true); else PC_WRITE(false, false);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(pc_count_kernel, grid, block, 0, st, depth, g, z_lo, z_hi, tile_count, tiles);
  hipLaunchKernelGGL(pc_scan_kernel, dim3((unsigned)B), dim3(kScanThreads), 0, st, tile_count, tiles, counts);
  if (photo) PC_WRITE(true, true); else PC_WRITE(true, false);
#undef PC_WRITE
  return hipGetLastError();
}

}  // namespace mde
