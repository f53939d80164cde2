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
// file (_build.PER_FILE) and cloud_source.h's pragma, no fast-math flag in the build.
//
// Structure.  Tiles of 1024 samples, a sample's rank within its tile, the scan of the tiles' counts and
// the LDS-staged store are compact_store.h's (shared with depth_mesh.hip).
//   organized: pc_write_kernel<false> alone; a tile's first record index is its first sample index.
//   compact, three launches on the stream:
//     pc_count_kernel            tile_count[b][g]  = kept samples of tile g
//     tile_scan_kernel           tile_count[b][g] := exclusive prefix (one workgroup per image,
//                                walking the tiles 256 at a time with a running carry, so any
//                                number of tiles), counts[b] = total
//     pc_write_kernel<true>      evaluates the same keep() again, ranks, writes from the prefix
//   No workgroup ever waits on memory another workgroup writes: the order between the three
//   steps is the stream's.  (A single-pass look-back scan would spin on its predecessors' flags
//   and so rely on them being scheduled; it saves one read of the depth map, which is a quarter
//   of what the records cost to write.)  Integer counts and a fixed order: the result is the
//   same bits on every run.

#include <hip/hip_runtime.h>

#include <type_traits>

#include "compact_store.h"
#include "mde_ops.h"

namespace mde {
namespace {

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

template <bool COMPACT, bool COLOUR>
__global__ void __launch_bounds__(kThreads)
pc_write_kernel(const float* __restrict__ depth, Geom g, const unsigned char* __restrict__ photo, int pitch,
                int swap_rb, const float* __restrict__ f_px_dev, float fx, float fy, float cx, float cy, float z_lo,
                float z_hi, unsigned char* __restrict__ records, const int* __restrict__ tile_first,
                int* __restrict__ counts, int tiles) {
  using Rec = typename std::conditional<COLOUR, Rec15, Rec12>::type;
  constexpr int rec = (int)sizeof(Rec);
  __shared__ uint4 s_stage[stage_vecs(kTile * rec)];
  __shared__ int s_cnt[kSegs];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const int plane = g.hs * g.ws;
  // the camera arrives as loose arguments: a struct argument's fields are fetched from the kernarg segment
  // where they are first used, which put a second, dependent fetch in front of the first sample
  const Camera cam = {photo, f_px_dev, pitch, swap_rb, fx, fy, cx, cy};
  const Focal f = cam.focal(b);
  const float* img = depth + (size_t)b * g.h * g.w;

  Rec r[kPasses];
  bool k[kPasses];
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    int v = 0, u = 0;
    k[p] = sample_pixel(g, blockIdx.x * (unsigned)kTile + (unsigned)(p * kThreads + t), v, u);
    float z = 0.f;
    if (k[p]) {
      z = img[(size_t)v * g.w + u];
      if (COMPACT) k[p] = keep(z, z_lo, z_hi);
    }
    if (k[p]) r[p] = unproject<Rec, COLOUR>(g, cam, f, b, v, u, z);
  }
  int rank[kPasses];
  const int n = tile_ranks(k, rank, s_cnt);  // records of this tile
  // first record of the tile within the image's region
  const int first = COMPACT ? tile_first[(size_t)b * tiles + blockIdx.x] : (int)blockIdx.x * kTile;
  if (!COMPACT && blockIdx.x == 0 && t == 0) counts[b] = plane;

  unsigned char* out = records + ((size_t)b * plane + (size_t)first) * rec;  // g0
  unsigned char* stage = stage_base(s_stage, out);
#pragma unroll
  for (int p = 0; p < kPasses; ++p)
    if (k[p]) *reinterpret_cast<Rec*>(stage + rank[p] * rec) = r[p];  // alignment 1: packed
  staged_store(out, stage, n * rec);
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
hipError_t launch_point_cloud(const CloudSource& src, int compact, float z_lo, float z_hi, void* records, int* counts,
                              void* ws, hipStream_t st) {
  const Geom g = make_geom(src.h, src.w, src.step);
  const float* depth = src.depth;
  const int B = src.B, tiles = point_cloud_tiles(src.h, src.w, src.step);
  const dim3 grid((unsigned)tiles, (unsigned)B), block(kThreads);
  int* tile_count = static_cast<int*>(ws);
  unsigned char* rec = static_cast<unsigned char*>(records);
#define PC_WRITE(COMPACT, COLOUR)                                                                                  \
  hipLaunchKernelGGL((pc_write_kernel<COMPACT, COLOUR>), grid, block, 0, st, depth, g, src.photo, src.pitch,       \
                     src.swap_rb, src.f_px_dev, src.fx, src.fy, src.cx, src.cy, z_lo, z_hi, rec, tile_count,       \
                     counts, tiles)
  if (!compact) {
    if (src.photo) PC_WRITE(false, true); else PC_WRITE(false, false);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(pc_count_kernel, grid, block, 0, st, depth, g, z_lo, z_hi, tile_count, tiles);
  hipLaunchKernelGGL(tile_scan_kernel, dim3((unsigned)B), dim3(kScanThreads), 0, st, tile_count, tiles, counts);
  if (src.photo) PC_WRITE(true, true); else PC_WRITE(true, false);
#undef PC_WRITE
  return hipGetLastError();
}

}  // namespace mde
