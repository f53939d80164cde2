// Meshes: the tail of reference models/metric_anything/demo_pointcloud.py (:142-149), on the device.
// Metric depth at the photo's size is cleaned of depth edges (the flying pixels a bilinear resize
// leaves between foreground and background), the quads of the sampled grid whose four corners survive
// are split into two triangles each, and the vertices they use and the faces are packed as PLY
// binary_little_endian records.
//
// Contract: include/mde.h, mde_op_depth_mesh (pointcloud.py:mesh_np is the numpy restatement the tests
// hold these kernels to, byte for byte).  On the sampled grid of mde_op_point_cloud, all float32:
//   valid(i, j) = z == z && z >= z_lo && z <= z_hi
//   edge        = valid && ((atol > 0 && diff > atol) || (rtol > 0 && diff / z > rtol)), diff = zmax - zmin
//                 over the valid samples of the 3 x 3 neighbourhood clipped to the grid
//   clean       = valid && !edge
//   quad (i, j), i < hs - 1, j < ws - 1, corners a = (i, j), b = (i, j + 1), c = (i + 1, j + 1),
//                 d = (i + 1, j): kept iff all four are clean; |za - zc| <= |zb - zd| splits it along a-c
//                 into (a, d, c), (a, c, b), else along b-d into (a, d, b), (b, d, c)
//   vertex      = faces ? one of its up to four quads is kept : clean
//
// Rounding discipline: as point_cloud.hip -- __f*_rn per step, -ffp-contract=off for the file
// (_build.PER_FILE) and cloud_source.h's pragma.
//
// Structure.  Six launches on the stream (four without faces), none of which waits on memory another
// workgroup writes: the order between them is the stream's.
//   mesh_mark_kernel     2D tiles of 16 x 64 samples with a two-sample halo (a vertex's fate depends on
//                        the 5 x 5 window of depth around it: vertex <- quads at -1..0 <- clean at -1..+1
//                        <- valid at -2..+2).  The 20 x 68 window goes through LDS once, samples that are
//                        invalid or off the grid as NaN; then clean on 18 x 66, kept quads on 17 x 65 and
//                        one flag byte per sample of the tile into ws.
//   mesh_count_kernel    per 1024-sample tile (compact_store.h's, in row-major sample order -- the order
//                        of the records): vertices, and triangles = 2 x kept quads
//   tile_scan_kernel     twice: exclusive prefixes of both, vertex_counts[b], face_counts[b]
//   mesh_vertex_kernel   the flagged samples' records, ranked within the tile, through the staged store;
//                        each vertex's compacted index into the int32 map [B][hs][ws] in ws
//   mesh_face_kernel     26 bytes per kept quad (two 13-byte PLY list entries), the four corner indices
//                        from the map, through the same staged store
// Integer counts and a fixed order: the same bytes on every run.
//
// ws: int tile_vertices[B][tiles], int tile_triangles[B][tiles], int index[B][hs * ws],
//     uchar flags[B][hs * ws].

#include <hip/hip_runtime.h>

#include <type_traits>

#include "compact_store.h"
#include "mde_ops.h"

namespace mde {
namespace {

// the flag byte of a sample (pointcloud.py: F_*)
constexpr unsigned char kValid = 1, kEdge = 2, kClean = 4, kQuad = 8, kDiagBD = 16, kVertex = 32;

constexpr int kTH = 16, kTW = 64;  // the mark kernel's tile, kTH * kTW = 4 samples per thread
constexpr int kZH = kTH + 4, kZW = kTW + 4;  // depth window
constexpr int kCH = kTH + 2, kCW = kTW + 2;  // clean: samples -1 .. kT
constexpr int kQH = kTH + 1, kQW = kTW + 1;  // quads: samples -1 .. kT - 1
static_assert(kTH * kTW == kTile && kTW == 64, "a wave writes one row of 64 flag bytes");

struct __attribute__((packed)) Face {
  unsigned char n;
  int i0, i1, i2;
};
struct __attribute__((packed)) Face2 {
  Face t[2];
};
static_assert(sizeof(Face) == 13 && sizeof(Face2) == 26, "PLY face list entries are tightly packed");

__global__ void __launch_bounds__(kThreads)
mesh_mark_kernel(const float* __restrict__ depth, Geom g, float z_lo, float z_hi, float rtol, float atol, int faces,
                 int tiles_x, unsigned char* __restrict__ flags) {
  __shared__ float s_z[kZH][kZW];
  __shared__ unsigned char s_clean[kCH][kCW];
  __shared__ unsigned char s_quad[kQH][kQW];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int i0 = ty * kTH, j0 = tx * kTW;  // the tile's first sample
  const float* img = depth + (size_t)b * g.h * g.w;
  const float nan = __int_as_float(0x7fc00000);

  // the depth window: sample (i0 - 2 + li, j0 - 2 + lj); NaN = not valid
  for (int e = t; e < kZH * kZW; e += kThreads) {
    const int li = e / kZW, lj = e - li * kZW;
    const int i = i0 - 2 + li, j = j0 - 2 + lj;
    float z = nan;
    if (i >= 0 && i < g.hs && j >= 0 && j < g.ws) {
      z = img[(size_t)(i * g.step) * g.w + (size_t)(j * g.step)];
      if (!keep(z, z_lo, z_hi)) z = nan;
    }
    s_z[li][lj] = z;
  }
  __syncthreads();

  // valid, edge, clean of sample (i0 - 1 + li, j0 - 1 + lj) = s_z[li + 1][lj + 1]
  for (int e = t; e < kCH * kCW; e += kThreads) {
    const int li = e / kCW, lj = e - li * kCW;
    const float z = s_z[li + 1][lj + 1];
    unsigned char f = 0;
    if (z == z) {
      float zmax = z, zmin = z;
#pragma unroll
      for (int di = 0; di < 3; ++di)
#pragma unroll
        for (int dj = 0; dj < 3; ++dj) {
          const float q = s_z[li + di][lj + dj];
          if (q == q) {
            zmax = fmaxf(zmax, q);
            zmin = fminf(zmin, q);
          }
        }
      const float diff = __fsub_rn(zmax, zmin);
      const bool edge = (atol > 0.f && diff > atol) || (rtol > 0.f && __fdiv_rn(diff, z) > rtol);
      f = kValid | (edge ? kEdge : kClean);
    }
    s_clean[li][lj] = f;
  }
  __syncthreads();

  // quad of sample (i0 - 1 + li, j0 - 1 + lj): a corner off the grid is not clean
  for (int e = t; e < kQH * kQW; e += kThreads) {
    const int li = e / kQW, lj = e - li * kQW;
    const unsigned char all = s_clean[li][lj] & s_clean[li][lj + 1] & s_clean[li + 1][lj + 1] & s_clean[li + 1][lj];
    s_quad[li][lj] = (all & kClean) != 0;
  }
  __syncthreads();

  unsigned char* out = flags + (size_t)b * g.hs * g.ws;
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const int li = p * (kThreads / kTW) + t / kTW, lj = t % kTW;
    const int i = i0 + li, j = j0 + lj;
    if (i >= g.hs || j >= g.ws) continue;
    unsigned char f = s_clean[li + 1][lj + 1];
    const bool own = s_quad[li + 1][lj + 1];
    if (own) {
      const float za = s_z[li + 2][lj + 2], zb = s_z[li + 2][lj + 3];
      const float zc = s_z[li + 3][lj + 3], zd = s_z[li + 3][lj + 2];
      f |= kQuad;
      if (!(fabsf(__fsub_rn(za, zc)) <= fabsf(__fsub_rn(zb, zd)))) f |= kDiagBD;
    }
    const bool vertex = faces ? (own || s_quad[li][lj] || s_quad[li][lj + 1] || s_quad[li + 1][lj]) : (f & kClean) != 0;
    if (vertex) f |= kVertex;
    out[(size_t)i * g.ws + j] = f;
  }
}

// tile_v[b][g] = vertices of tile g, tile_t[b][g] = triangles (2 per kept quad); tile_t null: no faces
__global__ void __launch_bounds__(kThreads)
mesh_count_kernel(const unsigned char* __restrict__ flags, int plane, int* __restrict__ tile_v,
                  int* __restrict__ tile_t, int tiles) {
  __shared__ int s_v[kThreads / 64], s_q[kThreads / 64];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const unsigned char* fl = flags + (size_t)b * plane;
  int nv = 0, nq = 0;  // wave-uniform
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const unsigned s = blockIdx.x * (unsigned)kTile + (unsigned)(p * kThreads + t);
    const unsigned char f = s < (unsigned)plane ? fl[s] : (unsigned char)0;
    nv += __popcll(__ballot((f & kVertex) != 0));
    nq += __popcll(__ballot((f & kQuad) != 0));
  }
  if ((t & 63) == 0) s_v[t >> 6] = nv, s_q[t >> 6] = nq;
  __syncthreads();
  if (t == 0) {
    int v = 0, q = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) v += s_v[i], q += s_q[i];
    tile_v[(size_t)b * tiles + blockIdx.x] = v;
    if (tile_t) tile_t[(size_t)b * tiles + blockIdx.x] = 2 * q;
  }
}

template <bool COLOUR>
__global__ void __launch_bounds__(kThreads)
mesh_vertex_kernel(const float* __restrict__ depth, Geom g, const unsigned char* __restrict__ photo, int pitch,
                   int swap_rb, const float* __restrict__ f_px_dev, float fx, float fy, float cx, float cy,
                   const unsigned char* __restrict__ flags, unsigned char* __restrict__ records,
                   const int* __restrict__ tile_first, int* __restrict__ index, int tiles) {
  using Rec = typename std::conditional<COLOUR, Rec15, Rec12>::type;
  constexpr int rec = (int)sizeof(Rec);
  __shared__ uint4 s_stage[stage_vecs(kTile * rec)];
  __shared__ int s_cnt[kSegs];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const int plane = g.hs * g.ws;
  // loose arguments, not a Camera: see pc_write_kernel (point_cloud.hip)
  const Camera cam = {photo, f_px_dev, pitch, swap_rb, fx, fy, cx, cy};
  const Focal f = cam.focal(b);
  const float* img = depth + (size_t)b * g.h * g.w;
  const unsigned char* fl = flags + (size_t)b * plane;

  Rec r[kPasses];
  bool k[kPasses];
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    int v = 0, u = 0;
    const unsigned s = blockIdx.x * (unsigned)kTile + (unsigned)(p * kThreads + t);
    k[p] = sample_pixel(g, s, v, u) && (fl[s] & kVertex) != 0;
    if (k[p]) r[p] = unproject<Rec, COLOUR>(g, cam, f, b, v, u, img[(size_t)v * g.w + u]);
  }
  int rank[kPasses];
  const int n = tile_ranks(k, rank, s_cnt);
  const int first = tile_first[(size_t)b * tiles + blockIdx.x];  // the tile's first vertex of image b
  unsigned char* out = records + ((size_t)b * plane + (size_t)first) * rec;
  unsigned char* stage = stage_base(s_stage, out);
  int* idx = index + (size_t)b * plane;
#pragma unroll
  for (int p = 0; p < kPasses; ++p)
    if (k[p]) {
      *reinterpret_cast<Rec*>(stage + rank[p] * rec) = r[p];  // alignment 1: packed
      idx[blockIdx.x * (unsigned)kTile + (unsigned)(p * kThreads + t)] = first + rank[p];
    }
  staged_store(out, stage, n * rec);
}

// quads: 2 * (hs - 1) * (ws - 1), the triangles of one image's region
__global__ void __launch_bounds__(kThreads)
mesh_face_kernel(Geom g, const unsigned char* __restrict__ flags, const int* __restrict__ index,
                 unsigned char* __restrict__ face_records, long long region_faces, const int* __restrict__ tile_first,
                 int tiles) {
  constexpr int rec = (int)sizeof(Face2);
  __shared__ uint4 s_stage[stage_vecs(kTile * rec)];
  __shared__ int s_cnt[kSegs];
  const int b = (int)blockIdx.y, t = (int)threadIdx.x;
  const int plane = g.hs * g.ws;
  const unsigned char* fl = flags + (size_t)b * plane;
  const int* idx = index + (size_t)b * plane;

  Face2 r[kPasses];
  bool k[kPasses];
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const unsigned s = blockIdx.x * (unsigned)kTile + (unsigned)(p * kThreads + t);
    const unsigned char f = s < (unsigned)plane ? fl[s] : (unsigned char)0;
    k[p] = (f & kQuad) != 0;  // only where i < hs - 1 and j < ws - 1: s + ws + 1 < plane
    if (k[p]) {
      const int a = idx[s], bb = idx[s + 1u], c = idx[s + (unsigned)g.ws + 1u], d = idx[s + (unsigned)g.ws];
      const bool bd = (f & kDiagBD) != 0;
      r[p].t[0].n = 3, r[p].t[0].i0 = a, r[p].t[0].i1 = d, r[p].t[0].i2 = bd ? bb : c;
      r[p].t[1].n = 3, r[p].t[1].i0 = bd ? bb : a, r[p].t[1].i1 = bd ? d : c, r[p].t[1].i2 = bd ? c : bb;
    }
  }
  int rank[kPasses];
  const int n = tile_ranks(k, rank, s_cnt);                      // kept quads of this tile
  const int first = tile_first[(size_t)b * tiles + blockIdx.x];  // the tile's first triangle of image b
  unsigned char* out = face_records + ((size_t)b * (size_t)region_faces + (size_t)first) * sizeof(Face);
  unsigned char* stage = stage_base(s_stage, out);
#pragma unroll
  for (int p = 0; p < kPasses; ++p)
    if (k[p]) *reinterpret_cast<Face2*>(stage + rank[p] * rec) = r[p];  // alignment 1: packed
  staged_store(out, stage, n * rec);
}

int mesh_tiles(const Geom& g) { return (int)(((long long)g.hs * g.ws + kTile - 1) / kTile); }

}  // namespace

size_t depth_mesh_ws_bytes(int B, int h, int w, int step) {
  const Geom g = make_geom(h, w, step);
  const size_t plane = (size_t)g.hs * g.ws;
  return (size_t)B * ((size_t)mesh_tiles(g) * 2 * sizeof(int) + plane * sizeof(int) + plane);
}

// Checks nothing: the one caller, mde_op_depth_mesh in ops_abi.hip, has refused what
// mde_op_point_cloud refuses, 2 * (hs - 1) * (ws - 1) of 2^31 - 256 or more with faces (int triangle
// index), bad tolerances, short buffers and a ws that is not 4-byte aligned.
hipError_t launch_depth_mesh(const CloudSource& src, float z_lo, float z_hi, float edge_rtol, float edge_atol,
                             int faces, void* vertices, int* vertex_counts, void* face_records, int* face_counts,
                             void* ws, hipStream_t st) {
  const Geom g = make_geom(src.h, src.w, src.step);
  const float* depth = src.depth;
  const int B = src.B;
  const int plane = g.hs * g.ws, tiles = mesh_tiles(g);
  int* tile_v = static_cast<int*>(ws);
  int* tile_t = tile_v + (size_t)B * tiles;
  int* index = tile_t + (size_t)B * tiles;
  unsigned char* flags = reinterpret_cast<unsigned char*>(index + (size_t)B * plane);
  const int tiles_x = (g.ws + kTW - 1) / kTW, tiles_y = (g.hs + kTH - 1) / kTH;  // tiles_x * tiles_y < 2^31 / 16
  const dim3 grid((unsigned)tiles, (unsigned)B), block(kThreads);

  hipLaunchKernelGGL(mesh_mark_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)B), block, 0, st, depth, g, z_lo,
                     z_hi, edge_rtol, edge_atol, faces, tiles_x, flags);
  hipLaunchKernelGGL(mesh_count_kernel, grid, block, 0, st, flags, plane, tile_v, faces ? tile_t : nullptr, tiles);
  hipLaunchKernelGGL(tile_scan_kernel, dim3((unsigned)B), dim3(kScanThreads), 0, st, tile_v, tiles, vertex_counts);
  if (faces)
    hipLaunchKernelGGL(tile_scan_kernel, dim3((unsigned)B), dim3(kScanThreads), 0, st, tile_t, tiles, face_counts);
  unsigned char* rec = static_cast<unsigned char*>(vertices);
#define MESH_VERTEX(COLOUR)                                                                                       \
  hipLaunchKernelGGL(mesh_vertex_kernel<COLOUR>, grid, block, 0, st, depth, g, src.photo, src.pitch, src.swap_rb, \
                     src.f_px_dev, src.fx, src.fy, src.cx, src.cy, flags, rec, tile_v, index, tiles)
  if (src.photo) MESH_VERTEX(true); else MESH_VERTEX(false);
#undef MESH_VERTEX
  if (faces)
    hipLaunchKernelGGL(mesh_face_kernel, grid, block, 0, st, g, flags, index, static_cast<unsigned char*>(face_records),
                       2LL * (g.hs - 1) * (g.ws - 1), tile_t, tiles);
  return hipGetLastError();
}

}  // namespace mde
