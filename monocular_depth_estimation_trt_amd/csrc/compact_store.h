// What point_cloud.hip and depth_mesh.hip share on top of cloud_source.h (the sampled grid, the camera,
// the unprojection and the fp-contract story): the PLY vertex record, a sample's rank among the kept
// ones of its tile, the scan of the tiles' counts and the LDS-staged store of a tile's odd-sized records.
// Device code in a header: each of the two files gets its own copy in its own anonymous namespace.
//
// Tiles.  A workgroup of 256 threads owns kTile = 1024 consecutive samples of one image; thread t takes
// samples t, t + 256, t + 512, t + 768 of the tile, so a wave reads 64 consecutive elements per load.  A
// sample's rank among the kept ones of its tile is the number of kept lanes below it (one ballot) plus
// the kept counts of the 16 (pass, wave) segments before its own.
//
// Store path.  A tile's records are one contiguous byte range [g0, g0 + n * rec) that starts at any
// alignment (rec is odd; and a compacted tile starts wherever its predecessors ended).  The records are
// staged in LDS at byte (g0 & 15) + rank * rec, i.e. with the same alignment modulo 16 as in global
// memory; then the 16-byte aligned middle of the range goes out as uint4 LDS loads and uint4 global
// stores (a wave writes 1 KiB contiguous per instruction) and the up to 15 bytes before and after it as
// single-byte stores.  A dword that two tiles share is never read or written whole: each tile stores
// exactly its own bytes.
#pragma once

#include "cloud_source.h"

namespace mde {
namespace {

constexpr int kThreads = 256;                 // 4 waves of 64
constexpr int kPasses = 4;                    // samples per thread
constexpr int kTile = kThreads * kPasses;     // samples per workgroup
constexpr int kSegs = kPasses * (kThreads / 64);
constexpr int kScanThreads = 256;             // tile_scan_kernel's one workgroup per image

static_assert(kThreads % 64 == 0, "ballots below are over wave64");

struct __attribute__((packed)) Rec12 {
  float x, y, z;
};
struct __attribute__((packed)) Rec15 {
  float x, y, z;
  unsigned char r, g, b;
};
static_assert(sizeof(Rec12) == 12 && sizeof(Rec15) == 15, "PLY vertex records are tightly packed");

// the one statement of validity: every kernel must agree on every sample
__device__ __forceinline__ bool keep(float z, float z_lo, float z_hi) { return z == z && z >= z_lo && z <= z_hi; }

// the record of pixel (v, u) of image b at depth z
template <typename Rec, bool COLOUR>
__device__ __forceinline__ Rec unproject(const Geom& g, const Camera& cam, Focal f, int b, int v, int u, float z) {
  Rec r;
  float X, Y;  // a packed field does not bind to a reference
  unproject_xy(cam, f, v, u, z, X, Y);
  r.x = X, r.y = Y, r.z = z;
  if constexpr (COLOUR) {
    unsigned char red, green, blue;
    photo_rgb(cam, g, b, v, u, red, green, blue);
    r.r = red, r.g = green, r.b = blue;
  }
  return r;
}

// rank[p] := the number of kept samples of the tile before this thread's sample of pass p, in sample
// order; returns the tile's number of kept samples.  s_cnt: kSegs ints of LDS.  Holds a __syncthreads:
// every thread of the workgroup calls it, once per s_cnt.
__device__ __forceinline__ int tile_ranks(const bool (&k)[kPasses], int (&rank)[kPasses], int* s_cnt) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {
    const unsigned long long m = __ballot(k[p]);
    rank[p] = __popcll(m & ((1ull << lane) - 1ull));  // kept lanes of the same wave and pass below this one
    if (lane == 0) s_cnt[p * (kThreads / 64) + wave] = __popcll(m);
  }
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int s = 0; s < kSegs; ++s) {
    const int c = s_cnt[s];
#pragma unroll
    for (int p = 0; p < kPasses; ++p)
      if (s < p * (kThreads / 64) + wave) rank[p] += c;
    n += c;
  }
  return n;
}

// whole uint4 of LDS for a tile's `bytes` behind up to 15 bytes of alignment shift
constexpr int stage_vecs(int bytes) { return (bytes + 15 + 15) / 16; }

// where a tile that goes to `out` stages its first byte: s_stage + (out & 15)
__device__ __forceinline__ unsigned char* stage_base(uint4* s_stage, const unsigned char* out) {
  return reinterpret_cast<unsigned char*>(s_stage) + (reinterpret_cast<uintptr_t>(out) & 15);
}

// stage[0, bytes) (stage = stage_base(s_stage, out), filled by the workgroup's threads) -> out[0, bytes).
// Holds the __syncthreads between the LDS writes and these reads: every thread of the workgroup calls it.
__device__ __forceinline__ void staged_store(unsigned char* __restrict__ out, const unsigned char* stage, int bytes) {
  __syncthreads();
  const int t = (int)threadIdx.x;
  const int shift = (int)(reinterpret_cast<uintptr_t>(out) & 15);
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

// in place: tile_count[b][.] becomes its exclusive prefix, counts[b] the total; any number of tiles
__global__ void __launch_bounds__(kScanThreads)
tile_scan_kernel(int* __restrict__ tile_count, int tiles, int* __restrict__ counts) {
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

}  // namespace
}  // namespace mde
