// The cloud source on the device, as point_cloud.hip, depth_mesh.hip and cloud_view.hip see it: the sampled
// grid of a depth map, the camera (photo, focal lengths, centre) and the pinhole unprojection of one
// sample.  Device code in a header: each including file gets its own copy in its own anonymous namespace,
// and all three are built with -ffp-contract=off (_build.PER_FILE); the pragma below says the same for the
// unprojection here and for the rest of the including file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mde_ops.h"

#pragma clang fp contract(off)

namespace mde {
namespace {

struct Geom {
  int h, w, step, hs, ws;  // hs * ws < 2^31 - 256 (the ABI wrappers)
};

inline Geom make_geom(int h, int w, int step) {
  Geom g;
  g.h = h, g.w = w, g.step = step;
  g.hs = (h + step - 1) / step, g.ws = (w + step - 1) / step;
  return g;
}

struct Focal {
  float fx, fy;
};

struct Camera {
  const unsigned char* photo;  // [B][h][pitch], three bytes per pixel; null: no colours
  const float* f_px_dev;       // [B]; null: fx, fy
  int pitch, swap_rb;
  float fx, fy, cx, cy;

  // image b's focal lengths: the device's, when given, for both axes
  __device__ __forceinline__ Focal focal(int b) const {
    Focal f = {fx, fy};
    if (f_px_dev) f.fx = f.fy = f_px_dev[b];
    return f;
  }
};

inline Camera make_camera(const CloudSource& src) {
  return {src.photo, src.f_px_dev, src.pitch, src.swap_rb, src.fx, src.fy, src.cx, src.cy};
}

// sample s of an image -> its pixel; returns false past the grid's end
// (s is unsigned: the last tile's sample indices run up to 1023 past hs * ws, past INT_MAX for the
// largest grids the wrappers let through)
__device__ __forceinline__ bool sample_pixel(const Geom& g, unsigned s, int& v, int& u) {
  if (s >= (unsigned)(g.hs * g.ws)) return false;
  const int i = (int)(s / (unsigned)g.ws), j = (int)(s - (unsigned)i * (unsigned)g.ws);
  v = i * g.step;
  u = j * g.step;
  return true;
}

// X, Y of pixel (v, u) at depth z (Z = z): each float32 step rounded on its own
__device__ __forceinline__ void unproject_xy(const Camera& cam, Focal f, int v, int u, float z, float& X, float& Y) {
  const float xn = __fdiv_rn(__fsub_rn((float)u, cam.cx), f.fx);
  const float yn = __fdiv_rn(__fsub_rn((float)v, cam.cy), f.fy);
  X = __fmul_rn(xn, z);
  Y = __fmul_rn(yn, z);
}

// the photo's bytes of pixel (v, u) of image b in output order R, G, B (cam.photo is not null)
__device__ __forceinline__ void photo_rgb(const Camera& cam, const Geom& g, int b, int v, int u, unsigned char& r,
                                          unsigned char& gr, unsigned char& bl) {
  const unsigned char* px = cam.photo + ((size_t)b * g.h + v) * cam.pitch + 3 * (size_t)u;
  const unsigned char c0 = px[0], c1 = px[1], c2 = px[2];
  r = cam.swap_rb ? c2 : c0;
  gr = c1;
  bl = cam.swap_rb ? c0 : c2;
}

}  // namespace
}  // namespace mde
