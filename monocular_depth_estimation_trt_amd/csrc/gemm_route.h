// The route launch_gemm takes for a problem: which kernel family, which tile
// configuration, how many split-K slices.  gemm_route() decides (validation
// and policy, no device call); launch_gemm() launches from the decision and
// keeps a copy for the tests (mde_debug_last_gemm_route, include/mde.h).
// The table of routes and the rule behind each: DESIGN.md section 4b.
#pragma once

#include "mde_ops.h"

namespace mde {

enum GemmRouteKind : int {
  ROUTE_NONE = 0,      // empty problem (M or N <= 0): nothing to launch
  ROUTE_TILE,          // one gemm_kernel launch (gemm.hip)
  ROUTE_SPLIT_STORE,   // E_STORE split-K: `slices` K slices of gemm_kernel on 64^2 tiles
  ROUTE_SPLIT_RESID,   // E_RESID split-K: `slices` K slices on 64^2 or 128^2 tiles
  ROUTE_CONV_DIRECT,   // launch_conv3 on the kernel `conv` names (conv.hip: conv3_kernel_choice)
  ROUTE_PANEL,         // launch_panel_gemm (gemm_panel.hip)
  ROUTE_GEMM256        // launch_gemm256 (gemm256.hip)
};

struct GemmRoute {
  int kind = ROUTE_NONE;
  // TILE / SPLIT_*: the gemm_kernel instantiation -- block tile, wave grid,
  // K-step and LDS ring depth
  int bm = 0, bn = 0, wm = 0, wn = 0, bk = 0, stages = 0;
  int slices = 1;        // K slices (1 = unsplit)
  int fused = 0;         // SPLIT_*: the split tail fused into the slices' launch (GemmParams::tile_cnt);
                         // 0: slices into the workspace, then the reduce launch
  int resize_first = 0;  // res1_up written into res1 by a resize launch before this route
  int conv = 0;          // CONV_DIRECT: the ConvKernel (mde_ops.h) launch_conv3 launches
};

// Validates p as launch_gemm always has and picks its route.  hipSuccess with
// the route in r, or hipErrorInvalidValue (r unspecified).
hipError_t gemm_route(const GemmParams& p, GemmRoute& r);

// slices of p's route when p is an E_STORE problem (1 = no split, or no valid route)
inline int gemm_store_split_slices(const GemmParams& p) {
  GemmRoute r;
  return p.emode == E_STORE && gemm_route(p, r) == hipSuccess ? r.slices : 1;
}

// the route the calling thread's last launch_gemm acted on
const GemmRoute& gemm_last_route();

}  // namespace mde
