"""Test helper (not a test module): maps for the bilinear upsampling sites,
float64 references of the resize, of the upsampling 3x3 conv and of the depth
head, and per-element bounds that come from the reference alone.

Sites.  Every one computes PyTorch's align_corners bilinear with the fp32
source coordinate of mde_device.h ac_scale / ac_index:
  f16 lerp   a + (b - a) w in packed f16, x then y, the weight rounded to f16:
             resize_kernel / the res1_up epilogue (upsample8), conv3_kernel's
             four-tap loader and upconv_kernel's two passes (lerp8);
  fp32 blend ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d) in fp32, rounded once to
             f16: the tile GEMM's A_CONV3_UP loader (gemm.hip), which takes the
             conv3x3_up / depth_head problems whose input channels are no
             multiple of 32;
  fp32       the same formula on fp32 maps: resize32, depth_postprocess.

Reference.  Source coordinate dst (in - 1) / (out - 1) in float64 (0 when out
== 1), floor, +1 neighbour clamped, the blend in float64; the 3x3 conv over
the upsampled map with ZERO padding.  The kernels' coordinate is the fp32
fl(fl((in - 1) / (out - 1)) dst): two roundings, so it differs from the
float64 one by at most DELTA(in) = 2^-23 in (> 2 x 2^-24 (in - 1), second order
included).  The blend is continuous and piecewise linear in the coordinate --
also across an integer hit, where a different floor yields the same value --
so the result moves by at most DELTA times the steepest tap difference next
to the cell: coord_term() takes the largest |horizontal| and |vertical|
neighbour difference over the 3 x 3 pixels around (y0, x0).

Map families (every value an f16 value with |v| <= 2^14, so that b - a, at
most 2^15, cannot overflow f16 in the lerp form; every channel differs and
the images of a batch differ):
  gauss    3 N(0, 1)
  ramp     a steep plane, 4096 (p_c x / (w - 1) - q_c y / (h - 1)) (1 + b) / B with
           p_c = (1 + c % 5) / 5, q_c = (1 + c % 7) / 7: a coordinate error is
           amplified by the slope
  checker  (-1)^(x + y + c + b) 2^(c % 6) (1 + (x + 2 y) % 3 / 4): the largest tap differences
  impulse  one nonzero pixel in every 5 x 5 cell, at (c % 5, c // 5 % 5) of the
           cell (+ b): over 25 channels it visits the last row, the last
           column and every tile seam; the rest is exactly 0, so is the bound
  dyadic   4 i, integer |i| <= R <= 64, for the exact shapes

Exact shapes.  n -> 2 n - 1, n -> 4 n - 3, n -> n, 2 n - 1 -> n and out == 1:
the fp32 scale is 1/2, 1/4, 1, 2 or 0 and every fp32 coordinate exact, the
weights in {0, 1/4, 1/2, 3/4}.  On a dyadic map: b - a is a multiple of 4 up
to 8 R (exact), (b - a) w an integer up to 6 R, t = a + (b - a) w an integer
up to 4 R; t1 - t0 an integer up to 8 R, (t1 - t0) w a multiple of 1/4 up to 6
R = 384 (1536 quarters: 11 bits) and the result a multiple of 1/4 up to 256.
Every step of the f16 lerp is exact, fused or not; the fp32 four-tap form is
exact a fortiori.  The upsampled map has ONE right value and every site is
held to equality with float64.  For the conv on top the upsampled values are
iu / 4 with |iu| <= 16 R and the weights iw / 64 on exact_cases' grid for K = 9
cin (int_range): products are multiples of 2^-8 and the test proves on its
own operands that sum |u| |w| stays below 2^24 of them, so fp32 accumulation
in any order is exact (test_bilinear_cases_cpu.py).

Bounds (U = 2^-11, the unit roundoff of f16).
  f16 lerp.  Taps a b (row y0), c d (row y1), wx, wy the weights, D = max(|b -
  a|, |d - c|), M = max |tap|, t0 t1 the exact row blends.  Level 1, unfused:
  fl(b - a), the f16 weight and the product each carry a relative U on a term
  of at most D; the sum one U on |t| <= M: e1 <= 3 U D + U M.  Level 2 the same
  on t1^ - t0^, whose inherited error is the convex combination of the two
  e1: e <= U (3 D + 3 |t1 - t0| + 2 M), first order.  A fused multiply-add
  only removes roundings.  The terms of order U^2 (6 U e1 and the like) are
  under 1 % of that and sit in the slack of w < 1; f16 subnormal results
  (gauss values times a tiny weight) add at most 2^-25 per operation, 6
  operations: TINY = 3 x 2^-24.  Plus coord_term().  The final rounding to f16
  is the level-2 U M: no separate half ulp.
  fp32 blend.  Half an f16 ulp of the reference (taken at |ref| + the rest,
  for a binade edge) + MARGIN x the error of the same fp32 formula with the
  same fp32 coordinates on the CPU, as the envelope E M: E the largest error
  / M of the case, M the local tap magnitude (ln_cases' convention), + coord_term().
  conv on top.  conv2d(bound_up, |w|) + MARGIN x the fp32-CPU accumulation error
  (envelope: the largest error / conv2d(|up|, |w|) of the case, times that) +
  half an f16 ulp for f16 outputs.  The head: relu is 1-Lipschitz, so the
  hidden bounds pass through sum_j |w2_j| . ; fp32 output, no ulp term.
  fp32 sites.  MARGIN x the error of torch's fp32 CPU F.interpolate against
  float64, as the envelope E M, + coord_term() (F.interpolate uses the same fp32
  coordinate, so E holds a sample of that term already).
MARGIN = 4 as in ln_cases: the kernels' other contraction and summation order.
"""

from __future__ import annotations

import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import exact_cases as X
from ln_cases import ulp16

U16 = 2.0 ** -11
TINY = 3 * 2.0 ** -24
MARGIN = 4.0
FAMILIES = ("gauss", "ramp", "checker", "impulse")      # general shapes; "dyadic" for the exact ones
USR, UTH, UPH = 12, 16, 18                               # conv.hip: source rows per tile, tile rows, patch rows
UPCONV_GRID = 768                                        # conv.hip upconv_grid: 3 workgroups x 256 CUs
DEFECTS = ("halfpixel", "scale_in_out", "swap_l", "swap_scales", "noclamp", "floor_int", "halo_replicate",
           "seam_drop")

# (sh, sw, uh, uw, the kernel a 32-channel conv3x3_up takes with "upconv" = 1): conv.hip upconv_eligible,
# restated in upconv_eligible() below and checked against this column by the CPU test
EXACT_SHAPES = [
    (10, 12, 19, 23, "upconv"),      # n -> 2 n - 1, two tile rows
    (6, 5, 21, 17, "upconv"),        # n -> 4 n - 3
    (12, 20, 12, 20, "upconv"),      # n -> n: 12 rows, the most an identity-size map may have
    (13, 20, 13, 20, "conv3_up"),    # n -> n with 13 rows: rows 0..13 are 14 source rows
    (19, 23, 10, 12, "conv3_up"),    # 2 n - 1 -> n, pure selection: 17 virtual rows span 19 source rows
    (5, 7, 1, 13, "conv3_up"),       # out == 1 (uh 1: below upconv's smallest height)
]
GENERAL_SHAPES = [
    (37, 40, 74, 70, "upconv"),      # the DPT ratios small: x 2 n and 296 -> 518; five tile rows, width 70
    (19, 13, 28, 37, "upconv"),      # tile 0 spans exactly 12 source rows
    (19, 13, 27, 37, "conv3_up"),    # ... 13 rows
    (1, 9, 2, 21, "upconv"),         # sh == 1, uh == 2: the smallest height upconv takes
    (7, 1, 18, 5, "upconv"),         # sw == 1
    (3, 11, 1, 30, "conv3_up"),      # uh == 1
    (8, 4, 14, 22, "upconv"),        # the fp32 coordinate of the last row and column lies above in - 1 (last_overshoots)
]
# (name, batch, cin, cout, sh, sw, uh, uw, switches, route): the routes of an A_CONV3_UP problem.  The exact
# shape of each comes first.  upconv_persist needs more than UPCONV_GRID tiles of 16 x 16: 28 images x 14 x 2 = 784
# (17 columns: the second tile column is one pixel wide, which keeps the reference small).
# kind=tile (cin 48, no multiple of 32): T128x32 for cout 32, T64 for cout 64 below M = 32768, T128x64 from
# there (183^2 = 33489), T128 for cout 128 from 240 tiles of 128^2 (M > 239 x 128 = 30592: 175^2 = 30625).
# Every route has an exact shape and a general one ("g").
UP_ROUTES = [
    ("conv3_up-32", 2, 32, 32, 10, 12, 19, 23, {"upconv": 0}, dict(kind="conv_direct", conv="conv3_up")),
    ("conv3_up-32g", 2, 32, 32, 19, 13, 28, 37, {"upconv": 0}, dict(kind="conv_direct", conv="conv3_up")),
    ("conv3_up-64", 2, 64, 32, 10, 12, 19, 23, {"upconv": 0}, dict(kind="conv_direct", conv="conv3_up")),
    ("conv3_up-64g", 2, 64, 32, 37, 40, 74, 70, {"upconv": 0}, dict(kind="conv_direct", conv="conv3_up")),
    ("conv3_up-256", 1, 256, 32, 10, 12, 19, 23, {}, dict(kind="conv_direct", conv="conv3_up")),
    ("conv3_up-256g", 1, 256, 32, 19, 13, 27, 37, {}, dict(kind="conv_direct", conv="conv3_up")),
    ("upconv-32", 2, 32, 32, 10, 12, 19, 23, {}, dict(kind="conv_direct", conv="upconv")),
    ("upconv-32g", 2, 32, 32, 19, 13, 28, 37, {}, dict(kind="conv_direct", conv="upconv")),
    ("upconv-64", 2, 64, 32, 6, 5, 21, 17, {}, dict(kind="conv_direct", conv="upconv")),
    ("upconv-64g", 2, 64, 32, 37, 40, 74, 70, {}, dict(kind="conv_direct", conv="upconv")),
    ("upconv-96", 2, 96, 32, 12, 20, 12, 20, {}, dict(kind="conv_direct", conv="upconv")),
    ("upconv-96g", 2, 96, 32, 7, 1, 18, 5, {}, dict(kind="conv_direct", conv="upconv")),
    ("upconv-128", 2, 128, 32, 10, 12, 19, 23, {}, dict(kind="conv_direct", conv="upconv")),
    ("upconv-128g", 2, 128, 32, 1, 9, 2, 21, {}, dict(kind="conv_direct", conv="upconv")),
    ("upconv_persist-32", 28, 32, 32, 112, 9, 223, 17, {}, dict(kind="conv_direct", conv="upconv_persist")),
    # 133 -> 224 rows: 12 of the 14 tile rows span exactly USR source rows, in workgroups that walk several tiles
    ("upconv_persist-32g", 28, 32, 32, 133, 10, 224, 17, {}, dict(kind="conv_direct", conv="upconv_persist")),
    ("tile128x32-48", 2, 48, 32, 10, 12, 19, 23, {}, dict(kind="tile", bm=128, bn=32)),
    ("tile128x32-48g", 2, 48, 32, 19, 13, 27, 37, {}, dict(kind="tile", bm=128, bn=32)),
    ("tile64-48", 2, 48, 64, 6, 5, 21, 17, {}, dict(kind="tile", bm=64, bn=64)),
    ("tile64-48g", 2, 48, 64, 37, 40, 74, 70, {}, dict(kind="tile", bm=64, bn=64)),
    ("tile128x64-48", 1, 48, 64, 92, 92, 183, 183, {}, dict(kind="tile", bm=128, bn=64)),
    ("tile128x64-48g", 1, 48, 64, 92, 92, 184, 184, {}, dict(kind="tile", bm=128, bn=64)),
    ("tile128-48", 1, 48, 128, 88, 88, 175, 175, {}, dict(kind="tile", bm=128, bn=128)),
    ("tile128-48g", 1, 48, 128, 88, 88, 176, 176, {}, dict(kind="tile", bm=128, bn=128)),
]
# the head (E_HEAD, 32 hidden channels): the same kernels; the tile route has one head tile, T128x32
HEAD_ROUTES = [r for r in UP_ROUTES if r[3] == 32 and r[0] not in ("conv3_up-256", "conv3_up-256g")]


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def is_exact(sh, sw, uh, uw):
    ok = lambda i, o: o == 1 or i == o or o == 2 * i - 1 or o == 4 * i - 3 or i == 2 * o - 1  # noqa: E731
    return ok(sh, uh) and ok(sw, uw)


# ---- maps -----------------------------------------------------------------------

@functools.lru_cache(maxsize=64)
def family_map(fam, B, C, h, w, R=64):
    """-> float64 [B][C][h][w], every value an f16 value, |v| <= 2^14."""
    g = gen("map", fam, B, C, h, w, R)
    b = torch.arange(B).view(B, 1, 1, 1).double()
    c = torch.arange(C).view(1, C, 1, 1).double()
    y = torch.arange(h).view(1, 1, h, 1).double()
    x = torch.arange(w).view(1, 1, 1, w).double()
    if fam == "gauss":
        v = 3.0 * torch.randn(B, C, h, w, generator=g, dtype=torch.float64)
    elif fam == "ramp":
        p, q = (1 + c % 5) / 5, (1 + c % 7) / 7
        v = 4096.0 * (p * x / max(w - 1, 1) - q * y / max(h - 1, 1)) * (1 + b) / B
    elif fam == "checker":
        v = (1 - 2 * ((x + y + c + b) % 2)) * 2.0 ** (c % 6) * (1 + ((x + 2 * y) % 3) / 4)
    elif fam == "impulse":
        hit = ((y + b) % 5 == c % 5) & ((x + b) % 5 == (c // 5) % 5)
        cell = torch.div(y, 5, rounding_mode="floor") + torch.div(x, 5, rounding_mode="floor")
        v = hit.double() * (1 - 2 * (cell % 2)) * (64.0 + 8 * c + b)
    elif fam == "dyadic":
        assert R <= 64
        v = 4.0 * torch.randint(-R, R + 1, (B, C, h, w), generator=g).double()
    else:
        raise ValueError(fam)
    v = v.expand(B, C, h, w).float().half().double().contiguous()
    assert float(v.abs().max()) <= 2.0 ** 14
    return v


def map_range(cin):
    """R of a dyadic map under a conv of cin input channels: the accumulator's
    standard deviation near exact_cases' SIGMA_Q quanta of 2^-8 -- upsampled
    values iu / 4 with |iu| <= 16 R against weights of int_range(9 cin)."""
    return max(2, min(64, X.int_range(9 * cin) // 8))


# ---- float64 reference (defect: one wrong formula built in) -----------------------

def axis64(n_in, n_out, defect=None, other=None):
    """-> (i0, i1, l1) of every destination index: float64 source coordinate.
    other = (in, out) of the other axis, for the swapped-scales defect."""
    dst = torch.arange(n_out, dtype=torch.float64)
    if defect == "halfpixel":
        src = ((dst + 0.5) * n_in / n_out - 0.5).clamp(min=0)
    elif defect == "scale_in_out":
        src = dst * n_in / n_out
    elif defect == "swap_scales":
        src = dst * (other[0] - 1) / (other[1] - 1) if other[1] > 1 else torch.zeros_like(dst)
    else:
        src = dst * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros_like(dst)
    src = src.clamp(max=n_in - 1)
    i0 = src.floor().long()
    l1 = src - i0
    if defect == "floor_int":       # an integer hit takes the pixel below it, whole
        hit = (l1 == 0) & (i0 > 0)
        i0 = torch.where(hit, i0 - 1, i0)
    if defect == "swap_l":
        l1 = 1 - l1
    i1 = i0 + 1 if defect == "noclamp" else i0 + (i0 < n_in - 1).long()
    return i0, i1, l1


def axis32(n_in, n_out):
    """The kernels' (and PyTorch's) fp32 coordinate: ac_scale, ac_index, each
    operation rounded to fp32."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    f = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = f.astype(np.int64)
    l1 = (f - i0.astype(np.float32)).astype(np.float32)
    i1 = i0 + (i0 < n_in - 1)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1)


def last_overshoots(n_in, n_out):
    """The fp32 coordinate of the last destination index lies above in - 1: its
    +1 neighbour then carries a weight of one fp32 ulp and must be clamped."""
    i0, _, l1 = axis32(n_in, n_out)
    return int(i0[-1]) == n_in - 1 and float(l1[-1]) > 0


def gather_taps(x, ya, xa):
    """x [B][C][h][w] read as the kernels do, [B][h][w][C] in one buffer (an
    unclamped +1 neighbour reads the next pixel / row / image; past the end,
    zeros) -> the four taps a b c d, each [B][C][uh][uw]."""
    B, C, h, w = x.shape
    flat = torch.cat([x.permute(0, 2, 3, 1).reshape(B * h * w, C), torch.zeros(w + 2, C, dtype=x.dtype)])
    base = (torch.arange(B) * h * w).view(B, 1, 1)
    y0, y1, _ = ya
    x0, x1, _ = xa

    def g(yy, xx):
        idx = base + yy.view(1, -1, 1) * w + xx.view(1, 1, -1)
        return flat[idx].permute(0, 3, 1, 2)
    return g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)


def up64(x, uh, uw, defect=None):
    """The float64 reference upsample of x [B][C][h][w] -> [B][C][uh][uw]."""
    h, w = x.shape[2:]
    if defect == "noclamp":
        # In float64 the last index hits in - 1 exactly and the unclamped
        # neighbour weighs 0: the defect shows only with the kernels' fp32
        # coordinate, where the last index can land one ulp above in - 1
        # (last_overshoots) and the next pixel / row gets that weight.
        ya, xa = ((i0, i0 + 1, l1.double()) for i0, _, l1 in (axis32(h, uh), axis32(w, uw)))
    else:
        ya, xa = axis64(h, uh, defect, (w, uw)), axis64(w, uw, defect, (h, uh))
    a, b, c, d = gather_taps(x, ya, xa)
    lx, ly = xa[2].view(1, 1, 1, -1), ya[2].view(1, 1, -1, 1)
    t0, t1 = a + (b - a) * lx, c + (d - c) * lx
    return t0 + (t1 - t0) * ly


def neighbour_slopes(x):
    """-> (sx, sy) [B][C][h][w]: the largest |horizontal| / |vertical| neighbour
    difference within the 3 x 3 pixels around each pixel."""
    dx, dy = torch.zeros_like(x), torch.zeros_like(x)
    dx[..., :-1] = (x[..., 1:] - x[..., :-1]).abs()
    dy[..., :-1, :] = (x[..., 1:, :] - x[..., :-1, :]).abs()
    pool = lambda t: F.max_pool2d(t, 3, 1, 1)  # noqa: E731
    return pool(dx), pool(dy)


def coord_term(x, uh, uw):
    """The fp32 coordinate against the float64 one: DELTA(in) x the steepest tap
    difference next to the cell, per axis."""
    h, w = x.shape[2:]
    ya, xa = axis64(h, uh), axis64(w, uw)
    sx, sy = neighbour_slopes(x)
    gx = gather_taps(sx, (ya[0], ya[0], None), (xa[0], xa[0], None))[0]
    gy = gather_taps(sy, (ya[0], ya[0], None), (xa[0], xa[0], None))[0]
    return 2.0 ** -23 * (w * gx * (uw > 1) + h * gy * (uh > 1))


def taps64(x, uh, uw):
    h, w = x.shape[2:]
    ya, xa = axis64(h, uh), axis64(w, uw)
    a, b, c, d = gather_taps(x, ya, xa)
    lx = xa[2].view(1, 1, 1, -1)
    return a, b, c, d, a + (b - a) * lx, c + (d - c) * lx


def bound_lerp(x, uh, uw):
    """The f16 lerp sites' per-element bound (module docstring)."""
    a, b, c, d, t0, t1 = taps64(x, uh, uw)
    D = torch.maximum((b - a).abs(), (d - c).abs())
    M = torch.stack([a.abs(), b.abs(), c.abs(), d.abs()]).amax(0)
    return U16 * (3 * D + 3 * (t1 - t0).abs() + 2 * M) + coord_term(x, uh, uw) + TINY * (M > 0)


def blend32(x, uh, uw):
    """ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d) in fp32 with the fp32
    coordinate, as gemm.hip's loader and the fp32 kernels write it."""
    h, w = x.shape[2:]
    ya, xa = axis32(h, uh), axis32(w, uw)
    a, b, c, d = (t.float() for t in gather_taps(x, ya, xa))
    lx1, ly1 = xa[2].view(1, 1, 1, -1), ya[2].view(1, 1, -1, 1)
    lx0, ly0 = 1 - lx1, 1 - ly1
    return ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)


def envelope(err, scale):
    """MARGIN x (the largest err / scale of the case) x scale, elementwise."""
    ok = scale > 0
    e = float((err[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0
    return MARGIN * e * scale


def tap_max(x, uh, uw):
    a, b, c, d, _, _ = taps64(x, uh, uw)
    return torch.stack([a.abs(), b.abs(), c.abs(), d.abs()]).amax(0)


def bound_blend32(x, uh, uw, f16_out=True):
    """The fp32-blend sites' bound; f16_out: rounded once to f16 (the tile
    GEMM's loader), else an fp32 output."""
    ref = up64(x, uh, uw)
    rest = envelope((blend32(x, uh, uw).double() - ref).abs(), tap_max(x, uh, uw)) + coord_term(x, uh, uw)
    return rest + 0.5 * ulp16(ref.abs() + rest) * (ref.abs() + rest > 0) if f16_out else rest


def bound_interp32(x, uh, uw):
    """The fp32 sites: MARGIN x torch's fp32 CPU F.interpolate against float64."""
    ref = up64(x, uh, uw)
    got = F.interpolate(x.float(), size=(uh, uw), mode="bilinear", align_corners=True).double()
    return envelope((got - ref).abs(), tap_max(x, uh, uw)) + coord_term(x, uh, uw)


# ---- emulations of the kernels' arithmetic (CPU test) -----------------------------

def lerp16(a, b, w, fused):
    """a + (b - a) w on f16 values; every operation rounded to f16, or the
    multiply-add fused (one rounding)."""
    d = b - a                                        # torch.half arithmetic: rounded
    if fused:
        return (a.double() + d.double() * w.double()).half()   # exact in float64 (11 + 11 bits, one add)
    return a + d * w


def up16_emulated(x, uh, uw, fused=False):
    """The two-level f16 lerp with the fp32 coordinate and the f16 weight."""
    h, w = x.shape[2:]
    ya, xa = axis32(h, uh), axis32(w, uw)
    a, b, c, d = (t.half() for t in gather_taps(x, ya, xa))
    lx, ly = xa[2].half().view(1, 1, 1, -1), ya[2].half().view(1, 1, -1, 1)
    return lerp16(lerp16(a, b, lx, fused), lerp16(c, d, lx, fused), ly, fused)


# ---- the upsampling conv ----------------------------------------------------------

def onehot_weights(cin, cout):
    """wt [cout][cin][3][3]: output channel j is tap j % 9 of input channel
    37 j % cin (37 is coprime to every cin here: all 8-channel chunks, the K
    tail of cin 48 included)."""
    wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    j = torch.arange(cout)
    wt[j, (37 * j) % cin, (j % 9) // 3, (j % 9) % 3] = 1.0
    return wt


def onehot_apply(t, cin, cout):
    """conv64(t, onehot_weights(cin, cout)) by indexing: output channel j is
    channel 37 j % cin of t shifted by tap j % 9, zero outside the map."""
    uh, uw = t.shape[2:]
    p = F.pad(t, (1, 1, 1, 1))
    return torch.stack([p[:, (37 * j) % cin, (j % 9) // 3:(j % 9) // 3 + uh, (j % 9) % 3:(j % 9) % 3 + uw]
                        for j in range(cout)], 1)


def conv_w16(cin, cout, key="w"):
    """Random-normal weights for the general shapes, f16 values: 0.5 N(0, 1) / sqrt(9 cin)
    (a ramp of 8192 stays below the f16 range), bias 0.02 N(0, 1) in fp32."""
    g = gen("upw16", cin, cout, key)
    wt = (0.5 * (9 * cin) ** -0.5 * torch.randn(cout, cin, 3, 3, generator=g)).half().double()
    return wt, (0.02 * torch.randn(cout, generator=g)).double()


def bound_head(hid, bound_hid, b1, w2, b2, hpe=None):
    """The metric = 0 head over hidden maps known to bound_hid: relu is
    1-Lipschitz, so sum_j |w2_j| bound_hid_j, + MARGIN x the fp32-CPU error of
    the dot product (envelope over sum_j relu(v_j) |w2_j| + |b2|)."""
    v = hid + b1.view(1, -1, 1, 1)
    if hpe is not None:
        v = v + hpe.T.reshape(1, 32, hid.shape[2], hid.shape[3])
    z = (F.relu(v) * w2.view(1, -1, 1, 1)).sum(1) + b2
    z32 = (F.relu(v.float()) * w2.float().view(1, -1, 1, 1)).sum(1) + b2
    scale = (F.relu(v) * w2.abs().view(1, -1, 1, 1)).sum(1) + abs(b2)
    return (bound_hid * w2.abs().view(1, -1, 1, 1)).sum(1) + envelope((z32.double() - z).abs(), scale)


def conv_w64(cin, cout, key="w"):
    """Weights iw / 64 on exact_cases' grid for K = 9 cin, bias ib / 256."""
    g = gen("upw", cin, cout, key)
    r = X.int_range(9 * cin)
    return X.ints(g, (cout, cin, 3, 3), r) / 64, X.ints(g, (cout,), 256) / 256


def conv64(up, wt, defect=None):
    """3x3 conv, pad 1, over the upsampled map: zero padding (the defect
    replicates the border instead)."""
    mode = "replicate" if defect == "halo_replicate" else "constant"
    return F.conv2d(F.pad(up, (1, 1, 1, 1), mode=mode), wt)


def seam_up64(x, uh, uw, ty):
    """The upsampled map as tile row ty of upconv_kernel would see it if its
    source-row count were clamped one short (USR - 1 instead of the span):
    the tile's last source row is not staged, and the H buffer holds there
    what the row USR slots earlier left behind (zero before any)."""
    h = x.shape[2]
    y0, y1, _ = axis64(h, uh)
    first, last = max(ty * UTH - 1, 0), min(ty * UTH - 1 + UPH - 1, uh - 1)
    lo, hi = int(y0[first]), int(y1[last])
    xs = x.clone()
    if hi - lo + 1 >= USR:           # the span fills the buffer: the clamp bites
        xs[:, :, hi] = x[:, :, hi - USR] if hi - USR >= 0 else 0.0
    return up64(xs, uh, uw)


def conv_up64(x, uh, uw, wt, defect=None):
    """conv3x3(upsample(x)) in float64 -> [B][cout][uh][uw]."""
    if defect == "seam_drop":
        out = conv64(up64(x, uh, uw), wt)
        for ty in range((uh + UTH - 1) // UTH):
            rows = slice(ty * UTH, min(ty * UTH + UTH, uh))
            out[:, :, rows] = conv64(seam_up64(x, uh, uw, ty), wt)[:, :, rows]
        return out
    return conv64(up64(x, uh, uw, None if defect == "halo_replicate" else defect), wt, defect)


def bound_conv(x, uh, uw, wt, bound_up, f16_out=True):
    """conv2d(bound_up, |w|) + MARGIN x the fp32-CPU accumulation error
    (envelope over conv2d(|up|, |w|)) [+ half an f16 ulp]."""
    up = up64(x, uh, uw)
    ref = conv64(up, wt)
    scale = conv64(up.abs(), wt.abs())
    acc = envelope((F.conv2d(F.pad(up.float(), (1, 1, 1, 1)), wt.float()).double() - ref).abs(), scale)
    rest = conv64(bound_up, wt.abs()) + acc
    return rest + 0.5 * ulp16(ref.abs() + rest) * (ref.abs() + rest > 0) if f16_out else rest


def head64(hid, b1, w2, b2, hpe=None):
    """relu(sum_j relu(hid_j + b1_j + hpe_j) w2_j + b2): the metric = 0 head over
    the conv's 32 hidden channels (hpe [uh uw][32], optional) -> [B][uh][uw]."""
    v = hid + b1.view(1, -1, 1, 1)
    if hpe is not None:
        v = v + hpe.T.reshape(1, 32, hid.shape[2], hid.shape[3])
    return F.relu((F.relu(v) * w2.view(1, -1, 1, 1)).sum(1) + b2)


def head_w(key="head"):
    """w2 from {+-1/4, +-1/2}, b2 = 1/8: products and sums stay on the 2^-10 grid."""
    g = gen("w2", key)
    w2 = torch.tensor([0.25, 0.5, -0.25, -0.5], dtype=torch.float64)[torch.randint(0, 4, (32,), generator=g)]
    return w2, 0.125


# ---- conv.hip's host policy restated ----------------------------------------------

def upconv_eligible(sh, uh):
    """conv.hip upconv_eligible's row test in the same fp32 arithmetic: every
    16-row tile's 18 virtual rows from at most USR source rows (and uh >= 2)."""
    if uh < 2:
        return False
    f = np.float32
    sy = f(sh - 1) / f(uh - 1)
    for ty in range((uh + UTH - 1) // UTH):
        iy0 = ty * UTH - 1
        first, last = max(iy0, 0), min(iy0 + UPH - 1, uh - 1)
        a0, l0 = int(f(sy * f(first))), int(f(sy * f(last)))
        if l0 + (1 if l0 < sh - 1 else 0) - a0 + 1 > USR:
            return False
    return True


def up_kernel(B, sh, uh, uw, upconv=1):
    """The conv= field of a 32-output-channel, 32..128-input-channel conv3x3_up."""
    if not (upconv and upconv_eligible(sh, uh)):
        return "conv3_up"
    return "upconv_persist" if B * ((uh + 15) // 16) * ((uw + 15) // 16) > UPCONV_GRID else "upconv"
