"""The bilinear upsampling sites against float64.

test_gpu_ops.py holds this family to 1e-2 + 1e-2 |ref| on random-normal data
and test_gpu_exact.py left it out.  Here every site that blends four taps is
compared with a float64 align_corners bilinear (bilinear_cases.py; its bounds
come from the reference alone and are proven in test_bilinear_cases_cpu.py):
on the exact shapes (ratios 1/2, 1/4, 1, 2, out == 1) with dyadic maps the
result has one right value and every site is held to EQUALITY; on the general
shapes every family is held to the per-element bound of the site's arithmetic.
Every GEMM-family case asserts its route, the conv.hip kernel included
(`conv=`), and every output starts as NaN.

1. The resize ops: mde_op_resize_bilinear (f16 lerp), mde_op_resize32 and
   mde_op_depth_postprocess (fp32, the latter with a clamp the map crosses on
   both sides), 8 and 72 channels.  The res1_up epilogue site needs nothing
   here: test_gpu_ops_engine_paths.py::test_conv_res1_up ties it bit for bit
   to mde_op_resize_bilinear.
2. The virtual map itself through each conv kernel: mde_op_conv3x3_up with
   one-hot weights, output channel j = tap j % 9 of input channel 37 j % cin,
   so the output IS the kernel's upsampled patch shifted by every tap, zero
   outside the map -- image border, tile seams and all nine taps in one
   launch.  conv3_kernel's four-tap loader at 32, 64 and 256 input channels,
   upconv_kernel per tile at 32 .. 128 and persistent (784 tiles), and the tile
   GEMM's fp32 register blend (cin 48) on its four tiles.  upconv_kernel and
   conv3_kernel at 32 channels are documented bit-identical: asserted.
3. Random weights on the same routes: conv3x3_up, depth_head, depth_head_pe;
   dyadic operands to equality (metric = 0), gauss and ramp to the conv bound,
   metric = 1 and 2 at the older head bar.
4. Both sides of the eligibility boundary: 19 -> 28 rows (12 source rows per
   tile) runs upconv_kernel, 19 -> 27 (13) conv3_kernel; an identity-size map
   of 12 rows upconv_kernel, of 13 rows conv3_kernel.

Every route has an exact shape and a general one.  The persistent kernel's
general shape, 133 -> 224 rows, puts 12 of its 14 tile rows at exactly 12 source
rows, in workgroups that walk several tiles through one H buffer.

Measured on an MI355X, the largest error / bound over all cases of a site (1
is the bound); every equality case held, and no kernel needed a change:
  resize_bilinear 0.856 (ramp 37 x 40 -> 74 x 70, the figure the CPU emulation
  of the unfused lerp gives); resize32 0.175; depth_postprocess 0.157;
  virtual map: conv3_kernel's loader 0.833, upconv_kernel 0.833 per tile (both
  ramp 37 x 40 -> 74 x 70, 64 channels; bit-identical at 32) and 0.910
  persistent (ramp 133 x 10 -> 224 x 17); the tile GEMM's loader 1.000 on ramp
  at the exact shapes on all four tiles -- the reference lies exactly half way
  between two f16 values there, the fp32 blend is exact and the error IS half
  an ulp -- and at most 0.997 otherwise;
  random weights: conv3x3_up 0.107 per tile / 0.136 persistent (f16 lerp
  routes), 0.266 .. 0.311 (the four tile routes); depth_head and depth_head_pe
  at most 0.018 -- conv2d(bound, |w|) is a worst-case sum;
  boundary 0.646 (19 -> 28 rows, ramp).

What this file catches that the older op tests do not (each defect built into
a scratch copy of the library; this file, test_gpu_ops.py,
test_gpu_ops_engine_paths.py, test_gpu_exact.py and test_gpu_gemm_route.py run
against it):
  * upconv_eligible's row test off by one (> USR + 1): the older files pass
    whole (653 cases); here test_eligibility_boundary[19 -> 27] and [13 -> 13]
    fail on the route record (conv=upconv where conv3_up is due).
  * the row halo replicated instead of zero in upconv_kernel's pass V: the
    older files notice too (23 cases at their 1e-2 bar: conv3x3_up,
    depth_head, upconv_matches_conv3, depth_head_pe); here 42 cases fail,
    every upconv and upconv_persist case of the three conv tests and both
    upconv sides of the boundary.
  * lx0 / lx1 swapped in the tile GEMM's A_CONV3_UP loader: the older files
    pass whole -- none runs that loader; here all 20 tile cases fail
    (virtual map and conv3x3_up on the four tiles, both heads).
"""

import pytest
import torch

import bilinear_cases as Bc
import exact_cases as X
from gpu_util import assert_equal, assert_route, close, conv_w, nhwc, op, ptr, stream, to16
from monocular_depth_estimation_trt_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = Bc.EXACT_SHAPES + Bc.GENERAL_SHAPES
SID = lambda s: "%dx%d-%dx%d" % s[:4]  # noqa: E731


def within(got, ref, bound, what):
    """|got - ref| <= bound per element (NaN never is); prints the largest
    error, and the largest error / bound where the bound is not zero."""
    g, r = got.detach().cpu().double(), ref.double()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    err = (g - r).abs()
    ok = bound > 0
    ratio = float((err / bound)[ok].nan_to_num(float("inf")).max()) if bool(ok.any()) else 0.0
    print(f"BILINEAR {what}: max err {float(err.nan_to_num(float('inf')).max()):.3e} max err/bound {ratio:.3f}")
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        idx = [int(v) for v in torch.unravel_index(torch.tensor(i), g.shape)]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound (worst {ratio:.3f} x), "
                             f"{int(torch.isnan(g).sum())} NaN; first {idx} got {float(g.flatten()[i])!r} "
                             f"ref {float(r.flatten()[i])!r} bound {float(bound.flatten()[i]):.3e}")


def families(exact):
    return ("dyadic",) + Bc.FAMILIES if exact else Bc.FAMILIES


# ---- 1. the resize ops ------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_resize_bilinear(gpu, shape):
    sh, sw, uh, uw, _ = shape
    B = 2
    for C in (8, 72):
        for fam in families(Bc.is_exact(sh, sw, uh, uw)):
            x = Bc.family_map(fam, B, C, sh, sw)
            out = torch.full((B, uh, uw, C), NAN, dtype=torch.float16, device=gpu)
            op("mde_op_resize_bilinear", ptr(nhwc(x).half().to(gpu)), B, sh, sw, C, uh, uw, ptr(out), stream())
            ref = nhwc(Bc.up64(x, uh, uw))
            what = f"resize_bilinear {fam} {SID(shape)} C {C}"
            if fam == "dyadic":
                assert_equal(out, to16(ref), what)
            else:
                within(out, ref, nhwc(Bc.bound_lerp(x, uh, uw)), what)


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_resize32(gpu, shape):
    sh, sw, uh, uw, _ = shape
    B = 2
    for C in (8, 72):
        for fam in families(Bc.is_exact(sh, sw, uh, uw)):
            x = Bc.family_map(fam, B, C, sh, sw)
            out = torch.full((B, uh, uw, C), NAN, dtype=torch.float32, device=gpu)
            op("mde_op_resize32", ptr(nhwc(x).float().to(gpu)), B, sh, sw, C, uh, uw, ptr(out), stream())
            ref = nhwc(Bc.up64(x, uh, uw))
            what = f"resize32 {fam} {SID(shape)} C {C}"
            if fam == "dyadic":
                assert_equal(out, ref.float(), what)
            else:
                within(out, ref, nhwc(Bc.bound_interp32(x, uh, uw)), what)


@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_depth_postprocess(gpu, shape):
    """One channel per image: the 72 channels of image 0 as a batch of 72
    depth maps; the clamp at +- a quarter of the map's range, which every
    family crosses on both sides (clamp is 1-Lipschitz: the same bound)."""
    sh, sw, uh, uw, _ = shape
    for fam in families(Bc.is_exact(sh, sw, uh, uw)):
        x = Bc.family_map(fam, 2, 72, sh, sw)[:1].transpose(0, 1).contiguous()    # [72][1][sh][sw]
        lo, hi = -0.25 * float(x.abs().max()), 0.25 * float(x.abs().max())
        lo, hi = float(torch.tensor(lo).float()), float(torch.tensor(hi).float())
        out = torch.full((72, uh, uw), NAN, dtype=torch.float32, device=gpu)
        op("mde_op_depth_postprocess", ptr(x[:, 0].float().contiguous().to(gpu)), 72, sh, sw, ptr(out), uh, uw, lo, hi,
           stream())
        up = Bc.up64(x, uh, uw)[:, 0]
        ref = up.clamp(lo, hi)
        if fam in ("dyadic", "gauss", "checker"):   # (a ramp over one row or column has one sign)
            assert bool((up < lo).any()) and bool((up > hi).any()), "the map must cross both clamp bounds"
        what = f"depth_postprocess {fam} {SID(shape)}"
        if fam == "dyadic":
            assert_equal(out, ref.float(), what)
        else:
            within(out, ref, Bc.bound_interp32(x, uh, uw)[:, 0], what)


# ---- 2. the virtual map through each conv kernel (one-hot weights) -----------------

def run_conv_up(gpu, x, uh, uw, wt, bias, act, switches):
    B, cin, sh, sw = x.shape
    cout = wt.shape[0]
    wp = conv_w(wt.float()).to(gpu)
    out = torch.full((B, uh, uw, cout), NAN, dtype=torch.float16, device=gpu)
    with _lib.tuning(**switches):
        op("mde_op_conv3x3_up", ptr(nhwc(x).half().to(gpu)), B, sh, sw, cin, uh, uw, ptr(wp), wp.shape[1], cout,
           ptr(bias.float().to(gpu)), act, ptr(out), stream())
    return out


def bound_up(route, x, uh, uw):
    """The upsampled map's bound for the arithmetic of the route's loader."""
    return Bc.bound_blend32(x, uh, uw) if route["kind"] == "tile" else Bc.bound_lerp(x, uh, uw)


@pytest.mark.parametrize("case", Bc.UP_ROUTES, ids=lambda c: c[0])
def test_virtual_map(gpu, case):
    name, B, cin, cout, sh, sw, uh, uw, switches, route = case
    wt = Bc.onehot_weights(cin, cout)
    for fam in families(Bc.is_exact(sh, sw, uh, uw)):
        x = Bc.family_map(fam, B, cin, sh, sw)
        out = run_conv_up(gpu, x, uh, uw, wt, torch.zeros(cout), 0, switches)
        assert_route(route, name)
        ref = nhwc(Bc.onehot_apply(Bc.up64(x, uh, uw), cin, cout))
        what = f"virtual map {name} {fam}"
        if fam == "dyadic":
            assert_equal(out, to16(ref), what)
        else:
            within(out, ref, nhwc(Bc.onehot_apply(bound_up(route, x, uh, uw), cin, cout)), what)
        if name.startswith("upconv-32"):   # conv.hip: the same two-level lerp in the same order, the same patch
            old = run_conv_up(gpu, x, uh, uw, wt, torch.zeros(cout), 0, {"upconv": 0})
            assert_route(dict(kind="conv_direct", conv="conv3_up"), name)
            assert torch.equal(out, old), f"{what}: upconv_kernel's patch differs from conv3_kernel's"


# ---- 3. random weights on the same routes ------------------------------------------

@pytest.mark.parametrize("case", Bc.UP_ROUTES, ids=lambda c: c[0])
def test_conv3x3_up(gpu, case):
    name, B, cin, cout, sh, sw, uh, uw, switches, route = case
    if Bc.is_exact(sh, sw, uh, uw):
        x = Bc.family_map("dyadic", B, cin, sh, sw, Bc.map_range(cin))
        wt, b = Bc.conv_w64(cin, cout)
        out = run_conv_up(gpu, x, uh, uw, wt, b, 0, switches)
        assert_route(route, name)
        assert_equal(out, to16(nhwc(Bc.conv_up64(x, uh, uw, wt) + b.view(1, -1, 1, 1))), f"conv3x3_up {name} dyadic")
        return
    wt, b = Bc.conv_w16(cin, cout)
    for fam in ("gauss", "ramp"):
        x = Bc.family_map(fam, B, cin, sh, sw)
        out = run_conv_up(gpu, x, uh, uw, wt, b.float().double(), 0, switches)
        assert_route(route, name)
        ref = Bc.conv_up64(x, uh, uw, wt) + b.float().double().view(1, -1, 1, 1)
        assert float(ref.abs().max()) < 60000.0
        within(out, nhwc(ref), nhwc(Bc.bound_conv(x, uh, uw, wt, bound_up(route, x, uh, uw))), f"conv3x3_up {name} {fam}")


def run_head(gpu, x, uh, uw, wt, b1, w2, b2, metric, hpe, switches):
    B, cin, sh, sw = x.shape
    wp = conv_w(wt.float()).to(gpu)
    out = torch.full((B, uh, uw), NAN, dtype=torch.float32, device=gpu)
    args = (ptr(nhwc(x).half().to(gpu)), B, sh, sw, cin, uh, uw, ptr(wp), wp.shape[1], ptr(b1.float().to(gpu)),
            ptr(w2.float().to(gpu)), b2, metric, 20.0)
    with _lib.tuning(**switches):
        if hpe is None:
            op("mde_op_depth_head", *args, ptr(out), stream())
        else:
            op("mde_op_depth_head_pe", *args, ptr(hpe.half().to(gpu)), hpe.shape[0], ptr(out), stream())
    return out


def head_route(route):
    return dict(kind="tile", bm=128, bn=32) if route["kind"] == "tile" else route


@pytest.mark.parametrize("pe", [0, 1], ids=["depth_head", "depth_head_pe"])
@pytest.mark.parametrize("case", Bc.HEAD_ROUTES, ids=lambda c: c[0])
def test_depth_head(gpu, case, pe):
    name, B, cin, _, sh, sw, uh, uw, switches, route = case
    hpe = X.resid16(Bc.gen("hpe", name), (uh * uw, 32)).double() if pe else None
    if Bc.is_exact(sh, sw, uh, uw):
        x = Bc.family_map("dyadic", B, cin, sh, sw, Bc.map_range(cin))
        wt, b1 = Bc.conv_w64(cin, 32)
        w2, b2 = Bc.head_w()
        out = run_head(gpu, x, uh, uw, wt, b1, w2, b2, 0, hpe, switches)
        assert_route(head_route(route), name)
        assert_equal(out, Bc.head64(Bc.conv_up64(x, uh, uw, wt), b1, w2, b2, hpe).float(), f"depth_head {name} dyadic pe {pe}")
        return
    wt, b1 = Bc.conv_w16(cin, 32)
    b1 = b1.float().double()
    w2 = (32 ** -0.5 * torch.randn(32, generator=Bc.gen("w2g", name))).float().double()
    b2 = 0.0625
    for fam in ("gauss", "ramp"):
        x = Bc.family_map(fam, B, cin, sh, sw)
        hid = Bc.conv_up64(x, uh, uw, wt)
        out = run_head(gpu, x, uh, uw, wt, b1, w2, b2, 0, hpe, switches)
        assert_route(head_route(route), name)
        bh = Bc.bound_conv(x, uh, uw, wt, bound_up(route, x, uh, uw), f16_out=False)
        within(out, Bc.head64(hid, b1, w2, b2, hpe), Bc.bound_head(hid, bh, b1, w2, b2, hpe), f"depth_head {name} {fam} pe {pe}")
    # metric 1 (sigmoid) and 2 (exp) at the older head bar, on gauss
    x = Bc.family_map("gauss", B, cin, sh, sw)
    v = Bc.conv_up64(x, uh, uw, wt) + b1.view(1, -1, 1, 1)
    if hpe is not None:
        v = v + hpe.T.reshape(1, 32, uh, uw)
    z = (torch.relu(v) * w2.view(1, -1, 1, 1)).sum(1) + b2
    for metric, ref in ((1, 20.0 * torch.sigmoid(z)), (2, torch.exp(z))):
        out = run_head(gpu, x, uh, uw, wt, b1, w2, b2, metric, hpe, switches)
        close(out, ref, 1e-2, 2e-2, f"depth_head {name} metric {metric} pe {pe}")


# ---- 4. both sides of the eligibility boundary --------------------------------------

@pytest.mark.parametrize("sh,sw,uh,uw,conv", [(19, 13, 28, 37, "upconv"), (19, 13, 27, 37, "conv3_up"),
                                             (12, 20, 12, 20, "upconv"), (13, 20, 13, 20, "conv3_up")])
def test_eligibility_boundary(gpu, sh, sw, uh, uw, conv):
    """Default switches, 32 channels: the kernel the route record names, and
    the virtual map within bounds either side (a source-row count clamped one
    short would blend a stale LDS row without a fault)."""
    B, cin = 2, 32
    wt = Bc.onehot_weights(cin, 32)
    route = dict(kind="conv_direct", conv=conv)
    for fam in ("dyadic",) if sh == uh else ("impulse", "ramp"):
        x = Bc.family_map(fam, B, cin, sh, sw)
        out = run_conv_up(gpu, x, uh, uw, wt, torch.zeros(32), 0, {})
        assert_route(route, f"{sh} -> {uh} rows")
        ref = nhwc(Bc.onehot_apply(Bc.up64(x, uh, uw), cin, 32))
        if fam == "dyadic":
            assert_equal(out, to16(ref), f"boundary {sh} -> {uh} {fam}")
        else:
            within(out, ref, nhwc(Bc.onehot_apply(Bc.bound_lerp(x, uh, uw), cin, 32)), f"boundary {sh} -> {uh} {fam}")
