"""Exact-operand probes: the GEMM, conv and attention routes against float64.

The sibling files hold the hot path to about 20 half-ulps of f16 on
random-normal data, or bit for bit to another route of ours.  Here the
operands are chosen so that the kernels' fp32 arithmetic is exact
(exact_cases.py; its claims are proven in test_exact_cases_cpu.py).  The
result then does not depend on tile shape, K order, split or wave count:
the float64 reference rounded once to f16 (not at all for fp32 outputs) is
the only correct output, and every route is held to EQUALITY with it.  A
failure prints the number of differing elements, their (row, col) bounding
box and the largest difference in f16 ulps: the box is what localises a
tile or tail bug.

1. Linear / conv families, one case per route of launch_gemm
   (test_linear_strided's shapes, the smallest that reach each), every case
   asserting the route it took.  The exact-fp32 kernels (fp32.hip) keep no
   route record: those cases assert none.
2. GELU: every finite f16 value through every epilogue that has one, against
   the float64 erf form at 0.5 ulp16 + 2.6e-5 (the bound mde_device.h
   documents) + 2^-20 |ref| (v_exp_f32, v_rcp_f32), and every site equal to
   the 64^2-tile site for the same (a, b).
3. Attention: a selection probe (the output row is one V row) and a uniform
   probe (the output is V's constant column; one leaked pad key moves it to
   another f16 value) on every launch shape the suite forces, each asserting
   what the launcher's record (mde_debug_last_attention_route) says ran --
   a forced shape that cannot run at a size (four key groups over three key
   tiles, a split that collapses) asserts its documented fallback.

Out of scope, by design: the LN-fold routes (they contain rsqrt);
conv3x3_up and the head ops (bilinear weights, sigmoid: test_gpu_bilinear.py
holds them to float64) -- conv3x3_up here only at the source's own size,
where every blend weight is 0, for its GELU site (test_gelu_upconv, on a map
of 8 rows: upconv_kernel takes an identity-size map of at most 12); the persistent conv,
whose 1024-tile threshold makes its smallest shape the workload's own -- it is
tied bit for bit to the per-tile kernel (test_conv_persist_bit_exact), which
this file pins to float64.

Measured on an MI355X.  GELU, max(err - 0.5 ulp16) over the sweep (the bound
allows 2.6e-5 + 2^-20 |ref|): 2.516e-5 at x = -3.0857 on the 64^2 tiles and
the 128^2 BK 32 tiles, 2.512e-5 at x = -3.0916 on gemm256, 2.511e-5 at x =
-3.0671 on the 128^2 BK 64 tiles, both panel kernels, the split-K store, the
conv, conv3_kernel's upsampling form (route conv=conv3_up) and upconv_kernel's
scalar gelu_erf (route conv=upconv); every site equal to the 64^2-tile site.
erff (mde_op_linear32): 1.331e-3 of max(|ref|, 2^-14) at x = -5.5398.
attention32's selection probe: at most 1.8e-7 relative.

What the probes catch that the older op tests do not (each defect built into
a scratch copy of the library, test_gpu_ops.py and this file run against it):
  * gelu_erf2's x^4 coefficient 0.001014263055 -> 0.00102: in test_gpu_ops.py
    only test_panel_gemm_bit_exact[linear_gelu, lnfold_gelu] fail (the panel
    kernel's hand-unrolled copy no longer matches), no test against a
    reference; here every test_gelu_* case but test_gelu_linear32 fails.
  * the split-K store kernel rounding the sum to f16 before the bias:
    test_gpu_ops.py passes whole; here test_linear_split_store (both),
    test_linear_res[split_store-*] (all three) and the split conv3x3 case fail.
  * vt_pos taken as the identity in the QKV epilogues: test_qkv_layout fails
    (all 7 cases), and test_qkv here (all 3).
"""

import ctypes as C
import functools

import pytest
import torch

import exact_cases as X
from gpu_util import (assert_attn_route, assert_equal, assert_route, close, conv_w, nhwc, op, pad_w, ptr,
                      run_attention, stream, to16, vt_perm)
from monocular_depth_estimation_trt_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")


def ln_partials_ref(xh):
    """(sum, squared deviations from the slice mean) per 32-column slice and
    row of f16 rows, fp64, slice-major [k/32][m][2] (GemmParams::lnst_*)."""
    v = xh.double().reshape(xh.shape[0], -1, 32)
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([v.sum(-1), m2], -1).transpose(0, 1).contiguous()


def lin_dev(gpu, m, n, k):
    a, w, b, acc = X.lin_case(m, n, k)
    return a.half().to(gpu), pad_w(w.float()).to(gpu), b.float().to(gpu), acc + b


def workspace(gpu, floats=5 << 20):
    return torch.empty(floats, dtype=torch.float32, device=gpu)


IDS = lambda cases: [c[0] for c in cases]  # noqa: E731


# ---- 1. linear and conv routes: equality with float64 ---------------------------

@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("route,m,n,k,switches,want", X.LINEAR_ROUTES, ids=IDS(X.LINEAR_ROUTES))
def test_linear(gpu, route, m, n, k, switches, want, act):
    a, wp, b, pre = lin_dev(gpu, m, n, k)
    out = torch.full((m, n), NAN, dtype=torch.float16, device=gpu)
    with _lib.tuning(**switches):
        op("mde_op_linear", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), act, ptr(out), n, stream())
    assert_route(want, route)
    assert_equal(out, to16(X.act64(pre, act)), f"linear {route} {m}x{n}x{k} act {act}")


@pytest.mark.parametrize("act", [0, 1])
def test_linear_split_store(gpu, act):
    """mde_op_linear_ws: the split (slices into the workspace + the reduce
    launch of elementwise.hip) and, with "splitk" = 0, the unsplit tiles both
    equal float64 -- and hence each other."""
    m, n, k = X.SPLIT_SHAPE
    a, wp, b, pre = lin_dev(gpu, m, n, k)
    ref = to16(X.act64(pre, act))
    ws = workspace(gpu)
    for splitk in (1, 0):
        out = torch.full((m, n), NAN, dtype=torch.float16, device=gpu)
        sl = C.c_int(0)
        with _lib.tuning(splitk=splitk):
            op("mde_op_linear_ws", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), act, ptr(out), n, ptr(ws),
               ws.numel(), C.byref(sl), stream())
        if splitk:
            assert sl.value > 1
            assert_route(dict(kind="split_store", bm=64, bn=64, slices=sl.value, fused=0), "linear_ws")
        else:
            assert sl.value == 1
            assert_route(dict(kind="tile", slices=1), "linear_ws splitk 0")
        assert_equal(out, ref, f"linear_ws splitk {splitk} ({sl.value} slices) act {act}")


def resid_operands(gpu, m, n, k, f16):
    g = X.gen("resid", m, n, k, f16)
    ls = X.layerscale(g, n)
    x0 = X.resid16(g, (m, n))
    x0 = x0 if f16 else x0.float()
    _, _, b, acc = X.lin_case(m, n, k)
    return ls.to(gpu), x0.to(gpu), x0.double() + ls.double() * (acc + b)


@pytest.mark.parametrize("route,m,n,k,switches,want", X.RESID32_ROUTES, ids=IDS(X.RESID32_ROUTES))
def test_linear_residual(gpu, route, m, n, k, switches, want):
    """x += ls (a W^T + b) on the fp32 stream: exact in fp32."""
    a, wp, b, _ = lin_dev(gpu, m, n, k)
    ls, x, ref = resid_operands(gpu, m, n, k, 0)
    with _lib.tuning(**switches):
        op("mde_op_linear_residual", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), ptr(ls), ptr(x), n, stream())
    assert_route(want, route)
    assert_equal(x, ref.float(), f"linear_residual {route} {m}x{n}x{k}")


@pytest.mark.parametrize("route,m,n,k,switches,want", X.RESID16_ROUTES, ids=IDS(X.RESID16_ROUTES))
def test_linear_residual_f16(gpu, route, m, n, k, switches, want):
    """The f16 stream: fp32 update, one rounding.  The LN partials are not
    part of the exactness claim: against float64 of the op's own f16 output at
    test_linear_residual_f16's bar (n % 32 == 0: the ABI's condition)."""
    a, wp, b, _ = lin_dev(gpu, m, n, k)
    ls, xh, ref = resid_operands(gpu, m, n, k, 1)
    part = torch.full((n // 32, m, 2), NAN, device=gpu) if n % 32 == 0 else None
    with _lib.tuning(**switches):
        op("mde_op_linear_residual_f16", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), ptr(ls), ptr(xh), n,
           ptr(part), stream())
    assert_route(want, route)
    assert_equal(xh, to16(ref), f"linear_residual_f16 {route} {m}x{n}x{k}")
    if part is not None:
        close(part, ln_partials_ref(xh.cpu()).float(), 1e-5, 1e-3, f"{route} ln partials")


RES_ROUTES = X.RES_ROUTES + [("split_store",) + X.SPLIT_SHAPE + ({}, dict(kind="split_store", bm=64, bn=64, fused=0))]


@pytest.mark.parametrize("act,relu,with_r1", [(0, 0, 0), (1, 1, 0), (0, 0, 1)], ids=["res0", "res0_relu", "res1"])
@pytest.mark.parametrize("route,m,n,k,switches,want", RES_ROUTES, ids=IDS(RES_ROUTES))
def test_linear_res(gpu, route, m, n, k, switches, want, act, relu, with_r1):
    """act(a W^T + b) + res0 (+ ReLU on it) + res1, all added in fp32 before the one rounding."""
    a, wp, b, pre = lin_dev(gpu, m, n, k)
    g = X.gen("res", m, n, k)
    r0, r1 = X.resid16(g, (m, n)), X.resid16(g, (m, n))
    ref = X.act64(pre, act) + (r0.double().relu() if relu else r0.double())
    if with_r1:
        ref = ref + r1.double()
    ws = workspace(gpu) if route == "split_store" else None
    out = torch.full((m, n), NAN, dtype=torch.float16, device=gpu)
    sl = C.c_int(0)
    with _lib.tuning(**switches):
        op("mde_op_linear_res", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), act, ptr(r0.to(gpu)), 0, relu,
           ptr(r1.to(gpu) if with_r1 else None), ptr(out), n, ptr(ws), ws.numel() if ws is not None else 0,
           C.byref(sl), None, 0, 0, stream())
    assert_route(want, route)
    assert (sl.value > 1) == (route == "split_store"), sl.value
    assert_equal(out, to16(ref), f"linear_res {route} {m}x{n}x{k} act {act} relu {relu} res1 {with_r1}")


@pytest.mark.parametrize("f16", [0, 1], ids=["x32", "xh"])
@pytest.mark.parametrize("route,m,n,k,switches,want", X.RESID_SPLIT_ROUTES, ids=IDS(X.RESID_SPLIT_ROUTES))
def test_linear_residual_split(gpu, route, m, n, k, switches, want, f16):
    """E_RESID split-K (splitk = 4): the slices' partial sums and their sum
    in slice order are exact, so the split equals float64 like the unsplit."""
    a, wp, b, _ = lin_dev(gpu, m, n, k)
    ls, x, ref = resid_operands(gpu, m, n, k, f16)
    ws = workspace(gpu, 4 * m * n)
    cnt = torch.zeros(1024, dtype=torch.int32, device=gpu)
    part = torch.full((n // 32, m, 2), NAN, device=gpu) if f16 else None
    with _lib.tuning(**switches):
        op("mde_op_linear_residual_split", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), ptr(ls),
           ptr(None if f16 else x), ptr(x if f16 else None), n, ptr(part), 4, ptr(ws), ws.numel(), ptr(cnt),
           cnt.numel(), ws.numel(), stream())
    r = assert_route(want, route)
    assert r["slices"] > 1, r
    assert_equal(x, to16(ref) if f16 else ref.float(), f"linear_residual_split {route} {'xh' if f16 else 'x32'}")
    if f16:
        close(part, ln_partials_ref(x.cpu()).float(), 1e-5, 1e-3, f"{route} ln partials")


def pad_w32(w, n_mult=128, k_mult=32):
    n, k = w.shape
    out = torch.zeros(-(-n // n_mult) * n_mult, -(-k // k_mult) * k_mult, dtype=torch.float32)
    out[:n, :k] = w
    return out


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("m,n,k", X.LINEAR32_SHAPES)
def test_linear32(gpu, m, n, k, act):
    """fp32 operands on the same grid: exact in fp32."""
    a, w, b, acc = X.lin_case(m, n, k)
    wp = pad_w32(w.float()).to(gpu)
    out = torch.full((m, n), NAN, device=gpu)
    op("mde_op_linear32", ptr(a.float().to(gpu)), k, ptr(wp), wp.shape[1], m, n, k, ptr(b.float().to(gpu)), act,
       ptr(out), n, stream())
    assert_equal(out, X.act64(acc + b, act).float(), f"linear32 {m}x{n}x{k} act {act}")


@pytest.mark.parametrize("m,n,k", X.LINEAR32_SHAPES)
def test_linear_residual32(gpu, m, n, k):
    a, w, b, acc = X.lin_case(m, n, k)
    ls, x, ref = resid_operands(gpu, m, n, k, 0)
    wp = pad_w32(w.float()).to(gpu)
    op("mde_op_linear_residual32", ptr(a.float().to(gpu)), k, ptr(wp), wp.shape[1], m, n, k, ptr(b.float().to(gpu)),
       ptr(ls), ptr(x), n, stream())
    assert_equal(x, ref.float(), f"linear_residual32 {m}x{n}x{k}")


QKV_WANT = {(2, 50, 6): dict(kind="tile", bm=64, bn=64), (3, 1371, 6): dict(kind="tile", bm=128, bn=128, bk=32),
            (100, 37, 6): dict(kind="tile", bm=128, bn=128, bk=32)}


@pytest.mark.parametrize("B,T,H", X.QKV_SHAPES)
def test_qkv(gpu, B, T, H):
    """q (x 0.125: exact), k and the key-permuted V^T by equality; the pad stays zero."""
    D = 64 * H
    Tp = -(-T // 64) * 64
    a, wp, b, pre = lin_dev(gpu, B * T, 3 * D, D)
    full = pre.reshape(B, T, 3, H, 64)
    q = torch.zeros(B * H, Tp, 64, dtype=torch.float16, device=gpu)
    k = torch.zeros_like(q)
    vt = torch.zeros(B * H, 64, Tp, dtype=torch.float16, device=gpu)
    op("mde_op_qkv", ptr(a), ptr(wp), wp.shape[1], ptr(b), B, T, H, Tp, 0.125, ptr(q), ptr(k), ptr(vt), stream())
    assert_route(QKV_WANT[(B, T, H)], f"qkv {B}x{T}x{H}")
    rq = to16(full[:, :, 0].permute(0, 2, 1, 3).reshape(B * H, T, 64) * 0.125)
    rk = to16(full[:, :, 1].permute(0, 2, 1, 3).reshape(B * H, T, 64))
    rv = to16(full[:, :, 2].permute(0, 2, 3, 1).reshape(B * H, 64, T))
    assert_equal(q[:, :T], rq, "q")
    assert_equal(k[:, :T], rk, "k")
    perm = vt_perm(T).to(gpu)
    assert_equal(vt[:, :, perm], rv, "vt (key-permuted storage)")
    pad = torch.ones(Tp, dtype=torch.bool, device=gpu)
    pad[perm] = False
    assert float(q[:, T:].abs().max()) == 0 and float(k[:, T:].abs().max()) == 0, "q / k pad must stay zero"
    assert float(vt[:, :, pad].abs().max()) == 0, "vt pad must stay zero"


def test_patch_embed(gpu):
    B, Hh, Ww, D = 2, 98, 98, 384
    img, w, b, pos, cls_pos, x64 = X.patch_case(B, Hh, Ww)
    ph, pw = Hh // 14, Ww // 14
    w16 = torch.zeros(D, 3, 14, 16)
    w16[..., :14] = w.float()
    wp = pad_w(w16.reshape(D, 672)).to(gpu)
    scratch = torch.full((B * ph * pw, 672), NAN, dtype=torch.float16, device=gpu)
    x = torch.full((B * (ph * pw + 1), D), NAN, device=gpu)
    op("mde_op_patch_embed", ptr(img.float().to(gpu)), B, Hh, Ww, ptr(wp), wp.shape[1], ptr(b.float().to(gpu)),
       ptr(pos.float().to(gpu)), ptr(cls_pos.float().to(gpu)), D, ptr(scratch), ptr(x), stream())
    assert_route(dict(kind="tile", bm=64, bn=64), "patch_embed")
    assert_equal(x, x64.float(), "patch_embed")


CONV_IDS = [f"{c[0]}x{c[1]}x{c[2]}_{c[3]}to{c[4]}_s{c[5]}_r{c[6]}a{c[7]}n{c[8]}"
            + "".join(f"_{k}{v}" for k, v in c[10].items()) for c in X.CONV_CASES]


@pytest.mark.parametrize("B,h,w,cin,cout,stride,relu_in,act,nres,with_ws,switches,kind", X.CONV_CASES, ids=CONV_IDS)
def test_conv3x3(gpu, B, h, w, cin, cout, stride, relu_in, act, nres, with_ws, switches, kind):
    geo = (B, h, w, cin, cout, stride, relu_in)
    x, wt, b, _ = X.conv_case(*geo)
    ref, res = X.conv_ref(geo, act, nres)
    wp = conv_w(wt.float()).to(gpu)
    ho, wo = ref.shape[2], ref.shape[3]
    rg = [nhwc(r).to(gpu) for r in res] + [None, None]
    out = torch.full((B, ho, wo, cout), NAN, dtype=torch.float16, device=gpu)
    xg, bg = nhwc(x).half().to(gpu), b.float().to(gpu)
    with _lib.tuning(**switches):
        if with_ws:
            ws = workspace(gpu)
            sl = C.c_int(0)
            op("mde_op_conv3x3_ws", ptr(xg), B, h, w, cin, ptr(wp), wp.shape[1], cout, stride, relu_in, ptr(bg), act,
               ptr(rg[0]), ptr(rg[1]), ptr(out), ptr(ws), ws.numel(), C.byref(sl), stream())
            assert (sl.value > 1) == (kind == "split_store"), sl.value
        else:
            op("mde_op_conv3x3", ptr(xg), B, h, w, cin, ptr(wp), wp.shape[1], cout, stride, relu_in, ptr(bg), act,
               ptr(rg[0]), ptr(rg[1]), ptr(out), stream())
    assert_route(dict(kind=kind, bm=64, bn=64) if kind != "conv_direct" else dict(kind=kind), str(geo))
    assert_equal(out, to16(nhwc(ref)), f"conv3x3 {geo} act {act} nres {nres} {switches}")


@pytest.mark.parametrize("s,cin,B,h,w", X.CONVT_CASES)
def test_conv_transpose(gpu, s, cin, B, h, w):
    x, wt, b, ref = X.convt_case(s, cin, B, h, w)
    wp = pad_w(wt.float().permute(2, 3, 1, 0).reshape(s * s * cin, cin)).to(gpu)
    out = torch.full((B, h * s, w * s, cin), NAN, dtype=torch.float16, device=gpu)
    op("mde_op_conv_transpose", ptr(nhwc(x).half().to(gpu)), B, h, w, cin, ptr(wp), wp.shape[1], cin, s,
       ptr(b.float().to(gpu)), ptr(out), stream())
    assert_route(dict(kind="tile", bm=64, bn=64), f"convT s{s}")
    assert_equal(out, to16(nhwc(ref)), f"convT s{s} cin {cin}")


@pytest.mark.parametrize("B,h,w,cin,cout,stride,relu_in,act,nres", X.CONV32_CASES)
def test_conv3x3_32(gpu, B, h, w, cin, cout, stride, relu_in, act, nres):
    geo = (B, h, w, cin, cout, stride, relu_in)
    x, wt, b, _ = X.conv_case(*geo)
    ref, res = X.conv_ref(geo, act, nres)
    wp = pad_w32(wt.float().permute(0, 2, 3, 1).reshape(cout, 9 * cin)).to(gpu)
    rg = [nhwc(r).float().to(gpu) for r in res] + [None, None]
    out = torch.full((B, ref.shape[2], ref.shape[3], cout), NAN, device=gpu)
    op("mde_op_conv3x3_32", ptr(nhwc(x).float().to(gpu)), B, h, w, cin, ptr(wp), wp.shape[1], cout, stride, relu_in,
       ptr(b.float().to(gpu)), act, ptr(rg[0]), ptr(rg[1]), ptr(out), stream())
    assert_equal(out, nhwc(ref).float(), f"conv3x3_32 {geo} act {act} nres {nres}")


@pytest.mark.parametrize("s,cin,B,h,w", X.CONVT_CASES)
def test_conv_transpose32(gpu, s, cin, B, h, w):
    x, wt, b, ref = X.convt_case(s, cin, B, h, w)
    wp = pad_w32(wt.float().permute(2, 3, 1, 0).reshape(s * s * cin, cin)).to(gpu)
    out = torch.full((B, h * s, w * s, cin), NAN, device=gpu)
    op("mde_op_conv_transpose32", ptr(nhwc(x).float().to(gpu)), B, h, w, cin, ptr(wp), wp.shape[1], cin, s,
       ptr(b.float().to(gpu)), ptr(out), stream())
    assert_equal(out, nhwc(ref).float(), f"convT32 s{s} cin {cin}")


# ---- 2. GELU: every finite f16 input through every epilogue that has one --------

def check_gelu(out, x, what):
    """|out - gelu64(x)| <= 0.5 ulp16 + 2.6e-5 + 2^-20 |ref| per element;
    prints the largest err - 0.5 ulp and where."""
    ref = X.gelu64(x)
    err = (out.cpu().double() - ref).abs()
    over = (err - 0.5 * X.ulp16(ref)).flatten()
    i = int(over.nan_to_num(float("inf")).argmax())
    print(f"GELU {what}: max(err - 0.5 ulp) {float(over[i]):.3e} at x = {float(x.flatten()[i])!r}")
    bad = ~(err <= X.gelu_bound(ref))
    assert not bool(bad.any()), (f"GELU {what}: {int(bad.sum())} outputs beyond 0.5 ulp + 2.6e-5 + 2^-20 |ref|, "
                                 f"worst err - 0.5 ulp {float(over[i]):.3e} at x = {float(x.flatten()[i])!r}")


def run_sweep(gpu, m, n, k, switches, use_ws=False):
    a, w, b = X.sweep_operands(m, n, k)
    wp = pad_w(w.float()).to(gpu)
    out = torch.full((m, n), NAN, dtype=torch.float16, device=gpu)
    with _lib.tuning(**switches):
        if use_ws:
            ws = workspace(gpu)
            sl = C.c_int(0)
            op("mde_op_linear_ws", ptr(a.to(gpu)), k, ptr(wp), wp.shape[1], m, n, k, ptr(b.to(gpu)), 2, ptr(out), n,
               ptr(ws), ws.numel(), C.byref(sl), stream())
            assert sl.value > 1
        else:
            op("mde_op_linear", ptr(a.to(gpu)), k, ptr(wp), wp.shape[1], m, n, k, ptr(b.to(gpu)), 2, ptr(out), n,
               stream())
    return out.cpu()


@pytest.fixture(scope="module")
def gelu_table(gpu):
    """GELU(fl32(a + b)) of every (finite f16 a, bias class) pair from the
    64^2-tile site (store_tile_lds / store_tile of gemm.hip's 64 x 64 kernel):
    [NSEQ][8] f16, the table every other site must reproduce."""
    m, n, k = X.GELU_TABLE_SHAPE
    out = run_sweep(gpu, m, n, k, {})
    assert_route(dict(kind="tile", bm=64, bn=64), "GELU table")
    idx, cls = X.sweep_index(m, n, k)
    tbl = torch.full((X.NSEQ, 8), NAN, dtype=torch.float16)
    tbl[idx, cls[None, :].expand_as(idx)] = out
    assert not bool(torch.isnan(tbl).any())
    return tbl


def test_gelu_tile64(gelu_table):
    idx = torch.arange(X.NSEQ)[:, None].expand(-1, 8)
    cls = torch.arange(8)[None, :].expand(X.NSEQ, -1)
    check_gelu(gelu_table, X.sweep_x(idx, cls), "64^2 tiles")


@pytest.mark.parametrize("site,m,n,k,switches,want", X.GELU_SITES, ids=IDS(X.GELU_SITES))
def test_gelu_site(gpu, gelu_table, site, m, n, k, switches, want):
    out = run_sweep(gpu, m, n, k, switches, use_ws=site == "split_store")
    assert_route(want, site)
    idx, cls = X.sweep_index(m, n, k)
    cls = cls[None, :].expand_as(idx)
    check_gelu(out, X.sweep_x(idx, cls), site)
    assert_equal(out, gelu_table[idx, cls], f"GELU {site} vs the 64^2-tile site")


def test_gelu_conv(gpu, gelu_table):
    """mde_op_conv3x3 with a centre-tap identity kernel, 64 -> 64 on a 31 x 32
    map (63488 inputs): conv3_kernel's epilogue (tile_epilogue.h)."""
    B, h, w, c = X.GELU_CONV
    x = X.finite_f16().reshape(B, h, w, c)
    wt = torch.zeros(c, c, 3, 3)
    wt[torch.arange(c), torch.arange(c), 1, 1] = 1.0
    wp = conv_w(wt).to(gpu)
    cls = torch.arange(c) % 8
    out = torch.full((B, h, w, c), NAN, dtype=torch.float16, device=gpu)
    op("mde_op_conv3x3", ptr(x.to(gpu)), B, h, w, c, ptr(wp), wp.shape[1], c, 1, 0,
       ptr(X.GELU_BIAS[cls].float().to(gpu)), 2, None, None, ptr(out), stream())
    assert_route(dict(kind="conv_direct", conv="conv3"), "GELU conv")
    idx = torch.arange(X.NSEQ).reshape(-1, c)
    cls = cls[None, :].expand_as(idx)
    check_gelu(out.cpu().reshape(-1, c), X.sweep_x(idx, cls), "conv3x3")
    assert_equal(out.reshape(-1, c), gelu_table[idx, cls], "GELU conv3x3 vs the 64^2-tile site")


@pytest.mark.parametrize("upconv", [1, 0])
def test_gelu_upconv(gpu, gelu_table, upconv):
    """The one scalar gelu_erf call (conv.hip upconv_kernel; with "upconv" = 0
    conv3_kernel's tile_epilogue.h site): mde_op_conv3x3_up at the source's own
    size -- align_corners scale exactly 1, every blend weight exactly 0, so the
    upsampled map is the map -- with a centre-tap identity kernel, 32 -> 32 on
    eight 8 x 31 maps.  upconv_kernel takes a map only when every 16-row tile
    reads at most 12 source rows (conv.hip upconv_eligible); at ratio 1 that
    is a map of at most 12 rows, and the route record says which kernel ran.
    The values ascend by bit pattern and one image holds 7936
    of them, so images 0..3 are the non-negative and 4..7 the negative
    values: a pixel's right and lower neighbours (the b of a + (b - a) w)
    have its sign, and b - a cannot overflow f16."""
    B, h, w, c = X.GELU_UPCONV
    assert B * h * w * c == X.NSEQ and (X.NSEQ // 2) % (h * w * c) == 0
    x = X.finite_f16().reshape(B, h, w, c)
    wt = torch.zeros(c, c, 3, 3)
    wt[torch.arange(c), torch.arange(c), 1, 1] = 1.0
    wp = conv_w(wt).to(gpu)
    cls = torch.arange(c) % 8
    out = torch.full((B, h, w, c), NAN, dtype=torch.float16, device=gpu)
    with _lib.tuning(upconv=upconv):
        op("mde_op_conv3x3_up", ptr(x.to(gpu)), B, h, w, c, h, w, ptr(wp), wp.shape[1], c,
           ptr(X.GELU_BIAS[cls].float().to(gpu)), 2, ptr(out), stream())
    assert_route(dict(kind="conv_direct", conv="upconv" if upconv else "conv3_up"), "GELU upconv")
    idx = torch.arange(X.NSEQ).reshape(-1, c)
    cls = cls[None, :].expand_as(idx)
    check_gelu(out.cpu().reshape(-1, c), X.sweep_x(idx, cls), f"conv3x3_up (upconv {upconv})")
    assert_equal(out.reshape(-1, c), gelu_table[idx, cls], f"GELU conv3x3_up (upconv {upconv}) vs the 64^2-tile site")


# mde_op_linear32's GELU is 0.5 x (1 + erff(x / sqrt 2)).  Measured on an MI355X over the sweep: the largest
# error relative to max(|ref|, 2^-14) is 1.331e-3, at x = -5.5398 (erff has reached -1 there: the output is 0
# where the value is -8.1e-8).  The bar is 4 x that and nowhere above test_linear32's 2e-5 + 2e-5 |ref|, which
# is the smaller of the two from |ref| = 3.8e-3 up.
ERFF_REL_MEASURED = 1.331e-3


def test_gelu_linear32(gpu):
    m, n, k = X.GELU32_SHAPE
    a, w, b = X.sweep_operands(m, n, k)
    wp = pad_w32(w.float()).to(gpu)
    out = torch.full((m, n), NAN, device=gpu)
    op("mde_op_linear32", ptr(a.float().to(gpu)), k, ptr(wp), wp.shape[1], m, n, k, ptr(b.to(gpu)), 2, ptr(out), n,
       stream())
    idx, cls = X.sweep_index(m, n, k)
    x = X.sweep_x(idx, cls[None, :].expand_as(idx))
    ref = X.gelu64(x)
    err = (out.cpu().double() - ref).abs()
    rel = (err / ref.abs().clamp(min=2.0 ** -14)).flatten()
    i = int(rel.nan_to_num(float("inf")).argmax())
    print(f"GELU linear32 (erff): max rel err {float(rel[i]):.3e} at x = {float(x.flatten()[i])!r}")
    bar = torch.minimum(4 * ERFF_REL_MEASURED * ref.abs().clamp(min=2.0 ** -14), 2e-5 + 2e-5 * ref.abs())
    bad = ~(err <= bar)
    assert not bool(bad.any()), f"{int(bad.sum())} outputs beyond the bar, max rel {float(rel[i]):.3e}"


# ---- 3. attention: selection and uniform probes on every launch shape ------------

LAUNCHES = X.ATTN_LAUNCHES


@functools.lru_cache(maxsize=None)
def selection(B, H, T, inverse):
    q, k, v, pis = X.selection_case(B, H, T, inverse)
    return q, k, v, X.selection_expected(v, pis, B, H, T)


@pytest.mark.parametrize("B,H,T", X.ATTN_SHAPES)
@pytest.mark.parametrize("launch,cfg,tail", LAUNCHES, ids=IDS(LAUNCHES))
def test_attention_selection(gpu, launch, cfg, tail, B, H, T):
    """Key pi(i) beats every other key of query i by 40 in log2 units: the
    other keys' P underflow to 0 in f16, the dominant P is a power of two and
    O / l = v (1 +- a few 2^-23) rounds back to v -- the output is v[pi],
    exactly.  The multiplicative permutation and its inverse: every key is
    selected from another tile and every query block reads every key tile."""
    for inverse in (0, 1):
        q, k, v, exp = selection(B, H, T, inverse)
        o = run_attention(gpu, launch, cfg, tail, q, k, v, B, H, T)
        assert_attn_route(X.attention_route_expected(cfg, tail, B, H, T), f"attention {launch} B{B} H{H} T{T}")
        assert_equal(o, exp, f"attention {launch} B{B} H{H} T{T} selection (inverse {inverse})")


@pytest.mark.parametrize("B,H,T", X.ATTN_SHAPES + [(1, 1, 1)])
@pytest.mark.parametrize("launch,cfg,tail", LAUNCHES, ids=IDS(LAUNCHES))
def test_attention_uniform(gpu, launch, cfg, tail, B, H, T):
    """q = 0: every real key weighs 1 / T and V's columns are constant, so the
    output is that constant; a leaked pad key (v = 0, the same score 0) scales
    the row by T / (T + 1) -- more than half an f16 ulp for every T here."""
    q, k, v, exp = X.uniform_case(B, H, T)
    o = run_attention(gpu, launch, cfg, tail, q, k, v, B, H, T)
    assert_attn_route(X.attention_route_expected(cfg, tail, B, H, T), f"attention {launch} B{B} H{H} T{T}")
    assert_equal(o, exp, f"attention {launch} B{B} H{H} T{T} uniform")


@pytest.mark.parametrize("B,H,T", X.ATTN_SHAPES)
def test_attention32_selection(gpu, B, H, T):
    """The same probe on fp32 tensors: relative error <= 2^-20.  fp32 keeps
    what f16 P drops -- the up to 11 keys one code bit away weigh 2^-40 each,
    about 1e-11 in all, which is more than 2^-20 |v| where |v[pi]| < 1e-5 --
    so the reference is the float64 softmax itself, not v[pi]."""
    Tp = -(-T // 64) * 64
    for inverse in (0, 1):
        q, k, v, _ = selection(B, H, T, inverse)
        ref = X.attention64(q, k, v).reshape(B, H, T, 64).permute(0, 2, 1, 3).reshape(B * T, H * 64)
        qg, kg, vg = (torch.zeros(B * H, Tp, 64, device=gpu) for _ in range(3))
        qg[:, :T], kg[:, :T], vg[:, :T] = q.float().to(gpu), k.float().to(gpu), v.float().to(gpu)
        o = torch.full((B * T, H * 64), NAN, device=gpu)
        op("mde_op_attention32", ptr(qg), ptr(kg), ptr(vg), ptr(o), B, H, T, Tp, H * 64, stream())
        err = (o.cpu().double() - ref).abs()
        rel = (err / ref.abs()).nan_to_num(0.0, posinf=float("inf"))
        print(f"attention32 B{B} H{H} T{T} (inverse {inverse}): max rel err {float(rel.max()):.3e}")
        bad = ~(err <= 2.0 ** -20 * ref.abs())
        assert not bool(bad.any()), (f"attention32 B{B} H{H} T{T} (inverse {inverse}): {int(bad.sum())} outputs, "
                                     f"max rel err {float(rel.max()):.3e}")
