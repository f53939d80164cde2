"""Op-level parity for the GemmParams options that only the engine graphs set
(csrc/mde_ops.h), through the ABI 11 wrappers mde_op_linear_res,
mde_op_conv3x3_res, mde_op_linear_lnfold_tok, mde_op_depth_head_pe,
mde_op_conv_transpose_ld and mde_op_linear_residual_split, plus row strides
(lda > K, ldo > N) on the existing ops.

Every kernel result is compared, element by element, with a float64 torch
reference over the f16-rounded operands, at the bars of the sibling test of the
same kernel in test_gpu_ops.py.  Where two routes run the same fp32 operations
in the same order (a table against its expansion, the fused split-K tail
against slices + reduce kernel, the resize folded into the conv epilogue
against a resize launch) the outputs are compared with torch.equal.

Guard bands: every output buffer has extra rows and, where ldo > N, extra
columns, pre-filled with a finite bit pattern; the cells a kernel must not
touch are compared as integers afterwards.

Inputs come from generators seeded by the problem's shape, so neither the
order of the tests nor test_gpu_ops.py's seeded sequence matters.
"""

import ctypes as C
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from gpu_util import close, conv_w, nhwc, op, pad_w, ptr, stream, vt_perm
from monocular_depth_estimation_trt_amd import _lib

pytestmark = pytest.mark.gpu

PAT16, PAT32 = 0x5A5A, 0x4B5A5A5A  # finite as f16 (203.25) and as f32 (1.43e7)
EXTRA = 3                          # guard rows behind every output
NAN = float("nan")
LOG2E = 1.4426950408889634


def gen(*key):
    """A generator of this file's own, seeded by the problem."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def guarded(rows, cols, dtype, dev):
    """[rows + EXTRA][cols] device buffer filled with the guard pattern."""
    t = torch.empty(rows + EXTRA, cols, dtype=dtype, device=dev)
    bits(t).fill_(PAT16 if dtype == torch.float16 else PAT32)
    return t


def assert_guard(buf, rows, c0, c1, what):
    """Only buf[:rows, c0:c1] may have been written."""
    b = bits(buf.reshape(buf.shape[0], -1))
    pat = PAT16 if buf.dtype == torch.float16 else PAT32
    assert bool((b[rows:] == pat).all()), f"{what}: rows >= {rows} written"
    assert bool((b[:rows, :c0] == pat).all()), f"{what}: columns < {c0} written"
    assert bool((b[:rows, c1:] == pat).all()), f"{what}: columns >= {c1} written"


def written(buf):
    """Number of elements of a guard-filled buffer that no longer hold the pattern."""
    return int((bits(buf) != (PAT16 if buf.dtype == torch.float16 else PAT32)).sum())


def act64(x, act):
    return F.relu(x) if act == 1 else (F.gelu(x) if act == 2 else x)


def counters(dev, n=1024):
    return torch.zeros(n, dtype=torch.int32, device=dev)


def ln_partials_ref(xh):
    """(sum, squared deviations from the slice mean) per 32-column slice and
    row of f16 rows, fp64, slice-major [k/32][m][2] (GemmParams::lnst_*)."""
    v = xh.double().reshape(xh.shape[0], -1, 32)
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([v.sum(-1), m2], -1).transpose(0, 1).contiguous()


# ---- (a) row strides on the existing ops --------------------------------------

@functools.lru_cache(maxsize=4)
def lin_problem(m, n, k):
    """a16 [m][k], w16 [n][k] (f16), bias, and a16 w16^T + bias in float64."""
    g = gen("lin", m, n, k)
    a16, w16, b = rn(g, m, k).half(), rn(g, n, k, scale=k ** -0.5).half(), rn(g, n, scale=0.1)
    return a16, w16, b, a16.double() @ w16.double().T + b.double()


def strided_a(a16, gap, dev):
    """A with lda = K + gap, the gap columns NaN."""
    m, k = a16.shape
    a = torch.full((m, k + gap), NAN, dtype=torch.float16)
    a[:, :k] = a16
    return a.to(dev)


@pytest.mark.parametrize("route,m,n,k,act,switches", [
    ("64^2 tiles", 77, 96, 40, 1, {}),
    ("128^2 tiles, BK 32", 2035, 1920, 72, 2, {}),
    ("128^2 tiles, 8 waves", 2035, 1920, 1032, 0, {"w8small": 1}),
    ("128^2 tiles, 4 waves", 2035, 1920, 1032, 0, {"w8small": 0}),
    ("gemm256", 300, 264, 72, 2, {"gemm256": 2}),
    ("panel kernel", 16129, 64, 384, 1, {}),
], ids=["t64", "t128_bk32", "t128_w8", "t128_w4", "gemm256", "panel"])
def test_linear_strided(gpu, route, m, n, k, act, switches):
    """lda > K and ldo > N on mde_op_linear (lda = K + 8 with NaN in the gap,
    ldo = N + 8), one case per route of launch_gemm: the 64^2 tiles (K = 40: a
    K tail), the 128^2 tiles at BK 32 (16 x 15 = 240 = kBigTileMin tiles), the
    128^2 tiles on 8 and on 4 waves (switch "w8small", K = 1032: a K tail of
    8), gemm256 ("gemm256" = 2) and the panel kernel at the smallest N (64) and
    M (63 panels of 256 rows + 1) panel_gemm_eligible accepts.  The NaN gap
    must not reach any output; the ldo gap and the rows past M stay as they
    were."""
    a16, w16, b, base = lin_problem(m, n, k)
    wp = pad_w(w16.float()).to(gpu)
    out = guarded(m, n + 8, torch.float16, gpu)
    with _lib.tuning(**switches):
        op("mde_op_linear", ptr(strided_a(a16, 8, gpu)), k + 8, ptr(wp), wp.shape[1], m, n, k, ptr(b.to(gpu)), act,
           ptr(out), n + 8, stream())
    r = _lib.last_gemm_route()
    want = {"64^2 tiles": dict(kind="tile", bm=64, bn=64),
            "128^2 tiles, BK 32": dict(kind="tile", bm=128, bn=128, wm=2, wn=2, bk=32),
            "128^2 tiles, 8 waves": dict(kind="tile", bm=128, bn=128, wm=2, wn=4, bk=64),
            "128^2 tiles, 4 waves": dict(kind="tile", bm=128, bn=128, wm=2, wn=2, bk=64),
            "gemm256": dict(kind="gemm256"), "panel kernel": dict(kind="panel")}[route]
    assert {f: r.get(f) for f in want} == want, (route, r)
    close(out[:m, :n], act64(base, act), 1e-2, 1e-2, f"linear {route} {m}x{n}x{k}")
    assert_guard(out, m, 0, n, f"linear {route}")


@pytest.mark.parametrize("m,n,k,act", [(300, 1152, 384, 0), (2035, 1920, 384, 2)])
def test_linear_lnfold_strided(gpu, m, n, k, act):
    """ldo > N on mde_op_linear_lnfold (ldo = N + 8): the 64^2 tiles (90 of
    them) and the 128^2 BK 32 tiles (240) with the LayerNorm fold in front of
    the LDS-staged epilogue, against test_linear_lnfold's reference order."""
    g = gen("lnfold", m, n, k)
    x = (rn(g, m, k) * 2 + 0.7).half()
    gm, bt = 1 + 0.2 * rn(g, k), 0.05 * rn(g, k)
    w, b = rn(g, n, k, scale=k ** -0.5), rn(g, n, scale=0.1)
    ln = F.layer_norm(x.double(), (k,), gm.double(), bt.double(), 1e-6).half().double()
    ref = act64(ln @ w.half().double().T + b.double(), act)
    wg = (w.double() * gm.double()[None, :]).float()
    c1 = wg.half().double().sum(1).float()
    c2 = (b.double() + w.half().double() @ bt.double()).float()
    wgp = pad_w(wg).to(gpu)
    out = guarded(m, n + 8, torch.float16, gpu)
    op("mde_op_linear_lnfold", ptr(x.to(gpu)), ptr(ln_partials_ref(x).float().to(gpu)), 1e-6, ptr(wgp), wgp.shape[1],
       ptr(c1.to(gpu)), ptr(c2.to(gpu)), m, n, k, act, ptr(out), n + 8, stream())
    r = _lib.last_gemm_route()
    assert (r["kind"], r["bm"], r["bn"], r["bk"]) == (("tile", 64, 64, 64) if m == 300 else ("tile", 128, 128, 32)), r
    close(out[:m, :n], ref, 1e-2, 1.5e-2, f"linear_lnfold ldo {m}x{n}x{k}")
    assert_guard(out, m, 0, n, "linear_lnfold")


@pytest.mark.parametrize("B,H,T", [(2, 6, 50), (3, 1, 65), (1, 2, 300)])
def test_attention_strided(gpu, B, H, T):
    """ldo > N on mde_op_attention (ldo = 64 H + 8): partial last query blocks
    (T = 50, 65, 300), against test_attention's reference at its bar."""
    g = gen("attn", B, H, T)
    Tp = -(-T // 64) * 64
    q = (rn(g, B * H, T, 64) * 0.125 * 2.0 * LOG2E).half()
    k = (rn(g, B * H, T, 64) * 2.0).half()
    v = rn(g, B * H, T, 64).half()
    ref = torch.softmax((q.double() @ k.double().transpose(1, 2)) / LOG2E, dim=-1) @ v.double()
    ref = ref.reshape(B, H, T, 64).permute(0, 2, 1, 3).reshape(B * T, H * 64)
    qg = torch.zeros(B * H, Tp, 64, dtype=torch.float16, device=gpu)
    kg = torch.zeros_like(qg)
    vtg = torch.zeros(B * H, 64, Tp, dtype=torch.float16, device=gpu)
    qg[:, :T], kg[:, :T] = q.to(gpu), k.to(gpu)
    vtg[:, :, vt_perm(T).to(gpu)] = v.transpose(1, 2).to(gpu)
    ldo = H * 64 + 8
    o = guarded(B * T, ldo, torch.float16, gpu)
    op("mde_op_attention", ptr(qg), ptr(kg), ptr(vtg), ptr(o), B, H, T, Tp, ldo, stream())
    close(o[:B * T, :H * 64], ref, 2e-2, 5e-3, f"attention ldo B{B} H{H} T{T}")
    assert_guard(o, B * T, 0, H * 64, "attention")


# ---- (b) dense E_STORE residual options ----------------------------------------

ROWS = 37  # res0_rows: neither M below is a tile multiple, so the table row wraps inside tiles


def linear_res(gpu, p, act, res0, res0_rows, res0_relu, res1, ldo, ws=None, cnt=None, slot=0):
    """One mde_op_linear_res call on problem p into a fresh guarded buffer -> (out, slices)."""
    a, wp, b, m, n, k = p
    out = guarded(m, ldo, torch.float16, gpu)
    sl = C.c_int(0)
    op("mde_op_linear_res", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), act, ptr(res0), res0_rows, res0_relu,
       ptr(res1), ptr(out), ldo, ptr(ws), ws.numel() if ws is not None else 0, C.byref(sl), ptr(cnt),
       cnt.numel() if cnt is not None else 0, slot, stream())
    return out, sl.value


def res_operands(m, n, k, ldo, gpu):
    a16, w16, b, base = lin_problem(m, n, k)
    g = gen("res", m, n, k, ldo)
    tab, full, r1 = rn(g, ROWS, ldo).half(), rn(g, m, ldo).half(), rn(g, m, ldo).half()  # mixed sign
    p = (a16.to(gpu), pad_w(w16.float()).to(gpu), b.to(gpu), m, n, k)
    return p, base, tab, full, r1


def check_linear_res(gpu, m, n, k, gap, combos, act=2, ws=None):
    """Runs every (res0_relu, table, res1) combination; with ws also under
    "splitk_fused" 0 and 1."""
    ldo = n + gap
    p, base, tab, full, r1 = res_operands(m, n, k, ldo, gpu)
    idx = torch.arange(m) % ROWS
    tg, fg, rg = tab.to(gpu), full.to(gpu), r1.to(gpu)
    exp = tab[idx].contiguous().to(gpu)  # the table expanded to [M][ldo]
    for relu, table, with_r1 in combos:
        what = f"linear_res {m}x{n}x{k} ldo {ldo} relu {relu} table {table} res1 {with_r1}"
        r0 = (tab[idx] if table else full)[:, :n].double()
        ref = act64(base, act) + (F.relu(r0) if relu else r0)
        if with_r1:
            ref = ref + r1[:, :n].double()
        res0, rows, res1 = (tg if table else fg), (ROWS if table else 0), (rg if with_r1 else None)
        if ws is None:
            out, _ = linear_res(gpu, p, act, res0, rows, relu, res1, ldo)
            again, _ = linear_res(gpu, p, act, res0, rows, relu, res1, ldo)
        else:
            outs = []
            for fused in (0, 1):
                cnt = counters(gpu)
                bits(ws).fill_(PAT32)
                with _lib.tuning(splitk_fused=fused):
                    o, S = linear_res(gpu, p, act, res0, rows, relu, res1, ldo, ws, cnt, ws.numel())
                    o2, _ = linear_res(gpu, p, act, res0, rows, relu, res1, ldo, ws, cnt, ws.numel())
                assert S > 1, f"{what}: expected a split, got {S} slices"
                r = _lib.last_gemm_route()
                assert (r["kind"], r["slices"], r["fused"]) == ("split_store", S, fused), (what, r)
                # the two-kernel form leaves S planes of M x N partial sums in ws, the fused form S slots of
                # 64 x 64 per tile: which of the two ran
                tiles = -(-m // 64) * -(-n // 64)
                assert written(ws) == (S * tiles * 4096 if fused else S * m * n), (what, fused, written(ws))
                assert int(cnt.abs().max()) == 0, f"{what}: counters not left zero"
                assert torch.equal(o, o2), f"{what}: fused {fused} second call differs"
                outs.append(o)
            out, again = outs
            assert torch.equal(outs[0], outs[1]), f"{what}: fused split differs from slices + reduce kernel"
        close(out[:m, :n], ref, 1e-2, 1e-2, what)
        assert_guard(out, m, 0, n, what)
        assert torch.equal(out, again), f"{what}: second call differs"
        if table:  # the same kernel and the same arithmetic on the expanded table
            if ws is None:
                full_out, _ = linear_res(gpu, p, act, exp, 0, relu, res1, ldo)
            else:
                full_out, _ = linear_res(gpu, p, act, exp, 0, relu, res1, ldo, ws, counters(gpu), ws.numel())
            assert torch.equal(out, full_out), f"{what}: table differs from its expansion"


ALL8 = [(relu, table, r1) for relu in (0, 1) for table in (1, 0) for r1 in (1, 0)]


@pytest.mark.parametrize("gap", [0, 8])
@pytest.mark.parametrize("n", [32, 48, 96])
def test_linear_res_small(gpu, n, gap):
    """res0_rows (VGGT's positional-embedding table, row m % 37) and res0_relu
    on the dense E_STORE epilogues at M = 185 = 5 x 37: the N <= 32 tile (128
    x 32), the N <= 64 tile and the 64^2 tiles of N = 96 (store_tile_lds, GELU
    before the adds), with ldo == N and ldo = N + 8 (ldo is the stride of the
    output and of the table).  All 8 combinations of res0_relu x (table |
    full-shape res0) x (res1 | none): against float64, the table bit-identical
    to its expansion, a second call bit-identical, guard bands."""
    check_linear_res(gpu, 185, n, 72, gap, ALL8)


@pytest.mark.parametrize("gap", [0, 8])
@pytest.mark.parametrize("n,switches", [(32, {}), (48, {}), (96, {}), (1920, {}), (264, {"gemm256": 2})],
                         ids=["n32", "n48", "n96", "n1920_t128", "n264_gemm256"])
def test_linear_res_large(gpu, n, switches, gap):
    """res0_rows and res0_relu at M = 2035 = 55 x 37 (many row tiles, the table
    wrapping inside each): the 128 x 32 and 64^2 tiles, the 128^2 BK 32 tiles
    (N = 1920: 240 tiles) and gemm256's LDS-staged epilogue ("gemm256" = 2, N =
    264), ldo == N and N + 8."""
    with _lib.tuning(**switches):
        check_linear_res(gpu, 2035, n, 72, gap, [(1, 1, 1), (0, 1, 0), (1, 0, 1)])


@pytest.mark.parametrize("gap", [0, 8])
def test_linear_res_split_store(gpu, gap):
    """res0_rows / res0_relu / res1 through the E_STORE split-K of a small grid
    (185 x 96 x 768: 6 tiles, 3 slices): splitk_store_kernel and, with switch
    "splitk_fused" = 1 and counters (GemmParams::tile_cnt), the fused tail in
    gemm.hip feeding store_tile_lds.  Fused and two-kernel outputs bit for bit,
    counters left zero, repeatable, table == expansion."""
    ws = torch.empty(1 << 18, dtype=torch.float32, device=gpu)
    check_linear_res(gpu, 185, 96, 768, gap, [(1, 1, 1), (0, 1, 0), (1, 0, 0)], act=1, ws=ws)


# ---- (c) a_tok: the cls-row skip of the DPT projects ---------------------------

@pytest.mark.parametrize("seqs,tokens,n,k", [(7, 38, 48, 384), (7, 38, 96, 384), (5, 50, 200, 1024),
                                             (101, 38, 1024, 384)])
def test_linear_lnfold_tok(gpu, seqs, tokens, n, k):
    """a_tok (mde_op_linear_lnfold_tok): GEMM row r reads A row and LN-partial
    row (r / (tokens - 1)) * tokens + 1 + r % (tokens - 1) -- gemm.hip's A
    loader and ln_partial_loads.  64^2 tiles at N = 48 and 96, K = 1024 with
    lnst_ns at its limit of 32, and 3737 rows on 30 x 8 = 240 tiles of 128^2
    with sequence boundaries inside tiles.  Every cls row of x and of the
    partials is NaN: the output must be finite, meet test_linear_lnfold's
    reference with the cls rows dropped, and equal mde_op_linear_lnfold on the
    gathered rows bit for bit (same M, N, K: the same kernel)."""
    g = gen("tok", seqs, tokens, n, k)
    rows, m = seqs * tokens, seqs * (tokens - 1)
    x = (rn(g, rows, k) * 2 + 0.7).half()
    gm, bt = 1 + 0.2 * rn(g, k), 0.05 * rn(g, k)
    w, b = rn(g, n, k, scale=k ** -0.5), rn(g, n, scale=0.1)
    keep = (torch.arange(rows) % tokens) != 0
    xs = x[keep]
    ref = F.layer_norm(xs.double(), (k,), gm.double(), bt.double(), 1e-6).half().double() @ w.half().double().T
    ref = act64(ref + b.double(), 2)
    wg = (w.double() * gm.double()[None, :]).float()
    c1 = wg.half().double().sum(1).float().to(gpu)
    c2 = (b.double() + w.half().double() @ bt.double()).float().to(gpu)
    wgp = pad_w(wg).to(gpu)
    part = ln_partials_ref(x).float()
    part_s = part[:, keep].contiguous()
    x[~keep] = NAN
    part[:, ~keep] = NAN
    out = guarded(m, n, torch.float16, gpu)
    op("mde_op_linear_lnfold_tok", ptr(x.to(gpu)), ptr(part.to(gpu)), 1e-6, ptr(wgp), wgp.shape[1], ptr(c1), ptr(c2),
       seqs, tokens, n, k, 2, ptr(out), n, stream())
    assert bool(torch.isfinite(out[:m]).all()), "a cls row reached the output"
    close(out[:m], ref, 1e-2, 1.5e-2, f"linear_lnfold_tok {seqs}x{tokens} n{n} k{k}")
    assert_guard(out, m, 0, n, "linear_lnfold_tok")
    gathered = guarded(m, n, torch.float16, gpu)
    op("mde_op_linear_lnfold", ptr(xs.to(gpu)), ptr(part_s.to(gpu)), 1e-6, ptr(wgp), wgp.shape[1], ptr(c1), ptr(c2), m,
       n, k, 2, ptr(gathered), n, stream())
    assert torch.equal(out, gathered), "a_tok differs from the same GEMM over the gathered rows"


# ---- (d) conv E_STORE residual options -----------------------------------------

@functools.lru_cache(maxsize=2)
def conv_problem(B, h, w, cin, cout, stride):
    """x16 NHWC, packed weights, bias and the float64 conv as [M][cout] rows."""
    g = gen("conv", B, h, w, cin, cout, stride)
    x16 = rn(g, B, cin, h, w).half()
    wt, b = rn(g, cout, cin, 3, 3, scale=(9 * cin) ** -0.5), rn(g, cout, scale=0.02)
    ref = F.conv2d(x16.double(), wt.half().double(), b.double(), stride=stride, padding=1)
    oh, ow = ref.shape[2], ref.shape[3]
    return nhwc(x16), conv_w(wt), b, ref.permute(0, 2, 3, 1).reshape(-1, cout), oh, ow


def conv_res(gpu, geo, x, wp, b, res0, relu, res1, up, out, ws=None, cnt=None):
    B, h, w, cin, cout, stride = geo
    sl = C.c_int(0)
    up_t, uh, uw = up if up is not None else (None, 0, 0)
    op("mde_op_conv3x3_res", ptr(x), B, h, w, cin, ptr(wp), wp.shape[1], cout, stride, 0, ptr(b), 0, ptr(res0), relu,
       ptr(res1), ptr(up_t), uh, uw, ptr(out), ptr(ws), ws.numel() if ws is not None else 0, C.byref(sl), ptr(cnt),
       cnt.numel() if cnt is not None else 0, ws.numel() if ws is not None else 0, stream())
    return sl.value


@pytest.mark.parametrize("route,B,h,w,cin,cout,stride,nres,split", [
    ("direct", 2, 19, 19, 64, 64, 1, 2, False), ("im2col", 1, 19, 19, 256, 64, 1, 1, False),
    ("im2col_s2", 1, 37, 37, 64, 64, 2, 2, False), ("split", 1, 19, 19, 384, 64, 1, 2, True)])
def test_conv_res0_relu(gpu, route, B, h, w, cin, cout, stride, nres, split):
    """res0_relu (add relu(res0), res0 of mixed sign) on the conv routes: the
    direct conv's LDS-staged epilogue (conv.hip), the implicit-im2col GEMM at
    stride 1 and 2 (store_tile_lds) and the split-K of a 19^2 map with a
    workspace -- splitk_store_kernel and, under "splitk_fused" = 1, the fused
    tail, bit for bit, counters left zero."""
    geo = (B, h, w, cin, cout, stride)
    x, wp, b, base, oh, ow = conv_problem(*geo)
    m = B * oh * ow
    g = gen("conv_res", *geo)
    res = [rn(g, m, cout).half() for _ in range(nres)]
    ref = base + F.relu(res[0].double()) + (res[1].double() if nres > 1 else 0)
    xg, wg, bg = x.to(gpu), wp.to(gpu), b.to(gpu)
    rg = [r.to(gpu) for r in res] + [None]
    what = f"conv res0_relu {route}"
    if not split:
        out = guarded(m, cout, torch.float16, gpu)
        conv_res(gpu, geo, xg, wg, bg, rg[0], 1, rg[1], None, out)
        assert _lib.last_gemm_route()["kind"] == ("conv_direct" if route == "direct" else "tile"), _lib.last_gemm_route()
        outs = [out]
    else:
        ws = torch.empty(1 << 20, dtype=torch.float32, device=gpu)
        outs = []
        for fused in (0, 1):
            cnt = counters(gpu)
            bits(ws).fill_(PAT32)
            out = guarded(m, cout, torch.float16, gpu)
            with _lib.tuning(splitk_fused=fused):
                S = conv_res(gpu, geo, xg, wg, bg, rg[0], 1, rg[1], None, out, ws, cnt)
            assert S > 1, f"{what}: expected a split, got {S}"
            r = _lib.last_gemm_route()
            assert (r["kind"], r["slices"], r["fused"]) == ("split_store", S, fused), (what, r)
            tiles = -(-m // 64) * -(-cout // 64)
            assert written(ws) == (S * tiles * 4096 if fused else S * m * cout), (what, fused, written(ws))
            assert int(cnt.abs().max()) == 0, f"{what}: counters not left zero"
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), f"{what}: fused split differs from slices + reduce kernel"
    close(outs[0][:m], ref, 1e-2, 1e-2, what)
    assert_guard(outs[0], m, 0, cout, what)


@pytest.mark.parametrize("nres", [1, 2])
def test_conv_res0_relu_persist(gpu, nres):
    """res0_relu in the persistent 64-channel conv (conv.hip conv64p_kernel, a
    grid of >= 1024 tiles: 14 x 150 x 133) with one and with two residuals,
    under "conv_persist" 0 (the per-tile direct conv), 1 and 2: bit-identical
    across the three, and against float64."""
    geo = (14, 150, 133, 64, 64, 1)
    x, wp, b, base, oh, ow = conv_problem(*geo)
    m = 14 * oh * ow
    g = gen("conv_persist", nres)
    res = [rn(g, m, 64).half() for _ in range(nres)]
    ref = base + F.relu(res[0].double()) + (res[1].double() if nres > 1 else 0)
    xg, wg, bg = x.to(gpu), wp.to(gpu), b.to(gpu)
    rg = [r.to(gpu) for r in res] + [None]
    got = []
    for flag in (0, 1, 2):
        out = guarded(m, 64, torch.float16, gpu)
        with _lib.tuning(conv_persist=flag):
            conv_res(gpu, geo, xg, wg, bg, rg[0], 1, rg[1], None, out)
        got.append(out)
    close(got[1][:m], ref, 1e-2, 1e-2, f"persistent conv res0_relu nres {nres}")
    assert_guard(got[1], m, 0, 64, "persistent conv")
    assert torch.equal(got[1], got[0]), "conv_persist = 1 differs from the per-tile kernel"
    assert torch.equal(got[2], got[0]), "conv_persist = 2 differs from the per-tile kernel"


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("case,B,h,w,cin,cout,sh,sw,with_res0,split", [
    ("direct", 2, 37, 45, 64, 64, 19, 23, True, False), ("direct_n32", 1, 74, 74, 96, 32, 37, 37, False, False),
    ("wide", 1, 37, 37, 64, 128, 19, 19, False, False), ("split", 1, 19, 19, 384, 64, 10, 10, True, True),
    ("same_size", 2, 19, 19, 64, 64, 19, 19, False, False), ("src_1x1", 1, 19, 19, 64, 64, 1, 1, False, False)])
def test_conv_res1_up(gpu, case, B, h, w, cin, cout, sh, sw, with_res0, split, fold):
    """res1_up (switch "resize_fold" 0 and 1): res1 = the bilinear
    (align_corners) upsample of a smaller map.  The direct conv reads it in
    its epilogue (64 and 32 output channels); N = 128, the split-K shape and
    "resize_fold" = 0 write the upsample into res1 first.  Against float64 with
    the upsample rounded to f16 (as test_conv3x3_up), and bit for bit against
    mde_op_resize_bilinear followed by the conv with that buffer as res1; a
    source of the output's size must equal the plain res1 call, and a 1 x 1
    source is a per-channel constant."""
    geo = (B, h, w, cin, cout, 1)
    x, wp, b, base, oh, ow = conv_problem(*geo)
    m = B * h * w
    g = gen("res1_up", case)
    u16 = rn(g, B, cout, sh, sw).half()
    r0 = rn(g, m, cout).half() if with_res0 else None
    up = F.interpolate(u16.double(), size=(h, w), mode="bilinear", align_corners=True).half().double()
    ref = base + up.permute(0, 2, 3, 1).reshape(m, cout) + (r0.double() if with_res0 else 0)
    xg, wg, bg, ug = x.to(gpu), wp.to(gpu), b.to(gpu), nhwc(u16).to(gpu)
    r0g = r0.to(gpu) if with_res0 else None
    ws = torch.empty(1 << 20, dtype=torch.float32, device=gpu) if split else None
    what = f"conv res1_up {case} fold {fold}"
    with _lib.tuning(resize_fold=fold):
        out = guarded(m, cout, torch.float16, gpu)
        scratch = guarded(m, cout, torch.float16, gpu)
        S = conv_res(gpu, geo, xg, wg, bg, r0g, 0, scratch, (ug, sh, sw), out, ws)
        assert (S > 1) == split, f"{what}: {S} slices"
        r = _lib.last_gemm_route()  # the direct conv reads res1_up itself; every other route has it resized first
        assert (r["kind"], r["resize_first"]) == (("split_store", 1) if split else
                                                  ("conv_direct", int(not fold or case == "wide"))), (what, r)
        close(out[:m], ref, 1e-2, 1e-2, what)
        assert_guard(out, m, 0, cout, what)
        assert_guard(scratch, m, 0, cout, what + " (res1 buffer)")
        # the two-launch form on the same conv route
        resized = guarded(m, cout, torch.float16, gpu)
        op("mde_op_resize_bilinear", ptr(ug), B, sh, sw, cout, h, w, ptr(resized), stream())
        two = guarded(m, cout, torch.float16, gpu)
        op("mde_op_conv3x3_ws", ptr(xg), B, h, w, cin, ptr(wg), wg.shape[1], cout, 1, 0, ptr(bg), 0, ptr(r0g),
           ptr(resized), ptr(two), ptr(ws), ws.numel() if split else 0, None, stream())
        assert torch.equal(out, two), f"{what}: differs from resize launch + conv"
        if (sh, sw) == (h, w):
            plain = guarded(m, cout, torch.float16, gpu)
            op("mde_op_conv3x3", ptr(xg), B, h, w, cin, ptr(wg), wg.shape[1], cout, 1, 0, ptr(bg), 0, ptr(r0g),
               ptr(ug), ptr(plain), stream())
            assert torch.equal(out, plain), f"{what}: a same-size source differs from plain res1"


# ---- (e) the head: hpe and head_metric = 2 -------------------------------------

@functools.lru_cache(maxsize=2)
def head_problem(B, sh, sw, uh, uw, cin):
    g = gen("head", B, sh, sw, uh, uw, cin)
    x16 = rn(g, B, cin, sh, sw).half()
    w1, b1 = rn(g, 32, cin, 3, 3, scale=(9 * cin) ** -0.5), rn(g, 32, scale=0.02)
    pe16 = rn(g, uh * uw, 32, scale=0.5).half()  # hpe_pix = uh * uw: m % hpe_pix wraps across the batch
    w2, b2 = rn(g, 32, scale=32 ** -0.5), 0.05
    up = F.interpolate(x16.double(), size=(uh, uw), mode="bilinear", align_corners=True).half().double()
    hid = F.conv2d(up, w1.half().double(), b1.double(), padding=1)
    hid = F.relu(hid + pe16.double().reshape(1, uh, uw, 32).permute(0, 3, 1, 2))
    z0 = (hid * w2.double().view(1, 32, 1, 1)).sum(1)
    w2 = w2 * min(1.0, 3.5 / float(z0.abs().max()))  # keep exp(z) well inside fp32 and the bar meaningful
    z = (hid * w2.double().view(1, 32, 1, 1)).sum(1) + b2
    return nhwc(x16), conv_w(w1), b1, pe16, w2, b2, z.reshape(-1)


# (upconv_kernel turns persistent past 768 tiles of 16 x 16: 2 x 200 x 200 has 338, 5 x 200 x 200 has 845)
HEAD_CASES = [(2, 24, 24, 42, 42, 32), (1, 9, 40, 16, 70, 64), (2, 100, 100, 200, 200, 128),
              (5, 100, 100, 200, 200, 64), (1, 1, 1, 1, 1, 32)]


@pytest.mark.parametrize("B,sh,sw,uh,uw,cin,metric",
                         [c + (mt,) for c in HEAD_CASES for mt in (0, 1, 2) if c[1] != 100 or mt == 2])
def test_depth_head_pe(gpu, B, sh, sw, uh, uw, cin, metric):
    """hpe (the hidden layer's positional embedding, pixel m % hpe_pix with
    hpe_pix = uh * uw wrapping across the batch) and head_metric = 2 (exp) in
    both head epilogues: store_tile<E_HEAD> of the 4-tap conv3_kernel (switch
    "upconv" = 0) and upconv_kernel ("upconv" = 1; one tile per workgroup up to
    2 x 200 x 200 x 128, the persistent grid at 5 x 200 x 200 x 64).  Against float64 at the head
    bar -- exp compared as log(out) against z, |z| <= 4 --, the two switches
    related as in test_upconv_matches_conv3, and hpe = 0 bit-identical to a
    call without hpe."""
    x, wp, b1, pe16, w2, b2, z = head_problem(B, sh, sw, uh, uw, cin)
    assert float(z.abs().max()) <= 4.0
    m = B * uh * uw
    ref = F.relu(z) if metric == 0 else (torch.sigmoid(z) * 20.0 if metric == 1 else z)
    xg, wg, bg, w2g, peg = x.to(gpu), wp.to(gpu), b1.to(gpu), w2.to(gpu), pe16.to(gpu)
    zero = torch.zeros_like(peg)
    outs = []
    for flag in (0, 1):
        what = f"depth_head_pe {B}x{uh}x{uw}x{cin} metric {metric} upconv {flag}"
        with _lib.tuning(upconv=flag):
            got = []
            for pe in (peg, zero):
                out = guarded(m, 1, torch.float32, gpu)
                op("mde_op_depth_head_pe", ptr(xg), B, sh, sw, cin, uh, uw, ptr(wg), wg.shape[1], ptr(bg), ptr(w2g),
                   b2, metric, 20.0, ptr(pe), uh * uw, ptr(out), stream())
                assert_guard(out, m, 0, 1, what)
                got.append(out)
            plain = guarded(m, 1, torch.float32, gpu)
            op("mde_op_depth_head", ptr(xg), B, sh, sw, cin, uh, uw, ptr(wg), wg.shape[1], ptr(bg), ptr(w2g), b2,
               metric, 20.0, ptr(plain), stream())
        assert torch.equal(got[1], plain), f"{what}: hpe = 0 differs from a call without hpe"
        o = got[0][:m, 0].double().cpu()
        assert bool((o > 0).all()) or metric != 2, f"{what}: exp must be positive"
        close(torch.log(o) if metric == 2 else o, ref, 1e-2, 2e-2, what)
        outs.append(got[0].cpu())
    if cin == 32:
        assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max()
    else:
        assert torch.allclose(outs[0], outs[1], rtol=2e-3, atol=2e-3), (outs[0] - outs[1]).abs().max()


# ---- (f) ConvTranspose into a concat slot --------------------------------------

@pytest.mark.parametrize("s,cin,B,h,w,switches", [(4, 48, 2, 7, 9, {}), (2, 96, 2, 7, 9, {}), (4, 48, 4, 36, 36, {}),
                                                  (2, 64, 1, 17, 17, {"gemm256": 2})],
                         ids=["s4_t64", "s2_t64", "s4_t128_bk32", "s2_gemm256"])
def test_conv_transpose_slot(gpu, s, cin, B, h, w, switches):
    """ldo > N on E_CONVT (mde_op_conv_transpose_ld): the ConvT writes channels
    [8, 8 + cout) of a map with cout + 16 channels, as the DA-V2 / Depth Pro
    concat buffers (ldo = c1p, out16 = base + sd0).  64^2 tiles, the 128^2 BK
    32 tiles (41 x 6 = 246) and gemm256's LDS-staged E_CONVT epilogue
    ("gemm256" = 2).  Against float64, bit for bit against the contiguous
    mde_op_conv_transpose, and the channels on both sides of the slot and the
    rows past the map untouched."""
    cout, ldo = cin, cin + 16
    g = gen("convt", s, cin, B, h, w)
    x16 = rn(g, B, cin, h, w).half()
    wt, b = rn(g, cin, cout, s, s, scale=cin ** -0.5), rn(g, cout, scale=0.02)
    ref = F.conv_transpose2d(x16.double(), wt.half().double(), b.double(), stride=s)
    px = B * h * s * w * s
    ref = ref.permute(0, 2, 3, 1).reshape(px, cout)
    wp = pad_w(wt.permute(2, 3, 1, 0).reshape(s * s * cout, cin)).to(gpu)
    xg, bg = nhwc(x16).to(gpu), b.to(gpu)
    base = guarded(px, ldo, torch.float16, gpu)
    flat = guarded(px, cout, torch.float16, gpu)
    with _lib.tuning(**switches):
        op("mde_op_conv_transpose_ld", ptr(xg), B, h, w, cin, ptr(wp), wp.shape[1], cout, s, ptr(bg),
           ptr(base.view(-1)[8:]), ldo, stream())
        op("mde_op_conv_transpose", ptr(xg), B, h, w, cin, ptr(wp), wp.shape[1], cout, s, ptr(bg), ptr(flat),
           stream())
    close(base[:px, 8:8 + cout], ref, 1e-2, 1e-2, f"convT slot s{s}")
    assert_guard(base, px, 8, 8 + cout, "convT slot")
    assert_guard(flat, px, 0, cout, "convT contiguous")
    assert torch.equal(base[:px, 8:8 + cout], flat[:px]), "slot differs from the contiguous ConvT"


# ---- (g) E_RESID split-K --------------------------------------------------------

def resid_split(gpu, p, x0, f16, splitk, ws, cnt):
    """One mde_op_linear_residual_split call from the initial stream x0 -> (x, partials)."""
    a, wp, b, ls, m, n, k = p
    x = guarded(m, n, x0.dtype, gpu)
    x[:m] = x0
    part = None
    if f16:
        part = torch.empty(n // 32 * m * 2 + 64, device=gpu)
        bits(part).fill_(PAT32)
    op("mde_op_linear_residual_split", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), ptr(ls),
       ptr(None if f16 else x), ptr(x if f16 else None), n, ptr(part), splitk, ptr(ws),
       ws.numel() if ws is not None else 0, ptr(cnt), cnt.numel() if cnt is not None else 0,
       ws.numel() if ws is not None else 0, stream())
    return x, part


@pytest.mark.parametrize("f16", [0, 1], ids=["x32", "xh"])
@pytest.mark.parametrize("route,m,n,k,switches,tiles,area", [
    ("64^2 slices", 300, 384, 1536, {}, 30, 4096),
    ("narrow tile", 1370, 384, 1536, {"narrow_resid": 1}, 0, 0),
    ("64^2 slices, narrow off", 1370, 384, 1536, {"narrow_resid": 0}, 132, 4096),
    ("128^2 x 4 slices, 8 waves", 1281, 1024, 1024, {"w8small": 1}, 88, 16384),
    ("128^2 x 4 slices, 4 waves", 1281, 1024, 1024, {"w8small": 0}, 88, 16384),
], ids=["t64", "narrow", "t64_narrow_off", "t128_w8", "t128_w4"])
def test_residual_splitk(gpu, route, m, n, k, switches, tiles, area, f16):
    """E_RESID split-K (splitk = 4 with `partial`) over the fp32 stream x32 and
    the f16 stream xh with its LN partials: the 64^2 slices, the 128^2 route
    that takes 4 slices (88 tiles, nk = 16) on 8 and on 4 waves ("w8small"), and
    the narrow_resid tile that replaces the split at 1370 x 384 ("narrow_resid"
    1 / 0).  Two-kernel form (splitk_resid_kernel, its 8-lane partial sums) and
    fused form (tile_cnt, switch "splitk_fused" = 1): x / xh bit for bit -- the
    slices are added in the same order --, LN partials of exactly the f16
    values written, counters left zero, repeatable, and the unsplit call
    (splitk = 0) within the same bars."""
    g = gen("resid", m, n, k)
    a16, w16 = rn(g, m, k).half(), rn(g, n, k, scale=k ** -0.5).half()
    b, ls = rn(g, n, scale=0.1), 0.5 + 0.1 * rn(g, n)
    x0 = rn(g, m, n) * 2
    x0 = x0.half() if f16 else x0
    ref = x0.double() + ls.double() * (a16.double() @ w16.double().T + b.double())
    p = (a16.to(gpu), pad_w(w16.float()).to(gpu), b.to(gpu), ls.to(gpu), m, n, k)
    x0g = x0.to(gpu)
    ws = torch.empty(8 << 20, dtype=torch.float32, device=gpu)
    bar = (1e-2, 1e-2) if f16 else (2e-3, 2e-3)
    what = f"residual split {route} {'xh' if f16 else 'x32'}"

    def check(x, part, tag):
        close(x[:m], ref, *bar, f"{what} {tag}")
        assert_guard(x, m, 0, n, f"{what} {tag}")
        if f16:
            cells = n // 32 * m * 2
            close(part[:cells].reshape(n // 32, m, 2), ln_partials_ref(x[:m].cpu()).float(), 1e-5, 1e-3,
                  f"{what} {tag} ln partials")
            assert written(part[cells:]) == 0, f"{what} {tag}: partials written past [n/32][m][2]"

    res = []
    with _lib.tuning(**switches):
        for fused in (0, 1):
            cnt = counters(gpu)
            bits(ws).fill_(PAT32)
            with _lib.tuning(splitk_fused=fused):
                x, part = resid_split(gpu, p, x0g, f16, 4, ws, cnt)
                x2, part2 = resid_split(gpu, p, x0g, f16, 4, ws, cnt)
            r = _lib.last_gemm_route()
            want = {"64^2 slices": dict(kind="split_resid", bm=64, bn=64, fused=fused),
                    "narrow tile": dict(kind="tile", bm=32, bn=64, stages=4, slices=1),
                    "64^2 slices, narrow off": dict(kind="split_resid", bm=64, bn=64, fused=fused),
                    "128^2 x 4 slices, 8 waves": dict(kind="split_resid", bm=128, bn=128, wn=4, slices=4, fused=fused),
                    "128^2 x 4 slices, 4 waves": dict(kind="split_resid", bm=128, bn=128, wn=2, slices=4, fused=fused),
                    }[route]
            assert {f: r.get(f) for f in want} == want and (tiles == 0 or r["slices"] > 1), (what, fused, r)
            # which form ran: S planes of M x N partial sums, or S slots of a tile's area per tile
            nw = written(ws)
            if tiles == 0:
                assert nw == 0, f"{what}: the narrow tile must not touch the workspace ({nw})"
            elif fused:
                assert nw % (tiles * area) == 0 and nw // (tiles * area) > 1, (what, "fused", nw)
            else:
                assert nw % (m * n) == 0 and nw // (m * n) > 1, (what, "two-kernel", nw)
            assert int(cnt.abs().max()) == 0, f"{what}: counters not left zero"
            check(x, part, f"fused {fused}")
            assert torch.equal(x, x2), f"{what} fused {fused}: second call differs"
            if f16:
                assert torch.equal(part, part2), f"{what} fused {fused}: second call's partials differ"
            res.append((x, part))
        unsplit, upart = resid_split(gpu, p, x0g, f16, 0, None, None)
        assert (_lib.last_gemm_route()["kind"], _lib.last_gemm_route()["slices"]) == ("tile", 1), _lib.last_gemm_route()
    assert torch.equal(res[0][0], res[1][0]), f"{what}: fused split differs from slices + reduce kernel"
    if f16:
        cells = n // 32 * m * 2
        close(res[1][1][:cells], res[0][1][:cells], 1e-5, 1e-3, f"{what}: fused vs two-kernel ln partials")
    check(unsplit, upart, "unsplit")
    close(unsplit[:m], res[0][0][:m].double().cpu(), *bar, f"{what}: unsplit vs split")
