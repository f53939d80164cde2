"""Every LayerNorm site the ABI reaches -- the row kernels, the producers of the
folded LayerNorm's partials and its consumers -- against float64 on the
adversarial row families of ln_cases.py, at bounds that come from the
reference alone (MARGIN x E_ref x max(|ref|, 1), plus half an f16 ulp for f16
outputs; test_ln_cases_cpu.py proves that no such bound can hide the defect
its family exists for).

Rows are B = 3, T = 7 (21 rows) unless a route needs more: a partial last
group for the 4-rows-per-workgroup and the 16-rows-per-workgroup kernels, the
cls rows 0, 7 and 14 in different wave slots.  Output buffers carry guard rows.
Row r takes family r % 6.  A const row must EQUAL beta rounded to the output
type at the row kernels.

Routes of the fold.  mde_op_linear_lnfold reaches the 64^2 tiles, the 128^2
tiles (BK 32 at K = 384, the 8-wave form at K = 1024), the panel kernel and,
with the switch "panel32" = 1, panel32_kernel, which has a statistics merge and
an rsqrt(var + eps) of its own (three consumer sites in all: gemm.hip's and
gemm_panel.hip's two); mde_op_qkv_lnfold runs on the 64^2 tiles, the panel
kernel and panel32_kernel's E_QKV form.  The route record says kind = "panel"
for both panel kernels: the panel32 cases also run the panel kernel on the same
operands and assert that the two outputs differ (assert_ran_panel32).
launch_gemm never routes a fold problem to gemm256 (gemm.hip gemm_route:
`!lnfold && gemm256_eligible`), so there is no such case here.  The producers
run on the route table of exact_cases.RESID16_ROUTES (64^2, 128 x 64, 128^2,
32 x 64 and the panel kernel at "panel" = 2) plus the split-K reduce in both
forms; every case asserts the route it took.

Each check prints its measured maxima per family (`MEASURE site family value`:
the error beyond half an f16 ulp for f16 outputs, the error itself for fp32
outputs, both relative to max(|ref|, 1)) before it asserts.

Measured on an MI355X, the maximum over every width, eps and case of a site,
next to the largest E_ref it was held to (the bound is 4 x E_ref):

  site                     gauss    lowvar   bigmean  slicestep outlier  const
  layernorm                2.8e-08  1.0e-08  1.8e-05  0        7.7e-09  0
  layernorm_f16            3.4e-08  4.5e-08  9.4e-06  6.3e-08  1.2e-09  0
  merge_tokens (LN)        5.0e-08  6.6e-09  1.4e-05  7.6e-08  9.5e-09  0
  tap_concat_ln            5.8e-08  1.9e-08  1.7e-05  8.0e-09  9.7e-09  0
    E_ref, fp32 rows       3.1e-07  2.9e-07  2.3e-05  2.9e-07  2.4e-07  0
    E_ref, f16 rows        3.1e-07  2.9e-07  6.9e-06  3.0e-07  2.6e-07  0
  qk_norm_rope             1.4e-08  5.2e-09  0        0        0        0
    E_ref                  1.1e-07  1.1e-07  9.7e-08  1.1e-07  2.1e-07  9.4e-10
  producers, sum           6.6e-08  0        0        6.5e-08  1.2e-07  0
  producers, M2            1.8e-07  1.7e-07  0        2.4e-07  2.9e-07  0
    E_ref                  2.0e-07  1.7e-07  0        2.3e-07  2.0e-07  0
  the fold, per route (max over its cases), with the E_ref of the case's own weights:
  lnfold 64^2 (n 96)       6.9e-07  7.5e-08  2.8e-04  5.8e-07  0        1.5e-03
    E_ref n 96, K 384      2.1e-06  1.0e-06  6.4e-04  3.0e-06  1.2e-06  1.1e-03
  lnfold 128^2 BK 32       1.6e-06  4.4e-07  4.2e-04  1.6e-06  6.1e-07  2.8e-03
    E_ref n 1920, K 384    5.9e-06  2.0e-06  1.2e-03  5.3e-06  3.3e-06  3.0e-03
  lnfold panel             2.0e-06  5.6e-07  6.2e-04  1.5e-06  6.8e-07  2.7e-03
  lnfold panel32           2.2e-06  4.4e-07  4.7e-04  1.5e-06  6.9e-07  2.3e-03
    E_ref n 1536, K 384    5.3e-06  1.8e-06  9.8e-04  5.7e-06  2.7e-06  3.1e-03
  qkv_lnfold 64^2          7.5e-07  3.9e-07  3.3e-04  7.1e-07  1.8e-07  1.9e-03
  qkv_lnfold panel         1.8e-06  4.1e-07  4.9e-04  1.3e-06  1.0e-06  1.9e-03
  qkv_lnfold panel32       1.9e-06  5.8e-07  5.0e-04  1.4e-06  5.9e-07  1.8e-03
    E_ref n 1152, K 384    5.0e-06  2.3e-06  9.7e-04  5.0e-06  3.0e-06  2.0e-03
  linear_lnfold_tok        8.8e-07  0        2.6e-04  7.2e-08  0        1.6e-03
    E_ref n 64, K 384      2.5e-06  1.0e-06  4.6e-04  3.6e-06  1.5e-06  1.0e-03
  lnfold 64^2, K 1024      6.1e-07  1.2e-07  7.0e-04  2.5e-06  3.8e-07  4.8e-03
    E_ref n 96, K 1024     2.5e-06  1.3e-06  6.1e-04  5.2e-06  2.0e-06  2.3e-03
  lnfold 128^2, K 1024     2.9e-06  8.9e-07  1.2e-03  3.5e-06  1.0e-06  6.3e-03
    E_ref n 1920, K 1024   4.5e-06  1.8e-06  8.6e-04  8.0e-06  3.3e-06  3.3e-03
  panel / panel32 + GELU   3.0e-05 on every family (gelu_erf's 2.6e-5) but bigmean 4.9e-04 / 4.4e-04 and
                           const 1.0e-03 / 1.3e-03

(The producers' figures are relative to the slice's own sum of |x| and its own
M2.  The fold's const rows are its loosest: rstd = eps^-1/2 = 1000 multiplies
the rounding of x Wg^T - mean c1; the kernels sit at up to 2.1 x E_ref there
(64^2, K = 1024) and at up to 1.4 x on bigmean (128^2, K = 1024), inside the
margin of 4.)

What the first run of this file found: at D = 384 and 768 -- and 2 D = 768,
1536 in tap_concat_ln -- every const row missed beta by up to 5e-5 in
layernorm, layernorm32, merge_tokens, rows_layernorm and tap_concat_ln.  x -
sum * (1 / D) was contracted into one fma, so the deviation came from the
unrounded product 1.5 (1 + 2^-25); mde_device.h row_mean now rounds the mean
first.  layernorm_f16 and qk_norm_rope did not show it and are left as they were.

What these tests catch that the older ones do not.  Each defect was built into
a scratch copy of the library, and the older LayerNorm / fold tests
(test_gpu_ops.py, test_gpu_vggt.py, test_gpu_depth_pro.py,
test_gpu_ops_engine_paths.py, test_gpu_panel_switch.py, test_gpu_exact.py: 80
cases) and the two new files (153 cases) run against it:
  * eps dropped at gemm.hip's consumer, rsqrtf(var): no older test against a
    reference fails -- only the four that tie the panel kernel to the tiles bit
    for bit (test_panel_gemm_bit_exact[lnfold_gelu, qkv_lnfold],
    test_store_across_switch[lnfold_gelu, lnfold_gelu_ragged]).  Here every tile
    case of test_linear_lnfold (7), test_qkv_lnfold (2) and
    test_linear_lnfold_tok (2) fails; the panel cases pass, as they must: the
    panel kernel has its own consumer site.
  * 1 / D -> 1 / (D - 1) in row_layernorm: of the older tests only
    test_merge_tokens_op[*-True] (D = 128) fails; test_layernorm,
    test_row_layernorm_kernels_bit_identical and the engine tests pass.  Here
    all of test_layernorm (20), test_merge_tokens_ln (20), test_layernorm32 (20)
    and test_rows_layernorm (12) fail, at every width up to 1024.
  * the between-slice term dropped in ln_merge_stats: the older fold tests do
    fail (test_linear_lnfold 7 of 7, test_linear_lnfold_strided 2,
    test_linear_lnfold_tok 4) -- their rows' slice means differ enough --, and
    so do all 14 fold cases here.
(These three runs were made before the panel32 and the panel qkv cases were
added.)  The same eps defect at gemm_panel.hip's two sites, the older fold /
panel tests (35 cases) and this file's fold cases (20) against each:
  * at panel32_kernel's site: all 35 older cases pass, test_panel32_matches_
    tile_kernel among them; here exactly test_linear_lnfold[panel32,
    panel32_gelu, panel32_eps5] and test_qkv_lnfold[panel32, panel32_eps5] fail.
  * at panel_gemm_kernel's site: the older tests fail only in the four
    bit-equality ties named above; here exactly test_linear_lnfold[panel,
    panel_gelu, panel_eps5] and test_qkv_lnfold[panel] fail.
"""

import functools

import pytest
import torch

import exact_cases as X
import ln_cases as L
from gpu_util import op, pad_w, ptr, stream, vt_perm
from monocular_depth_estimation_trt_amd import _lib
from test_gpu_ops_engine_paths import assert_guard, guarded

pytestmark = pytest.mark.gpu

B, T = 3, 7
ROWS = B * T


def check(got, ref, bnd, what, fam_idx=None, f16=True):
    """|got - ref| <= bnd elementwise (NaN fails); prints the per-family maxima first."""
    g = got.detach().double().cpu().reshape(ref.shape)
    err = (g - ref).abs()
    fam = (torch.arange(ref.shape[0]) % L.NF) if fam_idx is None else fam_idx
    excess = ((err - 0.5 * L.ulp16(ref)) if f16 else err) / ref.abs().clamp(min=1.0)
    for i, f in enumerate(L.FAMILIES):
        r = fam == i
        if bool(r.any()):
            print(f"MEASURE {what} {f} {max(float(excess[r].nan_to_num(float('inf')).max()), 0.0):.3e}")
    bad = ~(err <= bnd)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        row = i // (ref.numel() // ref.shape[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, rows of "
            f"{sorted({L.FAMILIES[int(fam[r])] for r in bad.reshape(ref.shape[0], -1).any(1).nonzero().flatten()})}; "
            f"first at row {row} ({L.FAMILIES[int(fam[row])]}): got {float(g.flatten()[i])!r} ref "
            f"{float(ref.flatten()[i])!r} err {float(err.flatten()[i]):.3e} bound {float(bnd.flatten()[i]):.3e}")


def dev32(t, gpu):
    return t.float().to(gpu)


def const_rows_equal_beta(y, b, fam, f16, what):
    r = (fam == L.FAMILIES.index("const")).nonzero().flatten()
    want = b.float().half() if f16 else b.float()
    got = y.detach().cpu()[r]
    assert torch.equal(got, want.expand_as(got)), f"{what}: a const row is not beta"


# ---- row kernels ---------------------------------------------------------------------

def ln_site(gpu, opname, d, eps, skip, f16_in, f16_out):
    x = L.rows(ROWS, d, f16_in)
    g, b = L.affine(d)
    ref = L.layernorm64(x, g, b, eps, T, bool(skip))
    fam = (L.skip_map(ROWS, T) if skip else torch.arange(ROWS)) % L.NF
    n_out = ref.shape[0]
    y = guarded(n_out, d, torch.float16 if f16_out else torch.float32, gpu)
    xd = x.float().half().to(gpu) if f16_in else dev32(x, gpu)
    op(opname, ptr(xd), ptr(y), ptr(dev32(g, gpu)), ptr(dev32(b, gpu)), ROWS, d, eps, T, skip, stream())
    what = f"{opname} D{d} eps{eps:g} skip{skip}"
    check(y[:n_out], ref, L.bound("ln", ref, n_out, d, eps, f16_in, f16_out, row_family=fam), what, fam, f16_out)
    const_rows_equal_beta(y[:n_out], b, fam, f16_out, what)
    assert_guard(y, n_out, 0, d, what)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("d", L.LN_WIDTHS)
def test_layernorm(gpu, d, eps, skip):
    ln_site(gpu, "mde_op_layernorm", d, eps, skip, False, True)


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("d", L.LN_WIDTHS)
def test_layernorm_f16(gpu, d, eps, skip):
    """layernorm_h8_kernel: the hand-written copy, 16 lanes per row."""
    ln_site(gpu, "mde_op_layernorm_f16", d, eps, skip, True, True)


def merge_source_rows(Bn, n, G, pad, base, Tt):
    """The source row of every output pixel (b, Y, X) of a merged level map
    (depth_pro_ops.hip merge_tokens_kernel), row-major."""
    HW = n * G - 2 * (n - 1) * pad

    def split(v):
        first, mid = G - pad, G - 2 * pad
        if n == 1 or v < first:
            return 0, v
        k = v - first
        p = min(1 + k // mid, n - 1)
        return p, pad + k - (p - 1) * mid
    out = []
    for b in range(Bn):
        for Y in range(HW):
            for Xc in range(HW):
                (pr, ty), (pc, tx) = split(Y), split(Xc)
                out.append(((base + pr * n + pc) * Bn + b) * Tt + 1 + ty * G + tx)
    return torch.tensor(out)


@pytest.mark.parametrize("n,pad", [(1, 0), (2, 1)])
@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("d", L.LN_WIDTHS)
def test_merge_tokens_ln(gpu, d, eps, n, pad):
    G = 3
    Tt, nseq = G * G + 1, n * n * B
    x = L.rows(nseq * Tt, d)
    g, b = L.affine(d)
    src = merge_source_rows(B, n, G, pad, 0, Tt)
    ref = L.layernorm64(x, g, b, eps)[src]
    fam = src % L.NF
    y = guarded(len(src), d, torch.float16, gpu)
    op("mde_op_merge_tokens", ptr(dev32(x, gpu)), B, Tt, d, n, G, pad, 0, ptr(dev32(g, gpu)), ptr(dev32(b, gpu)), eps,
       ptr(y), stream())
    what = f"merge_tokens D{d} eps{eps:g} n{n}"
    check(y[:len(src)], ref, L.bound("ln", ref, len(src), d, eps, False, True, row_family=fam), what, fam)
    const_rows_equal_beta(y[:len(src)], b, fam, True, what)
    assert_guard(y, len(src), 0, d, what)


@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("d", L.TAP_WIDTHS)
def test_tap_concat_ln(gpu, d, eps):
    """LayerNorm over cat(xa, xb), 2 D wide (tap_concat_ln_kernel: its own copy of the two passes)."""
    npre = 1
    x = L.rows(ROWS, 2 * d)
    g, b = L.affine(2 * d)
    keep = L.skip_map(ROWS, T)
    ref = L.layernorm64(x, g, b, eps)[keep]
    fam = keep % L.NF
    y = guarded(len(keep), 2 * d, torch.float16, gpu)
    xa, xb = x[:, :d].contiguous(), x[:, d:].contiguous()
    op("mde_op_tap_concat_ln", ptr(dev32(xa, gpu)), ptr(dev32(xb, gpu)), B, T, npre, d, ptr(dev32(g, gpu)),
       ptr(dev32(b, gpu)), eps, ptr(y), stream())
    what = f"tap_concat_ln D{d} eps{eps:g}"
    check(y[:len(keep)], ref, L.bound("ln", ref, len(keep), 2 * d, eps, False, True, row_family=fam), what, fam)
    const_rows_equal_beta(y[:len(keep)], b, fam, True, what)
    assert_guard(y, len(keep), 0, 2 * d, what)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_qk_norm_rope(gpu, eps):
    """qk_norm_rope_kernel (the third copy, 8 lanes per row): special tokens
    (position (0, 0)) are the plain LayerNorm, times q_scale for q; grid tokens
    the oracle's rope2d of the float64 LayerNorm; pad rows stay zero."""
    from monocular_depth_estimation_trt_amd import pack_vggt
    from oracle import vggt_ref
    gh = gw = 3
    npre, H, nseq, frames = 5, 1, 3, 2
    P = npre + gh * gw
    Tt, Tpad, BH = frames * P, 32, nseq * H
    cos16, sin16 = (torch.from_numpy(t) for t in pack_vggt.rope_tables(gw + 2))     # [pos][16]: the op's tables
    cos, sin = torch.cat((cos16, cos16), -1), torch.cat((sin16, sin16), -1)         # the oracle's duplicated form
    pos = vggt_ref.rope_positions(gh, gw, npre).repeat(frames, 1).repeat(BH, 1)      # [BH Tt][2]
    qs = 0.125 * 1.4426950408889634
    bufs, refs, affs = [], [], []
    for name, scale in (("q", qs), ("k", 1.0)):
        x = L.rows(BH * Tt, 64, True, key=name)
        g, b = L.affine(64, key=name)
        ref = L.qk_rope64(x, g, b, eps, pos, cos, sin, scale)
        special = (pos == 0).all(1)
        assert torch.equal(ref[special], (L.layernorm64(x, g, b, eps) * scale)[special])
        buf = torch.zeros(BH, Tpad, 64, dtype=torch.float16, device=gpu)
        buf[:, :Tt] = x.float().half().reshape(BH, Tt, 64).to(gpu)
        bufs.append(buf)
        refs.append(ref)
        affs += [dev32(g, gpu), dev32(b, gpu)]
    op("mde_op_qk_norm_rope", ptr(bufs[0]), ptr(bufs[1]), ptr(affs[0]), ptr(affs[1]), ptr(affs[2]), ptr(affs[3]), BH,
       Tt, Tpad, P, npre, gw, ptr(cos16.to(gpu)), ptr(sin16.to(gpu)), qs, eps, stream())
    for name, buf, ref in zip("qk", bufs, refs):
        check(buf[:, :Tt], ref, L.bound("qkrope", ref, BH * Tt, 64, eps, True, True), f"qk_norm_rope {name} eps{eps:g}")
        assert float(buf[:, Tt:].abs().max()) == 0.0, "pad rows written"


# ---- producers of the partials -------------------------------------------------------

def check_partials(part, x, what, m):
    """part [n/32][m][2] against the float64 partials of the rows x, per family, each
    cell relative to its own slice (ln_cases.partials_bound)."""
    ref = L.partials64(x)
    g = part.detach().double().cpu().reshape(ref.shape)
    err, bnd = (g - ref).abs(), L.partials_bound(x)
    rel = err / L.partials_scale(x)
    for i, f in enumerate(L.FAMILIES):
        r = L.family_rows(m, f)
        print(f"MEASURE {what} {f} sum {float(rel[:, r, 0].nan_to_num(float('inf')).max()):.3e} "
              f"m2 {float(rel[:, r, 1].nan_to_num(float('inf')).max()):.3e}")
    bad = ~(err <= bnd)
    if bool(bad.any()):
        s, r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} partials outside the bound; first slice {s} "
                             f"row {r} ({L.family_of(r)}) {'sum M2'.split()[c]}: got {float(g[s, r, c])!r} ref "
                             f"{float(ref[s, r, c])!r} bound {float(bnd[s, r, c]):.3e}")


PRODUCER_ROUTES = [c for c in X.RESID16_ROUTES if c[0] != "gemm256"] + \
    [("t64_300", 300, 384, 384, {}, dict(kind="tile", bm=64, bn=64))]


@pytest.mark.parametrize("route,m,n,k,switches,want", PRODUCER_ROUTES, ids=[c[0] for c in PRODUCER_ROUTES])
def test_producer_partials(gpu, route, m, n, k, switches, want):
    """a = 0, bias = 0, layer_scale = 1: xh stays the family rows, bit for bit, and
    the partials are those of the family rows."""
    x = L.rows(m, n, True)
    xh = guarded(m, n, torch.float16, gpu)
    xh[:m] = x.float().half().to(gpu)
    a = torch.zeros(m, k, dtype=torch.float16, device=gpu)
    wp = pad_w(X.lin_case(128, n, k)[1].float()).to(gpu)     # any finite weights: a = 0
    part = torch.full((n // 32 * m * 2 + 64,), float("nan"), device=gpu)
    with _lib.tuning(**switches):
        op("mde_op_linear_residual_f16", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(torch.zeros(n, device=gpu)),
           ptr(torch.ones(n, device=gpu)), ptr(xh), n, ptr(part), stream())
    r = _lib.last_gemm_route()
    assert {f: r.get(f) for f in want} == want, (route, want, r)
    assert torch.equal(xh[:m].cpu(), x.float().half()), f"{route}: x + 1 * (0 + 0) changed x"
    assert_guard(xh, m, 0, n, route)
    cells = n // 32 * m * 2
    check_partials(part[:cells], x, f"producer {route} {m}x{n}", m)
    assert bool(torch.isnan(part[cells:]).all()), f"{route}: partials written past [n/32][m][2]"


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("route,m,n,k,switches,want", X.RESID_SPLIT_ROUTES, ids=[c[0] for c in X.RESID_SPLIT_ROUTES])
def test_producer_partials_splitk(gpu, route, m, n, k, switches, want, fused):
    """The split-K reduce (two kernels) and the fused tail, splitk = 4."""
    x = L.rows(m, n, True)
    xh = guarded(m, n, torch.float16, gpu)
    xh[:m] = x.float().half().to(gpu)
    a = torch.zeros(m, k, dtype=torch.float16, device=gpu)
    wp = pad_w(X.lin_case(128, n, k)[1].float()).to(gpu)     # any finite weights: a = 0
    part = torch.full((n // 32 * m * 2 + 64,), float("nan"), device=gpu)
    ws = torch.empty(8 << 20, dtype=torch.float32, device=gpu)
    cnt = torch.zeros(1024, dtype=torch.int32, device=gpu)
    with _lib.tuning(splitk_fused=fused, **switches):
        op("mde_op_linear_residual_split", ptr(a), k, ptr(wp), wp.shape[1], m, n, k, ptr(torch.zeros(n, device=gpu)),
           ptr(torch.ones(n, device=gpu)), ptr(None), ptr(xh), n, ptr(part), 4, ptr(ws), ws.numel(), ptr(cnt),
           cnt.numel(), ws.numel(), stream())
    r = _lib.last_gemm_route()
    want = dict(want, fused=fused)
    assert {f: r.get(f) for f in want} == want, (route, want, r)
    assert torch.equal(xh[:m].cpu(), x.float().half()), f"{route}: x + 1 * (0 + 0) changed x"
    assert_guard(xh, m, 0, n, route)
    cells = n // 32 * m * 2
    check_partials(part[:cells], x, f"producer split {route} fused{fused}", m)
    assert bool(torch.isnan(part[cells:]).all()) and int(cnt.abs().max()) == 0


@pytest.mark.parametrize("route,m,n,k,switches,want", [X.RESID16_ROUTES[0], X.RESID16_ROUTES[2]], ids=["t64", "t128"])
def test_producer_partials_of_written_rows(gpu, route, m, n, k, switches, want):
    """An ordinary update (a != 0) on exact operands: the rows written are known
    exactly, and the partials are theirs.  These rows are no family: the bound is 4 x
    the error of the fp32 evaluation on these very rows, per cell scale."""
    a, w, b, acc = X.lin_case(m, n, k)
    g = X.gen("resid", m, n, k, 1)
    ls, x0 = X.layerscale(g, n), X.resid16(g, (m, n))
    rows = (x0.double() + ls.double() * (acc + b)).float().half()
    xh = x0.to(gpu)
    part = torch.full((n // 32, m, 2), float("nan"), device=gpu)
    wp = pad_w(w.float()).to(gpu)
    with _lib.tuning(**switches):
        op("mde_op_linear_residual_f16", ptr(a.half().to(gpu)), k, ptr(wp), wp.shape[1], m, n, k, ptr(b.float().to(gpu)),
           ptr(ls.to(gpu)), ptr(xh), n, ptr(part), stream())
    assert torch.equal(xh.cpu(), rows), f"{route}: xh is not the float64 result rounded once"
    x = rows.double()
    ref, scale = L.partials64(x), L.partials_scale(x)
    e = max(float(((L.partials32(x, o).double() - ref).abs() / scale).max()) for o in (0, 1))
    rel = (part.double().cpu() - ref).abs() / scale
    print(f"MEASURE producer written rows {route} sum {float(rel[..., 0].max()):.3e} m2 {float(rel[..., 1].max()):.3e} "
          f"E_ref {e:.3e}")
    assert bool((rel <= L.MARGIN * e).all()), (route, float(rel.max()), e)


# ---- consumers -------------------------------------------------------------------------

def fold_bound(pre, post, m, n, k, eps, act):
    """The fold's bound before the activation, carried through it: GELU's slope is at
    most 1.13, and gelu_erf adds its documented 2.6e-5 + 2^-20 |ref| (exact_cases.gelu_bound)."""
    b = L.bound("fold", pre, m, k, eps, True, False, n)
    if act == 2:
        b = 1.13 * b + 2.6e-5 + 2.0 ** -20 * post.abs()
    return b + 0.5 * L.ulp16(post)


def assert_ran_panel32(got32, got_panel, what):
    """The route record says kind = "panel" for panel_gemm_kernel and panel32_kernel alike.
    launch_panel_gemm takes panel32_kernel for every E_STORE / E_QKV problem while the switch is 1, and
    the two kernels add the same products in another fp32 association: over this many outputs they
    cannot agree bit for bit, so a differing output shows that the switch selected another kernel."""
    assert not torch.equal(got32, got_panel), f"{what}: panel32 = 1 gave the panel kernel's bits"


@functools.lru_cache(maxsize=4)
def fold_operands(m, n, k, eps):
    x = L.rows(m, k, True)
    wg16, c1, c2 = L.fold_weights(n, k)
    return x, wg16, c1, c2, L.fold64(x, wg16, c1, c2, eps)


FOLD_ROUTES = [   # (route, m, n, k, act, eps, switches, route fields)
    ("t64", 77, 96, 384, 0, 1e-6, {}, dict(kind="tile", bm=64, bn=64)),
    ("t64_eps5", 77, 96, 384, 0, 1e-5, {}, dict(kind="tile", bm=64, bn=64)),
    ("t128_bk32", 2035, 1920, 384, 0, 1e-6, {}, dict(kind="tile", bm=128, bn=128, bk=32)),
    ("t128_bk32_eps5", 2035, 1920, 384, 0, 1e-5, {}, dict(kind="tile", bm=128, bn=128, bk=32)),
    ("panel", 16397, 1536, 384, 0, 1e-6, {}, dict(kind="panel")),
    ("panel_gelu", 16397, 1536, 384, 2, 1e-6, {}, dict(kind="panel")),
    ("panel_eps5", 16397, 1536, 384, 0, 1e-5, {}, dict(kind="panel")),
    # panel32_kernel (switch "panel32"): its own stats_merge and rsqrtf(var + ln_eps), gemm_panel.hip
    ("panel32", 16397, 1536, 384, 0, 1e-6, {"panel32": 1}, dict(kind="panel")),
    ("panel32_gelu", 16397, 1536, 384, 2, 1e-6, {"panel32": 1}, dict(kind="panel")),
    ("panel32_eps5", 16397, 1536, 384, 0, 1e-5, {"panel32": 1}, dict(kind="panel")),
    ("t64_k1024", 77, 96, 1024, 0, 1e-6, {}, dict(kind="tile", bm=64, bn=64)),
    ("t128_k1024", 2035, 1920, 1024, 0, 1e-6, {}, dict(kind="tile", bm=128, bn=128, bk=64)),
    ("t128_k1024_eps5", 2035, 1920, 1024, 0, 1e-5, {}, dict(kind="tile", bm=128, bn=128, bk=64)),
]


@pytest.mark.parametrize("route,m,n,k,act,eps,switches,want", FOLD_ROUTES, ids=[c[0] for c in FOLD_ROUTES])
def test_linear_lnfold(gpu, route, m, n, k, act, eps, switches, want):
    x, wg16, c1, c2, pre = fold_operands(m, n, k, eps)
    post = X.gelu64(pre) if act == 2 else pre
    wgp = pad_w(wg16.float()).to(gpu)
    xd, part, c1d, c2d = x.float().half().to(gpu), dev32(L.partials64(x), gpu), dev32(c1, gpu), dev32(c2, gpu)

    def run(sw):
        out = guarded(m, n, torch.float16, gpu)
        with _lib.tuning(**sw):
            op("mde_op_linear_lnfold", ptr(xd), ptr(part), eps, ptr(wgp), wgp.shape[1], ptr(c1d), ptr(c2d), m, n, k, act,
               ptr(out), n, stream())
        r = _lib.last_gemm_route()
        assert {f: r.get(f) for f in want} == want, (route, sw, want, r)
        return out

    out = run(switches)
    check(out[:m], post, fold_bound(pre, post, m, n, k, eps, act), f"linear_lnfold {route}")
    assert_guard(out, m, 0, n, route)
    if switches.get("panel32"):
        assert_ran_panel32(out, run(dict(switches, panel32=0)), route)


QKV_CASES = [   # (case, B, T, H, eps, switches, route fields)
    ("t64", 2, 50, 6, 1e-6, {}, dict(kind="tile")),
    ("t64_eps5", 2, 50, 6, 1e-5, {}, dict(kind="tile")),
    ("panel", 480, 37, 6, 1e-6, {"panel32": 0}, dict(kind="panel")),
    ("panel32", 480, 37, 6, 1e-6, {"panel32": 1}, dict(kind="panel")),      # panel32_kernel<E_QKV, ., fold>
    ("panel32_eps5", 480, 37, 6, 1e-5, {"panel32": 1}, dict(kind="panel")),
]


@pytest.mark.parametrize("case,Bq,Tq,H,eps,switches,want", QKV_CASES, ids=[c[0] for c in QKV_CASES])
def test_qkv_lnfold(gpu, case, Bq, Tq, H, eps, switches, want):
    D, Tp, m = 64 * H, -(-Tq // 64) * 64, Bq * Tq
    qs = 0.125
    x, wg16, c1, c2, pre = fold_operands(m, 3 * D, D, eps)
    wgp = pad_w(wg16.float()).to(gpu)
    xd, part, c1d, c2d = x.float().half().to(gpu), dev32(L.partials64(x), gpu), dev32(c1, gpu), dev32(c2, gpu)

    def run(sw):
        q = torch.zeros(Bq * H, Tp, 64, dtype=torch.float16, device=gpu)
        kk = torch.zeros_like(q)
        vt = torch.zeros(Bq * H, 64, Tp, dtype=torch.float16, device=gpu)
        with _lib.tuning(**sw):
            op("mde_op_qkv_lnfold", ptr(xd), ptr(part), eps, ptr(wgp), wgp.shape[1], ptr(c1d), ptr(c2d), Bq, Tq, H, Tp,
               qs, ptr(q), ptr(kk), ptr(vt), stream())
        r = _lib.last_gemm_route()
        assert {f: r.get(f) for f in want} == want, (case, sw, want, r)
        return q, kk, vt

    q, kk, vt = run(switches)
    full = pre.reshape(Bq, Tq, 3, H, 64)
    bnd_pre = L.bound("fold", pre, m, D, eps, True, False, 3 * D).reshape(Bq, Tq, 3, H, 64)
    perm = vt_perm(Tq).to(gpu)
    # every (batch, head) block of Tq rows keeps the token order: row t of block (b, h) is x row b Tq + t
    fam = ((torch.arange(Bq)[:, None, None] * Tq + torch.arange(Tq)[None, None, :]).expand(Bq, H, Tq) % L.NF).reshape(-1)
    for name, idx, scale, got in (("q", 0, qs, q[:, :Tq]), ("k", 1, 1.0, kk[:, :Tq]),
                                  ("v", 2, 1.0, vt[:, :, perm].transpose(1, 2))):
        ref = (full[:, :, idx] * scale).permute(0, 2, 1, 3).reshape(Bq * H * Tq, 64)
        bnd = (bnd_pre[:, :, idx] * scale).permute(0, 2, 1, 3).reshape(Bq * H * Tq, 64) + 0.5 * L.ulp16(ref)
        check(got.reshape(Bq * H * Tq, 64), ref, bnd, f"qkv_lnfold {case} {name} eps{eps:g}", fam)
    pad = torch.ones(Tp, dtype=torch.bool, device=gpu)
    pad[perm] = False
    assert float(q[:, Tq:].abs().max()) == 0 and float(vt[:, :, pad].abs().max()) == 0, "pad must stay zero"
    if switches.get("panel32"):
        assert_ran_panel32(torch.cat([t.flatten() for t in (q, kk, vt)]),
                           torch.cat([t.flatten() for t in run(dict(switches, panel32=0))]), case)


@pytest.mark.parametrize("eps", L.EPS)
def test_linear_lnfold_tok(gpu, eps):
    """3 sequences of 7 tokens, the cls rows (NaN in x and in the partials) skipped."""
    n, k = 64, 384
    x, wg16, c1, c2, pre = fold_operands(ROWS, n, k, eps)
    keep = L.skip_map(ROWS, T)
    ref, fam = pre[keep], keep % L.NF
    xd, part = x.float().half(), L.partials64(x).float()
    xd[torch.arange(0, ROWS, T)] = float("nan")
    part[:, torch.arange(0, ROWS, T)] = float("nan")
    out = guarded(len(keep), n, torch.float16, gpu)
    wgp = pad_w(wg16.float()).to(gpu)
    op("mde_op_linear_lnfold_tok", ptr(xd.to(gpu)), ptr(part.to(gpu)), eps, ptr(wgp), wgp.shape[1], ptr(dev32(c1, gpu)),
       ptr(dev32(c2, gpu)), B, T, n, k, 0, ptr(out), n, stream())
    bnd = L.bound("fold", ref, len(keep), k, eps, True, True, n, row_family=fam)
    check(out[:len(keep)], ref, bnd, f"linear_lnfold_tok eps{eps:g}", fam)
    assert_guard(out, len(keep), 0, n, "linear_lnfold_tok")
