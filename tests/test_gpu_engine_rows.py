"""The kernels that had no op-level entry point and were reached only through
whole-engine comparisons at depth-map tolerances, through the ABI 12 wrappers:
launch_layernorm32 (with its T / skip_cls form), launch_rows_layernorm,
launch_prefix_rows, launch_cls_rows, launch_fov_final, launch_head32, and the
patch embed in the two forms the engines run (E_PATCH over the f16 stream with
LN partials / tok0 != 1, and the P32 + gemm32 form of the exact-fp32 engine).

The LayerNorms run on ln_cases.py's row families at its fp32 bounds (4 x E_ref
x max(|ref|, 1), no f16 half ulp: this is where a variance over D - 1 shows on
every element at D = 1024).  The copies are held to equality, with every other
row of the stream and the guard rows behind it untouched.  The patch embeds
run on exact_cases.patch_case operands, for which fp32 accumulation is exact:
equality with float64.  fov_final and head32 are held to 4 x the error of the
same formula in fp32 on the CPU (a dot product; a dot product and expf),
head32 per range of |z|.

head32 and __expf.  head32_kernel computes exp(z) as the hardware's exp2 of z
log2 e; the product's rounding is an error of |z| 2^-24 log2 e in the exponent,
that is |z| 6e-8 relative in the result, on top of the fp32 dot product's own
rounding of z (which the CPU's fp32 evaluation has too).  Measured on an
MI355X, error relative to max(|ref|, 1) (E_ref of the fp32 dot + expf on the
CPU behind it; the bound is 4 x E_ref, no margin had to be raised):

  |z| in        ReLU               max_depth * sigmoid   exp
  [0, 1)        6.1e-08 (9.3e-08)  1.9e-07 (1.9e-07)     1.1e-07 (1.4e-07)
  [1, 5)        1.9e-07 (2.1e-07)  3.6e-07 (4.2e-07)     6.8e-07 (9.7e-07)
  [5, 10)       2.2e-07 (1.9e-07)  8.7e-08 (1.0e-07)     1.6e-06 (1.9e-06)
  [10, 20.5)    2.4e-07 (2.3e-07)  1.0e-07 (1.0e-07)     4.2e-06 (3.1e-06)

For the "exact-fp32" engine's output that means: a metric map (sigmoid) is
within 4e-7 of max_depth's scale of float64 wherever z lies, and an exp head
carries the relative error of z's own fp32 rounding, 2e-7 |z|, of which
__expf's argument scaling is about a third -- the head is as exact as an fp32
evaluation with a library expf.  sigmoid(-100) and sigmoid(100) give exactly 0
and max_depth.
Other measured maxima: layernorm32 2.3e-07 / 1.9e-07 / 2.2e-05 / 2.4e-07 /
1.5e-07 / 0 and rows_layernorm 2.2e-07 / 1.7e-07 / 1.4e-05 / 2.4e-07 / 8.3e-08
/ 0 over gauss / lowvar / bigmean / slicestep / outlier / const (E_ref 3.1e-07
/ 2.9e-07 / 2.3e-05 / 2.9e-07 / 2.4e-07 / 0); fov_final 9.9e-08 at K = 1000
(E_ref 2.0e-07) and 3.6e-08 at K = 7 (1.3e-07); the patch rows' M2 partials
1.3e-07 of the slice's M2 (E_ref 1.8e-07), their sums exact.
"""

import functools

import pytest
import torch

import exact_cases as X
import ln_cases as L
from gpu_util import op, pad_w, ptr, stream
from test_gpu_ops_engine_paths import assert_guard, guarded
from test_gpu_rows import check, const_rows_equal_beta, dev32, ln_site

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ---- LayerNorm with fp32 output ---------------------------------------------------------

@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("d", L.LN_WIDTHS)
def test_layernorm32(gpu, d, eps, skip):
    ln_site(gpu, "mde_op_layernorm32", d, eps, skip, False, False)


@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("d", L.TAP_WIDTHS)
def test_rows_layernorm(gpu, d, eps):
    """In place over rows [5, 9) of 3 sequences; rows [0, 5) bit-unchanged."""
    nseq, T, row0 = 3, 9, 5
    x = L.rows(nseq * T, d)
    g, b = L.affine(d)
    r = torch.arange(nseq * T)
    normed = r % T >= row0
    buf = guarded(nseq * T, d, torch.float32, gpu)
    buf[:nseq * T] = dev32(x, gpu)
    op("mde_op_rows_layernorm", ptr(buf), ptr(dev32(g, gpu)), ptr(dev32(b, gpu)), nseq, T, row0, d, eps, stream())
    got = buf[:nseq * T].cpu()
    assert torch.equal(got[~normed], x.float()[~normed]), "a row below row0 changed"
    ref, fam = L.layernorm64(x, g, b, eps)[normed], r[normed] % L.NF
    what = f"rows_layernorm D{d} eps{eps:g}"
    check(got[normed], ref, L.bound("ln", ref, ref.shape[0], d, eps, False, False, row_family=fam), what, fam, f16=False)
    const_rows_equal_beta(got[normed], b, fam, False, what)
    assert_guard(buf, nseq * T, 0, d, what)


# ---- the row copies -------------------------------------------------------------------------

def nan_stream(rows, d, gpu):
    buf = guarded(rows, d, torch.float32, gpu)
    buf[:rows] = NAN
    return buf


@pytest.mark.parametrize("d", [128, 384])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("sets", [1, 2])
def test_prefix_rows(gpu, sets, frames, d):
    """6 sequences; with 2 sets and 3 frames, sequences 0 and 3 take set 0, the rest set 1."""
    nseq, T, npre = 6, 9, 5
    pre = torch.randn(sets, npre, d, generator=L.gen("prefix", sets, d))
    buf = nan_stream(nseq * T, d, gpu)
    op("mde_op_prefix_rows", ptr(buf), ptr(pre.to(gpu)), nseq, T, npre, d, frames, sets, stream())
    got = buf[:nseq * T].cpu().reshape(nseq, T, d)
    which = [1 if sets == 2 and s % frames else 0 for s in range(nseq)]
    if sets == 2 and frames == 3:
        assert which == [0, 1, 1, 0, 1, 1]
    assert torch.equal(got[:, :npre], pre[which]), "prefix rows differ from their source"
    assert bool(torch.isnan(got[:, npre:]).all()), "a row past the prefix was written"
    assert_guard(buf, nseq * T, 0, d, "prefix_rows")


@pytest.mark.parametrize("d", [384, 1024])
def test_cls_rows(gpu, d):
    nseq, T = 3, 7
    cls = torch.randn(d, generator=L.gen("cls", d))
    buf = nan_stream(nseq * T, d, gpu)
    op("mde_op_cls_rows", ptr(buf), ptr(cls.to(gpu)), nseq, T, d, stream())
    got = buf[:nseq * T].cpu().reshape(nseq, T, d)
    assert torch.equal(got[:, 0], cls.expand(nseq, d)), "cls rows differ from their source"
    assert bool(torch.isnan(got[:, 1:]).all()), "a row past the cls row was written"
    assert_guard(buf, nseq * T, 0, d, "cls_rows")


# ---- fov_final -----------------------------------------------------------------------------------

def dot_e_ref(k):
    """The error of an fp32 dot product of this kind (64 samples, two orders), relative to max(|ref|, 1)."""
    g = L.gen("fov_eref", k)
    a = torch.randn(64, k, generator=g).half().double()
    w = (torch.randn(k, generator=g) * k ** -0.5).float().double()
    ref = a @ w + 0.37
    p = a.float() * w.float()
    e = max(float(((s.double()[:, 0] + 0.37 - ref).abs() / ref.abs().clamp(min=1)).max())
            for s in (p.sum(-1, keepdim=True), p.cumsum(-1)[:, -1:]))
    return e


@pytest.mark.parametrize("k", [1000, 7])
def test_fov_final(gpu, k):
    """K = 1000: not a multiple of the 256 threads; K = 7: most threads idle."""
    Bf = 3
    g = L.gen("fov", k)
    a = torch.randn(Bf, k, generator=g).half()
    w = (torch.randn(k, generator=g) * k ** -0.5).float()
    bias = 0.37
    ref = a.double() @ w.double() + float(torch.tensor(bias, dtype=torch.float32))
    out = guarded(1, Bf, torch.float32, gpu)
    op("mde_op_fov_final", ptr(a.to(gpu)), ptr(w.to(gpu)), bias, k, Bf, ptr(out), stream())
    got = out[0].double().cpu()
    e = dot_e_ref(k)
    rel = (got - ref).abs() / ref.abs().clamp(min=1)
    print(f"MEASURE fov_final K{k} {float(rel.max()):.3e} E_ref {e:.3e}")
    assert bool((rel <= L.MARGIN * e).all()), (k, rel.tolist(), e)
    assert_guard(out, 1, 0, Bf, "fov_final")


def test_fov_final_exact(gpu):
    """in = i / 4, w = j / 64 with small integers: every product and partial sum is exact in fp32 in any order."""
    Bf, k = 3, 300
    g = L.gen("fov_exact")
    a = X.ints(g, (Bf, k), 16) / 4
    w = X.ints(g, (k,), 16) / 64
    out = guarded(1, Bf, torch.float32, gpu)
    op("mde_op_fov_final", ptr(a.half().to(gpu)), ptr(w.float().to(gpu)), 0.25, k, Bf, ptr(out), stream())
    assert torch.equal(out[0].cpu(), (a @ w + 0.25).float()), "fov_final: an exact sum is not exact"


# ---- head32 ------------------------------------------------------------------------------------------

Z_RANGES = ((0.0, 1.0), (1.0, 5.0), (5.0, 10.0), (10.0, 20.5))


@functools.lru_cache(maxsize=None)
def head_operands(m=300):
    """hid [m][32] >= 0 and w2 such that z = b2 + hid . w2 sweeps [-20, 20] over the rows; the last two
    rows sit at -100 and +100."""
    g = L.gen("head32", m)
    w2 = torch.randn(32, generator=g) * 0.2
    w2[0], w2[1] = 0.75, -0.5
    hid = torch.rand(m, 32, generator=g)
    hid[:, :2] = 0
    b2 = 0.1
    noise = hid.double() @ w2.double() + b2
    target = torch.linspace(-20, 20, m, dtype=torch.float64)
    target[-2], target[-1] = -100.0, 100.0
    t = target - noise
    hid[:, 0] = (t.clamp(min=0) / 0.75).float()
    hid[:, 1] = ((-t).clamp(min=0) / 0.5).float()
    z64 = hid.double() @ w2.double() + float(torch.tensor(b2, dtype=torch.float32))
    return hid, w2, b2, z64


def head_act(z, metric, max_depth):
    if metric == 2:
        return z.exp()
    if metric == 1:
        return torch.tensor(max_depth, dtype=torch.float32).to(z.dtype) * torch.sigmoid(z)
    return z.clamp(min=0)


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_head32(gpu, metric):
    """M = 300 (a partial block of 256), z sweeping [-20, 20]; bound per |z| range = 4 x the error of the
    fp32 dot product + expf on the CPU against float64 exp / sigmoid."""
    hid, w2, b2, z64 = head_operands()
    m, max_depth = hid.shape[0], 20.0
    sweep = z64.abs() <= 20.5
    z32 = (hid @ w2 + b2)
    z32b = (hid * w2).cumsum(-1)[:, -1] + b2
    out = guarded(1, m, torch.float32, gpu)
    op("mde_op_head32", ptr(hid.to(gpu)), ptr(w2.to(gpu)), b2, m, metric, max_depth, ptr(out), stream())
    got = out[0].double().cpu()
    ref = head_act(z64, metric, max_depth)
    assert bool(torch.isfinite(got[sweep] if metric == 2 else got).all())   # exp(100) is past fp32
    for lo, hi in Z_RANGES:
        r = sweep & (z64.abs() >= lo) & (z64.abs() < hi)
        scale = ref[r].abs().clamp(min=1)
        e = max(float(((head_act(z, metric, max_depth).double()[r] - ref[r]).abs() / scale).max()) for z in (z32, z32b))
        rel = (got[r] - ref[r]).abs() / scale
        print(f"MEASURE head32 metric{metric} |z| in [{lo}, {hi}) {float(rel.max()):.3e} E_ref {e:.3e}")
        assert bool((rel <= L.MARGIN * e).all()), (metric, lo, hi, float(rel.max()), e)
    if metric == 1:    # sigmoid(-100) and sigmoid(100): 0 and max_depth, finite
        assert got[-2].item() == 0.0 and got[-1].item() == max_depth, got[-2:].tolist()
    assert_guard(out, 1, 0, m, "head32")


# ---- patch embed, the engines' forms -------------------------------------------------------------

def patch_operands(gpu, Bp, H, W, D=384):
    img, w, b, pos, cls_pos, x = X.patch_case(Bp, H, W, D)
    w16 = torch.zeros(D, 3, 14, 16, dtype=torch.float64)
    w16[..., :14] = w
    return (img.float().to(gpu), w16.reshape(D, 672).float(), b.float().to(gpu), pos.float().to(gpu),
            cls_pos.float().to(gpu), cls_pos, x)


@pytest.mark.parametrize("Bp,H,W", [(2, 98, 98), (1, 126, 183)], ids=["2x98x98", "odd_width"])
def test_patch_embed_stream_f16(gpu, Bp, H, W):
    """E_PATCH over the f16 stream: xh = float64 rounded once, the patch rows' partials those of xh, the
    cls rows' partials cls_st, packed at row b T.  126 x 183: 9 x 13 patches, an odd row pitch -- the
    scalar load path of patch_prep_kernel."""
    D = 384
    img, w, b, pos, cls32, cls_pos, x = patch_operands(gpu, Bp, H, W)
    npch = (H // 14) * (W // 14)
    T = npch + 1
    wp = pad_w(w).to(gpu)
    cls_st = L.partials64(cls_pos.float().half().double()[None])[:, 0].float()       # [D/32][2]
    xh = guarded(Bp * T, D, torch.float16, gpu)
    part = torch.full((D // 32 * Bp * T * 2 + 64,), NAN, device=gpu)
    scratch = torch.full((Bp * npch, 672), NAN, dtype=torch.float16, device=gpu)
    op("mde_op_patch_embed_stream", ptr(img), Bp, H, W, ptr(wp), wp.shape[1], ptr(b), ptr(pos), ptr(cls32), D, T, 1,
       ptr(scratch), ptr(None), ptr(xh), ptr(part), ptr(cls_st.to(gpu)), stream())
    want = x.float().half()
    assert torch.equal(xh[:Bp * T].cpu(), want), "xh is not the float64 result rounded once"
    assert_guard(xh, Bp * T, 0, D, "patch_embed_stream xh")
    cells = D // 32 * Bp * T * 2
    assert bool(torch.isnan(part[cells:]).all()), "partials written past [D/32][B T][2]"
    got = part[:cells].reshape(D // 32, Bp * T, 2).cpu()
    r = torch.arange(Bp * T)
    cls_rows, patch_rows = r[r % T == 0], r[r % T != 0]
    assert torch.equal(got[:, cls_rows], cls_st[:, None].expand(-1, Bp, -1)), "the cls rows' partials are not cls_st"
    rows = want.double()[patch_rows]
    ref, scale = L.partials64(rows), L.partials_scale(rows)
    e = max(float(((L.partials32(rows, o).double() - ref).abs() / scale).max()) for o in (0, 1))
    rel = (got[:, patch_rows].double() - ref).abs() / scale
    print(f"MEASURE patch_embed_stream partials sum {float(rel[..., 0].max()):.3e} m2 {float(rel[..., 1].max()):.3e} "
          f"E_ref {e:.3e}")
    assert bool((rel <= L.MARGIN * e).all()), (float(rel.max()), e)


def test_patch_embed_stream_x32_tok0(gpu):
    """tok0 = 5 and no cls_pos (VGGT: the prefix rows belong to another kernel): rows 0 .. 4 of every
    sequence untouched, the patch rows exact."""
    Bp, H, W, D, tok0 = 2, 98, 98, 384, 5
    img, w, b, pos, cls32, cls_pos, x = patch_operands(gpu, Bp, H, W)
    npch = 49
    T = tok0 + npch
    wp = pad_w(w).to(gpu)
    x32 = nan_stream(Bp * T, D, gpu)
    scratch = torch.full((Bp * npch, 672), NAN, dtype=torch.float16, device=gpu)
    op("mde_op_patch_embed_stream", ptr(img), Bp, H, W, ptr(wp), wp.shape[1], ptr(b), ptr(pos), ptr(None), D, T, tok0,
       ptr(scratch), ptr(x32), ptr(None), ptr(None), ptr(None), stream())
    got = x32[:Bp * T].cpu().reshape(Bp, T, D)
    assert bool(torch.isnan(got[:, :tok0]).all()), "a row below tok0 was written"
    assert torch.equal(got[:, tok0:], x.float().reshape(Bp, npch + 1, D)[:, 1:]), "patch rows differ from float64"
    assert_guard(x32, Bp * T, 0, D, "patch_embed_stream x32")


@pytest.mark.parametrize("with_cls", [0, 1], ids=["no_cls", "cls_and_partials"])
def test_patch_embed_stream_f16_tok0(gpu, with_cls):
    """E_PATCH over the f16 stream with tok0 = 5.  Without cls_pos: rows 0 .. 4 of every sequence
    untouched.  With cls_pos, ln_partials and cls_st: row 0 is the cls row and carries cls_st, rows 1 .. 4
    and their partials untouched, the patch rows and their partials as at tok0 = 1."""
    Bp, H, W, D, tok0, npch = 2, 98, 98, 384, 5, 49
    img, w, b, pos, cls32, cls_pos, x = patch_operands(gpu, Bp, H, W)
    T = tok0 + npch
    wp = pad_w(w).to(gpu)
    xh = guarded(Bp * T, D, torch.float16, gpu)
    xh[:Bp * T] = NAN
    cells = D // 32 * Bp * T * 2
    part = torch.full((cells + 64,), NAN, device=gpu)
    cls_st = L.partials64(cls_pos.float().half().double()[None])[:, 0].float()
    scratch = torch.full((Bp * npch, 672), NAN, dtype=torch.float16, device=gpu)
    op("mde_op_patch_embed_stream", ptr(img), Bp, H, W, ptr(wp), wp.shape[1], ptr(b), ptr(pos),
       ptr(cls32 if with_cls else None), D, T, tok0, ptr(scratch), ptr(None), ptr(xh), ptr(part if with_cls else None),
       ptr(cls_st.to(gpu) if with_cls else None), stream())
    got = xh[:Bp * T].cpu().reshape(Bp, T, D)
    want = x.float().half().reshape(Bp, npch + 1, D)
    assert torch.equal(got[:, tok0:], want[:, 1:]), "patch rows are not the float64 result rounded once"
    first = 1 if with_cls else 0
    assert bool(torch.isnan(got[:, first:tok0]).all()), "a row below tok0 was written"
    assert_guard(xh, Bp * T, 0, D, "patch_embed_stream xh tok0")
    if not with_cls:
        assert bool(torch.isnan(part).all())
        return
    assert torch.equal(got[:, 0], want[:, 0]), "the cls row is not cls_pos rounded once"
    assert bool(torch.isnan(part[cells:]).all()), "partials written past [D/32][B T][2]"
    p = part[:cells].reshape(D // 32, Bp, T, 2).cpu()
    assert torch.equal(p[:, :, 0], cls_st[:, None].expand(-1, Bp, -1)), "the cls rows' partials are not cls_st"
    assert bool(torch.isnan(p[:, :, 1:tok0]).all()), "partials of a row below tok0 written"
    rows = want[:, 1:].reshape(Bp * npch, D).double()
    ref, scale = L.partials64(rows), L.partials_scale(rows)
    e = max(float(((L.partials32(rows, o).double() - ref).abs() / scale).max()) for o in (0, 1))
    rel = (p[:, :, tok0:].reshape(D // 32, Bp * npch, 2).double() - ref).abs() / scale
    print(f"MEASURE patch_embed_stream tok0 partials sum {float(rel[..., 0].max()):.3e} m2 {float(rel[..., 1].max()):.3e} "
          f"E_ref {e:.3e}")
    assert bool((rel <= L.MARGIN * e).all()), (float(rel.max()), e)


@pytest.mark.parametrize("Bp,H,W", [(2, 98, 98), (1, 126, 183)], ids=["2x98x98", "odd_width"])
def test_patch_embed32(gpu, Bp, H, W):
    """The exact-fp32 engine's form (fp32 patch rows + gemm32 E_PATCH): equality with float64."""
    D = 384
    img, w, b, pos, cls32, cls_pos, x = patch_operands(gpu, Bp, H, W)
    npch = (H // 14) * (W // 14)
    wp = torch.zeros(D, 672)
    wp[:, :] = w
    x32 = nan_stream(Bp * (npch + 1), D, gpu)
    scratch = torch.full((Bp * npch, 672), NAN, device=gpu)
    op("mde_op_patch_embed32", ptr(img), Bp, H, W, ptr(wp.to(gpu)), 672, ptr(b), ptr(pos), ptr(cls32), D, ptr(scratch),
       ptr(x32), stream())
    assert torch.equal(x32[:Bp * (npch + 1)].cpu(), x.float()), "x32 differs from float64"
    assert_guard(x32, Bp * (npch + 1), 0, D, "patch_embed32")
