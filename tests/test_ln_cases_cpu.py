"""ln_cases.py's claims, proven on the CPU: the families are what they say, the
references agree with each other, the bounds come out of the fp32 evaluation
where the file says they do -- and, for every defect the families exist for,
the float64 reference with that defect built in moves by AT LEAST 4 x THE BOUND
on some element of some family, at every width and eps the GPU file uses.  A
bound can therefore never be wide enough to hide the defect it exists for.

Where a defect is only provable for some output types, the cap is stated at the
case.  Variance over D - 1 moves an output by 1 / (2 D) of (ref - beta).  On an
element of ordinary size that beats 4 x half an f16 ulp only up to D = 384; the
f16 sites still show it at every width (13 x the bound at D = 2048) because
the bound is elementwise and some outputs lie near 0, where an f16 ulp is
small; the fp32-output sites (layernorm32, rows_layernorm) show it on every
element.  A one-pass fp32 variance moves bigmean rows by about 1e-3, less than
4 x half an f16 ulp: it is proven for the fp32 outputs, at every width.
"""

import functools

import pytest
import torch

import ln_cases as L

W_F16_OUT = sorted(set(L.LN_WIDTHS) | {2 * d for d in L.TAP_WIDTHS})   # layernorm*, merge_tokens, tap_concat_ln
W_F32_OUT = sorted(set(L.LN_WIDTHS) | set(L.TAP_WIDTHS))               # layernorm32, rows_layernorm
FOLD_K = (384, 1024)
M = 12 * L.NF    # rows of a proof matrix


def detection(ref, bad, bnd):
    """max over the elements of |bad - ref| / bound (a moved element under a zero bound counts as inf)."""
    d = (bad - ref).abs()
    r = torch.where(bnd > 0, d / bnd.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, float("inf")),
                                                                     torch.zeros_like(d)))
    return r


def detected(ref, bad, bnd, fam=None):
    r = detection(ref, bad, bnd)
    if fam is not None:
        r = r[L.family_rows(ref.shape[0], fam)]
    return float(r.max())


# ---- the families -----------------------------------------------------------------

@pytest.mark.parametrize("d", [64, 384, 1024])
def test_families(d):
    x = L.rows(M, d)
    xh = L.rows(M, d, f16=True)
    assert torch.equal(xh, xh.float().half().double()) and torch.equal(x, x.float().double())
    var = x.var(-1, unbiased=False)
    f = lambda name: L.family_rows(M, name)  # noqa: E731
    assert float(var[f("lowvar")].min()) > 5e-7 and float(var[f("lowvar")].max()) < 1e-4
    assert float((x[f("bigmean")].mean(-1) - 64).abs().max()) < 0.3 and float(var[f("bigmean")].max()) < 0.5
    assert torch.equal(x[f("const")], torch.full((len(f("const")), d), 1.5, dtype=torch.float64))
    assert float(x[f("const")].sum(-1)[0]) == 1.5 * d
    o = x[f("outlier")]
    assert bool((o[:, 7] == 300).all()) and bool((o[:, d - 3] == -180).all())
    # slicestep: the slice means step by 0.5; the between-slice part dominates the variance from 4 slices on
    s = x[f("slicestep")].reshape(-1, d // 32, 32).mean(-1)
    assert float((s[:, 1:] - s[:, :-1] - 0.5).abs().max()) < 0.3
    # every family in every group of 6 consecutive rows
    assert [L.family_of(r) for r in range(6)] == list(L.FAMILIES)


def test_skip_map():
    assert L.skip_map(21, 7).tolist() == [r for r in range(21) if r % 7]


# ---- the references agree with each other -------------------------------------------

@pytest.mark.parametrize("d", [64, 384, 1024])
def test_merge_of_partials_is_the_row_statistics(d):
    x = L.rows(M, d, f16=True)
    mean, var = L.stats64(x)
    m2, v2 = L.merge64(L.partials64(x))
    assert float((mean - m2).abs().max()) <= 1e-12 * 64
    assert float(((var - v2).abs() / var.clamp(min=1e-30)).max()) <= 1e-9


@pytest.mark.parametrize("k", FOLD_K)
def test_fold_is_layernorm_then_linear(k):
    """With c1 the exact row sum, the fold's definition IS ((x - mean) rstd) Wg16^T + c2."""
    x = L.rows(M, k, f16=True)
    wg16, _, c2 = L.fold_weights(64, k)
    mean, var = L.stats64(x)
    direct = ((x - mean) * (var + 1e-6).rsqrt()) @ wg16.T + c2
    fold = L.fold64(x, wg16, wg16.sum(1), c2, 1e-6)
    assert float(((fold - direct).abs() / direct.abs().clamp(min=1)).max()) <= 1e-9


def test_rope_tables_are_the_oracles():
    from oracle import vggt_ref
    cos, sin = L.rope_tables64(9)
    c32, s32 = vggt_ref.rope_tables(32, 9)
    assert float((cos - c32.double()).abs().max()) <= 2e-7 and float((sin - s32.double()).abs().max()) <= 2e-7
    x = torch.randn(3, 11, 64, generator=L.gen("rope"))
    pos = torch.stack([torch.arange(11) % 9, (torch.arange(11) * 4) % 9], 1)
    assert torch.equal(L.rope2d_t(x, pos, c32, s32), vggt_ref.rope2d(x, pos))


# ---- E_ref ------------------------------------------------------------------------------

def test_e_ref_is_fp32_rounding():
    """A few fp32 ulps except where the family cancels (bigmean: mean 64 against a
    deviation of 0.5 loses 7 bits; the const fold: rstd = eps^-1/2 multiplies the
    GEMM's rounding)."""
    for d in W_F16_OUT:
        for eps in L.EPS:
            for f16 in (False, True):
                e = {f: L.e_ref("ln", f, d, eps, f16) for f in L.FAMILIES}
                print("ln", d, eps, f16, {k: f"{v:.2e}" for k, v in e.items()})
                assert e["const"] == 0.0
                assert all(0 < e[f] <= 6e-7 for f in ("gauss", "lowvar", "slicestep", "outlier")), e
                assert 0 < e["bigmean"] <= 1e-4, e
    for k in FOLD_K:
        p = {f: L.e_ref("partials", f, k, 1e-6, True) for f in L.FAMILIES}
        print("partials", k, {a: f"{v:.2e}" for a, v in p.items()})
        assert all(v <= 6e-7 for v in p.values()), p
        for eps in L.EPS:
            e = {f: L.e_ref("fold", f, k, eps, True) for f in L.FAMILIES}
            print("fold", k, eps, {a: f"{v:.2e}" for a, v in e.items()})
            assert all(0 < e[f] <= 1e-5 for f in ("gauss", "lowvar", "slicestep", "outlier")), e
            assert e["bigmean"] <= 2e-3 and e["const"] <= 5e-3, e


def test_margins_only_raise():
    """An entry of ln_cases.MARGINS raises a family's margin, never lowers it.  Its cap -- a quarter
    of the smallest defect shift -- is what the proofs below assert: they take their bounds through
    ln_cases.bound, with the raised margin in it, and demand shift >= 4 x bound."""
    assert all(v >= L.MARGIN for v in L.MARGINS.values())


# ---- every defect moves the reference by >= 4 x the bound ------------------------------

# the proofs are conditions on the inputs: they run on the matrices the GPU files use (rows(m, d) is
# seeded by m) and on this file's own 72 rows
PROOF_ROWS = L.LN_ROWS + (M,)


def ln_case(d, eps, f16_in, f16_out, defect, T=1, skip=False, m=M):
    x = L.rows(m, d, f16_in)
    g, b = L.affine(d)
    ref = L.layernorm64(x, g, b, eps, T, skip)
    bad = L.layernorm64(x, g, b, eps, T, skip, defect=defect)
    fam = None if not skip else L.skip_map(m, T) % L.NF
    bnd = L.bound("ln", ref, ref.shape[0], d, eps, f16_in, f16_out, row_family=fam)
    return ref, bad, bnd, fam


@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("f16_in,f16_out", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("defect", ["eps0", "eps_swapped", "eps_outside"])
def test_ln_eps_defects_show_on_lowvar(defect, f16_in, f16_out, eps):
    for m in PROOF_ROWS:
        for d in (W_F16_OUT if f16_out else W_F32_OUT):
            ref, bad, bnd, _ = ln_case(d, eps, f16_in, f16_out, defect, m=m)
            r = detected(ref, bad, bnd, "lowvar")
            assert r >= 4, (defect, m, d, eps, r)
            # ... and on the older tests' kind of row it stays inside this file's bound for f16 outputs
            if f16_out and defect != "eps_outside":
                assert detected(ref, bad, bnd, "gauss") < 1, (defect, m, d)


@pytest.mark.parametrize("eps", L.EPS)
def test_ln_dminus1(eps):
    """fp32 outputs and f16 outputs, every width (the f16 ones through their outputs near 0)."""
    for m in PROOF_ROWS:
        for d in W_F32_OUT:
            ref, bad, bnd, _ = ln_case(d, eps, False, False, "dminus1", m=m)
            assert detected(ref, bad, bnd) >= 4, (m, d, eps)
        for f16_in in (False, True):
            for d in W_F16_OUT:
                ref, bad, bnd, _ = ln_case(d, eps, f16_in, True, "dminus1", m=m)
                r = detected(ref, bad, bnd)
                print("dminus1 f16 out", m, d, eps, f16_in, f"{r:.1f}")
                assert r >= 4, (m, d, eps, f16_in, r)


@pytest.mark.parametrize("eps", L.EPS)
def test_ln_onepass_variance_shows_on_bigmean(eps):
    """fp32 outputs, every width; with f16 outputs the half ulp hides it."""
    for m in PROOF_ROWS:
        for d in W_F32_OUT:
            ref, bad, bnd, _ = ln_case(d, eps, False, False, "onepass32", m=m)
            assert detected(ref, bad, bnd, "bigmean") >= 4, (m, d, eps, detected(ref, bad, bnd, "bigmean"))


@pytest.mark.parametrize("defect", ["cls_kept", "cls_off_by_one"])
@pytest.mark.parametrize("f16_out", [True, False])
def test_ln_skip_cls_row_position(defect, f16_out):
    B, T = 3, 7
    for d in L.LN_WIDTHS:
        x = L.rows(B * T, d)
        g, b = L.affine(d)
        ref = L.layernorm64(x, g, b, 1e-6, T, True)
        bad = L.layernorm64(x, g, b, 1e-6, T, True, defect=defect)
        assert ref.shape == bad.shape == (B * (T - 1), d)
        bnd = L.bound("ln", ref, ref.shape[0], d, 1e-6, False, f16_out, row_family=L.skip_map(B * T, T) % L.NF)
        r = detection(ref, bad, bnd).amax(1)
        # no row dropped: every output row after the first cls row moves; the wrong row dropped:
        # the first output row of every sequence
        moved = (r >= 4).nonzero().flatten().tolist()
        if defect == "cls_kept":
            assert len(moved) >= B * (T - 1) - (T - 1), (defect, d, moved)
        else:
            assert moved == [s * (T - 1) for s in range(B)], (defect, d, moved)


@functools.lru_cache(maxsize=2)
def fold_problem(m, n, k):
    """The GPU file's own operands for (m, n, k), with x Wg16^T computed once."""
    x = L.rows(m, k, True)
    wg16, c1, c2 = L.fold_weights(n, k)
    return x, wg16, c1, c2, x @ wg16.T


FOLD_DEFECTS = [("eps0", None, "lowvar"), ("eps_swapped", None, "lowvar"), ("no_between", None, "slicestep"),
                ("wrong_pairing", None, "slicestep"), ("wrong_count", None, "slicestep"),
                (None, "m2_about_zero", "bigmean")]


@pytest.mark.parametrize("m,n,k", L.FOLD_SHAPES + ((M, 64, 384), (M, 64, 1024)))
def test_fold_defects(m, n, k):
    """Every fold problem of the GPU file, on its own rows and weights, at both eps."""
    x, wg16, c1, c2, acc = fold_problem(m, n, k)
    rows = {f: L.family_rows(m, f) for f in L.FAMILIES}
    for eps in L.EPS:
        ref = L.fold64(x, wg16, c1, c2, eps, acc=acc)
        bnd = L.bound("fold", ref, m, k, eps, True, True, n)
        for defect, part_defect, fam in FOLD_DEFECTS:
            i = rows[fam]
            bad = L.fold64(x[i], wg16, c1, c2, eps, defect, part_defect, acc=acc[i])
            r = float(detection(ref[i], bad, bnd[i]).max())
            assert r >= 4, (defect or part_defect, fam, m, n, k, eps, r)
            if defect == "no_between":   # the issue's table: the relative move itself is > 1 somewhere
                assert float(((bad - ref[i]).abs() / ref[i].abs().clamp(min=1)).max()) > 1


@pytest.mark.parametrize("m,k", L.PRODUCER_SHAPES + tuple((M, k) for k in FOLD_K))
def test_partials_m2_about_zero_shows_on_bigmean(m, k):
    """On the producers' own matrices (rows(m, n): k is the row width here)."""
    x = L.rows(m, k, True)
    ref, bad = L.partials64(x), L.partials64(x, "m2_about_zero")
    bnd = L.partials_bound(x)
    r = detection(ref, bad, bnd)[:, L.family_rows(m, "bigmean"), 1]
    assert float(r.min()) >= 4      # every bigmean cell
    # the bound is relative to the slice's own M2: a low-variance slice is held as tightly as any
    low = L.family_rows(m, "lowvar")
    assert float((bnd[:, low, 1] / ref[:, low, 1]).max()) <= 4 * 6e-7


@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("defect,fam", [("eps0", "lowvar"), ("eps_swapped", "lowvar"), ("dminus1", None)])
def test_qk_rope_defects(defect, fam, eps):
    """On the q and k matrices of the GPU test (84 rows, keys "q" and "k") and on this file's 72 rows."""
    for m, key in ((84, "q"), (84, "k"), (M, "rows")):
        x = L.rows(m, 64, True, key=key)
        g, b = L.affine(64, key="affine" if key == "rows" else key)
        cos, sin = (t.float() for t in L.rope_tables64(9))
        pos = torch.stack([torch.arange(m) % 9, (torch.arange(m) * 4) % 9], 1)
        ref = L.qk_rope64(x, g, b, eps, pos, cos, sin, 0.18)
        bad = L.qk_rope64(x, g, b, eps, pos, cos, sin, 0.18, defect=defect)
        assert detected(ref, bad, L.bound("qkrope", ref, m, 64, eps, True, True), fam) >= 4, (m, key)
