"""Test helper (not a test module): adversarial LayerNorm rows, float64
references of every LayerNorm form the library has, and bounds that come from
the reference alone.

Row families.  Row r of any test matrix takes family r % 6, so every tile and
every workgroup sees them mixed:

  gauss      rn * 3 + 1.5                     the older tests' kind of row
  lowvar     rn * 1e-3 * 2^(r % 4)            variance 1e-6 .. 6e-5: eps decides the result
  bigmean    64 + rn * 0.5                    one-pass variance, x Wg - mean c1, M2 about 0
  slicestep  slice s of 32 columns centred at 0.5 (s - mean_s), + rn * 0.25
                                              the between-slice term and the slice order of the merge
  outlier    rn, column 7 = 300, column D - 3 = -180   sums that lose the small terms, f16 range
  const      1.5 everywhere                   the deviation is exactly 0: the output IS beta

For f16-input sites the rows are rounded to f16 first and every reference is
computed from the rounded values.

References (float64, rounded once to the output type by the caller):
layernorm64 (with the cls-skip row map), partials64 (sum and M2 about the slice
mean per 32-column slice), fold64 -- the fold's own definition rstd (x Wg16^T -
mean c1) + c2 with exact statistics, no intermediate f16 rounding --, and
qk_rope64.  Each takes a `defect` that builds one wrong formula into it; the
CPU test (test_ln_cases_cpu.py) proves that every defect moves the reference
by at least 4 x the bound on some family.

Bounds.  E_ref(kind, family, ...) is the largest error, relative to max(|ref|,
1), of a plain fp32 evaluation of the same formula on the CPU against float64
(two-pass LayerNorm; partials from 32-term fp32 sums; the fold with an fp32
GEMM and an fp32 merge of the partials), over SAMPLE rows of the family and
two summation orders (torch's blocked sum and the strict index order).  The
GPU bound is MARGIN x E_ref x max(|ref|, 1) for fp32 outputs, plus half an
f16 ulp of the reference for f16 outputs.  MARGIN = 4 covers the kernels'
other summation order (per-lane index order, then a butterfly) and v_rsq_f32
against a correctly rounded root, a few fp32 ulps each.

E_ref is a sample maximum, not a worst case: SAMPLE rows of the family (not
the test's own rows), for the fold against the weights of the case itself
(fold_weights(n, k): the same n, so the same Wg, c1 and c2 the kernel is
given).  A test with many more outputs than the sample can meet a larger
fp32 error than the sample did; that, too, has to fit in the factor MARGIN,
which is why the factor is 4 and not the 2 the summation order alone needs.
"""

from __future__ import annotations

import functools
import zlib

import torch

FAMILIES = ("gauss", "lowvar", "bigmean", "slicestep", "outlier", "const")
NF = len(FAMILIES)
SAMPLE = 32          # rows per family E_ref is measured on
MARGIN = 4.0
# A family's margin where a stated property of an instruction needs more than
# 4 (never above a quarter of the smallest defect shift the CPU test proves;
# the reason stands next to the number): {(kind, family): margin}
MARGINS = {}

# widths of the with_row_per<...> lists
LN_WIDTHS = (128, 256, 384, 768, 1024)          # layernorm, layernorm_f16, layernorm32, merge_tokens
TAP_WIDTHS = (128, 256, 384, 512, 768, 1024)    # tap_concat_ln (the row is 2 D wide), rows_layernorm
EPS = (1e-6, 1e-5)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def family_of(r):
    return FAMILIES[r % NF]


def rows(m, d, f16=False, key="rows"):
    """-> float64 [m][d]; row r of family r % 6 (f16: every value an f16 value)."""
    g = gen(key, m, d)
    rn = torch.randn(m, d, generator=g, dtype=torch.float64)
    x = torch.empty(m, d, dtype=torch.float64)
    ns = max(d // 32, 1)
    step = 0.5 * (torch.arange(d) // 32 - (ns - 1) / 2.0).double()
    for f in FAMILIES:
        r = family_rows(m, f)
        if f == "gauss":
            x[r] = rn[r] * 3 + 1.5
        elif f == "lowvar":
            x[r] = rn[r] * 1e-3 * (2.0 ** (r % 4).double())[:, None]
        elif f == "bigmean":
            x[r] = 64 + rn[r] * 0.5
        elif f == "slicestep":
            x[r] = step + rn[r] * 0.25
        elif f == "outlier":
            o = rn[r]
            o[:, 7], o[:, d - 3] = 300.0, -180.0
            x[r] = o
        else:
            x[r] = 1.5
    # fp32 values at least (the device buffers are fp32 or f16)
    return (x.float().half() if f16 else x.float()).double()


def family_rows(m, fam):
    """Indices r < m with r % 6 == the family's."""
    return torch.arange(FAMILIES.index(fam), m, NF)


def affine(d, key="affine"):
    """gamma = 1 + 0.1 rn, beta = 0.02 rn: fp32 values as float64."""
    g = gen(key, d)
    gm = (1 + 0.1 * torch.randn(d, generator=g)).float().double()
    bt = (0.02 * torch.randn(d, generator=g)).float().double()
    return gm, bt


def ulp16(ref):
    """Spacing of the f16 values around ref (float64); 2^-24 in the subnormal range."""
    a = ref.double().abs()
    e = torch.frexp(a)[1] - 1
    e = torch.where(a > 0, e, torch.full_like(e, -14)).clamp(min=-14, max=15)
    return torch.ldexp(torch.ones_like(a), e - 10)


def skip_map(rows_, T):
    """Input rows the skip_cls form keeps, in output order."""
    r = torch.arange(rows_)
    return r[r % T != 0]


# ---- float64 references (defect: one wrong formula built in) ---------------------

def stats64(x, defect=None):
    """-> (mean, var) [m][1] of float64 rows."""
    d = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    if defect == "onepass32":      # E[x^2] - mean^2 in fp32
        x32 = x.float()
        m32 = x32.sum(-1, keepdim=True) / d
        v32 = (x32 * x32).sum(-1, keepdim=True) / d - m32 * m32
        return m32.double(), v32.double()
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / ((d - 1) if defect == "dminus1" else d)
    return mean, var


def rstd64(var, eps, defect=None):
    if defect == "eps0":
        eps = 0.0
    elif defect == "eps_swapped":
        eps = 1e-5 if eps < 3e-6 else 1e-6
    elif defect == "eps_outside":   # 1 / (sqrt(var) + eps)
        return 1.0 / (var.sqrt() + eps)
    return (var + eps).rsqrt()


def layernorm64(x, g, b, eps, T=1, skip_cls=False, defect=None):
    mean, var = stats64(x, defect)
    y = (x - mean) * rstd64(var, eps, defect) * g + b
    if skip_cls:
        if defect == "cls_kept":        # no row dropped: the first B (T - 1) rows
            return y[:x.shape[0] // T * (T - 1)]
        if defect == "cls_off_by_one":  # the row after the cls row dropped instead
            r = torch.arange(x.shape[0])
            return y[r[r % T != 1]]
        return y[skip_map(x.shape[0], T)]
    return y


def partials64(x, defect=None):
    """-> [d / 32][m][2]: (sum, M2 about the slice mean) per 32-column slice."""
    v = x.reshape(x.shape[0], -1, 32)
    about = 0.0 if defect == "m2_about_zero" else v.mean(-1, keepdim=True)
    m2 = ((v - about) ** 2).sum(-1)
    return torch.stack([v.sum(-1), m2], -1).transpose(0, 1).contiguous()


def merge64(part, defect=None):
    """(mean, var) [m][1] from the partials by Chan et al.'s merge:
    var = sum_s (M2_s + 32 (mean_s - mean)^2) / D."""
    ns = part.shape[0]
    s, m2 = part[..., 0], part[..., 1]           # [ns][m]
    n_used = ns - 1 if defect == "wrong_count" else ns
    mean = s[:n_used].sum(0) / (32 * ns)
    ms = s / 32
    if defect == "wrong_pairing":
        # Chan's two-set merge applied slice after slice with the accumulated
        # side's count taken as one slice's 32: M2 += M2_s + delta^2 32 32 / 64
        acc_mean, acc_m2 = ms[0], m2[0]
        for i in range(1, ns):
            delta = ms[i] - acc_mean
            acc_m2 = acc_m2 + m2[i] + delta * delta * 16
            acc_mean = (acc_mean + ms[i]) / 2
        return mean[:, None], (acc_m2 / (32 * ns))[:, None]
    between = 0.0 if defect == "no_between" else 32 * (ms - mean) ** 2
    var = (m2 + between)[:n_used].sum(0) / (32 * ns)
    return mean[:, None], var[:, None]


def fold_weights(n, k, key="fold"):
    """-> Wg16 [n][k] (f16 values), c1 = sum_k Wg16 (fp32 value), c2 (fp32 value), float64.
    The weights have a column mean of about 0.3 / sqrt k, so c1 is not small
    and mean c1 cancels against x Wg^T as in the model."""
    g = gen(key, n, k)
    gm, bt = affine(k, key)
    w = (torch.randn(n, k, generator=g, dtype=torch.float64) + 0.3) * k ** -0.5
    wg16 = (w * gm).float().half().double()
    bias = 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    c1 = wg16.sum(1).float().double()
    c2 = (bias + w.float().half().double() @ bt).float().double()
    return wg16, c1, c2


def fold64(x, wg16, c1, c2, eps, defect=None, part_defect=None, acc=None):
    """rstd (x Wg16^T - mean c1) + c2 with the statistics merged from the
    (float64) partials of x: exact, equal to stats64 when no defect is set.
    acc: x Wg16^T where the caller has it already."""
    mean, var = merge64(partials64(x, part_defect), defect)
    acc = x @ wg16.T if acc is None else acc
    return rstd64(var, eps, defect) * (acc - mean * c1) + c2


# (m, n, k) of every fold problem the GPU file runs (test_gpu_rows.py FOLD_ROUTES,
# test_qkv_lnfold, test_linear_lnfold_tok): the CPU proofs run on these very operands
FOLD_SHAPES = ((77, 96, 384), (2035, 1920, 384), (16397, 1536, 384), (77, 96, 1024), (2035, 1920, 1024),
               (100, 1152, 384), (17760, 1152, 384), (21, 64, 384))
# (m, n) of every producer matrix the GPU file runs (rows(m, n, f16))
PRODUCER_SHAPES = ((77, 96), (2035, 1920), (16129, 64), (300, 384), (1281, 1024))
# rows of the row-kernel matrices the GPU files use: 3 x 7, rows_layernorm's 3 x 9, merge_tokens' 30 and 120
LN_ROWS = (21, 27, 30, 120)


def rope_tables64(max_pos, dim=32, base=100.0):
    """The oracle's rope_tables (oracle/vggt_ref.py) in float64: [max_pos][dim]."""
    inv = 1.0 / base ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    ang = torch.cat((ang, ang), -1)
    return ang.cos(), ang.sin()


def rope2d_t(x, pos, cos, sin):
    """The oracle's rope2d on x [..., T, 64], pos [T][2], in x's dtype."""
    def r1(v, p):
        h = v.shape[-1] // 2
        return v * cos[p] + torch.cat((-v[..., h:], v[..., :h]), -1) * sin[p]
    v, hz = x.chunk(2, -1)
    return torch.cat((r1(v, pos[:, 0]), r1(hz, pos[:, 1])), -1)


def qk_rope64(x, g, b, eps, pos, cos32, sin32, scale, defect=None):
    """LayerNorm(64) -> rope2d with the fp32 tables the op is given -> * scale."""
    return rope2d_t(layernorm64(x, g, b, eps, defect=defect), pos, cos32.double(), sin32.double()) * scale


# ---- the same formulas in plain fp32 (E_ref) -----------------------------------

def _sum32(x, order):
    """fp32 sum over the last axis: torch's blocked order, or the strict index order."""
    return x.sum(-1, keepdim=True) if order == 0 else x.cumsum(-1)[..., -1:]


def layernorm32(x, g, b, eps, order=0):
    x, g, b = x.float(), g.float(), b.float()
    d = x.shape[-1]
    mean = _sum32(x, order) / d
    c = x - mean
    var = _sum32(c * c, order) / d
    return c * torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32)) * g + b


def partials32(x, order=0):
    v = x.float().reshape(x.shape[0], -1, 32)
    s = _sum32(v, order)
    c = v - s / 32
    return torch.stack([s[..., 0], _sum32(c * c, order)[..., 0]], -1).transpose(0, 1).contiguous()


def merge32(part):
    """Chan et al.'s merge in fp32, pairwise over the slices (a tree)."""
    ns = part.shape[0]
    s, m2 = part[..., 0], part[..., 1]

    def tree(t):
        t = list(t)
        while len(t) > 1:
            t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return t[0]
    mean = tree(s) / (32 * ns)
    dev = s / 32 - mean
    var = tree(m2 + 32 * dev * dev) / (32 * ns)
    return mean[:, None], var[:, None]


def fold32(x, wg16, c1, c2, eps, order=0):
    mean, var = merge32(partials32(x, order))
    acc = x.float() @ wg16.float().T
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    return rstd * (acc - mean * c1.float()) + c2.float()


def qk_rope32(x, g, b, eps, pos, cos32, sin32, scale, order=0):
    return rope2d_t(layernorm32(x, g, b, eps, order), pos, cos32, sin32) * torch.tensor(scale, dtype=torch.float32)


def _rel(got32, ref64):
    return float(((got32.double() - ref64).abs() / ref64.abs().clamp(min=1.0)).max())


@functools.lru_cache(maxsize=None)
def e_ref(kind, fam, d, eps=1e-6, f16=False, n=64):
    """E_ref of one site kind ("ln", "partials", "fold", "qkrope"), family,
    width and eps; f16: f16-valued input rows; n: the fold's output width."""
    x = rows(NF * SAMPLE, d, f16, key=("eref", kind))[family_rows(NF * SAMPLE, fam)]
    if kind == "ln":
        g, b = affine(d)
        ref = layernorm64(x, g, b, eps)
        return max(_rel(layernorm32(x, g, b, eps, o), ref) for o in (0, 1))
    if kind == "partials":
        # each cell relative to max(|its own value|, the cell's scale): see partials_bound
        ref = partials64(x)
        scale = partials_scale(x)
        return max(float(((partials32(x, o).double() - ref).abs() / scale).max()) for o in (0, 1))
    if kind == "fold":
        wg16, c1, c2 = fold_weights(n, d)
        ref = fold64(x, wg16, c1, c2, eps)
        return max(_rel(fold32(x, wg16, c1, c2, eps, o), ref) for o in (0, 1))
    if kind == "qkrope":
        g, b = affine(d)
        cos, sin = (t.float() for t in rope_tables64(9))
        pos = torch.stack([torch.arange(x.shape[0]) % 9, (torch.arange(x.shape[0]) * 4) % 9], 1)
        ref = qk_rope64(x, g, b, eps, pos, cos, sin, 0.18)
        return max(_rel(qk_rope32(x, g, b, eps, pos, cos, sin, 0.18, o), ref) for o in (0, 1))
    raise KeyError(kind)


def partials_scale(x):
    """What a slice's (sum, M2) are held relative to -- the slice's OWN sum of
    |x| and its own M2 (at least the rounding floor of 32 squared deviations,
    32 (2^-24 max|x|)^2: a const slice's M2 is 0): [d / 32][m][2]."""
    v = x.reshape(x.shape[0], -1, 32)
    sabs = v.abs().sum(-1)
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    floor = 32 * (2.0 ** -24 * v.abs().amax(-1)) ** 2
    return torch.stack([sabs, torch.maximum(m2, floor)], -1).transpose(0, 1).contiguous().clamp(min=1e-300)


def margin(kind, fam):
    return MARGINS.get((kind, fam), MARGIN)


def bound(kind, ref, m_rows, d, eps=1e-6, f16_in=False, f16_out=True, n=64, row_family=None):
    """Elementwise bound for a site's output `ref` [m][...]: row i's family is
    row_family[i] (default i % 6)."""
    fam_idx = torch.arange(m_rows) % NF if row_family is None else row_family
    e = torch.tensor([margin(kind, f) * e_ref(kind, f, d, eps, f16_in, n) for f in FAMILIES],
                     dtype=torch.float64)[fam_idx]
    b = e.reshape(-1, *([1] * (ref.dim() - 1))) * ref.abs().clamp(min=1.0)
    return b + 0.5 * ulp16(ref) if f16_out else b


def partials_bound(x, f16_in=True):
    """Bound for a producer's partials [d / 32][m][2] of the rows x: relative to
    the slice's own scale (partials_scale), per family."""
    m, d = x.shape
    e = torch.tensor([margin("partials", f) * e_ref("partials", f, d, 1e-6, f16_in) for f in FAMILIES],
                     dtype=torch.float64)[torch.arange(m) % NF]
    return e[None, :, None] * partials_scale(x)
