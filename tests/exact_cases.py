"""Test helper (not a test module): operands for which the kernels' fp32
arithmetic is EXACT, and float64 references of the same operations.

Dyadic operands (linear / conv families).  a = ia / 4, w = iw / 64 with
integer ia, iw in [-R, R]; bias = ib / 256, |ib| <= 256; f16 residuals and the
residual streams on the 1 / 256 grid with |r| <= 8; LayerScale from {0.25,
0.5, 1}.  Every operand is an f16 value, every product a multiple of 2^-8 and
every partial sum, in any order, at most K R^2 of those quanta -- below 2^22
for every case here -- so fp32 accumulation, split-K partial sums, acc + b
and x + ls (acc + b) are exact with or without contraction, whatever the tile
shape, K order, split or wave count.  The float64 result rounded once to f16
(not at all for the fp32 outputs) is then the only correct output.

R is chosen per reduction length (int_range): the sum's standard deviation is
held near SIGMA_Q quanta (2^13.5: about 47), so that a large share of the
outputs needs a real f16 rounding and a good part of those are exact ties.
At K = 4096 this gives R = 16, the grid a = ia / 4, w = iw / 64 over [-16, 16].

GELU sweep.  Selector weights pick one A element per output, so the
accumulator is exactly that element and the epilogue sees x = fl32(a + b);
A holds every finite f16 value (sweep_*), bias one of 8 values k / 4096.

Attention.  A selection probe (one key beats every other by 40 in the log2
units of attention.hip: the output row IS one row of V) and a uniform probe
(q = 0, constant V columns: the output IS that constant; a leaked pad key
scales it by T / (T + 1), which is another f16 value for T <= 2047).
"""

from __future__ import annotations

import functools
import math
import re
import zlib

import numpy as np
import torch
import torch.nn.functional as F

SIGMA_Q = 2.0 ** 13.5   # target standard deviation of an accumulator, in quanta of 2^-8
QUANTUM = 2.0 ** -8


def gen(*key):
    """A generator seeded by the problem."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def int_range(k, relu_in=False):
    """R for a reduction over k products: ia, iw uniform on [-R, R] have
    variance ~ R^2 / 3, a product R^4 / 9 (half of it behind a ReLU on a), the
    sum k times that -- solved for a standard deviation of SIGMA_Q."""
    per = SIGMA_Q / math.sqrt(k) * (math.sqrt(2.0) if relu_in else 1.0)
    return max(4, min(128, int(round(math.sqrt(3.0 * per)))))


def ints(g, shape, r):
    return torch.randint(-r, r + 1, shape, generator=g).double()


def stats16(ref):
    """(share of ref's elements that are not f16 values, share that lie
    exactly half way between two f16 values, max |ref|)."""
    r = ref.double().flatten()
    h = r.float().half().double()      # ref is exact in fp32: one rounding
    inexact = h != r
    # a tie: the two neighbours are equally far -- ref +- its error are both f16 values
    other = (2.0 * r - h)
    tie = inexact & (other.float().half().double() == other) & ((other - r).abs() == (h - r).abs())
    return float(inexact.double().mean()), float(tie.double().mean()), float(r.abs().max())


def shuffled_f32(a, w, key, chunks=7):
    """a [m][k] w[n][k]^T in float32: K permuted, cut into uneven chunks,
    each chunk a float32 matmul, the chunk results added in float32."""
    g = gen("shuffle", key)
    k = a.shape[-1]
    perm = torch.randperm(k, generator=g)
    cuts = sorted(set(torch.randint(1, k, (chunks - 1,), generator=g).tolist())) if k > 1 else []
    a32, w32 = a.float(), w.float()
    out = None
    for lo, hi in zip([0] + cuts, cuts + [k]):
        idx = perm[lo:hi]
        part = a32[..., idx] @ w32[..., idx].transpose(-1, -2)
        out = part if out is None else out + part
    return out


# ---- linear family --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lin_case(m, n, k, tag="lin"):
    """-> a [m][k], w [n][k], bias [n], acc = a w^T (no bias), all float64 (a, w f16 values)."""
    g = gen(tag, m, n, k)
    r = int_range(k)
    a, w = ints(g, (m, k), r) / 4, ints(g, (n, k), r) / 64
    b = ints(g, (n,), 256) / 256
    return a, w, b, a @ w.T


def resid16(g, shape):
    """f16 residual on the 1 / 256 grid, |r| <= 8."""
    return (ints(g, shape, 2048) / 256).half()


def layerscale(g, n):
    return torch.tensor([0.25, 0.5, 1.0])[torch.randint(0, 3, (n,), generator=g)].float()


def act64(x, act):
    return F.relu(x) if act == 1 else x


# (route, m, n, k, switches, the fields of _lib.last_gemm_route() a dense E_STORE launch must show)
LINEAR_ROUTES = [
    ("t64", 77, 96, 40, {}, dict(kind="tile", bm=64, bn=64)),
    ("t128_bk32", 2035, 1920, 72, {}, dict(kind="tile", bm=128, bn=128, wm=2, wn=2, bk=32)),
    ("t128_w8", 2035, 1920, 1032, {"w8small": 1}, dict(kind="tile", bm=128, bn=128, wm=2, wn=4, bk=64)),
    ("t128_w4", 2035, 1920, 1032, {"w8small": 0}, dict(kind="tile", bm=128, bn=128, wm=2, wn=2, bk=64)),
    ("gemm256", 300, 264, 72, {"gemm256": 2}, dict(kind="gemm256")),
    ("panel", 16129, 64, 384, {}, dict(kind="panel")),
]
SPLIT_SHAPE = (361, 1024, 1024)   # mde_op_linear_ws: split_store, and tile with splitk = 0

# the same shapes through the other epilogues: the route each takes (gemm.hip pick_tile / gemm_route)
RESID32_ROUTES = [   # E_RESID over the fp32 stream
    ("t64", 77, 96, 40, {}, dict(kind="tile", bm=64, bn=64)),
    ("t128x64", 2035, 1920, 72, {}, dict(kind="tile", bm=128, bn=64, wm=4, wn=1)),
    ("t128", 2035, 1920, 1032, {}, dict(kind="tile", bm=128, bn=128, wm=2, wn=2, bk=64)),
    ("gemm256", 300, 264, 72, {"gemm256": 2}, dict(kind="gemm256")),
    ("narrow", 16129, 64, 384, {}, dict(kind="tile", bm=32, bn=64)),
]
RESID16_ROUTES = RESID32_ROUTES + [   # E_RESID over the f16 stream: the panel kernel at "panel" = 2
    ("panel", 16129, 64, 384, {"panel": 2}, dict(kind="panel")),
]
RES_ROUTES = [   # E_STORE with res0 / res1: no panel kernel (N = 64 takes the 64^2 tiles)
    ("t64", 77, 96, 40, {}, dict(kind="tile", bm=64, bn=64)),
    ("t128_bk32", 2035, 1920, 72, {}, dict(kind="tile", bm=128, bn=128, wm=2, wn=2, bk=32)),
    ("t128_w8", 2035, 1920, 1032, {"w8small": 1}, dict(kind="tile", bm=128, bn=128, wm=2, wn=4, bk=64)),
    ("gemm256", 300, 264, 72, {"gemm256": 2}, dict(kind="gemm256")),
    ("n64", 16129, 64, 384, {}, dict(kind="tile", bm=64, bn=64)),
]
# E_RESID split-K (mde_op_linear_residual_split, splitk = 4): 64^2 slices and the 128^2 x 4 slices
RESID_SPLIT_ROUTES = [
    ("t64", 300, 384, 1536, {}, dict(kind="split_resid", bm=64, bn=64)),
    ("t128", 1281, 1024, 1024, {}, dict(kind="split_resid", bm=128, bn=128, slices=4)),
]
LINEAR32_SHAPES = [(77, 96, 40), (1370, 384, 1536)]
QKV_SHAPES = [(2, 50, 6), (3, 1371, 6), (100, 37, 6)]


def linear_shapes():
    """Every (m, n, k) of the linear family the GPU file runs."""
    s = {c[1:4] for c in LINEAR_ROUTES + RESID16_ROUTES + RES_ROUTES + RESID_SPLIT_ROUTES}
    s |= {SPLIT_SHAPE} | set(LINEAR32_SHAPES) | {(b * t, 3 * 64 * h, 64 * h) for b, t, h in QKV_SHAPES}
    return sorted(s)


# ---- conv family ----------------------------------------------------------------

# (B, h, w, cin, cout, stride, relu_in, act, nres, workspace, switches, route kind): the direct conv, the
# implicit-GEMM 64^2 tiles (stride 2; wide K on a map that fills the 8 x 16 tiles badly) or their split-K
CONV_CASES = [
    (2, 19, 19, 64, 64, 1, 1, 1, 0, 0, {}, "conv_direct"),
    (2, 19, 19, 64, 64, 1, 0, 0, 2, 0, {}, "conv_direct"),
    (2, 19, 19, 64, 64, 2, 0, 0, 0, 0, {}, "tile"),
    (1, 37, 37, 384, 384, 2, 0, 0, 0, 0, {}, "tile"),
    (2, 30, 45, 32, 32, 1, 1, 1, 0, 0, {}, "conv_direct"),
    (2, 30, 45, 32, 32, 1, 0, 0, 2, 0, {}, "conv_direct"),
    (1, 7, 7, 256, 256, 2, 0, 0, 0, 0, {}, "tile"),
    (1, 19, 19, 1024, 256, 1, 0, 0, 0, 1, {}, "split_store"),
    (1, 19, 19, 1024, 256, 1, 0, 0, 0, 1, {"splitk": 0}, "tile"),
    (1, 75, 75, 128, 128, 1, 1, 1, 0, 0, {"conv_narrow": 1}, "conv_direct"),
    (1, 75, 75, 128, 128, 1, 1, 1, 0, 0, {"conv_narrow": 0}, "conv_direct"),
]
CONV32_CASES = [(2, 19, 19, 64, 64, 1, 0, 0, 2), (2, 20, 22, 48, 64, 1, 1, 1, 0), (1, 37, 37, 384, 384, 2, 0, 0, 0)]
CONVT_CASES = [(4, 48, 2, 7, 9), (2, 96, 2, 7, 9)]   # (s, cin = cout, B, h, w)


@functools.lru_cache(maxsize=None)
def conv_case(B, h, w, cin, cout, stride, relu_in):
    """-> x [B][cin][h][w], wt [cout][cin][3][3], bias, conv (no bias), all float64 (x, wt f16 values)."""
    g = gen("conv", B, h, w, cin, cout, stride, relu_in)
    r = int_range(9 * cin, relu_in)
    x, wt = ints(g, (B, cin, h, w), r) / 4, ints(g, (cout, cin, 3, 3), r) / 64
    b = ints(g, (cout,), 256) / 256
    acc = F.conv2d(F.relu(x) if relu_in else x, wt, None, stride=stride, padding=1)
    return x, wt, b, acc


def conv_ref(case, act, nres):
    """-> (float64 reference NCHW, the f16 residuals NCHW)."""
    x, wt, b, acc = conv_case(*case)
    g = gen("convres", case, nres)
    res = [resid16(g, tuple(acc.shape)) for _ in range(nres)]
    ref = act64(acc + b.view(1, -1, 1, 1), act)
    for r in res:
        ref = ref + r.double()
    return ref, res


def conv_shuffled_f32(case):
    """The conv as im2col in float32, K shuffled and chunked (shuffled_f32)."""
    x, wt, b, acc = conv_case(*case)
    stride, relu_in = case[5], case[6]
    cols = F.unfold((F.relu(x) if relu_in else x).float(), 3, padding=1, stride=stride)   # [B][cin 9][L]
    out = shuffled_f32(cols.transpose(1, 2), wt.reshape(wt.shape[0], -1), case)            # [B][L][cout]
    return out.transpose(1, 2).reshape(acc.shape)


@functools.lru_cache(maxsize=None)
def convt_case(s, cin, B, h, w):
    """-> x [B][cin][h][w], wt [cin][cout][s][s], bias, ConvTranspose (with bias), all float64."""
    g = gen("convt", s, cin, B, h, w)
    r = int_range(cin)
    x, wt = ints(g, (B, cin, h, w), r) / 4, ints(g, (cin, cin, s, s), r) / 64
    b = ints(g, (cin,), 256) / 256
    return x, wt, b, F.conv_transpose2d(x, wt, b, stride=s)


@functools.lru_cache(maxsize=None)
def patch_case(B, H, W, D=384):
    """-> img, w [D][3][14][14], bias, pos [ph pw][D], cls_pos [D], x [B (ph pw + 1)][D], all float64."""
    g = gen("patch", B, H, W, D)
    r = int_range(588)
    ph, pw = H // 14, W // 14
    img, w = ints(g, (B, 3, H, W), r) / 4, ints(g, (D, 3, 14, 14), r) / 64
    b, pos, cls_pos = ints(g, (D,), 256) / 256, ints(g, (ph * pw, D), 2048) / 256, ints(g, (D,), 2048) / 256
    t = F.conv2d(img[..., :ph * 14, :pw * 14], w, b, stride=14).flatten(2).transpose(1, 2) + pos
    x = torch.cat([cls_pos.expand(B, 1, D), t], 1).reshape(B * (ph * pw + 1), D)
    return img, w, b, pos, cls_pos, x


# ---- GELU -----------------------------------------------------------------------

def finite_f16():
    """Every finite f16 value, by bit pattern: +0 .. 65504, then -0 .. -65504 (63488 values)."""
    bits = np.concatenate([np.arange(0x0000, 0x7C00), np.arange(0x8000, 0xFC00)]).astype(np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16)


NSEQ = 63488
GELU_BIAS = torch.tensor([0, 1, -3, 37, -170, 341, -512, 512], dtype=torch.float64) / 4096   # |b| <= 1 / 8


def sweep_index(m, n, k):
    """Which (value, bias class) each output of the sweep sees: column j
    selects A[i][j % sel], sel = min(n, k), which holds value (i sel + j % sel)
    % NSEQ; its bias class is (j // sel + j) % 8.  -> (value index [m][n], class [n])."""
    sel = min(n, k)
    j = torch.arange(n)
    idx = (torch.arange(m)[:, None] * sel + (j % sel)[None, :]) % NSEQ
    return idx, (j // sel + j) % 8


def sweep_operands(m, n, k):
    """-> A [m][k] f16 (every finite f16 value in its first sel columns, row
    after row; finite filler behind them, which the selector multiplies by
    zero), W [n][k] f16 selector, bias [n] fp32."""
    assert m * min(n, k) >= NSEQ, "the sweep must hold every finite f16 value"
    sel = min(n, k)
    seq = finite_f16()
    a = seq[(torch.arange(m)[:, None] * sel + torch.arange(k)[None, :]) % NSEQ].contiguous()
    w = torch.zeros(n, k, dtype=torch.float16)
    j = torch.arange(n)
    w[j, j % sel] = 1.0
    return a, w, GELU_BIAS[sweep_index(m, n, k)[1]].float()


def sweep_x(idx, cls):
    """x = fl32(a + b) of the outputs (value index, bias class), as the epilogue forms it."""
    return finite_f16().float()[idx] + GELU_BIAS.float()[cls]


# the sweep's shape per epilogue site: (site, m, n, k, switches, route fields)
GELU_SITES = [
    ("t128_bk32", 2035, 1920, 72, {}, dict(kind="tile", bm=128, bn=128, bk=32)),
    ("t128_bk64", 2035, 1920, 1032, {}, dict(kind="tile", bm=128, bn=128, bk=64)),
    ("gemm256", 900, 264, 72, {"gemm256": 2}, dict(kind="gemm256")),
    ("panel", 16129, 64, 384, {"panel32": 0}, dict(kind="panel")),      # the hand-unrolled copy (epi_pair)
    ("panel32", 16129, 64, 384, {"panel32": 1}, dict(kind="panel")),    # panel32_kernel's gelu_erf2
    ("split_store", 361, 1024, 1024, {}, dict(kind="split_store", bm=64, bn=64)),   # elementwise.hip
]
GELU_TABLE_SHAPE = (7936, 64, 8)    # the 64^2-tile site: every (value, class) pair exactly once
GELU32_SHAPE = (1588, 96, 40)       # mde_op_linear32 (erff)
GELU_CONV = (1, 31, 32, 64)         # B, h, w, channels: 31 x 32 x 64 = NSEQ
GELU_UPCONV = (8, 8, 31, 32)        # conv3x3_up at ratio 1: 8 rows, a map upconv_kernel takes (<= 12 source rows)


def gelu64(x):
    """0.5 x (1 + erf(x / sqrt 2)) in float64, the 1 + erf as erfc (no cancellation for x << 0)."""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def ulp16(ref):
    """Spacing of the f16 values around ref (float64); 2^-24 in the subnormal range."""
    a = ref.double().abs()
    e = torch.frexp(a)[1] - 1
    e = torch.where(a > 0, e, torch.full_like(e, -14)).clamp(min=-14, max=15)
    return torch.ldexp(torch.ones_like(a), e - 10)


def gelu_bound(ref, hw_margin=True):
    """0.5 ulp16(ref) + 2.6e-5 (the bound mde_device.h documents) + 2^-20 |ref|
    (one ulp each for the hardware's v_exp_f32 and v_rcp_f32)."""
    b = 0.5 * ulp16(ref) + 2.6e-5
    return b + 2.0 ** -20 * ref.abs() if hw_margin else b


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gelu_erf_emulated(x):
    """mde_device.h gelu_erf restated in float32, one rounding per operation,
    the fmas as written, exp2 and the reciprocal correctly rounded."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    xc = np.clip(x, f(-8.0), f(8.0))
    x2 = xc * xc
    t = _fma32(_fma32(np.full_like(x, f(0.001014263055)), x2, np.full_like(x, f(-0.106775724))), x2,
               np.full_like(x, f(-2.301121339)))
    z = xc * t
    d = f(1.0) + np.exp2(z.astype(np.float64)).astype(f)
    r = (1.0 / d.astype(np.float64)).astype(f)
    return x * r


# ---- attention ------------------------------------------------------------------

ATTN_SHAPES = [(1, 2, 1370), (2, 3, 300), (2, 3, 129), (3, 1, 65)]   # (B, H, T); (1, 1, 1) for the uniform probe
ATTN_CFGS = "4g2 8g2 4g4 8g4 12g3 16g4 6g2 8g2m 8g4m 8 4 8q2 4q2 8r3 4r4 4s2 4s3 8m 4m".split()
# (name, cfg or None for the policy, "attn_tail" or None for its default): every launch shape the suite forces
ATTN_LAUNCHES = ([("policy", None, None), ("ws", None, None)] + [(c, c, None) for c in ATTN_CFGS]
                 + [(f"8m_tail{t}", "8m", t) for t in (0, 1, 2)])


# What mde_op_attention / _ws launch at the shapes above, from the promises of
# launch_attention's comment block: 256-query workgroups of 8 waves once
# ceil(T / 256) B H >= 512, else 128-query groups of 4 waves; below 256 such
# groups the keys split while each split keeps 7 key tiles (T = 1370: 22
# tiles, 3 splits; T <= 300: under 14 tiles, none); a 3-way split whose
# 64-query grid fits the CUs (44 <= 256) runs as four key groups in one
# 8-wave workgroup.  The "attn16" switch covers the unsplit 8-wave shape only.
ATTN_POLICY = {
    (1, 2, 1370): dict(kernel="mfma32", nw=8, groups=4, split=1, ring=2, qs=1, tail=0, nqb=22, nkt=22),
    (2, 3, 300): dict(kernel="mfma32", nw=4, groups=1, split=1, ring=2, qs=1, tail=0, nqb=3, nkt=5),
    (2, 3, 129): dict(kernel="mfma32", nw=4, groups=1, split=1, ring=2, qs=1, tail=0, nqb=2, nkt=3),
    (3, 1, 65): dict(kernel="mfma32", nw=4, groups=1, split=1, ring=2, qs=1, tail=0, nqb=1, nkt=2),
    (1, 1, 1): dict(kernel="mfma32", nw=4, groups=1, split=1, ring=2, qs=1, tail=0, nqb=1, nkt=1),
}
ATTN_TAIL_DEFAULT = 2   # the library's "attn_tail" (include/mde.h)


def attention_route_expected(cfg, tail, B, H, T):
    """What _lib.last_attention_route() must show after a launch of cfg (None:
    the policy) at (B, H, T), by the contract of the cfg string (mde.h
    mde_op_attention_cfg, mde_ops.h): "<waves>[s<split>][g<groups>][r<ring>]
    [q2][m]".
      g<n>: n key groups of waves / n query waves, each at least one 64-key
        tile -- with fewer tiles than groups the ungrouped 32x32x16 kernel
        runs instead (8 waves for "8...", else 4), "m" or not.
      m: the 16x16x32 kernel, handed the "attn_tail" switch.
      s<n>: ceil(tiles / n) key tiles per split, hence S = ceil(tiles / that)
        non-empty splits (the workspace of mde_op_attention_ws_bytes holds 8);
        S = 1 launches unsplit, without the combine kernel.
      r<n>: ring depth 3 or 4 (else 2); q2: two 32-query sub-tiles per wave.
    nqb = ceil(T / (32 x query waves x sub-tiles))."""
    if cfg is None:
        return dict(ATTN_POLICY[(B, H, T)])
    nkt = -(-T // 64)
    f = re.fullmatch(r"(\d+)(?:s(\d+))?(?:g(\d+))?(?:r(\d+))?(q2)?(m)?", cfg)
    assert f, cfg
    nw, split, groups, ring = int(f[1]), int(f[2] or 1), int(f[3] or 1), int(f[4] or 2)
    qs, m16 = 2 if f[5] else 1, bool(f[6])
    want = dict(kernel="mfma16" if m16 else "mfma32", nw=nw, groups=groups, split=1, ring=ring, qs=qs, tail=0, nkt=nkt)
    if groups > 1 and nkt < groups:    # the fallback: ungrouped, 32x32x16
        want.update(kernel="mfma32", nw=8 if nw == 8 else 4, groups=1)
    elif m16:
        want["tail"] = ATTN_TAIL_DEFAULT if tail is None else tail
    if split > 1:
        per = -(-nkt // split)
        want["split"] = -(-nkt // per)
        if want["split"] > 1:
            want["tiles"] = per
    want["nqb"] = -(-T // (32 * (want["nw"] // want["groups"]) * qs))
    return want


def coprime_mult(T):
    """A multiplier coprime to T: 577 (mod T) or the next one that is."""
    m = max(577 % T, 2)
    while math.gcd(m, T) != 1:
        m += 1
    return m


def selection_perm(T, head, inverse):
    """pi(i) = (mult i + 123 + 17 head) mod T, or its inverse permutation."""
    pi = (coprime_mult(T) * torch.arange(T) + 123 + 17 * head) % T
    return torch.argsort(pi) if inverse else pi


def selection_case(B, H, T, inverse):
    """-> q, k, v [B H][T][64] (f16) and pi [B H][T]: k[j] carries the +-1
    binary code of j in its first ceil(log2 T) features, q[i] 20 x the code of
    pi(i): key pi(i) scores 20 nbits, every other key at least 40 less."""
    nb = max(1, math.ceil(math.log2(T)))
    bit = torch.arange(nb)
    code = (((torch.arange(T)[:, None] >> bit[None, :]) & 1) * 2 - 1).float()   # [T][nb]
    pis = torch.stack([selection_perm(T, bh % H, inverse) for bh in range(B * H)])
    q = torch.zeros(B * H, T, 64)
    k = torch.zeros(B * H, T, 64)
    k[:, :, :nb] = code
    q[:, :, :nb] = 20.0 * code[pis]
    v = torch.randn(B * H, T, 64, generator=gen("sel", B, H, T, inverse))
    return q.half(), k.half(), v.half(), pis


def selection_expected(v, pis, B, H, T):
    """v[bh][pi(i)] in the op's [B T][H 64] layout."""
    o = torch.gather(v, 1, pis[:, :, None].expand(-1, -1, 64))
    return o.reshape(B, H, T, 64).permute(0, 2, 1, 3).reshape(B * T, H * 64)


def uniform_values(head):
    """64 distinct f16 values in [0.25, 4) of both signs, mantissas spread over
    all 10 bits; column 0 is 1.0 and column 1 is 1 - 2^-11."""
    c = np.arange(64)
    mant = (c * 977 + 131 * head + 1) % 1024
    bits = ((c & 1) << 15) | ((13 + (c >> 1) % 4) << 10) | mant
    bits[0], bits[1] = 0x3C00, 0x3BFF
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(torch.float16)


def uniform_case(B, H, T):
    """-> q = 0, k = randn, v [B H][T][64] with constant columns, expected [B T][H 64]."""
    q = torch.zeros(B * H, T, 64, dtype=torch.float16)
    k = torch.randn(B * H, T, 64, generator=gen("uni", B, H, T)).half()
    val = torch.stack([uniform_values(bh % H) for bh in range(B * H)])                  # [B H][64]
    v = val[:, None, :].expand(-1, T, -1).contiguous()
    exp = val.reshape(B, 1, H * 64).expand(-1, T, -1).reshape(B * T, H * 64).contiguous()
    return q, k, v, exp


def attention_emulated(q, k, v):
    """The kernels' arithmetic in fp32: scores in log2 units, P = 2^(s - max)
    rounded to f16 for the P V product, the row sum l kept in fp32, O / l
    rounded to f16."""
    s = q.float() @ k.float().transpose(1, 2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    return ((p.half().float() @ v.float()) / l).half()


def attention64(q, k, v):
    """The softmax of the log2-unit scores and P V in float64 -> [B H][T][64]."""
    s = q.double() @ k.double().transpose(1, 2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return (p @ v.double()) / p.sum(-1, keepdim=True)
