"""Test helper (not a test module): attention inputs with GRADED softmax
weights, their float64 reference and a per-element error bound computed from
the reference alone (test_gpu_attention.py runs them on the kernels,
test_attention_cases_cpu.py proves the claims made here on a CPU model).

exact_cases.py's selection and uniform probes pin attention.hip bit for bit,
but only at softmax weights 0, 1 and 1 / T: every rescale factor the kernels
form there is 2^0 or 0 in effect.  The families here put weight everywhere in
between, at the places where a flash-attention loop goes wrong.

Inputs.  q, k, v f16 [B H][T][64] in the op's contract: q already in log2
units (score = q . k, weight 2^score).  v is random normal.

Integer-score families.  q and k hold small integers in separate feature
ranges -- k[j] a one-hot code of its 32-key block (features 0..47), a one-hot
of j % 4 (48..51), flags for two plateaus, the last key and "every key"
(56..59); q[i] the value each code contributes -- so every score is an integer
below 2^11 in magnitude: exact in f16 operands, in the fp32 MFMA and in
float64.  Then every P = 2^(s - m_run) is a power of two, and so is every
rescale factor alpha, every merge weight a0 / ag and every combine weight w:
exact in f16 and fp32 while they are representable.  The score of key j for
query i is a block term f_i(j // 32) plus a within-block term -(j % 4), so
every block holds its own maximum at its first key -- the block and tile
positions are what the kernels' control flow sees.

Rows differ inside a wave.  The kernels vote per wave (attn_fwd_kernel: 32
queries, attn16_body: 16) whether any row's block maximum exceeds the running
one by more than RESCALE_T = 8, and then rescale EVERY row of the wave by its
own max(mx, 0).  Query groups of 32 alternate: an even group's rows all take
the family's step s (the vote is unanimous, so s = 8 really reaches P = 256
without a rescale), an odd group's rows take steps s, 3, 9, -40 in turn (rows
dragged into a rescale by a neighbour, with a delta of their own in [0, 8];
the falling row's block maximum is below its running one, which must stay).

  ramp<r>, r = 7, 8, 9   f = r b.  The running max moves only when exceeded by
        more than 8: at 9 every block rescales (delta 9); at 8 block 1 sits
        exactly at the threshold (P = 256, no rescale) and block 2 rescales by
        16, and so on alternately; at 7 P reaches 128 and every second block
        rescales by 14.
  ramp16  f = 16 ((b + phase) // 2): a step of 16 every second block, phase 0
        on a tile's block 0 (never a pending P), phase 1 on its block 1
        (always one); phase by query group, mixed in every fourth.
  down<r>, r = 1, 9   f = -r b: the max is in the first block, later keys fall
        through the normal, subnormal and flushed ranges of f16 P.
  saw<d>, d = 8, 9, 12, 25   f = d ((b + 1) // 2): in every 64-key tile block 1
        is d above block 0 -- attn16_body's pending-P path (block 0's P waits
        for its P.V while block 1 raises the max); at 25 (f16)alpha is 0.
  peaks<d>, d = 0, 1, 3, 8, 9, 13   two plateaus of equal width (the keys of
        the last block: 26, 12, 1, 1 at T = 1370, 300, 129, 65), the first
        keys and the last keys of the row, maxima d apart, over a background
        10..12 below the higher one.  The first and the last key tile lie in
        different key groups for 2, 3 and 4 groups and in different splits for
        "s2" / "s3" at every T here; at T = 300 with 4 groups the last group
        is empty.  Even (sequence, head) pairs have the higher plateau first,
        odd ones last.  Rows also carry a constant offset 0, -160, +160, -40
        (by i // 8): softmax does not see it, a merge that takes a maximum
        over something that is not a score does.
  graded  scores i.i.d. uniform integers in [-12, 0] as far as rank 64 allows:
        key j belongs to one of 64 random classes, q[i] holds an independent
        value per class.
  tail_near  the row's maximum is the last real key T - 1 (by 1..6 over every
        other key).  tail_far: key T - 1 is the ONLY key within 14 of the
        maximum (16 above the next).  The last block holds 26, 12, 1, 1 real
        keys: the masked block carries the weight.

General family (P inexact, non-power-of-two factors).  randf: scores 3 x
randn.  spiky: test_gpu_ops.py's generator (dominant keys early and late).

Reference.  float64 softmax of the exact float64 scores of the f16 operands:
w = 2^(s - max) / sum, ref = w v, S = w |v|.

Bound, per output element, from the reference only:

    bound = 1/2 ulp16(ref) + (epsP + (T / 16 + 8) 2^-24) S + flush
    flush = sum_j min(w_ij, 2^-25) |v_j|  over the keys with s_ij < max_i - 14

  * m_run never exceeds the row's final maximum (it only ever takes the value
    of a block maximum), so P = 2^(s - m_run) >= 2^(s - max): a key within 14
    of the final maximum has P >= 2^-14, a normal f16 number -- exact for the
    integer families (epsP = 0), relative error 2^-11 otherwise.  P <= 2^8 by
    the threshold, inside f16's range.
  * Below that P is subnormal: its absolute error is at most half a subnormal
    step, 2^-25, and never more than P itself (flushed); later rescales are
    powers of two below 1 applied in fp32.  The final l is at least 1 (the
    maximal key weighs 1), so after the division the error per key is at most
    min(w, 2^-25) |v|: the flush term.
  * fp32: O and l take one rounding per MFMA k-step of 16 keys (T / 16 of
    them) and a few in the rescales, the key-group merge, the split combine,
    1 / l and the product with it (the 8), each at most 2^-24 of a partial sum
    that S bounds.
  * General family: epsP = 2^-11 + 2^-18 -- the f16 rounding of P, and
    v_exp_f32 with the fp32 score's own rounding.  attn16_body (kernel mfma16)
    scales a pending P by (f16)alpha, one more f16 rounding, and rounds the f16
    product, another: 2 x 2^-11 more, taken on the whole row.  For the integer
    families both are exact (powers of two) until they flush, which the flush
    term already holds: a product below 2^-24 belongs to a key more than 14
    below the new maximum.
  * The final f16 rounding: 1/2 ulp16.

attention32 (fp32.hip, fp32 operands and output; the same families): no f16
term.  attn32_kernel accumulates O by v_mfma_f32_32x32x2_f32, one rounding
per 2 keys (T / 2), sums l over a lane's 16 keys in turn, across the lane
halves and into the running sum (17 + T / 32), computes P by v_exp_f32 (one
ulp in numerator and denominator), merges four key groups through LDS and
multiplies by 1 / l.  A score is 32 MFMA steps of 2 dims: absolute error at
most 33 x 2^-24 A_ij with A = |q| . |k|, hence a relative error ln 2 times
that in P, in numerator and denominator -- for the general families only: the
integer families' scores are exact in fp32 and their serr is 0, as epsP is:

    bound32 = (T / 2 + T / 32 + 48) 2^-24 S + 2^-22 |ref| + serr
    serr    = 2 x ln 2 x 33 x 2^-24 sum_j w_ij A_ij |v_j|   (general families)

For the integer families this lies inside the (T + 64) 2^-23 S + 2^-21 |ref|
a key-by-key fp32 sum would need (the MFMA halves the roundings); for the
general ones serr is what that form leaves out.
"""

from __future__ import annotations

import functools
import math

import torch

import exact_cases as X

LOG2E = 1.4426950408889634
F_BLK, F_IN, F_A, F_B, F_LAST, F_ALL = 0, 48, 56, 57, 58, 59
MIXED_STEPS = (None, 3, 9, -40)     # an odd query group's rows: the family's step, then these, in turn
ROW_OFFSETS = (0, -160, 160, -40)  # peaks: a constant per row, by i // 8

INTEGER_FAMILIES = (["ramp7", "ramp8", "ramp9", "ramp16", "down1", "down9", "saw8", "saw9", "saw12", "saw25"]
                    + [f"peaks{d}" for d in (0, 1, 3, 8, 9, 13)] + ["graded", "tail_near", "tail_far"])
GENERAL_FAMILIES = ["randf", "spiky"]
FAMILIES = INTEGER_FAMILIES + GENERAL_FAMILIES
# the families built to reach the rescale branch, the exact threshold and the pending-P path (CPU test)
RESCALE_FAMILIES = ["ramp7", "ramp8", "ramp9", "ramp16", "saw8", "saw9", "saw12", "saw25"]

EPS_P = 2.0 ** -11 + 2.0 ** -18
EPS_PEND = 2.0 * 2.0 ** -11


def steps(T, s):
    """Step per query: s in the even 32-query groups, s, 3, 9, -40 in turn in the odd ones."""
    i = torch.arange(T)
    mixed = torch.tensor([s if m is None else m for m in MIXED_STEPS])[i % 4]
    return torch.where((i // 32) % 2 == 0, torch.full_like(i, s), mixed)


def block_terms(family, T):
    """f_i(b) [T][blocks] (int64) of a block-term family, or None."""
    nkb = -(-T // 32)
    i, b = torch.arange(T)[:, None], torch.arange(nkb)[None, :]
    name, num = family.rstrip("0123456789"), int("0" + family[len(family.rstrip("0123456789")):])
    if family == "ramp16":
        grp = i // 32
        phase = torch.where(grp % 4 < 2, grp % 2, i % 2)
        return 16 * ((b + phase) // 2)
    if name == "ramp":
        return steps(T, num)[:, None] * b
    if name == "down":
        return -steps(T, num)[:, None] * b
    if name == "saw":
        return steps(T, num)[:, None] * ((b + 1) // 2)
    if name == "peaks":
        return -10 - (i + b) % 3
    if name == "tail_near" or name == "tail_far":
        return -1 - (i + b) % 6
    return None


def integer_qk(family, B, H, T):
    """q, k [B H][T][64] float64 holding integers (see the module docstring)."""
    nkb = -(-T // 32)
    assert nkb <= F_IN - F_BLK
    j = torch.arange(T)
    q = torch.zeros(B * H, T, 64, dtype=torch.float64)
    k = torch.zeros(B * H, T, 64, dtype=torch.float64)
    if family == "graded":
        for bh in range(B * H):
            g = X.gen("graded", B, H, T, bh)
            k[bh, j, torch.randint(0, 64, (T,), generator=g)] = 1.0
            q[bh] = -torch.randint(0, 13, (T, 64), generator=g).double()
        return q, k
    k[:, j, F_BLK + j // 32] = 1.0
    k[:, j, F_IN + j % 4] = 1.0
    q[:, :, F_IN:F_IN + 4] = -torch.arange(4).double()
    for bh in range(B * H):
        f = block_terms(family, T)
        q[bh, :, F_BLK:F_BLK + nkb] = f.double()
        if family.startswith("peaks"):
            d, w = int(family[5:]), T - 32 * (nkb - 1)
            top_a, top_b = (0, -d) if bh % 2 == 0 else (-d, 0)
            k[bh, :w, F_A] = 1.0
            k[bh, T - w:, F_B] = 1.0
            k[bh, :, F_ALL] = 1.0
            q[bh, :, F_A] = (top_a - f[:, 0]).double()
            q[bh, :, F_B] = (top_b - f[:, nkb - 1]).double()
            q[bh, :, F_ALL] = torch.tensor(ROW_OFFSETS)[(torch.arange(T) // 8) % 4].double()
        if family.startswith("tail"):
            k[bh, T - 1, F_LAST] = 1.0
            lift = 0 if family == "tail_near" else 16
            q[bh, :, F_LAST] = (lift - (f[:, nkb - 1] - (T - 1) % 4)).double()
    return q, k


def general_qk(family, B, H, T):
    g = X.gen(family, B, H, T)
    if family == "randf":
        c = math.sqrt(3.0 / 8.0)   # 64 products of variance c^4: a score of standard deviation 3
        return torch.randn(B * H, T, 64, generator=g) * c, torch.randn(B * H, T, 64, generator=g) * c
    assert family == "spiky" and T > 10
    q = torch.randn(B * H, T, 64, generator=g) * 0.125 * 2.0 * LOG2E
    k = torch.randn(B * H, T, 64, generator=g) * 2.0
    k[:, T - 10] = q.mean(1) * 60.0
    k[:, 3] = q.mean(1) * 30.0
    return q, k


def op_layout(x, B, H, T):
    """[B H][T][64] -> the op's [B T][H 64]."""
    return x.reshape(B, H, T, 64).permute(0, 2, 1, 3).reshape(B * T, H * 64).contiguous()


class Case:
    """One (family, B, H, T): the f16 operands, the float64 reference and the
    parts of the bounds, all outputs in the op's [B T][H 64] layout."""

    def __init__(self, family, B, H, T):
        self.family, self.B, self.H, self.T = family, B, H, T
        self.integer = family in INTEGER_FAMILIES
        q, k = integer_qk(family, B, H, T) if self.integer else general_qk(family, B, H, T)
        self.q, self.k = q.half(), k.half()
        self.v = torch.randn(B * H, T, 64, generator=X.gen("v", family, B, H, T)).half()
        if self.integer:
            assert torch.equal(self.q.double(), q) and torch.equal(self.k.double(), k)
        qd, kd, vd = self.q.double(), self.k.double(), self.v.double()
        s = qd @ kd.transpose(1, 2)
        mx = s.amax(-1, keepdim=True)
        p = torch.exp2(s - mx)
        w = p / p.sum(-1, keepdim=True)
        av = vd.abs()
        self.ref = op_layout(w @ vd, B, H, T)
        self.S = op_layout(w @ av, B, H, T)
        self.flush = op_layout((torch.minimum(w, torch.tensor(2.0 ** -25, dtype=torch.float64)) * (s < mx - 14)) @ av,
                               B, H, T)
        self.serr = torch.zeros_like(self.ref) if self.integer else op_layout(
            (w * (qd.abs() @ kd.abs().transpose(1, 2))) @ av, B, H, T) * (2.0 * math.log(2.0) * 33.0 * 2.0 ** -24)

    def scores64(self):
        return self.q.double() @ self.k.double().transpose(1, 2)

    def bound(self, kernel):
        """The f16 op's bound; kernel "mfma32" or "mfma16" (the pending-P term)."""
        eps = 0.0 if self.integer else EPS_P + (EPS_PEND if kernel == "mfma16" else 0.0)
        return 0.5 * X.ulp16(self.ref) + (eps + (self.T / 16 + 8) * 2.0 ** -24) * self.S + self.flush

    def bound32(self):
        return ((self.T / 2 + self.T / 32 + 48) * 2.0 ** -24 * self.S + 2.0 ** -22 * self.ref.abs() + self.serr)


@functools.lru_cache(maxsize=None)
def case(family, B, H, T):
    return Case(family, B, H, T)


# ---- which launches must agree bit for bit ----------------------------------------

def tail2_rows(T):
    """Queries the 8-wave mfma16 kernel runs as two key groups at "attn_tail" =
    2: a partial last 256-query block of at most 128 queries, two key tiles up."""
    first = (-(-T // 256) - 1) * 256
    return first if T - first <= 128 and T > 64 else T


def order_key(route, T):
    """Launches with equal keys sum every output in the same order: the MFMA
    shape, the key groups (their tile ranges follow from the count), the key
    splits; waves, ring depth and query sub-tiles only move queries between
    waves.  The 8-wave mfma16 kernel at tail = 2 regroups its last rows."""
    regroup = (route["kernel"] == "mfma16" and route["nw"] == 8 and route["groups"] == 1 and route["tail"] == 2
               and tail2_rows(T) < T)
    return (route["kernel"], route["groups"], route["split"], route["tiles"], regroup)
