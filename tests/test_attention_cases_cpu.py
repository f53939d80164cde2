"""attention_cases.py proven on the CPU: a numpy model of attention.hip's two
block loops stays inside the bound on every (family, shape) the GPU file
runs, the integer families' scores are integers, the rescale families reach
the rows they were built for, and the bound is tight enough that each of nine
defects built into the model breaks it by a factor of 4 or more.

The model (model_range, model) restates the kernels operation for operation in
float32 / float16 where the kernels round:
  * 32-key blocks, two per 64-key tile, keys >= T at -inf;
  * the first block of a key range sets m_run to its row maximum; later
    blocks vote per wave (32 queries for attn_fwd_kernel, 16 for
    attn16_body) on mx > RESCALE_T and then every row of the wave takes
    delta = max(mx, 0): m_run += delta, O and l *= 2^-delta;
  * P = f16(exp2(S')); attn_fwd_kernel sums l from the fp32 p per lane half
    (two chains of 8, the halves added at the end) and accumulates O in two
    k-steps of 16 keys; attn16_body sums l from the f16 P (the all-ones MFMA)
    and accumulates O one 32-key MFMA at a time, and it computes block 1's
    scores and rescale BEFORE block 0's P.V, scaling the pending f16 P by
    (f16)alpha in f16;
  * key groups: ceil(tiles / groups) tiles each, merged on group 0 with
    a0 = 2^(m_0 - mmax), ag = 2^(m_g - mmax), an empty last group skipped;
  * key splits: (O, m, l) per split, attn_combine_kernel's w = 2^(m_s - m);
  * "attn_tail" = 2: the 8-wave mfma16 kernel's partial last query block as
    two key groups (attention_cases.tail2_rows);
  * O / l through fp32 1 / l, rounded to f16.
exp2 and the MFMA's inner sum are taken correctly rounded (float64, one
rounding): what the hardware adds to that is what the bound's 2^-18 and + 8
are for, and test_gpu_attention.py measures it.

Measured here (max err / bound over every (sequence, head) pair of each case,
test_model_within_bound prints each with -s): 0.875..0.998 on the integer
families, where the bound is 1.0 to 1.3 half-ulps of the result; randf
0.725..0.841 (mfma32) and 0.239..0.287 (mfma16), spiky 0.701..0.930 and
0.275..0.364.  These are the figures the kernels themselves give on an MI355X
in 83 of the 84 cases to the three digits printed; graded at T = 1370 differs
in the last (0.938 here, 0.939 there, mfma32).

Which family catches which defect (test_defect_moves_result: the defect moves
some output of that family by >= 4 bounds at T = 300, on the route DEFECTS lists):
  l not rescaled             ramp9   (mfma32)
  O not rescaled             ramp9   (mfma16)
  pending P not scaled       saw9    (mfma16)
  merge weight e^x           peaks3  (mfma32, 2 key groups)
  merge weight, wrong sign   peaks3  (mfma16, 2 key groups)
  mmax over an empty group   peaks0  (T = 300, 4 groups; the rows at offset -160)
  combine: m of another split  peaks8  (splits)
  threshold 16               ramp16  (P = 2^16 is inf in f16)
  fmaxf(mx, 0) dropped       ramp9   (the mixed waves' falling rows: m_run falls, O and l overflow)
"""

import numpy as np
import pytest
import torch

import attention_cases as A
import exact_cases as X

F32, F16 = np.float32, np.float16


def exp2f(x):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(np.asarray(x, dtype=np.float64)).astype(F32)


def to16(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(x, dtype=F32).astype(F16)


# lane half hh of attn_fwd_kernel holds keys (r & 3) + 8 (r >> 2) + 4 hh of a block, r = 0..15
HALF_KEYS = [[(r & 3) + 8 * (r >> 2) + 4 * hh for r in range(16)] for hh in (0, 1)]


class Stats:
    def __init__(self):
        self.rescaled = self.at_threshold = self.pending = 0


def model_range(s32, vpad, T, kt0, kt1, kernel, defects, st):
    """One wave group's pass over key tiles [kt0, kt1) for all T queries ->
    (m [T], l [T], O [T][64]), unnormalised, as the kernel holds them after
    its loop (l with the lane halves added).  An empty range: (0, 0, 0)."""
    wave = 32 if kernel == "mfma32" else 16
    thr = F32(16.0 if "threshold16" in defects else 8.0)
    m = np.zeros(T, F32)
    acc = np.zeros((T, 64), F32)
    l = np.zeros((T, 2), F32)   # mfma32: per lane half; mfma16: column 0

    def vote(mx):
        t = np.zeros(-(-T // wave) * wave, bool)
        t[:T] = mx > thr
        return np.repeat(t.reshape(-1, wave).any(1), wave)[:T]

    def scores(kt, blk):
        k0 = kt * 64 + blk * 32
        sc = np.full((T, 32), -np.inf, F32)
        n = max(0, min(32, T - k0))
        sc[:, :n] = (s32[:, k0:k0 + n] - m[:, None]).astype(F32)
        return sc

    def rescale(sc, first, pend):
        nonlocal m, acc, l
        mx = sc.max(1)
        if first:
            delta = mx
            trig = np.ones(T, bool)
        else:
            trig = vote(mx)
            st.rescaled += int((trig & (mx > thr)).sum())
            st.at_threshold += int((~trig & (mx == thr)).sum())
            if pend is not None:
                st.pending += int((trig & (mx > thr)).sum())
            delta = np.where(trig, mx if "no_fmax0" in defects else np.maximum(mx, F32(0)), F32(0)).astype(F32)
        m = (m + delta).astype(F32)
        sc = (sc - delta[:, None]).astype(F32)
        if not first:
            alpha = exp2f(-delta)
            if "l_not_rescaled" not in defects:
                l = (l * alpha[:, None]).astype(F32)
            if "o_not_rescaled" not in defects:
                acc = (acc * alpha[:, None]).astype(F32)
            if pend is not None and "pending_not_scaled" not in defects:
                with np.errstate(under="ignore"):
                    pend = (pend * to16(alpha)[:, None]).astype(F16)   # f16 x f16, rounded to f16
        return sc, pend

    def pv(P, kt, blk, ksteps):
        nonlocal acc
        k0 = kt * 64 + blk * 32
        n = 32 // ksteps
        for s in range(ksteps):
            part = P[:, s * n:(s + 1) * n].astype(np.float64) @ vpad[k0 + s * n:k0 + (s + 1) * n]
            acc = (acc + part).astype(F32)

    for kt in range(kt0, kt1):
        first = kt == kt0
        if kernel == "mfma32":
            for blk in (0, 1):
                sc, _ = rescale(scores(kt, blk), first and blk == 0, None)
                p = exp2f(sc)
                for hh in (0, 1):
                    ls = [p[:, HALF_KEYS[hh][0]], p[:, HALF_KEYS[hh][1]]]
                    for r in range(2, 16):
                        ls[r & 1] = (ls[r & 1] + p[:, HALF_KEYS[hh][r]]).astype(F32)
                    l[:, hh] = (l[:, hh] + (ls[0] + ls[1]).astype(F32)).astype(F32)
                pv(to16(p), kt, blk, 2)
        else:
            s0, _ = rescale(scores(kt, 0), first, None)
            s1 = scores(kt, 1)             # against the max block 0 left
            p0 = to16(exp2f(s0))
            s1, p0 = rescale(s1, False, p0)
            p1 = to16(exp2f(s1))
            for blk, P in ((0, p0), (1, p1)):
                pv(P, kt, blk, 1)
                l[:, 0] = (l[:, 0] + P.astype(np.float64).sum(1)).astype(F32)
    return m, (l[:, 0] + l[:, 1]).astype(F32), acc


def merge_groups(parts, nonempty, defects):
    """attention.hip's LDS merge on group 0: parts[g] = (m, l, O)."""
    m0, l0, o0 = parts[0]
    mmax = m0.copy()
    for g in range(1, len(parts)):
        if nonempty[g]:
            mmax = np.maximum(mmax, parts[g][0])
        elif "empty_group_max" in defects:
            mmax = np.maximum(mmax, F32(40.0))   # the skipped group's stale m, taken as +40

    def weight(mg):
        if "merge_exp_e" in defects:
            return np.exp((mg - mmax).astype(np.float64)).astype(F32)
        if "merge_sign" in defects:
            return exp2f(mmax - mg)
        return exp2f(mg - mmax)

    a0 = weight(m0)
    l0, o0 = (l0 * a0).astype(F32), (o0 * a0[:, None]).astype(F32)
    for g in range(1, len(parts)):
        if not nonempty[g]:
            continue
        mg, lg, og = parts[g]
        ag = weight(mg)
        l0 = (l0 + ag.astype(np.float64) * lg).astype(F32)
        o0 = (o0 + ag[:, None].astype(np.float64) * og).astype(F32)
    return mmax, l0, o0


def finish(l, o):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F32(1.0) / l).astype(F32)
        return to16((o * inv[:, None]).astype(F32))


def model_bh(s64, v, T, kernel, groups=1, split_tiles=0, defects=(), st=None, memo=None):
    """One (sequence, head): s64 [T][T] float64 scores, v [T][64] f16 -> f16 [T][64].
    memo: a dict that keeps the passes over a key range for the next route of the same head."""
    st = st or Stats()
    nkt = -(-T // 64)
    s32 = s64.astype(F32)
    vpad = np.zeros((nkt * 64, 64), np.float64)
    vpad[:T] = v.astype(np.float64)

    def run(kt0, kt1):
        if memo is None:
            return model_range(s32, vpad, T, kt0, kt1, kernel, defects, st)
        key = (kernel, kt0, kt1, tuple(defects))
        if key not in memo:
            memo[key] = model_range(s32, vpad, T, kt0, kt1, kernel, defects, st)
        return memo[key]

    if split_tiles:
        parts = [run(a, min(nkt, a + split_tiles))
                 for a in range(0, nkt, split_tiles)]
        S = len(parts)
        m = np.max([p[0] for p in parts], 0)
        lsum, acc = np.zeros(T, F32), np.zeros((T, 64), F32)
        for s, (ms, ls, os_) in enumerate(parts):
            w = exp2f((parts[(s + 1) % S][0] if "combine_other_m" in defects else ms) - m)
            lsum = (lsum + w.astype(np.float64) * ls).astype(F32)
            acc = (acc + w[:, None].astype(np.float64) * os_).astype(F32)
        return finish(lsum, acc)
    if groups == 1:
        _, l, o = run(0, nkt)
        return finish(l, o)
    gper = -(-nkt // groups)
    parts = [run(min(nkt, g * gper), min(nkt, g * gper + gper))
             for g in range(groups)]
    _, l, o = merge_groups(parts, [g * gper < nkt for g in range(groups)], defects)
    return finish(l, o)


def model(c, kernel, groups=1, split_tiles=0, tail2=False, defects=(), st=None, heads=None, memo=None):
    """The whole case in the op's layout (heads: only these (sequence, head) pairs, else NaN)."""
    s = c.scores64().numpy()
    out = np.full((c.B * c.H, c.T, 64), np.nan, F16)
    with np.errstate(all="ignore"):   # the defects overflow on purpose
        for bh in range(c.B * c.H) if heads is None else heads:
            v = c.v[bh].numpy()
            mm = None if memo is None else memo.setdefault(bh, {})
            o = model_bh(s[bh], v, c.T, kernel, groups, split_tiles, defects, st, mm)
            if tail2 and A.tail2_rows(c.T) < c.T:
                r = A.tail2_rows(c.T)
                o[r:] = model_bh(s[bh], v, c.T, kernel, 2, 0, defects, st, mm)[r:]
            out[bh] = o
    return A.op_layout(torch.from_numpy(out), c.B, c.H, c.T)


def routes(T):
    """(kernel, groups, split tiles, tail2) of every summation order the launches of the GPU file take at T."""
    nkt = -(-T // 64)
    r = [("mfma32", 1, 0, False), ("mfma16", 1, 0, False), ("mfma16", 1, 0, True)]
    r += [("mfma32", g, 0, False) for g in (2, 3, 4) if nkt >= g]
    r += [("mfma16", g, 0, False) for g in (2, 4) if nkt >= g]
    r += [("mfma32", 1, -(-nkt // n), False) for n in (2, 3)]
    return sorted(set(r))


SHAPES = X.ATTN_SHAPES


@pytest.mark.parametrize("B,H,T", SHAPES)
@pytest.mark.parametrize("family", A.FAMILIES)
def test_model_within_bound(family, B, H, T):
    c = A.case(family, B, H, T)
    worst, memo = {}, {}
    for kernel, groups, tiles, tail2 in routes(T):
        out = model(c, kernel, groups, tiles, tail2, memo=memo)   # every (sequence, head) pair
        r = float(((out.double() - c.ref).abs() / c.bound(kernel)).nan_to_num(float("inf")).max())
        worst[kernel] = max(worst.get(kernel, 0.0), r)
        assert r <= 1.0, (family, T, kernel, groups, tiles, tail2, r)
    print(f"model {family} T{T}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("B,H,T", SHAPES)
@pytest.mark.parametrize("family", A.INTEGER_FAMILIES)
def test_integer_scores(family, B, H, T):
    """Integers in float64, below 2^11 (exact f16 operands, exact in the fp32
    MFMA whatever the order), and the same numbers from a float32 product."""
    c = A.case(family, B, H, T)
    s = c.scores64()
    assert bool((s == s.round()).all()) and float(s.abs().max()) < 2048
    assert float(c.q.abs().max()) < 2048 and float(c.k.abs().max()) <= 1
    assert torch.equal((c.q.float() @ c.k.float().transpose(1, 2)).double(), s)


def test_family_properties():
    """The claims of the module docstring about tails, peaks and graded."""
    for B, H, T in SHAPES:
        s = A.case("tail_near", B, H, T).scores64()
        assert bool((s.argmax(-1) == T - 1).all()) and bool((s[..., :T - 1].amax(-1) < s[..., T - 1]).all())
        s = A.case("tail_far", B, H, T).scores64()
        assert bool((s[..., :T - 1].amax(-1) < s[..., T - 1] - 14).all())
        s = A.case("graded", B, H, T).scores64()
        assert float(s.max()) == 0 and float(s.min()) == -12
        nkt, w = -(-T // 64), T - 32 * (-(-T // 32) - 1)
        for d in (0, 13):
            s = A.case(f"peaks{d}", B, H, T).scores64()
            for bh in range(B * H):
                hi, lo = (s[bh, :, 0], s[bh, :, T - w]) if bh % 2 == 0 else (s[bh, :, T - w], s[bh, :, 0])   # the plateaus' first keys
                assert bool((hi - lo == d).all()) and bool((s[bh].amax(-1) == hi).all())
        # the plateaus (first w keys, last w keys) lie in different key groups and splits
        assert w <= 32 and (T - w) // 64 == nkt - 1
        for n in (2, 3, 4):   # n key groups (run only with a tile each), "s2" / "s3": ceil(tiles / n) tiles apiece
            if nkt >= n or n < 4:
                per = -(-nkt // n)
                assert 0 // per != (nkt - 1) // per
    assert -(-300 // 64) == 5 and 3 * -(-5 // 4) >= 5   # T = 300, 4 groups: the last group starts past the tiles


# the kinds of row each rescale family must produce in the model: "r" rows that took the rescale branch on
# their own maximum, "t" rows at mx == 8 exactly that did not rescale, "p" rescales with a P pending (mfma16)
PURPOSE = {"ramp7": "r", "ramp8": "rt", "ramp9": "r", "ramp16": "rp", "saw8": "rtp", "saw9": "rp", "saw12": "rp",
           "saw25": "rp"}


@pytest.mark.parametrize("family", A.RESCALE_FAMILIES)
def test_rescale_coverage(family):
    B, H, T = 2, 3, 300
    c = A.case(family, B, H, T)
    for kernel in ("mfma32", "mfma16"):
        st = Stats()
        model(c, kernel, st=st, heads=[0])
        got = dict(r=st.rescaled, t=st.at_threshold, p=st.pending)
        print(f"{family} {kernel}: {got}")
        for kind in PURPOSE[family]:
            if kind == "p" and kernel == "mfma32":
                continue
            assert got[kind] > 0, (family, kernel, got)
    if family == "ramp16":   # phase 0 rescales on a tile's block 0 only, phase 1 on its block 1 only
        st = Stats()
        model(c, "mfma16", st=st, heads=[0])
        assert 0 < st.pending < st.rescaled


# defect -> where it must show: (family, (B, H, T), kernel, groups, split tiles)
DEFECTS = {
    "l_not_rescaled": ("ramp9", (2, 3, 300), "mfma32", 1, 0),
    "o_not_rescaled": ("ramp9", (2, 3, 300), "mfma16", 1, 0),
    "pending_not_scaled": ("saw9", (2, 3, 300), "mfma16", 1, 0),
    "merge_exp_e": ("peaks3", (2, 3, 300), "mfma32", 2, 0),
    "merge_sign": ("peaks3", (2, 3, 300), "mfma16", 2, 0),
    "empty_group_max": ("peaks0", (2, 3, 300), "mfma32", 4, 0),
    "combine_other_m": ("peaks8", (2, 3, 300), "mfma32", 1, 2),
    "threshold16": ("ramp16", (2, 3, 300), "mfma32", 1, 0),
    "no_fmax0": ("ramp9", (2, 3, 300), "mfma32", 1, 0),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_defect_moves_result(defect):
    """Each defect, built into the model, moves some output of its family by
    at least 4 bounds (NaN and inf count as moved) -- and hence fails the GPU
    test, whose bar is 1 bound from the reference."""
    family, (B, H, T), kernel, groups, tiles = DEFECTS[defect]
    c = A.case(family, B, H, T)
    good = model(c, kernel, groups, tiles, heads=[0, 1])
    bad = model(c, kernel, groups, tiles, defects=(defect,), heads=[0, 1])
    mask = ~torch.isnan(good)
    moved = ((bad.double() - good.double()).abs() / c.bound(kernel))[mask].nan_to_num(float("inf"), posinf=float("inf"))
    print(f"{defect}: {family} T{T} {kernel} g{groups} s{tiles}: moved by {float(moved.max()):.3g} bounds")
    assert float(moved.max()) >= 4.0, (defect, float(moved.max()))
