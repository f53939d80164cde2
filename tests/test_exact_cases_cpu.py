"""The constructions of exact_cases.py, proven on the CPU: what
test_gpu_exact.py holds the kernels to is only as good as these claims.

For every case list of the GPU file: the operands are f16 values, a float32
evaluation in a shuffled, chunked K order equals the float64 reference bit
for bit (so any fp32 accumulation order on the device must too), a large
share of the f16 outputs needs a real rounding and a good part of those are
ties, and nothing comes near the f16 range.  The fp32-output ops (fp32
residual stream, patch embed, the exact-fp32 kernels) have no f16 rounding to
exercise: conditions 1, 2 and 4 only.

GELU: mde_device.h's gelu_erf restated in float32 stays within 0.5 ulp16 +
2.6e-5 of the float64 erf form at every x = fl32(a + b) the GPU sweep feeds
it.  Attention: an fp32 emulation of the kernels' arithmetic returns the
selected V row / the constant column exactly.
"""

import numpy as np
import pytest
import torch

import exact_cases as X

MIN_INEXACT, MIN_TIES, MAX_ABS = 0.25, 0.05, 60000.0   # conditions, not measurements


def survives_half(*ts):
    return all(torch.equal(t.half().double(), t) for t in ts)


def check_f16_output(ref, what):
    inexact, ties, amax = X.stats16(ref)
    print(f"{what}: inexact {inexact:.3f} ties {ties:.3f} max |ref| {amax:.1f}")
    assert inexact >= MIN_INEXACT, (what, inexact)
    assert ties >= MIN_TIES, (what, ties)
    assert amax < MAX_ABS, (what, amax)


@pytest.mark.parametrize("m,n,k", X.linear_shapes())
def test_linear_cases(m, n, k):
    a, w, b, acc = X.lin_case(m, n, k)
    assert survives_half(a, w) and torch.equal(b.float().double(), b)
    assert torch.equal(X.shuffled_f32(a, w, (m, n, k)).double(), acc), "fp32 accumulation is not exact"
    g = X.gen("cpu", m, n, k)
    ls, x0 = X.layerscale(g, n).double(), X.resid16(g, (m, n)).double()
    upd = x0 + ls * (acc + b)                      # E_RESID; E_STORE + res0 + res1 has the same magnitudes
    for ref in (acc + b, upd):
        assert torch.equal(ref.float().double(), ref), "the epilogue's fp32 value is not exact"
    for act in (0, 1):
        check_f16_output(X.act64(acc + b, act), f"linear {m}x{n}x{k} act {act}")
    check_f16_output(upd, f"residual update {m}x{n}x{k}")
    check_f16_output(0.125 * (acc + b), f"q scale {m}x{n}x{k}")


@pytest.mark.parametrize("case", sorted({c[:9] for c in X.CONV_CASES} | set(X.CONV32_CASES)))
def test_conv_cases(case):
    geo, act, nres = case[:7], case[7], case[8]
    x, wt, b, acc = X.conv_case(*geo)
    assert survives_half(x, wt)
    assert torch.equal(X.conv_shuffled_f32(geo).double(), acc), "fp32 accumulation is not exact"
    ref, res = X.conv_ref(geo, act, nres)
    assert torch.equal(ref.float().double(), ref)
    check_f16_output(ref, f"conv {case}")


@pytest.mark.parametrize("case", X.CONVT_CASES)
def test_conv_transpose_cases(case):
    x, wt, b, ref = X.convt_case(*case)
    assert survives_half(x, wt)
    s, cin = case[0], case[1]
    # every output pixel is one cin-long dot product: (pixel, cin) x (cin, s s cout)
    flat = X.shuffled_f32(x.permute(0, 2, 3, 1).reshape(-1, cin), wt.permute(2, 3, 1, 0).reshape(-1, cin), case)
    B, _, h, w = x.shape
    got = flat.double().reshape(B, h, w, s, s, cin).permute(0, 5, 1, 3, 2, 4).reshape(B, cin, h * s, w * s)
    assert torch.equal(got + b.view(1, -1, 1, 1), ref), "fp32 accumulation is not exact"
    check_f16_output(ref, f"convT {case}")


def test_patch_embed_case():
    img, w, b, pos, cls_pos, x = X.patch_case(2, 98, 98)
    assert survives_half(img, w)
    assert torch.equal(x.float().double(), x) and float(x.abs().max()) < MAX_ABS
    cols = torch.nn.functional.unfold(img, 14, stride=14).transpose(1, 2)        # [B][patch][588]
    got = X.shuffled_f32(cols, w.reshape(384, 588), "patch").double() + b + pos
    assert torch.equal(got.reshape(2, 49, 384), x.reshape(2, 50, 384)[:, 1:]), "fp32 accumulation is not exact"


# ---- GELU -----------------------------------------------------------------------

def test_gelu_emulation_on_every_f16():
    x = X.finite_f16().float()
    ref = X.gelu64(x)
    err = (torch.from_numpy(X.gelu_erf_emulated(x.numpy())).double() - ref).abs()
    i = int(err.argmax())
    print(f"gelu_erf emulation: max |err| {float(err[i]):.3e} at x = {float(x[i])}")
    assert float(err.max()) <= 2.6e-5
    assert int((err > X.gelu_bound(ref, hw_margin=False)).sum()) == 0


@pytest.mark.parametrize("shape", list(dict.fromkeys([X.GELU_TABLE_SHAPE, X.GELU32_SHAPE]
                                                     + [s[1:4] for s in X.GELU_SITES])), ids=str)
def test_gelu_sweep(shape):
    """The sweep of this shape shows the epilogue every finite f16 value, and
    the emulation keeps the documented bound at the x it forms from them."""
    m, n, k = shape
    a, w, b = X.sweep_operands(m, n, k)
    idx, cls = X.sweep_index(m, n, k)
    assert torch.isfinite(a.float()).all()
    acc = a.double() @ w.double().T if m * n * k < 5e8 else None
    if acc is not None:   # the selector: the accumulator is one A element
        assert torch.equal(acc, X.finite_f16().double()[idx])
    assert len(torch.unique(idx)) == X.NSEQ, "a finite f16 value never reaches the epilogue"
    x = X.sweep_x(idx, cls[None, :].expand_as(idx))
    pairs = torch.unique(idx.flatten() * 8 + cls[None, :].expand_as(idx).flatten())
    if shape == X.GELU_TABLE_SHAPE:
        assert len(pairs) == X.NSEQ * 8, "the table site must see every (value, class) pair"
    xs = torch.unique(x)
    ref = X.gelu64(xs)
    err = (torch.from_numpy(X.gelu_erf_emulated(xs.numpy())).double() - ref).abs()
    over = err - X.gelu_bound(ref, hw_margin=False)
    i = int(over.argmax())
    print(f"sweep {shape}: {len(xs)} distinct x, max(err - bound) {float(over[i]):.3e} at x = {float(xs[i])}")
    assert float(over.max()) <= 0.0


# ---- attention ------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("B,H,T", X.ATTN_SHAPES)
def test_selection_probe(B, H, T, inverse):
    q, k, v, pis = X.selection_case(B, H, T, inverse)
    assert all(len(torch.unique(p)) == T for p in pis), "pi is not a permutation"
    s = q[0].float() @ k[0].float().T
    top = torch.topk(s, 2, dim=-1)
    assert torch.equal(top.indices[:, 0], pis[0]) and float((top.values[:, 0] - top.values[:, 1]).min()) >= 40.0
    o = X.attention_emulated(q, k, v).reshape(B, H, T, 64).permute(0, 2, 1, 3).reshape(B * T, H * 64)
    assert torch.equal(o, X.selection_expected(v, pis, B, H, T))
    if inverse:   # the two permutations of a head are each other's inverse
        fwd = X.selection_perm(T, 0, 0)
        assert torch.equal(fwd[pis[0]], torch.arange(T))


@pytest.mark.parametrize("B,H,T", X.ATTN_SHAPES + [(1, 1, 1)])
def test_uniform_probe(B, H, T):
    q, k, v, exp = X.uniform_case(B, H, T)
    for h in range(H):
        val = X.uniform_values(h)
        assert len(torch.unique(val)) == 64 and float(val[0]) == 1.0 and float(val[1]) == 1.0 - 2.0 ** -11
    o = X.attention_emulated(q, k, v).reshape(B, H, T, 64).permute(0, 2, 1, 3).reshape(B * T, H * 64)
    assert torch.equal(o, exp)
    # fp32 sums of T equal f16 values are exact in any order: j val needs at most 22 bits
    val32 = v[0, 0].float()
    assert torch.equal((np.float32(T) * val32).double(), T * val32.double())
    # one leaked pad key (v = 0, the same score) lands on another f16 value
    if T > 1:
        leaked = (exp.double() * T / (T + 1)).half()
        assert not bool((leaked == exp).any())
