"""The constructions of bilinear_cases.py, proven on the CPU on the operands
test_gpu_bilinear.py gives the kernels.

1. The shape lists: conv.hip's eligibility rule restated in the same fp32
   arithmetic gives the kernel each list entry names -- 19 -> 28 rows spans
   exactly 12 source rows (upconv), 19 -> 27 spans 13 (conv3_up); an identity
   map of 12 rows is taken, one of 13 is not -- and every route case sits on
   its side of the thresholds it is there for.
2. Exact shapes: the fp32 coordinate is exact with weights in {0, 1/4, 1/2,
   3/4}; on the dyadic maps the two-level f16 lerp, every operation rounded
   or the multiply-adds fused, and the fp32 four-tap form both EQUAL float64,
   and the result is an f16 value.  Under a conv: sum |u| |w| stays below 2^24
   quanta of 2^-8 (any fp32 accumulation order is exact), an fp32 conv equals
   float64, and the metric = 0 head's dot product likewise on its 2^-10 grid.
3. General shapes: the emulations stay inside the bounds on every family
   (worst measured: f16 lerp 0.86 of its bound, on ramp 37 x 40 -> 74 x 70).
4. Each defect built into the REFERENCE moves it by at least 4 x the bound on
   some family and shape of the GPU file.
"""

import pytest
import torch
import torch.nn.functional as F

import bilinear_cases as Bc
import exact_cases as X

SHAPES = Bc.EXACT_SHAPES + Bc.GENERAL_SHAPES
SID = lambda s: "%dx%d-%dx%d" % s[:4]  # noqa: E731


def survives_half(*ts):
    return all(torch.equal(t.half().double(), t) for t in ts)


def test_shape_lists():
    for sh, sw, uh, uw, want in SHAPES:
        assert Bc.up_kernel(2, sh, uh, uw) == want, (sh, sw, uh, uw, want)
        assert Bc.up_kernel(2, sh, uh, uw, upconv=0) == "conv3_up"
    assert all(Bc.is_exact(*s[:4]) for s in Bc.EXACT_SHAPES) and not any(Bc.is_exact(*s[:4]) for s in Bc.GENERAL_SHAPES)
    # both sides of the USR boundary, and of the identity-size limit
    assert Bc.upconv_eligible(19, 28) and not Bc.upconv_eligible(19, 27)
    assert Bc.upconv_eligible(12, 12) and not Bc.upconv_eligible(13, 13)
    assert Bc.upconv_eligible(8, 8), "test_gpu_exact.py::test_gelu_upconv's map"
    assert not Bc.upconv_eligible(31, 31), "a 31-row identity map is conv3_kernel's"
    y0, y1, _ = Bc.axis64(133, 224)   # the persistent case: tile rows at exactly USR source rows
    spans = [int(y1[min(t * 16 + 16, 223)]) - int(y0[max(t * 16 - 1, 0)]) + 1 for t in range(14)]
    assert max(spans) == Bc.USR and spans.count(Bc.USR) == 12 and Bc.upconv_eligible(133, 224)
    y0, y1, _ = Bc.axis64(19, 28)
    assert int(y1[16]) - int(y0[0]) + 1 == 12   # tile 0: virtual rows -1 .. 16, the first of them padding
    y0, y1, _ = Bc.axis64(19, 27)
    assert int(y1[16]) - int(y0[0]) + 1 == 13
    assert Bc.last_overshoots(8, 14) and Bc.last_overshoots(4, 22)
    kinds = set()
    for name, B, cin, cout, sh, sw, uh, uw, sw_, route in Bc.UP_ROUTES:
        M = B * uh * uw
        if route["kind"] == "conv_direct":
            assert cin % 32 == 0 and cout == 32
            want = "conv3_up" if cin > 128 else Bc.up_kernel(B, sh, uh, uw, sw_.get("upconv", 1))
            assert route["conv"] == want, (name, want)
            kinds.add(want)
        else:   # gemm.hip pick_tile, E_STORE
            assert cin % 32 and cin % 8 == 0
            big = -(-M // 128) * -(-cout // 128)
            tile = (128, 32) if cout <= 32 else ((128, 64) if M >= 32768 else (64, 64)) if cout <= 64 else \
                ((128, 128) if big >= 240 else (64, 64))
            assert (route["bm"], route["bn"]) == tile, (name, tile)
            kinds.add(tile)
    assert kinds == {"conv3_up", "upconv", "upconv_persist", (128, 32), (64, 64), (128, 64), (128, 128)}


@pytest.mark.parametrize("shape", Bc.EXACT_SHAPES, ids=SID)
def test_exact_upsample(shape):
    sh, sw, uh, uw, _ = shape
    for n_in, n_out in ((sh, uh), (sw, uw)):
        i0, i1, l1 = Bc.axis32(n_in, n_out)
        j0, j1, m1 = Bc.axis64(n_in, n_out)
        assert torch.equal(i0, j0) and torch.equal(i1, j1) and torch.equal(l1.double(), m1)
        assert set((4 * m1).tolist()) <= {0.0, 1.0, 2.0, 3.0}
    for C in (8, 72):
        x = Bc.family_map("dyadic", 2, C, sh, sw)
        ref = Bc.up64(x, uh, uw)
        assert survives_half(x, ref), "the upsampled dyadic map is not an f16 value"
        for fused in (False, True):
            assert torch.equal(Bc.up16_emulated(x, uh, uw, fused).double(), ref), f"f16 lerp (fused {fused}) is not exact"
        assert torch.equal(Bc.blend32(x, uh, uw).double(), ref), "the fp32 four-tap form is not exact"
        assert torch.equal(F.interpolate(x.float(), size=(uh, uw), mode="bilinear", align_corners=True).double(), ref)
        assert len(torch.unique(ref)) > 100 or ref.numel() < 4000


@pytest.mark.parametrize("route", [r for r in Bc.UP_ROUTES if Bc.is_exact(*r[4:8])], ids=lambda r: r[0])
def test_exact_conv(route):
    name, B, cin, cout, sh, sw, uh, uw, _, _ = route
    x = Bc.family_map("dyadic", B, cin, sh, sw, Bc.map_range(cin))
    up = Bc.up64(x, uh, uw)
    wt, b1 = Bc.conv_w64(cin, cout)
    assert survives_half(x, up, wt) and torch.equal((up * 4).round(), up * 4)
    ref = Bc.conv64(up, wt)
    quanta = float(Bc.conv64(up.abs(), wt.abs()).max()) / X.QUANTUM
    assert quanta < 2.0 ** 24, (name, quanta)
    got = F.conv2d(F.pad(up.float(), (1, 1, 1, 1)), wt.float())
    assert torch.equal(got.double(), ref), "fp32 accumulation is not exact"
    full = ref + b1.view(1, -1, 1, 1)
    assert torch.equal(full.float().double(), full)
    inexact, ties, amax = X.stats16(full)
    print(f"{name}: conv inexact {inexact:.3f} ties {ties:.3f} max |ref| {amax:.1f} sum |u| |w| {quanta:.3g} quanta")
    assert inexact >= 0.1 and amax < 60000.0, (name, inexact, amax)
    if cout == 32:   # the head on top: sum_j relu(.) w2_j on the 2^-10 grid
        w2, b2 = Bc.head_w()
        hpe = X.resid16(Bc.gen("hpe", name), (uh * uw, 32)).double()
        for pe in (None, hpe):
            v = full if pe is None else full + pe.T.reshape(1, 32, uh, uw)
            assert torch.equal(v.float().double(), v)
            hq = float((F.relu(v) * w2.abs().view(1, -1, 1, 1)).sum(1).max()) * 1024
            assert hq < 2.0 ** 24, (name, hq)
            z = Bc.head64(ref, b1, w2, b2, pe)
            z32 = F.relu((F.relu(v.float()) * w2.float().view(1, -1, 1, 1)).sum(1) + b2)
            assert torch.equal(z32.double(), z), "the head's fp32 dot product is not exact"
            assert float((z > 0).double().mean()) > 0.2, "the head's ReLU leaves too little"


@pytest.mark.parametrize("shape", Bc.GENERAL_SHAPES, ids=SID)
def test_emulations_within_bounds(shape):
    sh, sw, uh, uw, _ = shape
    for fam in Bc.FAMILIES:
        for C in (8, 72):
            x = Bc.family_map(fam, 2, C, sh, sw)
            ref, bd = Bc.up64(x, uh, uw), Bc.bound_lerp(x, uh, uw)
            worst = 0.0
            for fused in (False, True):
                e = (Bc.up16_emulated(x, uh, uw, fused).double() - ref).abs()
                assert bool((e <= bd).all()), (fam, shape, fused, float((e - bd).max()))
                worst = max(worst, float((e / bd)[bd > 0].max()) if bool((bd > 0).any()) else 0.0)
            b32 = Bc.bound_blend32(x, uh, uw)
            e32 = (Bc.blend32(x, uh, uw).half().double() - ref).abs()
            assert bool((e32 <= b32).all()), (fam, shape, float((e32 - b32).max()))
            # a zero neighbourhood leaves a zero bound: the output must be exactly zero there
            assert bool((ref[bd == 0] == 0).all()) and bool((ref[b32 == 0] == 0).all())
            print(f"{fam} {SID(shape)} C {C}: f16 lerp emulation at most {worst:.3f} of its bound")


def onehot_shift(defect, fam, B, cin, sh, sw, uh, uw):
    """(largest shift of the one-hot conv's reference / its bound, where the bound is not zero;
    whether a zero-bound element moved)."""
    x = Bc.family_map(fam, B, cin, sh, sw)
    wt = Bc.onehot_weights(cin, 32)
    ref, bad = Bc.conv_up64(x, uh, uw, wt), Bc.conv_up64(x, uh, uw, wt, defect)
    bd = Bc.conv64(torch.maximum(Bc.bound_lerp(x, uh, uw), Bc.bound_blend32(x, uh, uw)), wt)
    d = (bad - ref).abs()
    return (float((d / bd)[bd > 0].max()) if bool((bd > 0).any()) else 0.0), bool((d[bd == 0] > 0).any())


@pytest.mark.parametrize("defect", Bc.DEFECTS)
def test_defects_move_the_reference(defect):
    """>= 4 x the bound (the looser of the f16-lerp and the fp32-blend bound, so
    that both kinds of site see it) on some family and shape; through the
    one-hot conv, which is how the GPU file reads the conv kernels' map."""
    best = (0.0, None)
    for sh, sw, uh, uw, _ in Bc.GENERAL_SHAPES:
        if defect == "swap_scales" and (uh == 1 or uw == 1):
            continue
        for fam in Bc.FAMILIES:
            r, zero_moved = onehot_shift(defect, fam, 2, 32, sh, sw, uh, uw)
            r = float("inf") if zero_moved else r
            if r > best[0]:
                best = (r, (fam, sh, sw, uh, uw))
    print(f"{defect}: moves the reference by {best[0]:.3g} x the bound on {best[1]}")
    assert best[0] >= 4.0, (defect, best)


@pytest.mark.parametrize("defect", [d for d in Bc.DEFECTS if d not in ("halo_replicate", "seam_drop")])
def test_defects_move_the_resize(defect):
    """The same for the resize ops, which see the upsampled map directly."""
    best = 0.0
    for sh, sw, uh, uw, _ in Bc.GENERAL_SHAPES:
        if defect == "swap_scales" and (uh == 1 or uw == 1):
            continue
        for fam in Bc.FAMILIES:
            x = Bc.family_map(fam, 2, 72, sh, sw)
            bd = torch.maximum(torch.maximum(Bc.bound_lerp(x, uh, uw), Bc.bound_blend32(x, uh, uw)),
                               Bc.bound_interp32(x, uh, uw))
            d = (Bc.up64(x, uh, uw, defect) - Bc.up64(x, uh, uw)).abs()
            if bool((d[bd == 0] > 0).any()):
                best = float("inf")
            elif bool((bd > 0).any()):
                best = max(best, float((d / bd)[bd > 0].max()))
    print(f"{defect}: moves the resize reference by {best:.3g} x the bound")
    assert best >= 4.0, (defect, best)
