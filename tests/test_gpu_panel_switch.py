"""The panel GEMM's panel switch (gemm_panel.hip panel_gemm_kernel): a
workgroup walks a contiguous range of (panel, chunk) units; when the range
crosses a panel boundary the next panel's A fragments and LayerNorm statistics
are loaded while the previous unit's epilogue still runs, and the new panel's
first unit waits for its fragments by count.  A wait count that is too lax
reads stale fragments or a W chunk that has not landed; nothing but the values
shows it.  So: the smallest shapes that reach every switch path, each compared
bit for bit with the 128^2 kernel (switch "panel" = 0), which has no panels.

The CPU test restates the unit partition and asserts that these shapes reach
the paths they are here for; if it fails, the shapes change, not the assertion.
"""

import collections

import pytest
import torch

K = 384
PBM, PBN, G = 256, 64, 256  # panel rows, unit columns, workgroups (one per CU)

# (M, N) of the cases below
SHAPES = {"store_gelu": (65760, 128), "lnfold_gelu": (90000, 384), "lnfold_gelu_ragged": (16397, 1536),
          "qkv_lnfold": (444 * 37, 384), "resid": (16397, 384)}


def partition(m, n, g=G):
    """Per workgroup the runs [(panel, first local unit, units)] of its even
    contiguous share of the panel-major (panel, chunk) units -- gunit / t0 /
    nu of the kernel at its default partition."""
    nch, npan = n // PBN, -(-m // PBM)
    units = nch * npan
    g = min(g, units)
    out = []
    for wg in range(g):
        t0 = wg * units // g
        nu = (wg + 1) * units // g - t0
        runs, j = [], 0
        while j < nu:
            pnl = (t0 + j) // nch
            jend = min(nu, j + (pnl + 1) * nch - (t0 + j))
            runs.append((pnl, j, jend - j))
            j = jend
        out.append((nu, runs))
    return nch, npan, out


def test_partition_reaches_every_switch_path():
    switches = collections.Counter()
    one_then_switch = ends_on_last = ragged_by_switch = 0
    second_unit = collections.Counter()  # the run's second unit: with / without a chunk DMA of its own
    run_len = collections.Counter()
    first_phase = {}
    for case, (m, n) in SHAPES.items():
        nch, npan, wgs = partition(m, n)
        first_phase[case] = set()
        for nu, runs in wgs:
            switches[len(runs) - 1] += 1
            assert sum(r[2] for r in runs) == nu and nu >= 1
            for i, (pnl, j0, ln) in enumerate(runs):
                run_len[min(ln, 5)] += 1
                if i + 1 < len(runs) and ln == 1:
                    one_then_switch += 1
                if i > 0:
                    first_phase[case].add(runs[0][2])
                    if pnl == npan - 1 and m % PBM:
                        ragged_by_switch += 1
                if ln >= 2:
                    second_unit[j0 + 1 + 2 < nu] += 1
        nu, runs = wgs[-1]
        if runs[-1][0] == npan - 1 and len(runs) > 1:
            ends_on_last += 1
    # workgroups with 0, 1 and 2 switches
    assert switches[0] and switches[1] and switches[2], switches
    # a switch after a run of exactly one unit; a final run ending on the last panel
    assert one_then_switch and ends_on_last, (one_then_switch, ends_on_last)
    # the ragged last panel (live rows < 256) entered through a switch
    assert ragged_by_switch
    # every workgroup of the 6-unit-per-panel case switches, from every phase of a panel
    nch, npan, wgs = partition(*SHAPES["lnfold_gelu"])
    assert all(len(runs) >= 2 for _, runs in wgs) and first_phase["lnfold_gelu"] == set(range(1, nch + 1))
    # runs of one, two, three, four and more units (the peeled unit alone, the
    # pair loop entered or not, with and without its odd last unit)
    assert all(run_len[k] for k in range(1, 6)), run_len
    # the run's second unit both where it issued a chunk DMA and where it did not
    assert second_unit[True] and second_unit[False], second_unit


# ---- GPU cases -----------------------------------------------------------------

GEN = torch.Generator().manual_seed(20260518)


def rn(*shape, scale=1.0):
    return torch.randn(*shape, generator=GEN) * scale


def ln_partials(xh):
    """(sum, squared deviations from the slice mean) per 32-column slice and
    row of the f16 rows, slice-major [k/32][m][2] fp32 (GemmParams::lnst_*)."""
    v = xh.double().reshape(xh.shape[0], -1, 32)
    m2 = ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([v.sum(-1), m2], -1).transpose(0, 1).contiguous().float()


def same(a, b, what):
    if not torch.equal(a, b):
        d = (a.float() - b.float()).abs()
        rows = torch.nonzero(d.reshape(d.shape[0], -1).amax(1) > 0).flatten()[:12].tolist()
        raise AssertionError(f"{what}: panel kernel differs from the 128^2 kernel ({int((d > 0).sum())} elements, "
                             f"max {float(d.max())}, first rows {rows})")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["store_gelu", "lnfold_gelu", "lnfold_gelu_ragged"])
def test_store_across_switch(gpu, case):
    from gpu_util import op, pad_w, ptr, stream
    from monocular_depth_estimation_trt_amd import _lib
    m, n = SHAPES[case]
    x = (rn(m, K) * 2 + 0.3).half().to(gpu)
    wp = pad_w(rn(n, K, scale=K ** -0.5)).to(gpu)
    b = rn(n, scale=0.1).to(gpu)
    fold = case != "store_gelu"
    part = ln_partials(x) if fold else None
    c1 = rn(n).to(gpu)
    outs = []
    for panel in (1, 0):
        out = torch.full((m, n), float("nan"), dtype=torch.float16, device=gpu)
        with _lib.tuning(panel=panel):
            if fold:
                op("mde_op_linear_lnfold", ptr(x), ptr(part), 1e-6, ptr(wp), wp.shape[1], ptr(c1), ptr(b), m, n, K, 2,
                   ptr(out), n, stream())
            else:
                op("mde_op_linear", ptr(x), K, ptr(wp), wp.shape[1], m, n, K, ptr(b), 2, ptr(out), n, stream())
        outs.append(out)
    assert torch.isfinite(outs[0]).all(), f"{case}: outputs not all written"
    same(outs[0], outs[1], case)


@pytest.mark.gpu
def test_qkv_across_switch(gpu):
    """heads = 2: a panel is 6 units, q q k k v v, so the switch falls between
    a V^T unit (its key-permuted scalar stores in the standalone epilogue) and
    a q unit; T = 37 puts image boundaries inside every panel."""
    from gpu_util import op, pad_w, ptr, stream
    from monocular_depth_estimation_trt_amd import _lib
    B, T, H = 444, 37, 2
    D, Tp = 64 * H, 64
    assert (B * T, 3 * D) == SHAPES["qkv_lnfold"]
    a = (rn(B * T, K) * 2 + 0.3).half().to(gpu)
    wp = pad_w(rn(3 * D, K, scale=K ** -0.5)).to(gpu)
    b = rn(3 * D, scale=0.1).to(gpu)
    part = ln_partials(a)
    c1 = rn(3 * D).to(gpu)
    res = []
    for panel in (1, 0):
        q = torch.zeros(B * H, Tp, 64, dtype=torch.float16, device=gpu)
        kk = torch.zeros_like(q)
        vt = torch.zeros(B * H, 64, Tp, dtype=torch.float16, device=gpu)
        with _lib.tuning(panel=panel):
            op("mde_op_qkv_lnfold", ptr(a), ptr(part), 1e-6, ptr(wp), wp.shape[1], ptr(c1), ptr(b), B, T, H, Tp, 0.125,
               ptr(q), ptr(kk), ptr(vt), stream())
        res.append((q, kk, vt))
    assert float(res[0][0].abs().max()) > 0 and float(res[0][2].abs().max()) > 0
    for name, x0, x1 in zip("q k vt".split(), res[0], res[1]):
        same(x0, x1, f"qkv {name}")


@pytest.mark.gpu
def test_resid_across_switch(gpu):
    """The f16-residual form (switch "panel" = 2): xh bit for bit; the LN
    partials of the rows written sum the same 32 f16 values in another
    grouping, so they agree to fp32 rounding (as test_panel_gemm_bit_exact)."""
    from gpu_util import close, op, pad_w, ptr, stream
    from monocular_depth_estimation_trt_amd import _lib
    m, n = SHAPES["resid"]
    a = (rn(m, K) * 2).half().to(gpu)
    wp = pad_w(rn(n, K, scale=K ** -0.5)).to(gpu)
    b = rn(n, scale=0.1).to(gpu)
    ls = (0.5 + 0.1 * rn(n)).to(gpu)
    x0 = (rn(m, n) * 2).half().to(gpu)
    res = []
    for panel in (2, 0):
        xh = x0.clone()
        part = torch.full((n // 32, m, 2), float("nan"), device=gpu)
        with _lib.tuning(panel=panel):
            op("mde_op_linear_residual_f16", ptr(a), K, ptr(wp), wp.shape[1], m, n, K, ptr(b), ptr(ls), ptr(xh), n,
               ptr(part), stream())
        res.append((xh, part))
    same(res[0][0], res[1][0], "resid xh")
    assert torch.isfinite(res[0][1]).all(), "partials not all written"
    close(res[0][1], res[1][1].float(), 1e-5, 1e-4, "resid ln partials")
