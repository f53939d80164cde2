"""Per-segment timing of the panel GEMM (gemm_panel.hip built with -DPX_TRACE):
runs one fc1-shaped launch (ViT-S B=48: M 65760, N 1536, K 384, GELU; LN
fold with --fold) through the C ABI with the switch on, reads the s_memtime
stamps of the eight traced workgroups and prints, per segment kind, the work
time and the barrier wait, and for panel_gemm_kernel the cost of the panel
switch and of the prologue (the stamps: gemm_panel.hip PTRACE).

    python tools/panel_trace.py LIB [--act 2] [--n 1536] [--fold]

A qkv-shaped launch is --n 1152 --act 0: the plain-store kernel at the qkv
GEMM's size (the head-split kernel's scattered stores and its switch form 1
are not traced by it; a -DPX_STREAM=2 build runs form 1 in every kernel).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def switch_report(t, nsegs, unit_len, ghz):
    """panel_gemm_kernel's rows 90-95: the mid-run panel switch and the
    prologue, in s_memtime ticks and us at the in-kernel clock.  The switch's
    first segment is the standalone epilogue where the build has one (PX_STREAM
    0, and form 1 with the new panel's loads issued in front of it) and the
    issue of the new panel's 24 A loads where it has none (form 2)."""
    us = lambda ticks: ticks / (ghz * 1e3)
    sw_rows, pro_rows, tail = [], [], []
    for b in range(8):
        n = nsegs[b]
        if n < 3:
            continue
        st, en, wt = t[b, :, :, 0], t[b, :, :, 1], t[b, :, :, 2]
        ul = unit_len[b]
        k = int(t[b, 0, 94, 0]) if t[b, 0, 93, 0] > 0 else -1
        if 1 <= k <= n - 2:
            a, e, w, s = t[b, :, 93, 0], t[b, :, 93, 1], t[b, :, 93, 2], st[:, k]
            # what the switch adds to the two units around it, barrier to barrier
            excess = (st[:, k + 1].max() - st[:, k - 1].max()) - 2 * ul
            sw_rows.append(((e - a).mean(), (w - e).mean(), (s - w).mean(), (st[:, k + 1] - s).mean(), excess, k))
        if k != 1:
            ent, p0, p1, u0 = t[b, :, 95, 0], t[b, :, 91, 0], t[b, :, 92, 0], st[:, 0]
            excess = (st[:, 1].max() - ent.min()) - ul
            pro_rows.append(((p0 - ent).mean(), (p1 - p0).mean(), (u0 - p1).mean(), (st[:, 1] - u0).mean(), excess))
        tail.append((t[b, :, 90, 0] - wt[:, n - 1]).mean())
    if pro_rows:
        r = np.array(pro_rows, dtype=np.float64).mean(0)
        print(f"prologue (ticks, {len(pro_rows)} workgroups): entry -> tables filled, chunks issued {r[0]:6.0f}  "
              f"first panel issued -> its waits done {r[1]:6.0f}  -> first MFMA (unit 0's barrier) {r[2]:6.0f}  "
              f"first unit {r[3]:6.0f}")
        print(f"prologue excess (entry -> unit 1's barrier, less one regular unit): {r[4]:6.0f} ticks = {us(r[4]):.2f} us")
    for row in sw_rows:
        print(f"switch before unit {row[5]:2d} (ticks): epilogue / loads issued {row[0]:6.0f}  loads + waits {row[1]:6.0f}  "
              f"-> barrier {row[2]:6.0f}  first unit {row[3]:6.0f}  excess over two regular units {row[4]:6.0f} "
              f"= {us(row[4]):.2f} us")
    if sw_rows:
        r = np.array([x[:5] for x in sw_rows], dtype=np.float64)
        print(f"switch, mean over {len(r)} workgroups: epilogue / loads issued {r[:, 0].mean():6.0f}  loads + waits {r[:, 1].mean():6.0f}  "
              f"-> barrier {r[:, 2].mean():6.0f}  first unit {r[:, 3].mean():6.0f}  excess {r[:, 4].mean():6.0f} ticks "
              f"= {us(r[:, 4].mean()):.2f} us (min {us(r[:, 4].min()):.2f}, max {us(r[:, 4].max()):.2f})")
    if tail:
        print(f"tail (last unit's wait -> stores drained): {np.mean(tail):6.0f} ticks = {us(np.mean(tail)):.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--act", type=int, default=2)
    ap.add_argument("--n", type=int, default=1536)
    ap.add_argument("--m", type=int, default=65760)
    ap.add_argument("--fold", action="store_true", help="LayerNorm folded into the GEMM (the engine's fc1 / qkv form)")
    a = ap.parse_args()
    import torch
    from gpu_util import pad_w, ptr, stream
    from monocular_depth_estimation_trt_amd import _lib
    _lib.use_library(a.lib)
    L = _lib.lib()
    _lib.set_tuning("panel", 1)
    dev = torch.device("cuda:0")
    m, n, k = a.m, a.n, 384
    x = torch.randn(m, k, device=dev).half()
    wp = pad_w(torch.randn(n, k) * k ** -0.5).to(dev)
    b = torch.randn(n, device=dev) * 0.1
    out = torch.empty(m, n, dtype=torch.float16, device=dev)
    if a.fold:
        # (sum, squared deviations from the slice mean) per 32-column slice, slice-major
        v = x.float().reshape(m, -1, 32)
        st = torch.stack([v.sum(-1), ((v - v.mean(-1, keepdim=True)) ** 2).sum(-1)], -1).transpose(0, 1).contiguous()
        c1 = wp[:n, :k].float().sum(1).contiguous()

        def launch():
            L.mde_op_linear_lnfold(ptr(x), ptr(st), 1e-6, ptr(wp), wp.shape[1], ptr(c1), ptr(b), m, n, k, a.act,
                                   ptr(out), n, stream())
    else:
        def launch():
            L.mde_op_linear(ptr(x), k, ptr(wp), wp.shape[1], m, n, k, ptr(b), a.act, ptr(out), n, stream())
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    buf = np.zeros((8, 8, 96, 4), dtype=np.uint64)
    fn = getattr(L, "mde_debug_panel_trace")
    fn.argtypes = [C.c_void_p]
    assert fn(buf.ctypes.data) == 0
    t = buf.astype(np.int64)
    nsegs = [int((t[blk, 0, :90, 0] > 0).sum()) for blk in range(8)]
    print(f"units recorded per wave, traced workgroups 16 + 33 i: {nsegs}")
    # a panel switch in front of unit k (panel_gemm_kernel: row 94 holds k)
    # lengthens unit k - 1's barrier-to-barrier interval and unit k is the
    # run's first: both stay out of the per-unit figures
    pg = bool((t[:, :, 93, 1] > 0).any())
    sws = [int(t[blk, 0, 94, 0]) if pg and t[blk, 0, 93, 0] > 0 else -1 for blk in range(8)]
    rows, unit_len = [], []
    for blk in range(8):
        st, en, wt = t[blk, :, :, 0], t[blk, :, :, 1], t[blk, :, :, 2]
        mine = []
        for u in range(1, nsegs[blk] - 1):
            if u in (sws[blk] - 1, sws[blk]):
                continue
            length = st[:, u + 1].max() - st[:, u].max()  # barrier to barrier
            work = (en[:, u] - st[:, u]).mean()            # after barrier -> before the end-of-unit wait
            wait = (wt[:, u] - en[:, u]).mean()            # the counted vmcnt
            skew = (st[:, u + 1] - wt[:, u]).mean()        # waiting at the barrier
            spread = (en[:, u] - st[:, u]).max() - (en[:, u] - st[:, u]).min()
            mine.append((length, work, wait, skew, spread))
        rows += mine
        unit_len.append(float(np.median([x[0] for x in mine])) if mine else 0.0)
    r = np.array(rows, dtype=np.float64)
    print(f"unit (s_memtime ticks, n={len(r)}): length {r[:, 0].mean():7.0f}  work {r[:, 1].mean():7.0f}  "
          f"vmcnt wait {r[:, 2].mean():7.0f}  barrier {r[:, 3].mean():7.0f}  work spread over waves {r[:, 4].mean():7.0f}")

    # in-kernel clock: memtime ticks per 100 MHz realtime tick over each wave's units
    ck = []
    for blk in range(8):
        for w in range(8):
            nseg = nsegs[blk]
            mt, rt = t[blk, w, :nseg, 0], t[blk, w, :nseg, 3]
            if nseg > 1 and rt[-1] > rt[0]:
                ck.append((mt[-1] - mt[0]) / (rt[-1] - rt[0]) * 0.1)
    ghz = float(np.median(ck)) if ck else 0.0
    if ck:
        first_last = [(t[b, 0, nsegs[b] - 1, 3] - t[b, 0, 0, 3]) / 100.0 for b in range(8) if nsegs[b] > 1]
        print(f"in-kernel clock {ghz:.3f} GHz (median over waves); first -> last unit start {np.median(first_last):.1f} us")
    # whole-kernel phases: realtime stamps, us
    rt = t[:, :, :, 3].astype(np.float64) / 100.0
    if (t[:, :, 95, 3] > 0).all():
        ent, end = rt[:, :, 95], rt[:, :, 90]
        print(f"entry -> end {np.median(end - ent):.2f} us; entry -> first unit {np.median(rt[:, :, 0] - ent):.2f} us "
              f"(median over the traced workgroups' waves)")
        if pg and ghz > 0:
            switch_report(t, nsegs, unit_len, ghz)
        else:  # panel32_kernel's rows
            p0, p1, u0 = rt[:, :, 91], rt[:, :, 92], rt[:, :, 0]
            print(f"per wave (median, us): entry -> first panel load start {np.median(p0 - ent):.2f}, "
                  f"first panel load {np.median(p1 - p0):.2f}, -> first unit {np.median(u0 - p1):.2f}")
            sw = t[:, :, 93, 3] > 0
            if sw.any():
                print(f"mid-run panel switch (epilogue + A load + stats + drain): "
                      f"{np.median((rt[:, :, 94] - rt[:, :, 93])[sw]):.2f} us over {int(sw.sum())} waves")
        print(f"spread of kernel-entry times over the traced workgroups: {ent[:, 0].max() - ent[:, 0].min():.2f} us; "
              f"of end times {end[:, 0].max() - end[:, 0].min():.2f} us")
    lo = np.array([(t[b, :4, 1:nsegs[b] - 1, 1] - t[b, :4, 1:nsegs[b] - 1, 0]).mean() for b in range(8)])
    hi = np.array([(t[b, 4:, 1:nsegs[b] - 1, 1] - t[b, 4:, 1:nsegs[b] - 1, 0]).mean() for b in range(8)])
    print(f"work per unit: waves 0-3 {lo.mean():7.0f}  waves 4-7 {hi.mean():7.0f}")


if __name__ == "__main__":
    main()
