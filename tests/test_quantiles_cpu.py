"""visualize.quantiles_np (the numpy statement of mde_op_depth_quantiles, written with a sort) against a
direct statement with np.percentile, np.isfinite, slicing and min / max; the reference's robust_range and
distribution on top of it; colorize_ranged_np against colorize_np's fixed mode.  Every comparison is
exact float64 equality with NaN equal to NaN.  No GPU."""

import numpy as np
import pytest

import quantile_cases as qc

from monocular_depth_estimation_trt_amd import visualize as vz


def direct(maps, q, positive_only=False, reciprocal=False, pooled=False, sample_cap=0):
    """The contract with numpy's own percentile.  With three quantiles the third takes the max's slot."""
    x = np.asarray(maps, np.float32)
    x = x[None] if x.ndim == 2 else x
    pools, n_valid = [], []
    with np.errstate(all="ignore"):
        for im in x:
            v = im.ravel()
            ok = np.isfinite(v) & (v > 0) if positive_only else np.isfinite(v)
            v = v[ok]
            n_valid.append(v.size)
            if sample_cap > 0 and v.size > sample_cap:
                v = v[:: max(1, v.size // sample_cap)]
            v = np.where(v == 0, np.float64(0.0), v.astype(np.float64))  # -0 counts as +0
            pools.append(1.0 / v if reciprocal else v)
        if pooled:
            pools, n_valid = [np.concatenate(pools)], [sum(n_valid)]
        rows = np.zeros((len(pools), 8))
        for r, v, nv in zip(rows, pools, n_valid):
            r[0], r[1] = nv, v.size
            if v.size == 0:
                r[2:6] = np.nan
                r[6:] = 0.0, 1.0
                continue
            qv = np.percentile(v, list(q))
            r[2], r[3] = v.min(), v.max()
            r[4:4 + min(len(q), 2)] = qv[:2]
            if len(q) == 3:
                r[3] = qv[2]
            vmin, vmax = qv[0], qv[-1]
            if not np.isfinite(vmin) or not np.isfinite(vmax) or vmax <= vmin:
                vmin, vmax = v.min(), v.max()
                if vmax <= vmin:
                    vmax = vmin + 1.0
            r[6:] = vmin, vmax
    return rows


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


FLAGS = [(p, r, pooled) for p in (False, True) for r in (False, True) for pooled in (False, True)]


@pytest.mark.parametrize("regime", qc.REGIMES)
def test_quantiles_np_equals_np_percentile(regime):
    for B, h, w, _ in qc.SHAPES:
        x = qc.maps(regime, B, h, w)
        for positive_only, reciprocal, pooled in FLAGS:
            for cap in (0, 64):
                for q in qc.QS:
                    got = vz.quantiles_np(x, q, positive_only, reciprocal, pooled, cap)
                    want = direct(x, q, positive_only, reciprocal, pooled, cap)
                    assert got.shape == (1 if pooled else B, 8)
                    assert same(got, want), (regime, (B, h, w), positive_only, reciprocal, pooled, cap, q, got, want)


def test_reciprocal_is_the_percentile_of_one_over_x():
    x = qc.maps("lognormal", 1, 100, 131)[0]
    v = x.astype(np.float64).ravel()
    row = vz.quantiles_np(x, (2.0, 50.0, 98.0), True, True)[0]
    assert same(vz.row_quantiles(row, 3), np.percentile(1.0 / v, [2, 50, 98]))
    assert row[vz.Q_MIN] == (1.0 / v).min() and row[vz.Q_NVALID] == v.size == row[vz.Q_NUSED]
    # mixed signs and zeros: 1 / x ascends inside each sign, 1 / 0 = +inf is on top
    y = qc.maps("sprinkled", 1, 100, 131)[0]
    u = y.ravel()[np.isfinite(y.ravel())].astype(np.float64)
    with np.errstate(all="ignore"):
        want = np.percentile(1.0 / np.where(u == 0, 0.0, u), [10, 40])
    assert same(vz.row_quantiles(vz.quantiles_np(y, (10.0, 40.0), False, True)[0], 2), want)


def test_pooled_is_the_concatenation():
    x = qc.maps("sprinkled", 3, 37, 53)
    cat = np.concatenate([im.ravel()[np.isfinite(im.ravel()) & (im.ravel() > 0)] for im in x]).astype(np.float64)
    row = vz.quantiles_np(x, (2.0, 98.0), True, False, True, 0)
    assert row.shape == (1, 8) and row[0, 0] == cat.size
    assert same(row[0, 4:6], np.percentile(cat, [2, 98])) and same(row[0, 2:4], [cat.min(), cat.max()])
    assert vz.robust_range_np(x, sample_cap=0) == tuple(np.percentile(cat, [2, 98]))
    assert vz.robust_range_np(list(x), sample_cap=0) == vz.robust_range_np(x, sample_cap=0)
    # every image has its own stride: 3 x 1961 pixels, a cap of 64
    parts = []
    for im in x:
        v = im.ravel()[np.isfinite(im.ravel()) & (im.ravel() > 0)]
        parts.append(v[:: max(1, v.size // 64)] if v.size > 64 else v)
    row = vz.quantiles_np(x, (2.0, 98.0), True, False, True, 64)[0]
    assert row[1] == sum(p.size for p in parts)
    assert same(row[4:6], np.percentile(np.concatenate(parts).astype(np.float64), [2, 98]))


def test_fallbacks():
    const = np.full((7, 9), 2.5, np.float32)
    assert same(vz.quantiles_np(const, (2.0, 98.0), True)[0], [63, 63, 2.5, 2.5, 2.5, 2.5, 2.5, 3.5])
    assert vz.robust_range_np(const) == (2.5, 3.5)
    empty = np.full((7, 9), np.nan, np.float32)
    nan = np.nan
    assert same(vz.quantiles_np(empty, (2.0, 98.0))[0], [0, 0, nan, nan, nan, nan, 0.0, 1.0])
    assert vz.robust_range_np(empty) == (0.0, 1.0) and vz.distribution_np(empty) is None
    assert same(vz.quantiles_np(np.zeros((3, 5), np.float32), (2.0, 98.0), True)[0], [0, 0, nan, nan, nan, nan, 0, 1])
    one = qc.maps("one_valid", 1, 7, 9)[0]
    assert same(vz.quantiles_np(one, (2.0, 50.0, 98.0))[0], [1, 1, 4.0, 4.0, 4.0, 4.0, 4.0, 5.0])
    assert same(vz.quantiles_np(one, (50.0,))[0], [1, 1, 4.0, 4.0, 4.0, 0.0, 4.0, 5.0])
    # one quantile is both ends of the range, which then falls back to min, max
    x = qc.maps("lognormal", 1, 7, 9)[0]
    row = vz.quantiles_np(x, (50.0,))[0]
    assert row[4] == np.median(x.astype(np.float64)) and tuple(row[6:]) == (x.min(), x.max()) and row[5] == 0
    # 1 / 0 = +inf twice at the top of a reciprocal sample: p100 is inf - inf = NaN, as np.percentile's
    # is, and the range is min, max
    z = np.array([[0.0, -0.0, 1.0, 2.0, 4.0]], np.float32)
    row = vz.quantiles_np(z, (0.0, 100.0), False, True)[0]
    assert same(row, [5, 5, 0.25, np.inf, 0.25, nan, 0.25, np.inf])


@pytest.mark.parametrize("n_valid", [64, 65, 127, 128, 129, 200])
def test_stride_rule_at_a_small_cap(n_valid):
    x = qc.with_n_valid(n_valid)
    v = x.ravel()[np.isfinite(x.ravel()) & (x.ravel() > 0)]
    assert v.size == n_valid
    stride = {64: 1, 65: 1, 127: 1, 128: 2, 129: 2, 200: 3}[n_valid]
    used = v[::stride].astype(np.float64)
    row = vz.quantiles_np(x, (2.0, 98.0), True, False, False, 64)[0]
    assert row[0] == n_valid and row[1] == used.size == -(-n_valid // stride)
    assert same(row[2:6], [used.min(), used.max(), *np.percentile(used, [2, 98])])
    assert same(row, direct(x, (2.0, 98.0), True, False, False, 64)[0])


@pytest.mark.parametrize("side, stride", [(450, 1), (640, 2)])
def test_stride_rule_at_the_reference_cap(side, stride):
    """202500 // 200000 = 1: above the cap and still every pixel; 409600 // 200000 = 2."""
    x = qc.maps("lognormal", 1, side, side)[0]
    v = x.ravel().astype(np.float64)[::stride]
    row = vz.quantiles_np(x, (2.0, 98.0), True, False, False, vz.SAMPLE_CAP)[0]
    assert row[0] == side * side and row[1] == v.size
    assert same(row[4:6], np.percentile(v, [2, 98]))
    assert vz.robust_range_np(x) == tuple(np.percentile(v, [2, 98]))


def test_distribution_np():
    """demo.py:distribution: np.percentile and np.median over the finite pixels.  The median's lerp
    a + (b - a) * 0.5 equals np.median's (a + b) / 2 where both are exact, which float32 values of one
    sign within 2^29 of each other are in float64."""
    x = qc.maps("lognormal", 1, 37, 53)[0].copy()
    x[3, 4:20] = np.nan
    x[9, 7] = np.inf
    fin = x[np.isfinite(x)].astype(np.float64)
    d = vz.distribution_np(x)
    assert d == {"p02": np.percentile(fin, 2), "median": np.median(fin), "p98": np.percentile(fin, 98),
                 "valid_pct": float(fin.size) / x.size * 100.0}
    line = vz.format_distribution(d)
    assert line.startswith("[MDET] depth : p02 ") and line.endswith("%")
    words = line.split()
    assert [float(words[i]) for i in (4, 6, 8)] == [d["p02"], d["median"], d["p98"]]
    assert float(words[10][:-1]) == d["valid_pct"]


def test_colorize_ranged_np():
    x = qc.maps("sprinkled", 2, 37, 53)
    for vmin, vmax in ((0.5, 20.0), (2.5, 2.5), (5.0, 1.0), (-np.inf, np.inf)):
        for swap_rb in (True, False):
            want, _ = vz.colorize_np(x, "fixed", vmin=vmin, vmax=vmax, swap_rb=swap_rb)
            assert vz.colorize_ranged_np(x, (vmin, vmax), swap_rb=swap_rb).tobytes() == want.tobytes()
    # an axis per image; positive_only makes 0 and the negatives bad; reciprocal draws 1 / x
    ranges = np.array([[0.5, 20.0], [1.0, 3.0]])
    per = vz.colorize_ranged_np(x, ranges)
    assert per[1].tobytes() == vz.colorize_np(x[1], "fixed", vmin=1.0, vmax=3.0)[0].tobytes()
    pos = vz.colorize_ranged_np(x, ranges, positive_only=True)
    bad = np.array(vz.BAD_VIZ[::-1], np.uint8)
    assert (pos[~(x > 0)] == bad).all() and (pos[x > 0] == per[x > 0]).all() and (per[x == 0] != bad).any()
    y = qc.maps("lognormal", 1, 37, 53)[0]  # 1 / x in float64 is not the float32 quotient widened
    rec = vz.colorize_ranged_np(y, (0.05, 2.0), True, True)
    t = np.clip((1.0 / y.astype(np.float64) - 0.05) / (2.0 - 0.05), 0, 1)
    assert (rec == vz.lut("turbo", vz.BAD_VIZ)[:, ::-1][np.minimum((t * 256).astype(int), 255)]).all()


def test_arguments():
    for bad in ((), (1, 2, 3, 4), (-1.0,), (101.0,), (np.nan,)):
        with pytest.raises(ValueError):
            vz.quantiles_np(np.ones((2, 2), np.float32), bad)
    with pytest.raises(ValueError):
        vz.quantiles_np(np.ones((2, 2), np.float32), (50.0,), sample_cap=-1)
