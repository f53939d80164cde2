"""The cases tests/golden/gt_eval_cases.npz records the reference's results for
(tests/golden/make_gt_golden.py writes it; test_depth_eval_cpu.py and
test_gpu_depth_eval.py read it), and the two properties the derived tolerances
of DESIGN.md, "Scoring against ground truth", stand on.

A case is (name, input key, policy, pred_is_inverse, fit_finite_only,
max_depth or None); an input is (pred, gt, mask), float32 / float32 / bool."""

import os

import numpy as np

from monocular_depth_estimation_trt_amd import evaluate as ev

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_eval_cases.npz")
SIZES = {(9, 5): 20260905, (37, 53): 20263753, (100, 76): 20261076}  # (h, w) -> seed
LARGE = ((600, 800), 20260680)  # regenerated on the GPU box, too large to commit
EDGE_HW, EDGE_SEED = (8, 12), 20260812
MAX_DEPTH = 15.0
# columns of the recorded results
COLS = ("status", "scale", "shift", "n", "abs_rel", "rmse", "log10", "delta1", "delta2", "delta3", "orientation")
BAND = 1e-9          # no ratio within this relative distance of a delta threshold
COND_CAP = 100.0     # cap on the conditioning of the fit's and the orientation's differences
THRESHOLDS = (1.25, 1.5625, 1.953125)


def synthetic_inputs(h, w, seed):
    """{"metric" | "inverse" | "depth": (pred, gt, mask)} of one seeded image."""
    c = ev.synthetic_gt_case(h, w, seed)
    return {k: (c[k], c["gt"], c["mask"]) for k in ("metric", "inverse", "depth")}


def regular_cases(h, w):
    """Every policy x both pred_is_inverse x max_depth on and off, each policy
    on the prediction that claims it: none and scale on the metric one,
    scale_shift on the inverse-depth or the depth one as the flag says."""
    out = []
    for policy in ev.POLICIES:
        for inverse in (False, True):
            kind = "metric" if policy != "scale_shift" else ("inverse" if inverse else "depth")
            for md in (None, MAX_DEPTH):
                out.append((f"{h}x{w}/{policy}/inv{int(inverse)}/md{md or 0:g}", f"{h}x{w}/{kind}", policy, inverse,
                            policy == "scale", md))
    return out


def edge_inputs():
    """Small hand-made inputs around the contract's corners."""
    h, w = EDGE_HW
    c = ev.synthetic_gt_case(h, w, EDGE_SEED)
    gt, metric = c["gt"], c["metric"]
    full = np.ones((h, w), bool)

    def only(*pix):
        m = np.zeros((h, w), bool)
        for p in pix:
            m[p] = True
        return m

    ins = {
        "one_pixel": (metric, gt, only((3, 4))),
        "two_pixels": (metric, gt, only((0, 0), (7, 11))),
        "all_masked": (metric, gt, np.zeros((h, w), bool)),
        # 0.5 and its reciprocal 2: every sum of the fit is exact in any order, so n Sxx - Sx^2 is exactly 0
        "constant": (np.full((h, w), 0.5, np.float32), gt, c["mask"]),
    }
    nan_pred = metric.copy()
    nan_pred[1, 2] = nan_pred[6, 9] = np.nan
    ins["nan_pred"] = (nan_pred, gt, c["mask"] | only((1, 2), (6, 9)))
    for kind in ("depth", "inverse"):
        p = c[kind].copy()
        p[0, 1], p[2, 3], p[5, 5] = 0.0, -0.75, -3.0
        ins[f"nonpositive_{kind}"] = (p, gt, c["mask"] | only((0, 1), (2, 3), (5, 5)))
    p, g = metric.copy(), gt.copy()
    p[0, 0], p[0, 1], p[0, 2], p[0, 3], p[0, 4], p[0, 5] = np.nan, np.inf, -np.inf, 0.0, -2.0, 1e-7
    g[1, 0] = g[1, 1] = 0.0
    g[2, 0] = g[2, 1] = np.float32(MAX_DEPTH)                                  # exactly at the limit: scored
    g[3, 0] = g[3, 1] = np.nextafter(np.float32(MAX_DEPTH), np.float32(np.inf))  # one ulp beyond: dropped
    ins["mixed"] = (p, g, full)
    return {f"edge/{k}": v for k, v in ins.items()}


def edge_cases():
    out = []
    for key in edge_inputs():
        for policy, inverse, finite_only in (("none", False, False), ("scale", False, False), ("scale", False, True),
                                             ("scale_shift", False, False), ("scale_shift", True, False)):
            for md in (None, MAX_DEPTH):
                out.append((f"{key}/{policy}/inv{int(inverse)}/fin{int(finite_only)}/md{md or 0:g}", key, policy,
                            inverse, finite_only, md))
    return out


def all_inputs():
    ins = {}
    for (h, w), seed in SIZES.items():
        for kind, v in synthetic_inputs(h, w, seed).items():
            ins[f"{h}x{w}/{kind}"] = v
    ins.update(edge_inputs())
    return ins


def all_cases():
    return [c for (h, w) in SIZES for c in regular_cases(h, w)] + edge_cases()


def band_distance(aligned, gt, mask, max_depth=None):
    """The smallest relative distance of any scored pixel's ratio to a delta
    threshold (inf when nothing is scored): above BAND, a ratio computed from a
    scale and shift that differ in the last bits falls on the same side."""
    p, g = np.asarray(aligned, np.float64), np.asarray(gt, np.float64)
    with np.errstate(all="ignore"):
        m = (np.asarray(mask) != 0) & np.isfinite(p) & (g > 0)
        if max_depth:
            m &= g <= max_depth
        if not m.any():
            return float("inf")
        p, g = np.maximum(p[m], 1e-6), g[m]
        ratio = np.maximum(p / g, g / p)
        return float(min(np.min(np.abs(ratio / t - 1.0)) for t in THRESHOLDS))


def conditioning(pred, gt, mask, policy, inverse):
    """(fit, orientation): how much the differences the closed forms take
    amplify the relative error of their sums -- (n Sxx + Sx^2) / (n Sxx - Sx^2)
    for the scale_shift fit (1 otherwise), the larger of Saa / saa and Sbb / sbb
    for the orientation."""
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    with np.errstate(all="ignore"):
        m = (np.asarray(mask) != 0) & (g > 0) & np.isfinite(p)
        a, b = p[m], g[m]
        n = a.size
        orient = max(np.sum(a * a) / (np.sum(a * a) - np.sum(a) ** 2 / n),
                     np.sum(b * b) / (np.sum(b * b) - np.sum(b) ** 2 / n))
        fit = 1.0
        if policy == "scale_shift":
            v = m if inverse else m & (p > 0)
            x = p[v] if inverse else 1.0 / p[v]
            fit = (x.size * np.sum(x * x) + np.sum(x) ** 2) / (x.size * np.sum(x * x) - np.sum(x) ** 2)
    return float(fit), float(orient)


def load_fixture():
    """{"inputs": {key: (pred, gt, mask)}, "cases": [(case tuple, {column: value}, skip message or "")]}"""
    z = np.load(FIXTURE, allow_pickle=False)
    keys = [str(k) for k in z["input_keys"]]
    inputs = {k: (z[f"pred{i}"], z[f"gt{i}"], z[f"mask{i}"] != 0) for i, k in enumerate(keys)}
    cases = []
    for i, name in enumerate(z["case_name"]):
        md = float(z["case_max_depth"][i])
        case = (str(name), str(z["case_input"][i]), str(z["case_policy"][i]), bool(z["case_inverse"][i]),
                bool(z["case_finite_only"][i]), md if md > 0 else None)
        cases.append((case, dict(zip(COLS, (float(v) for v in z["case_result"][i]))), str(z["case_skip"][i])))
    return {"inputs": inputs, "cases": cases}
