"""Generate tests/golden/gt_eval_cases.npz (run once, where the reference
repository is checked out):

    python tests/golden/make_gt_golden.py /path/to/Monocular_Depth_Estimation_TRT

Records what the reference's own scoring computes -- its core/gt.py, pure
numpy, imported here and only here -- for the cases of
tests/depth_eval_cases.py: the per-image call sequence of its
tools/evaluate_gt.py:555-583 (mask & gt > 0, orientation, align or the named
scale-only path on the finite predictions, metrics).  The fixture holds the
inputs (float32 prediction and ground truth, uint8 mask), one row of results
per case (depth_eval_cases.COLS; NaN where the reference returns no such
key) and the ValueError text where it skips the image.

Before writing, the two properties the derived tolerances stand on are
asserted for every case that is scored: no ratio within 1e-9 (relative) of a
delta threshold, and -- for the seeded distributions -- a conditioning of at
most 100 for the fit's and the orientation's differences.
"""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import depth_eval_cases as dc  # noqa: E402


def reference_score(gt_mod, pred, g, mask, policy, inverse, finite_only, max_depth):
    """evaluate_gt.py:555-583 for one image -> (row of dc.COLS, skip message, aligned or None)."""
    row = dict.fromkeys(dc.COLS, float("nan"))
    m = np.asarray(mask, bool) & (g > 0)
    row["orientation"] = gt_mod.orientation(pred, g, m)
    try:
        if policy == "scale" and finite_only:
            aligned, fit = gt_mod.scale_only(pred, g, m & np.isfinite(pred))
        else:
            aligned, fit = gt_mod.align(pred, g, m, policy, inverse)
    except ValueError as e:
        msg = str(e)
        row["status"] = 2.0 if "underdetermined" in msg else 1.0
        row["n"] = 0.0
        return row, msg, None
    r = gt_mod.metrics(aligned, g, m, max_depth=max_depth)
    row["status"] = 0.0
    row["scale"] = fit.get("scale", float("nan"))
    row["shift"] = fit.get("shift", float("nan"))
    for k in ("n", "abs_rel", "rmse", "log10", "delta1", "delta2", "delta3"):
        row[k] = float(r.get(k, float("nan")))
    return row, "", aligned


def main(reference_root):
    sys.path.insert(0, reference_root)
    from core import gt as gt_mod  # the reference's scoring: generation time only

    inputs = dc.all_inputs()
    keys = list(inputs)
    cases = dc.all_cases()
    rows, skips = [], []
    worst_band, worst_fit, worst_orient = float("inf"), 0.0, 0.0
    with np.errstate(all="ignore"):
        for name, key, policy, inverse, finite_only, md in cases:
            pred, g, mask = inputs[key]
            row, msg, aligned = reference_score(gt_mod, pred, g, mask, policy, inverse, finite_only, md)
            rows.append([row[c] for c in dc.COLS])
            skips.append(msg)
            if aligned is None:
                continue
            band = dc.band_distance(aligned, g, np.asarray(mask, bool) & (g > 0), md)
            assert band > dc.BAND, (name, band)
            worst_band = min(worst_band, band)
            if not key.startswith("edge/"):
                fit, orient = dc.conditioning(pred, g, mask, policy, inverse)
                assert fit <= dc.COND_CAP and orient <= dc.COND_CAP, (name, fit, orient)
                worst_fit, worst_orient = max(worst_fit, fit), max(worst_orient, orient)
    out = {"input_keys": np.array(keys), "case_name": np.array([c[0] for c in cases]),
           "case_input": np.array([c[1] for c in cases]), "case_policy": np.array([c[2] for c in cases]),
           "case_inverse": np.array([c[3] for c in cases], np.uint8),
           "case_finite_only": np.array([c[4] for c in cases], np.uint8),
           "case_max_depth": np.array([c[5] or 0.0 for c in cases], np.float64),
           "case_result": np.array(rows, np.float64), "case_skip": np.array(skips)}
    for i, k in enumerate(keys):
        pred, g, mask = inputs[k]
        out[f"pred{i}"], out[f"gt{i}"], out[f"mask{i}"] = pred, g, np.asarray(mask, np.uint8)
    np.savez_compressed(dc.FIXTURE, **out)
    print(f"{dc.FIXTURE}: {len(cases)} cases ({sum(bool(s) for s in skips)} skipped by the reference), "
          f"{os.path.getsize(dc.FIXTURE)} bytes; closest ratio to a threshold {worst_band:.3e}, "
          f"conditioning fit {worst_fit:.2f} orientation {worst_orient:.2f}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
