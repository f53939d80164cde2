"""Scoring against ground truth, the parts that need no GPU: evaluate.py's
numpy restatement against the reference's recorded results
(tests/golden/gt_eval_cases.npz, written by tests/golden/make_gt_golden.py from
the reference's core/gt.py), the policy table, and the ABI's argument checks."""

import ctypes
import math
import os

import numpy as np
import pytest

import depth_eval_cases as dc
from conftest import ROOT

RTOL = 1e-13  # score_np and the reference differ in summation order only (pairwise sums against dot products)


@pytest.fixture(scope="module")
def fixture():
    return dc.load_fixture()


@pytest.fixture(scope="module")
def ev():
    from monocular_depth_estimation_trt_amd import evaluate
    return evaluate


@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


def close(a, b, rtol):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b or abs(a - b) <= rtol * abs(b)


def as_columns(ev, r):
    """A score_np / DeviceEval.result() dict as the fixture's columns."""
    nan = float("nan")
    if "skip" in r:
        row = dict.fromkeys(dc.COLS, nan)
        row.update(status=float(r["status"]), n=0.0, orientation=r["orientation"])
        return row
    row = {"status": 0.0, "scale": r["fit"].get("scale", nan), "shift": r["fit"].get("shift", nan), "n": float(r["n"]),
           "orientation": r["orientation"]}
    row.update({k: r[k] for k in ev.METRIC_KEYS})
    return row


def test_fixture_holds_the_cases_the_suite_names(fixture):
    assert [c[0] for c in fixture["cases"]] == dc.all_cases()
    ins = dc.all_inputs()
    assert sorted(fixture["inputs"]) == sorted(ins)
    for k, (p, g, m) in ins.items():  # the seeded inputs regenerate bit for bit
        fp, fg, fm = fixture["inputs"][k]
        assert fp.tobytes() == p.tobytes() and fg.tobytes() == g.tobytes() and np.array_equal(fm, m), k
    skipped = {c[0][0] for c in fixture["cases"] if c[2]}
    for must in ("edge/one_pixel/scale/inv0/fin0/md0", "edge/one_pixel/scale_shift/inv1/fin0/md0",
                 "edge/constant/scale_shift/inv0/fin0/md0", "edge/all_masked/scale/inv0/fin1/md15"):
        assert must in skipped, must


def test_score_np_matches_the_reference(fixture, ev):
    """Every recorded result: status and counts exact, delta fractions exact
    (the band is empty), everything else to 1e-13 relative, NaN where the
    reference has NaN or no such key; the skip text word for word."""
    for case, ref, skip in fixture["cases"]:
        name, key, policy, inverse, finite_only, md = case
        pred, g, mask = fixture["inputs"][key]
        r = ev.score_np(pred, g, mask, policy, inverse, finite_only, md)
        assert r.get("skip", "") == skip, (name, r)
        ours = as_columns(ev, r)
        for col in ("status", "n", "delta1", "delta2", "delta3"):
            assert close(ours[col], ref[col], 0.0), (name, col, ours[col], ref[col])
        for col in ("scale", "shift", "abs_rel", "rmse", "log10", "orientation"):
            assert close(ours[col], ref[col], RTOL), (name, col, ours[col], ref[col])


def test_what_the_tolerances_stand_on(fixture, ev):
    """Asserted when the fixture was written, and again here on our own
    alignment: no scored ratio within 1e-9 of a delta threshold; conditioning
    of the fit and of the orientation at most 100 on the seeded inputs."""
    for case, ref, skip in fixture["cases"]:
        name, key, policy, inverse, finite_only, md = case
        if skip:
            continue
        pred, g, mask = fixture["inputs"][key]
        m = mask & (g > 0)
        aligned, _ = ev.align_np(pred, g, m & np.isfinite(pred) if finite_only and policy == "scale" else m, policy,
                                 inverse)
        assert dc.band_distance(aligned, g, m, md) > dc.BAND, name
        if not key.startswith("edge/"):
            fit, orient = dc.conditioning(pred, g, mask, policy, inverse)
            assert fit <= dc.COND_CAP and orient <= dc.COND_CAP, (name, fit, orient)


def test_edge_semantics(fixture, ev):
    """What the edge cases are there to pin, said outright."""
    by_name = {c[0][0]: (c[1], c[2]) for c in fixture["cases"]}
    # a NaN prediction under the mask: the plain scale fit is NaN and nothing is scored; narrowed, it is scored
    ref, _ = by_name["edge/nan_pred/scale/inv0/fin0/md0"]
    assert math.isnan(ref["scale"]) and ref["n"] == 0 and math.isnan(ref["abs_rel"])
    ref, _ = by_name["edge/nan_pred/scale/inv0/fin1/md0"]
    assert ref["scale"] > 0 and ref["n"] > 0
    # non-positive depth predictions are left out of the fit and of the score
    p, g, m = fixture["inputs"]["edge/nonpositive_depth"]
    r = ev.score_np(p, g, m, "scale_shift", False)
    assert r["n_fit"] == r["n"] == int(np.count_nonzero(m & (p > 0)))
    assert by_name["edge/nonpositive_depth/scale_shift/inv0/fin0/md0"][0]["n"] == r["n"]
    # the range limit is inclusive
    p, g, m = fixture["inputs"]["edge/mixed"]
    n_all = by_name["edge/mixed/none/inv0/fin0/md0"][0]["n"]
    n_lim = by_name["edge/mixed/none/inv0/fin0/md15"][0]["n"]
    ok = m & (g > 0) & np.isfinite(p)
    assert n_all == np.count_nonzero(ok) and n_lim == np.count_nonzero(ok & (g <= np.float32(15.0)))
    assert np.count_nonzero(ok & (g == np.float32(15.0))) == 2 and n_lim < n_all
    # nothing measured: not an error under policy none, n = 0 and NaN metrics
    r = ev.score_np(*fixture["inputs"]["edge/all_masked"], "none")
    assert r["n"] == 0 and math.isnan(r["abs_rel"]) and math.isnan(r["orientation"])
    assert by_name["edge/one_pixel/scale_shift/inv0/fin0/md0"][1] == ev.SKIP_FEW
    assert by_name["edge/constant/scale_shift/inv1/fin0/md0"][1] == ev.SKIP_CONSTANT


def test_policy_table(ev):
    """The reference's policy_for / policy_for_normalised (core/gt.py:152-218)
    and what the committed specs earn: VGGT's `unknown` is not scored unless
    the caller names the scale-only path."""
    from monocular_depth_estimation_trt_amd import spec
    assert ev.policy_for("metric") == "none"
    assert ev.policy_for("relative") == "scale_shift"
    for other in ("unknown", "normalised", None, ""):
        assert ev.policy_for(other) is None
    assert ev.policy_for_normalised("normalised") == "scale"
    assert ev.policy_for_normalised("unknown") is None and ev.policy_for_normalised("metric") is None
    assert ev.policy_for_normalised("unknown", scale_only=True) == "scale"
    assert ev.spec_policy(spec.load("depth_anything_v2")) == ("none", False)
    assert ev.spec_policy(spec.load("depth_pro")) == ("none", False)
    assert ev.spec_policy(spec.load("depth_anything_ac")) == ("scale_shift", True)
    assert ev.spec_policy(spec.load("distill_any_depth")) == ("scale_shift", True)
    with pytest.raises(ValueError, match="not scored"):
        ev.spec_policy(spec.load("vggt"))
    assert ev.spec_policy(spec.load("vggt"), scale_only=True) == ("scale", False)
    with pytest.raises(ValueError, match="output_form"):
        ev.spec_policy({"depth_scale": "relative"})
    with pytest.raises(ValueError, match="unknown alignment policy"):
        ev.score_np(np.ones((2, 2)), np.ones((2, 2)), np.ones((2, 2)), "affine")


def test_header_names_the_tile_and_the_slots():
    txt = open(os.path.join(ROOT, "include", "mde.h")).read()
    assert "#define MDE_DEPTH_EVAL_TILE 1024" in txt
    for slot in ("status", "n_fit", "scale", "shift", "abs_rel", "rmse", "log10", "delta1", "delta2", "delta3",
                 "orientation"):
        assert slot in txt, slot


def test_ws_bytes_is_zero_for_refused_sizes(lib):
    f = lib.mde_op_depth_eval_ws_bytes
    tiles = -(-600 * 800 // 1024)
    assert f(1, 600, 800) == tiles * 20 * 8 and f(3, 600, 800) == 3 * tiles * 20 * 8
    assert f(1, 1, 1) == 20 * 8
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -3), (65536, 8, 8), (1, 46341, 46341),
                (1, 1 << 16, 1 << 15), (1, 2, (1 << 30) - 128)):
        assert f(*bad) == 0, bad
    assert f(65535, 1, 1) == 65535 * 20 * 8
    assert f(1, 1, (1 << 31) - 257) > 0  # the largest plane the op takes


def test_argument_checks_answer_without_a_gpu(lib):
    """MDE_ERR_ARG before any device call (the pointers are never dereferenced)."""
    p, big = 4096, 1 << 30
    nan = float("nan")

    def err(msg, pred=p, gt=p, mask=p, batch=1, h=8, w=8, policy=2, inv=0, fin=0, md=0.0, out=p, ws=p, ws_bytes=big):
        rc = lib.mde_op_depth_eval(pred, gt, mask, batch, h, w, policy, inv, fin, md, out, ws, ws_bytes, None)
        assert rc == 1, (rc, lib.mde_last_error())
        assert msg in lib.mde_last_error(), lib.mde_last_error()

    err(b"null", pred=None)
    err(b"null", gt=None)
    err(b"null", mask=None)
    err(b"null", out=None)
    err(b"positive", batch=0)
    err(b"positive", h=0)
    err(b"positive", w=-8)
    err(b"policy", policy=3)
    err(b"policy", policy=-1)
    err(b"2^31 - 256", h=1 << 16, w=1 << 15)
    err(b"2^31 - 256", h=1, w=(1 << 31) - 256)
    err(b"batch > 65535", batch=65536)
    err(b"NaN", md=nan)
    err(b"mde_op_depth_eval_ws_bytes", ws=None)
    err(b"mde_op_depth_eval_ws_bytes", ws_bytes=20 * 8 - 1)
    err(b"mde_op_depth_eval_ws_bytes", h=600, w=800, ws_bytes=469 * 20 * 8 - 1)
    err(b"aligned", ws=p + 4)
    err(b"aligned", out=p + 4)


def test_driver_options_are_checked_before_an_engine_is_built(ev, tmp_path):
    import argparse
    from monocular_depth_estimation_trt_amd import spec
    ap = argparse.ArgumentParser()
    ev.add_gt_arguments(ap)
    g = np.full((6, 8, 1), 2.0, np.float64)
    np.save(tmp_path / "gt.npy", g)
    np.save(tmp_path / "mask.npy", np.ones((6, 8), np.uint8))
    gt_args = ["--gt", str(tmp_path / "gt.npy"), "--gt-mask", str(tmp_path / "mask.npy")]
    metric, relative, vggt = (spec.load(m) for m in ("depth_pro", "depth_anything_ac", "vggt"))
    assert ev.check_gt_arguments(ap.parse_args([]), metric, True) is None
    assert ev.check_gt_arguments(ap.parse_args(gt_args), metric, True) == ("none", False)
    assert ev.check_gt_arguments(ap.parse_args(gt_args + ["--max-depth", "15"]), relative, True) == ("scale_shift", True)
    for argv, device_map, sp, msg in ((gt_args, False, metric, "host-postprocess"),
                                      (gt_args[:2], True, metric, "--gt-mask"),
                                      (["--max-depth", "15"], True, metric, "go with --gt"),
                                      (gt_args + ["--max-depth", "0"], True, metric, "positive"),
                                      (gt_args, True, vggt, "not scored")):
        with pytest.raises(SystemExit, match=msg):
            ev.check_gt_arguments(ap.parse_args(argv), sp, device_map)
    gt, mask = ev.load_gt_arguments(ap.parse_args(gt_args), (6, 8))  # the trailing channel axis is dropped
    assert gt.dtype == np.float32 and gt.shape == (6, 8) and mask.dtype == bool and mask.all()
    with pytest.raises(SystemExit, match="not resized"):
        ev.load_gt_arguments(ap.parse_args(gt_args), (6, 9))
    line = ev.format_score(ev.score_np(np.full((6, 8), 0.5), gt, mask, "scale"))
    assert line.startswith("n 48 abs_rel 0.00000 ") and line.endswith("fit scale 4")
    assert ev.format_score(ev.score_np(np.full((6, 8), 0.5), gt, mask, "scale_shift")).startswith("skip (scale_shift is")


def test_python_wrapper_refuses_what_the_op_refuses(ev):
    with pytest.raises(ValueError, match="does not take"):
        ev.DeviceEval(1, 0, 8)
    with pytest.raises(ValueError, match="does not take"):
        ev.DeviceEval(70000, 8, 8)
    assert ev.ws_bytes(2, 37, 53) == 2 * 2 * 20 * 8
    assert ctypes.sizeof(ctypes.c_double) * ev.OUT_SLOTS == 128
