"""Scoring against ground truth on the device (csrc/depth_eval.hip) through the C ABI, the Python
owner (evaluate.DeviceEval) and the drivers' --gt.

Every check is against evaluate.score_np and, where tests/golden/gt_eval_cases.npz has the case,
against the reference's recorded results.  Tolerances ("Scoring against ground truth"):
status, n, n_fit and n_mask exact; the delta fractions exact (each test asserts that no ratio lies
within 1e-9 of a threshold); scale, shift, abs_rel, rmse, log10 and the orientation to 1e-11
relative, with the conditioning of the fit and of the orientation asserted to be at most 100.  Where
the fit passes through its pixels exactly (two fit pixels under scale_shift) the metrics are rounding
noise around 0 and p / |p - g| is unbounded; they are then held to the absolute 1e-11 (times the
largest ground truth for the rmse), which is what the error of scale and shift allows.

Every call writes into `out` and a scratch buffer filled with 0xA5 inside guard bytes; the helper
checks that nothing outside out[batch][16] and the first mde_op_depth_eval_ws_bytes of scratch changed.

Workgroup sizes, for the shapes below: a workgroup of 128 threads owns a tile of 1024 pixels and the
finalising workgroup adds the tiles' partial sums 256 at a time.  9 x 5 = 45 pixels is less than a
wave; 37 x 53 = 1961 is two tiles, the second partly filled, and odd, so that image 1 of a batch
starts off the 16-byte boundary the vector loads want (the scalar path); 100 x 76 = 7600 is 8 tiles,
a multiple of 4 (the vector path for every image); 600 x 800 = 480000 is 469 tiles, more than one
finalising pass of 256 threads.
"""

import ctypes as C
import functools
import json
import math

import numpy as np
import pytest
import torch

import depth_eval_cases as dc
from gpu_util import op, ptr, stream

from monocular_depth_estimation_trt_amd import evaluate as ev

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64
RTOL = 1e-11
COMBOS = [(policy, inverse, md) for policy in ev.POLICIES for inverse in (False, True) for md in (None, dc.MAX_DEPTH)]


@functools.lru_cache(maxsize=None)
def fixture():
    return dc.load_fixture()


@functools.lru_cache(maxsize=None)
def seeded(h, w):
    """The seeded image of one size: {"gt", "mask", "metric", "inverse", "depth"}, never written."""
    seed = dc.LARGE[1] if (h, w) == dc.LARGE[0] else dc.SIZES[(h, w)]
    c = ev.synthetic_gt_case(h, w, seed)
    for v in c.values():
        v.setflags(write=False)
    return c


def claimed(c, policy, inverse):
    """The prediction that claims the policy (depth_eval_cases.regular_cases)."""
    return c["metric" if policy != "scale_shift" else ("inverse" if inverse else "depth")]


def device_eval(pred, gt, mask, policy, inverse=False, finite_only=False, max_depth=None):
    """mde_op_depth_eval on [B][h][w] inputs; checks the guards; returns out as float64 [B][16]."""
    pred, gt, mask = (np.asarray(a) for a in (pred, gt, mask))
    if pred.ndim == 2:
        pred, gt, mask = pred[None], gt[None], mask[None]
    B, h, w = pred.shape
    d_pred = torch.from_numpy(np.array(pred, np.float32)).cuda()
    d_gt = torch.from_numpy(np.array(gt, np.float32)).cuda()
    d_mask = torch.from_numpy((mask != 0).astype(np.uint8) * np.uint8(0xC3)).cuda()  # any nonzero byte is "measured"
    need = ev.ws_bytes(B, h, w)
    assert need == B * -(-h * w // 1024) * 20 * 8
    d_out = torch.full((PAD + B * 128 + PAD,), FILL, dtype=torch.uint8, device="cuda")
    d_ws = torch.full((need + PAD,), FILL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 16 == 0 and d_ws.data_ptr() % 8 == 0
    op("mde_op_depth_eval", ptr(d_pred), ptr(d_gt), ptr(d_mask), B, h, w, ev.POLICIES.index(policy), int(inverse),
       int(finite_only), float(max_depth or 0.0), C.c_void_p(d_out.data_ptr() + PAD), ptr(d_ws), need, stream())
    out, wsb = d_out.cpu().numpy(), d_ws.cpu().numpy()
    assert (out[:PAD] == FILL).all() and (out[PAD + B * 128:] == FILL).all(), "bytes outside out[batch][16] written"
    assert (wsb[need:] == FILL).all(), "scratch written past mde_op_depth_eval_ws_bytes"
    return out[PAD:PAD + B * 128].view(np.float64).reshape(B, 16).copy()


def close(a, b, rtol, floor=0.0):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return a == b or abs(a - b) <= rtol * max(abs(b), floor)


def check_row(row, pred, gt, mask, policy, inverse=False, finite_only=False, max_depth=None, ref=None, what="",
              cond_cap=dc.COND_CAP):
    """One image's out[16] against score_np (and the recorded reference row `ref`).  Returns score_np's dict."""
    want = ev.score_np(pred, gt, mask, policy, inverse, finite_only, max_depth)
    got = ev.result_dict(row, policy)
    m = (np.asarray(mask) != 0) & (np.asarray(gt) > 0)
    assert row[ev.N_MASK] == np.count_nonzero(m), what
    assert (row[13:] == 0).all(), what
    assert got.get("skip", "") == want.get("skip", ""), (what, got, want)
    assert close(got["orientation"], want["orientation"], RTOL), (what, got["orientation"], want["orientation"])
    if ref is not None:
        assert row[ev.STATUS] == ref["status"], (what, row[ev.STATUS], ref["status"])
        assert close(got["orientation"], ref["orientation"], RTOL), (what, got["orientation"], ref["orientation"])
    if "skip" in want:
        assert got["status"] == want["status"] and row[ev.N] == 0, what
        assert np.isnan(row[[ev.SCALE, ev.SHIFT]]).all() and np.isnan(row[ev.ABS_REL:ev.DELTA3 + 1]).all(), what
        return want
    # what the tolerances stand on, asserted on the very inputs of this check
    with np.errstate(all="ignore"):
        fit_mask = m & np.isfinite(pred) if (policy == "scale" and finite_only) else m
        aligned, _ = ev.align_np(pred, gt, fit_mask, policy, inverse)
        assert dc.band_distance(aligned, gt, m, max_depth) > dc.BAND, what
    if cond_cap and np.count_nonzero(m & np.isfinite(pred)) > 2:
        fit_cond, orient_cond = dc.conditioning(pred, gt, mask, policy, inverse)
        assert fit_cond <= cond_cap and orient_cond <= cond_cap, (what, fit_cond, orient_cond)
    assert got["n"] == want["n"] and got["n_fit"] == want["n_fit"], (what, got, want)
    exact_fit = policy == "scale_shift" and want["n_fit"] == 2
    floors = {"abs_rel": 1.0, "log10": 1.0, "rmse": float(np.max(np.asarray(gt)[m]))} if exact_fit else {}
    sides = [("score_np", dict(want, **want["fit"]))]
    if ref is not None:
        assert got["n"] == ref["n"], (what, got["n"], ref["n"])
        sides.append(("reference", ref))
    for side, w_ in sides:
        for k in ("delta1", "delta2", "delta3"):
            assert close(got[k], w_[k], 0.0), (what, side, k, got[k], w_[k])
        for k in ("abs_rel", "rmse", "log10"):
            assert close(got[k], w_[k], RTOL, floors.get(k, 0.0)), (what, side, k, got[k], w_[k])
        for k in got["fit"]:
            assert close(got["fit"][k], w_[k], RTOL), (what, side, k, got["fit"][k], w_[k])
    return want


@pytest.mark.parametrize("group", ["9x5", "37x53", "100x76", "edge"])
def test_recorded_cases(gpu, group):
    """Every case of the fixture, sizes 9 x 5 (less than a wave), 37 x 53 and 100 x 76 and the edge
    inputs: the device against score_np and against what the reference recorded."""
    fx = fixture()
    n = 0
    for case, ref, skip in fx["cases"]:
        name, key, policy, inverse, finite_only, md = case
        if not key.startswith(group + "/"):
            continue
        pred, gt, mask = fx["inputs"][key]
        row = device_eval(pred, gt, mask, policy, inverse, finite_only, md)[0]
        want = check_row(row, pred, gt, mask, policy, inverse, finite_only, md, ref=ref, what=name,
                         cond_cap=None if group == "edge" else dc.COND_CAP)
        assert want.get("skip", "") == skip, name
        n += 1
    assert n == (10 * len(dc.edge_inputs()) if group == "edge" else 12)


@pytest.mark.parametrize("policy, inverse, md", COMBOS)
def test_many_tiles(gpu, policy, inverse, md):
    """600 x 800, regenerated from its seed: 469 tiles, two passes of the finalising workgroup."""
    c = seeded(600, 800)
    pred = claimed(c, policy, inverse)
    row = device_eval(pred, c["gt"], c["mask"], policy, inverse, policy == "scale", md)[0]
    want = check_row(row, pred, c["gt"], c["mask"], policy, inverse, policy == "scale", md, what="600x800")
    assert want["n"] > 200000 and (md is None or want["n"] < np.count_nonzero(c["mask"]))


@pytest.mark.parametrize("shape", [(9, 5), (37, 53), (100, 76)], ids=lambda s: "%dx%d" % s)
def test_batch2_different_masks(gpu, shape):
    """Two images with different predictions, ground truth and masks in one call; with an odd plane
    (9 x 5, 37 x 53) image 1 starts off the 16-byte boundary."""
    h, w = shape
    c = seeded(h, w)
    rng = np.random.Generator(np.random.PCG64(h * 1009 + w))
    mask1 = rng.random((h, w)) < 0.5
    gt1 = np.ascontiguousarray(c["gt"][::-1, ::-1])
    for policy, inverse, md in COMBOS:
        p0 = claimed(c, policy, inverse)
        noisy = gt1 * np.exp(rng.normal(0.0, 0.15, (h, w)))
        p1 = {"metric": noisy, "inverse": 2.0 / noisy + 0.1, "depth": 1.0 / (2.0 / noisy + 0.1)}[
            "metric" if policy != "scale_shift" else ("inverse" if inverse else "depth")].astype(np.float32)
        out = device_eval(np.stack([p0, p1]), np.stack([c["gt"], gt1]), np.stack([c["mask"], mask1]), policy,
                          inverse, policy == "scale", md)
        w0 = check_row(out[0], p0, c["gt"], c["mask"], policy, inverse, policy == "scale", md, what=f"image 0 {policy}")
        w1 = check_row(out[1], p1, gt1, mask1, policy, inverse, policy == "scale", md, what=f"image 1 {policy}")
        assert w0["n"] != w1["n"] and not np.array_equal(out[0], out[1])


def pattern_mask(name, h, w):
    m = np.zeros((h, w), bool)
    flat = m.reshape(-1)
    if name == "all":
        flat[:] = True
    elif name == "one":
        flat[h * w // 3] = True
    elif name == "two":
        flat[5], flat[h * w - 7] = True, True
    elif name == "last":  # only the last pixel of the last tile
        flat[-1] = True
    elif name == "checker":
        vv, uu = np.mgrid[0:h, 0:w]
        m[(vv + uu) % 2 == 0] = True
    elif name == "random":
        flat[np.random.Generator(np.random.PCG64(77 + h)).random(h * w) < 0.5] = True
    else:
        assert name == "none"
    return m


@pytest.mark.parametrize("shape", [(37, 53), (100, 76), (600, 800)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["all", "none", "one", "two", "last", "checker", "random"])
def test_mask_patterns(gpu, name, shape):
    h, w = shape
    c = seeded(h, w)
    mask = pattern_mask(name, h, w)
    combos = COMBOS if shape != (600, 800) else [("none", False, None), ("scale_shift", True, dc.MAX_DEPTH)]
    for policy, inverse, md in combos:
        pred = claimed(c, policy, inverse)
        row = device_eval(pred, c["gt"], mask, policy, inverse, policy == "scale", md)[0]
        want = check_row(row, pred, c["gt"], mask, policy, inverse, policy == "scale", md, what=f"{name} {policy}")
        few = name in ("none", "one", "last")
        if few and policy != "none":
            assert row[ev.STATUS] == 1 and want["skip"] == ev.SKIP_FEW
        elif few:
            assert row[ev.STATUS] == 0 and row[ev.N] <= 1 and math.isnan(row[ev.ORIENTATION])
            if name == "none":
                assert row[ev.N] == 0 and np.isnan(row[ev.ABS_REL:ev.DELTA3 + 1]).all()
        else:
            assert row[ev.STATUS] == 0 and row[ev.N_FIT] == (0 if policy == "none" else np.count_nonzero(mask))


def spiked(pred, gt, values, gt_values=()):
    """Copies with `values` written into the prediction at pixels spread over every tile (and over
    both passes and several lanes of a tile), `gt_values` into the ground truth at others."""
    p, g = np.array(pred), np.array(gt)
    n = p.size
    spots = [int(i) for i in np.linspace(3, n - 2, 4 * len(values)).astype(np.int64)]
    for k, i in enumerate(spots):
        p.reshape(-1)[i] = values[k % len(values)]
    for k, v in enumerate(gt_values):
        for i in (11 + 2 * k, n // 2 + 2 * k + 1, n - 20 + 2 * k):
            g.reshape(-1)[i] = v
    return p, g


@pytest.mark.parametrize("shape", [(37, 53), (100, 76)], ids=lambda s: "%dx%d" % s)
def test_prediction_and_ground_truth_values(gpu, shape):
    """NaN, +-inf, 0, negatives and values below 1e-6 in the prediction under a full mask; ground truth
    with zeros and with values exactly at and one ulp beyond max_depth.  (A prediction below 1e-6 is
    1e7 in disparity and would alone decide a fit in disparity, so the depth-output scale_shift case
    takes the other values only.)"""
    h, w = shape
    c = seeded(h, w)
    mask = np.ones((h, w), bool)
    md32 = np.float32(dc.MAX_DEPTH)
    gt_values = (0.0, md32, np.nextafter(md32, np.float32(np.inf)))
    bad = [np.nan, np.inf, -np.inf, 0.0, -1.5]
    for policy, inverse, md in COMBOS:
        tiny = [] if (policy == "scale_shift" and not inverse) else [1e-7, 3e-9]
        pred, gt = spiked(claimed(c, policy, inverse), c["gt"], bad + tiny, gt_values)
        for finite_only in ((False, True) if policy == "scale" else (False,)):
            row = device_eval(pred, gt, mask, policy, inverse, finite_only, md)[0]
            want = check_row(row, pred, gt, mask, policy, inverse, finite_only, md,
                             what=f"{policy} inv{inverse} fin{finite_only} md{md}")
            measured = int(np.count_nonzero(gt > 0))
            assert row[ev.N_MASK] == measured == h * w - 3
            if policy == "scale" and not finite_only:
                assert math.isnan(row[ev.SCALE]) and row[ev.N] == 0  # one NaN under the mask: as the reference
            else:
                assert 0 < want["n"] < measured
    at = ev.score_np(*spiked(c["metric"], c["gt"], bad, gt_values), mask, "none", max_depth=dc.MAX_DEPTH)
    beyond = ev.score_np(*spiked(c["metric"], c["gt"], bad, gt_values[:2] + (md32,)), mask, "none",
                         max_depth=dc.MAX_DEPTH)
    assert beyond["n"] - at["n"] == 3  # the limit is inclusive, one ulp beyond it is out


@pytest.mark.parametrize("shape", [(100, 76), (600, 800)], ids=lambda s: "%dx%d" % s)
def test_constant_prediction_is_status_2(gpu, shape):
    """0.5 everywhere (2 in disparity): every sum is exact, n Sxx - Sx^2 is exactly 0."""
    h, w = shape
    c = seeded(h, w)
    pred = np.full((h, w), 0.5, np.float32)
    for inverse in (False, True):
        row = device_eval(pred, c["gt"], c["mask"], "scale_shift", inverse)[0]
        want = check_row(row, pred, c["gt"], c["mask"], "scale_shift", inverse, what="constant")
        assert row[ev.STATUS] == 2 and want["skip"] == ev.SKIP_CONSTANT and row[ev.N_FIT] == np.count_nonzero(c["mask"])
    row = device_eval(pred, c["gt"], c["mask"], "scale")[0]  # one parameter is determined
    check_row(row, pred, c["gt"], c["mask"], "scale", what="constant, scale", cond_cap=None)
    assert row[ev.STATUS] == 0 and math.isnan(row[ev.ORIENTATION])


def test_two_runs_give_the_same_bytes(gpu):
    c = seeded(600, 800)
    for policy, inverse in (("scale_shift", True), ("scale", False)):
        a = device_eval(claimed(c, policy, inverse), c["gt"], c["mask"], policy, inverse, False, dc.MAX_DEPTH)
        b = device_eval(claimed(c, policy, inverse), c["gt"], c["mask"], policy, inverse, False, dc.MAX_DEPTH)
        assert a.tobytes() == b.tobytes()


def test_device_eval_in_a_captured_graph(gpu):
    """One DeviceEval.enqueue (four kernels) captured into a torch.cuda.graph on a side stream,
    replayed on a changed prediction."""
    h, w = 100, 76
    c = seeded(h, w)
    pa = c["inverse"]
    pb = (c["inverse"] * np.float32(1.7) + np.float32(0.05)).astype(np.float32)
    d_pred = torch.from_numpy(np.array(pa)).cuda()
    with ev.DeviceEval(1, h, w) as de:
        de.upload_gt(c["gt"], c["mask"])
        kw = dict(pred_is_inverse=True, max_depth=dc.MAX_DEPTH)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            de.enqueue(d_pred.data_ptr(), s.cuda_stream, "scale_shift", **kw)  # warm: the kernels are loaded
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            de.enqueue(d_pred.data_ptr(), s.cuda_stream, "scale_shift", **kw)
        fits = []
        for p in (pa, pb):
            d_pred.copy_(torch.from_numpy(np.array(p)))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            de.download(0)
            check_row(de.raw()[0], p, c["gt"], c["mask"], "scale_shift", True, False, dc.MAX_DEPTH, what="replay")
            fits.append(de.result()[0]["fit"])
        assert fits[0] != fits[1]
    with pytest.raises(RuntimeError):
        de.result()  # freed


def test_device_eval_run_batch2(gpu):
    """run() = enqueue, download, result: one dict per image in the reference's words."""
    h, w = 37, 53
    c = seeded(h, w)
    one = pattern_mask("one", h, w)
    pred = np.stack([c["metric"], c["metric"]])
    d_pred = torch.from_numpy(pred).cuda()
    torch.cuda.synchronize()
    with ev.DeviceEval(2, h, w) as de:
        de.upload_gt(np.stack([c["gt"], c["gt"]]), np.stack([c["mask"], one]))
        with pytest.raises(RuntimeError):
            de.result()  # nothing enqueued yet
        r = de.run(d_pred.data_ptr(), 0, "scale", fit_finite_only=True, max_depth=dc.MAX_DEPTH)
        check_row(de.raw()[0], c["metric"], c["gt"], c["mask"], "scale", False, True, dc.MAX_DEPTH, what="run")
        assert set(r[0]) == {"n", "abs_rel", "rmse", "log10", "delta1", "delta2", "delta3", "orientation", "fit",
                             "n_fit"} and set(r[0]["fit"]) == {"scale"}
        assert r[1] == {"skip": ev.SKIP_FEW, "status": 1, "orientation": r[1]["orientation"]}
        assert math.isnan(r[1]["orientation"])
        r = de.run(d_pred.data_ptr(), 0, "none")
        assert r[0]["fit"] == {} and r[1]["n"] == 1
        with pytest.raises(ValueError):
            de.enqueue(d_pred.data_ptr(), 0, "affine")


# ---- the drivers' --gt ---------------------------------------------------------------------------

def photo(h, w):
    return np.random.Generator(np.random.PCG64(h * 131 + w + 7)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def check_driver_score(path, out, depth, gt, mask, policy, inverse, md, model):
    """The JSON the driver wrote (and the line it printed) against score_np of the map it returned."""
    line = [l for l in out.splitlines() if l.startswith("[MDET] gt : ")]
    assert len(line) == 1 and f"policy {policy}" in line[0], out
    r = json.load(open(path))
    assert (r["model"], r["policy"], r["pred_is_inverse"], r["max_depth"]) == (model, policy, inverse, md)
    want = ev.score_np(depth, gt, mask, policy, inverse, policy == "scale", md)
    assert "skip" not in want and r["n"] == want["n"] > 1000 and r["n_fit"] == want["n_fit"]
    assert f"n {r['n']} abs_rel {r['abs_rel']:0.5f}" in line[0]
    with np.errstate(all="ignore"):
        aligned, _ = ev.align_np(depth, gt, mask & (gt > 0), policy, inverse)
    assert dc.band_distance(aligned, gt, mask & (gt > 0), md) > dc.BAND
    # the map is the engine's, not seeded: the bound is linear in the conditioning, 1e-11 up to the cap of 100
    fit_cond, orient_cond = dc.conditioning(depth, gt, mask, policy, inverse)
    for k in ("delta1", "delta2", "delta3"):
        assert r[k] == want[k], (k, r[k], want[k])
    for k in ("abs_rel", "rmse", "log10"):
        assert close(r[k], want[k], RTOL * max(1.0, fit_cond / dc.COND_CAP)), (k, r[k], want[k], fit_cond)
    for k, v in want["fit"].items():
        assert close(r["fit"][k], v, RTOL * max(1.0, fit_cond / dc.COND_CAP)), (k, r["fit"][k], v, fit_cond)
    assert close(r["orientation"], want["orientation"], RTOL * max(1.0, orient_cond / dc.COND_CAP)), orient_cond
    return r


def test_dav2_driver_gt(gpu, tmp_path, capsys):
    """depth_anything_v2 (spec: metric -> none) on a 120 x 160 photo."""
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    h, w = 120, 160
    c = ev.synthetic_gt_case(h, w, 4242)
    np.save(tmp_path / "src.npy", photo(h, w))
    np.save(tmp_path / "gt.npy", c["gt"])
    np.save(tmp_path / "mask.npy", c["mask"])
    args = ["--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--image",
            str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench"), "--source", "synthetic:vits:metric:1234",
            "--gt", str(tmp_path / "gt.npy"), "--gt-mask", str(tmp_path / "mask.npy")]
    depth = run.main(args + ["--max-depth", "15", "--gt-out", str(tmp_path / "score.json")])
    check_driver_score(tmp_path / "score.json", capsys.readouterr().out, depth, c["gt"], c["mask"], "none", False,
                       15.0, "depth_anything_v2")
    with pytest.raises(SystemExit, match="host-postprocess"):
        run.main(args + ["--host-postprocess"])
    with pytest.raises(SystemExit, match="--gt-mask"):
        run.main(args[:-2])
    np.save(tmp_path / "small.npy", c["gt"][:-1])
    with pytest.raises(SystemExit, match="not resized"):
        run.main(args[:-3] + [str(tmp_path / "small.npy"), "--gt-mask", str(tmp_path / "mask.npy")])


def test_depth_anything_ac_driver_gt(gpu, tmp_path, capsys):
    """depth_anything_ac inherits the DA-V2 driver; its spec says relative, inverse_depth: scale and
    shift fitted in disparity.  The ground truth is made from the map a first run returns, so that the
    fit is determined: 1 / gt affine in the prediction, with noise."""
    from monocular_depth_estimation_trt_amd.models.depth_anything_ac import run
    h, w = 120, 160
    np.save(tmp_path / "src.npy", photo(h, w))
    args = ["--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--image",
            str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench")]
    first = run.main(args)
    rng = np.random.Generator(np.random.PCG64(99))
    lo, hi = float(first.min()), float(first.max())
    assert hi > lo
    disp = 0.05 + 0.45 * (first.astype(np.float64) - lo) / (hi - lo)
    gt = (np.exp(rng.normal(0.0, 0.15, (h, w))) / disp).astype(np.float32)
    mask = rng.random((h, w)) < 0.7
    np.save(tmp_path / "gt.npy", gt)
    np.save(tmp_path / "mask.npy", mask)
    capsys.readouterr()
    depth = run.main(args + ["--gt", str(tmp_path / "gt.npy"), "--gt-mask", str(tmp_path / "mask.npy")])
    assert np.array_equal(depth, first)
    r = check_driver_score(tmp_path / "bench" / "depth_anything_ac_gt.json", capsys.readouterr().out, depth, gt, mask,
                           "scale_shift", True, None, "depth_anything_ac")
    assert r["fit"]["scale"] > 0 and r["orientation"] < 0  # an inverse-depth output runs against depth


def test_depth_pro_driver_gt(gpu, tmp_path, capsys):
    """depth_pro (spec: metric -> none) on a 120 x 160 photo."""
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    h, w = 120, 160
    c = ev.synthetic_gt_case(h, w, 4343)
    np.save(tmp_path / "src.npy", photo(h, w))
    np.save(tmp_path / "gt.npy", c["gt"])
    np.save(tmp_path / "mask.npy", c["mask"])
    args = ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations",
            "2", "--warmup", "1", "--image", str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench"),
            "--gt", str(tmp_path / "gt.npy"), "--gt-mask", str(tmp_path / "mask.npy")]
    depth, _ = run.main(args)
    check_driver_score(tmp_path / "bench" / "depth_pro_gt.json", capsys.readouterr().out, depth, c["gt"], c["mask"],
                       "none", False, None, "depth_pro")
    with pytest.raises(SystemExit, match="host-postprocess"):
        run.main(args + ["--host-postprocess"])


def test_vggt_driver_is_left_alone():
    """Its spec says `unknown`: no --gt there, and nothing scores it by default."""
    from monocular_depth_estimation_trt_amd import spec
    from monocular_depth_estimation_trt_amd.models.vggt import run
    with pytest.raises(ValueError):
        ev.spec_policy(spec.load("vggt"))
    assert "--gt" not in open(run.__file__).read()
