"""Scoring a depth map against measured ground truth, on the device: the
per-image call sequence of the reference's `tools/evaluate_gt.py:555-583` over
its `core/gt.py` (`orientation`, `align`, `metrics`) as `mde_op_depth_eval`
(csrc/depth_eval.hip).  The map that the device post-process left in device
memory is scored there; 16 doubles per image come back instead of the map.

`align_np`, `metrics_np`, `orientation_np` and `score_np` restate the
include/mde.h contract in numpy float64 (the kernels are held to them within
the summation-order tolerance of DESIGN.md, "Scoring against ground truth", and
they to the reference's recorded results in tests/golden/gt_eval_cases.npz);
`policy_for` / `policy_for_normalised` choose the alignment from a spec's
`depth_scale`; `DeviceEval` owns the buffers and drives the op.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional

import numpy as np

from . import _lib
from .common_runtime import EventPair, HostDeviceMem, stream_synchronize

POLICIES = ("none", "scale", "scale_shift")
OUT_SLOTS = 16
# out[b][.] of mde_op_depth_eval (include/mde.h)
STATUS, N_FIT, SCALE, SHIFT, N, ABS_REL, RMSE, LOG10, DELTA1, DELTA2, DELTA3, ORIENTATION, N_MASK = range(13)
METRIC_KEYS = ("abs_rel", "rmse", "log10", "delta1", "delta2", "delta3")
# the reference's three ValueErrors of align (core/gt.py:53, :66, :82)
SKIP_FEW = "alignment needs at least two valid pixels"
SKIP_FEW_POSITIVE = "scale_shift needs at least two positive-depth pixels"
SKIP_CONSTANT = "scale_shift is underdetermined; the prediction is constant"


class AlignmentSkip(ValueError):
    """The fit is not determined by the data (status 1 or 2 of the op)."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = int(status)


def policy_for(depth_scale) -> Optional[str]:
    """The alignment a spec's `depth_scale` earns: metric -> none (it claims
    metres), relative -> scale_shift (it claims ordering only), anything else
    -> None: not scored.  `unknown` (VGGT) stays unscored."""
    return {"metric": "none", "relative": "scale_shift"}.get(depth_scale)


def policy_for_normalised(depth_scale, scale_only: bool = False) -> Optional[str]:
    """The one-parameter path of a normalised-coordinate output: `scale` when
    the spec declares `normalised`, or when the caller names it (`scale_only`)
    for a model whose spec does not; never reached from policy_for."""
    return "scale" if (depth_scale == "normalised" or scale_only) else None


def skip_message(status: int, n_mask: int) -> str:
    """The reference's ValueError text for a failed fit."""
    if int(status) == 2:
        return SKIP_CONSTANT
    return SKIP_FEW if n_mask < 2 else SKIP_FEW_POSITIVE


def _policy_index(policy) -> int:
    if policy in POLICIES:
        return POLICIES.index(policy)
    if isinstance(policy, (int, np.integer)) and 0 <= int(policy) < len(POLICIES):
        return int(policy)
    raise ValueError(f"unknown alignment policy {policy!r}; expected one of {POLICIES}")


def _f64(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64)


def align_np(pred, gt, mask, policy, pred_is_inverse=False):
    """(aligned prediction over the whole frame, fitted parameters) for one
    image; `mask` is used as given (score_np passes mask & gt > 0, narrowed to
    finite predictions where asked).  Raises AlignmentSkip."""
    policy = POLICIES[_policy_index(policy)]
    p, g = _f64(pred), _f64(gt)
    m = np.asarray(mask) != 0
    if policy == "none":
        return p, {}
    n_mask = int(np.count_nonzero(m))
    if n_mask < 2:
        raise AlignmentSkip(1, skip_message(1, n_mask))
    with np.errstate(all="ignore"):
        if policy == "scale":
            pm, gm = p[m], g[m]
            spg, spp = float(np.sum(pm * gm)), float(np.sum(pm * pm))
            s = spg / (1e-12 if 1e-12 > spp else spp)  # a NaN spp stays NaN
            return p * s, {"scale": float(s)}
        valid = m & (g > 0) & np.isfinite(p)
        if not pred_is_inverse:
            valid &= p > 0
        n = int(np.count_nonzero(valid))
        if n < 2:
            raise AlignmentSkip(1, skip_message(1, n_mask))
        x = p[valid] if pred_is_inverse else 1.0 / p[valid]
        y = 1.0 / g[valid]
        sx, sy, sxx, sxy = float(np.sum(x)), float(np.sum(y)), float(np.sum(x * x)), float(np.sum(x * y))
        denom = n * sxx - sx * sx
        if abs(denom) < 1e-12:
            raise AlignmentSkip(2, skip_message(2, n_mask))
        s = (n * sxy - sx * sy) / denom
        t = (sy - s * sx) / n
        xa = p if pred_is_inverse else 1.0 / np.where(p > 0, p, np.nan)
        disp = xa * s + t
        return np.where(disp > 1e-8, 1.0 / disp, np.inf), {"scale": float(s), "shift": float(t)}


def metrics_np(aligned, gt, mask, max_depth=None):
    """n, abs_rel, rmse, log10, delta1..3 over mask & isfinite(aligned) &
    gt > 0 (& gt <= max_depth when a limit > 0 is given); {"n": 0} when empty."""
    p, g = _f64(aligned), _f64(gt)
    with np.errstate(all="ignore"):
        m = (np.asarray(mask) != 0) & np.isfinite(p) & (g > 0)
        if max_depth is not None and max_depth > 0:
            m &= g <= float(np.float32(max_depth))
        n = int(np.count_nonzero(m))
        if not n:
            return {"n": 0}
        p, g = np.maximum(p[m], 1e-6), g[m]
        ratio = np.maximum(p / g, g / p)
        d = p - g
        return {"n": n,
                "abs_rel": float(np.sum(np.abs(d) / g) / n),
                "rmse": float(math.sqrt(float(np.sum(d * d)) / n)),
                "log10": float(np.sum(np.abs(np.log10(p) - np.log10(g))) / n),
                "delta1": float(np.count_nonzero(ratio < 1.25) / n),
                "delta2": float(np.count_nonzero(ratio < 1.5625) / n),
                "delta3": float(np.count_nonzero(ratio < 1.953125) / n)}


def orientation_np(pred, gt, mask) -> float:
    """Pearson correlation of pred and gt over mask & isfinite(pred) & gt > 0,
    in the uncentred form; NaN when undefined."""
    p, g = _f64(pred), _f64(gt)
    with np.errstate(all="ignore"):
        m = (np.asarray(mask) != 0) & np.isfinite(p) & (g > 0)
        n = int(np.count_nonzero(m))
        if n < 2:
            return float("nan")
        a, b = p[m], g[m]
        sa, sb = float(np.sum(a)), float(np.sum(b))
        saa = float(np.sum(a * a)) - sa * sa / n
        sbb = float(np.sum(b * b)) - sb * sb / n
        if saa <= 0 or sbb <= 0:
            return float("nan")
        sab = float(np.sum(a * b)) - sa * sb / n
        return float(sab / math.sqrt(saa * sbb))


def score_np(pred, gt, mask, policy, pred_is_inverse=False, fit_finite_only=False, max_depth=None) -> dict:
    """The whole contract for one image [h, w], as DeviceEval.result() words
    it: {"n", "abs_rel", ..., "delta3", "orientation", "fit", "n_fit"}, or
    {"skip": message, "status": 1 | 2, "orientation"} when the fit fails."""
    policy = POLICIES[_policy_index(policy)]
    p32 = np.asarray(pred, dtype=np.float32)
    g32 = np.asarray(gt, dtype=np.float32)
    if p32.ndim != 2 or g32.shape != p32.shape or np.shape(mask) != p32.shape:
        raise ValueError(f"pred, gt and mask must share one [h, w] shape, got {p32.shape}, {g32.shape}, {np.shape(mask)}")
    with np.errstate(all="ignore"):
        m = (np.asarray(mask) != 0) & (g32 > 0)
        orient = orientation_np(p32, g32, m)
        fit_mask = m & np.isfinite(p32) if (policy == "scale" and fit_finite_only) else m
        try:
            aligned, fit = align_np(p32, g32, fit_mask, policy, pred_is_inverse)
        except AlignmentSkip as e:
            return {"skip": str(e), "status": e.status, "orientation": orient}
        if policy == "scale":
            n_fit = int(np.count_nonzero(fit_mask))
        elif policy == "scale_shift":
            v = m & np.isfinite(p32)
            n_fit = int(np.count_nonzero(v if pred_is_inverse else v & (p32 > 0)))
        else:
            n_fit = 0
        r = metrics_np(aligned, g32, m, max_depth)
    for k in METRIC_KEYS:
        r.setdefault(k, float("nan"))
    r["orientation"] = orient
    r["fit"] = fit
    r["n_fit"] = n_fit
    return r


def synthetic_gt_case(h: int, w: int, seed: int) -> dict:
    """Seeded stand-ins for one image (numpy PCG64), float32 [h, w]: ground
    truth g ~ U(0.5, 20) metres, a mask with 70 % valid, and three predictions
    with multiplicative noise e = N(0, 0.15^2): `metric` g * exp(e),
    `inverse` 3 / (g * exp(e)) + 0.2 (a relative inverse-depth output) and
    `depth`, its reciprocal.  What the fixtures, the tests and
    tools/bench_eval.py score."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    g = rng.uniform(0.5, 20.0, (h, w))
    noisy = g * np.exp(rng.normal(0.0, 0.15, (h, w)))
    mask = rng.random((h, w)) < 0.7
    inverse = 3.0 / noisy + 0.2
    return {"gt": g.astype(np.float32), "mask": mask, "metric": noisy.astype(np.float32),
            "inverse": inverse.astype(np.float32), "depth": (1.0 / inverse).astype(np.float32)}


def ws_bytes(batch: int, h: int, w: int) -> int:
    """Device scratch the op needs (mde_op_depth_eval_ws_bytes); 0: refused."""
    return int(_lib.lib().mde_op_depth_eval_ws_bytes(int(batch), int(h), int(w)))


def depth_eval(d_pred: int, d_gt: int, d_mask: int, batch: int, h: int, w: int, policy, pred_is_inverse: bool,
               fit_finite_only: bool, max_depth: Optional[float], d_out: int, d_ws: int, ws_nbytes: int,
               stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream` (mde_op_depth_eval)."""
    _lib.call("mde_op_depth_eval", C.c_void_p(int(d_pred or 0)), C.c_void_p(int(d_gt or 0)),
              C.c_void_p(int(d_mask or 0)), int(batch), int(h), int(w), _policy_index(policy),
              int(bool(pred_is_inverse)), int(bool(fit_finite_only)), float(max_depth or 0.0),
              C.c_void_p(int(d_out or 0)), C.c_void_p(int(d_ws or 0)), int(ws_nbytes), C.c_void_p(int(stream or 0)))


def result_dict(row, policy) -> dict:
    """One image's out[16] as the dict score_np returns."""
    policy = POLICIES[_policy_index(policy)]
    row = np.asarray(row, dtype=np.float64)
    status = int(row[STATUS])
    if status:
        return {"skip": skip_message(status, int(row[N_MASK])), "status": status,
                "orientation": float(row[ORIENTATION])}
    r = {"n": int(row[N])}
    for i, k in enumerate(METRIC_KEYS):
        r[k] = float(row[ABS_REL + i])
    r["orientation"] = float(row[ORIENTATION])
    r["fit"] = ({} if policy == "none" else {"scale": float(row[SCALE])} if policy == "scale"
                else {"scale": float(row[SCALE]), "shift": float(row[SHIFT])})
    r["n_fit"] = int(row[N_FIT])
    return r


class DeviceEval:
    """Owns the ground truth and mask on the device, `out` (device + pinned
    host) and the scratch for `batch` maps [h, w].

    upload_gt(gt, mask) copies the measured side once; enqueue(d_pred, stream,
    policy, ...) only enqueues the four kernels (capturable); download(stream)
    brings the 128 bytes per image back and synchronizes; result() is one dict
    per image in the reference's words (see score_np); run() = enqueue,
    download, result."""

    def __init__(self, batch: int, h: int, w: int):
        self.batch, self.h, self.w = int(batch), int(h), int(w)
        self.gt: Optional[HostDeviceMem] = None
        self.mask: Optional[HostDeviceMem] = None
        self.out: Optional[HostDeviceMem] = None
        self._ws = 0
        self._ws_bytes = ws_bytes(self.batch, self.h, self.w)
        self._policy = None
        if self._ws_bytes == 0:
            raise ValueError(f"mde_op_depth_eval does not take batch {batch}, {h}x{w}")
        n = self.batch * self.h * self.w
        try:
            self.gt = HostDeviceMem(n, np.float32)
            self.mask = HostDeviceMem(n, np.uint8)
            self.out = HostDeviceMem(self.batch * OUT_SLOTS, np.float64)
            p = C.c_void_p()
            _lib.call("mde_rt_malloc", C.byref(p), self._ws_bytes)
            self._ws = int(p.value)
        except Exception:
            self.free()
            raise

    def _alive(self):
        if self.out is None:
            raise RuntimeError("DeviceEval already freed")

    def upload_gt(self, gt, mask, stream: int = 0) -> None:
        """gt: float [batch, h, w] (or [h, w] for batch 1) in metres; mask: the
        same shape, nonzero = measured.  Synchronizes `stream`."""
        self._alive()
        shape = (self.batch, self.h, self.w)
        g = np.asarray(gt, dtype=np.float32).reshape(shape)
        m = (np.asarray(mask) != 0).reshape(shape)
        self.gt.host[:] = g.reshape(-1)
        self.mask.host[:] = m.reshape(-1)
        s = C.c_void_p(int(stream or 0))
        for mem in (self.gt, self.mask):
            _lib.call("mde_rt_memcpy_htod_async", C.c_void_p(mem.device), mem.host.ctypes.data_as(C.c_void_p),
                      mem.nbytes, s)
        stream_synchronize(stream)

    def enqueue(self, d_pred: int, stream: int, policy, pred_is_inverse: bool = False, fit_finite_only: bool = False,
                max_depth: Optional[float] = None) -> None:
        """The kernels on `stream`, nothing else.  d_pred: device float32
        [batch][h][w] (DevicePostprocess.mem.device)."""
        self._alive()
        self._policy = POLICIES[_policy_index(policy)]
        depth_eval(d_pred, self.gt.device, self.mask.device, self.batch, self.h, self.w, self._policy,
                   pred_is_inverse, fit_finite_only, max_depth, self.out.device, self._ws, self._ws_bytes, stream)

    def download(self, stream: int) -> None:
        self._alive()
        _lib.call("mde_rt_memcpy_dtoh_async", self.out.host.ctypes.data_as(C.c_void_p), C.c_void_p(self.out.device),
                  self.out.nbytes, C.c_void_p(int(stream or 0)))
        stream_synchronize(stream)

    def raw(self) -> np.ndarray:
        """out as float64 [batch, 16]; valid after download()."""
        self._alive()
        return self.out.host.reshape(self.batch, OUT_SLOTS)

    def result(self) -> List[dict]:
        """One dict per image; valid after download()."""
        if self._policy is None:
            raise RuntimeError("DeviceEval.result() before enqueue()")
        return [result_dict(row, self._policy) for row in self.raw()]

    def run(self, d_pred: int, stream: int, policy, **kw) -> List[dict]:
        self.enqueue(d_pred, stream, policy, **kw)
        self.download(stream)
        return self.result()

    def free(self) -> None:
        for m in (self.gt, self.mask, self.out):
            if m is not None:
                m.free()
        self.gt = self.mask = self.out = None
        if self._ws:
            _lib.call("mde_rt_free", C.c_void_p(self._ws))
            self._ws = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def spec_policy(spec: dict, scale_only: bool = False):
    """(policy, pred_is_inverse) for a model's spec.json, or raises ValueError
    saying why the model is not scored: the reference's alignment_policy plus
    its refusal of a relative model without a declared `output_form`."""
    scale = spec.get("depth_scale")
    policy = policy_for(scale) or policy_for_normalised(scale, scale_only)
    if policy is None:
        raise ValueError(f"depth_scale {scale!r} earns no alignment policy: the model is not scored "
                         f"(name the scale-only path to score a normalised-coordinate output)")
    form = spec.get("output_form")
    if policy == "scale_shift" and form not in ("depth", "inverse_depth"):
        raise ValueError("a relative model needs output_form 'depth' or 'inverse_depth' in its spec to be scored")
    return policy, form == "inverse_depth"


def load_gt(gt_path, mask_path, hw):
    """The drivers' --gt / --gt-mask: two .npy maps of the source size `hw`
    (a trailing channel axis is dropped, as the reference does)."""
    g = np.load(gt_path, allow_pickle=False)
    m = np.load(mask_path, allow_pickle=False)
    g = g[..., 0] if g.ndim == 3 else g
    m = m[..., 0] if m.ndim == 3 else m
    if g.shape != tuple(hw) or m.shape != tuple(hw):
        raise ValueError(f"--gt {g.shape} and --gt-mask {m.shape} must have the map's size {tuple(hw)}: "
                         f"ground truth is not resized")
    return g.astype(np.float32), m != 0


def device_score(d_pred: int, h: int, w: int, stream: int, gt, mask, policy, pred_is_inverse=False,
                 max_depth: Optional[float] = None):
    """What the model drivers' --gt does: DeviceEval on one device map [h][w]
    at `d_pred`.  Returns (ms of the kernels + the 128-byte D2H between two
    hipEvents on `stream`, the result dict)."""
    with DeviceEval(1, h, w) as de:
        de.upload_gt(gt, mask, stream)
        with EventPair(stream) as ev:
            de.enqueue(d_pred, stream, policy, pred_is_inverse=pred_is_inverse,
                       fit_finite_only=policy == "scale", max_depth=max_depth)
            de.download(stream)
            ev.stop()
            stream_synchronize(stream)
            return ev.ms(), de.result()[0]


def format_score(r: dict) -> str:
    """The drivers' one `[MDET] gt : ...` line."""
    if "skip" in r:
        return f"skip ({r['skip']}), orientation {r['orientation']:+0.4f}"
    s = (f"n {r['n']} abs_rel {r['abs_rel']:0.5f} rmse {r['rmse']:0.5f} log10 {r['log10']:0.5f} "
         f"delta1 {r['delta1']:0.5f} delta2 {r['delta2']:0.5f} delta3 {r['delta3']:0.5f} "
         f"orientation {r['orientation']:+0.4f}")
    if r["fit"]:
        s += " fit " + " ".join(f"{k} {v:0.6g}" for k, v in r["fit"].items())
    return s


def add_gt_arguments(ap) -> None:
    """The model drivers' --gt options."""
    ap.add_argument("--gt", default="", metavar="DEPTH.npy",
                    help="score the depth map against this ground truth (metres, the map's size); needs --gt-mask")
    ap.add_argument("--gt-mask", default="", metavar="MASK.npy", help="with --gt: nonzero = measured pixel")
    ap.add_argument("--max-depth", type=float, default=None,
                    help="with --gt: ground truth beyond this range is not scored")
    ap.add_argument("--gt-out", default="", metavar="PATH.json",
                    help="with --gt: where the result goes (default <out-dir>/<model>_gt.json)")


def check_gt_arguments(a, model_spec: dict, device_map: bool):
    """--gt's conditions that can be answered before an engine is built.
    Returns (policy, pred_is_inverse) from the model's spec, or None without
    --gt; SystemExit otherwise."""
    if not a.gt:
        if a.gt_mask or a.max_depth is not None or a.gt_out:
            raise SystemExit("--gt-mask, --max-depth and --gt-out go with --gt")
        return None
    if not a.gt_mask:
        raise SystemExit("--gt needs --gt-mask (which pixels were measured)")
    if not device_map:
        raise SystemExit("--gt scores the map the device post-process left in device memory: not with "
                         "--host-postprocess")
    if a.max_depth is not None and not a.max_depth > 0:
        raise SystemExit("--max-depth must be positive")
    try:
        return spec_policy(model_spec)
    except ValueError as e:
        raise SystemExit(f"--gt: {e}")


def load_gt_arguments(a, hw):
    """(gt, mask) of the drivers' --gt / --gt-mask for a map of size `hw`,
    before an engine is built; SystemExit when they do not fit."""
    try:
        return load_gt(a.gt, a.gt_mask, hw)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))


def driver_score(a, model: str, policy_inverse, gt_mask, d_pred: int, hw, stream: int) -> dict:
    """The drivers' --gt: score the device map [hw] at `d_pred` against
    `gt_mask` = (gt, mask), print the `[MDET] gt : ...` line and write the
    result as JSON."""
    import json
    import os
    policy, inverse = policy_inverse
    gt, mask = gt_mask
    ms, r = device_score(d_pred, hw[0], hw[1], stream, gt, mask, policy, inverse, a.max_depth)
    r = dict(r, model=model, policy=policy, pred_is_inverse=bool(inverse), max_depth=a.max_depth,
             height=int(hw[0]), width=int(hw[1]))
    print(f"[MDET] gt : policy {policy} (device, kernels + D2H of 128 bytes, hipEvents: {ms:0.3f} ms) "
          f"{format_score(r)}")
    path = a.gt_out or os.path.join(a.out_dir, f"{model}_gt.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(r, f, indent=1)
    return r


__all__ = ["POLICIES", "METRIC_KEYS", "AlignmentSkip", "policy_for", "policy_for_normalised", "skip_message",
           "align_np", "metrics_np", "orientation_np", "score_np", "synthetic_gt_case", "ws_bytes", "depth_eval", "result_dict",
           "DeviceEval", "spec_policy", "load_gt", "device_score", "format_score", "add_gt_arguments",
           "check_gt_arguments", "load_gt_arguments", "driver_score"]
