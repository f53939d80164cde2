"""Colour frames on the device: the closing lines of the reference drivers
(`models/depth_pro/onnx2trt.py:156-168`, `models/depth_anything_v2/
onnx2trt.py:131-150`, `models/vggt/onnx2trt.py:122-142`) and its
`core/viz.py:colorize` as `mde_op_depth_colorize` (csrc/depth_colorize.hip).
The map that the device post-process left in device memory is ranged and
looked up in a colour table there; 3 bytes per pixel come back instead of 4.

`colorize_np` restates the include/mde.h contract in numpy (the kernels are
held to it byte for byte, and it to matplotlib's `turbo` through the
reference's lines in tests/golden/colorize_cases.npz); `lut` builds the
257-entry table from colormaps.py; `mode_for` chooses the recipe from a spec's
`depth_scale`; `DeviceColorize` owns the buffers and drives the op.

Robust range: the reference's `core/viz.py` (`robust_range`, `display_ranges`,
`qualitative_display`) and `demo.py:distribution` as `mde_op_depth_quantiles`
(csrc/depth_quantiles.hip) and `mde_op_depth_colorize_ranged`.  `quantiles_np`
and `colorize_ranged_np` restate their contracts in numpy (with a sort, not
with `np.percentile`, so that the two can be tested against each other);
`robust_range_np` and `distribution_np` are the reference's functions on top;
`DeviceQuantiles` owns the op's buffers, and `DeviceColorize.enqueue` with
mode "robust" chains the two ops without a host read in between.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib, colormaps
from .common_runtime import EventPair, HostDeviceMem, stream_synchronize
from .preprocess import resize_u8

MODES = ("inverse_auto", "minmax_u8", "fixed")
TILE = 4096              # MDE_DEPTH_COLORIZE_TILE
BAD = (0, 0, 0)          # what matplotlib draws for a pixel without an index
BAD_VIZ = (60, 60, 66)   # core/viz.py's invalid colour, for mode "fixed"


def lut(name: str = "turbo", bad=BAD) -> np.ndarray:
    """uint8 [257, 3] in R, G, B order: the 256 colours of `name`, then `bad`."""
    if name not in colormaps.TABLES:
        raise ValueError(f"unknown colour map {name!r}; expected one of {tuple(colormaps.TABLES)}")
    bad = np.asarray(bad)
    if bad.shape != (3,) or (bad < 0).any() or (bad > 255).any():
        raise ValueError(f"bad colour must be three values in 0..255, got {bad!r}")
    return np.concatenate([colormaps.TABLES[name], bad.astype(np.uint8)[None]])


def mode_index(mode) -> int:
    if mode in MODES:
        return MODES.index(mode)
    if isinstance(mode, (int, np.integer)) and 0 <= int(mode) < len(MODES):
        return int(mode)
    raise ValueError(f"unknown colour mode {mode!r}; expected one of {MODES}")


def mode_for(spec: dict) -> str:
    """The recipe a spec's `depth_scale` earns: relative -> minmax_u8 (the
    relative driver's), metric and anything else -> inverse_auto."""
    return "minmax_u8" if spec.get("depth_scale") == "relative" else "inverse_auto"


def _finite_range(v: np.ndarray):
    fin = v[np.isfinite(v)]
    if fin.size == 0:
        return None
    return np.float32(fin.min()), np.float32(fin.max())


def index_np(x, mode, map_is_inverse=False, denom_eps=0.0, vmin=None, vmax=None):
    """(table index int32 [h, w] in 0..256, (lo, hi) float32) of one image
    [h, w]: the contract of mde_op_depth_colorize up to the table look-up."""
    f32 = np.float32
    mode = MODES[mode_index(mode)]
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f"index_np takes one [h, w] map, got {x.shape}")
    with np.errstate(all="ignore"):
        if mode == "fixed":
            if vmin is None or vmax is None:
                raise ValueError("mode 'fixed' needs vmin and vmax")
            vmin, vmax = float(vmin), float(vmax)
            if vmin != vmin or vmax != vmax:
                raise ValueError("vmin and vmax must not be NaN")
            if vmax <= vmin:
                vmax = vmin + 1e-6
            t = (x.astype(np.float64) - vmin) / (vmax - vmin)
            bad = ~np.isfinite(x) | np.isnan(t)
            t = np.clip(np.where(bad, 0.0, t), 0.0, 1.0)
            idx = np.minimum((t * 256.0).astype(np.int32), 255)
            return np.where(bad, 256, idx).astype(np.int32), (f32(vmin), f32(vmax))
        if mode == "inverse_auto":
            v = x if map_is_inverse else f32(1.0) / x
            top = f32(256.0)
        else:
            v, top = x, f32(255.0)
        r = _finite_range(v)
        if r is None:
            lo = hi = d = f32(np.nan)
        elif mode == "inverse_auto":
            vmn, vmx = r
            c = f32(1.0 / 250)
            lo = vmn if vmn > c else c
            hi = vmx if vmx < f32(10.0) else f32(10.0)
            if vmx > f32(10.0) and vmn <= c:
                d = f32(10.0 - 1.0 / 250 + float(denom_eps))
            else:
                d = f32(f32(hi - lo) + f32(denom_eps))
        else:
            lo, hi = r
            d = f32(hi - lo)
        t = ((v - lo) / d) * top
        assert t.dtype == np.float32
        nan = np.isnan(t)
        inside = ~nan & (t >= 0) & (t < top)
        idx = np.where(inside, t, 0).astype(np.int32)
        idx = np.where(nan, 256, np.where(t < 0, 0, np.where(t >= top, 255, idx)))
        return idx.astype(np.int32), (f32(lo), f32(hi))


def colorize_np(map, mode, map_is_inverse=False, denom_eps=0.0, vmin=None, vmax=None, cmap="turbo", swap_rb=True,
                bad=None) -> Tuple[np.ndarray, np.ndarray]:
    """The whole contract in numpy: map [h, w] -> (picture uint8 [h, w, 3],
    range float32 [2]), or [batch, h, w] -> ([batch, h, w, 3], [batch, 2]),
    each image ranged on its own.  `bad`: the colour of a pixel without an
    index (default: black, BAD_VIZ in mode 'fixed')."""
    mode = MODES[mode_index(mode)]
    table = lut(cmap, bad if bad is not None else (BAD_VIZ if mode == "fixed" else BAD))
    if swap_rb:
        table = table[:, ::-1]
    x = np.asarray(map, dtype=np.float32)
    if x.ndim not in (2, 3):
        raise ValueError(f"colorize_np takes [h, w] or [batch, h, w], got {x.shape}")
    pics, ranges = [], []
    for im in x.reshape(-1, *x.shape[-2:]):
        idx, r = index_np(im, mode, map_is_inverse, denom_eps, vmin, vmax)
        pics.append(table[idx])
        ranges.append(r)
    pics, ranges = np.ascontiguousarray(np.stack(pics)), np.array(ranges, dtype=np.float32)
    return (pics[0], ranges[0]) if x.ndim == 2 else (pics, ranges)


SAMPLE_CAP = 200000      # core/viz.py:robust_range's subsample
ROW = 8                  # doubles per row of mde_op_depth_quantiles
# out[row][.] of mde_op_depth_quantiles (include/mde.h); with three quantiles the third takes Q_MAX's slot
Q_NVALID, Q_NUSED, Q_MIN, Q_MAX, Q_Q0, Q_Q1, Q_VMIN, Q_VMAX = range(8)
DISTRIBUTION_Q = (2.0, 50.0, 98.0)


def _check_q(q_percent) -> Tuple[float, ...]:
    q = tuple(float(p) for p in np.atleast_1d(np.asarray(q_percent, dtype=np.float64)))
    if not 1 <= len(q) <= 3 or not all(0.0 <= p <= 100.0 for p in q):
        raise ValueError(f"q_percent must be one to three percentages in [0, 100], got {q_percent!r}")
    return q


def _sample_np(im, positive_only, reciprocal, sample_cap):
    """(n_valid, the sample float64 [n_used]) of one image."""
    x = np.asarray(im, dtype=np.float32).ravel()
    ok = np.isfinite(x)
    if positive_only:
        ok &= x > 0
    v = x[ok]
    n_valid = int(v.size)
    stride = max(1, n_valid // sample_cap) if sample_cap > 0 and n_valid > sample_cap else 1
    v = v[::stride].astype(np.float64) + 0.0  # -0 counts as +0
    return n_valid, (1.0 / v if reciprocal else v)


def _quantile_sorted(s: np.ndarray, p: float) -> np.float64:
    """np.percentile(method linear) of sorted float64 `s` (n >= 1), operation by operation."""
    n = s.size
    q = np.float64(p) / np.float64(100.0)
    top = np.float64(n - 1)
    vi = top * q
    fl = np.floor(vi)
    if vi >= top:
        prev = nxt = n - 1
    else:
        prev = int(fl)
        nxt = prev + 1
    g = vi - fl
    d = s[nxt] - s[prev]
    return s[prev] + d * g if g < 0.5 else s[nxt] - d * (np.float64(1.0) - g)


def quantiles_np(maps, q_percent, positive_only=False, reciprocal=False, pooled=False, sample_cap=0) -> np.ndarray:
    """The contract of mde_op_depth_quantiles in numpy: maps [h, w] or
    [batch, h, w] -> float64 [rows, 8], rows = 1 when pooled, else batch."""
    q = _check_q(q_percent)
    sample_cap = int(sample_cap)
    if sample_cap < 0:
        raise ValueError("sample_cap must not be negative")
    x = np.asarray(maps, dtype=np.float32)
    if x.ndim not in (2, 3):
        raise ValueError(f"quantiles_np takes [h, w] or [batch, h, w], got {x.shape}")
    x = x.reshape(-1, *x.shape[-2:])
    with np.errstate(all="ignore"):
        parts = [_sample_np(im, positive_only, reciprocal, sample_cap) for im in x]
        if pooled:
            parts = [(sum(n for n, _ in parts), np.concatenate([v for _, v in parts]))]
        out = np.zeros((len(parts), ROW), dtype=np.float64)
        for o, (n_valid, v) in zip(out, parts):
            o[Q_NVALID], o[Q_NUSED] = n_valid, v.size
            if v.size == 0:
                o[Q_MIN:Q_Q1 + 1] = np.nan
                o[Q_VMIN], o[Q_VMAX] = 0.0, 1.0
                continue
            s = np.sort(v)
            qv = [_quantile_sorted(s, p) for p in q]
            o[Q_MIN], o[Q_MAX] = s[0], s[-1]
            o[Q_Q0] = qv[0]
            if len(q) >= 2:
                o[Q_Q1] = qv[1]
            if len(q) == 3:
                o[Q_MAX] = qv[2]
            vmin, vmax = qv[0], qv[-1]
            if not np.isfinite(vmin) or not np.isfinite(vmax) or vmax <= vmin:
                vmin, vmax = s[0], s[-1]
                if vmax <= vmin:
                    vmax = vmin + np.float64(1.0)
            o[Q_VMIN], o[Q_VMAX] = vmin, vmax
    return out


def row_quantiles(row, nq: int) -> Tuple[float, ...]:
    """The nq quantiles of one row of mde_op_depth_quantiles / quantiles_np."""
    return tuple(float(row[i]) for i in (Q_Q0, Q_Q1, Q_MAX)[:nq])


def robust_range_np(maps, lo_pct=2.0, hi_pct=98.0, positive_only=True, reciprocal=False,
                    sample_cap=SAMPLE_CAP) -> Tuple[float, float]:
    """core/viz.py:robust_range: one (vmin, vmax) pooled over every map given
    ([h, w], [batch, h, w] or a list of equally sized maps)."""
    r = quantiles_np(maps, (lo_pct, hi_pct), positive_only, reciprocal, True, sample_cap)[0]
    return float(r[Q_VMIN]), float(r[Q_VMAX])


def distribution_row(row, pixels: int) -> Optional[dict]:
    """demo.py:distribution from a row computed with DISTRIBUTION_Q and
    positive_only off over `pixels` pixels; None when nothing is finite."""
    if row[Q_NVALID] == 0:
        return None
    p02, med, p98 = row_quantiles(row, 3)
    return {"p02": p02, "median": med, "p98": p98, "valid_pct": float(row[Q_NVALID]) / pixels * 100.0}


def distribution_np(map) -> Optional[dict]:
    """demo.py:distribution of one map [h, w]: the numbers printed under a panel."""
    x = np.asarray(map, dtype=np.float32)
    return distribution_row(quantiles_np(x, DISTRIBUTION_Q)[0], x.size)


def format_distribution(d: Optional[dict]) -> str:
    if d is None:
        return "[MDET] depth : no finite pixel"
    return (f"[MDET] depth : p02 {d['p02']!r} median {d['median']!r} p98 {d['p98']!r} "
            f"valid {d['valid_pct']!r}%")


def colorize_ranged_np(map, ranges, positive_only=False, reciprocal=False, cmap="turbo", swap_rb=True,
                       bad=BAD_VIZ) -> np.ndarray:
    """The contract of mde_op_depth_colorize_ranged in numpy: map [h, w] or
    [batch, h, w] on `ranges` = (vmin, vmax), shared, or [batch, 2]."""
    table = lut(cmap, bad)
    if swap_rb:
        table = table[:, ::-1]
    x = np.asarray(map, dtype=np.float32)
    if x.ndim not in (2, 3):
        raise ValueError(f"colorize_ranged_np takes [h, w] or [batch, h, w], got {x.shape}")
    ims = x.reshape(-1, *x.shape[-2:])
    ranges = np.broadcast_to(np.asarray(ranges, dtype=np.float64).reshape(-1, 2), (len(ims), 2))
    pics = []
    with np.errstate(all="ignore"):
        for im, (vmin, vmax) in zip(ims, ranges):
            if vmax <= vmin:
                vmax = vmin + np.float64(1e-6)
            ok = np.isfinite(im)
            if positive_only:
                ok &= im > 0
            y = im.astype(np.float64)
            if reciprocal:
                y = 1.0 / y
            t = (y - vmin) / (vmax - vmin)
            bad_px = ~ok | np.isnan(t)
            t = np.clip(np.where(bad_px, 0.0, t), 0.0, 1.0)
            idx = np.where(bad_px, 256, np.minimum((t * 256.0).astype(np.int32), 255))
            pics.append(table[idx])
    pics = np.ascontiguousarray(np.stack(pics))
    return pics[0] if x.ndim == 2 else pics


def quantiles_ws_bytes(batch: int, h: int, w: int) -> int:
    """Device scratch mde_op_depth_quantiles needs (mde_op_depth_quantiles_ws_bytes); 0: refused."""
    return int(_lib.lib().mde_op_depth_quantiles_ws_bytes(int(batch), int(h), int(w)))


def depth_quantiles(d_map: int, batch: int, h: int, w: int, positive_only: bool, reciprocal: bool, pooled: bool,
                    sample_cap: int, q_percent, d_out: int, d_ws: int, ws_nbytes: int, stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream` (mde_op_depth_quantiles)."""
    q = _check_q(q_percent)
    _lib.call("mde_op_depth_quantiles", C.c_void_p(int(d_map or 0)), int(batch), int(h), int(w),
              int(bool(positive_only)), int(bool(reciprocal)), int(bool(pooled)), int(sample_cap),
              (C.c_double * len(q))(*q), len(q), C.c_void_p(int(d_out or 0)), C.c_void_p(int(d_ws or 0)),
              int(ws_nbytes), C.c_void_p(int(stream or 0)))


def depth_colorize_ranged(d_map: int, batch: int, h: int, w: int, positive_only: bool, reciprocal: bool,
                          d_range: int, range_stride: int, d_lut: int, swap_rb: bool, d_out: int,
                          stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream` (mde_op_depth_colorize_ranged)."""
    _lib.call("mde_op_depth_colorize_ranged", C.c_void_p(int(d_map or 0)), int(batch), int(h), int(w),
              int(bool(positive_only)), int(bool(reciprocal)), C.c_void_p(int(d_range or 0)), int(range_stride),
              C.c_void_p(int(d_lut or 0)), int(bool(swap_rb)), C.c_void_p(int(d_out or 0)),
              C.c_void_p(int(stream or 0)))


class DeviceQuantiles:
    """Owns the rows (device + pinned host) and the scratch of
    mde_op_depth_quantiles for `batch` maps [h, w].

    enqueue(d_map, stream, q_percent, ...) only enqueues (capturable);
    download(stream) brings the rows back and synchronizes; result() is
    float64 [rows, 8] (rows = 1 after a pooled call), a view that the next
    download overwrites.  `out.device + 8 * Q_VMIN` with stride ROW is what
    mde_op_depth_colorize_ranged reads."""

    def __init__(self, batch: int, h: int, w: int):
        self.batch, self.h, self.w = int(batch), int(h), int(w)
        self.out: Optional[HostDeviceMem] = None
        self.rows = self.batch
        self._ws = 0
        self._ws_bytes = quantiles_ws_bytes(self.batch, self.h, self.w)
        if self._ws_bytes == 0:
            raise ValueError(f"mde_op_depth_quantiles does not take batch {batch}, {h}x{w}")
        try:
            self.out = HostDeviceMem(self.batch * ROW, np.float64)
            p = C.c_void_p()
            _lib.call("mde_rt_malloc", C.byref(p), self._ws_bytes)
            self._ws = int(p.value)
        except Exception:
            self.free()
            raise

    def _alive(self):
        if self.out is None:
            raise RuntimeError("DeviceQuantiles already freed")

    def enqueue(self, d_map: int, stream: int, q_percent=(2.0, 98.0), positive_only: bool = False,
                reciprocal: bool = False, pooled: bool = False, sample_cap: int = 0) -> None:
        self._alive()
        depth_quantiles(d_map, self.batch, self.h, self.w, positive_only, reciprocal, pooled, sample_cap, q_percent,
                        self.out.device, self._ws, self._ws_bytes, stream)
        self.rows = 1 if pooled else self.batch

    def download(self, stream: int) -> None:
        self._alive()
        _lib.call("mde_rt_memcpy_dtoh_async", self.out.host.ctypes.data_as(C.c_void_p), C.c_void_p(self.out.device),
                  self.rows * ROW * 8, C.c_void_p(int(stream or 0)))
        stream_synchronize(stream)

    def result(self) -> np.ndarray:
        """float64 [rows, 8]; valid after download()."""
        self._alive()
        return self.out.host[:self.rows * ROW].reshape(self.rows, ROW)

    def run(self, d_map: int, stream: int, q_percent=(2.0, 98.0), **kw) -> np.ndarray:
        self.enqueue(d_map, stream, q_percent, **kw)
        self.download(stream)
        return self.result()

    def free(self) -> None:
        if self.out is not None:
            self.out.free()
        self.out = None
        if self._ws:
            _lib.call("mde_rt_free", C.c_void_p(self._ws))
            self._ws = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def ws_bytes(batch: int, h: int, w: int) -> int:
    """Device scratch modes 0 and 1 need (mde_op_depth_colorize_ws_bytes); 0: refused."""
    return int(_lib.lib().mde_op_depth_colorize_ws_bytes(int(batch), int(h), int(w)))


def depth_colorize(d_map: int, batch: int, h: int, w: int, mode, map_is_inverse: bool, denom_eps: float,
                   vmin: Optional[float], vmax: Optional[float], d_lut: int, swap_rb: bool, d_out: int, d_range: int,
                   d_ws: int, ws_nbytes: int, stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream` (mde_op_depth_colorize)."""
    _lib.call("mde_op_depth_colorize", C.c_void_p(int(d_map or 0)), int(batch), int(h), int(w), mode_index(mode),
              int(bool(map_is_inverse)), float(denom_eps), float(0.0 if vmin is None else vmin),
              float(0.0 if vmax is None else vmax), C.c_void_p(int(d_lut or 0)), int(bool(swap_rb)),
              C.c_void_p(int(d_out or 0)), C.c_void_p(int(d_range or 0)), C.c_void_p(int(d_ws or 0)), int(ws_nbytes),
              C.c_void_p(int(stream or 0)))


class DeviceColorize:
    """Owns the picture and the range (device + pinned host), the device
    colour tables (bad colour black, then bad colour BAD_VIZ) and the scratch
    for `batch` maps [h, w].

    enqueue(d_map, stream, mode, ...) only enqueues the kernels (capturable);
    download(stream) brings the picture and the range back and synchronizes;
    result() is the picture uint8 [batch, h, w, 3], range() float32
    [batch, 2], both views that the next download overwrites; run() = enqueue,
    download, result.

    Mode "robust" (core/viz.py:robust_range and colorize) is not one of the
    op's modes: mde_op_depth_quantiles writes the q_percent display range of
    each image (of all of them when pooled) and mde_op_depth_colorize_ranged
    reads it from device memory, with no host read in between; range() is then
    float64.  Its DeviceQuantiles is allocated by the first such enqueue, or
    by the constructor with robust=True (for a capture)."""

    def __init__(self, batch: int, h: int, w: int, cmap: str = "turbo", robust: bool = False):
        self.batch, self.h, self.w = int(batch), int(h), int(w)
        self.cmap = cmap
        self.quant: Optional[DeviceQuantiles] = None
        self._robust = False  # whether the last enqueue was mode "robust"
        self._own_range = True  # ... and took its own quantiles
        self.out: Optional[HostDeviceMem] = None
        self.rng: Optional[HostDeviceMem] = None
        self.lut: Optional[HostDeviceMem] = None
        self._ws = 0
        self._ws_bytes = ws_bytes(self.batch, self.h, self.w)
        if self._ws_bytes == 0:
            raise ValueError(f"mde_op_depth_colorize does not take batch {batch}, {h}x{w}")
        tables = np.concatenate([lut(cmap, BAD), lut(cmap, BAD_VIZ)])  # an unknown name is refused here
        try:
            self.out = HostDeviceMem(self.batch * self.h * self.w * 3, np.uint8)
            self.rng = HostDeviceMem(self.batch * 2, np.float32)
            self.lut = HostDeviceMem(tables.size, np.uint8)
            self.lut.host[:] = tables.reshape(-1)
            _lib.call("mde_rt_memcpy_htod_async", C.c_void_p(self.lut.device),
                      self.lut.host.ctypes.data_as(C.c_void_p), self.lut.nbytes, None)
            _lib.call("mde_rt_device_synchronize")
            p = C.c_void_p()
            _lib.call("mde_rt_malloc", C.byref(p), self._ws_bytes)
            self._ws = int(p.value)
            if robust:
                self.quant = DeviceQuantiles(self.batch, self.h, self.w)
        except Exception:
            self.free()
            raise

    def _alive(self):
        if self.out is None:
            raise RuntimeError("DeviceColorize already freed")

    def enqueue(self, d_map: int, stream: int, mode, map_is_inverse: bool = False, denom_eps: float = 0.0,
                vmin: Optional[float] = None, vmax: Optional[float] = None, swap_rb: bool = True,
                q_percent=(2.0, 98.0), positive_only: bool = True, reciprocal: bool = False, pooled: bool = False,
                sample_cap: int = SAMPLE_CAP, d_range: int = 0) -> None:
        """The kernels on `stream`, nothing else.  d_map: device float32
        [batch][h][w] (DevicePostprocess.mem.device).  A pixel without an index
        is drawn BAD_VIZ in modes 'fixed' and 'robust', black otherwise.
        q_percent .. d_range: mode 'robust' only.  d_range: a device double[2]
        that already holds the axis every image shares (a range pooled over
        more maps than these); no quantiles are taken then and range() has
        nothing to report."""
        self._alive()
        self._robust = mode == "robust"
        self._own_range = not d_range
        if self._robust and d_range:
            depth_colorize_ranged(d_map, self.batch, self.h, self.w, positive_only, reciprocal, d_range, 0,
                                  self.lut.device + 257 * 3, swap_rb, self.out.device, stream)
            return
        if self._robust:
            if self.quant is None:
                self.quant = DeviceQuantiles(self.batch, self.h, self.w)
            self.quant.enqueue(d_map, stream, q_percent, positive_only, reciprocal, pooled, sample_cap)
            depth_colorize_ranged(d_map, self.batch, self.h, self.w, positive_only, reciprocal,
                                  self.quant.out.device + 8 * Q_VMIN, 0 if pooled else ROW,
                                  self.lut.device + 257 * 3, swap_rb, self.out.device, stream)
            return
        mode = MODES[mode_index(mode)]
        if mode == "fixed" and (vmin is None or vmax is None):
            raise ValueError("mode 'fixed' needs vmin and vmax")
        d_lut = self.lut.device + (257 * 3 if mode == "fixed" else 0)
        depth_colorize(d_map, self.batch, self.h, self.w, mode, map_is_inverse, denom_eps, vmin, vmax, d_lut, swap_rb,
                       self.out.device, self.rng.device, self._ws, self._ws_bytes, stream)

    def download(self, stream: int) -> None:
        self._alive()
        for m in (self.out,) if self._robust else (self.out, self.rng):
            _lib.call("mde_rt_memcpy_dtoh_async", m.host.ctypes.data_as(C.c_void_p), C.c_void_p(m.device), m.nbytes,
                      C.c_void_p(int(stream or 0)))
        if self._robust and self._own_range:
            self.quant.download(stream)
        stream_synchronize(stream)

    def result(self) -> np.ndarray:
        """The picture, uint8 [batch, h, w, 3]; valid after download()."""
        self._alive()
        return self.out.host.reshape(self.batch, self.h, self.w, 3)

    def range(self) -> np.ndarray:
        """float32 [batch, 2] (float64 after mode 'robust'): the range each image was drawn on;
        valid after download()."""
        self._alive()
        if self._robust and not self._own_range:
            raise RuntimeError("the axis was the caller's (d_range)")
        if self._robust:
            return np.broadcast_to(self.quant.result()[:, Q_VMIN:], (self.batch, 2))
        return self.rng.host.reshape(self.batch, 2)

    def run(self, d_map: int, stream: int, mode, **kw) -> np.ndarray:
        self.enqueue(d_map, stream, mode, **kw)
        self.download(stream)
        return self.result()

    def free(self) -> None:
        for m in (self.out, self.rng, self.lut):
            if m is not None:
                m.free()
        self.out = self.rng = self.lut = None
        if self.quant is not None:
            self.quant.free()
            self.quant = None
        if self._ws:
            _lib.call("mde_rt_free", C.c_void_p(self._ws))
            self._ws = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def save_image(path: str, bgr: np.ndarray) -> str:
    """Writes a uint8 [H, W, 3] BGR picture: a .npy holding exactly that, or
    any format Pillow can encode when it is installed (the mirror of
    preprocess.load_image_bgr).  Without Pillow the array goes to `path` +
    '.npy'.  Returns the path written."""
    import os
    bgr = np.asarray(bgr)
    if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError(f"expected a uint8 [H, W, 3] BGR image, got {bgr.dtype} {bgr.shape}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if not path.lower().endswith(".npy"):
        try:
            from PIL import Image
        except ImportError:
            path += ".npy"
        else:
            Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(path)
            return path
    np.save(path, np.ascontiguousarray(bgr))
    return path


def device_color(d_map: int, h: int, w: int, stream: int, mode, resize_hw=None, **kw):
    """What the model drivers' --color does: DeviceColorize on one device map
    [h][w] at `d_map`.  Returns (ms of the kernels + the D2H of the picture
    between two hipEvents on `stream`, picture uint8 [h, w, 3], (lo, hi)).
    `resize_hw` = (H, W): the picture is resized to that size on the device
    (mde_op_resize_u8, cv2's INTER_LINEAR; the VGGT driver's closing resize to
    the photo's size) and only the resized one, [H, W, 3], is downloaded.
    Mode "robust" with `d_range` (DeviceColorize.enqueue) reports `range_host`."""
    range_host = kw.pop("range_host", None)
    s = C.c_void_p(int(stream or 0))
    big = None
    try:
        with DeviceColorize(1, h, w) as dc:
            if resize_hw is not None:
                H, W = int(resize_hw[0]), int(resize_hw[1])
                big = HostDeviceMem(H * W * 3, np.uint8)
            with EventPair(stream) as ev:
                dc.enqueue(d_map, stream, mode, **kw)
                if big is None:
                    dc.download(stream)
                else:
                    resize_u8(dc.out.device, 1, h, w, 3 * w, False, big.device, H, W, stream)
                    if mode == "robust" and not kw.get("d_range"):
                        dc.quant.download(stream)
                    for m in (big,) if mode == "robust" else (big, dc.rng):
                        _lib.call("mde_rt_memcpy_dtoh_async", m.host.ctypes.data_as(C.c_void_p),
                                  C.c_void_p(m.device), m.nbytes, s)
                ev.stop()
                stream_synchronize(stream)
                ms = ev.ms()
            lo, hi = range_host if range_host is not None else dc.range()[0]
            pic = dc.result()[0].copy() if big is None else big.host.reshape(H, W, 3).copy()
            return ms, pic, (float(lo), float(hi))
    finally:
        if big is not None:
            big.free()


def device_distribution(d_map: int, h: int, w: int, stream: int) -> Optional[dict]:
    """demo.py:distribution of the device map [h][w] at `d_map`: one call of
    mde_op_depth_quantiles with DISTRIBUTION_Q, 64 bytes come back."""
    with DeviceQuantiles(1, h, w) as dq:
        return distribution_row(dq.run(d_map, stream, DISTRIBUTION_Q).copy()[0], h * w)


def add_robust_arguments(ap) -> None:
    ap.add_argument("--color-robust", type=float, nargs="*", default=None, metavar="PCT",
                    help="draw on the map's own LO..HI percentile range (default 2 98; the reference's "
                         "core/viz.py:robust_range) instead of its min..max recipe, and print its p02 / median / p98")
    ap.add_argument("--color-robust-near", action="store_true",
                    help="the robust range of proximity (1 / depth for a depth output; core/viz.py:"
                         "qualitative_display): warm is near")


def add_color_arguments(ap) -> None:
    """The model drivers' --color options."""
    ap.add_argument("--color", default="", metavar="PATH",
                    help="write the turbo-coloured BGR picture of the depth map (an image file with Pillow, else .npy)")
    ap.add_argument("--color-range", type=float, nargs=2, default=None, metavar=("VMIN", "VMAX"),
                    help="with --color: draw depth on this fixed axis in metres instead of the map's own range")
    add_robust_arguments(ap)


def robust_percent(a) -> Optional[Tuple[float, float]]:
    """(LO, HI) when --color-robust or --color-robust-near asks for the robust
    range, else None; SystemExit for anything but none or two percentages."""
    given = getattr(a, "color_robust", None)
    if given is None:
        return (2.0, 98.0) if getattr(a, "color_robust_near", False) else None
    if len(given) == 0:
        return (2.0, 98.0)
    if len(given) != 2 or not all(0.0 <= v <= 100.0 for v in given):
        raise SystemExit("--color-robust takes nothing or LO HI, two percentages in 0..100")
    return (float(given[0]), float(given[1]))


def check_color_arguments(a, device_map: bool) -> None:
    """--color's conditions that can be answered before an engine is built;
    SystemExit otherwise."""
    robust = robust_percent(a)
    if robust is not None and a.color_range is not None:
        raise SystemExit("--color-robust and --color-range exclude each other")
    if not a.color:
        if a.color_range is not None:
            raise SystemExit("--color-range goes with --color")
        if robust is not None:
            raise SystemExit("--color-robust goes with --color")
        return
    if not device_map:
        raise SystemExit("--color runs on the device post-process's depth map: do not combine it with "
                         "--host-postprocess")
    if a.color_range is not None and not all(v == v for v in a.color_range):
        raise SystemExit("--color-range must not be NaN")


def color_kwargs(a, model_spec: dict) -> dict:
    """mode and its arguments for DeviceColorize.enqueue from the drivers'
    options and the model's spec."""
    if getattr(a, "color_range", None) is not None:
        return {"mode": "fixed", "vmin": float(a.color_range[0]), "vmax": float(a.color_range[1])}
    robust = robust_percent(a)
    if robust is not None:
        # robust_range ignores non-positive values; what is ranged follows the spec as mode_for does: a
        # metric map is depth (its proximity is 1 / depth), the relative driver's is drawn as it is
        near = bool(getattr(a, "color_robust_near", False))
        return {"mode": "robust", "q_percent": robust, "positive_only": True,
                "reciprocal": near and model_spec.get("depth_scale") != "relative"}
    return {"mode": mode_for(model_spec)}


def pooled_range(a, model_spec: dict, d_maps: int, batch: int, hw, stream: int):
    """The robust options' range pooled over `batch` device maps [hw] at
    `d_maps` (core/viz.py: "pooled, not per-array"): (DeviceQuantiles that
    holds it on the device, (vmin, vmax)), or None without those options.
    The caller frees the DeviceQuantiles after the last driver_color."""
    kw = color_kwargs(a, model_spec)
    if kw["mode"] != "robust":
        return None
    dq = DeviceQuantiles(batch, hw[0], hw[1])
    try:
        row = dq.run(d_maps, stream, kw["q_percent"], positive_only=kw["positive_only"],
                     reciprocal=kw["reciprocal"], pooled=True, sample_cap=SAMPLE_CAP)[0]
        return dq, (float(row[Q_VMIN]), float(row[Q_VMAX]))
    except Exception:
        dq.free()
        raise


def driver_color(a, model_spec: dict, d_map: int, hw, stream: int, resize_hw=None,
                 denom_eps: float = 0.0, shared=None) -> np.ndarray:
    """The drivers' --color: colour the device map [hw] at `d_map`, print the
    `[MDET] color : ...` line and write the picture.  `resize_hw`: resize it to
    that size on the device first (device_color); `denom_eps`: the epsilon of
    the inverse_auto recipe's denominator (the VGGT driver's 1e-6); `shared`:
    what pooled_range returned, the axis this map shares with others.  With
    the robust options one `[MDET] depth : ...` line follows."""
    kw = color_kwargs(a, model_spec)
    if kw["mode"] == "inverse_auto":
        kw["denom_eps"] = denom_eps
    if kw["mode"] == "robust" and shared is not None:
        kw["d_range"] = shared[0].out.device + 8 * Q_VMIN
        kw["range_host"] = shared[1]
    ms, bgr, (lo, hi) = device_color(d_map, hw[0], hw[1], stream, resize_hw=resize_hw, **kw)
    path = save_image(a.color, bgr)
    print(f"[MDET] color : mode {kw['mode']} range {lo:0.6g}..{hi:0.6g} (device, kernels + D2H of {bgr.nbytes} "
          f"bytes, hipEvents: {ms:0.3f} ms) -> {path}")
    if kw["mode"] == "robust":
        print(format_distribution(device_distribution(d_map, hw[0], hw[1], stream)))
    return bgr


__all__ = ["MODES", "TILE", "BAD", "BAD_VIZ", "lut", "mode_index", "mode_for", "index_np", "colorize_np", "ws_bytes",
           "depth_colorize", "DeviceColorize", "save_image", "device_color", "add_color_arguments",
           "check_color_arguments", "color_kwargs", "driver_color", "SAMPLE_CAP", "ROW", "DISTRIBUTION_Q",
           "quantiles_np", "row_quantiles", "robust_range_np", "distribution_row", "distribution_np",
           "format_distribution", "colorize_ranged_np", "quantiles_ws_bytes", "depth_quantiles",
           "depth_colorize_ranged", "DeviceQuantiles", "device_distribution", "add_robust_arguments",
           "robust_percent", "pooled_range"]
