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
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib, colormaps
from .common_runtime import HostDeviceMem, stream_synchronize
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
    download, result."""

    def __init__(self, batch: int, h: int, w: int, cmap: str = "turbo"):
        self.batch, self.h, self.w = int(batch), int(h), int(w)
        self.cmap = cmap
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
        except Exception:
            self.free()
            raise

    def _alive(self):
        if self.out is None:
            raise RuntimeError("DeviceColorize already freed")

    def enqueue(self, d_map: int, stream: int, mode, map_is_inverse: bool = False, denom_eps: float = 0.0,
                vmin: Optional[float] = None, vmax: Optional[float] = None, swap_rb: bool = True) -> None:
        """The kernels on `stream`, nothing else.  d_map: device float32
        [batch][h][w] (DevicePostprocess.mem.device).  A pixel without an index
        is drawn BAD_VIZ in mode 'fixed', black otherwise."""
        self._alive()
        mode = MODES[mode_index(mode)]
        if mode == "fixed" and (vmin is None or vmax is None):
            raise ValueError("mode 'fixed' needs vmin and vmax")
        d_lut = self.lut.device + (257 * 3 if mode == "fixed" else 0)
        depth_colorize(d_map, self.batch, self.h, self.w, mode, map_is_inverse, denom_eps, vmin, vmax, d_lut, swap_rb,
                       self.out.device, self.rng.device, self._ws, self._ws_bytes, stream)

    def download(self, stream: int) -> None:
        self._alive()
        for m in (self.out, self.rng):
            _lib.call("mde_rt_memcpy_dtoh_async", m.host.ctypes.data_as(C.c_void_p), C.c_void_p(m.device), m.nbytes,
                      C.c_void_p(int(stream or 0)))
        stream_synchronize(stream)

    def result(self) -> np.ndarray:
        """The picture, uint8 [batch, h, w, 3]; valid after download()."""
        self._alive()
        return self.out.host.reshape(self.batch, self.h, self.w, 3)

    def range(self) -> np.ndarray:
        """float32 [batch, 2]: the range each image was drawn on; valid after download()."""
        self._alive()
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
    the photo's size) and only the resized one, [H, W, 3], is downloaded."""
    s = C.c_void_p(int(stream or 0))
    ev = [C.c_void_p(), C.c_void_p()]
    big = None
    try:
        for e in ev:
            _lib.call("mde_rt_event_create", C.byref(e))
        with DeviceColorize(1, h, w) as dc:
            if resize_hw is not None:
                H, W = int(resize_hw[0]), int(resize_hw[1])
                big = HostDeviceMem(H * W * 3, np.uint8)
            _lib.call("mde_rt_event_record", ev[0], s)
            dc.enqueue(d_map, stream, mode, **kw)
            if big is None:
                dc.download(stream)
            else:
                resize_u8(dc.out.device, 1, h, w, 3 * w, False, big.device, H, W, stream)
                for m in (big, dc.rng):
                    _lib.call("mde_rt_memcpy_dtoh_async", m.host.ctypes.data_as(C.c_void_p), C.c_void_p(m.device),
                              m.nbytes, s)
            _lib.call("mde_rt_event_record", ev[1], s)
            stream_synchronize(stream)
            ms = C.c_float()
            _lib.call("mde_rt_event_elapsed_ms", C.byref(ms), ev[0], ev[1])
            lo, hi = dc.range()[0]
            pic = dc.result()[0].copy() if big is None else big.host.reshape(H, W, 3).copy()
            return float(ms.value), pic, (float(lo), float(hi))
    finally:
        if big is not None:
            big.free()
        for e in ev:
            if e:
                _lib.call("mde_rt_event_destroy", e)


def add_color_arguments(ap) -> None:
    """The model drivers' --color options."""
    ap.add_argument("--color", default="", metavar="PATH",
                    help="write the turbo-coloured BGR picture of the depth map (an image file with Pillow, else .npy)")
    ap.add_argument("--color-range", type=float, nargs=2, default=None, metavar=("VMIN", "VMAX"),
                    help="with --color: draw depth on this fixed axis in metres instead of the map's own range")


def check_color_arguments(a, device_map: bool) -> None:
    """--color's conditions that can be answered before an engine is built;
    SystemExit otherwise."""
    if not a.color:
        if a.color_range is not None:
            raise SystemExit("--color-range goes with --color")
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
    return {"mode": mode_for(model_spec)}


def driver_color(a, model_spec: dict, d_map: int, hw, stream: int, resize_hw=None,
                 denom_eps: float = 0.0) -> np.ndarray:
    """The drivers' --color: colour the device map [hw] at `d_map`, print the
    `[MDET] color : ...` line and write the picture.  `resize_hw`: resize it to
    that size on the device first (device_color); `denom_eps`: the epsilon of
    the inverse_auto recipe's denominator (the VGGT driver's 1e-6)."""
    kw = color_kwargs(a, model_spec)
    if kw["mode"] == "inverse_auto":
        kw["denom_eps"] = denom_eps
    ms, bgr, (lo, hi) = device_color(d_map, hw[0], hw[1], stream, resize_hw=resize_hw, **kw)
    path = save_image(a.color, bgr)
    print(f"[MDET] color : mode {kw['mode']} range {lo:0.6g}..{hi:0.6g} (device, kernels + D2H of {bgr.nbytes} "
          f"bytes, hipEvents: {ms:0.3f} ms) -> {path}")
    return bgr


__all__ = ["MODES", "TILE", "BAD", "BAD_VIZ", "lut", "mode_index", "mode_for", "index_np", "colorize_np", "ws_bytes",
           "depth_colorize", "DeviceColorize", "save_image", "device_color", "add_color_arguments",
           "check_color_arguments", "color_kwargs", "driver_color"]
