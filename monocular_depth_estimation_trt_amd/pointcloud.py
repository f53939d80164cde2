"""Point clouds on the device: the tail of the reference's
`models/depth_pro/onnx2trt_pointcloud.py:172-184` -- pinhole unprojection of
the metric depth map at the photo's size, colours from the photo, a `.ply` --
as `mde_op_point_cloud` (csrc/point_cloud.hip): the depth map that the device
post-process left in device memory is unprojected, invalid pixels are dropped
in row-major order and the survivors are packed as PLY binary_little_endian
vertex records, so the D2H copy carries the file's body.

`unproject_np` restates the include/mde.h contract in numpy float32 (the
kernels are held to it bit for bit), `DevicePointCloud` owns the buffers and
drives the op, `write_ply` / `read_ply` put the records into a file and read
them back.
"""

from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np

from . import _lib
from .common_runtime import HostDeviceMem, stream_synchronize

_XYZ = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
_RGB = [("red", "u1"), ("green", "u1"), ("blue", "u1")]
_PLY_TYPE = {"<f4": "float", "|u1": "uchar"}


def vertex_dtype(colour: bool) -> np.dtype:
    """The packed PLY vertex record: x, y, z float32 little-endian, then red,
    green, blue uint8 when `colour`; itemsize 15 or 12, no padding."""
    return np.dtype(_XYZ + (_RGB if colour else []))


def grid(h: int, w: int, step: int = 1):
    """(hs, ws): the sampled grid of every step-th pixel on both axes."""
    if h < 1 or w < 1 or step < 1:
        raise ValueError("h, w and step must be positive")
    return -(-int(h) // int(step)), -(-int(w) // int(step))


def unproject_np(depth, fx, fy, cx, cy, photo=None, swap_rb=False, step=1, compact=False, z_lo=1e-4, z_hi=1e4):
    """The include/mde.h contract of mde_op_point_cloud for one image, in numpy
    float32 with one rounding per operation:

        xn = (float32(u) - cx) / fx,  yn = (float32(v) - cy) / fy
        X = xn * z,  Y = yn * z,  Z = z

    over the pixels (v, u) = (i * step, j * step).  depth: [h, w]; photo:
    optional uint8 [h, w, 3] (any strides), its channels reversed when swap_rb.
    Returns a 1-D `vertex_dtype` array in row-major pixel order: all hs * ws
    samples when not compact (a NaN z gives NaN x, y, z), else those with
    z == z and z_lo <= z <= z_hi."""
    f32 = np.float32
    z = np.asarray(depth, dtype=np.float32)
    if z.ndim != 2:
        raise ValueError(f"depth must be [h, w], got {z.shape}")
    h, w = z.shape
    hs, ws = grid(h, w, step)
    z = z[::step, ::step]
    u = np.arange(ws, dtype=np.int64) * step
    v = np.arange(hs, dtype=np.int64) * step
    with np.errstate(invalid="ignore", over="ignore"):
        xn = (u.astype(f32) - f32(cx)) / f32(fx)
        yn = (v.astype(f32) - f32(cy)) / f32(fy)
        x = xn[None, :] * z
        y = yn[:, None] * z
    assert x.dtype == y.dtype == np.float32
    out = np.empty((hs, ws), vertex_dtype(photo is not None))
    out["x"], out["y"], out["z"] = x, y, z
    if photo is not None:
        p = np.asarray(photo)
        if p.dtype != np.uint8 or p.shape != (h, w, 3):
            raise ValueError(f"photo must be uint8 [{h}, {w}, 3], got {p.dtype} {p.shape}")
        p = p[::step, ::step]
        r, b = (2, 0) if swap_rb else (0, 2)
        out["red"], out["green"], out["blue"] = p[..., r], p[..., 1], p[..., b]
    out = out.reshape(-1)
    if compact:
        zf = z.reshape(-1)
        with np.errstate(invalid="ignore"):
            out = out[(zf == zf) & (zf >= f32(z_lo)) & (zf <= f32(z_hi))]
    return out


def ws_bytes(batch: int, h: int, w: int, step: int = 1) -> int:
    """Device scratch the compact mode needs (mde_op_point_cloud_ws_bytes)."""
    return int(_lib.lib().mde_op_point_cloud_ws_bytes(int(batch), int(h), int(w), int(step)))


def point_cloud(d_depth: int, batch: int, h: int, w: int, step: int, d_photo: int, pitch: int, swap_rb: bool,
                d_f_px: int, fx: float, fy: float, cx: float, cy: float, compact: bool, z_lo: float, z_hi: float,
                d_records: int, records_bytes: int, d_counts: int, d_ws: int, ws_nbytes: int, stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream` (mde_op_point_cloud)."""
    _lib.call("mde_op_point_cloud", C.c_void_p(int(d_depth)), int(batch), int(h), int(w), int(step),
              C.c_void_p(int(d_photo or 0)), int(pitch), int(bool(swap_rb)), C.c_void_p(int(d_f_px or 0)),
              float(fx), float(fy), float(cx), float(cy), int(bool(compact)), float(z_lo), float(z_hi),
              C.c_void_p(int(d_records)), int(records_bytes), C.c_void_p(int(d_counts)), C.c_void_p(int(d_ws or 0)),
              int(ws_nbytes), C.c_void_p(int(stream or 0)))


class DevicePointCloud:
    """Owns the vertex records and the counts (device + pinned host) and the
    compaction scratch for `batch` depth maps [h, w], with or without colour,
    sampling every `step`-th pixel.

    enqueue(d_depth, stream, ...) only enqueues the kernels (capturable);
    download(stream) brings the counts back, synchronizes, then copies only
    the counted bytes of each image's region and synchronizes again; result()
    is one `vertex_dtype` view of counts[b] records per image, valid until the
    next download; run() = enqueue, download, result."""

    def __init__(self, batch: int, h: int, w: int, colour: bool, step: int = 1):
        self.batch, self.h, self.w, self.step = int(batch), int(h), int(w), int(step)
        self.colour = bool(colour)
        self.hs, self.ws = grid(self.h, self.w, self.step)
        self.dtype = vertex_dtype(self.colour)
        self.region = self.hs * self.ws * self.dtype.itemsize  # bytes per image
        self.records: Optional[HostDeviceMem] = None
        self.counts: Optional[HostDeviceMem] = None
        self._ws = 0
        self._ws_bytes = ws_bytes(self.batch, self.h, self.w, self.step)
        if self._ws_bytes == 0:
            raise ValueError(f"mde_op_point_cloud does not take batch {batch}, {h}x{w}, step {step}")
        try:
            self.records = HostDeviceMem(self.batch * self.region, np.uint8)
            self.counts = HostDeviceMem(self.batch, np.dtype(np.int32))
            p = C.c_void_p()
            _lib.call("mde_rt_malloc", C.byref(p), self._ws_bytes)
            self._ws = int(p.value)
        except Exception:
            self.free()
            raise

    def enqueue(self, d_depth: int, stream: int, d_photo: int = 0, pitch: int = 0, swap_rb: bool = False,
                d_f_px: int = 0, fx: Optional[float] = None, fy: Optional[float] = None,
                cx: Optional[float] = None, cy: Optional[float] = None, compact: bool = True,
                z_lo: float = 1e-4, z_hi: float = 1e4) -> None:
        """The kernels on `stream`, nothing else.  d_f_px: device float[batch]
        focal lengths (DepthProDevicePostprocess.f_px.device), else fx (and fy,
        default fx); cx, cy default to w / 2, h / 2 like the reference."""
        if self.records is None:
            raise RuntimeError("DevicePointCloud already freed")
        if bool(d_photo) != self.colour:
            raise ValueError("DevicePointCloud(colour=%s) %s a photo" % (self.colour, "needs" if self.colour else
                                                                         "does not take"))
        if not d_f_px and fx is None:
            raise ValueError("DevicePointCloud.enqueue needs d_f_px or fx")
        fx = 0.0 if fx is None else float(fx)
        fy = fx if fy is None else float(fy)
        point_cloud(d_depth, self.batch, self.h, self.w, self.step, d_photo, pitch or 3 * self.w, swap_rb, d_f_px,
                    fx, fy, self.w / 2 if cx is None else cx, self.h / 2 if cy is None else cy, compact, z_lo, z_hi,
                    self.records.device, self.records.nbytes, self.counts.device, self._ws, self._ws_bytes, stream)

    def download(self, stream: int) -> None:
        """Counts first, then only the counted bytes; synchronizes `stream` twice."""
        if self.records is None:
            raise RuntimeError("DevicePointCloud already freed")
        s = C.c_void_p(int(stream or 0))
        _lib.call("mde_rt_memcpy_dtoh_async", self.counts.host.ctypes.data_as(C.c_void_p),
                  C.c_void_p(self.counts.device), self.counts.nbytes, s)
        stream_synchronize(stream)
        host = self.records.host
        for b in range(self.batch):
            n = int(self.counts.host[b]) * self.dtype.itemsize
            if n:
                _lib.call("mde_rt_memcpy_dtoh_async", C.c_void_p(host.ctypes.data + b * self.region),
                          C.c_void_p(self.records.device + b * self.region), n, s)
        stream_synchronize(stream)

    def result(self) -> List[np.ndarray]:
        """One view of counts[b] records per image; valid after download()."""
        if self.records is None:
            raise RuntimeError("DevicePointCloud already freed")
        host, item = self.records.host, self.dtype.itemsize
        return [host[b * self.region:b * self.region + int(self.counts.host[b]) * item].view(self.dtype)
                for b in range(self.batch)]

    def run(self, d_depth: int, stream: int, **kw) -> List[np.ndarray]:
        self.enqueue(d_depth, stream, **kw)
        self.download(stream)
        return self.result()

    def free(self) -> None:
        for m in (self.records, self.counts):
            if m is not None:
                m.free()
        self.records = self.counts = None
        if self._ws:
            _lib.call("mde_rt_free", C.c_void_p(self._ws))
            self._ws = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def device_ply(path, d_depth: int, h: int, w: int, stream: int, step: int = 1, img_bgr: Optional[np.ndarray] = None,
               d_f_px: int = 0, f_px: Optional[float] = None, z_lo: float = 1e-4, z_hi: float = 1e4):
    """What the model drivers' --ply does: DevicePointCloud in compact mode on
    one device depth map [h][w] at `d_depth`, with the given `f_px` or else the
    device focal length `d_f_px`, cx, cy = w / 2, h / 2, colours from the BGR
    photo `img_bgr` [h, w, 3] (uploaded here, once, before the timed part),
    written to `path`.  Returns (ms of the kernels + D2H between two hipEvents
    on `stream`, number of points)."""
    if img_bgr is not None and (img_bgr.dtype != np.uint8 or img_bgr.shape != (h, w, 3)):
        raise ValueError(f"the photo must be uint8 [{h}, {w}, 3], got {img_bgr.dtype} {img_bgr.shape}")
    s = C.c_void_p(int(stream or 0))
    photo = None
    ev = [C.c_void_p(), C.c_void_p()]
    try:
        for e in ev:
            _lib.call("mde_rt_event_create", C.byref(e))
        if img_bgr is not None:
            photo = HostDeviceMem(h * w * 3, np.uint8)
            photo.host = np.ascontiguousarray(img_bgr).reshape(-1)
            _lib.call("mde_rt_memcpy_htod_async", C.c_void_p(photo.device), photo.host.ctypes.data_as(C.c_void_p),
                      photo.nbytes, s)
        with DevicePointCloud(1, h, w, colour=photo is not None, step=step) as cloud:
            _lib.call("mde_rt_event_record", ev[0], s)
            cloud.enqueue(d_depth, stream, d_photo=photo.device if photo else 0, pitch=3 * w, swap_rb=True,
                          d_f_px=0 if f_px is not None else d_f_px, fx=f_px, z_lo=z_lo, z_hi=z_hi)
            cloud.download(stream)
            _lib.call("mde_rt_event_record", ev[1], s)
            stream_synchronize(stream)
            records = cloud.result()[0]
            write_ply(path, records)
            ms = C.c_float()
            _lib.call("mde_rt_event_elapsed_ms", C.byref(ms), ev[0], ev[1])
            return float(ms.value), int(records.shape[0])
    finally:
        if photo is not None:
            photo.free()
        for e in ev:
            if e:
                _lib.call("mde_rt_event_destroy", e)


def ply_header(count: int, colour: bool) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(count)}"]
    lines += [f"property {_PLY_TYPE[np.dtype(t).str]} {name}" for name, t in _XYZ + (_RGB if colour else [])]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_ply(path, records: np.ndarray) -> None:
    """The ASCII header, then the bytes of `records` (a 1-D `vertex_dtype`
    array, e.g. one element of DevicePointCloud.result()) as they are."""
    records = np.asarray(records)
    colour = records.dtype == vertex_dtype(True)
    if records.ndim != 1 or not (colour or records.dtype == vertex_dtype(False)):
        raise ValueError(f"write_ply wants a 1-D vertex_dtype array, got {records.dtype} {records.shape}")
    with open(path, "wb") as f:
        f.write(ply_header(records.shape[0], colour))
        f.write(np.ascontiguousarray(records).tobytes())


def read_ply(path) -> np.ndarray:
    """Read a file of exactly write_ply's form back into a `vertex_dtype` array."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: no PLY header")
    body = end + len(b"end_header\n")
    lines = data[:body].decode("ascii", errors="replace").split("\n")
    if len(lines) < 3 or not lines[2].startswith("element vertex "):
        raise ValueError(f"{path}: not a vertex-only PLY header")
    count = int(lines[2][len("element vertex "):])
    for colour in (True, False):
        if data[:body] == ply_header(count, colour):
            dt = vertex_dtype(colour)
            if len(data) - body != count * dt.itemsize:
                raise ValueError(f"{path}: {len(data) - body} body bytes, the header promises {count * dt.itemsize}")
            return np.frombuffer(data, dtype=dt, count=count, offset=body).copy()
    raise ValueError(f"{path}: the header is not one write_ply writes")


__all__ = ["vertex_dtype", "grid", "unproject_np", "ws_bytes", "point_cloud", "DevicePointCloud", "device_ply", "ply_header",
           "write_ply", "read_ply"]
