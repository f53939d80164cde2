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

The preview of that cloud -- the reference's `core/viz.py:render_points`, what
`demo.py:cloud_figure` shows: an orthographic, z-buffered picture seen from
above-left -- is `mde_op_cloud_view` (csrc/cloud_view.hip), drawn from the
depth map without the records leaving the device.  `render_np` restates its
contract in numpy (the kernels are held to it, the picture byte for byte and
the view row bit for bit), `DeviceCloudView` owns the buffers and drives the
op, `device_cloud_view` is what the drivers' `--cloud-view` calls.

The mesh of that cloud -- the reference's `models/metric_anything/
demo_pointcloud.py:142-149`: depth edges (flying pixels) dropped, two triangles
per surviving 2 x 2 block, no unreferenced vertices -- is `mde_op_depth_mesh`
(csrc/depth_mesh.hip).  `mesh_np` restates its contract in numpy float32 (the
kernels are held to it byte for byte), `DeviceMesh` owns the buffers and
drives the op, `write_ply_mesh` / `read_ply_mesh` handle the vertex + face
PLY, `device_mesh` is what the drivers' `--mesh` and `--ply-edge-rtol` call.

The three Device* classes take the same cloud source -- a device depth map, a
sampling step, an optional device photo, a focal length on the device or on
the host, cx, cy -- and share `_CloudOp` for it.

The drivers' cloud outputs (models/depth_pro/run.py, models/depth_anything_v2/
run.py and the models that go through it) are one stage here:
`add_cloud_arguments` declares the options, `check_cloud_arguments` and
`check_photo_size` refuse what cannot be served, `run_cloud_outputs` uploads
the `--image` photo once and runs, in this order, each with one `[MDET]` line:

`--ply PATH [--ply-step N]`: the reference's onnx2trt_pointcloud.py:172-184.
The metric depth at the source size is unprojected with the focal length
(x = (u - W/2) / f_px * z, y likewise) and written as a binary PLY, coloured
from the `--image` photo (no colours without one).  It runs on the device
(`DevicePointCloud`) on the map the device post-process left there, drops
depths outside the driver's clamp and downloads the PLY records; `--ply-step
N` keeps every N-th pixel on both axes.  `--ply-edge-rtol R` gives the cloud
`--mesh`'s edge filter (no flying pixels), without faces.

`--mesh PATH [--mesh-step N] [--edge-rtol R] [--edge-atol A]`: the reference's
demo_pointcloud.py:142-149.  The samples on a depth edge -- a 3x3 spread of
depth above `--edge-rtol` (default 0.1, the reference's) times the depth, or
above `--edge-atol` metres -- are dropped, the 2x2 blocks that survive whole
become two triangles each, and the vertices they use and the faces are packed
on the device (`DeviceMesh`) and written as a binary PLY with `element vertex`
and `element face`.

`--cloud-view PATH [--cloud-view-size H W] [--cloud-view-angles ELEV AZIM]
[--cloud-view-step N]`: the reference's core/viz.py:render_points.  An
orthographic, z-buffered picture of that cloud seen from above-left, drawn on
the device (`DeviceCloudView`); only the picture comes back, and the file is
written like `--color`'s (visualize.save_image).
"""

from __future__ import annotations

import contextlib
import ctypes as C
from typing import List, Optional

import numpy as np

from . import _lib
from .common_runtime import EventPair, HostDeviceMem, stream_synchronize

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


class _CloudOp:
    """What DevicePointCloud, DeviceMesh and DeviceCloudView share: the cloud
    source's geometry and `colour` flag, the op's scratch, the checks and the
    camera defaults of enqueue's source arguments, and the release.  A
    subclass names its op and its HostDeviceMem attributes; the first of them
    being None means freed."""

    _OP = ""
    _BUFFERS = ()

    def __init__(self, batch: int, h: int, w: int, colour: bool, step: int):
        self.batch, self.h, self.w, self.step = int(batch), int(h), int(w), int(step)
        self.colour = bool(colour)
        for name in self._BUFFERS:
            setattr(self, name, None)
        self._ws = 0
        self._ws_bytes = 0

    def _allocate(self, ws_nbytes: int, geometry: str, **buffers) -> None:
        """The scratch of `ws_nbytes` (0: the op refuses `geometry`) and the
        named buffers, each a (size, dtype) for HostDeviceMem."""
        self._ws_bytes = ws_nbytes
        if ws_nbytes == 0:
            raise ValueError(f"{self._OP} does not take {geometry}")
        try:
            for name, (size, dtype) in buffers.items():
                setattr(self, name, HostDeviceMem(size, dtype))
            p = C.c_void_p()
            _lib.call("mde_rt_malloc", C.byref(p), self._ws_bytes)
            self._ws = int(p.value)
        except Exception:
            self.free()
            raise

    def _live(self) -> None:
        if getattr(self, self._BUFFERS[0]) is None:
            raise RuntimeError(f"{type(self).__name__} already freed")

    def _source(self, d_depth, d_photo, pitch, swap_rb, d_f_px, fx, fy, cx, cy):
        """The thirteen cloud-source arguments of the op from enqueue's: fy
        defaults to fx, cx, cy to w / 2, h / 2 like the reference, the pitch to
        packed rows."""
        name = type(self).__name__
        self._live()
        if bool(d_photo) != self.colour:
            raise ValueError(f"{name}(colour={self.colour}) {'needs' if self.colour else 'does not take'} a photo")
        if not d_f_px and fx is None:
            raise ValueError(f"{name}.enqueue needs d_f_px or fx")
        fx = 0.0 if fx is None else float(fx)
        fy = fx if fy is None else float(fy)
        return (d_depth, self.batch, self.h, self.w, self.step, d_photo, pitch or 3 * self.w, swap_rb, d_f_px, fx, fy,
                self.w / 2 if cx is None else cx, self.h / 2 if cy is None else cy)

    def run(self, d_depth: int, stream: int, **kw):
        self.enqueue(d_depth, stream, **kw)
        self.download(stream)
        return self.result()

    def free(self) -> None:
        for name in self._BUFFERS:
            if getattr(self, name) is not None:
                getattr(self, name).free()
            setattr(self, name, None)
        if self._ws:
            _lib.call("mde_rt_free", C.c_void_p(self._ws))
            self._ws = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


class DevicePointCloud(_CloudOp):
    """Owns the vertex records and the counts (device + pinned host) and the
    compaction scratch for `batch` depth maps [h, w], with or without colour,
    sampling every `step`-th pixel.

    enqueue(d_depth, stream, ...) only enqueues the kernels (capturable);
    download(stream) brings the counts back, synchronizes, then copies only
    the counted bytes of each image's region and synchronizes again; result()
    is one `vertex_dtype` view of counts[b] records per image, valid until the
    next download; run() = enqueue, download, result."""

    _OP = "mde_op_point_cloud"
    _BUFFERS = ("records", "counts")

    def __init__(self, batch: int, h: int, w: int, colour: bool, step: int = 1):
        super().__init__(batch, h, w, colour, step)
        self.hs, self.ws = grid(self.h, self.w, self.step)
        self.dtype = vertex_dtype(self.colour)
        self.region = self.hs * self.ws * self.dtype.itemsize  # bytes per image
        self._allocate(ws_bytes(self.batch, self.h, self.w, self.step), f"batch {batch}, {h}x{w}, step {step}",
                       records=(self.batch * self.region, np.uint8), counts=(self.batch, np.dtype(np.int32)))

    def enqueue(self, d_depth: int, stream: int, d_photo: int = 0, pitch: int = 0, swap_rb: bool = False,
                d_f_px: int = 0, fx: Optional[float] = None, fy: Optional[float] = None,
                cx: Optional[float] = None, cy: Optional[float] = None, compact: bool = True,
                z_lo: float = 1e-4, z_hi: float = 1e4) -> None:
        """The kernels on `stream`, nothing else.  d_f_px: device float[batch]
        focal lengths (DepthProDevicePostprocess.f_px.device), else fx (and fy,
        default fx); cx, cy default to w / 2, h / 2 like the reference."""
        point_cloud(*self._source(d_depth, d_photo, pitch, swap_rb, d_f_px, fx, fy, cx, cy), compact, z_lo, z_hi,
                    self.records.device, self.records.nbytes, self.counts.device, self._ws, self._ws_bytes, stream)

    def download(self, stream: int) -> None:
        """Counts first, then only the counted bytes; synchronizes `stream` twice."""
        self._live()
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
        self._live()
        host, item = self.records.host, self.dtype.itemsize
        return [host[b * self.region:b * self.region + int(self.counts.host[b]) * item].view(self.dtype)
                for b in range(self.batch)]


@contextlib.contextmanager
def _device_photo(img_bgr, d_photo: int, h: int, w: int, stream: int):
    """The device pointer of the drivers' BGR photo (0: no colours): `d_photo`
    when the caller has uploaded it already, else `img_bgr`, checked against
    uint8 [h, w, 3] and uploaded once on `stream`, freed when the block ends."""
    if d_photo or img_bgr is None:
        yield int(d_photo or 0)
        return
    if img_bgr.dtype != np.uint8 or img_bgr.shape != (h, w, 3):
        raise ValueError(f"the photo must be uint8 [{h}, {w}, 3], got {img_bgr.dtype} {img_bgr.shape}")
    photo = HostDeviceMem(h * w * 3, np.uint8)
    try:
        photo.host = np.ascontiguousarray(img_bgr).reshape(-1)
        _lib.call("mde_rt_memcpy_htod_async", C.c_void_p(photo.device), photo.host.ctypes.data_as(C.c_void_p),
                  photo.nbytes, C.c_void_p(int(stream or 0)))
        yield photo.device
    finally:
        photo.free()


def _timed(op: _CloudOp, d_depth: int, stream: int, d_photo: int, d_f_px: int, f_px, **kw) -> float:
    """enqueue + download of `op` with the drivers' camera -- the BGR photo at
    `d_photo`, the given `f_px` or else the device focal length `d_f_px`, cx,
    cy = w / 2, h / 2 -- between two hipEvents on `stream`; the ms."""
    with EventPair(stream) as ev:
        op.enqueue(d_depth, stream, d_photo=d_photo, pitch=3 * op.w, swap_rb=True,
                   d_f_px=0 if f_px is not None else d_f_px, fx=f_px, **kw)
        op.download(stream)
        ev.stop()
        stream_synchronize(stream)
        return ev.ms()


def device_ply(path, d_depth: int, h: int, w: int, stream: int, step: int = 1, img_bgr: Optional[np.ndarray] = None,
               d_f_px: int = 0, f_px: Optional[float] = None, z_lo: float = 1e-4, z_hi: float = 1e4, d_photo: int = 0):
    """What the model drivers' --ply does: DevicePointCloud in compact mode on
    one device depth map [h][w] at `d_depth`, with the given `f_px` or else the
    device focal length `d_f_px`, cx, cy = w / 2, h / 2, colours from the BGR
    photo `img_bgr` [h, w, 3] (uploaded here, once, before the timed part) or
    the one already at `d_photo`, written to `path`.  Returns (ms of the
    kernels + D2H between two hipEvents on `stream`, number of points)."""
    with _device_photo(img_bgr, d_photo, h, w, stream) as d_photo, \
            DevicePointCloud(1, h, w, colour=bool(d_photo), step=step) as cloud:
        ms = _timed(cloud, d_depth, stream, d_photo, d_f_px, f_px, z_lo=z_lo, z_hi=z_hi)
        records = cloud.result()[0]
        write_ply(path, records)
        return ms, int(records.shape[0])


VIEW_ROW = 8             # doubles per view row of mde_op_cloud_view
# view_out[b][.] of mde_op_cloud_view (include/mde.h)
V_NVALID, V_C0, V_C1, V_C2, V_SPAN, V_SCALE, V_INSIDE = range(7)
VIEW_SIZE = (320, 420)   # core/viz.py:render_points' defaults
VIEW_ANGLES = (-18.0, 24.0)
VIEW_BG = (22, 22, 26)
VIEW_GREY = 200          # the colour of a cloud without a photo


def view_trig(elev_deg: float, azim_deg: float):
    """(cos_a, sin_a, cos_e, sin_e) as the reference forms them: np.cos / np.sin
    of np.deg2rad of the azimuth and the elevation."""
    a, e = np.deg2rad(np.float64(azim_deg)), np.deg2rad(np.float64(elev_deg))
    return float(np.cos(a)), float(np.sin(a)), float(np.cos(e)), float(np.sin(e))


def _order_key(x32: np.ndarray) -> np.ndarray:
    """The order-preserving uint32 key of float32 values (csrc/depth_quantiles.hip's
    plain key): -0 counts as +0."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def render_np(depth, fx, fy, cx, cy, size=VIEW_SIZE, elev_deg=VIEW_ANGLES[0], azim_deg=VIEW_ANGLES[1], photo=None,
              swap_rb=False, step=1, view=None, bg=VIEW_BG):
    """The include/mde.h contract of mde_op_cloud_view for one image, in numpy:
    the reference's core/viz.py:render_points on the cloud of `unproject_np`,
    with the centre and the span from `visualize.quantiles_np` and a packed
    64-bit minimum for the z-test.  Returns (picture uint8 [out_h, out_w, 3]
    in R, G, B order, view row float64 [8]).  `view`: a view row whose centre
    and scale (slots 1, 2, 3, 5) are used instead of selecting them."""
    from .visualize import Q_NVALID, Q_Q0, quantiles_np
    out_h, out_w = int(size[0]), int(size[1])
    if out_h < 1 or out_w < 1:
        raise ValueError("the picture's sizes must be positive")
    rec = unproject_np(depth, fx, fy, cx, cy, photo=photo, swap_rb=swap_rb, step=step)
    h, w = np.asarray(depth).shape
    hs, ws = grid(h, w, step)
    X, Y, Z = rec["x"], rec["y"], rec["z"]
    cos_a, sin_a, cos_e, sin_e = (np.float64(t) for t in view_trig(elev_deg, azim_deg))
    row = np.zeros(VIEW_ROW, np.float64)
    with np.errstate(all="ignore"):
        valid = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z > 0)

        def rotate(c):
            dx, dy, dz = X.astype(np.float64) - c[0], Y.astype(np.float64) - c[1], Z.astype(np.float64) - c[2]
            x1 = cos_a * dx + sin_a * dz
            z1 = (-sin_a) * dx + cos_a * dz
            y2 = cos_e * dy - sin_e * z1
            z2 = sin_e * dy + cos_e * z1
            return x1, y2, z2

        if view is not None:
            view = np.asarray(view, dtype=np.float64).reshape(VIEW_ROW)
            c, span, scale = view[V_C0:V_C2 + 1].copy(), view[V_SPAN], view[V_SCALE]
        elif not valid.any():
            c, span = np.zeros(3, np.float64), np.float64(1.0)
            scale = np.float64(0.46 * min(out_h, out_w)) / span
        else:
            planes = np.where(valid[None], np.stack([X, Y, Z]), np.float32(np.nan)).reshape(3, hs, ws)
            q = quantiles_np(planes, (50.0,))
            assert q[0][Q_NVALID] == valid.sum()
            c = q[:, Q_Q0].copy()
            x1, y2, _ = rotate(c)
            pool = np.where(valid[None], np.stack([np.abs(x1), np.abs(y2)]).astype(np.float32), np.float32(np.nan))
            span = quantiles_np(pool.reshape(2, hs, ws), (99.0,), pooled=True)[0][Q_Q0]
            if not np.isfinite(span) or span <= 0:
                span = np.float64(1.0)
            scale = np.float64(0.46 * min(out_h, out_w)) / span
        x1, y2, z2 = rotate(c)
        u = np.rint(x1 * scale + out_w / 2.0)
        v = np.rint(y2 * scale + out_h / 2.0)
        inside = valid & (u >= 0) & (u < out_w) & (v >= 0) & (v < out_h)
        idx = np.flatnonzero(inside)
        pixel = v[idx].astype(np.int64) * out_w + u[idx].astype(np.int64)
        packed = (_order_key(z2[idx].astype(np.float32)).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    zbuf = np.full(out_h * out_w, empty, np.uint64)
    np.minimum.at(zbuf, pixel, packed)
    hit = zbuf != empty
    win = (zbuf[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    pic = np.empty((out_h * out_w, 3), np.uint8)
    pic[:] = np.asarray(bg, np.uint8)
    if photo is not None:
        pic[hit] = np.stack([rec["red"][win], rec["green"][win], rec["blue"][win]], axis=-1)
    else:
        pic[hit] = VIEW_GREY
    row[V_NVALID], row[V_C0:V_C2 + 1], row[V_SPAN], row[V_SCALE], row[V_INSIDE] = valid.sum(), c, span, scale, idx.size
    return pic.reshape(out_h, out_w, 3), row


def cloud_view_ws_bytes(batch: int, h: int, w: int, step: int, out_h: int, out_w: int) -> int:
    """Device scratch mde_op_cloud_view needs (mde_op_cloud_view_ws_bytes); 0: refused."""
    return int(_lib.lib().mde_op_cloud_view_ws_bytes(int(batch), int(h), int(w), int(step), int(out_h), int(out_w)))


def cloud_view(d_depth: int, batch: int, h: int, w: int, step: int, d_photo: int, pitch: int, swap_rb: bool,
               d_f_px: int, fx: float, fy: float, cx: float, cy: float, trig, d_view_in: int, bg, out_swap_rb: bool,
               d_out: int, out_h: int, out_w: int, d_view_out: int, d_ws: int, ws_nbytes: int, stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream` (mde_op_cloud_view); trig =
    (cos_a, sin_a, cos_e, sin_e), e.g. view_trig(elev_deg, azim_deg)."""
    _lib.call("mde_op_cloud_view", C.c_void_p(int(d_depth or 0)), int(batch), int(h), int(w), int(step),
              C.c_void_p(int(d_photo or 0)), int(pitch), int(bool(swap_rb)), C.c_void_p(int(d_f_px or 0)),
              float(fx), float(fy), float(cx), float(cy), *(float(t) for t in trig), C.c_void_p(int(d_view_in or 0)),
              (C.c_int * 3)(*(int(c) for c in bg)), int(bool(out_swap_rb)), C.c_void_p(int(d_out or 0)), int(out_h),
              int(out_w), C.c_void_p(int(d_view_out or 0)), C.c_void_p(int(d_ws or 0)), int(ws_nbytes),
              C.c_void_p(int(stream or 0)))


class DeviceCloudView(_CloudOp):
    """Owns the pictures uint8 [batch][out_h][out_w][3] and the view rows
    float64 [batch][8] (device + pinned host) and the scratch of
    mde_op_cloud_view for `batch` depth maps [h, w], with or without colour,
    sampling every `step`-th pixel.

    enqueue(d_depth, stream, ...) only enqueues (capturable) -- with `view=`,
    a host array of view rows, one small H2D copy from pinned memory comes
    first; download(stream) brings the pictures and the view rows back and
    synchronizes; result() is the [batch, out_h, out_w, 3] pictures and view()
    the [batch, 8] rows, valid until the next download; run() = enqueue,
    download, result."""

    _OP = "mde_op_cloud_view"
    _BUFFERS = ("pictures", "views", "view_in")

    def __init__(self, batch: int, h: int, w: int, out_hw=VIEW_SIZE, colour: bool = True, step: int = 1):
        super().__init__(batch, h, w, colour, step)
        self.out_h, self.out_w = int(out_hw[0]), int(out_hw[1])
        rows = (self.batch * VIEW_ROW, np.dtype(np.float64))
        self._allocate(cloud_view_ws_bytes(self.batch, self.h, self.w, self.step, self.out_h, self.out_w),
                       f"batch {batch}, {h}x{w}, step {step}, picture {self.out_h}x{self.out_w}",
                       pictures=(self.batch * self.out_h * self.out_w * 3, np.uint8), views=rows, view_in=rows)

    def enqueue(self, d_depth: int, stream: int, d_photo: int = 0, pitch: int = 0, swap_rb: bool = False,
                d_f_px: int = 0, fx: Optional[float] = None, fy: Optional[float] = None,
                cx: Optional[float] = None, cy: Optional[float] = None, elev_deg: float = VIEW_ANGLES[0],
                azim_deg: float = VIEW_ANGLES[1], view=None, d_view: int = 0, bg=VIEW_BG,
                out_swap_rb: bool = False) -> None:
        """The kernels on `stream`.  Focal lengths and cx, cy as for
        DevicePointCloud.enqueue.  `view`: host view rows [batch, 8] (or one
        row for all) whose centre and scale fix the camera; `d_view`: the same
        already in device memory -- `self.views.device` keeps the camera of
        the previous enqueue."""
        source = self._source(d_depth, d_photo, pitch, swap_rb, d_f_px, fx, fy, cx, cy)
        if view is not None and d_view:
            raise ValueError("DeviceCloudView.enqueue takes view or d_view, not both")
        if view is not None:
            rows = np.broadcast_to(np.asarray(view, dtype=np.float64).reshape(-1, VIEW_ROW), (self.batch, VIEW_ROW))
            self.view_in.host = np.ascontiguousarray(rows).reshape(-1)
            _lib.call("mde_rt_memcpy_htod_async", C.c_void_p(self.view_in.device),
                      self.view_in.host.ctypes.data_as(C.c_void_p), self.view_in.nbytes, C.c_void_p(int(stream or 0)))
            d_view = self.view_in.device
        cloud_view(*source, view_trig(elev_deg, azim_deg), d_view, bg, out_swap_rb, self.pictures.device, self.out_h,
                   self.out_w, self.views.device, self._ws, self._ws_bytes, stream)

    def download(self, stream: int, sync: bool = True) -> None:
        """The pictures and the view rows; synchronizes `stream` unless `sync`
        is off (the caller's own synchronisation then makes them valid)."""
        self._live()
        s = C.c_void_p(int(stream or 0))
        for m in (self.pictures, self.views):
            _lib.call("mde_rt_memcpy_dtoh_async", m.host.ctypes.data_as(C.c_void_p), C.c_void_p(m.device), m.nbytes, s)
        if sync:
            stream_synchronize(stream)

    def result(self) -> np.ndarray:
        """uint8 [batch, out_h, out_w, 3]; valid after download()."""
        self._live()
        return self.pictures.host.reshape(self.batch, self.out_h, self.out_w, 3)

    def view(self) -> np.ndarray:
        """float64 [batch, 8] view rows; valid after download()."""
        self._live()
        return self.views.host.reshape(self.batch, VIEW_ROW)


def device_cloud_view(path, d_depth: int, h: int, w: int, stream: int, size=VIEW_SIZE, elev_deg: float = VIEW_ANGLES[0],
                      azim_deg: float = VIEW_ANGLES[1], step: int = 1, img_bgr: Optional[np.ndarray] = None,
                      d_f_px: int = 0, f_px: Optional[float] = None, d_photo: int = 0):
    """What the model drivers' --cloud-view does: DeviceCloudView on one device
    depth map [h][w] at `d_depth`, camera and colours as for `device_ply`; the
    BGR picture goes to `path` through visualize.save_image.  Returns (ms of
    the kernels + D2H between two hipEvents on `stream`, the view row)."""
    from .visualize import save_image
    with _device_photo(img_bgr, d_photo, h, w, stream) as d_photo, \
            DeviceCloudView(1, h, w, size, colour=bool(d_photo), step=step) as cv:
        ms = _timed(cv, d_depth, stream, d_photo, d_f_px, f_px, elev_deg=elev_deg, azim_deg=azim_deg,
                    out_swap_rb=True)
        save_image(str(path), cv.result()[0])
        return ms, cv.view()[0].copy()


def add_cloud_view_arguments(ap, picture: bool = True) -> None:
    """The drivers' --cloud-view options; `picture` off: only its size, angles
    and step (models/depth_pro/stream.py names its own output)."""
    if picture:
        ap.add_argument("--cloud-view", default="", metavar="PATH",
                        help="write a z-buffered orthographic picture of the point cloud (colours from --image)")
    ap.add_argument("--cloud-view-size", type=int, nargs=2, default=list(VIEW_SIZE), metavar=("H", "W"))
    ap.add_argument("--cloud-view-angles", type=float, nargs=2, default=list(VIEW_ANGLES), metavar=("ELEV", "AZIM"),
                    help="degrees; the default looks from above-left")
    ap.add_argument("--cloud-view-step", type=int, default=1, help="draw every N-th pixel on both axes")


def check_cloud_view_arguments(a) -> None:
    """--cloud-view's conditions that need no engine."""
    if not a.cloud_view:
        return
    if min(a.cloud_view_size) < 1:
        raise SystemExit("--cloud-view-size must be positive")
    if a.cloud_view_step < 1:
        raise SystemExit("--cloud-view-step must be positive")
    if not all(np.isfinite(v) for v in a.cloud_view_angles):
        raise SystemExit("--cloud-view-angles must be finite")


def driver_cloud_view(a, d_depth: int, hw, stream: int, img_bgr=None, d_f_px: int = 0, f_px=None, d_photo: int = 0):
    """The drivers' --cloud-view: the picture of the device map [hw] at
    `d_depth` and its `[MDET] cloud view ...` line.  Returns the view row."""
    ms, row = device_cloud_view(a.cloud_view, d_depth, hw[0], hw[1], stream, size=a.cloud_view_size,
                                elev_deg=a.cloud_view_angles[0], azim_deg=a.cloud_view_angles[1],
                                step=a.cloud_view_step, img_bgr=img_bgr, d_f_px=d_f_px, f_px=f_px, d_photo=d_photo)
    print(f"[MDET] cloud view (device, kernels + D2H, hipEvents) {hw[0]}x{hw[1]} step {a.cloud_view_step} -> "
          f"{a.cloud_view_size[0]}x{a.cloud_view_size[1]} {a.cloud_view} : {ms:0.3f} ms, {int(row[V_NVALID])} valid "
          f"points, {int(row[V_INSIDE])} inside the picture")
    return row


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


# ---- meshes: mde_op_depth_mesh (csrc/depth_mesh.hip) ---------------------------------------------------
# The reference's models/metric_anything/demo_pointcloud.py:142-149 -- depth edges dropped, a triangle
# mesh over what is left, no unreferenced vertices.  mesh_np restates the include/mde.h contract.

FACE_DTYPE = np.dtype([("n", "u1"), ("i0", "<i4"), ("i1", "<i4"), ("i2", "<i4")])  # 13 bytes, a PLY list entry
# the flag byte of a sample (csrc/depth_mesh.hip writes the same byte into its scratch)
F_VALID, F_EDGE, F_CLEAN, F_QUAD, F_DIAG_BD, F_VERTEX = 1, 2, 4, 8, 16, 32
EDGE_RTOL = 0.1          # demo_pointcloud.py:143


def _max3x3(a: np.ndarray) -> np.ndarray:
    """Maximum over the 3 x 3 neighbourhood clipped to the array (-inf outside)."""
    p = np.full((a.shape[0] + 2, a.shape[1] + 2), -np.inf, a.dtype)
    p[1:-1, 1:-1] = a
    out = a.copy()
    for di in range(3):
        for dj in range(3):
            np.maximum(out, p[di:di + a.shape[0], dj:dj + a.shape[1]], out=out)
    return out


def mesh_np(depth, fx, fy, cx, cy, photo=None, swap_rb=False, step=1, z_lo=1e-4, z_hi=1e4, edge_rtol=EDGE_RTOL,
            edge_atol=0.0, faces=True):
    """The include/mde.h contract of mde_op_depth_mesh for one image, in numpy
    float32 with one rounding per operation, on the sampled grid of
    `unproject_np`:

        valid = z == z and z_lo <= z <= z_hi
        diff  = zmax - zmin over the valid samples of the clipped 3 x 3 window
        edge  = valid and ((atol > 0 and diff > atol) or (rtol > 0 and diff / z > rtol))
        clean = valid and not edge
        quad (i, j) kept iff a = (i, j), b = (i, j + 1), c = (i + 1, j + 1), d = (i + 1, j) are clean;
        |za - zc| <= |zb - zd|: triangles (a, d, c), (a, c, b), else (a, d, b), (b, d, c)
        vertex = one of its quads is kept (faces) / clean (not faces)

    Returns (vertex records, 1-D `vertex_dtype`, row-major; face records, 1-D
    FACE_DTYPE, row-major by quad, empty without `faces`; flags uint8 [hs, ws],
    the F_* bits)."""
    f32 = np.float32
    zfull = np.asarray(depth, dtype=np.float32)
    rtol, atol = f32(edge_rtol), f32(edge_atol)
    if not (rtol >= 0 and atol >= 0):
        raise ValueError("edge_rtol and edge_atol must not be negative or NaN")
    rec = unproject_np(zfull, fx, fy, cx, cy, photo=photo, swap_rb=swap_rb, step=step)
    z = zfull[::step, ::step]
    hs, ws = z.shape
    with np.errstate(all="ignore"):
        valid = (z == z) & (z >= f32(z_lo)) & (z <= f32(z_hi))
        zmax = _max3x3(np.where(valid, z, f32(-np.inf)))
        zmin = -_max3x3(np.where(valid, -z, f32(-np.inf)))
        diff = zmax - zmin
        ratio = diff / z
        assert diff.dtype == ratio.dtype == np.float32
        edge = valid & (((atol > 0) & (diff > atol)) | ((rtol > 0) & (ratio > rtol)))
        clean = valid & ~edge
        quad = np.zeros((hs, ws), bool)
        bd = np.zeros((hs, ws), bool)
        if hs > 1 and ws > 1:
            quad[:-1, :-1] = clean[:-1, :-1] & clean[:-1, 1:] & clean[1:, 1:] & clean[1:, :-1]
            bd[:-1, :-1] = quad[:-1, :-1] & ~(np.abs(z[:-1, :-1] - z[1:, 1:]) <= np.abs(z[:-1, 1:] - z[1:, :-1]))
    if faces:
        vertex = quad.copy()
        vertex[:, 1:] |= quad[:, :-1]
        vertex[1:, :] |= quad[:-1, :]
        vertex[1:, 1:] |= quad[:-1, :-1]
    else:
        vertex = clean
    flags = (valid * F_VALID + edge * F_EDGE + clean * F_CLEAN + quad * F_QUAD + bd * F_DIAG_BD
             + vertex * F_VERTEX).astype(np.uint8)
    index = (np.cumsum(vertex.reshape(-1), dtype=np.int64) - 1).reshape(hs, ws)
    tri = np.zeros((0, 2), FACE_DTYPE)
    if faces and quad.any():
        qi, qj = np.nonzero(quad)  # row-major
        a, b, c, d = index[qi, qj], index[qi, qj + 1], index[qi + 1, qj + 1], index[qi + 1, qj]
        split = bd[qi, qj]
        tri = np.empty((qi.size, 2), FACE_DTYPE)
        tri["n"] = 3
        tri["i0"][:, 0], tri["i1"][:, 0], tri["i2"][:, 0] = a, d, np.where(split, b, c)
        tri["i0"][:, 1], tri["i1"][:, 1], tri["i2"][:, 1] = np.where(split, b, a), np.where(split, d, c), \
            np.where(split, c, b)
    return rec[vertex.reshape(-1)], tri.reshape(-1), flags


def mesh_ws_bytes(batch: int, h: int, w: int, step: int = 1) -> int:
    """Device scratch mde_op_depth_mesh needs (mde_op_depth_mesh_ws_bytes); 0: refused."""
    return int(_lib.lib().mde_op_depth_mesh_ws_bytes(int(batch), int(h), int(w), int(step)))


def depth_mesh(d_depth: int, batch: int, h: int, w: int, step: int, d_photo: int, pitch: int, swap_rb: bool,
               d_f_px: int, fx: float, fy: float, cx: float, cy: float, z_lo: float, z_hi: float, edge_rtol: float,
               edge_atol: float, faces: bool, d_vertices: int, vertices_bytes: int, d_vertex_counts: int, d_faces: int,
               faces_bytes: int, d_face_counts: int, d_ws: int, ws_nbytes: int, stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream` (mde_op_depth_mesh)."""
    _lib.call("mde_op_depth_mesh", C.c_void_p(int(d_depth)), int(batch), int(h), int(w), int(step),
              C.c_void_p(int(d_photo or 0)), int(pitch), int(bool(swap_rb)), C.c_void_p(int(d_f_px or 0)),
              float(fx), float(fy), float(cx), float(cy), float(z_lo), float(z_hi), float(edge_rtol),
              float(edge_atol), int(bool(faces)), C.c_void_p(int(d_vertices)), int(vertices_bytes),
              C.c_void_p(int(d_vertex_counts)), C.c_void_p(int(d_faces or 0)), int(faces_bytes),
              C.c_void_p(int(d_face_counts or 0)), C.c_void_p(int(d_ws or 0)), int(ws_nbytes),
              C.c_void_p(int(stream or 0)))


class DeviceMesh(_CloudOp):
    """Owns the vertex and face records and the two counts (device + pinned
    host) and the scratch of mde_op_depth_mesh for `batch` depth maps [h, w],
    with or without colour, sampling every `step`-th pixel; `faces` off: the
    edge-filtered cloud only, no face buffers.

    enqueue(d_depth, stream, ...) only enqueues the kernels (capturable);
    download(stream) brings both counts back, synchronizes once, then copies
    only the counted bytes of each image's regions and synchronizes again;
    result() is one (`vertex_dtype` view, FACE_DTYPE view) pair per image,
    valid until the next download; run() = enqueue, download, result."""

    _OP = "mde_op_depth_mesh"
    _BUFFERS = ("vertices", "face_records", "counts")  # counts [2][batch]: vertices, triangles

    def __init__(self, batch: int, h: int, w: int, colour: bool, step: int = 1, faces: bool = True):
        super().__init__(batch, h, w, colour, step)
        self.faces = bool(faces)
        self.hs, self.ws = grid(self.h, self.w, self.step)
        self.dtype = vertex_dtype(self.colour)
        self.region = self.hs * self.ws * self.dtype.itemsize                       # vertex bytes per image
        self.face_region = 2 * (self.hs - 1) * (self.ws - 1) * FACE_DTYPE.itemsize  # face bytes per image
        buffers = dict(vertices=(self.batch * self.region, np.uint8))
        if self.faces:  # at least one byte: the op wants a pointer even where no quad exists
            buffers["face_records"] = (max(self.batch * self.face_region, 1), np.uint8)
        self._allocate(mesh_ws_bytes(self.batch, self.h, self.w, self.step), f"batch {batch}, {h}x{w}, step {step}",
                       **buffers, counts=(2 * self.batch, np.dtype(np.int32)))

    def enqueue(self, d_depth: int, stream: int, d_photo: int = 0, pitch: int = 0, swap_rb: bool = False,
                d_f_px: int = 0, fx: Optional[float] = None, fy: Optional[float] = None,
                cx: Optional[float] = None, cy: Optional[float] = None, z_lo: float = 1e-4, z_hi: float = 1e4,
                edge_rtol: float = EDGE_RTOL, edge_atol: float = 0.0) -> None:
        """The kernels on `stream`, nothing else.  Focal lengths and cx, cy as
        for DevicePointCloud.enqueue."""
        depth_mesh(*self._source(d_depth, d_photo, pitch, swap_rb, d_f_px, fx, fy, cx, cy), z_lo, z_hi, edge_rtol,
                   edge_atol, self.faces, self.vertices.device, self.batch * self.region, self.counts.device,
                   self.face_records.device if self.faces else 0, self.batch * self.face_region if self.faces else 0,
                   self.counts.device + 4 * self.batch if self.faces else 0, self._ws, self._ws_bytes, stream)

    def download(self, stream: int) -> None:
        """Both counts first, then only the counted bytes; synchronizes `stream` twice."""
        self._live()
        s = C.c_void_p(int(stream or 0))
        if not self.faces:
            self.counts.host[self.batch:] = 0
        _lib.call("mde_rt_memcpy_dtoh_async", self.counts.host.ctypes.data_as(C.c_void_p),
                  C.c_void_p(self.counts.device), self.counts.nbytes if self.faces else 4 * self.batch, s)
        stream_synchronize(stream)
        for b in range(self.batch):
            for mem, region, n in ((self.vertices, self.region, int(self.counts.host[b]) * self.dtype.itemsize),
                                   (self.face_records, self.face_region,
                                    int(self.counts.host[self.batch + b]) * FACE_DTYPE.itemsize)):
                if n:
                    _lib.call("mde_rt_memcpy_dtoh_async", C.c_void_p(mem.host.ctypes.data + b * region),
                              C.c_void_p(mem.device + b * region), n, s)
        stream_synchronize(stream)

    def result(self):
        """One (vertices, faces) pair of views per image; valid after download()."""
        self._live()
        out = []
        for b in range(self.batch):
            nv, nf = int(self.counts.host[b]), int(self.counts.host[self.batch + b])
            v = self.vertices.host[b * self.region:b * self.region + nv * self.dtype.itemsize].view(self.dtype)
            f = (self.face_records.host[b * self.face_region:b * self.face_region + nf * FACE_DTYPE.itemsize]
                 .view(FACE_DTYPE) if self.faces else np.zeros(0, FACE_DTYPE))
            out.append((v, f))
        return out


def mesh_header(vertex_count: int, face_count: int, colour: bool) -> bytes:
    lines = ply_header(vertex_count, colour).decode("ascii").split("\n")[:-2]  # without end_header
    lines += [f"element face {int(face_count)}", "property list uchar int vertex_indices"]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_ply_mesh(path, vertices: np.ndarray, faces: np.ndarray) -> None:
    """The ASCII header with `element vertex` and `element face`, then the
    bytes of `vertices` (1-D `vertex_dtype`) and of `faces` (1-D FACE_DTYPE) as
    they are -- as they came off the card."""
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    colour = vertices.dtype == vertex_dtype(True)
    if vertices.ndim != 1 or not (colour or vertices.dtype == vertex_dtype(False)):
        raise ValueError(f"write_ply_mesh wants a 1-D vertex_dtype array, got {vertices.dtype} {vertices.shape}")
    if faces.ndim != 1 or faces.dtype != FACE_DTYPE:
        raise ValueError(f"write_ply_mesh wants a 1-D FACE_DTYPE array, got {faces.dtype} {faces.shape}")
    with open(path, "wb") as f:
        f.write(mesh_header(vertices.shape[0], faces.shape[0], colour))
        f.write(np.ascontiguousarray(vertices).tobytes())
        f.write(np.ascontiguousarray(faces).tobytes())


def read_ply_mesh(path):
    """Read a file of exactly write_ply_mesh's form back: (vertices, faces)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: no PLY header")
    body = end + len(b"end_header\n")
    counts = {}
    for line in data[:body].decode("ascii", errors="replace").split("\n"):
        part = line.split(" ")
        if len(part) == 3 and part[0] == "element" and part[2].isdigit():
            counts[part[1]] = int(part[2])
    if set(counts) != {"vertex", "face"}:
        raise ValueError(f"{path}: not a vertex + face PLY header")
    for colour in (True, False):
        if data[:body] == mesh_header(counts["vertex"], counts["face"], colour):
            dt = vertex_dtype(colour)
            nv, nf = counts["vertex"] * dt.itemsize, counts["face"] * FACE_DTYPE.itemsize
            if len(data) - body != nv + nf:
                raise ValueError(f"{path}: {len(data) - body} body bytes, the header promises {nv + nf}")
            faces = np.frombuffer(data, dtype=FACE_DTYPE, count=counts["face"], offset=body + nv).copy()
            if (faces["n"] != 3).any():
                raise ValueError(f"{path}: a face that is not a triangle")
            return np.frombuffer(data, dtype=dt, count=counts["vertex"], offset=body).copy(), faces
    raise ValueError(f"{path}: the header is not one write_ply_mesh writes")


def device_mesh(path, d_depth: int, h: int, w: int, stream: int, step: int = 1, img_bgr: Optional[np.ndarray] = None,
                d_f_px: int = 0, f_px: Optional[float] = None, z_lo: float = 1e-4, z_hi: float = 1e4,
                edge_rtol: float = EDGE_RTOL, edge_atol: float = 0.0, faces: bool = True, d_photo: int = 0):
    """What the model drivers' --mesh does (and, with `faces` off, --ply with
    --ply-edge-rtol): DeviceMesh on one device depth map [h][w] at `d_depth`,
    camera and colours as for `device_ply`, written to `path` (a mesh PLY, or
    with `faces` off write_ply's vertex-only file).  Returns (ms of the kernels
    + D2H between two hipEvents on `stream`, vertices, triangles)."""
    with _device_photo(img_bgr, d_photo, h, w, stream) as d_photo, \
            DeviceMesh(1, h, w, colour=bool(d_photo), step=step, faces=faces) as mesh:
        ms = _timed(mesh, d_depth, stream, d_photo, d_f_px, f_px, z_lo=z_lo, z_hi=z_hi, edge_rtol=edge_rtol,
                    edge_atol=edge_atol)
        vertices, tri = mesh.result()[0]
        if faces:
            write_ply_mesh(path, vertices, tri)
        else:
            write_ply(path, vertices)
        return ms, int(vertices.shape[0]), int(tri.shape[0])


def add_mesh_arguments(ap) -> None:
    """The drivers' --mesh options and --ply's edge filter."""
    ap.add_argument("--mesh", default="", metavar="PATH",
                    help="write a triangle mesh (binary PLY; colours from --image) of the metric depth without its "
                         "depth edges")
    ap.add_argument("--mesh-step", type=int, default=1, help="with --mesh: keep every N-th pixel on both axes")
    ap.add_argument("--edge-rtol", type=float, default=EDGE_RTOL,
                    help="with --mesh: a sample whose 3x3 depth spread / depth exceeds this is an edge (0: off)")
    ap.add_argument("--edge-atol", type=float, default=0.0,
                    help="with --mesh: a sample whose 3x3 depth spread exceeds this is an edge (0: off)")
    ap.add_argument("--ply-edge-rtol", type=float, default=None, metavar="R",
                    help="with --ply: drop depth edges (flying pixels) from the cloud, as --edge-rtol does for --mesh")


def check_mesh_arguments(a) -> None:
    """The conditions of --mesh and --ply-edge-rtol that need no engine."""
    if a.mesh:
        if a.mesh_step < 1:
            raise SystemExit("--mesh-step must be positive")
        if not (a.edge_rtol >= 0 and a.edge_atol >= 0):
            raise SystemExit("--edge-rtol and --edge-atol must not be negative")
    if a.ply_edge_rtol is not None:
        if not a.ply:
            raise SystemExit("--ply-edge-rtol needs --ply")
        if not a.ply_edge_rtol >= 0:
            raise SystemExit("--ply-edge-rtol must not be negative")


def driver_mesh(a, d_depth: int, hw, stream: int, img_bgr=None, d_f_px: int = 0, f_px=None, z_lo=1e-4, z_hi=1e4,
                d_photo: int = 0):
    """The drivers' --mesh: the mesh of the device map [hw] at `d_depth` and
    its `[MDET] mesh ...` line.  Returns (vertices, triangles)."""
    ms, nv, nf = device_mesh(a.mesh, d_depth, hw[0], hw[1], stream, step=a.mesh_step, img_bgr=img_bgr, d_f_px=d_f_px,
                             f_px=f_px, z_lo=z_lo, z_hi=z_hi, edge_rtol=a.edge_rtol, edge_atol=a.edge_atol,
                             d_photo=d_photo)
    print(f"[MDET] mesh (device, kernels + D2H, hipEvents) {hw[0]}x{hw[1]} step {a.mesh_step} rtol {a.edge_rtol:g} "
          f"atol {a.edge_atol:g} -> {a.mesh} : {ms:0.3f} ms, {nv} vertices, {nf} triangles")
    return nv, nf


def driver_ply(a, d_depth: int, hw, stream: int, img_bgr=None, d_f_px: int = 0, f_px=None, z_lo=1e-4, z_hi=1e4,
               d_photo: int = 0):
    """The drivers' --ply: `device_ply`, or with --ply-edge-rtol the
    edge-filtered cloud of `device_mesh`, and its `[MDET] point cloud ...`
    line.  Returns (ms, points)."""
    kw = dict(step=a.ply_step, img_bgr=img_bgr, d_f_px=d_f_px, f_px=f_px, z_lo=z_lo, z_hi=z_hi, d_photo=d_photo)
    if a.ply_edge_rtol is None:
        ms, n = device_ply(a.ply, d_depth, hw[0], hw[1], stream, **kw)
    else:
        ms, n = device_mesh(a.ply, d_depth, hw[0], hw[1], stream, edge_rtol=a.ply_edge_rtol, faces=False, **kw)[:2]
    print(f"[MDET] point cloud (device, kernels + D2H, hipEvents) {hw[0]}x{hw[1]} step {a.ply_step} -> {a.ply} : "
          f"{ms:0.3f} ms, {n} points")
    return ms, n


def _asked(a):
    """Those of --ply, --mesh and --cloud-view that the parsed arguments ask for, in the order they run."""
    return [opt for opt, path in (("--ply", a.ply), ("--mesh", a.mesh), ("--cloud-view", a.cloud_view)) if path]


def add_cloud_arguments(ap, needs_f_px: bool = False) -> None:
    """The drivers' cloud outputs: --ply, --mesh and --cloud-view with their
    options (the module's docstring describes them)."""
    ap.add_argument("--ply", default="", metavar="PATH",
                    help="write the point cloud (binary PLY; colours from --image) of the metric depth"
                         + ("; needs --f-px" if needs_f_px else ""))
    ap.add_argument("--ply-step", type=int, default=1, help="with --ply: keep every N-th pixel on both axes")
    add_mesh_arguments(ap)
    add_cloud_view_arguments(ap)


def check_cloud_arguments(a, needs_f_px: bool = False, metric: bool = True, no_device_map: str = "") -> None:
    """What can be refused without a device, option by option: first whether
    this driver can serve it -- `needs_f_px`: the model predicts no focal
    length, so --f-px is required; `metric` off: a relative model (a driver
    asks again with what the opened engine says); `no_device_map`: why there is
    no device depth map to run on, if there is none -- then the option's own
    values."""
    def servable(opt):
        if needs_f_px and (a.f_px is None or not a.f_px > 0):
            raise SystemExit(f"{opt} needs --f-px (a positive focal length in pixels): this model predicts none")
        if not metric:
            raise SystemExit(f"{opt} needs a metric model: relative depth is not turned into metres")
        if no_device_map:
            raise SystemExit(f"{opt} runs on the device post-process's depth map: {no_device_map}")

    if a.ply:
        servable("--ply")
        if a.ply_step < 1:
            raise SystemExit("--ply-step must be positive")
    if a.mesh:
        servable("--mesh")
    check_mesh_arguments(a)
    if a.cloud_view:
        servable("--cloud-view")
    check_cloud_view_arguments(a)


def check_photo_size(a, img_bgr, hw) -> None:
    """The colours come from the --image photo: the map must have its size."""
    asked = _asked(a)
    if asked and img_bgr is not None and tuple(hw) != img_bgr.shape[:2]:
        raise SystemExit(f"{asked[0]} takes its colours from the --image photo: --src-hw must be the photo's size")


def run_cloud_outputs(a, d_depth: int, hw, stream: int, img_bgr=None, d_f_px: int = 0, f_px=None, z_lo=1e-4,
                      z_hi=1e4) -> None:
    """The drivers' --ply, --mesh and --cloud-view, in this order, on the
    device map [hw] at `d_depth`, with the given `f_px` or else the device
    focal length `d_f_px`; `z_lo`, `z_hi`: the driver's clamp.  The photo is
    uploaded once for all of them."""
    if not _asked(a):
        return
    with _device_photo(img_bgr, 0, hw[0], hw[1], stream) as d_photo:
        kw = dict(d_f_px=d_f_px, f_px=f_px, d_photo=d_photo)
        if a.ply:
            driver_ply(a, d_depth, hw, stream, z_lo=z_lo, z_hi=z_hi, **kw)
        if a.mesh:
            driver_mesh(a, d_depth, hw, stream, z_lo=z_lo, z_hi=z_hi, **kw)
        if a.cloud_view:
            driver_cloud_view(a, d_depth, hw, stream, **kw)


__all__ = ["vertex_dtype", "grid", "unproject_np", "ws_bytes", "point_cloud", "DevicePointCloud", "device_ply", "ply_header",
           "write_ply", "read_ply", "view_trig", "render_np", "cloud_view_ws_bytes", "cloud_view", "DeviceCloudView",
           "device_cloud_view", "add_cloud_view_arguments", "check_cloud_view_arguments", "driver_cloud_view",
           "FACE_DTYPE", "mesh_np", "mesh_ws_bytes", "depth_mesh", "DeviceMesh", "mesh_header", "write_ply_mesh",
           "read_ply_mesh", "device_mesh", "add_mesh_arguments", "check_mesh_arguments", "driver_mesh", "driver_ply",
           "add_cloud_arguments", "check_cloud_arguments", "check_photo_size", "run_cloud_outputs"]
