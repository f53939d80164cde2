"""On-device depth post-process: the reference's
`models/depth_anything_v2/onnx2trt.py:111-117` -- bilinear
(align_corners=True) resize of the [B,h,w] depth map back to the source
image size, then clamp to [1e-3, 1e3] -- as one HIP kernel
(`mde_op_depth_postprocess`), so the D2H copy carries the final map.

Depth Pro's post-process (`models/depth_pro/onnx2trt.py:118-134`: focal length
from the predicted FOV, rescale, bilinear align_corners=False, 1 / clamp) the
same way (`mde_op_dp_postprocess`, `DepthProDevicePostprocess`), next to its
numpy restatement and the reference's torch statement.
"""

from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .common_runtime import HostDeviceMem, stream_synchronize


def resize_clamp(d_in: int, batch: int, ih: int, iw: int, d_out: int, oh: int, ow: int,
                 lo: float = 1e-3, hi: float = 1e3, stream: int = 0) -> None:
    """Device pointers in/out (fp32), enqueued on `stream`."""
    _lib.call("mde_op_depth_postprocess", C.c_void_p(int(d_in)), int(batch), int(ih), int(iw),
              C.c_void_p(int(d_out)), int(oh), int(ow), float(lo), float(hi), C.c_void_p(int(stream or 0)))


class DevicePostprocess:
    """Owns the resized map (device + pinned host); `run(d_depth, stream)`
    returns a host view [batch, oh, ow] that the next call overwrites."""

    def __init__(self, batch: int, ih: int, iw: int, oh: int, ow: int, lo: float = 1e-3, hi: float = 1e3):
        self.shape = (int(batch), int(oh), int(ow))
        self.src = (int(ih), int(iw))
        self.lo, self.hi = float(lo), float(hi)
        self.mem: Optional[HostDeviceMem] = HostDeviceMem(batch * oh * ow, np.dtype(np.float32))

    def run(self, d_depth: int, stream: int) -> np.ndarray:
        if self.mem is None:
            raise RuntimeError("DevicePostprocess already freed")
        b, oh, ow = self.shape
        resize_clamp(d_depth, b, self.src[0], self.src[1], self.mem.device, oh, ow, self.lo, self.hi, stream)
        host = self.mem.host
        _lib.call("mde_rt_memcpy_dtoh_async", host.ctypes.data_as(C.c_void_p), C.c_void_p(self.mem.device),
                  host.nbytes, C.c_void_p(int(stream or 0)))
        stream_synchronize(stream)
        return self.mem.host.reshape(self.shape)

    def free(self) -> None:
        if self.mem is not None:
            self.mem.free()
            self.mem = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def depth_pro_postprocess_np(inv: np.ndarray, fov_deg, src_hw, f_px=None):
    """The include/mde.h contract of mde_op_dp_postprocess in numpy float32,
    one rounding per operation in the contract's order (the kernel is held to
    it bit for bit, except np.tan against the device's tanf when the focal
    length comes from `fov_deg`).  inv: [ih, iw] -> (depth [H, W], f_px
    float), or [B, ih, iw] / [B, 1, ih, iw] -> (depth [B, H, W], f_px
    float32 [B]); fov_deg: one angle per image, ignored when f_px is given.
    A NaN in the blended map stays NaN (np.maximum / np.minimum propagate it,
    as torch.clamp does and as the kernel's clamp is written to)."""
    from .preprocess import resize_bilinear_f32
    f32 = np.float32
    inv = np.asarray(inv, dtype=np.float32)
    single = inv.ndim == 2
    maps = inv.reshape(-1, *inv.shape[-2:])
    H, W = int(src_hw[0]), int(src_hw[1])
    if f_px is None:
        fov = np.asarray(fov_deg, dtype=np.float32).reshape(-1)[:maps.shape[0]]
        if fov.shape[0] != maps.shape[0]:
            raise ValueError(f"{maps.shape[0]} maps but {fov.shape[0]} fov_deg values")
        f = (f32(0.5) * f32(W)) / np.tan(f32(0.5) * (fov * f32(np.pi / 180)))
    else:
        if not float(f_px) > 0:
            raise ValueError("f_px must be positive")
        f = np.full(maps.shape[0], f_px, dtype=np.float32)
    k = f32(W) / f
    m = resize_bilinear_f32(maps * k[:, None, None], H, W)
    depth = f32(1) / np.minimum(np.maximum(m, f32(1e-4)), f32(1e4))
    assert depth.dtype == f.dtype == np.float32
    return (depth[0], float(f[0])) if single else (depth, f)


def dp_postprocess(d_inv: int, batch: int, ih: int, iw: int, d_fov: int, f_px: float, d_f_px_out: int, d_out: int,
                   oh: int, ow: int, stream: int = 0) -> None:
    """Device pointers in/out (fp32), enqueued on `stream`; d_fov = 0 takes the host float f_px."""
    _lib.call("mde_op_dp_postprocess", C.c_void_p(int(d_inv)), int(batch), int(ih), int(iw),
              C.c_void_p(int(d_fov or 0)), float(f_px), C.c_void_p(int(d_f_px_out or 0)), C.c_void_p(int(d_out)),
              int(oh), int(ow), C.c_void_p(int(stream or 0)))


class DepthProDevicePostprocess:
    """Owns the metric depth map and the focal lengths (device + pinned host);
    `run(d_inv, d_fov, stream, f_px=None)` enqueues mde_op_dp_postprocess on
    the engine's output bindings in place, brings both back and synchronizes
    once.  Returns (host view [batch, oh, ow], f_px float32 [batch]) that the
    next call overwrites.  With f_px given, d_fov is not read (it may be 0)."""

    def __init__(self, batch: int, ih: int, iw: int, oh: int, ow: int):
        self.shape = (int(batch), int(oh), int(ow))
        self.src = (int(ih), int(iw))
        self.mem: Optional[HostDeviceMem] = None
        self.f_px: Optional[HostDeviceMem] = None
        try:
            self.mem = HostDeviceMem(self.shape[0] * self.shape[1] * self.shape[2], np.dtype(np.float32))
            self.f_px = HostDeviceMem(self.shape[0], np.dtype(np.float32))
        except Exception:
            self.free()
            raise

    def run(self, d_inv: int, d_fov: int, stream: int, f_px: Optional[float] = None):
        self.enqueue(d_inv, d_fov, stream, f_px=f_px)
        stream_synchronize(stream)
        return self.result()

    def result(self):
        """The host views of the last enqueue(); valid once its stream has synchronized."""
        if self.mem is None:
            raise RuntimeError("DepthProDevicePostprocess already freed")
        return self.mem.host.reshape(self.shape), self.f_px.host

    def enqueue(self, d_inv: int, d_fov: int, stream: int, f_px: Optional[float] = None) -> None:
        """The kernel and both downloads on `stream`, without synchronizing (run() = enqueue,
        synchronize, result; a caller timing the leg records its events around this)."""
        if self.mem is None:
            raise RuntimeError("DepthProDevicePostprocess already freed")
        if f_px is None and not d_fov:
            raise ValueError("DepthProDevicePostprocess.run needs the fov_deg binding or an f_px")
        b, oh, ow = self.shape
        dp_postprocess(d_inv, b, self.src[0], self.src[1], 0 if f_px is not None else d_fov,
                       0.0 if f_px is None else f_px, self.f_px.device, self.mem.device, oh, ow, stream)
        for m in (self.mem, self.f_px):
            _lib.call("mde_rt_memcpy_dtoh_async", m.host.ctypes.data_as(C.c_void_p), C.c_void_p(m.device),
                      m.nbytes, C.c_void_p(int(stream or 0)))

    def free(self) -> None:
        for m in (self.mem, self.f_px):
            if m is not None:
                m.free()
        self.mem = self.f_px = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def depth_pro_postprocess(canonical_inverse_depth: np.ndarray, fov_deg: np.ndarray, src_hw, f_px=None):
    """Reference `models/depth_pro/onnx2trt.py:100-117` (outside its timed
    loop): focal length from the predicted FOV (unless given), inverse depth
    rescaled by W / f_px, bilinear (align_corners=False) to the source size
    when it differs from the engine's, depth = 1 / clamp(inv, 1e-4, 1e4).
    Returns (depth [H, W] float32, f_px float)."""
    import torch
    import torch.nn.functional as F
    inv = torch.from_numpy(np.ascontiguousarray(canonical_inverse_depth, dtype=np.float32)).reshape(
        1, 1, *canonical_inverse_depth.shape[-2:])
    H, W = int(src_hw[0]), int(src_hw[1])
    if f_px is None:
        fov = torch.from_numpy(np.asarray(fov_deg, dtype=np.float32).reshape(-1)[:1])
        f_px = 0.5 * W / torch.tan(0.5 * torch.deg2rad(fov.to(torch.float)))
    else:
        f_px = torch.tensor([float(f_px)])
    inv = inv * (W / f_px)
    if (H, W) != tuple(inv.shape[-2:]):
        inv = F.interpolate(inv, size=(H, W), mode="bilinear", align_corners=False)
    depth = 1.0 / torch.clamp(inv, min=1e-4, max=1e4)
    return depth.squeeze().numpy(), float(f_px.squeeze())
