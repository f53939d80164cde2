"""Pre-process for the DA-V2 family (the input half): the
reference's `core/preprocess.py:preprocess_for` for `depth_anything_v2`,
`depth_anything_ac` and `distill_any_depth` -- cvtColor(BGR2RGB), a
`cv2.resize(INTER_LINEAR)` stretch on uint8 to the engine size, /255, ImageNet
standardise, NCHW float32 -- on the host in numpy (`preprocess_host`) and on
the device as one HIP kernel (`DevicePreprocess`, csrc/preprocess.hip).

`cv2` is not a dependency.  `resize_linear_u8` restates OpenCV's published
fixed-point algorithm for 8-bit images (the contract is spelled out in
include/mde.h at mde_op_resize_u8); parity with cv2 itself is not pinned here
("Device preprocess").  What is pinned: the kernel is bit-identical
to `resize_linear_u8`, and `resize_linear_u8` stays within one level of exact
bilinear interpolation.

Depth Pro's pre-process is another function (normalise, then torch's float32
bilinear) and has its own section further down; VGGT's (square pad with
white, one cv2 INTER_CUBIC on uint8, /255) follows it; the last section is the
DA-V2 family's `native` profile (no stretch: a keep-ratio cv2 INTER_CUBIC on
the float image, `preprocess_native_host` / `NativePreprocess`).
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .common_runtime import HostDeviceMem, stream_synchronize

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
# model -> dtype of the /255 division (core/preprocess.py:_builders scale_dtype); the
# standardise step is float64 for all three
SCALE_DTYPE = {"depth_anything_v2": np.float64, "distill_any_depth": np.float64, "depth_anything_ac": np.float32}
OUTPUTS = ("float32_nchw", "uint8_nhwc")
COEF_BITS = 11  # cv2's INTER_RESIZE_COEF_BITS: weights are multiples of 1 / 2048


def _axis_table(dst: int, src: int, clamp_fraction: bool):
    """Per output index of one axis: (tap0, tap1, w0, w1) as integer arrays."""
    scale = 1.0 / (float(dst) / float(src))  # float64; not src / dst
    pos = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    base = np.floor(pos)
    frac = pos - base  # float32
    lo = base.astype(np.int32)
    if clamp_fraction:  # horizontal: the border pixels are copied, not blended
        frac = np.where((lo < 0) | (lo >= src - 1), np.float32(0), frac)
    one, full = np.float32(1), np.float32(1 << COEF_BITS)
    w0 = np.rint((one - frac) * full).astype(np.int32)
    w1 = np.rint(frac * full).astype(np.int32)
    return np.clip(lo, 0, src - 1), np.clip(lo + 1, 0, src - 1), w0, w1


def resize_linear_u8(img_hwc_u8: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """`cv2.resize(img, (ow, oh), interpolation=cv2.INTER_LINEAR)` for a uint8
    [H, W, C] image, in numpy integer arithmetic: whole-image gathers through
    per-axis tables, the horizontal pass first (exact integers), then the
    vertical pass with cv2's two truncating shifts.  An exact 2x reduction on
    both axes is cv2's area path (the rounded mean of each 2x2 block)."""
    img = np.asarray(img_hwc_u8)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError(f"resize_linear_u8 wants a uint8 [H, W, C] image, got {img.dtype} {img.shape}")
    sh, sw = img.shape[:2]
    oh, ow = int(oh), int(ow)
    if oh < 1 or ow < 1 or sh < 1 or sw < 1:
        raise ValueError("resize_linear_u8: sizes must be positive")
    if sw == 2 * ow and sh == 2 * oh:
        blocks = img.astype(np.int32).reshape(oh, 2, ow, 2, -1)
        return ((blocks.sum(axis=(1, 3)) + 2) >> 2).astype(np.uint8)
    x0, x1, a0, a1 = _axis_table(ow, sw, clamp_fraction=True)
    y0, y1, b0, b1 = _axis_table(oh, sh, clamp_fraction=False)
    # int32 holds every intermediate: H <= 255 * 2049, b * (H >> 4) <= 2048 * 32656
    rows = img[:, x0].astype(np.int32) * a0[None, :, None] + img[:, x1].astype(np.int32) * a1[None, :, None]
    rows >>= 4
    top = (rows[y0] * b0[:, None, None]) >> 16
    bottom = (rows[y1] * b1[:, None, None]) >> 16
    out = (top + bottom + 2) >> 2
    return out.astype(np.uint8)


def normalize_lut(model: str) -> np.ndarray:
    """float32 [3][256]: channel c of pixel value u after the reference's
    `scale` and `standardize` for `model`, computed in their dtypes."""
    if model not in SCALE_DTYPE:
        raise KeyError(f"no preprocessing declared for {model!r} (have {sorted(SCALE_DTYPE)})")
    u = np.arange(256, dtype=np.uint8)[:, None].repeat(3, axis=1)  # [256][3]: every value in every channel
    return np.ascontiguousarray(_normalize(u, model).T)


def _normalize(img_u8: np.ndarray, model: str) -> np.ndarray:
    """[..., 3] uint8 RGB -> float32, the reference's scale() then standardize()."""
    x = img_u8.astype(SCALE_DTYPE[model]) / 255.0  # float32 stays float32 against a Python float
    x = (x - np.asarray(IMAGENET_MEAN, np.float64)) / np.asarray(IMAGENET_STD, np.float64)  # float64
    return x.astype(np.float32)


def check_second_stage(model: str, h: int, w: int) -> None:
    """The reference runs a second, cubic resize on the float image
    (keep-ratio for v2 / ac, snap for distill); at its built profiles that is
    the identity, and only then is this module its counterpart."""
    if model not in SCALE_DTYPE:
        raise KeyError(f"no preprocessing declared for {model!r} (have {sorted(SCALE_DTYPE)})")
    if h % 14 or w % 14 or (model != "distill_any_depth" and h > w):
        raise ValueError(f"{model} at {h}x{w}: the reference's second resize stage is not the identity there "
                         f"(needs multiples of 14{'' if model == 'distill_any_depth' else ' and h <= w'})")


def preprocess_host(img_bgr: np.ndarray, model: str, size: Tuple[int, int]):
    """BGR uint8 [H, W, 3] frame -> (float32 [1, 3, h, w] blob, (src_h, src_w)):
    `core/preprocess.py:preprocess_for(img_bgr, model, size)` on the host."""
    h, w = int(size[0]), int(size[1])
    check_second_stage(model, h, w)
    img = np.asarray(img_bgr)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"preprocess_host wants a uint8 [H, W, 3] BGR image, got {img.dtype} {img.shape}")
    rgb = resize_linear_u8(img[:, :, ::-1], h, w)
    blob = np.ascontiguousarray(_normalize(rgb, model).transpose(2, 0, 1)[None])
    return blob, (img.shape[0], img.shape[1])


def load_image_bgr(path: str) -> np.ndarray:
    """uint8 [H, W, 3] BGR: a .npy holding exactly that, or any image file
    Pillow can decode (its decoders are not guaranteed byte-identical to
    cv2.imread's)."""
    if path.lower().endswith(".npy"):
        img = np.load(path, allow_pickle=False)
    else:
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError(f"decoding {path} needs Pillow, which is not installed; convert the image to a "
                               f".npy holding a uint8 [H, W, 3] BGR array instead") from e
        with Image.open(path) as im:
            img = np.asarray(im.convert("RGB"))[:, :, ::-1]
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"{path}: expected a uint8 [H, W, 3] BGR image, got {img.dtype} {img.shape}")
    return np.ascontiguousarray(img)


def resize_u8(d_src: int, batch: int, sh: int, sw: int, pitch: int, swap_rb: bool, d_dst: int, oh: int, ow: int,
              stream: int = 0, d_lut: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream`: uint8 NHWC out, or with
    `d_lut` (device float[3][256]) float32 NCHW out."""
    head = (C.c_void_p(int(d_src)), int(batch), int(sh), int(sw), int(pitch), int(bool(swap_rb)))
    tail = (C.c_void_p(int(d_dst)), int(oh), int(ow), C.c_void_p(int(stream or 0)))
    if d_lut:
        _lib.call("mde_op_resize_u8_norm", *head, C.c_void_p(int(d_lut)), *tail)
    else:
        _lib.call("mde_op_resize_u8", *head, *tail)


class _FramePreprocess:
    """What the device pre-processes share: the source frame (pinned host +
    device), an optional device LUT, run / fill_binding / free and the context
    manager.  A subclass passes its geometry, the size of one output element
    and its LUT to __init__ and implements _enqueue (one kernel, no sync)."""

    def __init__(self, src_hw, dst_hw, batch: int, output: str, itemsize: int, lut: Optional[np.ndarray]):
        self.src = (int(src_hw[0]), int(src_hw[1]))
        self.dst = (int(dst_hw[0]), int(dst_hw[1]))
        self.batch = int(batch)
        self.output = output
        self.itemsize = int(itemsize)  # bytes of one output element
        self.mem: Optional[HostDeviceMem] = None
        self.lut: Optional[HostDeviceMem] = None
        try:
            self.mem = HostDeviceMem(self.batch * self.src[0] * self.src[1] * 3, np.uint8)
            if lut is not None:  # float32, or float64 where the subclass's kernel reads doubles
                lut_dtype = np.float64 if lut.dtype == np.float64 else np.float32
                self.lut = HostDeviceMem(lut.size, lut_dtype)
                self.lut.host = np.ascontiguousarray(lut, dtype=lut_dtype)
                _lib.call("mde_rt_memcpy_htod_async", C.c_void_p(self.lut.device),
                          self.lut.host.ctypes.data_as(C.c_void_p), self.lut.nbytes, None)
                _lib.call("mde_rt_device_synchronize")
        except Exception:
            self.free()
            raise

    def _enqueue(self, d_src: int, pitch: int, swap_rb: bool, d_dst: int, stream: int) -> None:
        raise NotImplementedError

    def run_device(self, d_src: int, pitch: int, d_dst: int, stream: int, swap_rb: bool = True) -> None:
        """Frames already on the device: [batch][src_h][pitch] bytes, BGR unless swap_rb=False."""
        if self.mem is None:
            raise RuntimeError(f"{type(self).__name__} already freed")
        self._enqueue(d_src, pitch, swap_rb, d_dst, stream)

    def run(self, img_bgr: np.ndarray, d_dst: int, stream: int) -> None:
        if self.mem is None:
            raise RuntimeError(f"{type(self).__name__} already freed")
        img = np.asarray(img_bgr)
        want = (self.batch, self.src[0], self.src[1], 3)
        if img.dtype != np.uint8 or img.shape not in (want, want[1:] if self.batch == 1 else want):
            raise ValueError(f"{type(self).__name__}.run wants a uint8 BGR array of shape {want}, got {img.dtype} "
                             f"{img.shape}")
        host = self.mem.host
        np.copyto(host.reshape(want), img.reshape(want))
        _lib.call("mde_rt_memcpy_htod_async", C.c_void_p(self.mem.device), host.ctypes.data_as(C.c_void_p),
                  host.nbytes, C.c_void_p(int(stream or 0)))
        self.run_device(self.mem.device, 3 * self.src[1], d_dst, stream)

    def fill_binding(self, img_bgr: np.ndarray, binding: HostDeviceMem, stream: int) -> None:
        """run() into an input binding of allocate_buffers, then bring the same
        bytes back into its pinned host side in stream order and synchronize:
        do_inference's own upload of `binding.host` then rewrites the device
        side with what is already there."""
        need = self.batch * self.dst[0] * self.dst[1] * 3 * self.itemsize
        if binding.nbytes < need:
            raise ValueError(f"binding holds {binding.nbytes} bytes, the {self.output} result needs {need}")
        self.run(img_bgr, binding.device, stream)
        _lib.call("mde_rt_memcpy_dtoh_async", binding.host.ctypes.data_as(C.c_void_p), C.c_void_p(binding.device),
                  need, C.c_void_p(int(stream or 0)))
        stream_synchronize(stream)

    def free(self) -> None:
        for m in (self.mem, self.lut):
            if m is not None:
                m.free()
        self.mem = self.lut = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


class DevicePreprocess(_FramePreprocess):
    """Owns the source frame (pinned host + device) and the device LUT;
    `run(img_bgr, d_dst, stream)` copies the frame to the device and enqueues
    the resize straight into the engine's input binding `d_dst`:
    output "float32_nchw" -> [batch][3][oh][ow] float32 (binding "input"),
    "uint8_nhwc" -> [batch][oh][ow][3] uint8 RGB (binding "image_u8").
    run() and run_device() only enqueue.  run() stages the frame in the one
    pinned buffer this object owns and copies it from there asynchronously, so
    the caller must synchronize `stream` (or otherwise know that copy has
    finished) before the next run() overwrites the buffer; fill_binding() does.
    The result is on the device in stream order: anything that reads `d_dst`
    must be enqueued on `stream` or after a synchronize of it (the streams of
    allocate_buffers are non-blocking: the null stream does not wait for them)."""

    def __init__(self, src_h: int, src_w: int, oh: int, ow: int, model: str, output: str = "float32_nchw",
                 batch: int = 1):
        if output not in OUTPUTS:
            raise ValueError(f"output must be one of {OUTPUTS}, got {output!r}")
        check_second_stage(model, int(oh), int(ow))
        f32 = output == "float32_nchw"
        super().__init__((src_h, src_w), (oh, ow), batch, output, 4 if f32 else 1,
                         normalize_lut(model) if f32 else None)

    def _enqueue(self, d_src, pitch, swap_rb, d_dst, stream):
        resize_u8(d_src, self.batch, self.src[0], self.src[1], pitch, swap_rb, d_dst, self.dst[0], self.dst[1],
                  stream, self.lut.device if self.lut is not None else 0)


# ---- Depth Pro -------------------------------------------------------------
# Its pre-process is not the stretch above (and has no entry in SCALE_DTYPE):
# reference models/depth_pro/onnx2trt.py:56-74 normalises first (ToTensor,
# Normalize(0.5, 0.5)) and then resizes the float image with torch's bilinear,
# align_corners=False.  The contract is spelled out in include/mde.h at
# mde_op_dp_preprocess; resize_bilinear_f32 restates it in numpy float32, one
# rounding per operation in the contract's order, and the kernel
# (csrc/depth_pro_photo.hip) is held to it bit for bit.


def depth_pro_lut() -> np.ndarray:
    """float32 [256]: pixel value u after ToTensor and Normalize(0.5, 0.5),
    ((float32(u) / 255) - 0.5) / 0.5 with every step in float32."""
    u = np.arange(256, dtype=np.float32)
    return ((u / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)


def _axis_lin(dst: int, src: int):
    """Per output index of one axis: (i0, i1, l0, l1), float32 weights."""
    f32 = np.float32
    scale = f32(src) / f32(dst)
    x = scale * (np.arange(dst, dtype=np.float32) + f32(0.5)) - f32(0.5)
    x = np.maximum(x, f32(0))
    i0 = np.minimum(x.astype(np.int64), src - 1)
    i1 = np.minimum(i0 + 1, src - 1)
    l1 = np.clip(x - i0.astype(np.float32), f32(0), f32(1))
    l0 = f32(1) - l1
    assert x.dtype == l0.dtype == l1.dtype == np.float32
    return i0, i1, l0, l1


def resize_bilinear_f32(img_chw_f32: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """`F.interpolate(img, (oh, ow), mode="bilinear", align_corners=False)`
    for a float32 [..., H, W] image as the include/mde.h contract states it:
    out = b0 * (a0 * v00 + a1 * v01) + b1 * (a0 * v10 + a1 * v11), float32
    throughout.  The horizontal blend runs over whole source rows first; per
    element that is the contract's operation order."""
    img = np.asarray(img_chw_f32)
    if img.dtype != np.float32 or img.ndim < 2:
        raise ValueError(f"resize_bilinear_f32 wants a float32 [..., H, W] image, got {img.dtype} {img.shape}")
    sh, sw = img.shape[-2:]
    oh, ow = int(oh), int(ow)
    if oh < 1 or ow < 1 or sh < 1 or sw < 1:
        raise ValueError("resize_bilinear_f32: sizes must be positive")
    x0, x1, a0, a1 = _axis_lin(ow, sw)
    y0, y1, b0, b1 = _axis_lin(oh, sh)
    rows = a0 * img[..., x0] + a1 * img[..., x1]  # [..., sh, ow]
    out = b0[:, None] * rows[..., y0, :] + b1[:, None] * rows[..., y1, :]
    assert out.dtype == np.float32
    return out


def preprocess_depth_pro_host(img_bgr: np.ndarray, size: int):
    """BGR uint8 [H, W, 3] photo -> (float32 [1, 3, size, size] blob, (H, W)):
    the reference's cvtColor(BGR2RGB), transform and F.interpolate on the host."""
    img = np.asarray(img_bgr)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"preprocess_depth_pro_host wants a uint8 [H, W, 3] BGR image, got {img.dtype} {img.shape}")
    x = depth_pro_lut()[img[:, :, ::-1]].transpose(2, 0, 1)
    blob = np.ascontiguousarray(resize_bilinear_f32(x, int(size), int(size))[None])
    return blob, (img.shape[0], img.shape[1])


def dp_preprocess(d_src: int, batch: int, sh: int, sw: int, pitch: int, swap_rb: bool, d_lut: int, d_dst: int,
                  oh: int, ow: int, stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream`: float32 NCHW out through `d_lut` (device float[256])."""
    _lib.call("mde_op_dp_preprocess", C.c_void_p(int(d_src)), int(batch), int(sh), int(sw), int(pitch),
              int(bool(swap_rb)), C.c_void_p(int(d_lut)), C.c_void_p(int(d_dst)), int(oh), int(ow),
              C.c_void_p(int(stream or 0)))


class DepthProPreprocess(_FramePreprocess):
    """DevicePreprocess's counterpart for Depth Pro: owns the source frame
    (pinned host + device) and the device LUT float[256]; run / run_device /
    fill_binding write the engine's "input" binding, float32
    [batch][3][size][size], under the same stream-order rules."""

    def __init__(self, src_h: int, src_w: int, size: int, batch: int = 1):
        super().__init__((src_h, src_w), (size, size), batch, "float32_nchw", 4, depth_pro_lut())

    def _enqueue(self, d_src, pitch, swap_rb, d_dst, stream):
        dp_preprocess(d_src, self.batch, self.src[0], self.src[1], pitch, swap_rb, self.lut.device, d_dst,
                      self.dst[0], self.dst[1], stream)


# ---- VGGT --------------------------------------------------------------------
# Reference models/vggt/onnx2trt.py:32-53 over core/preprocess.py:
# resize_square_pad and _builders().vggt: BGR->RGB, pad to a square with white
# at source resolution, ONE cv2.resize(INTER_CUBIC) on uint8 to size^2, /255 in
# float32, rank 5.  The contract is spelled out in include/mde.h at
# mde_op_resize_cubic_u8; resize_cubic_u8 restates OpenCV's published scalar
# fixed-point algorithm in numpy integers, and the kernel
# (csrc/preprocess_cubic.hip) is held to it bit for bit.  As for the linear
# resize, parity with cv2 itself is not pinned here (cv2 is not a dependency).
# One more caveat for cubic: vectorised builds of OpenCV evaluate the vertical
# pass in float32 (beta / 2^22 multiply-adds, then round) instead of the integer
# form, and can differ from it by one level on pixels whose exact sum sits at a
# rounding boundary.  The contract is the scalar integer form.  What is pinned:
# the kernel is bit-identical to resize_cubic_u8, and resize_cubic_u8 stays
# within the bound derived in DESIGN.md ("VGGT photo path") of exact bicubic
# interpolation.

CUBIC_A = np.float32(-0.75)  # cv2's interpolateCubic
VGGT_PAD = (255, 255, 255)   # core/preprocess.py:_builders().vggt pad_value


def _axis_cubic_f32(dst: int, src: int):
    """Per output index of one axis: (taps int32 [4][dst], clamped to
    [0, src - 1], coefficients float32 [4][dst]); float32 with one rounding
    per operation, in the contract's order.  What the 8-bit and the float
    cubic resize share."""
    f32 = np.float32
    scale = 1.0 / (float(dst) / float(src))  # float64; not src / dst
    pos = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    base = np.floor(pos)
    x = pos - base  # float32
    A, one = CUBIC_A, f32(1)
    x1 = x + one
    c0 = ((A * x1 - f32(5) * A) * x1 + f32(8) * A) * x1 - f32(4) * A
    c1 = (((A + f32(2)) * x - (A + f32(3))) * x) * x + one
    g = one - x
    c2 = (((A + f32(2)) * g - (A + f32(3))) * g) * g + one
    c3 = ((one - c0) - c1) - c2
    c = np.stack([c0, c1, c2, c3])
    assert c.dtype == np.float32
    taps = np.clip(base.astype(np.int32)[None] + np.arange(-1, 3, dtype=np.int32)[:, None], 0, src - 1)
    return taps, c


def _axis_cubic(dst: int, src: int):
    """Per output index of one axis: (taps int32 [4][dst], clamped to
    [0, src - 1], weights int32 [4][dst]): _axis_cubic_f32's coefficients
    rounded to multiples of 1 / 2048."""
    taps, c = _axis_cubic_f32(dst, src)
    k = np.rint(c * np.float32(1 << COEF_BITS)).astype(np.int32)
    return taps, k


def resize_cubic_u8(img_hwc_u8: np.ndarray, oh: int, ow: int, pad=(0, 0, 0, 0), pad_value=(0, 0, 0)) -> np.ndarray:
    """`cv2.resize(cv2.copyMakeBorder(img, *pad, cv2.BORDER_CONSTANT, value=
    pad_value), (ow, oh), interpolation=cv2.INTER_CUBIC)` for a uint8
    [H, W, 3] image, in numpy integer arithmetic: whole-image gathers through
    per-axis tables, the horizontal pass first (exact integers, no shift), then
    the vertical pass with cv2's one rounding shift and the clamp to 0..255.
    pad = (top, bottom, left, right); pad_value is in the image's own channel
    order.  The border is materialised here, on the host, only."""
    img = np.asarray(img_hwc_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"resize_cubic_u8 wants a uint8 [H, W, 3] image, got {img.dtype} {img.shape}")
    oh, ow = int(oh), int(ow)
    top, bottom, left, right = (int(p) for p in pad)
    value = np.asarray(pad_value)
    if oh < 1 or ow < 1 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("resize_cubic_u8: sizes must be positive")
    if min(top, bottom, left, right) < 0:
        raise ValueError(f"resize_cubic_u8: negative pad {pad}")
    if value.shape != (3,) or (value < 0).any() or (value > 255).any():
        raise ValueError(f"resize_cubic_u8: pad_value must be three values in 0..255, got {pad_value!r}")
    sh, sw = img.shape[:2]
    padded = np.empty((top + sh + bottom, left + sw + right, 3), np.uint8)
    padded[:] = value.astype(np.uint8)
    padded[top:top + sh, left:left + sw] = img
    tx, a = _axis_cubic(ow, padded.shape[1])
    ty, b = _axis_cubic(oh, padded.shape[0])
    # int32 holds every intermediate: sum |k| <= 2818 per axis, 255 * 2818^2 + 2^21 < 2^31
    rows = sum(padded[:, tx[i]].astype(np.int32) * a[i][None, :, None] for i in range(4))
    v = sum(rows[ty[j]] * b[j][:, None, None] for j in range(4))
    assert v.dtype == np.int32
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def square_pad_geometry(h: int, w: int, dst: int):
    """((top, bottom, left, right), (x1, y1, x2, y2)) of the reference's
    resize_square_pad(symmetric=True): the same count on both sides, so an odd
    difference leaves the padded frame one short of square (768 x 1025 is
    padded to 1024 x 1025 and the two axes get different scales); the float
    box, on the dst x dst grid, uses dst / max_dim all the same -- these four
    floats are what the crop rounds."""
    h, w, dst = int(h), int(w), int(dst)
    if h < 1 or w < 1 or dst < 1:
        raise ValueError("square_pad_geometry: sizes must be positive")
    max_dim = max(h, w)
    left = (max_dim - w) // 2
    top = (max_dim - h) // 2
    scale = dst / max_dim
    return (top, top, left, left), (left * scale, top * scale, (left + w) * scale, (top + h) * scale)


def box_window(box):
    """(y0, x0, ch, cw) of the reference's depth[int(round(y1)):int(round(y2)),
    int(round(x1)):int(round(x2))]."""
    x1, y1, x2, y2 = (int(round(v)) for v in box)
    return y1, x1, y2 - y1, x2 - x1


def vggt_lut() -> np.ndarray:
    """float32 [3][256]: pixel value u after the reference's scale,
    float32(u) / 255 in float32, the same for every channel."""
    u = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.ascontiguousarray(np.broadcast_to(u, (3, 256)))


def _vggt_frames(frames_bgr) -> np.ndarray:
    fr = np.asarray(frames_bgr)
    if fr.ndim == 3:
        fr = fr[None]
    if fr.dtype != np.uint8 or fr.ndim != 4 or fr.shape[3] != 3 or fr.shape[0] < 1:
        raise ValueError(f"VGGT wants uint8 BGR frames [S, H, W, 3] of one size, got {fr.dtype} {fr.shape}")
    return fr


def preprocess_vggt_host(frames_bgr, size: int):
    """BGR uint8 frames [S, H, W, 3] (or one [H, W, 3]) -> (float32
    [1, S, 3, size, size] blob in [0, 1], box (x1, y1, x2, y2)):
    `core/preprocess.py:preprocess_for(frame, 'vggt', (size, size))` per frame
    on the host."""
    fr = _vggt_frames(frames_bgr)
    size = int(size)
    pad, box = square_pad_geometry(fr.shape[1], fr.shape[2], size)
    lut = vggt_lut()[0]
    out = [lut[resize_cubic_u8(f[:, :, ::-1], size, size, pad, VGGT_PAD)].transpose(2, 0, 1) for f in fr]
    return np.ascontiguousarray(np.stack(out)[None]), box


def resize_cubic_u8_device(d_src: int, batch: int, sh: int, sw: int, pitch: int, swap_rb: bool, pad, pad_value,
                           d_dst: int, oh: int, ow: int, stream: int = 0, d_lut: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream`: uint8 NHWC out, or with
    `d_lut` (device float[3][256]) float32 NCHW out.  pad = (top, bottom, left,
    right); pad_value in output channel order."""
    head = (C.c_void_p(int(d_src)), int(batch), int(sh), int(sw), int(pitch), int(bool(swap_rb)),
            *(int(p) for p in pad), *(int(v) for v in pad_value))
    tail = (C.c_void_p(int(d_dst)), int(oh), int(ow), C.c_void_p(int(stream or 0)))
    if d_lut:
        _lib.call("mde_op_resize_cubic_u8_norm", *head, C.c_void_p(int(d_lut)), *tail)
    else:
        _lib.call("mde_op_resize_cubic_u8", *head, *tail)


def crop_f32(d_src: int, batch: int, h: int, w: int, y0: int, x0: int, ch: int, cw: int, d_dst: int,
             stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream`: rows [y0, y0 + ch), columns
    [x0, x0 + cw) of float32 maps [batch][h][w] -> [batch][ch][cw]."""
    _lib.call("mde_op_crop_f32", C.c_void_p(int(d_src)), int(batch), int(h), int(w), int(y0), int(x0), int(ch),
              int(cw), C.c_void_p(int(d_dst)), C.c_void_p(int(stream or 0)))


class VggtPreprocess(_FramePreprocess):
    """DevicePreprocess's counterpart for VGGT: owns the S source frames of one
    size (pinned host + device) and the device LUT float[3][256]; run /
    run_device / fill_binding write the engine's "images" binding, float32
    [1][frames][3][size][size], under the same stream-order rules.  `.pad` is
    the virtual border (top, bottom, left, right), `.box` the content box
    (x1, y1, x2, y2) on the size x size grid that the crop rounds."""

    def __init__(self, src_h: int, src_w: int, size: int, frames: int = 1):
        self.pad, self.box = square_pad_geometry(src_h, src_w, size)
        super().__init__((src_h, src_w), (size, size), frames, "float32_nchw", 4, vggt_lut())

    def _enqueue(self, d_src, pitch, swap_rb, d_dst, stream):
        resize_cubic_u8_device(d_src, self.batch, self.src[0], self.src[1], pitch, swap_rb, self.pad, VGGT_PAD, d_dst,
                               self.dst[0], self.dst[1], stream, self.lut.device)


# ---- DA-V2 family, native profile ---------------------------------------------
# Reference models/depth_anything_ac/onnx2trt.py:50-77 (`profile = 'native'`)
# over core/preprocess.py: preprocess_for(img, model, size, stretch=False) --
# BGR->RGB, NO first resize, /255 in the model's scale dtype, then the second
# geometry stage ResizeStep("keep_ratio", interp="cubic") on the FLOAT image
# (short side to `target`, aspect kept, sides snapped to multiples of 14),
# standardise in float64, float32 NCHW.  The contract is spelled out in
# include/mde.h at mde_op_resize_cubic_f_norm; resize_cubic_float restates
# OpenCV's published scalar INTER_CUBIC for CV_32FC3 / CV_64FC3 in numpy, one
# rounding per operation in the contract's order, and the kernel
# (csrc/preprocess_cubic.hip) is held to it bit for bit.  Parity with cv2
# itself is not pinned (cv2 is not a dependency; DESIGN.md "Native profile"
# says what that leaves open).

NATIVE_ROUNDING = {"depth_anything_ac": "ceil", "depth_anything_v2": "constrain"}


def native_size(model: str, src_h: int, src_w: int, target: int = 518, multiple: int = 14) -> Tuple[int, int]:
    """(h, w) of the network input for a src_h x src_w photo: the reference's
    resize_keep_ratio(bound="lower") over _round_to_multiple, in the same
    float64 expressions (300 x 400 at target 42 gives h * scale =
    42.00000000000001 and `ceil` makes 56 of it: reproduced, not corrected).
    depth_anything_ac rounds up; depth_anything_v2 rounds half to even and
    falls back to up where that lands below `target`."""
    if model not in NATIVE_ROUNDING:
        raise ValueError(f"{model} has no native size: its second resize stage is "
                         f"{'a snap to the engine size' if model == 'distill_any_depth' else 'not declared'}, "
                         f"not a keep-ratio rule (have {sorted(NATIVE_ROUNDING)})")
    src_h, src_w, target, multiple = int(src_h), int(src_w), int(target), int(multiple)
    if src_h < 1 or src_w < 1 or target < 1 or multiple < 1:
        raise ValueError("native_size: sizes, target and multiple must be positive")
    scale = target / min(src_h, src_w)  # float64

    def snap(x: float) -> int:
        q = x / multiple
        if NATIVE_ROUNDING[model] == "ceil":
            y = int(np.ceil(q)) * multiple
        else:
            y = int(np.round(q) * multiple)  # half to even
            if y < target:
                y = int(np.ceil(q) * multiple)
        return max(y, multiple)

    return snap(src_h * scale), snap(src_w * scale)


def scale_lut(model: str) -> np.ndarray:
    """T[256]: pixel value u after the reference's `scale`, u.astype(T) / 255.0
    in the model's scale dtype T."""
    return np.arange(256, dtype=np.uint8).astype(SCALE_DTYPE[model]) / 255.0


def resize_cubic_float(img_hwc: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """`cv2.resize(img, (ow, oh), interpolation=cv2.INTER_CUBIC)` for a float32
    or float64 [H, W, 3] image, dtype preserved: OpenCV's scalar algorithm with
    _axis_cubic_f32's positions, taps and float32 coefficients, the horizontal
    pass over whole rows first, then the vertical pass, every product and sum
    rounded once in the image's dtype, left to right; no clamp."""
    img = np.asarray(img_hwc)
    if img.dtype not in (np.float32, np.float64) or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"resize_cubic_float wants a float32 or float64 [H, W, 3] image, got {img.dtype} {img.shape}")
    oh, ow = int(oh), int(ow)
    if oh < 1 or ow < 1 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("resize_cubic_float: sizes must be positive")
    T = img.dtype
    tx, a = _axis_cubic_f32(ow, img.shape[1])
    ty, b = _axis_cubic_f32(oh, img.shape[0])
    assert a.dtype == b.dtype == np.float32
    # float32 * float32 stays float32; float64 * float32 is a float64 product (HResizeCubic<double, double, float>)
    rows = img[:, tx[0]] * a[0][None, :, None]
    for i in range(1, 4):
        rows = rows + img[:, tx[i]] * a[i][None, :, None]
    assert rows.dtype == T
    out = rows[ty[0]] * b[0][:, None, None]
    for j in range(1, 4):
        out = out + rows[ty[j]] * b[j][:, None, None]
    assert out.dtype == T
    return out


def preprocess_native_host(img_bgr: np.ndarray, model: str, target: int = 518):
    """BGR uint8 [H, W, 3] photo -> (float32 [1, 3, h, w] blob, (src_h, src_w))
    with (h, w) = native_size(model, H, W, target): the reference's
    `preprocess_for(img_bgr, model, (target, .), stretch=False)` on the host."""
    img = np.asarray(img_bgr)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"preprocess_native_host wants a uint8 [H, W, 3] BGR image, got {img.dtype} {img.shape}")
    h, w = native_size(model, img.shape[0], img.shape[1], target)
    x = img[:, :, ::-1].astype(SCALE_DTYPE[model]) / 255.0  # float32 stays float32 against a Python float
    assert x.dtype == SCALE_DTYPE[model]
    x = resize_cubic_float(x, h, w)
    x = (x - np.asarray(IMAGENET_MEAN, np.float64)) / np.asarray(IMAGENET_STD, np.float64)  # float64
    blob = np.ascontiguousarray(x.astype(np.float32).transpose(2, 0, 1)[None])
    return blob, (img.shape[0], img.shape[1])


def resize_cubic_f_norm(d_src: int, batch: int, sh: int, sw: int, pitch: int, swap_rb: bool, wide: bool, d_lut: int,
                        mean, std, d_dst: int, oh: int, ow: int, stream: int = 0) -> None:
    """Device pointers in/out, enqueued on `stream`: float32 NCHW out.  `d_lut`
    is a device float[256] (wide false) or double[256] (wide true) holding
    u / 255; mean and std are in output channel order."""
    _lib.call("mde_op_resize_cubic_f_norm", C.c_void_p(int(d_src)), int(batch), int(sh), int(sw), int(pitch),
              int(bool(swap_rb)), int(bool(wide)), C.c_void_p(int(d_lut)), *(float(m) for m in mean),
              *(float(s) for s in std), C.c_void_p(int(d_dst)), int(oh), int(ow), C.c_void_p(int(stream or 0)))


class NativePreprocess(_FramePreprocess):
    """DevicePreprocess's counterpart for the native profile of
    depth_anything_v2 / depth_anything_ac: owns the source frame (pinned host +
    device) and the device table of u / 255 in the model's scale dtype; run /
    run_device / fill_binding write the engine's "input" binding, float32
    [batch][3][h][w] with (h, w) = `.dst` = native_size(model, src_h, src_w,
    target), under the same stream-order rules.  The engine must have been
    packed for that size."""

    def __init__(self, src_h: int, src_w: int, model: str, target: int = 518, batch: int = 1):
        self.model = model
        self.target = int(target)
        dst = native_size(model, src_h, src_w, target)
        self.wide = SCALE_DTYPE[model] == np.float64
        super().__init__((src_h, src_w), dst, batch, "float32_nchw", 4, scale_lut(model))

    def _enqueue(self, d_src, pitch, swap_rb, d_dst, stream):
        resize_cubic_f_norm(d_src, self.batch, self.src[0], self.src[1], pitch, swap_rb, self.wide, self.lut.device,
                            IMAGENET_MEAN, IMAGENET_STD, d_dst, self.dst[0], self.dst[1], stream)


__all__ = ["resize_linear_u8", "normalize_lut", "preprocess_host", "load_image_bgr", "resize_u8",
           "DevicePreprocess", "check_second_stage", "depth_pro_lut", "resize_bilinear_f32",
           "preprocess_depth_pro_host", "dp_preprocess", "DepthProPreprocess", "resize_cubic_u8",
           "square_pad_geometry", "box_window", "vggt_lut", "preprocess_vggt_host", "resize_cubic_u8_device",
           "crop_f32", "VggtPreprocess", "native_size", "scale_lut", "resize_cubic_float",
           "preprocess_native_host", "resize_cubic_f_norm", "NativePreprocess"]
