"""Host side of the device preprocess (preprocess.py): the numpy restatement of
cv2's uint8 INTER_LINEAR, the normalisation LUT, preprocess_host, the ABI's
argument checks and the driver flag.  No GPU.

Parity with cv2 itself is not pinned (cv2 is absent; DESIGN.md "Device
preprocess").  Pinned here: the restatement against a scalar transcription of
the contract in include/mde.h, and against exact bilinear interpolation
(torch float64, align_corners=False) to within one level.  The 1.0 bound is a
property of the algorithm -- two 11-bit coefficient roundings and two
truncating shifts leave less than one level -- not a tuned tolerance.
"""

import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from monocular_depth_estimation_trt_amd import preprocess as pre
from monocular_depth_estimation_trt_amd import weights

MODELS = ("depth_anything_v2", "distill_any_depth", "depth_anything_ac")


def noise(h, w, seed=7):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(255 * x) // max(w - 1, 1), (255 * y) // max(h - 1, 1),
                     (255 * (x + y)) // max(h + w - 2, 1)], axis=-1).astype(np.uint8)


IMAGES = {"noise": noise, "ramp": ramp}


def scalar_linear(img, oh, ow):
    """The linear path of the include/mde.h contract, one pixel at a time."""
    sh, sw = img.shape[:2]
    f32 = np.float32

    def axis(d, dst, src):
        scale = 1.0 / (float(dst) / float(src))
        f = f32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        return s, f32(f - f32(s))

    def coef(f):
        return int(np.rint(f32(f32(1) - f) * f32(2048))), int(np.rint(f32(f * f32(2048))))

    out = np.empty((oh, ow, img.shape[2]), np.uint8)
    for oy in range(oh):
        sy, fy = axis(oy, oh, sh)
        b0, b1 = coef(fy)
        y0, y1 = min(max(sy, 0), sh - 1), min(max(sy + 1, 0), sh - 1)
        for ox in range(ow):
            sx, fx = axis(ox, ow, sw)
            if sx < 0:
                sx, fx = 0, f32(0)
            if sx >= sw - 1:
                sx, fx = sw - 1, f32(0)
            x1 = min(sx + 1, sw - 1)
            a0, a1 = coef(fx)
            for c in range(img.shape[2]):
                h0 = int(img[y0, sx, c]) * a0 + int(img[y0, x1, c]) * a1
                h1 = int(img[y1, sx, c]) * a0 + int(img[y1, x1, c]) * a1
                v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
                assert 0 <= v <= 255
                out[oy, ox, c] = v
    return out


def block_mean(img):
    s = img.astype(np.int64)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


@pytest.mark.parametrize("kind", IMAGES)
def test_identity_size_returns_the_input(kind):
    img = IMAGES[kind](28, 42)
    assert np.array_equal(pre.resize_linear_u8(img, 28, 42), img)


@pytest.mark.parametrize("kind", IMAGES)
def test_exact_half_on_both_axes_is_the_block_mean(kind):
    img = IMAGES[kind](56, 84)
    got = pre.resize_linear_u8(img, 28, 42)
    assert np.array_equal(got, block_mean(img))
    # the linear path agrees there (weights 1024 / 1024 on both axes, no border): the
    # special case is a shortcut, not another function
    assert np.array_equal(got, scalar_linear(img, 28, 42))


@pytest.mark.parametrize("kind", IMAGES)
def test_half_on_one_axis_only_stays_linear(kind):
    img = IMAGES[kind](56, 53)
    assert np.array_equal(pre.resize_linear_u8(img, 28, 42), scalar_linear(img, 28, 42))


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("shape", [(37, 53, 28, 42), (9, 5, 28, 14), (56, 84, 28, 42)])
def test_swap_rb_commutes_with_the_resize(kind, shape):
    sh, sw, oh, ow = shape
    img = IMAGES[kind](sh, sw)
    assert np.array_equal(pre.resize_linear_u8(img[:, :, ::-1], oh, ow), pre.resize_linear_u8(img, oh, ow)[:, :, ::-1])


@pytest.mark.parametrize("shape", [(37, 53, 28, 42), (9, 5, 28, 14), (13, 29, 14, 28)])
def test_matches_the_scalar_contract(shape):
    sh, sw, oh, ow = shape
    img = noise(sh, sw, seed=sh)
    assert np.array_equal(pre.resize_linear_u8(img, oh, ow), scalar_linear(img, oh, ow))


@pytest.mark.parametrize("kind", IMAGES)
@pytest.mark.parametrize("shape", [(37, 53, 28, 42), (9, 5, 28, 14), (31, 47, 98, 98), (600, 800, 392, 518),
                                   (13, 29, 14, 28)])
def test_within_one_level_of_exact_bilinear(kind, shape):
    sh, sw, oh, ow = shape
    img = IMAGES[kind](sh, sw)
    got = pre.resize_linear_u8(img, oh, ow).astype(np.float64)
    t = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    ref = F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    err = float(np.abs(got - ref).max())
    print(f"{kind} {shape}: max |restatement - bilinear| = {err:.4f}")
    assert err < 1.0, err


def reference_arithmetic(rgb_u8, model):
    """core/preprocess.py scale() + standardize() + the float32 cast, spelled out."""
    if model == "depth_anything_ac":
        x = rgb_u8.astype(np.float32) / 255.0
        assert x.dtype == np.float32
    else:
        x = rgb_u8.astype(np.float64) / 255.0
    x = (x - np.asarray((0.485, 0.456, 0.406), np.float64)) / np.asarray((0.229, 0.224, 0.225), np.float64)
    assert x.dtype == np.float64
    return x.astype(np.float32)


@pytest.mark.parametrize("model", MODELS)
def test_lut_gather_equals_reference_arithmetic(model):
    lut = pre.normalize_lut(model)
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    img = noise(33, 45, seed=11)
    got = np.stack([lut[c][img[:, :, c]] for c in range(3)], axis=-1)
    assert np.array_equal(got.view(np.uint32), reference_arithmetic(img, model).view(np.uint32))


def test_v2_and_ac_luts_differ():
    assert (pre.normalize_lut("depth_anything_v2").view(np.uint32)
            != pre.normalize_lut("depth_anything_ac").view(np.uint32)).any()
    assert np.array_equal(pre.normalize_lut("depth_anything_v2"), pre.normalize_lut("distill_any_depth"))
    with pytest.raises(KeyError):
        pre.normalize_lut("depth_pro")


def test_preprocess_host_at_engine_size_equals_synthetic_images():
    rgb = weights.synthetic_images_u8(1, 518, 518, first_seed=3)[0]
    blob, src_hw = pre.preprocess_host(np.ascontiguousarray(rgb[:, :, ::-1]), "depth_anything_v2", (518, 518))
    assert src_hw == (518, 518) and blob.dtype == np.float32 and blob.shape == (1, 3, 518, 518)
    assert np.array_equal(blob.view(np.uint32), weights.synthetic_images(1, 518, 518, first_seed=3).view(np.uint32))


def test_preprocess_host_resizes_and_refuses_other_second_stages():
    bgr = noise(60, 80, seed=2)
    blob, src_hw = pre.preprocess_host(bgr, "depth_anything_ac", (28, 42))
    want = reference_arithmetic(pre.resize_linear_u8(bgr[:, :, ::-1], 28, 42), "depth_anything_ac")
    assert src_hw == (60, 80) and np.array_equal(blob[0], want.transpose(2, 0, 1))
    with pytest.raises(ValueError):
        pre.preprocess_host(bgr, "depth_anything_v2", (30, 42))   # not a multiple of 14
    with pytest.raises(ValueError):
        pre.preprocess_host(bgr, "depth_anything_v2", (42, 28))   # keep-ratio stage would resize


@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


@pytest.mark.parametrize("fn", ["mde_op_resize_u8", "mde_op_resize_u8_norm"])
def test_ops_check_arguments_before_any_device_call(lib, fn):
    p = ctypes.c_void_p(4096)  # never dereferenced: the checks run first

    def call(src=p, sh=8, sw=8, pitch=24, oh=4, ow=4):
        head = (src, 1, sh, sw, pitch, 1)
        if fn.endswith("_norm"):
            return getattr(lib, fn)(*head, p, p, oh, ow, None)
        return getattr(lib, fn)(*head, p, oh, ow, None)

    for kw in (dict(src=None), dict(oh=0), dict(pitch=23)):
        assert call(**kw) == 1, kw
        assert fn.encode() + b":" in lib.mde_last_error(), (kw, lib.mde_last_error())


def test_driver_parser_accepts_image():
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    a = run.build_parser().parse_args(["--image", "photo.npy", "--host-preprocess"])
    assert a.image == "photo.npy" and a.host_preprocess and a.src_hw is None


def test_load_image_bgr_npy(tmp_path):
    img = noise(5, 7)
    np.save(tmp_path / "a.npy", img)
    assert np.array_equal(pre.load_image_bgr(str(tmp_path / "a.npy")), img)
    np.save(tmp_path / "b.npy", img.astype(np.float32))
    with pytest.raises(ValueError):
        pre.load_image_bgr(str(tmp_path / "b.npy"))
