"""Host side of the DA-V2 family's native profile (preprocess.py, last section):
the keep-ratio size rule, the numpy restatement of cv2's scalar float
INTER_CUBIC, preprocess_native_host, the ABI's argument checks and the drivers'
flags.  No GPU.

Parity with cv2 itself is not pinned (cv2 is absent; DESIGN.md "Native
profile").  Pinned here: the size rule's values; the identity; the restatement
against exact bicubic interpolation with the same A = -0.75 and replicate
borders (torch float64, align_corners=False -- an independent implementation)
to within the bound DESIGN.md derives from the contract, written out again in
`bound` below: a property of the algorithm, not a tuned tolerance.
"""

import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from monocular_depth_estimation_trt_amd import preprocess as pre

AC, V2 = "depth_anything_ac", "depth_anything_v2"
MODELS = (AC, V2)

# (photo h, w, target) -> (depth_anything_ac, depth_anything_v2)
SIZES = {
    (2268, 3024, 518): ((518, 700), (518, 686)),
    (768, 1024, 518): ((518, 700), (518, 686)),
    (480, 640, 518): ((518, 700), (518, 686)),
    (600, 800, 518): ((518, 700), (518, 686)),
    (3024, 2268, 518): ((700, 518), (686, 518)),
    (1025, 769, 518): ((700, 518), (686, 518)),
    (60, 45, 518): ((700, 518), (686, 518)),
    (1080, 1920, 518): ((518, 924), (518, 924)),
    (720, 1280, 518): ((518, 924), (518, 924)),
    (100, 76, 518): ((686, 518), (686, 518)),
    (31, 47, 518): ((518, 798), (518, 784)),
    (37, 53, 28): ((28, 42), (28, 42)),
    (53, 37, 28): ((42, 28), (42, 28)),
    (9, 5, 28): ((56, 28), (56, 28)),
    (300, 400, 42): ((56, 70), (42, 56)),
    (100, 76, 42): ((56, 56), (56, 42)),
    (31, 47, 28): ((28, 56), (28, 42)),
    (29, 29, 28): ((28, 28), (28, 28)),
}

F32_HALF_ULP = 2.0 ** -24  # of a value in [1, 2)
F64_HALF_ULP = 2.0 ** -53


def noise(h, w, seed=7):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def exact_bicubic(img_u8, oh, ow):
    x = torch.from_numpy((img_u8 / 255.0).transpose(2, 0, 1)[None])
    assert x.dtype == torch.float64
    y = F.interpolate(x, size=(oh, ow), mode="bicubic", align_corners=False)
    return y[0].numpy().transpose(1, 2, 0)


def accumulation(half_ulp):
    """What the roundings of the two passes and of u / 255 move a result by, samples in [0, 1] and
    sum |c| <= 1.375 per axis ("Native profile"):
      horizontal  4 products below 1 (half an ulp each: half_ulp / 2) and 3 partial sums below 1.375 < 2
                  (half_ulp each) = 5 half_ulp, carried through the vertical pass: x 1.375
      vertical    4 products |H b| <= 1.375 and 3 partial sums <= 1.375^2 < 2: 7 half_ulp
      u / 255     one rounding of a value below 1, half_ulp / 2, through both passes: x 1.375^2"""
    return (5 * 1.375 + 7 + 0.5 * 1.375 ** 2) * half_ulp


def bound(sh, sw, dtype):
    """Between the contract and exact bicubic interpolation of a sh x sw image with samples in [0, 1]
    ("Native profile").  Per axis the four float32 weights differ from the exact ones by at most
    E in total:
      3 * src * 2^-24  the coordinate is rounded once to float32, |error| <= src * 2^-24, and the weights as
                       a function of the position change by at most sum |W'| = 3 per unit
      4e-5             float32 evaluation of the four polynomials: a dozen roundings of values below 8 each
    With sum |c| <= 1.375 on the other axis the sum moves by at most 1.375 * (Ex + Ey) + Ex * Ey; the
    accumulation roundings in the working type come on top."""
    ex, ey = (3 * src * 2.0 ** -24 + 4e-5 for src in (sw, sh))
    return 1.375 * (ex + ey) + ex * ey + accumulation(F32_HALF_ULP if dtype == np.float32 else F64_HALF_ULP)


@pytest.mark.parametrize("key", sorted(SIZES), ids=lambda k: "%dx%d@%d" % k)
def test_native_size_table(key):
    h, w, target = key
    assert pre.native_size(AC, h, w, target) == SIZES[key][0]
    assert pre.native_size(V2, h, w, target) == SIZES[key][1]
    if target == 518:
        assert pre.native_size(AC, h, w) == SIZES[key][0]  # the default target


def test_native_size_is_the_float64_expression():
    """300 / 300 * 42 is 42 in rationals; h * (42 / 300) is 42.00000000000001 in float64, and ceil takes it."""
    assert 300 * (42 / 300) > 42
    assert pre.native_size(AC, 300, 400, 42) == (56, 70)
    assert pre.native_size(V2, 300, 400, 42) == (42, 56)


def test_native_size_refusals():
    with pytest.raises(ValueError, match="snap"):
        pre.native_size("distill_any_depth", 480, 640)
    with pytest.raises(ValueError):
        pre.native_size("vggt", 480, 640)
    for bad in ((0, 5, 28), (5, 0, 28), (5, 5, 0)):
        with pytest.raises(ValueError):
            pre.native_size(AC, *bad)


def test_axis_cubic_shares_the_float_part():
    """_axis_cubic is _axis_cubic_f32 rounded to 1 / 2048, and returns what it returned."""
    for dst, src in ((28, 37), (56, 9), (700, 3024), (42, 42)):
        taps, c = pre._axis_cubic_f32(dst, src)
        taps_k, k = pre._axis_cubic(dst, src)
        assert c.dtype == np.float32 and c.shape == (4, dst) and k.dtype == np.int32
        assert np.array_equal(taps, taps_k)
        assert np.array_equal(k, np.rint(c * np.float32(2048)).astype(np.int32))
    _, c = pre._axis_cubic_f32(42, 42)  # fraction 0 everywhere
    assert np.array_equal(c, np.array([[0], [1], [0], [0]], np.float32).repeat(42, axis=1))
    assert not np.signbit(c).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_is_bit_exact(dtype):
    img = noise(28, 42).astype(dtype) / 255.0
    assert img.dtype == dtype
    out = pre.resize_cubic_float(img, 28, 42)
    assert out.dtype == dtype and out.tobytes() == img.tobytes()


@pytest.mark.parametrize("model", MODELS)
def test_native_host_equals_stretch_host_where_both_are_the_identity(model):
    img = noise(28, 42, seed=3)
    assert pre.native_size(model, 28, 42, 28) == (28, 42)
    blob, src_hw = pre.preprocess_native_host(img, model, target=28)
    want, _ = pre.preprocess_host(img, model, (28, 42))
    assert src_hw == (28, 42) and blob.dtype == np.float32 and blob.shape == (1, 3, 28, 42) and blob.flags.c_contiguous
    assert blob.tobytes() == want.tobytes()


SHAPES = [(37, 53, 28, 42), (9, 5, 56, 28), (300, 400, 56, 70), (53, 37, 42, 28)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_restatement_against_exact_bicubic(shape, dtype):
    sh, sw, oh, ow = shape
    u8 = noise(sh, sw)
    got = pre.resize_cubic_float(u8.astype(dtype) / 255.0, oh, ow)
    assert got.dtype == dtype and got.shape == (oh, ow, 3)
    err = float(np.abs(got.astype(np.float64) - exact_bicubic(u8, oh, ow)).max())
    print(f"{shape} {np.dtype(dtype).name}: max |restatement - exact bicubic| = {err:.3e}, bound {bound(sh, sw, dtype):.3e}")
    assert err <= bound(sh, sw, dtype)
    assert got.min() < 0 or got.max() > 1 or (sh, sw) == (oh, ow)  # overshoot is not clamped away


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_the_two_working_types_agree(shape):
    """The same taps and the same float32 coefficients: what differs is u / 255 and the 14 roundings of the
    accumulation, float32 against float64 -- accumulation(2^-24), 7.4 float32 ulps (2^-23) of 1.375."""
    sh, sw, oh, ow = shape
    u8 = noise(sh, sw, seed=11)
    a = pre.resize_cubic_float(u8.astype(np.float32) / 255.0, oh, ow)
    b = pre.resize_cubic_float(u8.astype(np.float64) / 255.0, oh, ow)
    assert a.dtype == np.float32 and b.dtype == np.float64
    err = float(np.abs(a.astype(np.float64) - b).max())
    tol = accumulation(F32_HALF_ULP) + accumulation(F64_HALF_ULP)
    print(f"{shape}: max |float32 - float64| = {err:.3e} = {err / 2.0 ** -23:.2f} ulp, bound {tol / 2.0 ** -23:.2f} ulp")
    assert tol < 8 * 2.0 ** -23
    assert err <= tol


def test_float32_path_never_promotes(monkeypatch):
    """float32 in, float32 out, and every intermediate of the float32 path is float32: the coefficients, the
    scaled image handed to the resize and the resize's result."""
    seen = []
    real = pre.resize_cubic_float

    def spy(img, oh, ow):
        out = real(img, oh, ow)
        seen.append((img.dtype, out.dtype))
        return out

    monkeypatch.setattr(pre, "resize_cubic_float", spy)
    blob, _ = pre.preprocess_native_host(noise(37, 53), AC, target=28)
    assert seen == [(np.dtype(np.float32), np.dtype(np.float32))] and blob.dtype == np.float32
    seen.clear()
    pre.preprocess_native_host(noise(37, 53), V2, target=28)
    assert seen == [(np.dtype(np.float64), np.dtype(np.float64))]
    assert pre.scale_lut(AC).dtype == np.float32 and pre.scale_lut(V2).dtype == np.float64
    want = np.arange(256).astype(np.float32) / 255.0
    assert pre.scale_lut(AC).tobytes() == want.tobytes()
    assert pre.scale_lut(V2).tobytes() == (np.arange(256) / 255.0).tobytes()
    for bad in (noise(8, 8), noise(8, 8).astype(np.float16), np.zeros((8, 8), np.float32)):
        with pytest.raises(ValueError):
            pre.resize_cubic_float(bad, 4, 4)


@pytest.mark.parametrize("model", MODELS)
def test_preprocess_native_host(model):
    img = noise(37, 53, seed=5)
    blob, src_hw = pre.preprocess_native_host(img, model, target=28)
    assert src_hw == (37, 53) and blob.dtype == np.float32 and blob.shape == (1, 3, 28, 42) and blob.flags.c_contiguous
    T = pre.SCALE_DTYPE[model]
    x = pre.resize_cubic_float(img[:, :, ::-1].astype(T) / 255.0, 28, 42)
    want = ((x - np.array(pre.IMAGENET_MEAN)) / np.array(pre.IMAGENET_STD)).astype(np.float32).transpose(2, 0, 1)
    assert blob[0].tobytes() == np.ascontiguousarray(want).tobytes()
    with pytest.raises(ValueError):
        pre.preprocess_native_host(img.astype(np.float32), model)
    with pytest.raises(ValueError):
        pre.preprocess_native_host(img, "distill_any_depth")


def test_exports():
    for name in ("native_size", "scale_lut", "resize_cubic_float", "preprocess_native_host", "resize_cubic_f_norm",
                 "NativePreprocess"):
        assert name in pre.__all__ and hasattr(pre, name)


def test_check_second_stage_still_refuses():
    for model in MODELS:
        with pytest.raises(ValueError):
            pre.check_second_stage(model, 168, 126)  # portrait
        with pytest.raises(ValueError):
            pre.preprocess_host(noise(60, 45), model, (168, 126))


@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


def test_op_checks_arguments_before_any_device_call(lib):
    p = ctypes.c_void_p(4096)  # never dereferenced: the checks run first
    nan = float("nan")

    def call(src=p, dst=p, lut=p, batch=1, sh=8, sw=8, pitch=24, wide=0, mean=(0.5, 0.4, 0.3), std=(0.2, 0.3, 0.4),
             oh=4, ow=4):
        return lib.mde_op_resize_cubic_f_norm(src, batch, sh, sw, pitch, 1, wide, lut, *mean, *std, dst, oh, ow, None)

    for kw in (dict(src=None), dict(dst=None), dict(lut=None), dict(batch=0), dict(sh=0), dict(sw=-1), dict(oh=0),
               dict(ow=0), dict(pitch=23), dict(wide=2), dict(wide=-1), dict(std=(0.0, 0.3, 0.4)),
               dict(std=(0.2, 0.0, 0.4)), dict(std=(0.2, 0.3, 0.0)), dict(std=(0.2, nan, 0.4)),
               dict(mean=(nan, 0.4, 0.3)), dict(lut=ctypes.c_void_p(4100), wide=1), dict(lut=ctypes.c_void_p(4097)),
               dict(sh=46341, sw=46341, pitch=3 * 46341), dict(oh=46341, ow=46341), dict(batch=65536)):
        assert call(**kw) == 1, kw
        assert b"mde_op_resize_cubic_f_norm:" in lib.mde_last_error(), (kw, lib.mde_last_error())


def test_version_is_12(lib):
    """The native profile's op came into ABI 11 without a new number; 12 is the row / head / patch-embed surfaces."""
    assert lib.mde_version() == 12


def test_driver_parser_defaults_are_unchanged():
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    a = run.build_parser().parse_args([])
    assert a.profile == "bench" and a.native_target == 518
    assert a.engine.endswith("depth_anything_v2_vits_518x518_fp16.mdeng")
    a = run.build_parser().parse_args(["--profile", "native", "--native-target", "126", "--image", "p.npy"])
    assert a.profile == "native" and a.native_target == 126


def test_native_engine_path_carries_the_size():
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    default = run.build_parser(AC).get_default("engine")
    assert run.native_engine_path(AC, default, default, (518, 700)).endswith("depth_anything_ac_vits_518x700_fp16.mdeng")
    assert run.native_engine_path(AC, "/x/mine.mdeng", default, (518, 700)) == "/x/mine.mdeng"


@pytest.mark.parametrize("argv,model,why", [
    (["--profile", "native"], AC, "--image"),
    (["--profile", "native", "--input", "x.npy"], AC, "--input"),
    (["--profile", "native", "--image", "p.npy", "--input", "x.npy"], V2, ""),
    (["--profile", "native", "--image", "p.npy", "--input-format", "uint8_nhwc"], V2, "uint8_nhwc"),
    (["--profile", "native", "--image", "p.npy"], "distill_any_depth", "distill_any_depth"),
    (["--profile", "native", "--image", "p.npy", "--native-target", "0"], AC, "--native-target"),
], ids=["no-image", "input", "image-and-input", "uint8", "distill", "target"])
def test_driver_refuses(argv, model, why):
    """Each refusal comes before the photo is opened (p.npy does not exist) and before any engine is built."""
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    with pytest.raises(SystemExit) as e:
        run.main(argv, model=model)
    assert why in str(e.value)
