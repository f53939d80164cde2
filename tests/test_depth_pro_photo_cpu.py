"""Host side of the Depth Pro photo path: the numpy restatements of the
include/mde.h contracts (preprocess.resize_bilinear_f32 / preprocess_depth_pro_host,
postprocess.depth_pro_postprocess_np) against torch on the CPU -- the reference's own
arithmetic (models/depth_pro/onnx2trt.py:56-74 and :118-134) -- the ABI's argument
checks and the driver's flags.  No GPU.

The restatements round every operation to float32 separately; torch's CPU kernel may
fuse scale * (d + 0.5) - 0.5 depending on the host's vector dispatch, so the comparison
carries a derived tolerance, not a bit pattern:

  the two orders differ by at most 1.5 ulp of a source coordinate x < S, so a blend
  weight differs by at most 1.5 S 2^-23 per axis; each weight multiplies a tap
  difference of at most 2 (inputs in [-1, 1]): 3 (sh + sw) 2^-23, and four blend
  roundings add 2^-21.
    pre-process   |restatement - torch| <= 3 (sh + sw) 2^-23 + 2^-21, absolute
    post-process  relative error of depth <= 9 (ih + iw) 2^-23 + 2^-20, for maps drawn
                  from [0.5, 2] (max / min <= 4, so the weight error times (max / min - 1)
                  is at most 3x the pre-process form; the last term covers the blend and
                  division roundings and a few ulp of tan)
    focal length  4 2^-23 relative
"""

import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from monocular_depth_estimation_trt_amd import postprocess as post
from monocular_depth_estimation_trt_amd import preprocess as pre

PRE_SHAPES = [(37, 53, 48),
              (9, 5, 28),      # upscale, all four borders
              (96, 128, 48),   # exact 2x reduction: torch has no area path, neither may this
              (100, 76, 64),
              (48, 48, 48)]    # identity
POST_SHAPES = [(48, 48, 37, 53), (48, 48, 100, 76), (28, 28, 9, 5), (64, 48, 96, 128), (48, 48, 48, 48)]
EPS = 2.0 ** -23


def pre_bar(sh, sw):
    return 3 * (sh + sw) * EPS + 2.0 ** -21


def post_bar(ih, iw):
    return 9 * (ih + iw) * EPS + 2.0 ** -20


def photo(sh, sw):
    return np.random.Generator(np.random.PCG64(sh * 10007 + sw)).integers(0, 256, size=(sh, sw, 3), dtype=np.uint8)


def inverse_depth(ih, iw, oh, ow):
    rng = np.random.Generator(np.random.PCG64((ih * 131 + iw) * 65537 + oh * 257 + ow))
    return rng.uniform(0.5, 2.0, size=(ih, iw)).astype(np.float32)


def torch_transform(rgb_u8):
    """torchvision's ToTensor + Normalize([0.5] * 3, [0.5] * 3), spelled out in torch."""
    t = torch.from_numpy(np.ascontiguousarray(rgb_u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean = torch.full((3, 1, 1), 0.5, dtype=torch.float32)
    std = torch.full((3, 1, 1), 0.5, dtype=torch.float32)
    return t.sub(mean).div(std)[None]


def test_lut_is_the_torch_transform_bit_for_bit():
    lut = pre.depth_pro_lut()
    assert lut.shape == (256,) and lut.dtype == np.float32
    ref = ((torch.arange(256, dtype=torch.float32) / 255) - 0.5) / 0.5
    assert np.array_equal(lut.view(np.uint32), ref.numpy().view(np.uint32))
    img = photo(7, 11)
    assert np.array_equal(lut[img].transpose(2, 0, 1)[None].view(np.uint32),
                          torch_transform(img).numpy().view(np.uint32))
    with pytest.raises(KeyError):
        pre.normalize_lut("depth_pro")  # the DA-V2 stretch is not this model's pre-process


@pytest.mark.parametrize("shape", PRE_SHAPES, ids=lambda s: "%dx%d-%d" % s)
def test_preprocess_host_matches_torch(shape):
    sh, sw, size = shape
    bgr = photo(sh, sw)
    blob, src_hw = pre.preprocess_depth_pro_host(bgr, size)
    assert src_hw == (sh, sw) and blob.shape == (1, 3, size, size) and blob.dtype == np.float32
    assert blob.flags["C_CONTIGUOUS"]
    x = torch_transform(bgr[:, :, ::-1])
    if (sh, sw) == (size, size):
        assert np.array_equal(blob.view(np.uint32), x.numpy().view(np.uint32))
        return
    ref = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False).numpy()
    err = float(np.abs(blob - ref).max())
    print(f"pre-process {shape}: max |restatement - torch| = {err:.3e} (bar {pre_bar(sh, sw):.3e})")
    assert err <= pre_bar(sh, sw), (err, pre_bar(sh, sw))
    assert np.abs(blob).max() <= 1.0


def test_resize_bilinear_f32_checks_its_input():
    with pytest.raises(ValueError):
        pre.resize_bilinear_f32(np.zeros((3, 4, 4), np.float64), 2, 2)
    with pytest.raises(ValueError):
        pre.resize_bilinear_f32(np.zeros((3, 4, 4), np.float32), 0, 2)
    with pytest.raises(ValueError):
        pre.preprocess_depth_pro_host(np.zeros((4, 4, 3), np.float32), 8)


def rel_err(got, ref):
    return float((np.abs(got.astype(np.float64) - ref) / np.abs(ref)).max())


@pytest.mark.parametrize("mode", ["fov", "f_px"])
@pytest.mark.parametrize("shape", POST_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_postprocess_np_matches_torch(shape, mode):
    ih, iw, oh, ow = shape
    inv = inverse_depth(ih, iw, oh, ow)
    rng = np.random.Generator(np.random.PCG64(oh * 1009 + ow))
    fov = np.array([rng.uniform(20.0, 90.0)], np.float32)
    f_px = None if mode == "fov" else float(rng.uniform(0.4, 1.6) * ow)
    ref, f_ref = post.depth_pro_postprocess(inv, fov, (oh, ow), f_px=f_px)
    got, f_got = post.depth_pro_postprocess_np(inv, fov, (oh, ow), f_px=f_px)
    assert got.shape == ref.shape == (oh, ow) and got.dtype == np.float32 and isinstance(f_got, float)
    assert abs(f_got - f_ref) <= 4 * EPS * abs(f_ref), (f_got, f_ref)
    if f_px is not None:
        assert f_got == float(np.float32(f_px))
    err = rel_err(got, ref)
    print(f"post-process {shape} {mode}: max rel |restatement - torch| = {err:.3e} (bar {post_bar(ih, iw):.3e})")
    assert err <= post_bar(ih, iw), (err, post_bar(ih, iw))


def test_postprocess_np_batch_equals_single():
    ih, iw, oh, ow = 48, 48, 37, 53
    inv = np.stack([inverse_depth(ih, iw, oh, ow), inverse_depth(ih, iw, ow, oh)])
    fov = np.array([35.0, 70.0], np.float32)
    got, f = post.depth_pro_postprocess_np(inv, fov, (oh, ow))
    assert got.shape == (2, oh, ow) and f.shape == (2,) and f.dtype == np.float32 and f[0] != f[1]
    for b in range(2):
        one, f1 = post.depth_pro_postprocess_np(inv[b], fov[b:b + 1], (oh, ow))
        assert np.array_equal(got[b].view(np.uint32), one.view(np.uint32)) and f1 == float(f[b])
    got4, _ = post.depth_pro_postprocess_np(inv[:, None], fov, (oh, ow))
    assert np.array_equal(got4, got)


@pytest.mark.parametrize("value, depth", [(1e-6, 1e4), (1e6, 1e-4)])
def test_postprocess_np_clamps(value, depth):
    """Constant maps below and above the clamp (k = 1: f_px = W)."""
    ih, iw, oh, ow = 48, 48, 37, 53
    inv = np.full((ih, iw), value, np.float32)
    ref, _ = post.depth_pro_postprocess(inv, None, (oh, ow), f_px=float(ow))
    got, f = post.depth_pro_postprocess_np(inv, None, (oh, ow), f_px=float(ow))
    assert f == float(ow)
    assert rel_err(got, ref) <= post_bar(ih, iw)
    assert np.array_equal(got, np.full((oh, ow), np.float32(1) / np.float32(1.0 / depth), np.float32))


def test_postprocess_np_keeps_nan_like_torch():
    """A non-finite engine output must not come out as a finite depth: NaN goes through the
    clamp as it does through torch.clamp, in exactly the same pixels."""
    ih, iw, oh, ow = 48, 48, 100, 76
    inv = inverse_depth(ih, iw, oh, ow).copy()
    inv[10, 17] = np.nan
    ref, _ = post.depth_pro_postprocess(inv, None, (oh, ow), f_px=60.0)
    got, _ = post.depth_pro_postprocess_np(inv, None, (oh, ow), f_px=60.0)
    assert np.isnan(got).any() and np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert rel_err(got[ok], ref[ok]) <= post_bar(ih, iw)


def test_driver_parser_accepts_the_photo_flags():
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    a = run.build_parser().parse_args(["--image", "photo.npy", "--host-preprocess", "--host-postprocess",
                                       "--f-px", "512.5"])
    assert a.image == "photo.npy" and a.host_preprocess and a.host_postprocess and a.f_px == 512.5
    assert a.src_hw is None and a.input == ""
    d = run.build_parser().parse_args([])
    assert d.image == "" and not d.host_preprocess and not d.host_postprocess and d.f_px is None


def test_driver_refuses_image_with_input():
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    with pytest.raises(SystemExit) as e:
        run.main(["--image", "photo.npy", "--input", "x.npy"])
    assert "exclusive" in str(e.value)


@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


P = ctypes.c_void_p(4096)  # never dereferenced: the checks run first
BIG = 2 ** 31 - 256        # a plane of this many elements is refused


@pytest.mark.parametrize("kw", [dict(src=None), dict(lut=None), dict(dst=None), dict(batch=0), dict(sh=0), dict(sw=-1),
                                dict(oh=0), dict(ow=0), dict(pitch=23), dict(oh=1, ow=BIG), dict(oh=65536, ow=32768),
                                dict(sh=65536, sw=32768, pitch=3 * 32768), dict(batch=65536)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_dp_preprocess_checks_arguments_before_any_device_call(lib, kw):
    def call(src=P, batch=1, sh=8, sw=8, pitch=24, lut=P, dst=P, oh=4, ow=4):
        return lib.mde_op_dp_preprocess(src, batch, sh, sw, pitch, 1, lut, dst, oh, ow, None)

    assert call(**kw) == 1, kw
    assert b"mde_op_dp_preprocess:" in lib.mde_last_error(), (kw, lib.mde_last_error())


@pytest.mark.parametrize("kw", [dict(inv=None), dict(out=None), dict(batch=0), dict(ih=0), dict(iw=-1), dict(oh=0),
                                dict(ow=0), dict(oh=1, ow=BIG), dict(ih=BIG, iw=1), dict(oh=65536, ow=32768),
                                dict(batch=65536), dict(fov=None, f_px=0.0), dict(fov=None, f_px=-1.0)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_dp_postprocess_checks_arguments_before_any_device_call(lib, kw):
    def call(inv=P, batch=1, ih=8, iw=8, fov=P, f_px=0.0, out=P, oh=4, ow=4):
        return lib.mde_op_dp_postprocess(inv, batch, ih, iw, fov, f_px, None, out, oh, ow, None)

    assert call(**kw) == 1, kw
    assert b"mde_op_dp_postprocess:" in lib.mde_last_error(), (kw, lib.mde_last_error())


def test_abi_version_is_12(lib):
    assert lib.mde_version() == 12
