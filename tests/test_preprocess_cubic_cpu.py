"""Host side of VGGT's photo path (preprocess.py, last section): the numpy
restatement of cv2's uint8 INTER_CUBIC behind a constant border, the square-pad
geometry, the LUT, preprocess_vggt_host, the ABI's argument checks and the
driver's flags.  No GPU.

Parity with cv2 itself is not pinned (cv2 is absent; DESIGN.md "VGGT photo
path").  Pinned here: the restatement against exact bicubic interpolation with
the same A = -0.75 and replicate borders (torch float64, align_corners=False --
an independent implementation) to within the bound DESIGN.md derives from the
contract, written out again in `bound` below: a property of the algorithm, not
a tuned tolerance.  Measured on the cases below: 0.57 .. 0.71 levels.
"""

import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from monocular_depth_estimation_trt_amd import preprocess as pre

WHITE = (255, 255, 255)


def noise(h, w, seed=7):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def padded(img, pad, value):
    t, b, l, r = pad
    out = np.empty((t + img.shape[0] + b, l + img.shape[1] + r, 3), np.uint8)
    out[:] = np.asarray(value, np.uint8)
    out[t:t + img.shape[0], l:l + img.shape[1]] = img
    return out


def exact_bicubic(img_u8, oh, ow):
    x = torch.from_numpy(img_u8.astype(np.float64).transpose(2, 0, 1)[None])
    y = F.interpolate(x, size=(oh, ow), mode="bicubic", align_corners=False)
    return np.clip(y[0].numpy().transpose(1, 2, 0), 0.0, 255.0)


def bound(ph, pw):
    """Levels between the contract and exact bicubic interpolation of a ph x pw
    image ("VGGT photo path").  Per axis the four weights k_i / 2048
    differ from the exact ones by at most E in total:
      4 * 0.5 / 2048   each k_i is rounded to a multiple of 1 / 2048
      3 * src * 2^-24  the coordinate is rounded once to float32, |error| <= src * 2^-24, and the weights as
                       a function of the position change by at most sum |W'| = 3 per unit
      4e-5             float32 evaluation of the four polynomials: a dozen roundings of values below 8 each
    With pixel values in [0, 255] and sum |c| <= 1.375 on the other axis the sum moves by at most
    255 * (1.375 * (Ex + Ey) + Ex * Ey); the final shift rounds to the nearest level, 0.5 more; clipping
    both sides to [0, 255] does not increase a difference."""
    ex, ey = (4 * 0.5 / 2048 + 3 * src * 2.0 ** -24 + 4e-5 for src in (pw, ph))
    return 0.5 + 255 * (1.375 * (ex + ey) + ex * ey)


CASES = [(37, 53, 28, 28, (0, 0, 0, 0)),
         (9, 5, 28, 14, (0, 0, 0, 0)),        # upscale, all four borders clamp
         (300, 400, 98, 98, (50, 50, 0, 0)),
         (30, 53, 28, 28, (11, 11, 0, 0)),    # one row short of square: the axis scales differ
         (53, 30, 28, 28, (0, 0, 11, 11))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d" % c[:4])
def test_restatement_within_derived_bound_of_exact_bicubic(case):
    sh, sw, oh, ow, pad = case
    img = noise(sh, sw)
    got = pre.resize_cubic_u8(img, oh, ow, pad, WHITE)
    assert got.dtype == np.uint8 and got.shape == (oh, ow, 3)
    p = padded(img, pad, WHITE)
    err = float(np.abs(got.astype(np.float64) - exact_bicubic(p, oh, ow)).max())
    lim = bound(*p.shape[:2])
    print(f"{case}: max |restatement - exact| = {err:.4f} levels, bound {lim:.4f}")
    assert 1.18 < lim < 1.30  # the derivation's own size at these shapes
    assert err <= lim


def test_bound_ingredients():
    """sum |c| <= 1.375 with the maximum at x = 0.5, sum |W'| <= 3, and the
    fixed-point weights: sums 2047 .. 2049, sum |k| <= 2818 (int32 holds V)."""
    A = -0.75
    x = np.linspace(0.0, 1.0, 100001)

    def w(t):
        t = np.abs(t)
        return np.where(t <= 1, ((A + 2) * t - (A + 3)) * t * t + 1, ((A * t - 5 * A) * t + 8 * A) * t - 4 * A)

    def dw(t):
        t = np.abs(t)
        return np.where(t <= 1, (3 * (A + 2) * t - 2 * (A + 3)) * t, (3 * A * t - 10 * A) * t + 8 * A)

    taps = np.stack([x + 1, x, 1 - x, 2 - x])
    s = np.abs(w(taps)).sum(0)
    assert abs(s.max() - 1.375) < 1e-12 and abs(x[s.argmax()] - 0.5) < 1e-12
    assert np.abs(dw(taps)).sum(0).max() <= 3.0 + 1e-12
    _, k = pre._axis_cubic(100000, 99991)  # fractions all over [0, 1)
    assert k.dtype == np.int32 and k.shape == (4, 100000)
    assert set(np.unique(k.sum(0))) == {2047, 2048, 2049}
    assert np.abs(k).sum(0).max() <= 2818
    assert 255 * 2818 ** 2 + (1 << 21) < 2 ** 31


def test_same_size_is_the_identity():
    """x = 0 on both axes: coefficients 0, 2048, 0, 0."""
    img = noise(28, 42)
    _, k = pre._axis_cubic(42, 42)
    assert (k == np.array([0, 2048, 0, 0])[:, None]).all()
    assert np.array_equal(pre.resize_cubic_u8(img, 28, 42), img)


def test_constant_image_stays_constant():
    """Every value 0..255, with that value as the pad colour: coefficient sums
    of 2047..2049 move 255 by less than 0.26 of a level, which the rounding
    shift absorbs."""
    for v in range(256):
        img = np.full((7, 12, 3), v, np.uint8)
        out = pre.resize_cubic_u8(img, 9, 9, (2, 2, 0, 0), (v, v, v))
        assert (out == v).all(), v
    img = np.empty((5, 6, 3), np.uint8)
    img[:] = (3, 128, 255)
    assert (pre.resize_cubic_u8(img, 13, 4, (0, 0, 1, 1), (3, 128, 255)) == np.array([3, 128, 255])).all()


def test_border_is_the_pad_colour_not_the_edge():
    """A black photo in a white border: the border rows come out white, the
    middle black; without the border everything is black."""
    out = pre.resize_cubic_u8(np.zeros((30, 53, 3), np.uint8), 28, 28, (11, 11, 0, 0), WHITE)
    assert (out[0] == 255).all() and (out[-1] == 255).all() and (out[14] == 0).all()
    assert (pre.resize_cubic_u8(np.zeros((30, 53, 3), np.uint8), 28, 28) == 0).all()


def test_pad_value_is_per_channel():
    img = noise(30, 53)
    out = pre.resize_cubic_u8(img, 28, 28, (11, 11, 0, 0), (7, 130, 250))
    assert (out[0] == np.array([7, 130, 250])).all()
    for c, v in enumerate((7, 130, 250)):
        one = pre.resize_cubic_u8(img, 28, 28, (11, 11, 0, 0), (v, v, v))
        assert np.array_equal(out[..., c], one[..., c])


def test_refuses_bad_arguments():
    img = noise(5, 6)
    for kw in (dict(pad=(0, -1, 0, 0)), dict(pad_value=(0, 0, 256)), dict(pad_value=(0, 0)), dict(oh=0)):
        args = dict(oh=4, ow=4)
        args.update(kw)
        with pytest.raises(ValueError):
            pre.resize_cubic_u8(img, **args)
    with pytest.raises(ValueError):
        pre.resize_cubic_u8(img.astype(np.float32), 4, 4)


def reference_geometry(w, h, dst):
    """core/preprocess.py:resize_square_pad(symmetric=True), its own lines."""
    max_dim = max(h, w)
    left = (max_dim - w) // 2
    top = (max_dim - h) // 2
    right, bottom = left, top
    scale = dst / max_dim
    x1, y1 = left * scale, top * scale
    x2, y2 = (left + w) * scale, (top + h) * scale
    return (top, bottom, left, right), (x1, y1, x2, y2)


@pytest.mark.parametrize("wh", [(1280, 720), (720, 1280), (900, 900), (3024, 2268), (1025, 768)],
                         ids=lambda s: "%dx%d" % s)
def test_square_pad_geometry_matches_the_reference_formulas(wh):
    w, h = wh
    pad, box = pre.square_pad_geometry(h, w, 518)
    assert (pad, box) == reference_geometry(w, h, 518)
    assert all(isinstance(v, int) for v in pad) and all(isinstance(v, float) for v in box)
    assert pad[0] == pad[1] and pad[2] == pad[3]  # the same count on both sides


def test_square_pad_geometry_odd_difference_is_one_short_of_square():
    pad, box = pre.square_pad_geometry(768, 1025, 518)
    assert pad == (128, 128, 0, 0) and pad[0] + 768 + pad[1] == 1024
    assert box == (0.0, 128 * (518 / 1025), 518.0, (128 + 768) * (518 / 1025))
    pad, _ = pre.square_pad_geometry(2268, 3024, 518)
    assert pad == (378, 378, 0, 0)
    pad, _ = pre.square_pad_geometry(1280, 720, 518)
    assert pad == (0, 0, 280, 280)


@pytest.mark.parametrize("wh", [(640, 480), (1280, 720), (1920, 1080), (720, 1280), (500, 500), (3024, 2268),
                                (100, 4000), (4000, 100)], ids=lambda s: "%dx%d" % s)
def test_box_rounds_inside_the_map(wh):
    w, h = wh
    _, box = pre.square_pad_geometry(h, w, 518)
    x1, y1, x2, y2 = (int(round(v)) for v in box)
    assert 0 <= y1 < y2 <= 518 and 0 <= x1 < x2 <= 518
    assert pre.box_window(box) == (y1, x1, y2 - y1, x2 - x1)


def test_vggt_lut():
    lut = pre.vggt_lut()
    assert lut.dtype == np.float32 and lut.shape == (3, 256) and lut.flags.c_contiguous
    want = np.arange(256).astype(np.float32) / 255.0  # the reference's img.astype(float32) / 255.0
    assert want.dtype == np.float32
    assert all(np.array_equal(lut[c].view(np.uint32), want.view(np.uint32)) for c in range(3))
    assert lut[0, 0] == 0 and lut[0, 255] == 1


def test_preprocess_vggt_host():
    frames = np.stack([noise(60, 80, seed=1), noise(60, 80, seed=2)])
    blob, box = pre.preprocess_vggt_host(frames, 98)
    pad, want_box = pre.square_pad_geometry(60, 80, 98)
    assert blob.dtype == np.float32 and blob.shape == (1, 2, 3, 98, 98) and blob.flags.c_contiguous
    assert box == want_box and pad == (10, 10, 0, 0)
    for s in range(2):
        rgb = pre.resize_cubic_u8(frames[s][:, :, ::-1], 98, 98, pad, WHITE)
        want = (rgb.astype(np.float32) / 255.0).transpose(2, 0, 1)
        assert np.array_equal(blob[0, s].view(np.uint32), want.view(np.uint32))
    assert (blob[0, :, :, 0] == 1).all()  # the white border
    assert not np.array_equal(blob[0, 0], blob[0, 1])
    one, _ = pre.preprocess_vggt_host(frames[0], 98)  # one [H, W, 3] frame
    assert np.array_equal(one[0, 0], blob[0, 0])
    with pytest.raises(ValueError):
        pre.preprocess_vggt_host(frames.astype(np.float32), 98)


def test_exports():
    for name in ("resize_cubic_u8", "square_pad_geometry", "vggt_lut", "preprocess_vggt_host", "VggtPreprocess",
                 "resize_cubic_u8_device", "crop_f32"):
        assert name in pre.__all__ and hasattr(pre, name)


@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


CUBIC_BAD = [dict(src=None), dict(dst=None), dict(batch=0), dict(sh=0), dict(sw=-1), dict(oh=0), dict(ow=0),
             dict(pitch=23), dict(pad=(-1, 0, 0, 0)), dict(pad=(0, -1, 0, 0)), dict(pad=(0, 0, -1, 0)),
             dict(pad=(0, 0, 0, -1)), dict(color=(256, 0, 0)), dict(color=(0, -1, 0)), dict(color=(0, 0, 1000)),
             dict(sh=46341, sw=46341, pitch=3 * 46341),              # source plane >= 2^31 - 256
             dict(pad=(2 ** 30, 2 ** 30, 0, 0)),                     # virtual plane (and more rows than an int holds)
             dict(pad=(0, 0, 2 ** 28, 0)),                           # virtual plane: 8 rows of 2^28 + 8 columns
             dict(oh=46341, ow=46341),                               # destination plane
             dict(batch=65536)]


@pytest.mark.parametrize("fn", ["mde_op_resize_cubic_u8", "mde_op_resize_cubic_u8_norm"])
def test_cubic_ops_check_arguments_before_any_device_call(lib, fn):
    p = ctypes.c_void_p(4096)  # never dereferenced: the checks run first

    def call(src=p, dst=p, lut=p, batch=1, sh=8, sw=8, pitch=24, pad=(0, 0, 0, 0), color=(0, 0, 0), oh=4, ow=4):
        head = (src, batch, sh, sw, pitch, 1, *pad, *color)
        if fn.endswith("_norm"):
            return getattr(lib, fn)(*head, lut, dst, oh, ow, None)
        return getattr(lib, fn)(*head, dst, oh, ow, None)

    bad = CUBIC_BAD + ([dict(lut=None)] if fn.endswith("_norm") else [])
    for kw in bad:
        assert call(**kw) == 1, kw
        assert fn.encode() + b":" in lib.mde_last_error(), (kw, lib.mde_last_error())


def test_crop_checks_arguments_before_any_device_call(lib):
    p = ctypes.c_void_p(4096)

    def call(src=p, dst=p, batch=1, h=8, w=8, y0=1, x0=1, ch=4, cw=4):
        return lib.mde_op_crop_f32(src, batch, h, w, y0, x0, ch, cw, dst, None)

    for kw in (dict(src=None), dict(dst=None), dict(batch=0), dict(h=0), dict(w=0), dict(ch=0), dict(cw=0),
               dict(y0=-1), dict(x0=-1), dict(y0=5), dict(x0=5), dict(ch=9), dict(cw=9),
               dict(y0=2 ** 31 - 1, ch=2), dict(h=46341, w=46341), dict(batch=65536)):
        assert call(**kw) == 1, kw
        assert b"mde_op_crop_f32:" in lib.mde_last_error(), (kw, lib.mde_last_error())


def test_version_is_12(lib):
    """The cubic ops came into ABI 11 without a new number; 12 is the row / head / patch-embed surfaces."""
    assert lib.mde_version() == 12


def test_driver_parser_accepts_images():
    from monocular_depth_estimation_trt_amd.models.vggt import run
    a = run.build_parser().parse_args(["--image", "a.npy", "b.npy", "--host-preprocess", "--color", "out.png"])
    assert a.image == ["a.npy", "b.npy"] and a.host_preprocess and a.color == "out.png"
    a = run.build_parser().parse_args([])  # every earlier default is still there
    assert (a.image, a.input, a.box, a.frames, a.iterations, a.warmup) == ([], "", None, 1, 100, 20)
    assert run.network_size("synthetic:vggt:tiny", 518) == 98
    assert run.network_size("synthetic:vggt:vggt_1b:2468", 518) == 518
    assert run.network_size("model.safetensors", 518) == 518


def test_driver_loads_frames(tmp_path):
    from monocular_depth_estimation_trt_amd.models.vggt import run
    f = np.stack([noise(6, 8, seed=1), noise(6, 8, seed=2)])
    np.save(tmp_path / "a.npy", f[0])
    np.save(tmp_path / "b.npy", f[1])
    np.save(tmp_path / "both.npy", f)
    np.save(tmp_path / "c.npy", noise(6, 9))
    assert np.array_equal(run.load_frames([str(tmp_path / "a.npy"), str(tmp_path / "b.npy")]), f)
    assert np.array_equal(run.load_frames([str(tmp_path / "both.npy")]), f)
    assert run.load_frames([str(tmp_path / "a.npy")]).shape == (1, 6, 8, 3)
    with pytest.raises(SystemExit):
        run.load_frames([str(tmp_path / "a.npy"), str(tmp_path / "c.npy")])
    for args in (["--image", "a.npy", "--input", "x.npy"], ["--host-preprocess"], ["--color", "o.png"]):
        with pytest.raises(SystemExit):
            run.main(args)
