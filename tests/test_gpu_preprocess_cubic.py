"""VGGT's photo path on the device (csrc/preprocess_cubic.hip) through the C ABI,
the Python class, the engine and the driver, against the numpy restatement
preprocess.resize_cubic_u8 -- bit for bit: both are integer arithmetic over
coefficients rounded the same way, so there is no tolerance.  (What the
restatement itself is held to: tests/test_preprocess_cubic_cpu.py.)  Every
destination is followed by a guard row that must come back untouched.
"""

import functools

import numpy as np
import pytest
import torch

from gpu_util import op, ptr, stream

from monocular_depth_estimation_trt_amd import pack_vggt, visualize, weights_vggt as WV
from monocular_depth_estimation_trt_amd import preprocess as pre
from monocular_depth_estimation_trt_amd.engine import Engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
WHITE = (255, 255, 255)
NO_PAD = (0, 0, 0, 0)
LANDSCAPE = (30, 53, 28, 28, (11, 11, 0, 0))   # the padded square is one row short: the axis scales differ
PORTRAIT = (53, 30, 28, 28, (0, 0, 11, 11))
CASES = [(37, 53, 28, 28, NO_PAD),
         (9, 5, 28, 14, NO_PAD),                # upscale, all four borders clamp
         (28, 42, 28, 42, NO_PAD),              # identity
         LANDSCAPE,
         PORTRAIT,
         (2268, 3024, 518, 518, (378, 378, 0, 0))]


def case_id(c):
    return "%dx%d-%dx%d" % c[:4] + ("-pad" if any(c[4]) else "")


@functools.lru_cache(maxsize=None)
def source(sh, sw, batch=1):
    """[batch][sh][sw][3] seeded noise; cached, never written."""
    rng = np.random.Generator(np.random.PCG64(sh * 10007 + sw))
    a = rng.integers(0, 256, size=(batch, sh, sw, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(sh, sw, oh, ow, pad, color, batch=1, swap_rb=0):
    """resize_cubic_u8 of source(...), read in output channel order; cached, never written."""
    r = np.stack([pre.resize_cubic_u8(im[:, :, ::-1] if swap_rb else im, oh, ow, pad, color)
                  for im in source(sh, sw, batch)])
    r.setflags(write=False)
    return r


def device_cubic(src_np, sh, sw, pitch, swap_rb, pad, color, oh, ow):
    """-> (result [B][oh][ow][3], the guard row after it)."""
    B = src_np.shape[0]
    d_src = torch.from_numpy(np.array(src_np)).cuda()  # a writable copy
    d_dst = torch.full((B * oh + 1, ow, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    op("mde_op_resize_cubic_u8", ptr(d_src), B, sh, sw, pitch, swap_rb, *pad, *color, ptr(d_dst), oh, ow, stream())
    out = d_dst.cpu().numpy()
    return out[:B * oh].reshape(B, oh, ow, 3), out[B * oh]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_resize_cubic_u8_bit_exact(gpu, case):
    sh, sw, oh, ow, pad = case
    got, guard = device_cubic(source(sh, sw), sh, sw, 3 * sw, 0, pad, WHITE, oh, ow)
    ref = expected(sh, sw, oh, ow, pad, WHITE)
    bad = got != ref
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (guard == SENTINEL).all()
    if (sh, sw) == (oh, ow) and not any(pad):
        assert np.array_equal(got, source(sh, sw))


@pytest.mark.parametrize("swap_rb", [0, 1])
def test_pad_colour_and_channel_order(gpu, swap_rb):
    """The pad colour is in output channel order whatever swap_rb says, and the
    taps past the photo's edge read it: a kernel that clamps at the photo's
    edge, or that swaps the colour with the pixels, differs here."""
    sh, sw, oh, ow, pad = LANDSCAPE
    color = (7, 130, 250)
    got, guard = device_cubic(source(sh, sw), sh, sw, 3 * sw, swap_rb, pad, color, oh, ow)
    ref = expected(sh, sw, oh, ow, pad, color, swap_rb=swap_rb)
    assert (ref[0, 0] == np.array(color)).all() and (ref[0, -1] == np.array(color)).all()
    assert not np.array_equal(ref, expected(sh, sw, oh, ow, NO_PAD, color, swap_rb=swap_rb))
    assert not np.array_equal(ref, expected(sh, sw, oh, ow, pad, color[::-1], swap_rb=swap_rb))
    assert np.array_equal(got, ref)
    assert (guard == SENTINEL).all()


@pytest.mark.parametrize("case", [LANDSCAPE, (9, 5, 28, 14, NO_PAD)], ids=case_id)
def test_padded_pitch_batch2(gpu, case):
    """Rows 5 bytes longer than 3*sw, the padding 0xFF, the pad colour 0: the
    filler must not reach any tap; two different frames."""
    sh, sw, oh, ow, pad = case
    pitch = 3 * sw + 5
    padded = np.full((2, sh, pitch), 0xFF, np.uint8)
    padded[:, :, :3 * sw] = source(sh, sw, 2).reshape(2, sh, 3 * sw)
    got, guard = device_cubic(padded, sh, sw, pitch, 0, pad, (0, 0, 0), oh, ow)
    assert np.array_equal(got, expected(sh, sw, oh, ow, pad, (0, 0, 0), 2))
    assert not np.array_equal(got[0], got[1])
    assert (guard == SENTINEL).all()


@pytest.mark.parametrize("case", [(37, 53, 28, 28, NO_PAD), PORTRAIT], ids=case_id)
def test_resize_cubic_u8_norm_bit_exact(gpu, case):
    sh, sw, oh, ow, pad = case
    lut = pre.vggt_lut()
    rgb = expected(sh, sw, oh, ow, pad, WHITE, 2, swap_rb=1)
    ref = np.stack([lut[c][rgb[..., c]] for c in range(3)], axis=1)  # [2][3][oh][ow]
    d_src = torch.from_numpy(source(sh, sw, 2).copy()).cuda()
    d_lut = torch.from_numpy(lut).cuda()
    d_dst = torch.full((2 * 3 * oh + 1, ow), float("nan"), dtype=torch.float32, device="cuda")
    op("mde_op_resize_cubic_u8_norm", ptr(d_src), 2, sh, sw, 3 * sw, 1, *pad, *WHITE, ptr(d_lut), ptr(d_dst), oh, ow,
       stream())
    out = d_dst.cpu().numpy()
    assert np.array_equal(out[:6 * oh].reshape(2, 3, oh, ow).view(np.uint32), ref.view(np.uint32))
    assert np.isnan(out[6 * oh]).all()


@pytest.mark.parametrize("window", [(3, 5, 11, 17), (0, 0, 23, 31)], ids=["odd-offsets", "full"])
def test_crop_f32(gpu, window):
    y0, x0, ch, cw = window
    maps = np.random.Generator(np.random.PCG64(5)).standard_normal((2, 23, 31)).astype(np.float32)
    d_src = torch.from_numpy(maps).cuda()
    d_dst = torch.full((2 * ch + 1, cw), float("nan"), dtype=torch.float32, device="cuda")
    op("mde_op_crop_f32", ptr(d_src), 2, 23, 31, y0, x0, ch, cw, ptr(d_dst), stream())
    out = d_dst.cpu().numpy()
    want = maps[:, y0:y0 + ch, x0:x0 + cw]
    assert np.array_equal(out[:2 * ch].reshape(2, ch, cw).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert np.isnan(out[2 * ch]).all()


def frames_60x80():
    return np.ascontiguousarray(source(60, 80, 2))


def _run(eng, d_images, shape):
    """The VGGT engine on an "images" tensor already on the device (current torch stream)."""
    ctx = eng.create_execution_context()
    out = torch.full(shape[:2] + shape[3:] + (1,), float("nan"), device="cuda")
    ctx.set_input_shape("images", shape)
    ctx.set_tensor_address("images", d_images.data_ptr())
    ctx.set_tensor_address("depth", out.data_ptr())
    ctx.execute_async_v3(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    ctx.destroy()
    return y


def test_vggt_preprocess_into_engine(gpu):
    """Two 60x80 BGR frames -> VggtPreprocess -> the tiny VGGT engine (98^2, S = 2), against the same
    engine fed the host-side preprocess."""
    cfg = WV.vggt_config("tiny")
    size = cfg["img"]
    assert size == 98
    blob = pack_vggt.pack_bytes(WV.synthetic_state_dict(cfg, 2468), cfg, 2)
    frames = frames_60x80()
    host_blob, box = pre.preprocess_vggt_host(frames, size)
    shape = (1, 2, 3, size, size)
    assert host_blob.shape == shape
    st = torch.cuda.current_stream().cuda_stream
    eng = Engine.from_bytes(blob, 0, profile=(shape,) * 3)
    try:
        y_host = _run(eng, torch.from_numpy(host_blob).cuda(), shape)
        d_images = torch.full(shape, float("nan"), device="cuda")
        with pre.VggtPreprocess(60, 80, size, frames=2) as vp:
            assert vp.box == box and vp.pad == (10, 10, 0, 0)
            vp.run(frames, d_images.data_ptr(), st)
            y_dev = _run(eng, d_images, shape)
        with pytest.raises(RuntimeError):
            vp.run(frames, d_images.data_ptr(), st)  # freed
    finally:
        eng.destroy()
    assert np.array_equal(d_images.cpu().numpy().view(np.uint32), host_blob.view(np.uint32))
    assert np.isfinite(y_dev).all() and np.array_equal(y_dev, y_host)


def test_driver_image(gpu, tmp_path, capsys):
    from monocular_depth_estimation_trt_amd.models.vggt import run
    frames = frames_60x80()
    np.save(tmp_path / "a.npy", frames[0])
    np.save(tmp_path / "b.npy", frames[1])
    args = ["--source", "synthetic:vggt:tiny", "--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2",
            "--warmup", "1", "--image", str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), "--out-dir",
            str(tmp_path / "bench")]
    d_dev = run.main(args + ["--color", str(tmp_path / "out.npy")])
    d_host = run.main(args + ["--host-preprocess"])
    _, box = pre.square_pad_geometry(60, 80, 98)
    x1, y1, x2, y2 = (int(round(v)) for v in box)
    assert (y2 - y1, x2 - x1) == (74, 98)
    assert d_dev.shape == (2, y2 - y1, x2 - x1) and d_dev.dtype == np.float32 and np.isfinite(d_dev).all()
    assert np.array_equal(d_dev, d_host)
    assert not np.array_equal(d_dev[0], d_dev[1])
    out = capsys.readouterr().out
    assert "[MDET] preprocess (device" in out and "[MDET] preprocess (host" in out and "[MDET] color :" in out
    for i, name in enumerate(("out.npy", "out_1.npy")):
        pic = np.load(tmp_path / name)
        assert pic.shape == (60, 80, 3) and pic.dtype == np.uint8
        small, _ = visualize.colorize_np(d_dev[i], "inverse_auto", map_is_inverse=False, denom_eps=1e-6)
        assert np.array_equal(pic, pre.resize_linear_u8(small, 60, 80))
