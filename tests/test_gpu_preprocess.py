"""Device preprocess (csrc/preprocess.hip) through the C ABI, against the numpy
restatement preprocess.resize_linear_u8 -- bit for bit: both are integer
arithmetic over coefficients rounded the same way, so there is no tolerance.
(What the restatement itself is held to: tests/test_preprocess_cpu.py.)
"""

import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from gpu_util import op, ptr, stream

from monocular_depth_estimation_trt_amd import pack
from monocular_depth_estimation_trt_amd import preprocess as pre
from monocular_depth_estimation_trt_amd.engine import Engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SHAPES = [(37, 53, 28, 42),
          (9, 5, 28, 14),       # upscale, all four borders
          (56, 84, 28, 42),     # the 2x path
          (56, 53, 28, 42),     # 2x on one axis only
          (28, 42, 28, 42),
          (600, 800, 392, 518),
          (2268, 3024, 518, 518)]


@functools.lru_cache(maxsize=None)
def source(sh, sw, batch=1):
    """[batch][sh][sw][3] seeded noise; cached, never written."""
    rng = np.random.Generator(np.random.PCG64(sh * 10007 + sw))
    a = rng.integers(0, 256, size=(batch, sh, sw, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(sh, sw, oh, ow, batch=1):
    """resize_linear_u8 of source(...), source channel order; cached, never written."""
    r = np.stack([pre.resize_linear_u8(im, oh, ow) for im in source(sh, sw, batch)])
    r.setflags(write=False)
    return r


def device_resize_u8(src_np, sh, sw, pitch, swap_rb, oh, ow):
    """-> (result [B][oh][ow][3], the guard row after it)."""
    B = src_np.shape[0]
    d_src = torch.from_numpy(np.array(src_np)).cuda()  # a writable copy
    d_dst = torch.full((B * oh + 1, ow, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    op("mde_op_resize_u8", ptr(d_src), B, sh, sw, pitch, swap_rb, ptr(d_dst), oh, ow, stream())
    out = d_dst.cpu().numpy()
    return out[:B * oh].reshape(B, oh, ow, 3), out[B * oh]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_resize_u8_bit_exact(gpu, shape):
    sh, sw, oh, ow = shape
    got, guard = device_resize_u8(source(sh, sw), sh, sw, 3 * sw, 0, oh, ow)
    ref = expected(sh, sw, oh, ow)
    bad = got != ref
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (guard == SENTINEL).all()


@pytest.mark.parametrize("swap_rb", [0, 1])
def test_resize_u8_batch2_and_swap(gpu, swap_rb):
    sh, sw, oh, ow = 37, 53, 28, 42
    got, guard = device_resize_u8(source(sh, sw, 2), sh, sw, 3 * sw, swap_rb, oh, ow)
    ref = expected(sh, sw, oh, ow, 2)
    assert np.array_equal(got, ref[..., ::-1] if swap_rb else ref)
    assert not np.array_equal(got[0], got[1])
    assert (guard == SENTINEL).all()


def test_resize_u8_padded_pitch(gpu):
    """Rows 5 bytes longer than 3*sw, the padding 0xFF: it must not leak into any tap."""
    sh, sw, oh, ow = 9, 5, 28, 14
    pitch = 3 * sw + 5
    padded = np.full((2, sh, pitch), 0xFF, np.uint8)
    padded[:, :, :3 * sw] = source(sh, sw, 2).reshape(2, sh, 3 * sw)
    got, guard = device_resize_u8(padded, sh, sw, pitch, 0, oh, ow)
    assert np.array_equal(got, expected(sh, sw, oh, ow, 2))
    assert (guard == SENTINEL).all()


@pytest.mark.parametrize("shape", [(37, 53, 28, 42), (600, 800, 392, 518)], ids=lambda s: "%dx%d-%dx%d" % s)
@pytest.mark.parametrize("model", ["depth_anything_v2", "depth_anything_ac"])
def test_resize_u8_norm_bit_exact(gpu, shape, model):
    sh, sw, oh, ow = shape
    lut = pre.normalize_lut(model)
    rgb = expected(sh, sw, oh, ow)[..., ::-1]  # swap_rb = 1 below
    ref = np.stack([lut[c][rgb[..., c]] for c in range(3)], axis=1)  # [1][3][oh][ow]
    d_src = torch.from_numpy(source(sh, sw).copy()).cuda()
    d_lut = torch.from_numpy(lut).cuda()
    d_dst = torch.full((3 * oh + 1, ow), float("nan"), dtype=torch.float32, device="cuda")
    op("mde_op_resize_u8_norm", ptr(d_src), 1, sh, sw, 3 * sw, 1, ptr(d_lut), ptr(d_dst), oh, ow, stream())
    out = d_dst.cpu().numpy()
    assert np.array_equal(out[:3 * oh].reshape(1, 3, oh, ow).view(np.uint32), ref.view(np.uint32))
    assert np.isnan(out[3 * oh]).all()


def _run(eng, d_in, shape):
    """The engine on an input already on the device (current torch stream)."""
    ctx = eng.create_execution_context()
    H, W = eng.input_hw
    out = torch.empty(shape[0], H, W, device="cuda")
    ctx.set_input_shape(eng.input_name, shape)
    ctx.set_tensor_address(eng.input_name, d_in.data_ptr())
    ctx.set_tensor_address("output", out.data_ptr())
    ctx.execute_async_v3(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    ctx.destroy()
    return y


def test_device_preprocess_into_engine(gpu):
    """(300,400) BGR frame -> DevicePreprocess -> synthetic 98x98 ViT-S engine, float and uint8
    bindings, against the same engines fed the host-side preprocess."""
    h = w = 98
    bgr = source(300, 400)[0]
    st = torch.cuda.current_stream().cuda_stream
    blob_f, _ = pack.synthetic_blob("vits", "metric", h, w)
    blob_u, _ = pack.synthetic_blob("vits", "metric", h, w, input_format="uint8_nhwc")
    prof_f = ((1, 3, h, w),) * 3
    prof_u = ((1, h, w, 3),) * 3
    with Engine.from_bytes(blob_f, 0, profile=prof_f) as ef, Engine.from_bytes(blob_u, 0, profile=prof_u) as eu:
        host_blob, src_hw = pre.preprocess_host(bgr, "depth_anything_v2", (h, w))
        assert src_hw == (300, 400)
        y_host_f = _run(ef, torch.from_numpy(host_blob).cuda(), (1, 3, h, w))
        host_u8 = pre.resize_linear_u8(bgr[:, :, ::-1], h, w)[None]
        y_host_u = _run(eu, torch.from_numpy(np.ascontiguousarray(host_u8)).cuda(), (1, h, w, 3))

        d_f = torch.full((1, 3, h, w), float("nan"), device="cuda")
        with pre.DevicePreprocess(300, 400, h, w, "depth_anything_v2") as dp:
            dp.run(bgr, d_f.data_ptr(), st)
            y_dev_f = _run(ef, d_f, (1, 3, h, w))
        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), host_blob.view(np.uint32))

        d_u = torch.full((1, h, w, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        with pre.DevicePreprocess(300, 400, h, w, "depth_anything_v2", output="uint8_nhwc") as dp:
            dp.run(bgr, d_u.data_ptr(), st)
            y_dev_u = _run(eu, d_u, (1, h, w, 3))
            # frames already on the device, RGB order: no swap
            d_rgb = torch.from_numpy(np.ascontiguousarray(bgr[:, :, ::-1])).cuda()
            d_u2 = torch.empty_like(d_u)
            dp.run_device(d_rgb.data_ptr(), 3 * 400, d_u2.data_ptr(), st, swap_rb=False)
            torch.cuda.synchronize()
        assert np.array_equal(d_u.cpu().numpy(), host_u8) and np.array_equal(d_u2.cpu().numpy(), host_u8)
        with pytest.raises(RuntimeError):
            dp.run(bgr, d_u.data_ptr(), st)  # freed
    assert np.isfinite(y_dev_f).all() and np.isfinite(y_dev_u).all()
    assert np.array_equal(y_dev_f, y_host_f)
    assert np.array_equal(y_dev_u, y_host_u)


@pytest.mark.parametrize("input_format", ["float32_nchw", "uint8_nhwc"])
def test_fill_binding_in_the_dropin_sequence(gpu, input_format):
    """allocate_buffers (its stream is non-blocking) -> fill_binding ->
    do_inference, whose own upload of inputs[0].host must carry the preprocessed bytes."""
    from monocular_depth_estimation_trt_amd import common
    from monocular_depth_estimation_trt_amd.common_runtime import allocate_buffers, do_inference, free_buffers
    h = w = 98
    bgr = source(300, 400)[0]
    u8 = input_format == "uint8_nhwc"
    want = (pre.resize_linear_u8(bgr[:, :, ::-1], h, w)[None] if u8
            else pre.preprocess_host(bgr, "depth_anything_v2", (h, w))[0])
    with tempfile.TemporaryDirectory() as td:
        with common.get_engine("synthetic:vits", os.path.join(td, "e_fp16.mdeng"), "fp16", None, input_hw=(h, w),
                               input_format=input_format) as engine, engine.create_execution_context() as ctx:
            inputs, outputs, bindings, st = allocate_buffers(engine, (1, h, w), profile_idx=0)
            inputs[0].host[:] = 0xEE if u8 else np.nan  # stale bytes a mis-ordered copy-back would leave
            with pre.DevicePreprocess(300, 400, h, w, "depth_anything_v2", output=input_format) as dp:
                dp.fill_binding(bgr, inputs[0], st)
            staged = inputs[0].host[:want.size].reshape(want.shape).copy()
            y_dev = do_inference(ctx, engine, bindings, inputs, outputs, st)[0].reshape(1, h, w).copy()
            inputs[0].host = want
            y_host = do_inference(ctx, engine, bindings, inputs, outputs, st)[0].reshape(1, h, w).copy()
            free_buffers(inputs, outputs, st)
    assert np.array_equal(staged.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
    assert np.isfinite(y_dev).all() and np.array_equal(y_dev, y_host)


def test_driver_image(gpu, capsys):
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    with tempfile.TemporaryDirectory() as td:
        np.save(os.path.join(td, "src.npy"), source(300, 400)[0])
        args = ["--engine", os.path.join(td, "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1",
                "--image", os.path.join(td, "src.npy"), "--out-dir", os.path.join(td, "bench")]
        d_dev = run.main(args)
        d_host = run.main(args + ["--host-preprocess"])
    assert d_dev.shape == (300, 400) and np.isfinite(d_dev).all() and d_dev.min() >= 1e-3
    assert np.array_equal(d_dev, d_host)
    out = capsys.readouterr().out
    assert "[MDET] preprocess (device" in out and "[MDET] preprocess (host" in out
