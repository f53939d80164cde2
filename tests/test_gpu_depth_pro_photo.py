"""Depth Pro photo path on the device (csrc/depth_pro_photo.hip) through the C ABI.

What pins what: the kernels are held bit for bit (uint32 views) to the numpy restatements
preprocess.resize_bilinear_f32 / postprocess.depth_pro_postprocess_np -- both sides round
every float32 operation separately, so there is no tolerance -- except where the focal
length comes from fov_deg on the device, whose tanf is the device's own: that branch is held
to the reference's torch arithmetic (postprocess.depth_pro_postprocess) within the
post-process bar derived in tests/test_depth_pro_photo_cpu.py, which also holds the
restatements themselves to torch.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_util import op, ptr, stream

from monocular_depth_estimation_trt_amd import pack_depth_pro, weights_depth_pro as WD
from monocular_depth_estimation_trt_amd import postprocess as post
from monocular_depth_estimation_trt_amd import preprocess as pre
from monocular_depth_estimation_trt_amd.engine import Engine

pytestmark = pytest.mark.gpu

PRE_SHAPES = [(37, 53, 48, 48),
              (9, 5, 28, 28),       # upscale, all four borders
              (96, 128, 48, 48),    # exact 2x reduction, still bilinear
              (100, 76, 64, 64),
              (48, 48, 48, 48),     # identity
              (600, 800, 392, 392)]
POST_SHAPES = [(48, 48, 37, 53),    # ow % 4 != 0: scalar stores and the row tail
               (48, 48, 100, 76),   # ow % 4 == 0: 16-byte stores
               (28, 28, 9, 5),
               (64, 48, 96, 128),
               (48, 48, 48, 48)]
EPS = 2.0 ** -23
SIZE = 1536


def post_bar(ih, iw):
    return 9 * (ih + iw) * EPS + 2.0 ** -20


@functools.lru_cache(maxsize=None)
def photo(sh, sw, batch=1):
    """[batch][sh][sw][3] seeded noise; cached, never written."""
    rng = np.random.Generator(np.random.PCG64(sh * 10007 + sw))
    a = rng.integers(0, 256, size=(batch, sh, sw, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected_pre(sh, sw, oh, ow, batch=1):
    """resize_bilinear_f32(lut[photo]), source channel order, [batch][3][oh][ow]; cached, never written."""
    lut = pre.depth_pro_lut()
    r = np.stack([pre.resize_bilinear_f32(lut[im].transpose(2, 0, 1), oh, ow) for im in photo(sh, sw, batch)])
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def inverse_depth(ih, iw, oh, ow, batch=1):
    rng = np.random.Generator(np.random.PCG64((ih * 131 + iw) * 65537 + oh * 257 + ow))
    a = rng.uniform(0.5, 2.0, size=(batch, ih, iw)).astype(np.float32)
    a.setflags(write=False)
    return a


def device_preprocess(src_np, sh, sw, pitch, swap_rb, oh, ow):
    """-> (result [B][3][oh][ow], the guard row after it)."""
    B = src_np.shape[0]
    d_src = torch.from_numpy(np.array(src_np)).cuda()  # a writable copy
    d_lut = torch.from_numpy(pre.depth_pro_lut()).cuda()
    d_dst = torch.full((B * 3 * oh + 1, ow), float("nan"), dtype=torch.float32, device="cuda")
    op("mde_op_dp_preprocess", ptr(d_src), B, sh, sw, pitch, swap_rb, ptr(d_lut), ptr(d_dst), oh, ow, stream())
    out = d_dst.cpu().numpy()
    return out[:B * 3 * oh].reshape(B, 3, oh, ow), out[B * 3 * oh]


def same_bits(got, ref):
    bad = got.view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32)
    return not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("shape", PRE_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_dp_preprocess_bit_exact(gpu, shape):
    sh, sw, oh, ow = shape
    got, guard = device_preprocess(photo(sh, sw), sh, sw, 3 * sw, 0, oh, ow)
    ok, where = same_bits(got, expected_pre(sh, sw, oh, ow))
    assert ok, where
    assert np.isnan(guard).all()


@pytest.mark.parametrize("swap_rb", [0, 1])
def test_dp_preprocess_batch2_and_swap(gpu, swap_rb):
    sh, sw, oh, ow = 37, 53, 48, 48
    got, guard = device_preprocess(photo(sh, sw, 2), sh, sw, 3 * sw, swap_rb, oh, ow)
    ref = expected_pre(sh, sw, oh, ow, 2)
    ok, where = same_bits(got, ref[:, ::-1] if swap_rb else ref)
    assert ok, where
    assert not np.array_equal(got[0], got[1])
    assert np.isnan(guard).all()


def test_dp_preprocess_padded_pitch(gpu):
    """Rows 5 bytes longer than 3*sw, the padding 0xFF: it must not leak into any tap."""
    sh, sw, oh, ow = 9, 5, 28, 28
    pitch = 3 * sw + 5
    padded = np.full((2, sh, pitch), 0xFF, np.uint8)
    padded[:, :, :3 * sw] = photo(sh, sw, 2).reshape(2, sh, 3 * sw)
    got, guard = device_preprocess(padded, sh, sw, pitch, 0, oh, ow)
    ok, where = same_bits(got, expected_pre(sh, sw, oh, ow, 2))
    assert ok, where
    assert np.isnan(guard).all()


def device_postprocess(inv_np, oh, ow, fov=None, f_px=0.0, offset=0):
    """-> (depth [B][oh][ow], the guard row after it, the floats before it, f_px_out [B]);
    `offset` floats are skipped at the start of the output allocation."""
    B, ih, iw = inv_np.shape
    d_inv = torch.from_numpy(np.array(inv_np)).cuda()
    d_fov = None if fov is None else torch.from_numpy(np.asarray(fov, np.float32)).cuda()
    d_f = torch.full((B + 1,), float("nan"), dtype=torch.float32, device="cuda")
    d_out = torch.full((offset + (B * oh + 1) * ow,), float("nan"), dtype=torch.float32, device="cuda")
    assert d_out.data_ptr() % 16 == 0
    op("mde_op_dp_postprocess", ptr(d_inv), B, ih, iw, ptr(d_fov), float(f_px), ptr(d_f),
       C.c_void_p(d_out.data_ptr() + 4 * offset), oh, ow, stream())
    out, f = d_out.cpu().numpy(), d_f.cpu().numpy()
    assert np.isnan(f[B])
    body = out[offset:offset + B * oh * ow].reshape(B, oh, ow)
    return body, out[offset + B * oh * ow:], out[:offset], f[:B]


@pytest.mark.parametrize("shape", POST_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_dp_postprocess_f_px_bit_exact(gpu, shape):
    ih, iw, oh, ow = shape
    inv = inverse_depth(*shape)
    f_px = float(np.float32(0.8 * ow + 0.37))
    got, guard, _, f = device_postprocess(inv, oh, ow, f_px=f_px)
    ref, f_ref = post.depth_pro_postprocess_np(inv, None, (oh, ow), f_px=f_px)
    ok, where = same_bits(got, ref)
    assert ok, where
    assert np.isnan(guard).all() and f[0] == f_ref[0] == np.float32(f_px)


@pytest.mark.parametrize("shape", [(48, 48, 37, 53), (48, 48, 100, 76)], ids=lambda s: "%dx%d-%dx%d" % s)
def test_dp_postprocess_batch2(gpu, shape):
    ih, iw, oh, ow = shape
    inv = inverse_depth(*shape, batch=2)
    got, guard, _, f = device_postprocess(inv, oh, ow, f_px=61.5)
    ref, _ = post.depth_pro_postprocess_np(inv, None, (oh, ow), f_px=61.5)
    ok, where = same_bits(got, ref)
    assert ok, where
    assert not np.array_equal(got[0], got[1])
    assert np.isnan(guard).all() and (f == np.float32(61.5)).all()


def test_dp_postprocess_unaligned_output(gpu):
    """ow % 4 == 0 but the map starts one float past a 16-byte boundary: scalar stores, and the
    float before the map stays untouched."""
    shape = (48, 48, 100, 76)
    ih, iw, oh, ow = shape
    inv = inverse_depth(*shape, batch=2)
    got, guard, before, _ = device_postprocess(inv, oh, ow, f_px=61.5, offset=1)
    ref, _ = post.depth_pro_postprocess_np(inv, None, (oh, ow), f_px=61.5)
    ok, where = same_bits(got, ref)
    assert ok, where
    assert np.isnan(guard).all() and np.isnan(before).all()


@pytest.mark.parametrize("value, depth", [(1e-6, 1e4), (1e6, 1e-4)])
def test_dp_postprocess_clamps(gpu, value, depth):
    ih, iw, oh, ow = 48, 48, 37, 53
    inv = np.full((1, ih, iw), value, np.float32)
    got, guard, _, _ = device_postprocess(inv, oh, ow, f_px=float(ow))
    assert np.array_equal(got, np.full((1, oh, ow), np.float32(1) / np.float32(1.0 / depth), np.float32))
    assert np.isnan(guard).all()


@pytest.mark.parametrize("shape", [(48, 48, 37, 53), (48, 48, 100, 76)], ids=lambda s: "%dx%d-%dx%d" % s)
def test_dp_postprocess_keeps_nan(gpu, shape):
    """A NaN tap stays NaN through the clamp (torch.clamp's behaviour, the restatement's too): the
    same pixels are NaN on the device as in the restatement, the others are bit-identical."""
    ih, iw, oh, ow = shape
    inv = np.array(inverse_depth(*shape))
    inv[0, 10, 17] = np.nan
    got, guard, _, _ = device_postprocess(inv, oh, ow, f_px=61.5)
    ref, _ = post.depth_pro_postprocess_np(inv, None, (oh, ow), f_px=61.5)
    nan = np.isnan(ref)
    assert nan.any() and not nan.all() and np.array_equal(np.isnan(got), nan)
    ok, where = same_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), ref))
    assert ok, where
    assert np.isnan(guard).all()


@pytest.mark.parametrize("shape", [(48, 48, 37, 53), (48, 48, 100, 76)], ids=lambda s: "%dx%d-%dx%d" % s)
def test_dp_postprocess_fov_on_device(gpu, shape):
    """Two images, two FOVs, the focal length computed on the device (its own tanf): against the
    reference's torch statement per image, and f_px_out against torch's focal length."""
    ih, iw, oh, ow = shape
    inv = inverse_depth(*shape, batch=2)
    fov = np.array([27.5, 81.25], np.float32)
    got, guard, _, f = device_postprocess(inv, oh, ow, fov=fov)
    assert np.isnan(guard).all()
    for b in range(2):
        ref, f_ref = post.depth_pro_postprocess(np.array(inv[b]), fov[b:b + 1], (oh, ow))  # a writable copy
        f_err = abs(float(f[b]) - f_ref) / abs(f_ref)
        err = float((np.abs(got[b].astype(np.float64) - ref) / np.abs(ref)).max())
        print(f"fov {fov[b]} {shape}: f_px {f[b]} vs {f_ref} (rel {f_err:.3e}, bar {4 * EPS:.3e}); "
              f"depth max rel {err:.3e} (bar {post_bar(ih, iw):.3e})")
        assert f_err <= 4 * EPS, (float(f[b]), f_ref)
        assert err <= post_bar(ih, iw), (err, post_bar(ih, iw))
    assert f[0] != f[1] and not np.array_equal(got[0], got[1])


@pytest.fixture(scope="module")
def tiny_blob(gpu):
    cfg = WD.depth_pro_config("tiny")
    return pack_depth_pro.pack_bytes(WD.synthetic_state_dict(cfg, 4321), cfg)


def test_device_preprocess_into_engine(tiny_blob):
    """(300, 400) BGR photo -> DepthProPreprocess -> the synthetic tiny Depth Pro engine (1536^2),
    against the same engine fed the host-side pre-process; then the drop-in sequence
    allocate_buffers -> fill_binding -> do_inference."""
    from monocular_depth_estimation_trt_amd.common_runtime import (allocate_buffers, do_inference, free_buffers,
                                                                   hip_call, stream_synchronize)
    bgr = photo(300, 400)[0]
    want, src_hw = pre.preprocess_depth_pro_host(bgr, SIZE)
    assert src_hw == (300, 400) and want.shape == (1, 3, SIZE, SIZE)
    with Engine.from_bytes(tiny_blob, 0) as engine, engine.create_execution_context() as ctx:
        inputs, outputs, bindings, st = allocate_buffers(engine)
        try:
            assert len(inputs) == 1 and len(outputs) == 2

            def infer():
                return [o.copy() for o in do_inference(ctx, engine, bindings, inputs, outputs, st)]

            inputs[0].host = want
            y_host = infer()
            # the binding filled on the device, the engine run on that stream without an upload
            inputs[0].host[:] = np.nan
            with pre.DepthProPreprocess(300, 400, SIZE) as dp:
                dp.run(bgr, inputs[0].device, st)
                for i in range(engine.num_io_tensors):
                    ctx.set_tensor_address(engine.get_tensor_name(i), bindings[i])
                ctx.execute_async_v3(stream_handle=st)
                filled = np.empty_like(want)
                y_dev = [np.empty_like(o.host) for o in outputs]
                for dst, src, n in [(filled, inputs[0].device, want.nbytes)] + \
                        [(y, o.device, o.nbytes) for y, o in zip(y_dev, outputs)]:
                    hip_call("mde_rt_memcpy_dtoh_async", dst.ctypes.data_as(C.c_void_p), C.c_void_p(src), n,
                             C.c_void_p(st))
                stream_synchronize(st)
                # the documented sequence: do_inference's own upload carries the same bytes
                dp.fill_binding(bgr, inputs[0], st)
                staged = inputs[0].host[:want.size].reshape(want.shape).copy()
                y_fill = infer()
            with pytest.raises(RuntimeError):
                dp.run(bgr, inputs[0].device, st)  # freed
        finally:
            free_buffers(inputs, outputs, st)
    ok, where = same_bits(filled, want)
    assert ok, where
    ok, where = same_bits(staged, want)
    assert ok, where
    for a, b, c in zip(y_host, y_dev, y_fill):
        assert np.isfinite(a).all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.fixture(scope="module")
def driver(gpu, tmp_path_factory):
    """run.main on a 300x400 photo with extra flags -> ((depth, f_px), stdout); the packed engine is
    built by the first call and reloaded by the others."""
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    td = tmp_path_factory.mktemp("dp_photo")
    np.save(td / "src.npy", photo(300, 400)[0])
    args = ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(td / "e_fp16.mdeng"), "--iterations", "2",
            "--warmup", "1", "--image", str(td / "src.npy"), "--out-dir", str(td / "bench")]
    results = {}

    def call(*extra):
        if extra not in results:
            results[extra] = run.main(args + list(extra))
        return results[extra]

    return call


def test_driver_image(driver, capsys):
    depth, f_px = driver()
    out = capsys.readouterr().out
    assert depth.shape == (300, 400) and depth.dtype == np.float32 and np.isfinite(depth).all()
    assert depth.min() >= np.float32(1e-4) and depth.max() <= np.float32(1e4)
    assert np.isfinite(f_px) and f_px > 0
    assert "[MDET] preprocess (device" in out and "[MDET] postprocess (device" in out


def test_driver_host_preprocess_is_bit_identical(driver, capsys):
    depth, f_px = driver()
    d_host, f_host = driver("--host-preprocess")
    out = capsys.readouterr().out
    assert np.array_equal(depth.view(np.uint32), d_host.view(np.uint32)) and f_px == f_host
    assert "[MDET] preprocess (host" in out and "[MDET] postprocess (device" in out


def test_driver_host_postprocess_within_the_bar(driver, capsys):
    depth, f_px = driver()
    d_host, f_host = driver("--host-postprocess")
    out = capsys.readouterr().out
    assert d_host.shape == (300, 400)
    err = float((np.abs(depth.astype(np.float64) - d_host) / np.abs(d_host)).max())
    print(f"driver: device vs torch post-process, max rel {err:.3e} (bar {post_bar(SIZE, SIZE):.3e}); "
          f"f_px {f_px} vs {f_host}")
    assert err <= post_bar(SIZE, SIZE), (err, post_bar(SIZE, SIZE))
    assert abs(f_px - f_host) <= 4 * EPS * abs(f_host)
    assert "[MDET] preprocess (device" in out and "[MDET] postprocess (host" in out


def test_driver_f_px(driver):
    depth, f_px = driver("--f-px", "500")
    assert f_px == 500.0 and depth.shape == (300, 400) and np.isfinite(depth).all()
    assert not np.array_equal(depth, driver()[0])
