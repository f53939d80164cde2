"""The DA-V2 family's native profile on the device (csrc/preprocess_cubic.hip,
resize_cubic_f_norm_kernel) through the C ABI, the Python class, the engine and
the drivers, against the numpy restatement preprocess.resize_cubic_float plus
the float64 standardise -- bit for bit: both evaluate the same IEEE operations
in the same order, none fused, so there is no tolerance.  (What the restatement
itself is held to: tests/test_preprocess_native_cpu.py.)  Every destination is
followed by a guard row that must come back untouched.
"""

import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from gpu_util import op, ptr, stream

from monocular_depth_estimation_trt_amd import _lib, pack, weights
from monocular_depth_estimation_trt_amd import preprocess as pre

pytestmark = pytest.mark.gpu

AC, V2 = "depth_anything_ac", "depth_anything_v2"
IMAGENET = (pre.IMAGENET_MEAN, pre.IMAGENET_STD)
LOPSIDED = ((0.125, 0.5, 0.875), (0.2, 0.45, 0.8))  # a channel mix-up moves every value
# (sh, sw, oh, ow, wide)
SMALL = [(37, 53, 28, 42), (53, 37, 42, 28),
         (9, 5, 56, 28),              # upscale, all four borders clamp
         (28, 42, 28, 42),            # identity
         (300, 400, 56, 70), (300, 400, 42, 56)]
CASES = [s + (wide,) for s in SMALL for wide in (0, 1)] + [(2268, 3024, 518, 700, 0), (768, 1024, 518, 686, 1)]


def case_id(c):
    return "%dx%d-%dx%d-%s" % (c[:4] + ("f64" if c[4] else "f32",))


@functools.lru_cache(maxsize=None)
def source(sh, sw, batch=1, seed=0):
    """[batch][sh][sw][3] seeded noise; cached, never written."""
    rng = np.random.Generator(np.random.PCG64(sh * 10007 + sw + 1000003 * seed))
    a = rng.integers(0, 256, size=(batch, sh, sw, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def lut(wide):
    return pre.scale_lut(V2 if wide else AC)


@functools.lru_cache(maxsize=None)
def expected(sh, sw, oh, ow, wide, batch=1, swap_rb=0, stats=IMAGENET, seed=0):
    """The contract on source(...): [batch][3][oh][ow] float32; cached, never written."""
    T = np.float64 if wide else np.float32
    mean, std = (np.asarray(v, np.float64) for v in stats)
    out = []
    for im in source(sh, sw, batch, seed):
        x = pre.resize_cubic_float((im[:, :, ::-1] if swap_rb else im).astype(T) / 255.0, oh, ow)
        assert x.dtype == T
        out.append(((x - mean) / std).astype(np.float32).transpose(2, 0, 1))
    r = np.ascontiguousarray(np.stack(out))
    r.setflags(write=False)
    return r


def device_native(src_np, sh, sw, pitch, swap_rb, wide, stats, oh, ow):
    """-> (result [B][3][oh][ow], the guard row after it); the destination starts as 0xA5 bytes."""
    B = src_np.shape[0]
    d_src = torch.from_numpy(np.array(src_np)).cuda()  # a writable copy
    d_lut = torch.from_numpy(lut(wide)).cuda()
    d_dst = torch.full((B * 3 * oh + 1, ow * 4), 0xA5, dtype=torch.uint8, device="cuda")
    op("mde_op_resize_cubic_f_norm", ptr(d_src), B, sh, sw, pitch, swap_rb, wide, ptr(d_lut), *stats[0], *stats[1],
       ptr(d_dst), oh, ow, stream())
    out = d_dst.cpu().numpy()
    return out[:B * 3 * oh].view(np.float32).reshape(B, 3, oh, ow), out[B * 3 * oh]


def same_bits(got, ref):
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), bad.size, np.argwhere(bad)[:4].tolist(),
                           float(np.abs(got.astype(np.float64) - ref).max()))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_is_the_restatement_bit_for_bit(gpu, case):
    sh, sw, oh, ow, wide = case
    got, guard = device_native(source(sh, sw), sh, sw, 3 * sw, 0, wide, IMAGENET, oh, ow)
    same_bits(got, expected(sh, sw, oh, ow, wide))
    assert (guard == 0xA5).all()
    again, _ = device_native(source(sh, sw), sh, sw, 3 * sw, 0, wide, IMAGENET, oh, ow)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("swap_rb", [0, 1])
def test_channel_order(gpu, swap_rb, wide):
    """mean / std are in output channel order whatever swap_rb says; a kernel that standardises before
    it swaps, or swaps the statistics with the pixels, differs here."""
    sh, sw, oh, ow = 37, 53, 28, 42
    got, guard = device_native(source(sh, sw), sh, sw, 3 * sw, swap_rb, wide, LOPSIDED, oh, ow)
    ref = expected(sh, sw, oh, ow, wide, swap_rb=swap_rb, stats=LOPSIDED)
    assert not np.array_equal(ref, expected(sh, sw, oh, ow, wide, swap_rb=1 - swap_rb, stats=LOPSIDED))
    assert not np.array_equal(ref, expected(sh, sw, oh, ow, wide, swap_rb=swap_rb,
                                            stats=(LOPSIDED[0][::-1], LOPSIDED[1][::-1])))
    same_bits(got, ref)
    assert (guard == 0xA5).all()


@pytest.mark.parametrize("case", [(37, 53, 28, 42, 0), (9, 5, 56, 28, 1)], ids=case_id)
def test_padded_pitch_batch2(gpu, case):
    """Rows 5 bytes longer than 3*sw, the padding 0xFF: the filler must not reach any tap; two
    different frames."""
    sh, sw, oh, ow, wide = case
    pitch = 3 * sw + 5
    padded = np.full((2, sh, pitch), 0xFF, np.uint8)
    padded[:, :, :3 * sw] = source(sh, sw, 2).reshape(2, sh, 3 * sw)
    got, guard = device_native(padded, sh, sw, pitch, 1, wide, IMAGENET, oh, ow)
    same_bits(got, expected(sh, sw, oh, ow, wide, batch=2, swap_rb=1))
    assert not np.array_equal(got[0], got[1])
    assert (guard == 0xA5).all()


@pytest.mark.parametrize("wide", [0, 1])
def test_one_enqueue_in_a_captured_graph(gpu, wide):
    """mde_op_resize_cubic_f_norm captured into a torch.cuda.graph on a side stream and replayed on a
    changed photo."""
    sh, sw, oh, ow = 53, 37, 42, 28
    a, b = source(sh, sw)[0], source(sh, sw, seed=1)[0]
    d_src = torch.from_numpy(np.array(a)).cuda()
    d_lut = torch.from_numpy(lut(wide)).cuda()
    d_dst = torch.full((3 * oh + 1, ow), float("nan"), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _lib.call("mde_op_resize_cubic_f_norm", C.c_void_p(d_src.data_ptr()), 1, sh, sw, 3 * sw, 1, wide,
                  C.c_void_p(d_lut.data_ptr()), *IMAGENET[0], *IMAGENET[1], C.c_void_p(d_dst.data_ptr()), oh, ow,
                  C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    assert torch.isnan(d_dst).all()  # captured, not run
    for photo, seed in ((a, 0), (b, 1)):
        d_src.copy_(torch.from_numpy(np.array(photo)))
        g.replay()
        torch.cuda.synchronize()
        out = d_dst.cpu().numpy()
        same_bits(out[:3 * oh].reshape(1, 3, oh, ow), expected(sh, sw, oh, ow, wide, swap_rb=1, seed=seed))
        assert np.isnan(out[3 * oh]).all()


def test_argument_errors_leave_dst_untouched(gpu):
    sh, sw, oh, ow = 9, 5, 56, 28
    d_src = torch.from_numpy(np.array(source(sh, sw))).cuda()
    d_lut = torch.from_numpy(lut(0)).cuda()
    d_dst = torch.full((3 * oh, ow * 4), 0xA5, dtype=torch.uint8, device="cuda")
    L = _lib.lib()

    def call(src=d_src, dst=d_dst, table=d_lut, batch=1, sh=sh, sw=sw, pitch=3 * sw, wide=0, std=IMAGENET[1],
             oh=oh, ow=ow):
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        return L.mde_op_resize_cubic_f_norm(p(src), batch, sh, sw, pitch, 1, wide, p(table), *IMAGENET[0], *std,
                                            p(dst), oh, ow, stream())

    for kw in (dict(src=None), dict(dst=None), dict(table=None), dict(batch=0), dict(sh=0), dict(sw=0), dict(oh=0),
               dict(ow=-1), dict(pitch=3 * sw - 1), dict(wide=2), dict(wide=-1), dict(std=(0.0, 0.224, 0.225)),
               dict(std=(0.229, 0.224, 0.0))):
        assert call(**kw) == 1, kw
        assert b"mde_op_resize_cubic_f_norm:" in L.mde_last_error(), (kw, L.mde_last_error())
    torch.cuda.synchronize()
    assert (d_dst.cpu().numpy() == 0xA5).all()
    assert call() == 0  # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    same_bits(d_dst.cpu().numpy().view(np.float32).reshape(1, 3, oh, ow), expected(sh, sw, oh, ow, 0, swap_rb=1))


PORTRAIT = (60, 45, 126)  # photo h, w, target -> 168 x 126 under depth_anything_ac's ceil


@pytest.mark.parametrize("model,photo", [(AC, PORTRAIT), (V2, (300, 400, 42))], ids=["ac-portrait", "v2-landscape"])
def test_fill_binding_in_the_dropin_sequence(gpu, tmp_path, model, photo):
    """allocate_buffers -> NativePreprocess.fill_binding -> do_inference: the binding holds the bytes of
    preprocess_native_host's blob, and the engine's depth is the same fed either way."""
    from monocular_depth_estimation_trt_amd import common
    from monocular_depth_estimation_trt_amd.common_runtime import allocate_buffers, do_inference, free_buffers
    sh, sw, target = photo
    bgr = source(sh, sw)[0]
    want, src_hw = pre.preprocess_native_host(bgr, model, target)
    h, w = pre.native_size(model, sh, sw, target)
    assert src_hw == (sh, sw) and want.shape == (1, 3, h, w)
    assert (h, w) == ((168, 126) if model == AC else (42, 56))
    with common.get_engine("synthetic:vits", str(tmp_path / "e_fp16.mdeng"), "fp16", None,
                           input_hw=(h, w)) as engine, engine.create_execution_context() as ctx:
        inputs, outputs, bindings, st = allocate_buffers(engine, (1, h, w), profile_idx=0)
        inputs[0].host[:] = np.nan  # stale bytes a mis-ordered copy-back would leave
        with pre.NativePreprocess(sh, sw, model, target=target) as npp:
            assert npp.dst == (h, w) and npp.output == "float32_nchw" and npp.wide == (model == V2)
            npp.fill_binding(bgr, inputs[0], st)
        with pytest.raises(RuntimeError):
            npp.run(bgr, inputs[0].device, st)  # freed
        staged = inputs[0].host[:want.size].reshape(want.shape).copy()
        y_dev = do_inference(ctx, engine, bindings, inputs, outputs, st)[0].reshape(1, h, w).copy()
        inputs[0].host = want
        y_host = do_inference(ctx, engine, bindings, inputs, outputs, st)[0].reshape(1, h, w).copy()
        free_buffers(inputs, outputs, st)
    same_bits(staged, want)
    assert np.isfinite(y_dev).all() and np.array_equal(y_dev, y_host)


def test_portrait_engine_vs_oracle(gpu):
    """168x126 (12x9 patches, h > w), fed what the native profile makes of a 60x45 photo: the
    comparison and tolerance of test_gpu_engine.py's 126x182 case."""
    from oracle import dav2_ref
    from test_gpu_engine import check, run_engine
    cfg = weights.model_config("vits", "metric")
    sd = weights.synthetic_state_dict(cfg, 99)
    sh, sw, target = PORTRAIT
    x = np.concatenate([pre.preprocess_native_host(im, AC, target)[0] for im in source(sh, sw, 2)])
    assert x.shape == (2, 3, 168, 126)
    ref = dav2_ref.forward(dav2_ref.to_torch(sd), cfg, x).numpy()
    y = run_engine(pack.pack_bytes(sd, cfg, 168, 126), x)
    assert y.shape == (2, 168, 126)
    check(y, ref, 20.0, "168x126 vs oracle")


def _drive(run, tmp_path, name, photo, target, extra=()):
    np.save(tmp_path / f"{name}.npy", photo)
    return ["--profile", "native", "--native-target", str(target), "--image", str(tmp_path / f"{name}.npy"),
            "--engine", str(tmp_path / f"{name}_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--out-dir",
            str(tmp_path / f"bench_{name}"), *extra]


def _record(tmp_path, name):
    import json
    d = tmp_path / f"bench_{name}"
    files = [f for f in os.listdir(d) if f.endswith(".json")]
    assert len(files) == 1, files
    with open(d / files[0], encoding="utf-8") as f:
        return json.load(f)


@pytest.mark.parametrize("shape", [(60, 45), (45, 60)], ids=["portrait", "landscape"])
def test_driver_depth_anything_ac(gpu, tmp_path, capsys, shape):
    from monocular_depth_estimation_trt_amd.models.depth_anything_ac import run
    sh, sw = shape
    args = _drive(run, tmp_path, "p", source(sh, sw)[0], 126)
    d_dev = run.main(args)
    rec = _record(tmp_path, "p")
    d_host = run.main(args + ["--host-preprocess"])
    ih, iw = pre.native_size(AC, sh, sw, 126)
    assert (ih, iw) == ((168, 126) if sh > sw else (126, 168))
    assert d_dev.shape == (sh, sw) and np.isfinite(d_dev).all() and d_dev.min() >= 1e-3
    assert np.array_equal(d_dev, d_host)
    assert (rec["profile"], rec["input_h"], rec["input_w"]) == ("native", ih, iw)
    out = capsys.readouterr().out
    assert f"[MDET] preprocess (device, H2D + kernel, hipEvents) [native, target 126] {sh}x{sw} -> {ih}x{iw}" in out
    assert f"[MDET] preprocess (host, numpy) [native, target 126] {sh}x{sw} -> {ih}x{iw}" in out


def test_driver_depth_anything_v2_with_color(gpu, tmp_path, capsys):
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    args = _drive(run, tmp_path, "q", source(300, 400)[0], 42)
    d_dev = run.main(args + ["--color", str(tmp_path / "out.npy")])
    rec = _record(tmp_path, "q")
    d_host = run.main(args + ["--host-preprocess"])
    assert d_dev.shape == (300, 400) and np.isfinite(d_dev).all() and d_dev.min() >= 1e-3
    assert np.array_equal(d_dev, d_host)
    assert (rec["profile"], rec["input_h"], rec["input_w"]) == ("native", 42, 56)
    pic = np.load(tmp_path / "out.npy")
    assert pic.shape == (300, 400, 3) and pic.dtype == np.uint8
    out = capsys.readouterr().out
    assert "[native, target 42] 300x400 -> 42x56" in out and "[MDET] color :" in out
