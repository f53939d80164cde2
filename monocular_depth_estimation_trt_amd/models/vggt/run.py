"""VGGT (depth only) on MI355X -- the counterpart of the reference driver
`models/vggt/onnx2trt.py:main` (:56-148), same sequence:

  photos -> pad to a square with white, one cubic resize on uint8, /255 ->
  images [1, S, 3, 518, 518] in [0, 1] -> get_engine -> create_execution_context
  -> allocate_buffers -> bench.measure(do_inference) (20 warmup / 100
  iterations) -> depth [S, 518, 518] -> crop to the content box
  (onnx2trt.py:131) -> bench.record -> turbo picture at the photo's size

    python -m monocular_depth_estimation_trt_amd.models.vggt.run \
        [--source synthetic:vggt:vggt_1b:2468 | model.pt | model.safetensors]
        [--image a.npy|a.jpg [b.npy ...]] [--host-preprocess] [--color out.png [--color-range VMIN VMAX | --color-robust [LO HI]] [--color-robust-near]]
        [--input x.npy] [--frames S] [--box x1 y1 x2 y2]

`--image` is S source-resolution BGR photos of one size -- .npy files holding
a uint8 [H,W,3] BGR array each (one .npy may hold all of them, [S,H,W,3]), or
image files if Pillow is installed.  They go through the reference's
core/preprocess.py:resize_square_pad (BGR->RGB, white border to a square, cv2
INTER_CUBIC on uint8, /255) on the device, straight into the engine's "images"
binding (preprocess.VggtPreprocess; `--host-preprocess`: the numpy statement
of the same arithmetic and the usual upload).  S sets the frame count, the
network size is the source's own (518 for a checkpoint, the preset's for a
synthetic source), and the content box is computed, not passed.  The depth maps
are cropped to int(round(.)) of that box on the device (mde_op_crop_f32) while
they are still in the engine's output binding; [S, ch, cw] comes back.

`--color PATH` is the reference driver's closing picture (onnx2trt.py:122-142):
the cropped map's inverse depth clipped to [1/250, 10] (its `+ 1e-6`
denominator), turbo-coloured, BGR, resized to the photo's size with cv2's
INTER_LINEAR -- all on the device (visualize.DeviceColorize, mde_op_resize_u8);
the picture is downloaded once.  Frame i > 0 goes to PATH with `_<i>` before
the extension.  `--color-range VMIN VMAX` draws depth on that fixed axis
instead.  One `[MDET] color : ...` line per frame is printed.

`--input` is a float32 [1, S, 3, 518, 518] array already square-padded,
resized and divided by 255; without it and without `--image` synthetic frames
are used.  `--box` is the content box of such an input (default: the whole
map); the crop is then a host slice.
"""

import argparse
import ctypes as C
import os
import time

import numpy as np

from monocular_depth_estimation_trt_amd import bench, common, spec, visualize, weights_vggt
from monocular_depth_estimation_trt_amd.common_runtime import (EventPair, HostDeviceMem, allocate_buffers, do_inference,
                                                               free_buffers, hip_call, stream_synchronize)
from monocular_depth_estimation_trt_amd.preprocess import (VggtPreprocess, box_window, crop_f32, load_image_bgr,
                                                           preprocess_vggt_host)

HERE = os.path.dirname(os.path.abspath(__file__))


def build_parser(model="vggt", s=None):
    s = s or spec.load(model)
    ap = argparse.ArgumentParser(prog=model)
    ap.add_argument("--source", default="synthetic:vggt:vggt_1b:2468")
    ap.add_argument("--frames", type=int, default=int(s.get("frames", 1)))
    ap.add_argument("--engine", default="")
    ap.add_argument("--input", default="")
    ap.add_argument("--image", default=[], nargs="+", metavar="PATH",
                    help="S source-resolution BGR photos of one size: .npy (uint8 [H,W,3], or one [S,H,W,3]) or "
                         "image files")
    ap.add_argument("--host-preprocess", action="store_true",
                    help="with --image: pre-process on the host (numpy) and upload, instead of on the device")
    ap.add_argument("--box", type=float, nargs=4, default=None)
    visualize.add_color_arguments(ap)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(os.getcwd(), "reports", "bench"))
    return ap


def network_size(source: str, spec_size: int) -> int:
    """The size a VGGT engine of `source` is packed at: a synthetic preset's
    own grid (`synthetic:vggt:tiny` is 98), else the spec's."""
    if common.is_vggt_source(source) and len(source.split(":")) > 2:
        return int(weights_vggt.vggt_config(source.split(":")[2])["img"])
    return spec_size


def load_frames(paths) -> np.ndarray:
    """uint8 [S, H, W, 3] BGR from --image's paths."""
    if len(paths) == 1 and paths[0].lower().endswith(".npy"):
        a = np.load(paths[0], allow_pickle=False)
        if a.ndim == 4:
            if a.dtype != np.uint8 or a.shape[3] != 3 or a.shape[0] < 1:
                raise ValueError(f"{paths[0]}: expected uint8 [S, H, W, 3] BGR frames, got {a.dtype} {a.shape}")
            return np.ascontiguousarray(a)
    frames = [load_image_bgr(p) for p in paths]
    if any(f.shape != frames[0].shape for f in frames):
        raise SystemExit(f"--image: the photos must have one size, got {[f.shape[:2] for f in frames]}")
    return np.stack(frames)


def _device_preprocess(frames, size, mem, stream):
    """VggtPreprocess into the engine's "images" binding `mem.device`, timed
    with hipEvents (H2D of the frames + the kernel); the pinned side of the
    binding gets the same bytes back, so the timed loop's upload is a no-op in
    value.  Returns (ms, box)."""
    with VggtPreprocess(frames.shape[1], frames.shape[2], size, frames=frames.shape[0]) as pre, \
            EventPair(stream) as ev:
        pre.run(frames, mem.device, stream)
        ev.stop()
        hip_call("mde_rt_memcpy_dtoh_async", mem.host.ctypes.data_as(C.c_void_p), C.c_void_p(mem.device),
                 mem.nbytes, C.c_void_p(stream))
        stream_synchronize(stream)
        return ev.ms(), pre.box


def _frame_path(path: str, i: int) -> str:
    root, ext = os.path.splitext(path)
    return path if i == 0 else f"{root}_{i}{ext}"


def _device_crop(a, s, d_depth, frames, size, box, photo_hw, stream):
    """The engine's depth [frames][size][size] at `d_depth` cropped to the
    rounded box on the device and downloaded; with --color each cropped map is
    coloured and resized to the photo's size while it is still there."""
    y0, x0, ch, cw = box_window(box)
    mem = HostDeviceMem(frames * ch * cw, np.float32)
    try:
        crop_f32(d_depth, frames, size, size, y0, x0, ch, cw, mem.device, stream)
        hip_call("mde_rt_memcpy_dtoh_async", mem.host.ctypes.data_as(C.c_void_p), C.c_void_p(mem.device), mem.nbytes,
                 C.c_void_p(stream))
        stream_synchronize(stream)
        depth = mem.host.reshape(frames, ch, cw).copy()
        if a.color:
            path = a.color
            # --color-robust: all views share one axis, pooled over the cropped maps
            shared = visualize.pooled_range(a, s, mem.device, frames, (ch, cw), stream) if frames > 1 else None
            try:
                for i in range(frames):
                    a.color = _frame_path(path, i)
                    visualize.driver_color(a, s, mem.device + 4 * i * ch * cw, (ch, cw), stream, resize_hw=photo_hw,
                                           denom_eps=1e-6, shared=shared)
            finally:
                a.color = path
                if shared is not None:
                    shared[0].free()
    finally:
        mem.free()
    return depth


def main(argv=None, model="vggt"):
    s = spec.load(model)
    a = build_parser(model, s).parse_args(argv)
    size = network_size(a.source, spec.size_of(s)[0])
    if a.image and (a.input or a.box):
        raise SystemExit("--image computes its own input and box: do not combine it with --input or --box")
    if a.host_preprocess and not a.image:
        raise SystemExit("--host-preprocess needs --image")
    if a.color and not a.image:
        raise SystemExit("--color draws the map cropped to the photo's content box at the photo's size: it needs "
                         "--image")
    visualize.check_color_arguments(a, device_map=True)
    photos = load_frames(a.image) if a.image else None
    box = a.box
    if photos is not None and a.host_preprocess:
        t0 = time.perf_counter()
        x, box = preprocess_vggt_host(photos, size)
        print(f"[MDET] preprocess (host, numpy) {photos.shape[0]} x {photos.shape[1]}x{photos.shape[2]} -> "
              f"{size}x{size} : {(time.perf_counter() - t0) * 1e3:0.3f} ms")
    elif photos is not None:
        x = None  # filled on the device, below
    else:
        x = (np.load(a.input, allow_pickle=False).astype(np.float32) if a.input
             else weights_vggt.synthetic_images(1, a.frames, size, first_seed=0))
        if x.ndim != 5 or x.shape[0] != 1 or x.shape[2:] != (3, size, size):
            raise ValueError(f"[MDET] input must be [1, S, 3, {size}, {size}], got {x.shape}")
    frames = photos.shape[0] if photos is not None else x.shape[1]
    engine_path = a.engine or os.path.join(HERE, "engine", f"vggt_only_depth_{size}x{size}_s{frames}_fp16.mdeng")
    with common.get_engine(a.source, engine_path, "fp16", None, input_hw=(size, size), frames=frames) as engine, \
            engine.create_execution_context() as context:
        inputs, outputs, bindings, stream = allocate_buffers(engine)
        if x is None:
            ms, box = _device_preprocess(photos, size, inputs[0], stream)
            print(f"[MDET] preprocess (device, H2D + kernel, hipEvents) {frames} x {photos.shape[1]}x"
                  f"{photos.shape[2]} -> {size}x{size} : {ms:0.3f} ms")
            x = inputs[0].host[:frames * 3 * size * size].reshape(1, frames, 3, size, size).copy()
        else:
            inputs[0].host = x
        outs, samples = bench.measure(
            lambda: do_inference(context, engine=engine, bindings=bindings, inputs=inputs, outputs=outputs,
                                 stream=stream), warmup=a.warmup, iterations=a.iterations)
        depth = outs[0].reshape(frames, size, size).copy()
        bench.record(model, samples, encoder="fixed", warmup=a.warmup, precision="fp16", profile="bench",
                     input_h=size, input_w=size, engine_path=engine_path, outputs={"depth": depth},
                     notes=f"source={a.source}; frames={frames}", model_input=x, out_dir=a.out_dir)
        if photos is not None:  # the engine's depth is still in outputs[0].device
            depth = _device_crop(a, s, outputs[0].device, frames, size, box, photos.shape[1:3], stream)
        free_buffers(inputs, outputs, stream)
    if photos is None and box:
        x1, y1, x2, y2 = box
        depth = depth[:, int(round(y1)):int(round(y2)), int(round(x1)):int(round(x2))]
    print(f"[MDET] max : {depth.max():0.5f} , min : {depth.min():0.5f}")
    return depth


if __name__ == "__main__":
    main()
