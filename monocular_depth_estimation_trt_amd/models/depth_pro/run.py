"""Depth Pro on MI355X -- the counterpart of the reference driver
`models/depth_pro/onnx2trt.py:main` (:42-125), same sequence:

  photo (normalised to [-1, 1], resized to 1536^2 with torch bilinear,
  align_corners=False) -> get_engine -> create_execution_context ->
  allocate_buffers -> bench.measure(do_inference) (20 warmup / 100
  iterations) -> post-process outside the timed loop (focal length from the
  predicted FOV, inverse depth * W / f_px, resize back to the source size,
  depth = 1 / clamp(inv, 1e-4, 1e4)) -> bench.record

    python -m monocular_depth_estimation_trt_amd.models.depth_pro.run \
        [--source synthetic:depth_pro | DepthPro.safetensors] [--image photo.npy|photo.jpg]
        [--input x.npy] [--src-hw H W] [--f-px F] [--host-preprocess] [--host-postprocess]
        [--ply out.ply] [--ply-step N] [--ply-edge-rtol R]
        [--mesh out.ply [--mesh-step N] [--edge-rtol R] [--edge-atol A]]
        [--cloud-view out.png [--cloud-view-size H W] [--cloud-view-angles ELEV AZIM] [--cloud-view-step N]]
        [--gt depth.npy --gt-mask mask.npy [--max-depth M] [--gt-out PATH.json]]
        [--color out.png [--color-range VMIN VMAX | --color-robust [LO HI]] [--color-robust-near]]

`--image` is a source-resolution BGR photo -- a .npy holding a uint8 [H,W,3]
BGR array, or an image file if Pillow is installed.  It is normalised and
resized on the device straight into the engine's input binding
(preprocess.DepthProPreprocess; `--host-preprocess`: the numpy statement of the
same arithmetic and the usual upload), and `--src-hw` defaults to its size.
`--input` is a float32 NCHW [1,3,H,W] image already normalised to [-1, 1]; it
is resized to 1536^2 on the host with torch like the reference does.  Without
either a synthetic 1536^2 image is used.

The post-process reads the engine's output bindings in place on the driver's
stream (postprocess.DepthProDevicePostprocess) and downloads the metric depth
at the source size; `--host-postprocess` downloads the 1536^2 map and runs the
reference's torch-CPU version.  `--f-px` is the reference's f_px0: a known
focal length in pixels instead of the predicted one.

`--ply`, `--mesh` and `--cloud-view` are pointcloud.py's one stage for the
cloud outputs, described there.  Here they run on the depth map and the focal
length the device post-process left on the device (`--f-px` instead, when
given), drop depths outside [1e-4, 1e4] and take their colours from the
`--image` photo (no colours with `--input` or the synthetic image); none of
them goes with `--host-postprocess`.

`--gt DEPTH.npy --gt-mask MASK.npy` scores the metric depth against measured
ground truth of the source size (the reference's tools/evaluate_gt.py:555-583
over its core/gt.py), on the device (evaluate.DeviceEval) from the map the
device post-process left there, with the alignment the spec's `depth_scale`
earns (metric: none).  One `[MDET] gt : ...` line is printed and the result
written as JSON (`--gt-out`, default <out-dir>/depth_pro_gt.json);
`--max-depth` drops ground truth beyond the sensor's range.

`--color PATH` is the reference driver's closing picture (onnx2trt.py:156-176):
inverse depth clipped to [1/250, 10], turbo-coloured, BGR, drawn on the device
(visualize.DeviceColorize) while the map is still there -- 3 bytes per pixel
come back.  `--color-range VMIN VMAX` draws depth on that fixed axis in metres
instead (the reference's core/viz.py:colorize).  One `[MDET] color : ...` line
is printed; the picture is an image file when Pillow is installed, else a .npy
holding the uint8 [H,W,3] BGR array.  models/depth_pro/stream.py does the same
for a frame sequence.
"""

import argparse
import ctypes as C
import os
import time

import numpy as np

from monocular_depth_estimation_trt_amd import bench, common, evaluate, spec, visualize, weights_depth_pro
from monocular_depth_estimation_trt_amd.common_runtime import (EventPair, allocate_buffers, do_inference,
                                                               free_buffers, hip_call, stream_synchronize)
from monocular_depth_estimation_trt_amd import pointcloud
from monocular_depth_estimation_trt_amd.postprocess import DepthProDevicePostprocess, depth_pro_postprocess
from monocular_depth_estimation_trt_amd.preprocess import (DepthProPreprocess, load_image_bgr,
                                                           preprocess_depth_pro_host)

HERE = os.path.dirname(os.path.abspath(__file__))


def preprocess(x: np.ndarray, size: int) -> np.ndarray:
    """onnx2trt.py:72-83: bilinear (align_corners=False) resize of the
    normalised image to size x size when it is not already that size."""
    if x.shape[-2:] == (size, size):
        return np.ascontiguousarray(x, dtype=np.float32)
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return F.interpolate(t, size=(size, size), mode="bilinear", align_corners=False).numpy()


def build_parser(model="depth_pro", size=None):
    size = size or spec.size_of(spec.load(model))[0]
    ap = argparse.ArgumentParser(prog=model)
    ap.add_argument("--source", default="synthetic:depth_pro:dinov2l16_384:4321")
    ap.add_argument("--engine", default=os.path.join(HERE, "engine", f"depth_pro_{size}x{size}_fp16.mdeng"))
    ap.add_argument("--input", default="")
    ap.add_argument("--image", default="", help="source-resolution BGR photo: .npy (uint8 [H,W,3]) or an image file")
    ap.add_argument("--host-preprocess", action="store_true",
                    help="with --image: pre-process on the host (numpy) and upload, instead of on the device")
    ap.add_argument("--host-postprocess", action="store_true",
                    help="download the engine's map and post-process with torch on the CPU")
    ap.add_argument("--f-px", type=float, default=None,
                    help="focal length in pixels (the reference's f_px0) instead of the predicted one")
    ap.add_argument("--src-hw", type=int, nargs=2, default=None,
                    help="source image size for the post-process (default: the image's / input's own size)")
    pointcloud.add_cloud_arguments(ap)
    evaluate.add_gt_arguments(ap)
    visualize.add_color_arguments(ap)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(os.getcwd(), "reports", "bench"))
    return ap


def _device_preprocess(img, size, mem, stream):
    """DepthProPreprocess into the engine's input binding `mem.device`, timed
    with hipEvents (H2D of the frame + the kernel); the pinned side of the
    binding gets the same bytes back, so the timed loop's upload is a no-op in
    value."""
    with DepthProPreprocess(img.shape[0], img.shape[1], size) as pre, EventPair(stream) as ev:
        pre.run(img, mem.device, stream)
        ev.stop()
        hip_call("mde_rt_memcpy_dtoh_async", mem.host.ctypes.data_as(C.c_void_p), C.c_void_p(mem.device),
                 mem.nbytes, C.c_void_p(stream))
        stream_synchronize(stream)
        return ev.ms()


def _device_postprocess(outputs, size, src_hw, f_px, stream, consume=None):
    """DepthProDevicePostprocess on the output bindings in place, timed with
    hipEvents (kernel + D2H of the depth map and the focal length).  Returns
    (depth, f_px, ms); `consume(d_map, d_f_px)` is then called with the device
    pointers of the map and of the focal length the post-process used, while
    they are still there -- outside the timed part."""
    if f_px is None and len(outputs) < 2:
        raise SystemExit("this engine has no fov_deg output: pass --f-px")
    with DepthProDevicePostprocess(1, size, size, *src_hw) as pp:
        with EventPair(stream) as ev:
            pp.enqueue(outputs[0].device, outputs[1].device if len(outputs) > 1 else 0, stream, f_px=f_px)
            ev.stop()
            stream_synchronize(stream)
            ms = ev.ms()
        depth, f = pp.result()
        depth, f = depth[0].copy(), float(f[0])
        if consume:
            consume(pp.mem.device, pp.f_px.device)
        return depth, f, ms


def main(argv=None, model="depth_pro"):
    s = spec.load(model)
    size = spec.size_of(s)[0]
    a = build_parser(model, size).parse_args(argv)
    if a.image and a.input:
        raise SystemExit("--image and --input are exclusive")
    if a.host_preprocess and not a.image:
        raise SystemExit("--host-preprocess needs --image")
    if a.f_px is not None and not a.f_px > 0:
        raise SystemExit("--f-px must be positive")
    pointcloud.check_cloud_arguments(
        a, no_device_map="do not combine it with --host-postprocess" if a.host_postprocess else "")
    gt_policy = evaluate.check_gt_arguments(a, s, device_map=not a.host_postprocess)
    visualize.check_color_arguments(a, device_map=not a.host_postprocess)
    img = load_image_bgr(a.image) if a.image else None
    if img is not None and not a.host_preprocess:
        x = None  # filled on the device, below
        H, W = img.shape[:2]
    else:
        t0 = time.perf_counter()
        if img is not None:
            x, (H, W) = preprocess_depth_pro_host(img, size)
            how = "host, numpy"
        else:
            x = (np.load(a.input, allow_pickle=False).astype(np.float32) if a.input
                 else weights_depth_pro.synthetic_images(1, size, first_seed=0))
            H, W = x.shape[-2:]
            x = preprocess(x, size)
            how = "host, torch resize of a normalised tensor"
        print(f"[MDET] preprocess ({how}) {H}x{W} -> {size}x{size} : {(time.perf_counter() - t0) * 1e3:0.3f} ms")
    src_hw = tuple(a.src_hw) if a.src_hw else (H, W)
    gt_maps = evaluate.load_gt_arguments(a, src_hw) if gt_policy else None
    pointcloud.check_photo_size(a, img, src_hw)
    output_shapes = (1, 1, size, size)
    with common.get_engine(a.source, a.engine, "fp16", None, input_hw=(size, size)) as engine, \
            engine.create_execution_context() as context:
        inputs, outputs, bindings, stream = allocate_buffers(engine)
        if x is None:
            ms = _device_preprocess(img, size, inputs[0], stream)
            print(f"[MDET] preprocess (device, H2D + kernel, hipEvents) {H}x{W} -> {size}x{size} : {ms:0.3f} ms")
            x = inputs[0].host[:3 * size * size].reshape(1, 3, size, size).copy()
        else:
            inputs[0].host = x
        outs, samples = bench.measure(
            lambda: do_inference(context, engine=engine, bindings=bindings, inputs=inputs, outputs=outputs,
                                 stream=stream), warmup=a.warmup, iterations=a.iterations)
        if a.host_postprocess:
            t0 = time.perf_counter()
            inv = outs[0].reshape(output_shapes).copy()
            fov = outs[1].copy() if len(outs) > 1 else None
            depth, f_px = depth_pro_postprocess(inv, fov, src_hw, f_px=a.f_px)
            print(f"[MDET] postprocess (host, torch) {size}x{size} -> {src_hw[0]}x{src_hw[1]} : "
                  f"{(time.perf_counter() - t0) * 1e3:0.3f} ms")
        else:  # the engine's outputs are still in outputs[*].device
            def consume(d_map, d_f_px):
                pointcloud.run_cloud_outputs(a, d_map, src_hw, stream, img_bgr=img, d_f_px=d_f_px, f_px=a.f_px,
                                             z_lo=1e-4, z_hi=1e4)
                if gt_policy:
                    evaluate.driver_score(a, model, gt_policy, gt_maps, d_map, src_hw, stream)
                if a.color:
                    visualize.driver_color(a, s, d_map, src_hw, stream)

            depth, f_px, ms = _device_postprocess(outputs, size, src_hw, a.f_px, stream, consume)
            print(f"[MDET] postprocess (device, kernel + D2H, hipEvents) {size}x{size} -> {src_hw[0]}x{src_hw[1]} : "
                  f"{ms:0.3f} ms")
        bench.record(model, samples, encoder="fixed", warmup=a.warmup, precision="fp16", profile="native",
                     input_h=size, input_w=size, engine_path=a.engine, outputs={"depth": depth, "f_px": np.array(f_px)},
                     notes=f"source={a.source}; 1536x1536 is upstream fixed", model_input=x, out_dir=a.out_dir)
        free_buffers(inputs, outputs, stream)
    print(f"[MDET] max : {depth.max()} , min : {depth.min()}")
    if a.f_px is not None:
        print(f"[MDET] focal length (given) : {f_px:0.2f}")
    else:
        print(f"[MDET] predicted Focal length (by Depth Pro) : {f_px:0.2f}")
    return depth, f_px


if __name__ == "__main__":
    main()
