"""Depth Anything V2 (and its family) on MI355X -- the counterpart of the
reference drivers `models/depth_anything_v2/onnx2trt.py:main` (:42-127),
`models/depth_anything_ac/onnx2trt.py` and `models/distill_any_depth/
onnx2trt.py` (the same ViT-S DA-V2 graph, relative head), same sequence:

  input -> get_engine -> create_execution_context -> allocate_buffers ->
  bench.measure(do_inference) (20 warmup / 100 iterations) ->
  post-process (bilinear align_corners=True back to the source size, clamp
  [1e-3, 1e3], outside the timed loop) -> bench.record

    python -m monocular_depth_estimation_trt_amd.models.depth_anything_v2.run \
        [--source synthetic:vits:metric | ckpt.pth] [--input x.npy] [--src-hw H W]
        [--image photo.npy|photo.jpg] [--host-preprocess]
        [--input-format float32_nchw | uint8_nhwc] [--host-postprocess]
        [--ply out.ply --f-px F [--ply-step N] [--ply-edge-rtol R]]
        [--mesh out.ply --f-px F [--mesh-step N] [--edge-rtol R] [--edge-atol A]]
        [--cloud-view out.png --f-px F [--cloud-view-size H W] [--cloud-view-angles ELEV AZIM] [--cloud-view-step N]]
        [--gt depth.npy --gt-mask mask.npy [--max-depth M] [--gt-out PATH.json]]
        [--color out.png [--color-range VMIN VMAX | --color-robust [LO HI]] [--color-robust-near]]

`--image` is a source-resolution BGR photo -- a .npy holding a uint8 [H,W,3]
BGR array, or an image file if Pillow is installed -- taken through the
reference's core/preprocess.py:preprocess_for (BGR->RGB, cv2 INTER_LINEAR
stretch on uint8, /255, standardise) on the device, straight into the
engine's input binding (preprocess.DevicePreprocess; `--host-preprocess`: the
numpy version and the usual upload); `--src-hw` then defaults to the photo's
own size.  The pre-process is outside the timed loop, as in the reference.
`--input` is an already-preprocessed float32 NCHW [1,3,518,518] tensor (the
reference's core/preprocess.py needs cv2, absent here), or for
`--input-format uint8_nhwc` the uint8 [1,518,518,3] image the reference's
uint8 engine takes (core/onnx_tools.py:87-219: normalisation on the device);
without it a synthetic image of the spec's input domain is used.  The
post-process runs on the device (postprocess.DevicePostprocess) unless
`--host-postprocess` asks for the reference's torch-CPU version.

`--ply PATH` writes the point cloud of the metric depth map at the source size
(the reference's models/depth_pro/onnx2trt_pointcloud.py:172-184 tail, which
its docs/model_contracts.md allows for every "metric depth + focal length"
model), on the device (pointcloud.DevicePointCloud) from the map the device
post-process left there, coloured from the `--image` photo, depths outside this
driver's clamp [1e-3, 1e3] dropped.  There is no FOV head: `--f-px` (focal
length in pixels at the source size) is required.  Relative models (the
relative checkpoints, depth_anything_ac, distill_any_depth) are refused:
relative depth is not turned into metres.

`--mesh PATH` is the reference's models/metric_anything/demo_pointcloud.py:
142-149 under the same conditions as `--ply`: samples on a depth edge (3x3
spread of depth above `--edge-rtol`, default 0.1, times the depth, or above
`--edge-atol`) are dropped, the surviving 2x2 blocks become two triangles each
and the mesh is packed on the device (pointcloud.DeviceMesh) as a binary PLY
with vertices and faces.  `--ply-edge-rtol R` gives `--ply`'s cloud the same
edge filter, without faces.

`--cloud-view PATH` draws that cloud instead of packing it: the reference's
core/viz.py:render_points (demo.py:cloud_figure), an orthographic, z-buffered
picture seen from above-left, on the device (pointcloud.DeviceCloudView) under
the same conditions as `--ply`; only the picture comes back.

`--gt DEPTH.npy --gt-mask MASK.npy` scores the map against measured ground
truth of the same size (the reference's tools/evaluate_gt.py:555-583 over its
core/gt.py), on the device (evaluate.DeviceEval) from the map the device
post-process left there -- for distill_any_depth, which has no post-process,
the engine's output binding.  The alignment comes from the model's spec.json:
`depth_scale` metric -> none, relative -> scale and shift fitted in disparity,
`output_form` saying which way round the output runs.  One `[MDET] gt : ...`
line is printed and the result written as JSON (`--gt-out`, default
<out-dir>/<model>_gt.json); `--max-depth` drops ground truth beyond the
sensor's range.

`--color PATH` is the reference drivers' closing picture (onnx2trt.py:131-151):
the map, turbo-coloured, BGR, drawn on the device (visualize.DeviceColorize)
while the map is still there -- 3 bytes per pixel come back.  The recipe comes
from the spec's `depth_scale`: metric -> inverse depth clipped to [1/250, 10],
relative -> the map's own min..max in 256 steps.  `--color-range VMIN VMAX`
draws depth on that fixed axis instead (the reference's core/viz.py:colorize).
One `[MDET] color : ...` line is printed; the picture is an image file when
Pillow is installed, else a .npy holding the uint8 [H,W,3] BGR array.
"""

import argparse
import os
import time

import numpy as np

from monocular_depth_estimation_trt_amd import bench, common, evaluate, spec, visualize, weights
from monocular_depth_estimation_trt_amd import pointcloud
from monocular_depth_estimation_trt_amd.postprocess import DevicePostprocess
from monocular_depth_estimation_trt_amd.preprocess import (DevicePreprocess, load_image_bgr, preprocess_host,
                                                           resize_linear_u8)
from monocular_depth_estimation_trt_amd.common_runtime import (allocate_buffers, do_inference, free_buffers, hip_call,
                                                               stream_synchronize)

HERE = os.path.dirname(os.path.abspath(__file__))


def postprocess(depth: np.ndarray, src_hw) -> np.ndarray:
    """onnx2trt.py:111-117: bilinear(align_corners=True) to the source size, clamp."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(depth))[:, None]
    t = F.interpolate(t, tuple(src_hw), mode="bilinear", align_corners=True)[0, 0]
    return torch.clamp(t, min=1e-3, max=1e3).numpy()


def build_parser(model="depth_anything_v2", mc=None):
    mc = mc or spec.model_config_of(spec.load(model))
    input_h, input_w = mc["input_hw"]
    ap = argparse.ArgumentParser(prog=model)
    ap.add_argument("--source", default=f"synthetic:{mc['encoder']}:{mc['depth_type']}:1234")
    ap.add_argument("--engine", default=os.path.join(os.path.dirname(HERE), model, "engine",
                                                     f"{model}_{mc['encoder']}_{input_h}x{input_w}_fp16.mdeng"))
    ap.add_argument("--input", default="")
    ap.add_argument("--image", default="", help="source-resolution BGR photo: .npy (uint8 [H,W,3]) or an image file")
    ap.add_argument("--host-preprocess", action="store_true",
                    help="with --image: pre-process on the host (numpy) and upload, instead of on the device")
    ap.add_argument("--src-hw", type=int, nargs=2, default=None,
                    help="size of the returned map (default: the --image's own size, else 2268 3024)")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(os.getcwd(), "reports", "bench"))
    ap.add_argument("--input-format", choices=("float32_nchw", "uint8_nhwc"), default="float32_nchw")
    ap.add_argument("--host-postprocess", action="store_true")
    ap.add_argument("--ply", default="", metavar="PATH",
                    help="write the point cloud (binary PLY; colours from --image) of the metric depth; needs --f-px")
    ap.add_argument("--ply-step", type=int, default=1, help="with --ply: keep every N-th pixel on both axes")
    ap.add_argument("--f-px", type=float, default=None,
                    help="with --ply / --mesh / --cloud-view: focal length in pixels at the source size")
    pointcloud.add_mesh_arguments(ap)
    pointcloud.add_cloud_view_arguments(ap)
    evaluate.add_gt_arguments(ap)
    visualize.add_color_arguments(ap)
    return ap


NOT_METRIC = "--ply needs a metric model: relative depth is not turned into metres"


def _check_ply(a, mc, opt="--ply"):
    """--ply's (and --mesh's and --cloud-view's) conditions that can be answered before an engine is built."""
    if a.f_px is None or not a.f_px > 0:
        raise SystemExit(f"{opt} needs --f-px (a positive focal length in pixels): this model predicts none")
    if opt == "--ply" and a.ply_step < 1:
        raise SystemExit("--ply-step must be positive")
    fields = a.source.split(":")
    if mc["depth_type"] != "metric" or (fields[0] == "synthetic" and len(fields) > 2 and fields[2] == "relative"):
        raise SystemExit(NOT_METRIC.replace("--ply", opt))
    if a.host_postprocess or mc["postprocess"] == "none":
        raise SystemExit(f"{opt} runs on the device post-process's depth map: not with --host-postprocess or a model "
                         "without a post-process")


def _device_preprocess(img, model, input_hw, input_format, mem, stream):
    """DevicePreprocess into the engine's input binding `mem.device`, timed with
    hipEvents (H2D of the frame + the kernel); the pinned side of the binding
    gets the same bytes back, so the timed loop's upload is a no-op in value."""
    import ctypes as C
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        hip_call("mde_rt_event_create", C.byref(e))
    try:
        with DevicePreprocess(img.shape[0], img.shape[1], *input_hw, model, output=input_format) as pre:
            hip_call("mde_rt_event_record", ev[0], C.c_void_p(stream))
            pre.run(img, mem.device, stream)
            hip_call("mde_rt_event_record", ev[1], C.c_void_p(stream))
            hip_call("mde_rt_memcpy_dtoh_async", mem.host.ctypes.data_as(C.c_void_p), C.c_void_p(mem.device),
                     mem.nbytes, C.c_void_p(stream))
            stream_synchronize(stream)
        ms = C.c_float()
        hip_call("mde_rt_event_elapsed_ms", C.byref(ms), ev[0], ev[1])
    finally:
        for e in ev:
            hip_call("mde_rt_event_destroy", e)
    return float(ms.value)


def main(argv=None, model="depth_anything_v2"):
    model_spec = spec.load(model)
    mc = spec.model_config_of(model_spec)
    input_h, input_w = mc["input_hw"]
    a = build_parser(model, mc).parse_args(argv)
    u8 = a.input_format == "uint8_nhwc"
    if a.image and a.input:
        raise SystemExit("--image and --input are exclusive")
    if a.host_preprocess and not a.image:
        raise SystemExit("--host-preprocess needs --image")
    if a.ply:
        _check_ply(a, mc)
    if a.mesh:
        _check_ply(a, mc, "--mesh")
    pointcloud.check_mesh_arguments(a)
    if a.cloud_view:
        _check_ply(a, mc, "--cloud-view")
        pointcloud.check_cloud_view_arguments(a)
    gt_policy = evaluate.check_gt_arguments(a, model_spec, device_map=not a.host_postprocess)
    visualize.check_color_arguments(a, device_map=not a.host_postprocess)
    img = load_image_bgr(a.image) if a.image else None
    if a.src_hw is None:
        a.src_hw = list(img.shape[:2]) if img is not None else [2268, 3024]
    gt_hw = (input_h, input_w) if mc["postprocess"] == "none" else tuple(a.src_hw)  # the size of the scored map
    gt_maps = evaluate.load_gt_arguments(a, gt_hw) if gt_policy else None
    if a.ply and img is not None and tuple(a.src_hw) != img.shape[:2]:
        raise SystemExit("--ply takes its colours from the --image photo: --src-hw must be the photo's size")
    if a.mesh and img is not None and tuple(a.src_hw) != img.shape[:2]:
        raise SystemExit("--mesh takes its colours from the --image photo: --src-hw must be the photo's size")
    if a.cloud_view and img is not None and tuple(a.src_hw) != img.shape[:2]:
        raise SystemExit("--cloud-view takes its colours from the --image photo: --src-hw must be the photo's size")
    if u8 and a.engine.endswith("_fp16.mdeng"):
        a.engine = a.engine[:-len("_fp16.mdeng")] + "_u8_fp16.mdeng"
    if img is not None and a.host_preprocess:
        t0 = time.perf_counter()
        x = (resize_linear_u8(img[:, :, ::-1], input_h, input_w)[None] if u8
             else preprocess_host(img, model, (input_h, input_w))[0])
        print(f"[MDET] preprocess (host, numpy) {img.shape[0]}x{img.shape[1]} -> {input_h}x{input_w} : "
              f"{(time.perf_counter() - t0) * 1e3:0.3f} ms")
    elif img is not None:
        x = None  # filled on the device, below
    elif u8:
        x = (np.load(a.input, allow_pickle=False).astype(np.uint8) if a.input
             else weights.synthetic_images_u8(1, input_h, input_w, first_seed=0))
    else:
        x = (np.load(a.input, allow_pickle=False).astype(np.float32) if a.input
             else weights.synthetic_images(1, input_h, input_w, first_seed=0))
    output_shape = (1, input_h, input_w)
    with common.get_engine(a.source, a.engine, "fp16", None, encoder=mc["encoder"], depth_type=mc["depth_type"],
                           max_depth=mc["max_depth"], input_hw=(input_h, input_w),
                           input_format=a.input_format) as engine, \
            engine.create_execution_context() as context:
        if a.ply and not engine.info.metric:
            raise SystemExit(NOT_METRIC)
        if a.mesh and not engine.info.metric:
            raise SystemExit(NOT_METRIC.replace("--ply", "--mesh"))
        if a.cloud_view and not engine.info.metric:
            raise SystemExit(NOT_METRIC.replace("--ply", "--cloud-view"))
        inputs, outputs, bindings, stream = allocate_buffers(engine, output_shape, profile_idx=0)
        if x is None:
            ms = _device_preprocess(img, model, (input_h, input_w), a.input_format, inputs[0], stream)
            print(f"[MDET] preprocess (device, H2D + kernel, hipEvents) {img.shape[0]}x{img.shape[1]} -> "
                  f"{input_h}x{input_w} {a.input_format} : {ms:0.3f} ms")
            x = inputs[0].host[:3 * input_h * input_w].reshape(
                (1, input_h, input_w, 3) if u8 else (1, 3, input_h, input_w)).copy()
        else:
            inputs[0].host = x
        outs, samples = bench.measure(
            lambda: do_inference(context, engine=engine, bindings=bindings, inputs=inputs, outputs=outputs,
                                 stream=stream), warmup=a.warmup, iterations=a.iterations)
        if mc["postprocess"] == "none":   # distill_any_depth: the 518x518 map as is (its onnx2trt.py:98-100)
            depth = outs[0].reshape(output_shape)[0].copy()
            if gt_policy:  # no post-process: the engine's output binding is the map
                evaluate.driver_score(a, model, gt_policy, gt_maps, outputs[0].device, gt_hw, stream)
            if a.color:
                visualize.driver_color(a, model_spec, outputs[0].device, gt_hw, stream)
        elif a.host_postprocess:
            depth = postprocess(outs[0].reshape(output_shape), a.src_hw)
        else:  # the engine's output is still in outputs[0].device
            with DevicePostprocess(1, input_h, input_w, *a.src_hw) as pp:
                depth = pp.run(outputs[0].device, stream)[0].copy()
                if a.ply:  # the clamped map is still in pp.mem.device
                    ms, n = pointcloud.driver_ply(a, pp.mem.device, a.src_hw, stream, img_bgr=img, f_px=a.f_px,
                                                  z_lo=1e-3, z_hi=1e3)
                    print(f"[MDET] point cloud (device, kernels + D2H, hipEvents) {a.src_hw[0]}x{a.src_hw[1]} step "
                          f"{a.ply_step} -> {a.ply} : {ms:0.3f} ms, {n} points")
                if a.mesh:
                    pointcloud.driver_mesh(a, pp.mem.device, a.src_hw, stream, img_bgr=img, f_px=a.f_px, z_lo=1e-3,
                                           z_hi=1e3)
                if a.cloud_view:
                    pointcloud.driver_cloud_view(a, pp.mem.device, a.src_hw, stream, img_bgr=img, f_px=a.f_px)
                if gt_policy:
                    evaluate.driver_score(a, model, gt_policy, gt_maps, pp.mem.device, gt_hw, stream)
                if a.color:
                    visualize.driver_color(a, model_spec, pp.mem.device, gt_hw, stream)
        bench.record(model, samples, warmup=a.warmup, precision="fp16", profile="bench",
                     variant="u8" if u8 else "single",
                     input_h=input_h, input_w=input_w, engine_path=a.engine, outputs={"depth": depth},
                     encoder=mc["encoder"], notes=f"source={a.source}", model_input=x, out_dir=a.out_dir)
        print(f"[MDET] max : {depth.max():0.5f} , min : {depth.min():0.5f}")
        free_buffers(inputs, outputs, stream)
    return depth


if __name__ == "__main__":
    main()
