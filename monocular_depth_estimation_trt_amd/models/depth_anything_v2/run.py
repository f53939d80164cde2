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
        [--image photo.npy|photo.jpg] [--host-preprocess] [--profile bench|native [--native-target N]]
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
`--profile native` (depth_anything_v2 and depth_anything_ac; reference
models/depth_anything_ac/onnx2trt.py:50-77) does not stretch the photo to the
engine's square: the engine is built for preprocess.native_size of the photo
(short side `--native-target`, default 518, aspect kept, sides snapped to
multiples of 14: 518x700 for a 4:3 photo under depth_anything_ac's rule,
518x686 under depth_anything_v2's) and the photo reaches it through the
reference's keep-ratio cubic resize of the float image, on the device
(preprocess.NativePreprocess) or with `--host-preprocess` in numpy
(preprocess_native_host).  A default `--engine` path gets that size in its
name, so bench and native engines coexist.  Everything after the engine runs
unchanged on the source-size map.
`--input` is an already-preprocessed float32 NCHW [1,3,518,518] tensor (the
reference's core/preprocess.py needs cv2, absent here), or for
`--input-format uint8_nhwc` the uint8 [1,518,518,3] image the reference's
uint8 engine takes (core/onnx_tools.py:87-219: normalisation on the device);
without it a synthetic image of the spec's input domain is used.  The
post-process runs on the device (postprocess.DevicePostprocess) unless
`--host-postprocess` asks for the reference's torch-CPU version.

`--ply`, `--mesh` and `--cloud-view` are pointcloud.py's one stage for the
cloud outputs, described there (the reference's docs/model_contracts.md allows
them for every "metric depth + focal length" model).  Here they run on the map
the device post-process left on the device, coloured from the `--image` photo,
depths outside this driver's clamp [1e-3, 1e3] dropped.  There is no FOV head:
`--f-px` (focal length in pixels at the source size) is required.  Relative
models (the relative checkpoints, depth_anything_ac, distill_any_depth) are
refused: relative depth is not turned into metres.

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
from monocular_depth_estimation_trt_amd.preprocess import (NATIVE_ROUNDING, DevicePreprocess, NativePreprocess,
                                                           load_image_bgr, native_size, preprocess_host,
                                                           preprocess_native_host, resize_linear_u8)
from monocular_depth_estimation_trt_amd.common_runtime import (EventPair, allocate_buffers, do_inference,
                                                               free_buffers, hip_call, stream_synchronize)

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
    ap.add_argument("--profile", choices=("bench", "native"), default="bench",
                    help="bench: stretch the photo to the engine's size; native: keep its aspect ratio (short side "
                         "--native-target, multiples of 14) and build the engine for that size")
    ap.add_argument("--native-target", type=int, default=518, help="with --profile native: the short side")
    ap.add_argument("--src-hw", type=int, nargs=2, default=None,
                    help="size of the returned map (default: the --image's own size, else 2268 3024)")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(os.getcwd(), "reports", "bench"))
    ap.add_argument("--input-format", choices=("float32_nchw", "uint8_nhwc"), default="float32_nchw")
    ap.add_argument("--host-postprocess", action="store_true")
    ap.add_argument("--f-px", type=float, default=None,
                    help="with --ply / --mesh / --cloud-view: focal length in pixels at the source size")
    pointcloud.add_cloud_arguments(ap, needs_f_px=True)
    evaluate.add_gt_arguments(ap)
    visualize.add_color_arguments(ap)
    return ap


def _check_cloud(a, mc, metric):
    """pointcloud.check_cloud_arguments with what this driver knows: no FOV
    head, and no device map under --host-postprocess or without a post-process."""
    no_map = a.host_postprocess or mc["postprocess"] == "none"
    pointcloud.check_cloud_arguments(
        a, needs_f_px=True, metric=metric,
        no_device_map="not with --host-postprocess or a model without a post-process" if no_map else "")


def _check_native(a, model):
    """--profile native's refusals, before the photo is opened."""
    if a.input:
        raise SystemExit("--profile native does not take --input: an already-preprocessed tensor has no photo to "
                         "take the size rule from")
    if not a.image:
        raise SystemExit("--profile native needs --image: the engine's size follows the photo's")
    if a.input_format == "uint8_nhwc":
        raise SystemExit("--profile native does not take --input-format uint8_nhwc: the rule resizes the float "
                         "image after its division by 255, and a uint8 engine normalises after the resize")
    if model not in NATIVE_ROUNDING:
        raise SystemExit(f"--profile native is not for {model}: its second resize stage snaps to the engine's size, "
                         f"it has no keep-ratio rule (have {sorted(NATIVE_ROUNDING)})")
    if a.native_target < 1:
        raise SystemExit("--native-target must be positive")


def native_engine_path(model, engine, default, input_hw):
    """The default engine path with the native size in place of the spec's; a path the user gave stays."""
    if engine != default:
        return engine
    mc = spec.model_config_of(spec.load(model))
    return os.path.join(os.path.dirname(default), f"{model}_{mc['encoder']}_{input_hw[0]}x{input_hw[1]}_fp16.mdeng")


def _device_preprocess(img, model, input_hw, input_format, mem, stream, native_target=None):
    """DevicePreprocess (native_target: NativePreprocess) into the engine's input
    binding `mem.device`, timed with hipEvents (H2D of the frame + the kernel);
    the pinned side of the binding gets the same bytes back, so the timed loop's
    upload is a no-op in value."""
    import ctypes as C
    with (NativePreprocess(img.shape[0], img.shape[1], model, target=native_target) if native_target else
          DevicePreprocess(img.shape[0], img.shape[1], *input_hw, model, output=input_format)) as pre, \
            EventPair(stream) as ev:
        assert pre.dst == tuple(input_hw)
        pre.run(img, mem.device, stream)
        ev.stop()
        hip_call("mde_rt_memcpy_dtoh_async", mem.host.ctypes.data_as(C.c_void_p), C.c_void_p(mem.device),
                 mem.nbytes, C.c_void_p(stream))
        stream_synchronize(stream)
        return ev.ms()


def main(argv=None, model="depth_anything_v2"):
    model_spec = spec.load(model)
    mc = spec.model_config_of(model_spec)
    input_h, input_w = mc["input_hw"]
    parser = build_parser(model, mc)
    a = parser.parse_args(argv)
    u8 = a.input_format == "uint8_nhwc"
    native = a.profile == "native"
    if a.image and a.input:
        raise SystemExit("--image and --input are exclusive")
    if native:
        _check_native(a, model)
    if a.host_preprocess and not a.image:
        raise SystemExit("--host-preprocess needs --image")
    fields = a.source.split(":")
    _check_cloud(a, mc, metric=mc["depth_type"] == "metric" and
                 not (fields[0] == "synthetic" and len(fields) > 2 and fields[2] == "relative"))
    gt_policy = evaluate.check_gt_arguments(a, model_spec, device_map=not a.host_postprocess)
    visualize.check_color_arguments(a, device_map=not a.host_postprocess)
    img = load_image_bgr(a.image) if a.image else None
    if native:  # the engine's size follows the photo
        input_h, input_w = native_size(model, img.shape[0], img.shape[1], a.native_target)
        a.engine = native_engine_path(model, a.engine, parser.get_default("engine"), (input_h, input_w))
    how = f"native, target {a.native_target}" if native else "bench"
    if a.src_hw is None:
        a.src_hw = list(img.shape[:2]) if img is not None else [2268, 3024]
    gt_hw = (input_h, input_w) if mc["postprocess"] == "none" else tuple(a.src_hw)  # the size of the scored map
    gt_maps = evaluate.load_gt_arguments(a, gt_hw) if gt_policy else None
    pointcloud.check_photo_size(a, img, a.src_hw)
    if u8 and a.engine.endswith("_fp16.mdeng"):
        a.engine = a.engine[:-len("_fp16.mdeng")] + "_u8_fp16.mdeng"
    if img is not None and a.host_preprocess:
        t0 = time.perf_counter()
        x = (resize_linear_u8(img[:, :, ::-1], input_h, input_w)[None] if u8
             else preprocess_native_host(img, model, a.native_target)[0] if native
             else preprocess_host(img, model, (input_h, input_w))[0])
        print(f"[MDET] preprocess (host, numpy) [{how}] {img.shape[0]}x{img.shape[1]} -> {input_h}x{input_w} : "
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
        _check_cloud(a, mc, metric=engine.info.metric)
        inputs, outputs, bindings, stream = allocate_buffers(engine, output_shape, profile_idx=0)
        if x is None:
            ms = _device_preprocess(img, model, (input_h, input_w), a.input_format, inputs[0], stream,
                                    native_target=a.native_target if native else None)
            print(f"[MDET] preprocess (device, H2D + kernel, hipEvents) [{how}] {img.shape[0]}x{img.shape[1]} -> "
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
                # the clamped map is still in pp.mem.device
                pointcloud.run_cloud_outputs(a, pp.mem.device, a.src_hw, stream, img_bgr=img, f_px=a.f_px, z_lo=1e-3,
                                             z_hi=1e3)
                if gt_policy:
                    evaluate.driver_score(a, model, gt_policy, gt_maps, pp.mem.device, gt_hw, stream)
                if a.color:
                    visualize.driver_color(a, model_spec, pp.mem.device, gt_hw, stream)
        bench.record(model, samples, warmup=a.warmup, precision="fp16", profile=a.profile,
                     variant="u8" if u8 else "single",
                     input_h=input_h, input_w=input_w, engine_path=a.engine, outputs={"depth": depth},
                     encoder=mc["encoder"], notes=f"source={a.source}", model_input=x, out_dir=a.out_dir)
        print(f"[MDET] max : {depth.max():0.5f} , min : {depth.min():0.5f}")
        free_buffers(inputs, outputs, stream)
    return depth


if __name__ == "__main__":
    main()
