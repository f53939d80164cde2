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

`--ply PATH` is the reference's `onnx2trt_pointcloud.py:172-184`: the metric
depth at the source size is unprojected with the focal length (x = (u - W/2) /
f_px * z, y likewise) and written as a binary PLY, coloured from the `--image`
photo (no colours with `--input` or the synthetic image).  It runs on the
device (pointcloud.DevicePointCloud) on the depth map and the focal length the
device post-process left there, drops depths outside [1e-4, 1e4] and downloads
the PLY records; `--ply-step N` keeps every N-th pixel on both axes.

`--mesh PATH` is the reference's `models/metric_anything/demo_pointcloud.py:
142-149`: the samples on a depth edge -- a 3x3 spread of depth above
`--edge-rtol` (default 0.1, the reference's) times the depth, or above
`--edge-atol` metres -- are dropped, the 2x2 blocks that survive whole become
two triangles each, and the vertices they use and the faces are packed on the
device (pointcloud.DeviceMesh, `mde_op_depth_mesh`) and written as a binary PLY
with `element vertex` and `element face`.  `--ply-edge-rtol R` gives `--ply`'s
cloud the same edge filter (no flying pixels), without faces.

`--cloud-view PATH` is the reference's `core/viz.py:render_points` (what
`demo.py:cloud_figure` shows): an orthographic, z-buffered picture of that
cloud seen from above-left, drawn on the device from the depth map
(pointcloud.DeviceCloudView, `mde_op_cloud_view`); only the picture comes
back.  One `[MDET] cloud view ...` line is printed; the file is written like
`--color`'s.

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
from monocular_depth_estimation_trt_amd.common_runtime import (allocate_buffers, do_inference, free_buffers, hip_call,
                                                               stream_synchronize)
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
    ap.add_argument("--ply", default="", metavar="PATH",
                    help="write the point cloud (binary PLY; colours from --image) of the metric depth")
    ap.add_argument("--ply-step", type=int, default=1, help="with --ply: keep every N-th pixel on both axes")
    pointcloud.add_mesh_arguments(ap)
    pointcloud.add_cloud_view_arguments(ap)
    evaluate.add_gt_arguments(ap)
    visualize.add_color_arguments(ap)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(os.getcwd(), "reports", "bench"))
    return ap


class _Events:
    """A hipEvent pair on one stream; ms() after the stream has synchronized."""

    def __init__(self, stream):
        self.stream = C.c_void_p(stream)
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            hip_call("mde_rt_event_create", C.byref(e))

    def mark(self, i):
        hip_call("mde_rt_event_record", self.ev[i], self.stream)

    def ms(self):
        ms = C.c_float()
        hip_call("mde_rt_event_elapsed_ms", C.byref(ms), self.ev[0], self.ev[1])
        return float(ms.value)

    def free(self):
        for e in self.ev:
            hip_call("mde_rt_event_destroy", e)


def _device_preprocess(img, size, mem, stream):
    """DepthProPreprocess into the engine's input binding `mem.device`, timed
    with hipEvents (H2D of the frame + the kernel); the pinned side of the
    binding gets the same bytes back, so the timed loop's upload is a no-op in
    value."""
    ev = _Events(stream)
    try:
        with DepthProPreprocess(img.shape[0], img.shape[1], size) as pre:
            ev.mark(0)
            pre.run(img, mem.device, stream)
            ev.mark(1)
            hip_call("mde_rt_memcpy_dtoh_async", mem.host.ctypes.data_as(C.c_void_p), C.c_void_p(mem.device),
                     mem.nbytes, C.c_void_p(stream))
            stream_synchronize(stream)
        return ev.ms()
    finally:
        ev.free()


def _device_postprocess(outputs, size, src_hw, f_px, stream, ply=None, score=None, color=None, cloud_view=None,
                        mesh=None):
    """DepthProDevicePostprocess on the output bindings in place, timed with
    hipEvents (kernel + D2H of the depth map and the focal length); `ply` =
    (the parsed arguments, photo or None): then the point cloud of the map,
    while it is still on the device, with the focal length the post-process
    used (the fourth result, pointcloud.driver_ply's; else None); `mesh`:
    called with the map's and the focal length's device pointers (--mesh);
    `score`: called with
    the map's device pointer while it is still there (--gt); `color`: likewise
    (--color); `cloud_view`: likewise, with the device focal length as well
    (--cloud-view)."""
    if f_px is None and len(outputs) < 2:
        raise SystemExit("this engine has no fov_deg output: pass --f-px")
    ev = _Events(stream)
    try:
        with DepthProDevicePostprocess(1, size, size, *src_hw) as pp:
            ev.mark(0)
            pp.enqueue(outputs[0].device, outputs[1].device if len(outputs) > 1 else 0, stream, f_px=f_px)
            ev.mark(1)
            stream_synchronize(stream)
            depth, f = pp.result()
            depth, f, ms = depth[0].copy(), float(f[0]), ev.ms()
            cloud = None
            if ply:
                a, img = ply
                cloud = pointcloud.driver_ply(a, pp.mem.device, src_hw, stream, img_bgr=img, d_f_px=pp.f_px.device,
                                              f_px=f_px, z_lo=1e-4, z_hi=1e4)
            if mesh:
                mesh(pp.mem.device, pp.f_px.device)
            if score:
                score(pp.mem.device)
            if color:
                color(pp.mem.device)
            if cloud_view:
                cloud_view(pp.mem.device, pp.f_px.device)
            return depth, f, ms, cloud
    finally:
        ev.free()


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
    if a.ply and a.host_postprocess:
        raise SystemExit("--ply runs on the device post-process's depth map: do not combine it with "
                         "--host-postprocess")
    if a.ply and a.ply_step < 1:
        raise SystemExit("--ply-step must be positive")
    if a.mesh and a.host_postprocess:
        raise SystemExit("--mesh runs on the device post-process's depth map: do not combine it with "
                         "--host-postprocess")
    pointcloud.check_mesh_arguments(a)
    if a.cloud_view and a.host_postprocess:
        raise SystemExit("--cloud-view runs on the device post-process's depth map: do not combine it with "
                         "--host-postprocess")
    pointcloud.check_cloud_view_arguments(a)
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
    if a.ply and img is not None and src_hw != img.shape[:2]:
        raise SystemExit("--ply takes its colours from the --image photo: --src-hw must be the photo's size")
    if a.mesh and img is not None and src_hw != img.shape[:2]:
        raise SystemExit("--mesh takes its colours from the --image photo: --src-hw must be the photo's size")
    if a.cloud_view and img is not None and src_hw != img.shape[:2]:
        raise SystemExit("--cloud-view takes its colours from the --image photo: --src-hw must be the photo's size")
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
            score = (lambda d_map: evaluate.driver_score(a, model, gt_policy, gt_maps, d_map, src_hw, stream)) if gt_policy \
                else None
            color = (lambda d_map: visualize.driver_color(a, s, d_map, src_hw, stream)) if a.color else None
            view = (lambda d_map, d_f: pointcloud.driver_cloud_view(a, d_map, src_hw, stream, img_bgr=img, d_f_px=d_f,
                                                                    f_px=a.f_px)) if a.cloud_view else None
            mesh = (lambda d_map, d_f: pointcloud.driver_mesh(a, d_map, src_hw, stream, img_bgr=img, d_f_px=d_f,
                                                              f_px=a.f_px, z_lo=1e-4, z_hi=1e4)) if a.mesh else None
            depth, f_px, ms, cloud = _device_postprocess(outputs, size, src_hw, a.f_px, stream,
                                                         ply=(a, img) if a.ply else None, score=score,
                                                         color=color, cloud_view=view, mesh=mesh)
            print(f"[MDET] postprocess (device, kernel + D2H, hipEvents) {size}x{size} -> {src_hw[0]}x{src_hw[1]} : "
                  f"{ms:0.3f} ms")
            if cloud:
                print(f"[MDET] point cloud (device, kernels + D2H, hipEvents) {src_hw[0]}x{src_hw[1]} step "
                      f"{a.ply_step} -> {a.ply} : {cloud[0]:0.3f} ms, {cloud[1]} points")
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
