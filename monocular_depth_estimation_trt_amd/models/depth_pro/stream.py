"""Depth Pro on a frame sequence -- the counterpart of the reference's live
paths `models/depth_pro/onnx2trt_video.py` (:69-81) and `onnx2trt_webcam.py`
(:96-104), whose output is the coloured frame and nothing else:

    python -m monocular_depth_estimation_trt_amd.models.depth_pro.stream \
        --frames FRAMES.npy --out OUT.npy [--color-range VMIN VMAX | --color-robust [LO HI]] [--color-robust-near] [--f-px F]
        [--cloud-view-out VIEWS.npy [--cloud-view-size H W] [--cloud-view-angles ELEV AZIM] [--cloud-view-step N]]
        [--source synthetic:depth_pro | DepthPro.safetensors] [--engine PATH]

`--frames` is a uint8 [T,H,W,3] BGR array; `--out` receives the uint8
[T,H,W,3] BGR colour frames.  Per frame, on one stream and with one
synchronisation at its end:

  H2D of the frame -> preprocess.DepthProPreprocess into the engine's input
  binding -> execute_async_v3 -> postprocess.dp_postprocess on the output
  bindings in place -> visualize.DeviceColorize on the metric map ->
  D2H of the colour frame (3 bytes per pixel)

The float map never leaves the card.  The colours are `run.py --color`'s:
inverse depth clipped to [1/250, 10] on each frame's own range, or depth on
the fixed axis of `--color-range`, which keeps the colours steady over a
sequence.  The reference's three closing lines are printed (iterations time,
average FPS, average inference time: wall clock per frame, everything above
included).  The FPS overlay (cv2.putText) and container I/O are not part of
this driver: frames come from and go to .npy arrays.

`--cloud-view-out VIEWS.npy` adds one point-cloud preview per frame (uint8
[T,h,w,3] BGR, `run.py --cloud-view`'s picture): pointcloud.DeviceCloudView on
the metric map, the focal length and the frame, all still in device memory,
enqueued before the frame's one synchronisation.  The camera -- centre and
scale -- is selected on the first frame and fixed from its view row for the
rest, so the sequence does not jitter; neither the float map nor the cloud
leaves the card.
"""

import argparse
import contextlib
import ctypes as C
import os
import time

import numpy as np

from monocular_depth_estimation_trt_amd import common, pointcloud, spec, visualize
from monocular_depth_estimation_trt_amd.common_runtime import (allocate_buffers, free_buffers, hip_call,
                                                               stream_synchronize)
from monocular_depth_estimation_trt_amd.postprocess import dp_postprocess
from monocular_depth_estimation_trt_amd.preprocess import DepthProPreprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def build_parser(model="depth_pro", size=None):
    size = size or spec.size_of(spec.load(model))[0]
    ap = argparse.ArgumentParser(prog=f"{model}.stream")
    ap.add_argument("--source", default="synthetic:depth_pro:dinov2l16_384:4321")
    ap.add_argument("--engine", default=os.path.join(HERE, "engine", f"depth_pro_{size}x{size}_fp16.mdeng"))
    ap.add_argument("--frames", default="", metavar="FRAMES.npy", help="uint8 [T,H,W,3] BGR frames")
    ap.add_argument("--out", default="", metavar="OUT.npy", help="where the uint8 [T,H,W,3] BGR colour frames go")
    ap.add_argument("--color-range", type=float, nargs=2, default=None, metavar=("VMIN", "VMAX"),
                    help="draw depth on this fixed axis in metres instead of each frame's own range")
    visualize.add_robust_arguments(ap)
    ap.add_argument("--f-px", type=float, default=None,
                    help="focal length in pixels instead of the predicted one")
    ap.add_argument("--cloud-view-out", default="", metavar="VIEWS.npy",
                    help="where the uint8 [T,h,w,3] BGR point-cloud previews go (camera fixed from the first frame)")
    pointcloud.add_cloud_view_arguments(ap, picture=False)
    return ap


def load_frames(path: str) -> np.ndarray:
    try:
        frames = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--frames: {e}")
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or 0 in frames.shape:
        raise SystemExit(f"--frames: expected a uint8 [T,H,W,3] BGR array, got {frames.dtype} {frames.shape}")
    return frames


def main(argv=None, model="depth_pro"):
    s = spec.load(model)
    size = spec.size_of(s)[0]
    a = build_parser(model, size).parse_args(argv)
    if not a.frames or not a.out:
        raise SystemExit("--frames FRAMES.npy and --out OUT.npy are both needed")
    if a.f_px is not None and not a.f_px > 0:
        raise SystemExit("--f-px must be positive")
    if a.color_range is not None and not all(v == v for v in a.color_range):
        raise SystemExit("--color-range must not be NaN")
    if a.color_range is not None and visualize.robust_percent(a) is not None:
        raise SystemExit("--color-robust and --color-range exclude each other")
    a.cloud_view = a.cloud_view_out
    pointcloud.check_cloud_view_arguments(a)
    frames = load_frames(a.frames)
    T, H, W = frames.shape[:3]
    kw = visualize.color_kwargs(a, s)
    colour = np.empty((T, H, W, 3), np.uint8)
    views = np.empty((T, *a.cloud_view_size, 3), np.uint8) if a.cloud_view_out else None
    view_rows = np.zeros((T, pointcloud.VIEW_ROW), np.float64)
    f_last = float("nan")
    with common.get_engine(a.source, a.engine, "fp16", None, input_hw=(size, size)) as engine, \
            engine.create_execution_context() as context:
        inputs, outputs, bindings, stream = allocate_buffers(engine)
        d_map, d_f = C.c_void_p(), C.c_void_p()
        try:
            if a.f_px is None and len(outputs) < 2:
                raise SystemExit("this engine has no fov_deg output: pass --f-px")
            for i in range(engine.num_io_tensors):
                context.set_tensor_address(engine.get_tensor_name(i), bindings[i])
            d_fov = outputs[1].device if a.f_px is None else 0
            hip_call("mde_rt_malloc", C.byref(d_map), H * W * 4)
            hip_call("mde_rt_malloc", C.byref(d_f), 4)
            with contextlib.ExitStack() as stack:
                pre = stack.enter_context(DepthProPreprocess(H, W, size))
                dc = stack.enter_context(visualize.DeviceColorize(1, H, W))
                cv = stack.enter_context(pointcloud.DeviceCloudView(1, H, W, a.cloud_view_size, colour=True,
                                                                    step=a.cloud_view_step)) if views is not None \
                    else None
                t0 = time.perf_counter()
                for t in range(T):
                    pre.run(frames[t], inputs[0].device, stream)
                    context.execute_async_v3(stream_handle=stream)
                    dp_postprocess(outputs[0].device, 1, size, size, d_fov, a.f_px or 0.0, d_f.value, d_map.value, H, W,
                                   stream)
                    dc.enqueue(d_map.value, stream, **kw)
                    if cv is not None:  # the frame is still in pre.mem.device; frames after the first keep its camera
                        cv.enqueue(d_map.value, stream, d_photo=pre.mem.device, pitch=3 * W, swap_rb=True,
                                   d_f_px=d_f.value, elev_deg=a.cloud_view_angles[0], azim_deg=a.cloud_view_angles[1],
                                   d_view=cv.views.device if t else 0, out_swap_rb=True)
                        cv.download(stream, sync=False)
                    dc.download(stream)  # the colour frame and its range; the one synchronisation
                    colour[t] = dc.result()[0]
                    if cv is not None:
                        views[t], view_rows[t] = cv.result()[0], cv.view()[0]
                dur_time = time.perf_counter() - t0
                # the last frame's map is still on the card
                dist = visualize.device_distribution(d_map.value, H, W, stream) if kw["mode"] == "robust" else None
                f_host = np.empty(1, np.float32)
                hip_call("mde_rt_memcpy_dtoh_async", f_host.ctypes.data_as(C.c_void_p), d_f, 4, C.c_void_p(stream))
                stream_synchronize(stream)
                f_last = float(f_host[0])
        finally:
            for p in (d_map, d_f):
                if p:
                    hip_call("mde_rt_free", p)
            free_buffers(inputs, outputs, stream)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.save(a.out, colour)
    if views is not None:
        os.makedirs(os.path.dirname(os.path.abspath(a.cloud_view_out)), exist_ok=True)
        np.save(a.cloud_view_out, views)
    avg_time = dur_time / T
    print(f"[MDET] {T} iterations time ({(1, 3, size, size)}): {dur_time:.4f} [sec]")
    print(f"[MDET] Average FPS: {1 / avg_time:.2f} [fps]")
    print(f"[MDET] Average inference time: {avg_time * 1000:.2f} [msec]")
    print(f"[MDET] focal_length : {f_last}")
    print(f"[MDET] color : mode {kw['mode']} (device; {T} frames of {H * W * 3} bytes came back, no float map) -> {a.out}")
    if kw["mode"] == "robust":
        print(visualize.format_distribution(dist))
    if views is not None:
        print(f"[MDET] cloud view (device; {T} previews of {views[0].nbytes} bytes came back, camera of frame 0: "
              f"scale {view_rows[0][pointcloud.V_SCALE]!r}) {H}x{W} step {a.cloud_view_step} -> "
              f"{a.cloud_view_size[0]}x{a.cloud_view_size[1]} {a.cloud_view_out} : valid points "
              f"{[int(r[pointcloud.V_NVALID]) for r in view_rows]}, inside the picture "
              f"{[int(r[pointcloud.V_INSIDE]) for r in view_rows]}")
    return colour


if __name__ == "__main__":
    main()
