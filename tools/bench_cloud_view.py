"""Time mde_op_cloud_view (csrc/cloud_view.hip) at the reference's photo size, 2268x3024, batch 1, with
colour, step 1, and record it (profiles/cloud_view_2268x3024.json):

  (a) the device op at the default picture, 320x420, and at 64x80, where about 1300 samples fall on every
      pixel and the 64-bit atomics on one address are at their worst.  The event window is split in two:
      the same enqueue with the camera fixed (view_in: clear, splat, resolve only) is timed on its own, and
      the selection (the planes, the three medians, the pooled 99th percentile, the view row) is the
      difference of the two medians;
  (b) the host path the op replaces, in the same process: D2H of the depth map, then pointcloud.render_np
      (run it with OMP_NUM_THREADS=16).

    OMP_NUM_THREADS=16 python tools/bench_cloud_view.py [--out profiles/cloud_view_2268x3024.json]

Every device figure: hipEvents around one enqueue on one stream, median of `--repeats` after `--warmup`
runs.  Host figures: time.perf_counter.  Needs the GPU; there is no fallback.
"""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pointcloud import device_ms, host_ms  # noqa: E402
from monocular_depth_estimation_trt_amd import _lib, pointcloud as pc  # noqa: E402
from monocular_depth_estimation_trt_amd.common_runtime import (HostDeviceMem, hip_call, stream_create,  # noqa: E402
                                                               stream_destroy, stream_synchronize)


def room(h, w, seed=0):
    """A tilted floor with a ripple and a step, 3 % NaN and 1 % zeros: the scene of the tests, at any size."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:h, 0:w]
    depth = (2.0 + 1.5 * y / h + 0.8 * np.sin(6.0 * x / w) + 1.2 * (x > w // 2) + rng.normal(0.0, 0.01, (h, w)))
    depth = depth.astype(np.float32)
    r = rng.random((h, w))
    depth[r < 0.03] = np.nan
    depth[(r >= 0.03) & (r < 0.04)] = 0.0
    return depth, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, nargs=2, default=[2268, 3024])
    ap.add_argument("--sizes", type=int, nargs="+", default=[320, 420, 64, 80], help="pictures: H W [H W ...]")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_view_2268x3024.json"))
    a = ap.parse_args(argv)
    h, w = a.hw
    sizes = list(zip(a.sizes[::2], a.sizes[1::2]))
    name = C.create_string_buffer(256)
    hip_call("mde_rt_device_name", 0, name, 256)
    stream = stream_create()
    s = C.c_void_p(stream)
    depth_np, photo_np = room(h, w)
    depth = HostDeviceMem(h * w, np.float32)
    depth.host = depth_np.reshape(-1)
    photo = HostDeviceMem(h * w * 3, np.uint8)
    photo.host = photo_np.reshape(-1)
    for m in (depth, photo):
        hip_call("mde_rt_memcpy_htod_async", C.c_void_p(m.device), m.host.ctypes.data_as(C.c_void_p), m.nbytes, s)
    stream_synchronize(stream)
    f_px = 0.9 * w
    rec = {"op": "mde_op_cloud_view (csrc/cloud_view.hip)", "device": name.value.decode(),
           "mde_abi": _lib.lib().mde_version(), "hw": [h, w], "batch": 1, "colour": True, "step": 1,
           "method": f"hipEvents around one enqueue on one stream, median of {a.repeats} after {a.warmup} warm-up "
                     f"runs; the selection is the full enqueue's median minus the fixed-camera enqueue's; host legs "
                     f"time.perf_counter, median of {a.host_repeats} after 1",
           "pictures": {}}
    kw = dict(d_photo=photo.device, pitch=3 * w, swap_rb=True, fx=f_px, out_swap_rb=True)
    for size in sizes:
        with pc.DeviceCloudView(1, h, w, size, colour=True) as cv:
            full = device_ms(lambda: cv.enqueue(depth.device, stream, **kw), stream, a.warmup, a.repeats)
            fixed = device_ms(lambda: cv.enqueue(depth.device, stream, d_view=cv.views.device, **kw), stream,
                              a.warmup, a.repeats)

            def leg():
                cv.enqueue(depth.device, stream, **kw)
                cv.download(stream)
            with_d2h = device_ms(leg, stream, a.warmup, a.repeats)
            row = cv.view()[0].copy()
            dev_pic = cv.result()[0].copy()
            entry = {"enqueue": full, "fixed_camera_clear_splat_resolve": fixed,
                     "selection_ms_by_difference": full["median_ms"] - fixed["median_ms"],
                     "enqueue_and_d2h": dict(with_d2h, d2h_bytes=int(dev_pic.nbytes) + 64),
                     "scratch_bytes": pc.cloud_view_ws_bytes(1, h, w, 1, *size),
                     "valid_points": int(row[pc.V_NVALID]), "inside_the_picture": int(row[pc.V_INSIDE]),
                     "samples_per_pixel": float(row[pc.V_INSIDE]) / (size[0] * size[1])}
            # the host path it replaces, from the same device depth map
            host = np.empty(h * w, np.float32)
            parts = {}

            def d2h():
                hip_call("mde_rt_memcpy_dtoh_async", host.ctypes.data_as(C.c_void_p), C.c_void_p(depth.device),
                         host.nbytes, s)
                stream_synchronize(stream)

            def render():
                parts["pic"], parts["row"] = pc.render_np(host.reshape(h, w), f_px, f_px, w / 2, h / 2, size=size,
                                                          photo=photo_np, swap_rb=True)

            def tail():
                d2h()
                render()

            entry["host_path"] = {"d2h_depth": dict(host_ms(d2h, 1, a.host_repeats), bytes=int(host.nbytes)),
                                  "render_np": host_ms(render, 1, a.host_repeats),
                                  "total": host_ms(tail, 1, a.host_repeats),
                                  "cpus": len(os.sched_getaffinity(0)),
                                  "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}
            entry["device_equals_host_bytes"] = bool(parts["pic"][..., ::-1].tobytes() == dev_pic.tobytes()
                                                     and np.array_equal(parts["row"], row, equal_nan=True))
            entry["host_path_over_device_leg"] = entry["host_path"]["total"]["median_ms"] / with_d2h["median_ms"]
            rec["pictures"]["%dx%d" % size] = entry
    for m in (depth, photo):
        m.free()
    stream_destroy(stream)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
