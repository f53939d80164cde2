"""Time mde_op_point_cloud (csrc/point_cloud.hip) at the reference's photo size, 2268x3024, batch
1, with colour, step 1, and record it (profiles/pointcloud_2268x3024.json):

  (a) bytes written per second of the point-cloud kernels, organized and compact (everything
      valid), next to mde_op_dp_postprocess at the same output size in the same process -- the
      project's existing write-bound kernel;
  (b) the host tail the op replaces (D2H of the depth map, numpy unproject_np in float32, which
      ends in the interleave into PLY vertex records) against the device leg (kernels + D2H of
      the counts and the counted records);
  (c) is the driver's own `[MDET] point cloud` line and is pasted in with --driver-line.

    python tools/bench_pointcloud.py [--out profiles/pointcloud_2268x3024.json]

Every device figure: hipEvents around one enqueue of the leg on one stream, median of `--repeats`
after `--warmup` runs.  Host figures: time.perf_counter, same counts.  Needs the GPU; there is no
fallback.
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monocular_depth_estimation_trt_amd import _lib, pointcloud as pc, postprocess as post  # noqa: E402
from monocular_depth_estimation_trt_amd.common_runtime import (HostDeviceMem, hip_call, stream_create,  # noqa: E402
                                                               stream_destroy, stream_synchronize)


def device_ms(fn, stream, warmup, repeats):
    """fn() enqueues (and may synchronize) on `stream`; ms between two events around it."""
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        hip_call("mde_rt_event_create", C.byref(e))
    per = []
    for i in range(warmup + repeats):
        hip_call("mde_rt_event_record", ev[0], C.c_void_p(stream))
        fn()
        hip_call("mde_rt_event_record", ev[1], C.c_void_p(stream))
        stream_synchronize(stream)
        ms = C.c_float()
        hip_call("mde_rt_event_elapsed_ms", C.byref(ms), ev[0], ev[1])
        if i >= warmup:
            per.append(float(ms.value))
    for e in ev:
        hip_call("mde_rt_event_destroy", e)
    return {"median_ms": statistics.median(per), "min_ms": min(per), "max_ms": max(per)}


def host_ms(fn, warmup, repeats):
    per = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            per.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(per), "min_ms": min(per), "max_ms": max(per)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, nargs=2, default=[2268, 3024])
    ap.add_argument("--engine-size", type=int, default=1536, help="side of the inverse-depth map the post-process reads")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--driver-line", default="", help="(c): the [MDET] point cloud line of a driver run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcloud_2268x3024.json"))
    a = ap.parse_args(argv)
    h, w = a.hw
    size = a.engine_size
    name = C.create_string_buffer(256)
    hip_call("mde_rt_device_name", 0, name, 256)
    stream = stream_create()
    s = C.c_void_p(stream)
    rng = np.random.Generator(np.random.PCG64(0))
    inv = HostDeviceMem(size * size, np.float32)
    inv.host = rng.uniform(0.05, 2.0, size=size * size).astype(np.float32)
    photo = HostDeviceMem(h * w * 3, np.uint8)
    photo.host = rng.integers(0, 256, size=h * w * 3, dtype=np.uint8)
    for m in (inv, photo):
        hip_call("mde_rt_memcpy_htod_async", C.c_void_p(m.device), m.host.ctypes.data_as(C.c_void_p), m.nbytes, s)
    stream_synchronize(stream)
    rec = {"op": "mde_op_point_cloud (csrc/point_cloud.hip)", "device": name.value.decode(),
           "mde_abi": _lib.lib().mde_version(), "hw": [h, w], "batch": 1, "colour": True, "step": 1,
           "method": f"hipEvents around one enqueue of the leg on one stream, median of {a.repeats} after {a.warmup} "
                     f"warm-up runs; host legs time.perf_counter, median of {a.host_repeats} after 1"}
    with post.DepthProDevicePostprocess(1, size, size, h, w) as pp, pc.DevicePointCloud(1, h, w, colour=True) as cloud:
        f_px = 0.8 * w
        written = h * w * 4
        t = device_ms(lambda: post.dp_postprocess(inv.device, 1, size, size, 0, f_px, pp.f_px.device, pp.mem.device,
                                                  h, w, stream), stream, a.warmup, a.repeats)
        rec["dp_postprocess_kernel"] = dict(t, written_bytes=written, written_gb_per_s=written / t["median_ms"] / 1e6)
        base = rec["dp_postprocess_kernel"]["written_gb_per_s"]
        kw = dict(d_photo=photo.device, pitch=3 * w, swap_rb=True, d_f_px=pp.f_px.device)
        written = h * w * 15
        rec["kernels"] = {}
        for mode, compact, share in (("organized", False, 0.5), ("compact_all_valid", True, 1 / 3)):
            t = device_ms(lambda: cloud.enqueue(pp.mem.device, stream, compact=compact, **kw), stream, a.warmup,
                          a.repeats)
            rate = written / t["median_ms"] / 1e6
            rec["kernels"][mode] = dict(t, written_bytes=written, read_bytes=h * w * (3 + 4 * (2 if compact else 1)),
                                        written_gb_per_s=rate, of_dp_postprocess_rate=rate / base,
                                        expected_at_least=share, meets_expectation=bool(rate / base >= share))
        # (b) the device leg: kernels + D2H of the counts and the counted records
        rec["device_leg"] = {}
        for mode, compact in (("organized", False), ("compact_all_valid", True)):
            def leg():
                cloud.enqueue(pp.mem.device, stream, compact=compact, **kw)
                cloud.download(stream)
            rec["device_leg"][mode] = dict(device_ms(leg, stream, a.warmup, a.repeats), d2h_bytes=written + 4)
        points = int(cloud.result()[0].shape[0])
        dev_bytes = cloud.result()[0].tobytes()
        # the host tail it replaces, from the same device depth map
        depth = pp.mem.host
        img = photo.host.reshape(h, w, 3)
        f_host = float(np.float32(f_px))
        parts = {}

        def d2h():
            hip_call("mde_rt_memcpy_dtoh_async", depth.ctypes.data_as(C.c_void_p), C.c_void_p(pp.mem.device),
                     depth.nbytes, s)
            stream_synchronize(stream)

        def unproject():
            parts["rec"] = pc.unproject_np(depth.reshape(h, w), f_host, f_host, w / 2, h / 2, photo=img, swap_rb=True,
                                           compact=True)

        def tail():
            d2h()
            unproject()

        rec["host_tail"] = {"d2h_depth": dict(host_ms(d2h, 1, a.host_repeats), bytes=int(depth.nbytes)),
                            "unproject_np_and_interleave": host_ms(unproject, 1, a.host_repeats),
                            "total": host_ms(tail, 1, a.host_repeats),
                            "cpus": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}
        rec["points"] = points
        rec["device_equals_host_bytes"] = bool(parts["rec"].tobytes() == dev_bytes)
        rec["host_tail_over_device_leg"] = (rec["host_tail"]["total"]["median_ms"]
                                            / rec["device_leg"]["compact_all_valid"]["median_ms"])
    if a.driver_line:
        rec["driver_line"] = a.driver_line
    for m in (inv, photo):
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
