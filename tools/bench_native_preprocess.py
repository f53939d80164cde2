"""Time the native profile's pre-process (mde_op_resize_cubic_f_norm,
csrc/preprocess_cubic.hip) at the reference's photo size: 2268x3024 -> 518x700
in float (depth_anything_ac) and -> 518x686 in double (depth_anything_v2), and
record it (profiles/native_preprocess.json).

    python tools/bench_native_preprocess.py [--out profiles/native_preprocess.json]

Per model: `--warmup` enqueues, then `--repeats` times ONE enqueue between two
hipEvents, stream synchronized after each; the figure is the median (the
latency of one isolated launch as the events see it, not the rate of a
saturated stream).  The device leg -- NativePreprocess.run: the photo staged
into pinned memory, its H2D copy and the kernel -- is timed the same way, and
preprocess_native_host (numpy) with the wall clock, median of `--host-repeats`.
These figures record what was measured; they set no bar.  Needs the GPU; there
is no fallback.
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

from monocular_depth_estimation_trt_amd import _lib, preprocess as pre  # noqa: E402
from monocular_depth_estimation_trt_amd.common_runtime import (EventPair, HostDeviceMem, hip_call,  # noqa: E402
                                                               stream_create, stream_destroy, stream_synchronize)


def event_timed(fn, stream, warmup, repeats):
    for _ in range(warmup):
        fn()
    stream_synchronize(stream)
    us = []
    for _ in range(repeats):
        with EventPair(stream) as ev:
            fn()
            ev.stop()
            stream_synchronize(stream)
            us.append(ev.ms() * 1e3)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--src-hw", type=int, nargs=2, default=[2268, 3024])
    ap.add_argument("--target", type=int, default=518)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_preprocess.json"))
    a = ap.parse_args(argv)
    sh, sw = a.src_hw
    name = C.create_string_buffer(256)
    hip_call("mde_rt_device_name", 0, name, 256)
    stream = stream_create()
    photo = np.random.Generator(np.random.PCG64(0)).integers(0, 256, size=(sh, sw, 3), dtype=np.uint8)
    rec = {"op": "cv2 float INTER_CUBIC keep-ratio resize + standardise (csrc/preprocess_cubic.hip, "
                 "resize_cubic_f_norm_kernel)", "device": name.value.decode(), "mde_abi": _lib.lib().mde_version(),
           "src_hw": [sh, sw], "target": a.target, "batch": 1,
           "method": f"hipEvents around one enqueue, stream synchronized after each, median of {a.repeats} after "
                     f"{a.warmup} warm-ups; host: time.perf_counter, median of {a.host_repeats}", "models": {}}
    for model in ("depth_anything_ac", "depth_anything_v2"):
        with pre.NativePreprocess(sh, sw, model, target=a.target) as npp:
            oh, ow = npp.dst
            dst = HostDeviceMem(3 * oh * ow, np.float32)
            npp.run(photo, dst.device, stream)  # leaves the photo on the device for the kernel-only timing
            stream_synchronize(stream)
            kernel = event_timed(lambda: npp.run_device(npp.mem.device, 3 * sw, dst.device, stream), stream,
                                 a.warmup, a.repeats)
            leg = event_timed(lambda: npp.run(photo, dst.device, stream), stream, a.warmup, a.repeats)
            dst.free()
        host = []
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            pre.preprocess_native_host(photo, model, a.target)
            host.append((time.perf_counter() - t0) * 1e3)
        rec["models"][model] = {"dst_hw": [oh, ow], "working_type": "float64" if npp.wide else "float32",
                                "kernel": kernel, "device_leg_h2d_plus_kernel": leg,
                                "photo_bytes": int(photo.nbytes), "written_bytes": 3 * oh * ow * 4,
                                "host_numpy_ms": {"median": statistics.median(host), "min": min(host)}}
    stream_destroy(stream)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
