"""Time mde_op_resize_u8 / mde_op_resize_u8_norm (csrc/preprocess.hip) at the
reference's photo size, 2268x3024 -> 518x518, with hipEvents, and record it
next to the bytes the kernel has to touch (profiles/preprocess_resize_u8.json).

    python tools/bench_preprocess.py [--out profiles/preprocess_resize_u8.json]

Per output: `--warmup` launches, then `--repeats` windows of `--launches`
back-to-back launches between two events; the figure is the median window
divided by its launch count (so it includes the launch gap of a saturated
stream, not the latency of one isolated launch).  The H2D copy of the frame
(pinned, one copy per event pair) is timed the same way.  Needs the GPU; there
is no fallback.
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monocular_depth_estimation_trt_amd import _lib, preprocess as pre  # noqa: E402
from monocular_depth_estimation_trt_amd.common_runtime import (HostDeviceMem, hip_call, stream_create,  # noqa: E402
                                                               stream_destroy, stream_synchronize)


def touched_bytes(sh, sw, oh, ow, out_bytes_per_value):
    """Distinct source bytes any tap reads (not rounded to cache lines), and the bytes written."""
    x0, x1, _, _ = pre._axis_table(ow, sw, True)
    y0, y1, _, _ = pre._axis_table(oh, sh, False)
    cols = np.union1d(x0, x1).size
    rows = np.union1d(y0, y1).size
    return {"source_tap_bytes": int(rows * cols * 3), "source_frame_bytes": int(sh * sw * 3),
            "written_bytes": int(oh * ow * 3 * out_bytes_per_value),
            "lut_bytes": 3 * 256 * 4 if out_bytes_per_value == 4 else 0}


def windows(fn, stream, warmup, repeats, launches):
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        hip_call("mde_rt_event_create", C.byref(e))
    for _ in range(warmup):
        fn()
    stream_synchronize(stream)
    per = []
    for _ in range(repeats):
        hip_call("mde_rt_event_record", ev[0], C.c_void_p(stream))
        for _ in range(launches):
            fn()
        hip_call("mde_rt_event_record", ev[1], C.c_void_p(stream))
        stream_synchronize(stream)
        ms = C.c_float()
        hip_call("mde_rt_event_elapsed_ms", C.byref(ms), ev[0], ev[1])
        per.append(ms.value * 1e3 / launches)
    for e in ev:
        hip_call("mde_rt_event_destroy", e)
    return {"median_us": statistics.median(per), "min_us": min(per), "max_us": max(per)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--src-hw", type=int, nargs=2, default=[2268, 3024])
    ap.add_argument("--dst-hw", type=int, nargs=2, default=[518, 518])
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--launches", type=int, default=20000)  # ~0.1 s a window
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_resize_u8.json"))
    a = ap.parse_args(argv)
    (sh, sw), (oh, ow) = a.src_hw, a.dst_hw
    name = C.create_string_buffer(256)
    hip_call("mde_rt_device_name", 0, name, 256)
    stream = stream_create()
    frame = HostDeviceMem(sh * sw * 3, np.uint8)
    frame.host = np.random.Generator(np.random.PCG64(0)).integers(0, 256, size=sh * sw * 3, dtype=np.uint8)
    dst = HostDeviceMem(oh * ow * 3, np.float32)
    rec = {"op": "cv2 uint8 INTER_LINEAR stretch (csrc/preprocess.hip)", "device": name.value.decode(),
           "mde_abi": _lib.lib().mde_version(), "src_hw": [sh, sw], "dst_hw": [oh, ow], "batch": 1,
           "method": f"hipEvents around {a.launches} back-to-back launches on one stream, median of {a.repeats} "
                     f"windows after {a.warmup} warm-up launches; us per launch", "outputs": {}}
    s = C.c_void_p(stream)

    def h2d():
        hip_call("mde_rt_memcpy_htod_async", C.c_void_p(frame.device), frame.host.ctypes.data_as(C.c_void_p),
                 frame.nbytes, s)
    t = windows(h2d, stream, 3, a.repeats, 10)
    rec["h2d_frame"] = dict(t, bytes=frame.nbytes, gb_per_s=frame.nbytes / t["median_us"] / 1e3)
    with pre.DevicePreprocess(sh, sw, oh, ow, "depth_anything_v2", output="float32_nchw") as dp_f, \
            pre.DevicePreprocess(sh, sw, oh, ow, "depth_anything_v2", output="uint8_nhwc") as dp_u:
        for key, dp, width in (("uint8_nhwc", dp_u, 1), ("float32_nchw", dp_f, 4)):
            t = windows(lambda: dp.run_device(frame.device, 3 * sw, dst.device, stream), stream, a.warmup,
                        a.repeats, a.launches)
            b = touched_bytes(sh, sw, oh, ow, width)
            moved = b["source_tap_bytes"] + b["written_bytes"] + b["lut_bytes"]
            rec["outputs"][key] = dict(t, **b, touched_bytes=moved, achieved_gb_per_s=moved / t["median_us"] / 1e3)
    frame.free()
    dst.free()
    stream_destroy(stream)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
