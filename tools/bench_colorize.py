"""Time mde_op_depth_colorize (csrc/depth_colorize.hip) at 768x1024 and at the reference's photo size,
2268x3024, batch 1, all three modes, and record it (profiles/depth_colorize.json):

  (a) the kernels alone: hipEvents around one DeviceColorize.enqueue;
  (b) the device leg: enqueue + the D2H of the colour frame (3 bytes per pixel) and its range;
  (c) the D2H copy of the float map (4 bytes per pixel) that colouring on the device replaces;
  (d) visualize.colorize_np, the numpy restatement, on the host for the same map -- what a caller
      would run after copying the map back.

    OMP_NUM_THREADS=16 python tools/bench_colorize.py [--out profiles/depth_colorize.json]

Bytes.  Modes 0 and 1 read the map twice (range pass, colour pass) and write 3 bytes per pixel: 11
bytes per pixel; mode 2 is the colour pass alone, 4 read + 3 written: 7 bytes per pixel.  The rates
are those bytes over the kernels' time, and their fraction of the 8.0 TB/s HBM3E peak and of the
6.29 TB/s a float4 copy reaches on this card; a 27 MB map fits the Infinity Cache, so the second read
of modes 0 and 1 need not come from HBM.

Every device figure: hipEvents around one enqueue of the leg on one stream, median of `--repeats`
after `--warmup` runs.  Host figures: time.perf_counter, median of `--host-repeats` after 1.  The
figures record what was measured; they set no bar.  Needs the GPU; there is no fallback.
"""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pointcloud import device_ms, host_ms  # noqa: E402
from monocular_depth_estimation_trt_amd import _lib, visualize as vz  # noqa: E402
from monocular_depth_estimation_trt_amd.common_runtime import (HostDeviceMem, hip_call, stream_create,  # noqa: E402
                                                               stream_destroy, stream_synchronize)

HBM_PEAK_GBPS = 8000.0
HBM_COPY_GBPS = 6290.0
CASES = (("inverse_auto", {}), ("minmax_u8", {}), ("fixed", {"vmin": 0.5, "vmax": 20.0}))


def bench_size(h, w, stream, a):
    s = C.c_void_p(stream)
    depth = np.random.Generator(np.random.PCG64(20260000 + h)).uniform(0.02, 900.0, (h, w)).astype(np.float32)
    dmap = HostDeviceMem(h * w, np.float32)
    dmap.host = depth.reshape(-1)
    hip_call("mde_rt_memcpy_htod_async", C.c_void_p(dmap.device), dmap.host.ctypes.data_as(C.c_void_p), dmap.nbytes, s)
    stream_synchronize(stream)
    rec = {"hw": [h, w], "pixels": h * w, "modes": {}}

    def d2h():
        hip_call("mde_rt_memcpy_dtoh_async", dmap.host.ctypes.data_as(C.c_void_p), C.c_void_p(dmap.device),
                 dmap.nbytes, s)
        stream_synchronize(stream)

    rec["d2h_float_map"] = dict(host_ms(d2h, 1, a.host_repeats), bytes=int(dmap.nbytes))
    with vz.DeviceColorize(1, h, w) as dc:
        for mode, kw in CASES:
            kernels = device_ms(lambda: dc.enqueue(dmap.device, stream, mode, **kw), stream, a.warmup, a.repeats)

            def leg():
                dc.enqueue(dmap.device, stream, mode, **kw)
                dc.download(stream)

            leg_t = device_ms(leg, stream, a.warmup, a.repeats)
            got = dc.result()[0].copy()
            parts = {}

            def host():
                parts["pic"], _ = vz.colorize_np(depth, mode, **kw)

            host_t = host_ms(host, 1, a.host_repeats)
            moved = (7 if mode == "fixed" else 11) * h * w
            gbps = moved / kernels["median_ms"] / 1e6
            rec["modes"][mode] = {
                "kernels": dict(kernels, bytes_counted=moved, gb_per_s=gbps,
                                fraction_of_hbm_peak=gbps / HBM_PEAK_GBPS,
                                fraction_of_float4_copy_rate=gbps / HBM_COPY_GBPS),
                "device_leg": dict(leg_t, d2h_bytes=int(got.nbytes) + 8),
                "host_colorize_np": host_t,
                "host_over_device_leg": host_t["median_ms"] / leg_t["median_ms"],
                "device_leg_shorter_than_float_map_d2h": bool(leg_t["median_ms"] < rec["d2h_float_map"]["median_ms"]),
                "bytes_equal": bool(got.tobytes() == parts["pic"].tobytes())}
    dmap.free()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[768, 1024, 2268, 3024], help="h w [h w ...]")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_colorize.json"))
    a = ap.parse_args(argv)
    name = C.create_string_buffer(256)
    hip_call("mde_rt_device_name", 0, name, 256)
    stream = stream_create()
    rec = {"op": "mde_op_depth_colorize (csrc/depth_colorize.hip)", "device": name.value.decode(),
           "mde_abi": _lib.lib().mde_version(), "batch": 1,
           "cpus": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "method": f"hipEvents around one enqueue of the leg on one stream, median of {a.repeats} after {a.warmup} "
                     f"warm-up runs; host legs time.perf_counter, median of {a.host_repeats} after 1",
           "bytes": "modes 0 and 1: map read twice + 3 written = 11 per pixel; mode 2: 4 read + 3 written = 7",
           "sizes": [bench_size(h, w, stream, a) for h, w in zip(a.sizes[::2], a.sizes[1::2])]}
    stream_destroy(stream)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
