"""Time the robust display range (mde_op_depth_quantiles + mde_op_depth_colorize_ranged) at 1536x1536
and at 518x518, batch 1, and record it (profiles/depth_quantiles.json) against the path it replaces:

  (a) the quantile op alone (eleven kernels), q = {2, 98}, positive_only, sample_cap 200000;
  (b) the device side: (a) + the ranged colour pass, no host read in between;
  (c) the device leg: (b) + the D2H of the colour frame (3 bytes per pixel) and the 64-byte row;
  (d) the replaced path: the D2H of the float map (4 bytes per pixel), then on the host the
      reference's robust_range with np.percentile (validity mask, subsample, percentile), then the
      mode-2 colouring on the device with the D2H of its frame.

    OMP_NUM_THREADS=16 python tools/bench_quantiles.py [--out profiles/depth_quantiles.json]

Every device figure: hipEvents around one enqueue of the leg on one stream, median of `--repeats` after
`--warmup` runs.  Host figures: time.perf_counter, median of `--host-repeats` after 1.  The figures
record what was measured; they set no bar.  Needs the GPU; there is no fallback.
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

Q = (2.0, 98.0)


def host_robust_range(depth):
    """core/viz.py:robust_range of one map, with numpy's percentile."""
    v = depth.astype(np.float64).ravel()
    v = v[np.isfinite(v) & (v > 0)]
    if v.size > vz.SAMPLE_CAP:
        v = v[:: max(1, v.size // vz.SAMPLE_CAP)]
    lo, hi = np.percentile(v, Q)
    return float(lo), float(hi)


def bench_size(h, w, stream, a):
    s = C.c_void_p(stream)
    g = np.random.Generator(np.random.PCG64(20260000 + h))
    depth = np.exp(g.normal(1.0, 0.8, (h, w))).astype(np.float32)  # metres, a long tail as a scene has
    depth[g.random((h, w)) < 0.01] = np.nan
    dmap = HostDeviceMem(h * w, np.float32)
    dmap.host = depth.reshape(-1)
    hip_call("mde_rt_memcpy_htod_async", C.c_void_p(dmap.device), dmap.host.ctypes.data_as(C.c_void_p), dmap.nbytes, s)
    stream_synchronize(stream)
    rec = {"hw": [h, w], "pixels": h * w}
    back = np.empty(h * w, np.float32)

    def d2h():
        hip_call("mde_rt_memcpy_dtoh_async", dmap.host.ctypes.data_as(C.c_void_p), C.c_void_p(dmap.device),
                 dmap.nbytes, s)
        stream_synchronize(stream)

    rec["d2h_float_map"] = dict(host_ms(d2h, 1, a.host_repeats), bytes=int(dmap.nbytes))
    kw = dict(q_percent=Q, positive_only=True, sample_cap=vz.SAMPLE_CAP)
    with vz.DeviceColorize(1, h, w, robust=True) as dc:
        rec["quantile_op"] = device_ms(lambda: dc.quant.enqueue(dmap.device, stream, Q, True, False, False,
                                                                 vz.SAMPLE_CAP), stream, a.warmup, a.repeats)
        rec["device_side"] = device_ms(lambda: dc.enqueue(dmap.device, stream, "robust", **kw), stream, a.warmup,
                                       a.repeats)

        def leg():
            dc.enqueue(dmap.device, stream, "robust", **kw)
            dc.download(stream)

        rec["device_leg"] = dict(device_ms(leg, stream, a.warmup, a.repeats), d2h_bytes=3 * h * w + 64)
        got, got_rng = dc.result()[0].copy(), tuple(float(v) for v in dc.range()[0])
        parts = {}

        def host_range():
            parts["rng"] = host_robust_range(depth)

        rec["host_robust_range_np_percentile"] = host_ms(host_range, 1, a.host_repeats)

        def replaced():
            d2h()
            back[:] = dmap.host
            lo, hi = host_robust_range(back.reshape(h, w))
            dc.enqueue(dmap.device, stream, "fixed", vmin=lo, vmax=hi)
            dc.download(stream)

        rec["device_leg_wall"] = host_ms(leg, 1, a.host_repeats)
        rec["replaced_path"] = host_ms(replaced, 1, a.host_repeats)  # leaves the mode-2 frame in dc.result()
        rec["range_equal"] = bool(got_rng == parts["rng"])
        rec["bytes_equal"] = bool(got.tobytes() == dc.result()[0].tobytes())
        rec["replaced_over_device_leg_wall"] = rec["replaced_path"]["median_ms"] / rec["device_leg_wall"]["median_ms"]
    dmap.free()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1536, 1536, 518, 518], help="h w [h w ...]")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_quantiles.json"))
    a = ap.parse_args(argv)
    name = C.create_string_buffer(256)
    hip_call("mde_rt_device_name", 0, name, 256)
    stream = stream_create()
    rec = {"op": "mde_op_depth_quantiles (csrc/depth_quantiles.hip) + mde_op_depth_colorize_ranged",
           "device": name.value.decode(), "mde_abi": _lib.lib().mde_version(), "batch": 1,
           "cpus": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "method": f"hipEvents around one enqueue of the leg on one stream, median of {a.repeats} after {a.warmup} "
                     f"warm-up runs; host and wall legs time.perf_counter, median of {a.host_repeats} after 1",
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
