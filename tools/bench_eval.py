"""Time mde_op_depth_eval (csrc/depth_eval.hip) at 768x1024 and at the reference's photo size,
2268x3024, batch 1, every policy, and record it (profiles/depth_eval.json):

  (a) the device leg: hipEvents around one DeviceEval.enqueue (four kernels), and around enqueue +
      the 128-byte download, with the bytes read per second (9 bytes per pixel, read twice);
  (b) evaluate.score_np, the numpy float64 restatement, on the host for the same image -- what a
      sweep would run after copying the map back;
  (c) the D2H copy of the depth map that scoring on the device replaces;
  (d) mde_op_depth_postprocess at the same output size in the same process, the project's existing
      bandwidth-bound kernel at that size, as a yardstick.

    OMP_NUM_THREADS=16 python tools/bench_eval.py [--out profiles/depth_eval.json]

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
from monocular_depth_estimation_trt_amd import _lib, evaluate as ev, postprocess as post  # noqa: E402
from monocular_depth_estimation_trt_amd.common_runtime import (HostDeviceMem, hip_call, stream_create,  # noqa: E402
                                                               stream_destroy, stream_synchronize)

CASES = (("none", False, "metric"), ("scale", False, "metric"), ("scale_shift", True, "inverse"),
         ("scale_shift", False, "depth"))


def bench_size(h, w, stream, a):
    s = C.c_void_p(stream)
    c = ev.synthetic_gt_case(h, w, 20260000 + h)
    engine_hw = (518, 518)
    small = HostDeviceMem(engine_hw[0] * engine_hw[1], np.float32)
    small.host = np.random.Generator(np.random.PCG64(1)).uniform(0.5, 20.0, small.host.size).astype(np.float32)
    pred = HostDeviceMem(h * w, np.float32)
    hip_call("mde_rt_memcpy_htod_async", C.c_void_p(small.device), small.host.ctypes.data_as(C.c_void_p),
             small.nbytes, s)
    rec = {"hw": [h, w], "pixels": h * w, "read_bytes": 2 * 9 * h * w, "policies": {}}
    with post.DevicePostprocess(1, *engine_hw, h, w) as pp, ev.DeviceEval(1, h, w) as de:
        de.upload_gt(c["gt"], c["mask"], stream)
        t = device_ms(lambda: post.resize_clamp(small.device, 1, *engine_hw, pp.mem.device, h, w, stream=stream),
                      stream, a.warmup, a.repeats)
        rec["depth_postprocess_kernel"] = dict(t, written_bytes=4 * h * w,
                                               written_gb_per_s=4 * h * w / t["median_ms"] / 1e6)

        def d2h():
            hip_call("mde_rt_memcpy_dtoh_async", pp.mem.host.ctypes.data_as(C.c_void_p), C.c_void_p(pp.mem.device),
                     pp.mem.nbytes, s)
            stream_synchronize(stream)

        rec["d2h_depth_map"] = dict(host_ms(d2h, 1, a.host_repeats), bytes=int(pp.mem.nbytes))
        for policy, inverse, kind in CASES:
            pred.host = c[kind].reshape(-1)
            hip_call("mde_rt_memcpy_htod_async", C.c_void_p(pred.device), pred.host.ctypes.data_as(C.c_void_p),
                     pred.nbytes, s)
            stream_synchronize(stream)
            kw = dict(pred_is_inverse=inverse, fit_finite_only=policy == "scale", max_depth=a.max_depth)
            kernels = device_ms(lambda: de.enqueue(pred.device, stream, policy, **kw), stream, a.warmup, a.repeats)

            def leg():
                de.enqueue(pred.device, stream, policy, **kw)
                de.download(stream)

            leg_t = device_ms(leg, stream, a.warmup, a.repeats)
            got = de.result()[0]
            parts = {}

            def host():
                parts["r"] = ev.score_np(c[kind], c["gt"], c["mask"], policy, inverse, policy == "scale", a.max_depth)

            host_t = host_ms(host, 1, a.host_repeats)
            want = parts["r"]
            worst = max(abs(got[k] - want[k]) / abs(want[k]) for k in ("abs_rel", "rmse", "log10", "orientation"))
            rec["policies"][f"{policy}{'_inverse' if inverse else ''}"] = {
                "kernels": dict(kernels, read_gb_per_s=rec["read_bytes"] / kernels["median_ms"] / 1e6),
                "device_leg": dict(leg_t, d2h_bytes=128),
                "host_score_np": host_t,
                "host_over_device_leg": host_t["median_ms"] / leg_t["median_ms"],
                "device_leg_shorter_than_host": bool(leg_t["median_ms"] < host_t["median_ms"]),
                "n": got["n"], "counts_equal": bool(got["n"] == want["n"] and got["n_fit"] == want["n_fit"]),
                "deltas_equal": bool(all(got[k] == want[k] for k in ("delta1", "delta2", "delta3"))),
                "worst_relative_difference": worst}
    for m in (small, pred):
        m.free()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[768, 1024, 2268, 3024], help="h w [h w ...]")
    ap.add_argument("--max-depth", type=float, default=15.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_eval.json"))
    a = ap.parse_args(argv)
    name = C.create_string_buffer(256)
    hip_call("mde_rt_device_name", 0, name, 256)
    stream = stream_create()
    rec = {"op": "mde_op_depth_eval (csrc/depth_eval.hip)", "device": name.value.decode(),
           "mde_abi": _lib.lib().mde_version(), "batch": 1, "max_depth": a.max_depth,
           "cpus": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "method": f"hipEvents around one enqueue of the leg on one stream, median of {a.repeats} after {a.warmup} "
                     f"warm-up runs; host legs time.perf_counter, median of {a.host_repeats} after 1",
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
