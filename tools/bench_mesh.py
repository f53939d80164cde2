"""Time mde_op_depth_mesh (csrc/depth_mesh.hip) at the reference's photo size, 2268x3024, batch 1, with
colour, step 1, on the mesh tests' scene (tests/mesh_cases.py) with its blocks scaled up by
`--scene-scale`, and record it (profiles/mesh_2268x3024.json):

  (a) record bytes written per second of the mesh op (with faces, and as the edge-filtered cloud), next
      to the compact point cloud on the same depth map and to mde_op_dp_postprocess at the same output
      size, all in this process -- the comparison is against the compact cloud measured here;
  (b) the host tail the op replaces (D2H of the depth map, then pointcloud.mesh_np) against the device leg
      (kernels + the two counts + D2H of the counted bytes).

    python tools/bench_mesh.py [--out profiles/mesh_2268x3024.json]

Every device figure: hipEvents around one enqueue of the leg on one stream, median of `--repeats` after
`--warmup` runs.  Host figures: time.perf_counter.  Needs the GPU; there is no fallback.  The reference's
own path (utils3d in float64, trimesh) is on none of the machines this runs on and is not measured.
"""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pointcloud import device_ms, host_ms  # noqa: E402
from mesh_cases import raw_scene  # noqa: E402
from monocular_depth_estimation_trt_amd import _lib, pointcloud as pc, postprocess as post  # noqa: E402
from monocular_depth_estimation_trt_amd.common_runtime import (HostDeviceMem, hip_call, stream_create,  # noqa: E402
                                                               stream_destroy, stream_synchronize)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, nargs=2, default=[2268, 3024])
    ap.add_argument("--scene-scale", type=int, default=8, help="the scene's blocks are 7 x 9 times this many pixels")
    ap.add_argument("--edge-rtol", type=float, default=pc.EDGE_RTOL)
    ap.add_argument("--engine-size", type=int, default=1536, help="side of the inverse-depth map the post-process reads")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_2268x3024.json"))
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
    depth = HostDeviceMem(h * w, np.float32)
    depth.host = raw_scene(h, w, a.scene_scale).reshape(-1)
    for m in (inv, photo, depth):
        hip_call("mde_rt_memcpy_htod_async", C.c_void_p(m.device), m.host.ctypes.data_as(C.c_void_p), m.nbytes, s)
    stream_synchronize(stream)
    f_px = float(np.float32(0.8 * w))
    rec = {"op": "mde_op_depth_mesh (csrc/depth_mesh.hip)", "device": name.value.decode(),
           "mde_abi": _lib.lib().mde_version(), "hw": [h, w], "batch": 1, "colour": True, "step": 1,
           "scene": f"tests/mesh_cases.py:raw_scene({h}, {w}, {a.scene_scale})", "edge_rtol": a.edge_rtol,
           "method": f"hipEvents around one enqueue of the leg on one stream, median of {a.repeats} after {a.warmup} "
                     f"warm-up runs; host legs time.perf_counter, median of {a.host_repeats} after 1"}
    kw = dict(d_photo=photo.device, pitch=3 * w, swap_rb=True, fx=f_px)
    with post.DepthProDevicePostprocess(1, size, size, h, w) as pp, pc.DevicePointCloud(1, h, w, colour=True) as cloud, \
            pc.DeviceMesh(1, h, w, colour=True) as mesh, pc.DeviceMesh(1, h, w, colour=True, faces=False) as clean:
        t = device_ms(lambda: post.dp_postprocess(inv.device, 1, size, size, 0, f_px, pp.f_px.device, pp.mem.device,
                                                  h, w, stream), stream, a.warmup, a.repeats)
        rec["dp_postprocess_kernel"] = dict(t, written_bytes=h * w * 4, written_gb_per_s=h * w * 4 / t["median_ms"] / 1e6)
        rows = {}
        t = device_ms(lambda: cloud.enqueue(depth.device, stream, compact=True, **kw), stream, a.warmup, a.repeats)
        cloud.download(stream)
        n = int(cloud.result()[0].shape[0])
        rows["point_cloud_compact"] = dict(t, points=n, written_bytes=n * 15, read_bytes=h * w * 8 + n * 3)
        for key, m in (("depth_mesh", mesh), ("depth_mesh_faces0", clean)):
            t = device_ms(lambda: m.enqueue(depth.device, stream, edge_rtol=a.edge_rtol, **kw), stream, a.warmup,
                          a.repeats)
            m.download(stream)
            v, f = m.result()[0]
            nv, nf = int(v.shape[0]), int(f.shape[0])
            rows[key] = dict(t, vertices=nv, triangles=nf, written_bytes=nv * 15 + nf * 13,
                             scratch_written_bytes=h * w + nv * 4, depth_read_bytes=h * w * 4 + nv * 4)
        base = rows["point_cloud_compact"]["written_bytes"] / rows["point_cloud_compact"]["median_ms"]
        for r in rows.values():
            r["written_gb_per_s"] = r["written_bytes"] / r["median_ms"] / 1e6
            r["of_compact_cloud_rate"] = r["written_bytes"] / r["median_ms"] / base
            r["of_compact_cloud_bytes"] = r["written_bytes"] / rows["point_cloud_compact"]["written_bytes"]
        rows["depth_mesh"]["expected_at_least"] = 0.5
        rows["depth_mesh"]["meets_expectation"] = bool(rows["depth_mesh"]["of_compact_cloud_rate"] >= 0.5)
        rec["kernels"] = rows

        def leg():
            mesh.enqueue(depth.device, stream, edge_rtol=a.edge_rtol, **kw)
            mesh.download(stream)

        rec["device_leg"] = dict(device_ms(leg, stream, a.warmup, a.repeats),
                                 d2h_bytes=rows["depth_mesh"]["written_bytes"] + 8)
        dev_v, dev_f = (x.tobytes() for x in mesh.result()[0])
        # the host tail it replaces, from the same device depth map
        z = np.empty(h * w, np.float32)
        img = photo.host.reshape(h, w, 3)
        parts = {}

        def d2h():
            hip_call("mde_rt_memcpy_dtoh_async", z.ctypes.data_as(C.c_void_p), C.c_void_p(depth.device), z.nbytes, s)
            stream_synchronize(stream)

        def mesh_np():
            parts["mesh"] = pc.mesh_np(z.reshape(h, w), f_px, f_px, w / 2, h / 2, photo=img, swap_rb=True,
                                       edge_rtol=a.edge_rtol)

        def tail():
            d2h()
            mesh_np()

        rec["host_tail"] = {"d2h_depth": dict(host_ms(d2h, 1, a.host_repeats), bytes=int(z.nbytes)),
                            "mesh_np": host_ms(mesh_np, 1, a.host_repeats), "total": host_ms(tail, 1, a.host_repeats),
                            "cpus": len(os.sched_getaffinity(0)), "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}
        flags = parts["mesh"][2]
        rec["edge_share"] = float(((flags & pc.F_EDGE) != 0).mean())
        rec["kept_quad_share"] = float(((flags & pc.F_QUAD) != 0).sum() / ((h - 1) * (w - 1)))
        rec["device_equals_host_bytes"] = bool(parts["mesh"][0].tobytes() == dev_v and parts["mesh"][1].tobytes() == dev_f)
        rec["host_tail_over_device_leg"] = rec["host_tail"]["total"]["median_ms"] / rec["device_leg"]["median_ms"]
    for m in (inv, photo, depth):
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
