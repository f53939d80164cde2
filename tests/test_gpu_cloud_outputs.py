"""Every cloud output in one driver run: --ply, --mesh and --cloud-view together through pointcloud.py's one
stage (run_cloud_outputs: the photo uploaded once, the three ops in turn on the map the post-process left
on the device), held to the same numpy restatements as the single-option driver tests.

The photo is 60 x 80 and --ply-step 2 samples a 30 x 40 grid: one 1024-sample tile and a partial second
one, and a ragged mesh mark tile -- the shapes at which a wrong grid or camera hand-over shows.
"""

import numpy as np
import pytest

import cloud_view_cases as cases
from test_gpu_cloud_view import driver_picture
from test_gpu_mesh import check_driver_cloud as check_driver_filtered_cloud, check_driver_mesh, spread_quantile
from test_gpu_pointcloud import check_driver_cloud

from monocular_depth_estimation_trt_amd import pointcloud as pc

pytestmark = pytest.mark.gpu

SIZE = (48, 64)


def outputs(td):
    return ["--ply", str(td / "c.ply"), "--ply-step", "2", "--mesh", str(td / "m.ply"), "--cloud-view",
            str(td / "v.npy"), "--cloud-view-size", str(SIZE[0]), str(SIZE[1])]


def one_line_each(out):
    for what in ("point cloud", "mesh", "cloud view"):
        assert sum(l.startswith(f"[MDET] {what} (device, ") for l in out.splitlines()) == 1, (what, out)


def check_outputs(td, depth, f_px, bgr, z_lo, z_hi):
    cloud = check_driver_cloud(td / "c.ply", depth, f_px, bgr, 2, z_lo, z_hi)
    v, t, _ = check_driver_mesh(td / "m.ply", depth, f_px, bgr, 1, z_lo, z_hi, pc.EDGE_RTOL)
    want, row = driver_picture(depth, f_px, bgr, size=SIZE)
    got = np.load(td / "v.npy")
    assert got.shape == (*SIZE, 3) and got.tobytes() == want.tobytes()
    return cloud, v, t, row


@pytest.fixture(scope="module")
def photo(tmp_path_factory):
    td = tmp_path_factory.mktemp("cloud_outputs")
    bgr = cases.colours(60, 80)
    np.save(td / "src.npy", bgr)
    return td, bgr


def test_dav2_every_cloud_output_in_one_run(gpu, photo, capsys):
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    td, bgr = photo
    args = ["--source", "synthetic:vits:metric:1234", "--engine", str(td / "dav2_fp16.mdeng"), "--iterations", "2",
            "--warmup", "1", "--image", str(td / "src.npy"), "--out-dir", str(td / "bench"), "--f-px", "70"]
    depth = run.main(args + outputs(td))
    out = capsys.readouterr().out
    one_line_each(out)
    cloud, v, t, row = check_outputs(td, depth, 70.0, bgr, 1e-3, 1e3)
    assert cloud.shape == (30 * 40,) and "1200 points" in out  # clamped into the range by the post-process
    assert f"{v.shape[0]} vertices, {t.shape[0]} triangles" in out
    assert f"{int(row[pc.V_NVALID])} valid points, {int(row[pc.V_INSIDE])} inside the picture" in out
    # --ply-edge-rtol: the edge-filtered cloud, through the mesh op without faces, in the same stage
    rtol = spread_quantile(depth, 2, 0.5)
    depth2 = run.main(args + outputs(td) + ["--ply-edge-rtol", repr(float(rtol))])
    out = capsys.readouterr().out
    one_line_each(out)
    assert np.array_equal(depth2, depth)
    filtered = check_driver_filtered_cloud(td / "c.ply", depth, 70.0, bgr, 2, 1e-3, 1e3, rtol)
    assert 0 < filtered.shape[0] < 30 * 40 and f"{filtered.shape[0]} points" in out


def test_depth_pro_every_cloud_output_in_one_run(gpu, photo, capsys):
    """With the focal length the post-process predicted, read by the three ops from device memory."""
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    td, bgr = photo
    depth, f_px = run.main(["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(td / "dp_fp16.mdeng"),
                            "--iterations", "2", "--warmup", "1", "--image", str(td / "src.npy"), "--out-dir",
                            str(td / "bench")] + outputs(td))
    out = capsys.readouterr().out
    one_line_each(out)
    cloud, v, t, row = check_outputs(td, depth, np.float32(f_px), bgr, 1e-4, 1e4)
    assert f"{cloud.shape[0]} points" in out and f"{v.shape[0]} vertices, {t.shape[0]} triangles" in out
    assert f"{int(row[pc.V_NVALID])} valid points, {int(row[pc.V_INSIDE])} inside the picture" in out
    lines = [l.split(" (")[0] for l in out.splitlines() if l.startswith("[MDET] ")]
    order = [lines.index(f"[MDET] {w}") for w in ("point cloud", "mesh", "cloud view", "postprocess")]
    assert order == sorted(order), lines  # each output prints its own line, before the post-process's
