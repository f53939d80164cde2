"""Writes tests/golden/cloud_view_cases.npz: the pictures that the reference's core/viz.py:render_points
draws of the scenes in tests/cloud_view_cases.py:GOLDEN (recorded results only).

    python tests/golden/make_cloud_view_golden.py /path/to/reference/checkout

The reference gets the float32 cloud of pointcloud.unproject_np (organized, with the photo's colours), its
own default point_px and background, and each scene's picture size and angles.  core.viz imports cv2 at
module level and render_points uses none of it, so where cv2 is not installed a stub module whose
attributes all read as 0 stands in for it.
"""

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cloud_view_cases as cases  # noqa: E402
from monocular_depth_estimation_trt_amd import pointcloud as pc  # noqa: E402


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return 0


def reference_viz(checkout):
    try:
        import cv2  # noqa: F401
    except ImportError:
        sys.modules["cv2"] = _Stub("cv2")
    sys.path.insert(0, checkout)
    from core import viz
    return viz


def main(argv):
    if len(argv) != 2:
        raise SystemExit(__doc__)
    viz = reference_viz(argv[1])
    out = {}
    for name, (h, w), size, elev, azim in cases.GOLDEN:
        depth, photo = cases.scene(h, w)
        rec = pc.unproject_np(depth, *cases.camera(h, w), photo=photo)
        xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1)
        rgb = np.stack([rec["red"], rec["green"], rec["blue"]], axis=-1)
        out[name] = viz.render_points(xyz, rgb, size=size, elev_deg=elev, azim_deg=azim)
        assert out[name].dtype == np.uint8 and out[name].shape == (*size, 3)
    path = os.path.join(HERE, "cloud_view_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv)
