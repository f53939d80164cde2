"""Seeded scenes and degenerate maps for the point-cloud preview (mde_op_cloud_view), shared by
tests/test_cloud_view_cpu.py, tests/test_gpu_cloud_view.py and tests/golden/make_cloud_view_golden.py.

Everything is cached and read-only: a test that changes a map copies it first."""

import functools

import numpy as np

# (name, depth map h x w, picture out_h x out_w, elev, azim): the scenes whose reference pictures
# tests/golden/cloud_view_cases.npz records.  The last one has 112 368 valid points, under the reference's
# thinning threshold of 120 000
GOLDEN = (("s60x80", (60, 80), (320, 420), -18.0, 24.0),
          ("s200x300", (200, 300), (320, 420), -18.0, 24.0),
          ("s200x300_small", (200, 300), (64, 80), -18.0, 24.0),
          ("s37x53_front", (37, 53), (41, 41), 0.0, 0.0),
          ("s300x390_turned", (300, 390), (96, 128), 30.0, -50.0))

ANGLES = ((-18.0, 24.0), (0.0, 0.0), (30.0, -50.0), (90.0, 0.0))


def camera(h, w):
    """fx, fy, cx, cy of the scenes."""
    return 0.9 * w, 0.9 * w, w / 2, h / 2


@functools.lru_cache(maxsize=None)
def scene(h, w, seed=0):
    """(depth float32 [h, w], photo uint8 [h, w, 3]): a tilted floor with a ripple and a step at the
    middle column, 3 % of the pixels NaN and 1 % of them 0, random colours so that a wrong winner shows."""
    rng = np.random.Generator(np.random.PCG64(seed * 1000003 + h * 1009 + w))
    y, x = np.mgrid[0:h, 0:w]
    depth = 2.0 + 1.5 * y / h + 0.8 * np.sin(6.0 * x / w) + 1.2 * (x > w // 2) + rng.normal(0.0, 0.01, (h, w))
    depth = depth.astype(np.float32)
    r = rng.random((h, w))
    depth[r < 0.03] = np.nan
    depth[(r >= 0.03) & (r < 0.04)] = 0.0
    photo = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    depth.setflags(write=False)
    photo.setflags(write=False)
    return depth, photo


@functools.lru_cache(maxsize=None)
def colours(h, w, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed * 7919 + h * 131 + w))
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _ro(z):
    z = np.ascontiguousarray(z, dtype=np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def degenerate(name, h=9, w=5):
    """(depth [h, w], (fx, fy, cx, cy)) per degenerate case."""
    z = np.full((h, w), np.nan, np.float32)
    cam = camera(h, w)
    if name == "all_invalid":
        z[::2] = 0.0
        z[0, 0], z[1, 1], z[2, 2] = np.inf, -np.inf, -3.0
    elif name == "one_valid":
        z[h // 2, w // 3] = 2.5
    elif name == "constant":        # with elev = azim = 0 every z2 is equal: the lowest index wins every pixel
        z[:] = 3.0
    elif name == "two_on_one_pixel":
        # the reference's "near point in front": with fx = 4 and integer cx, cy the samples (cy, cx + 1) at
        # z = 2 and (cy, cx + 2) at z = 1 both have X = 0.5, Y = 0 exactly, so at elev = azim = 0 they share
        # a pixel; the second is nearer and has the higher index
        cam = (4.0, 4.0, float(w // 2), float(h // 2))
        z[h // 2, w // 2 + 1] = 2.0
        z[h // 2, w // 2 + 2] = 1.0
    elif name == "nonfinite_and_negative":
        z[:] = scene(h, w, seed=3)[0]
        flat = z.reshape(-1)
        for i, bad in zip((1, 7, 11, 20, flat.size - 1), (np.inf, -np.inf, -1.0, -0.0, np.inf)):
            flat[i] = bad
    elif name == "x_overflows":     # X = xn * z overflows float32 at the borders: those samples are invalid
        cam = (1.0, 1.0, w / 2, h / 2)
        z[:] = 2.0
        z[:, 0] = z[:, -1] = 3.0e38  # |xn| >= 1.5: X is +-inf
        z[h // 2, w // 2] = 3.0e38   # |xn|, |yn| <= 0.5: X, Y stay finite, the sample is valid and far away
    else:
        raise KeyError(name)
    return _ro(z), cam


DEGENERATE = ("all_invalid", "one_valid", "constant", "two_on_one_pixel", "nonfinite_and_negative", "x_overflows")


@functools.lru_cache(maxsize=None)
def half_grid(h=9, w=8):
    """(depth, fx, fy, cx, cy, view row) whose X and Y are exact multiples of 0.5: fx = fy = 2, integer
    cx, cy, depth 1 or 2, so X = (u - cx) / 2 * z.  With centre 0, scale 1 and elev = azim = 0,
    x1 * scale + out_w / 2 lands exactly on k + 0.5 for half of the samples and round-half-even decides."""
    rng = np.random.Generator(np.random.PCG64(99))
    z = rng.integers(1, 3, (h, w)).astype(np.float32)
    z[0, 0] = np.nan
    view = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0])
    return _ro(z), 2.0, 2.0, float(w // 2), float(h // 2), view
