"""pointcloud.render_np, the numpy restatement of mde_op_cloud_view's contract (include/mde.h), on the CPU:
against hand-written pictures on the degenerate maps, against the reference's core/viz.py:render_points
through the recorded pictures of tests/golden/cloud_view_cases.npz (written by
tests/golden/make_cloud_view_golden.py), and its centre and span against np.median / np.percentile.

Measured here ("Point-cloud preview"):
  differing pixels against the reference's pictures, per scene of cloud_view_cases.GOLDEN: 0, 0, 0, 0, 0
  worst relative difference of the centre from np.median over the scenes: 0 in all five (the lerp
  a + (b - a) * 0.5 and np.median's (a + b) / 2 can differ by a rounding at an even count; here they do not)
  worst relative difference of the span from np.percentile(..., 99) of the float64 values: 5.6e-8 (5.6e-8,
  3.8e-8, 3.8e-8, 2.9e-8, 9.3e-9), the float32 rounding of |x1|, |y2| (half an ulp, 6.0e-8, bounds it)
"""

import os

import numpy as np
import pytest

import cloud_view_cases as cases

from monocular_depth_estimation_trt_amd import _lib, pointcloud as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud_view_cases.npz")
BG = np.array(pc.VIEW_BG, np.uint8)

# the measured worst cases (module docstring) with the factor-4 margin
CENTRE_RTOL = 4 * 0.0
SPAN_RTOL = 4 * 5.6e-8


def test_new_symbols_are_bound():
    assert "mde_op_cloud_view" in _lib.PROTOTYPES and "mde_op_cloud_view_ws_bytes" in _lib.PROTOTYPES
    assert _lib._RESTYPE["mde_op_cloud_view_ws_bytes"] is _lib.c_size_t
    assert len(_lib.PROTOTYPES["mde_op_cloud_view"]) == 27


def test_view_trig_is_the_reference_s():
    ca, sa, ce, se = pc.view_trig(-18.0, 24.0)
    a, e = np.deg2rad(24.0), np.deg2rad(-18.0)
    assert (ca, sa, ce, se) == (np.cos(a), np.sin(a), np.cos(e), np.sin(e))
    assert pc.view_trig(0.0, 0.0) == (1.0, 0.0, 1.0, 0.0)


def test_all_invalid_draws_the_background():
    z, cam = cases.degenerate("all_invalid")
    pic, row = pc.render_np(z, *cam, size=(7, 9), photo=cases.colours(9, 5))
    assert (pic == BG).all()
    assert row.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 0.46 * 7, 0.0, 0.0]
    pic, _ = pc.render_np(z, *cam, size=(2, 3), bg=(1, 2, 3))
    assert pic.tolist() == [[[1, 2, 3]] * 3] * 2


@pytest.mark.parametrize("angles", cases.ANGLES)
def test_one_valid_sample_sits_in_the_middle(angles):
    """The centre is the sample itself, the span falls back to 1.0, rint(0 + 9 / 2) = 4 and rint(7 / 2) = 4
    (half to even both times)."""
    z, cam = cases.degenerate("one_valid")
    col = cases.colours(9, 5)
    pic, row = pc.render_np(z, *cam, size=(7, 9), elev_deg=angles[0], azim_deg=angles[1], photo=col)
    want = np.empty((7, 9, 3), np.uint8)
    want[:] = BG
    want[4, 4] = col[4, 1]
    assert np.array_equal(pic, want)
    rec = pc.unproject_np(z, *cam)[4 * 5 + 1]
    assert row.tolist() == [1.0, float(rec["x"]), float(rec["y"]), 2.5, 1.0, 0.46 * 7, 1.0, 0.0]
    grey, _ = pc.render_np(z, *cam, size=(7, 9))
    assert grey[4, 4].tolist() == [200, 200, 200] and (grey.reshape(-1, 3)[:40] == BG).all()


def test_constant_depth_lowest_index_wins_every_pixel():
    """elev = azim = 0 on a plane z = 3: every z2 is 0, so each pixel shows its first sample in row-major
    order.  On a 3 x 3 picture of the 9 x 5 map several samples share each pixel."""
    z, cam = cases.degenerate("constant")
    col = cases.colours(9, 5)
    pic, row = pc.render_np(z, *cam, size=(3, 3), elev_deg=0.0, azim_deg=0.0, photo=col)
    rec = pc.unproject_np(z, *cam)
    c = [np.median(rec[k].astype(np.float64)) for k in "xyz"]
    scale = 0.46 * 3 / row[pc.V_SPAN]
    u = np.rint((rec["x"].astype(np.float64) - c[0]) * scale + 1.5)
    v = np.rint((rec["y"].astype(np.float64) - c[1]) * scale + 1.5)
    want = np.empty((3, 3, 3), np.uint8)
    want[:] = BG
    seen = set()
    for i in range(45):
        if 0 <= u[i] < 3 and 0 <= v[i] < 3 and (v[i], u[i]) not in seen:
            seen.add((v[i], u[i]))
            want[int(v[i]), int(u[i])] = col.reshape(-1, 3)[i]
    assert len(seen) < row[pc.V_INSIDE]  # pixels are shared
    assert np.array_equal(pic, want)
    assert row[pc.V_NVALID] == 45 and row[pc.V_C2] == 3.0


def test_near_point_in_front():
    """Two samples on one pixel: the nearer one is drawn although its index is higher; seen from behind
    (azim = 180) the other one is."""
    z, cam = cases.degenerate("two_on_one_pixel")
    col = cases.colours(9, 5)
    rec = pc.unproject_np(z, *cam)
    a, b = 4 * 5 + 3, 4 * 5 + 4
    assert (rec["x"][a], rec["y"][a], rec["z"][a]) == (0.5, 0.0, 2.0)
    assert (rec["x"][b], rec["y"][b], rec["z"][b]) == (0.5, 0.0, 1.0)
    pic, row = pc.render_np(z, *cam, size=(5, 5), elev_deg=0.0, azim_deg=0.0, photo=col)
    want = np.empty((5, 5, 3), np.uint8)
    want[:] = BG
    want[2, 2] = col[4, 4]
    assert np.array_equal(pic, want)
    assert row.tolist() == [2.0, 0.5, 0.0, 1.5, 1.0, 0.46 * 5, 2.0, 0.0]
    # the same camera turned round (sin(pi) is 1.2e-16, not 0: a span selected there would be of that size)
    pic, _ = pc.render_np(z, *cam, size=(5, 5), elev_deg=0.0, azim_deg=180.0, photo=col, view=row)
    assert pic[2, 2].tolist() == col[4, 3].tolist()


def test_nonfinite_negative_and_overflowing_samples_are_dropped():
    z, cam = cases.degenerate("nonfinite_and_negative")
    zz = np.array(z)
    _, row = pc.render_np(z, *cam, size=(7, 9))
    assert row[pc.V_NVALID] == (np.isfinite(zz) & (zz > 0)).sum() <= 45 - 5
    z, cam = cases.degenerate("x_overflows")
    with np.errstate(over="ignore"):
        rec = pc.unproject_np(z, *cam)
    assert np.isinf(rec["x"]).sum() == 18 and np.isfinite(z).all()
    pic, row = pc.render_np(z, *cam, size=(7, 9), elev_deg=0.0, azim_deg=0.0)
    assert row[pc.V_NVALID] == 45 - 18 and np.isfinite(row).all()
    assert 0 < (pic != BG).any(axis=-1).sum() <= row[pc.V_INSIDE]


def test_step_swap_and_fixed_view():
    h, w = 37, 53
    depth, photo = cases.scene(h, w)
    cam = cases.camera(h, w)
    full, row = pc.render_np(depth, *cam, size=(41, 41), photo=photo)
    swapped, _ = pc.render_np(depth, *cam, size=(41, 41), photo=photo, swap_rb=True)
    hit = (full != BG).any(axis=-1)
    assert np.array_equal(swapped[hit], full[hit][:, ::-1]) and (swapped[~hit] == BG).all() and hit.sum() > 100
    sub, row3 = pc.render_np(depth, *cam, size=(41, 41), photo=photo, step=3)
    d3 = depth[::3, ::3]
    assert row3[pc.V_NVALID] == (np.isfinite(d3) & (d3 > 0)).sum() and sub.shape == (41, 41, 3)
    shown = {tuple(c) for c in sub[(sub != BG).any(axis=-1)]}
    assert shown <= {tuple(c) for c in photo[::3, ::3].reshape(-1, 3)}  # only sampled pixels' colours
    again, row_again = pc.render_np(depth, *cam, size=(41, 41), photo=photo, view=row)
    assert np.array_equal(again, full) and np.array_equal(row_again, row)
    tight = row.copy()
    tight[pc.V_SCALE] *= 8
    _, row_tight = pc.render_np(depth, *cam, size=(41, 41), photo=photo, view=tight)
    assert 0 < row_tight[pc.V_INSIDE] < row[pc.V_INSIDE] / 4 and row_tight[pc.V_NVALID] == row[pc.V_NVALID]


def test_round_half_even_on_the_half_grid():
    z, fx, fy, cx, cy, view = cases.half_grid()
    pic, row = pc.render_np(z, fx, fy, cx, cy, size=(8, 10), elev_deg=0.0, azim_deg=0.0, view=view)
    rec = pc.unproject_np(z, fx, fy, cx, cy)
    ok = np.isfinite(rec["z"])
    x = rec["x"][ok].astype(np.float64) + 5.0
    assert ((x % 1.0) == 0.5).sum() > 10  # ties exist
    want = set()
    for xi, yi in zip(x, rec["y"][ok].astype(np.float64) + 4.0):
        u, v = round(xi), round(yi)  # Python's round is half to even
        if 0 <= u < 10 and 0 <= v < 8:
            want.add((v, u))
    got = {(int(v), int(u)) for v, u in zip(*np.nonzero((pic != BG).any(axis=-1)))}
    assert got == want and row[pc.V_INSIDE] >= len(want)


@pytest.fixture(scope="module")
def rendered():
    """render_np of every golden scene, once."""
    out = {}
    for name, (h, w), size, elev, azim in cases.GOLDEN:
        depth, photo = cases.scene(h, w)
        out[name] = pc.render_np(depth, *cases.camera(h, w), size=size, elev_deg=elev, azim_deg=azim, photo=photo)
    return out


@pytest.mark.parametrize("case", cases.GOLDEN, ids=lambda c: c[0])
def test_parity_with_the_reference_pictures(rendered, case):
    """At most 4 pixels per scene may differ from what the reference's render_points drew (ties between
    equal depths, which its unstable argsort breaks differently)."""
    name, _, size, _, _ = case
    with np.load(GOLDEN) as g:
        ref = g[name]
    pic, row = rendered[name]
    assert ref.shape == pic.shape == (*size, 3) and row[pc.V_NVALID] <= 120000
    diff = int((pic != ref).any(axis=-1).sum())
    print(f"{name}: {diff} of {size[0] * size[1]} pixels differ")
    assert diff <= 4
    assert (ref != BG).any(axis=-1).sum() > 100  # the recorded picture shows a cloud


@pytest.mark.parametrize("case", cases.GOLDEN, ids=lambda c: c[0])
def test_centre_and_span_against_numpy(rendered, case):
    name, (h, w), _, elev, azim = case
    depth, _ = cases.scene(h, w)
    rec = pc.unproject_np(depth, *cases.camera(h, w))
    pts = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1).astype(np.float64)
    pts = pts[np.isfinite(pts).all(axis=1) & (pts[:, 2] > 0)]
    centre = np.median(pts, axis=0)
    row = rendered[name][1]
    diff = np.abs(row[pc.V_C0:pc.V_C2 + 1] - centre)
    rel = np.divide(diff, np.abs(centre), out=np.zeros(3), where=diff > 0)  # an exact 0 median stays 0 / 0 = 0
    ca, sa, ce, se = pc.view_trig(elev, azim)
    p = pts - row[pc.V_C0:pc.V_C2 + 1]
    x1 = ca * p[:, 0] + sa * p[:, 2]
    z1 = -sa * p[:, 0] + ca * p[:, 2]
    y2 = ce * p[:, 1] - se * z1
    span = np.percentile(np.abs(np.stack([x1, y2])), 99.0)
    rel_span = abs(row[pc.V_SPAN] - span) / span
    print(f"{name}: centre rel {rel.max():.3e}, span rel {rel_span:.3e}")
    assert rel.max() <= CENTRE_RTOL
    assert rel_span <= SPAN_RTOL
    assert row[pc.V_SCALE] == 0.46 * min(case[2]) / row[pc.V_SPAN]
