"""Colour frames, the parts that need no GPU: visualize.py's numpy restatement against what
matplotlib drew through the reference's lines (tests/golden/colorize_cases.npz, written by
tests/golden/make_colorize_golden.py), the committed colour tables, the class rules of the
contract, the ABI's argument checks, the drivers' refusals and save_image.  Every comparison of
pictures is exact byte equality."""

import os

import numpy as np
import pytest

import colorize_cases as cc
from conftest import ROOT

CASES = [(r, v) for r in cc.REGIMES for v in cc.VARIANTS]


@pytest.fixture(scope="module")
def vz():
    from monocular_depth_estimation_trt_amd import visualize
    return visualize


@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


def same_range(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


@pytest.mark.parametrize("regime, variant", CASES)
def test_colorize_np_equals_what_matplotlib_drew(vz, regime, variant):
    fx = cc.load_fixture()
    pic, rng = vz.colorize_np(cc.case_input(regime, variant), **cc.case_kwargs(variant))
    want = fx[f"{regime}/{variant}/bgr"]
    assert pic.dtype == np.uint8 and pic.shape == (cc.H, cc.W, 3)
    assert pic.tobytes() == want.tobytes(), int((pic != want).any(axis=-1).sum())
    assert same_range(rng, fx[f"{regime}/{variant}/range"]), (rng, fx[f"{regime}/{variant}/range"])
    rgb, _ = vz.colorize_np(cc.case_input(regime, variant), swap_rb=False, **cc.case_kwargs(variant))
    assert rgb.tobytes() == np.ascontiguousarray(want[..., ::-1]).tobytes()


def test_the_regimes_clip_as_named(vz):
    """Each regime of the fixture is the one its name says: which end of [1/250, 10] clips."""
    c = np.float32(1.0 / 250)
    for regime, (low, high) in {"neither": (False, False), "high": (False, True), "low": (True, False),
                                "both": (True, True)}.items():
        inv = np.float32(1.0) / cc.depth_map(regime)
        assert (inv.min() <= c, inv.max() > 10) == (low, high), regime
        _, (lo, hi) = vz.colorize_np(cc.depth_map(regime), 0)
        assert (lo == c, hi == 10) == (low, high), regime


def test_committed_tables_equal_matplotlib(vz):
    matplotlib = pytest.importorskip("matplotlib")
    from monocular_depth_estimation_trt_amd import colormaps
    for name, table in colormaps.TABLES.items():
        cmap = matplotlib.colormaps[name]
        want = np.array([(np.asarray(cmap(i)[:3]) * 255).astype(np.uint8) for i in range(256)])
        assert table.shape == (256, 3) and table.dtype == np.uint8 and np.array_equal(table, want), name
    assert set(colormaps.TABLES) == {"turbo", "magma"}


def test_the_product_does_not_import_matplotlib():
    for name in ("colormaps.py", "visualize.py"):
        txt = open(os.path.join(ROOT, "monocular_depth_estimation_trt_amd", name)).read()
        assert "import matplotlib" not in txt and "from matplotlib" not in txt, name


def test_lut(vz):
    t = vz.lut("turbo")
    assert t.shape == (257, 3) and t.dtype == np.uint8 and tuple(t[256]) == (0, 0, 0) and tuple(t[0]) == (48, 18, 59)
    assert tuple(vz.lut("magma", vz.BAD_VIZ)[256]) == (60, 60, 66)
    with pytest.raises(ValueError, match="unknown colour map"):
        vz.lut("jet")
    with pytest.raises(ValueError, match="0..255"):
        vz.lut("turbo", (0, 0, 256))
    assert vz.mode_for({"depth_scale": "metric"}) == "inverse_auto"
    assert vz.mode_for({"depth_scale": "relative"}) == "minmax_u8"
    assert vz.mode_for({"depth_scale": "unknown"}) == vz.mode_for({}) == "inverse_auto"
    with pytest.raises(ValueError, match="unknown colour mode"):
        vz.colorize_np(np.ones((2, 2)), "rainbow")
    with pytest.raises(ValueError, match="vmin and vmax"):
        vz.colorize_np(np.ones((2, 2)), "fixed")


def test_class_rules_inverse_auto(vz):
    """depth 0 -> v = +inf -> the top colour; -0 -> -inf -> the bottom colour; NaN -> bad; a negative
    depth is a finite negative v: it takes part in the minimum and draws the bottom colour."""
    x = np.array([[1.0, 2.0, 4.0, 0.0, -0.0, np.nan, -2.0, np.inf, -np.inf]], np.float32)
    idx, (lo, hi) = vz.index_np(x, 0)
    # v = 1, .5, .25, inf, -inf, nan, -.5, 0, -0: vmn = -0.5 -> lo = 1/250; vmx = 1
    assert lo == np.float32(1.0 / 250) and hi == 1.0
    assert list(idx[0, 3:]) == [255, 0, 256, 0, 0, 0] and idx[0, 0] == 255 and 0 < idx[0, 2] < idx[0, 1] < 255
    pic, _ = vz.colorize_np(x, 0)
    t = vz.lut("turbo")[:, ::-1]
    assert np.array_equal(pic[0, 5], t[256]) and np.array_equal(pic[0, 3], t[255]) and np.array_equal(pic[0, 4], t[0])
    # the inverse-input form of the same values gives the same picture
    with np.errstate(all="ignore"):
        pic_inv, _ = vz.colorize_np(np.float32(1.0) / x, 0, map_is_inverse=True)
    assert pic_inv.tobytes() == pic.tobytes()


def test_class_rules_minmax_and_fixed(vz):
    x = np.array([[1.0, 2.0, 3.0, np.nan, np.inf, -np.inf, -1.0, 0.0]], np.float32)
    idx, (mn, mx) = vz.index_np(x, 1)
    assert (mn, mx) == (-1.0, 3.0)
    assert list(idx[0]) == [127, 191, 255, 256, 255, 0, 0, 63]
    idx, (lo, hi) = vz.index_np(x, 2, vmin=0.0, vmax=2.0)
    assert (lo, hi) == (0.0, 2.0) and list(idx[0]) == [128, 255, 255, 256, 256, 256, 0, 0]
    pic, _ = vz.colorize_np(x, 2, vmin=0.0, vmax=2.0, swap_rb=False)
    assert tuple(pic[0, 3]) == vz.BAD_VIZ and tuple(pic[0, 4]) == vz.BAD_VIZ
    # vmax <= vmin: the axis is [vmin, vmin + 1e-6]
    idx, (lo, hi) = vz.index_np(x, 2, vmin=2.0, vmax=1.0)
    assert list(idx[0]) == [0, 0, 255, 256, 256, 256, 0, 0] and lo == 2.0 and hi == np.float32(2.0 + 1e-6)


@pytest.mark.parametrize("mode", [0, 1])
def test_constant_and_all_nan_maps_are_bad(vz, mode):
    pic, rng = vz.colorize_np(np.full((3, 5), 2.5, np.float32), mode)
    assert (pic == 0).all()  # 0 / 0, as matplotlib draws it
    assert rng[0] == rng[1] == (np.float32(0.4) if mode == 0 else 2.5)
    pic, rng = vz.colorize_np(np.full((3, 5), np.nan, np.float32), mode)
    assert (pic == 0).all() and np.isnan(rng).all()
    pic, rng = vz.colorize_np(np.full((3, 5), np.inf if mode else 0.0, np.float32), mode)
    assert (pic == 0).all() and np.isnan(rng).all()  # no finite value: +inf - NaN is NaN too
    if mode == 0:  # the VGGT driver's eps makes a constant map 0 / 1e-6: the bottom colour
        pic, _ = vz.colorize_np(np.full((3, 5), 2.5, np.float32), 0, denom_eps=1e-6, swap_rb=False)
        assert (pic == vz.lut("turbo")[0]).all()


def test_batches_are_ranged_per_image(vz):
    maps = np.stack([cc.depth_map("neither"), cc.depth_map("both")])
    pics, rngs = vz.colorize_np(maps, 0)
    assert pics.shape == (2, cc.H, cc.W, 3) and rngs.shape == (2, 2)
    for i in range(2):
        pic, rng = vz.colorize_np(maps[i], 0)
        assert pics[i].tobytes() == pic.tobytes() and same_range(rngs[i], rng)


def test_header_names_the_tile(vz):
    txt = open(os.path.join(ROOT, "include", "mde.h")).read()
    assert f"#define MDE_DEPTH_COLORIZE_TILE {vz.TILE}" in txt
    for word in ("inverse_auto", "minmax_u8", "lut257x3", "range_out"):
        assert word in txt, word


def test_ws_bytes_is_zero_for_refused_sizes(lib, vz):
    f = lib.mde_op_depth_colorize_ws_bytes
    tiles = -(-600 * 800 // vz.TILE)
    assert f(1, 600, 800) == (tiles * 2 + 2) * 4 and f(3, 600, 800) == 3 * (tiles * 2 + 2) * 4
    assert f(1, 1, 1) == 16
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -3), (65536, 8, 8), (1, 46341, 46341),
                (1, 1 << 16, 1 << 15), (1, 2, (1 << 30) - 128)):
        assert f(*bad) == 0, bad
    assert f(65535, 1, 1) == 65535 * 16
    assert f(1, 1, (1 << 31) - 257) > 0  # the largest plane the op takes
    with pytest.raises(ValueError, match="does not take"):
        vz.DeviceColorize(1, 0, 8)
    with pytest.raises(ValueError, match="does not take"):
        vz.DeviceColorize(70000, 8, 8)


def test_argument_checks_answer_without_a_gpu(lib):
    """MDE_ERR_ARG before any device call (the pointers are never dereferenced)."""
    p, big = 4096, 1 << 30
    nan = float("nan")

    def err(msg, map_=p, batch=1, h=8, w=8, mode=0, inv=0, eps=0.0, vmin=0.0, vmax=1.0, lut=p, swap=1, out=p, rng=p,
            ws=p, ws_bytes=big):
        rc = lib.mde_op_depth_colorize(map_, batch, h, w, mode, inv, eps, vmin, vmax, lut, swap, out, rng, ws,
                                       ws_bytes, None)
        assert rc == 1, (rc, lib.mde_last_error())
        assert msg in lib.mde_last_error(), lib.mde_last_error()

    err(b"null", map_=None)
    err(b"null", out=None)
    err(b"null", lut=None)
    err(b"positive", batch=0)
    err(b"positive", h=0)
    err(b"positive", w=-8)
    err(b"mode", mode=3)
    err(b"mode", mode=-1)
    err(b"denom_eps is NaN", eps=nan)
    err(b"denom_eps is NaN", eps=nan, mode=2)
    err(b"vmin or vmax is NaN", mode=2, vmin=nan)
    err(b"vmin or vmax is NaN", mode=2, vmax=nan)
    err(b"2^31 - 256", h=1 << 16, w=1 << 15)
    err(b"2^31 - 256", h=1, w=(1 << 31) - 256)
    err(b"batch > 65535", batch=65536)
    for mode in (0, 1):
        err(b"mde_op_depth_colorize_ws_bytes", mode=mode, ws=None)
        err(b"mde_op_depth_colorize_ws_bytes", mode=mode, ws_bytes=15)
        err(b"mde_op_depth_colorize_ws_bytes", mode=mode, h=600, w=800, ws_bytes=(118 * 2 + 2) * 4 - 1)
        err(b"aligned", mode=mode, ws=p + 2)
    err(b"aligned", rng=p + 2)


def test_driver_options_are_checked_before_an_engine_is_built(vz, tmp_path):
    import argparse
    from monocular_depth_estimation_trt_amd import spec
    from monocular_depth_estimation_trt_amd.models.depth_anything_ac import run as ac_run
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run as dav2_run
    from monocular_depth_estimation_trt_amd.models.depth_pro import run as dp_run
    from monocular_depth_estimation_trt_amd.models.depth_pro import stream as dp_stream
    ap = argparse.ArgumentParser()
    vz.add_color_arguments(ap)
    assert vz.check_color_arguments(ap.parse_args([]), True) is None
    assert vz.check_color_arguments(ap.parse_args(["--color", "x.png"]), True) is None
    metric, relative = spec.load("depth_pro"), spec.load("depth_anything_ac")
    assert vz.color_kwargs(ap.parse_args(["--color", "x.png"]), metric) == {"mode": "inverse_auto"}
    assert vz.color_kwargs(ap.parse_args(["--color", "x.png"]), relative) == {"mode": "minmax_u8"}
    assert vz.color_kwargs(ap.parse_args(["--color", "x.png", "--color-range", "0.5", "20"]), relative) == \
        {"mode": "fixed", "vmin": 0.5, "vmax": 20.0}
    for argv, device_map, msg in ((["--color", "x.png"], False, "host-postprocess"),
                                  (["--color-range", "0", "1"], True, "goes with --color"),
                                  (["--color", "x.png", "--color-range", "nan", "1"], True, "NaN")):
        with pytest.raises(SystemExit, match=msg):
            vz.check_color_arguments(ap.parse_args(argv), device_map)
    color = ["--color", str(tmp_path / "c.npy")]
    for run in (dav2_run, ac_run, dp_run):
        with pytest.raises(SystemExit, match="--color runs on the device post-process's depth map"):
            run.main(color + ["--host-postprocess"])
        with pytest.raises(SystemExit, match="goes with --color"):
            run.main(["--color-range", "0", "10"])
    with pytest.raises(SystemExit, match="both needed"):
        dp_stream.main(["--out", str(tmp_path / "o.npy")])
    with pytest.raises(SystemExit, match="both needed"):
        dp_stream.main(["--frames", str(tmp_path / "f.npy")])
    np.save(tmp_path / "f.npy", np.zeros((2, 4, 6), np.uint8))
    with pytest.raises(SystemExit, match=r"uint8 \[T,H,W,3\]"):
        dp_stream.main(["--frames", str(tmp_path / "f.npy"), "--out", str(tmp_path / "o.npy")])
    with pytest.raises(SystemExit, match="--frames"):
        dp_stream.main(["--frames", str(tmp_path / "none.npy"), "--out", str(tmp_path / "o.npy")])
    with pytest.raises(SystemExit, match="NaN"):
        dp_stream.main(["--frames", str(tmp_path / "f.npy"), "--out", str(tmp_path / "o.npy"), "--color-range", "nan",
                        "3"])
    assert not (tmp_path / "o.npy").exists() and not (tmp_path / "c.npy").exists()


def test_save_image_npy(vz, tmp_path):
    bgr = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    path = vz.save_image(str(tmp_path / "sub" / "pic.npy"), bgr)
    assert path.endswith("pic.npy") and np.array_equal(np.load(path), bgr)
    with pytest.raises(ValueError, match="uint8"):
        vz.save_image(str(tmp_path / "bad.npy"), bgr.astype(np.float32))


def test_save_image_round_trips_a_png(vz, tmp_path):
    pytest.importorskip("PIL")
    from monocular_depth_estimation_trt_amd.preprocess import load_image_bgr
    bgr, _ = vz.colorize_np(cc.depth_map("neither"), 0)
    path = vz.save_image(str(tmp_path / "pic.png"), bgr)
    assert path.endswith("pic.png") and np.array_equal(load_image_bgr(path), bgr)
