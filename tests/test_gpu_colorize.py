"""Colour frames on the device (csrc/depth_colorize.hip) through the C ABI, the Python class and the
drivers, against visualize.colorize_np and against what matplotlib drew
(tests/golden/colorize_cases.npz).  Every comparison of pictures is exact byte equality; ranges are
compared as float32 values (NaN equal to NaN).

Shapes.  The colour pass groups 16 consecutive pixels of the flat batch, the range pass owns tiles of
4096 pixels of one image: 1 x 1 and 3 x 5 are less than one group (scalar path only); 37 x 53 = 1961
is 122 groups and a tail of 9; batches (2, 37, 53) and (3, 5, 7) start their later images inside a
group (1961 and 35 are odd), so one group carries two images' ranges; 32 x 48 is a multiple of 16 (no
tail); 100 x 131 = 13100 is three tiles and a partial one of 812.  device_colorize() checks on every
call that nothing outside out_u8, range_out and the first mde_op_depth_colorize_ws_bytes of scratch
changed.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import colorize_cases as cc
from gpu_util import op, ptr, stream

from monocular_depth_estimation_trt_amd import _lib
from monocular_depth_estimation_trt_amd import visualize as vz

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64
MANY = (100, 131)


@functools.lru_cache(maxsize=None)
def lut_dev(bad):
    return torch.from_numpy(vz.lut("turbo", bad).copy()).cuda()


def device_colorize(maps, mode, map_is_inverse=False, denom_eps=0.0, vmin=None, vmax=None, swap_rb=True,
                    with_range=True, map_off=0, out_off=0):
    """mde_op_depth_colorize on [B][h][w] maps; `map_off` floats and `out_off` bytes shift the two
    buffers off their 16-byte alignment.  Checks the guards; returns (picture [B, h, w, 3], range
    [B, 2] or None)."""
    maps = np.asarray(maps, np.float32)
    if maps.ndim == 2:
        maps = maps[None]
    B, h, w = maps.shape
    n = B * h * w
    mode = vz.mode_index(mode)
    d_map_all = torch.zeros(n + map_off, dtype=torch.float32, device="cuda")
    d_map_all[map_off:] = torch.from_numpy(maps.reshape(-1).copy())
    need = vz.ws_bytes(B, h, w)
    assert need == (B * -(-h * w // vz.TILE) * 2 + B * 2) * 4
    d_out = torch.full((PAD + out_off + 3 * n + PAD,), FILL, dtype=torch.uint8, device="cuda")
    d_rng = torch.full((PAD + 8 * B + PAD,), FILL, dtype=torch.uint8, device="cuda")
    d_ws = torch.full((need + PAD,), FILL, dtype=torch.uint8, device="cuda")
    assert d_map_all.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0 and d_ws.data_ptr() % 4 == 0
    first = PAD + out_off
    op("mde_op_depth_colorize", C.c_void_p(d_map_all.data_ptr() + 4 * map_off), B, h, w, mode, int(map_is_inverse),
       float(denom_eps), float(vmin or 0.0), float(vmax or 0.0), ptr(lut_dev(vz.BAD_VIZ if mode == 2 else vz.BAD)),
       int(swap_rb), C.c_void_p(d_out.data_ptr() + first), C.c_void_p(d_rng.data_ptr() + PAD if with_range else 0),
       ptr(d_ws), need, stream())
    del d_map_all
    out, rng, wsb = d_out.cpu().numpy(), d_rng.cpu().numpy(), d_ws.cpu().numpy()
    assert (out[:first] == FILL).all() and (out[first + 3 * n:] == FILL).all(), "bytes outside out_u8 written"
    assert (wsb[need:] == FILL).all(), "scratch written past mde_op_depth_colorize_ws_bytes"
    if mode == 2:
        assert (wsb == FILL).all(), "mode 2 reads and writes no scratch"
    assert (rng[:PAD] == FILL).all() and (rng[PAD + 8 * B:] == FILL).all(), "bytes outside range_out written"
    if not with_range:
        assert (rng == FILL).all()
    return (out[first:first + 3 * n].reshape(B, h, w, 3).copy(),
            rng[PAD:PAD + 8 * B].view(np.float32).reshape(B, 2).copy() if with_range else None)


def same_range(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


def check(maps, mode, what="", **kw):
    """The op against colorize_np; returns the picture."""
    maps = np.asarray(maps, np.float32)
    maps = maps[None] if maps.ndim == 2 else maps
    np_kw = {k: v for k, v in kw.items() if k not in ("with_range", "map_off", "out_off")}
    want, want_rng = vz.colorize_np(maps, mode, **np_kw)
    got, rng = device_colorize(maps, mode, **kw)
    diff = int((got != want).any(axis=-1).sum())
    assert got.tobytes() == want.tobytes(), (what, mode, kw, f"{diff} of {want.size // 3} pixels differ")
    if rng is not None:
        assert same_range(rng, want_rng), (what, mode, kw, rng, want_rng)
    return got


def mode_kwargs(mode):
    return dict(vmin=cc.FIXED_RANGE[0], vmax=cc.FIXED_RANGE[1]) if mode == 2 else {}


def batch_of(B, h, w):
    """B maps [h, w], each from another clipping regime."""
    names = list(cc.REGIMES)
    return np.stack([cc.depth_map(names[(i + 1) % 4], h, w) for i in range(B)])


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5), (1, 37, 53), (2, 37, 53), (3, 5, 7), (1, 32, 48)])
def test_op_equals_colorize_np(gpu, shape):
    maps = batch_of(*shape)
    for mode in (0, 1, 2):
        for swap_rb in (True, False):
            for with_range in (True, False):
                check(maps, mode, what=shape, swap_rb=swap_rb, with_range=with_range, **mode_kwargs(mode))


@pytest.mark.parametrize("regime", list(cc.REGIMES))
def test_recorded_cases(gpu, regime):
    """The device against what matplotlib drew through the reference's lines, and against colorize_np."""
    fx = cc.load_fixture()
    for variant in cc.VARIANTS:
        x, kw = cc.case_input(regime, variant), cc.case_kwargs(variant)
        mode = kw.pop("mode")
        got = check(x, mode, what=(regime, variant), **kw)
        assert got[0].tobytes() == fx[f"{regime}/{variant}/bgr"].tobytes(), (regime, variant)


@pytest.mark.parametrize("regime", list(cc.REGIMES))
def test_non_finite_zero_and_negative_pixels(gpu, regime):
    x = cc.sprinkled(regime)
    two = np.stack([x, cc.sprinkled(regime, seed=6)[::-1].copy()])
    with np.errstate(all="ignore"):
        for mode in (0, 1, 2):
            check(x, mode, what=regime, **mode_kwargs(mode))
            check(two, mode, what=regime, swap_rb=False, **mode_kwargs(mode))
        check(x, 0, what=regime, denom_eps=1e-6)
        check(np.float32(1.0) / x, 0, what=regime, map_is_inverse=True)


def test_constant_all_nan_and_degenerate_axis(gpu):
    const = np.full((37, 53), 2.5, np.float32)
    nans = np.full((37, 53), np.nan, np.float32)
    zeros = np.zeros((37, 53), np.float32)
    for mode in (0, 1):
        assert (check(const, mode) == 0).all()  # 0 / 0: bad, black
        assert (check(nans, mode) == 0).all()
        assert (check(np.stack([const, cc.depth_map("low"), nans]), mode)[1] != 0).any()
    _, rng = device_colorize(nans, 0)
    assert np.isnan(rng).all()
    _, rng = device_colorize(zeros, 0)  # 1 / 0 = +inf everywhere: no finite value
    assert np.isnan(rng).all()
    check(zeros, 0)
    check(const, 0, denom_eps=1e-6)  # 0 / 1e-6: the bottom colour
    check(const, 0, map_is_inverse=True)
    pic = check(nans, 2, vmin=0.0, vmax=1.0, swap_rb=False)
    assert (pic == np.array(vz.BAD_VIZ, np.uint8)).all()
    for vmin, vmax in ((2.5, 2.5), (5.0, 1.0), (2.5, -np.inf)):  # vmax <= vmin: the axis is [vmin, vmin + 1e-6]
        _, rng = device_colorize(cc.depth_map("neither"), 2, vmin=vmin, vmax=vmax)
        assert rng[0, 0] == np.float32(vmin) and rng[0, 1] == np.float32(vmin + 1e-6)
        check(cc.depth_map("neither"), 2, vmin=vmin, vmax=vmax)
    check(cc.depth_map("neither"), 2, vmin=-np.inf, vmax=np.inf)  # inf / inf: NaN t, bad


@pytest.mark.parametrize("where", ["first_tile", "last_partial_tile"])
def test_extremes_in_the_first_and_the_last_partial_tile(gpu, where):
    """13100 pixels are tiles of 4096, 4096, 4096 and 812: the extreme values sit once in the first
    tile and once in the partial one, and the range must find them there."""
    h, w = MANY
    assert h * w // vz.TILE == 3 and 0 < h * w % vz.TILE < vz.TILE
    x = np.array(cc.depth_map("neither", h, w)).reshape(-1)
    at = (17, 4001) if where == "first_tile" else (3 * vz.TILE + 5, h * w - 1)
    x[at[0]], x[at[1]] = 0.25, 40.0  # inside [1/250, 10] as inverse depth: the range is theirs alone
    x = x.reshape(h, w)
    for mode in (0, 1):
        _, rng = device_colorize(x, mode)
        assert tuple(rng[0]) == ((np.float32(1 / 40.0), 4.0) if mode == 0 else (0.25, 40.0))
        check(x, mode, what=where)
    check(np.stack([x, x[::-1].copy()]), 0, what=where)
    check(x, 2, vmin=0.5, vmax=20.0)


def test_misaligned_buffers(gpu):
    """out_u8 at every kind of offset: the first group starts at the one pixel where the output is
    16-byte aligned; when the map is not aligned there too, every pixel takes the scalar path."""
    maps = batch_of(2, 37, 53)
    paths = set()
    for out_off in (0, 1, 6, 13):
        for map_off in (0, 2, 3):
            head = ((16 - out_off % 16) * 11) % 16
            paths.add((4 * (map_off + head)) % 16 == 0)
            for mode in (0, 2):
                check(maps, mode, what=(out_off, map_off), out_off=out_off, map_off=map_off, **mode_kwargs(mode))
    assert paths == {True, False}


def test_two_runs_give_the_same_bytes(gpu):
    h, w = MANY
    maps = np.stack([cc.sprinkled("both", h, w), cc.sprinkled("high", h, w)])
    with np.errstate(all="ignore"):
        for mode in (0, 1, 2):
            a = device_colorize(maps, mode, **mode_kwargs(mode))
            b = device_colorize(maps, mode, **mode_kwargs(mode))
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refused_arguments_launch_nothing(gpu):
    h, w = 37, 53
    d_map = torch.from_numpy(np.array(cc.depth_map("neither"))).cuda()
    d_out = torch.full((3 * h * w,), FILL, dtype=torch.uint8, device="cuda")
    d_rng = torch.full((8,), FILL, dtype=torch.uint8, device="cuda")
    need = vz.ws_bytes(1, h, w)
    d_ws = torch.full((need,), FILL, dtype=torch.uint8, device="cuda")
    lut = lut_dev(vz.BAD)
    nan = float("nan")
    good = dict(map=d_map.data_ptr(), batch=1, h=h, w=w, mode=0, inv=0, eps=0.0, vmin=0.0, vmax=1.0, lut=lut.data_ptr(),
                swap=1, out=d_out.data_ptr(), rng=d_rng.data_ptr(), ws=d_ws.data_ptr(), ws_bytes=need)
    bad = [dict(map=0), dict(out=0), dict(lut=0), dict(batch=0), dict(h=0), dict(w=-1), dict(mode=3), dict(mode=-1),
           dict(eps=nan), dict(mode=2, vmin=nan), dict(mode=2, vmax=nan), dict(batch=65536), dict(ws=0),
           dict(ws_bytes=need - 1), dict(mode=1, ws=0), dict(mode=1, ws_bytes=need - 1), dict(h=1 << 16, w=1 << 15)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(_lib.MDEError) as e:
            op("mde_op_depth_colorize", C.c_void_p(a["map"]), a["batch"], a["h"], a["w"], a["mode"], a["inv"], a["eps"],
               a["vmin"], a["vmax"], C.c_void_p(a["lut"]), a["swap"], C.c_void_p(a["out"]), C.c_void_p(a["rng"]),
               C.c_void_p(a["ws"]), a["ws_bytes"], stream())
        assert e.value.code == 1, (change, e.value)
    torch.cuda.synchronize()
    for t in (d_out, d_rng, d_ws):
        assert (t.cpu().numpy() == FILL).all()
    assert vz.ws_bytes(65536, 8, 8) == 0 and vz.ws_bytes(1, 1 << 16, 1 << 15) == 0 and vz.ws_bytes(1, 0, 8) == 0


def test_device_colorize_class(gpu):
    """DeviceColorize end to end: enqueue, download, result, range; batch 2; every mode; freed after."""
    maps = batch_of(2, 37, 53)
    d_map = torch.from_numpy(maps.copy()).cuda()
    torch.cuda.synchronize()
    with vz.DeviceColorize(2, 37, 53) as dc:
        for mode, kw in (("inverse_auto", {}), ("inverse_auto", dict(denom_eps=1e-6)), ("minmax_u8", {}),
                         ("fixed", dict(vmin=0.5, vmax=20.0)), ("minmax_u8", dict(swap_rb=False))):
            pic = dc.run(d_map.data_ptr(), 0, mode, **kw)
            want, want_rng = vz.colorize_np(maps, mode, **kw)
            assert pic.shape == (2, 37, 53, 3) and pic.tobytes() == want.tobytes(), (mode, kw)
            assert same_range(dc.range(), want_rng), (mode, kw)
        with pytest.raises(ValueError, match="vmin and vmax"):
            dc.enqueue(d_map.data_ptr(), 0, "fixed")
        with pytest.raises(ValueError, match="unknown colour mode"):
            dc.enqueue(d_map.data_ptr(), 0, "rainbow")
    with pytest.raises(RuntimeError):
        dc.result()  # freed


def test_device_colorize_in_a_captured_graph(gpu):
    """One DeviceColorize.enqueue (three kernels and the scalar tail) captured into a torch.cuda.graph on
    a side stream, replayed on a changed map."""
    h, w = 37, 53
    pa, pb = cc.depth_map("high"), cc.depth_map("low")
    d_map = torch.from_numpy(np.array(pa)).cuda()
    with vz.DeviceColorize(1, h, w) as dc:
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dc.enqueue(d_map.data_ptr(), s.cuda_stream, "inverse_auto")  # warm: the kernels are loaded
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            dc.enqueue(d_map.data_ptr(), s.cuda_stream, "inverse_auto")
        pics = []
        for p in (pa, pb):
            d_map.copy_(torch.from_numpy(np.array(p)))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            dc.download(0)
            want, want_rng = vz.colorize_np(p, 0)
            assert dc.result()[0].tobytes() == want.tobytes() and same_range(dc.range()[0], want_rng)
            pics.append(dc.result()[0].copy())
        assert pics[0].tobytes() != pics[1].tobytes()


# ---- the drivers' --color ------------------------------------------------------------------------

def photo(h, w, seed=7):
    return np.random.Generator(np.random.PCG64(h * 131 + w + seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def color_line(out, mode, path):
    line = [l for l in out.splitlines() if l.startswith("[MDET] color : ")]
    assert len(line) == 1 and f"mode {mode} range " in line[0] and line[0].endswith(f"-> {path}"), out
    assert "(device, kernels + D2H of " in line[0] and " bytes, hipEvents: " in line[0], line[0]
    return line[0]


def check_driver_color(run_main, args, tmp_path, capsys, mode, first_of=lambda r: r):
    """`--color` writes the picture of the map the driver returns; then `--color-range` on that map's
    own extremes.  Returns the depth."""
    path = str(tmp_path / "color.npy")
    capsys.readouterr()
    depth = first_of(run_main(args + ["--color", path]))
    line = color_line(capsys.readouterr().out, mode, path)
    want, (lo, hi) = vz.colorize_np(depth, mode)
    got = np.load(path)
    assert got.dtype == np.uint8 and got.shape == depth.shape + (3,) and got.tobytes() == want.tobytes()
    assert f"range {lo:0.6g}..{hi:0.6g} " in line and f"D2H of {want.nbytes} bytes" in line
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 8  # a picture, not one colour
    vmin, vmax = float(depth.min()), float(depth.max())
    path2 = str(tmp_path / "fixed.npy")
    again = first_of(run_main(args + ["--color", path2, "--color-range", repr(vmin), repr(vmax)]))
    assert np.array_equal(again, depth)
    color_line(capsys.readouterr().out, "fixed", path2)
    want2, _ = vz.colorize_np(depth, "fixed", vmin=vmin, vmax=vmax)
    assert np.load(path2).tobytes() == want2.tobytes() and want2.tobytes() != want.tobytes()
    return depth


def test_dav2_driver_color(gpu, tmp_path, capsys):
    """depth_anything_v2 (spec: metric -> inverse_auto) on a 120 x 160 photo."""
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    np.save(tmp_path / "src.npy", photo(120, 160))
    args = ["--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--image",
            str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench"), "--source", "synthetic:vits:metric:1234"]
    check_driver_color(run.main, args, tmp_path, capsys, "inverse_auto")
    with pytest.raises(SystemExit, match="host-postprocess"):
        run.main(args + ["--color", str(tmp_path / "c.npy"), "--host-postprocess"])


def test_depth_anything_ac_driver_color(gpu, tmp_path, capsys):
    """depth_anything_ac inherits the DA-V2 driver; its spec says relative: minmax_u8."""
    from monocular_depth_estimation_trt_amd.models.depth_anything_ac import run
    np.save(tmp_path / "src.npy", photo(120, 160))
    args = ["--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--image",
            str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench")]
    check_driver_color(run.main, args, tmp_path, capsys, "minmax_u8")


def dp_args(tmp_path, image):
    return ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations",
            "2", "--warmup", "1", "--image", str(image), "--out-dir", str(tmp_path / "bench")]


def test_depth_pro_driver_color(gpu, tmp_path, capsys):
    """depth_pro (spec: metric -> inverse_auto) on a 120 x 160 photo."""
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    np.save(tmp_path / "src.npy", photo(120, 160))
    check_driver_color(run.main, dp_args(tmp_path, tmp_path / "src.npy"), tmp_path, capsys, "inverse_auto",
                       first_of=lambda r: r[0])


def test_depth_pro_stream(gpu, tmp_path, capsys):
    """stream.py on two different frames gives, for each, the bytes run.py --color gives for that
    frame alone; the float map is never downloaded."""
    from monocular_depth_estimation_trt_amd.models.depth_pro import run, stream as dp_stream
    frames = np.stack([photo(120, 160), photo(120, 160, seed=8)])
    np.save(tmp_path / "frames.npy", frames)
    engine = ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(tmp_path / "e_fp16.mdeng")]
    got = dp_stream.main(engine + ["--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "out.npy")])
    out = capsys.readouterr().out
    for words in ("[MDET] 2 iterations time (", "[MDET] Average FPS: ", "[MDET] Average inference time: "):
        assert sum(l.startswith(words) for l in out.splitlines()) == 1, out
    assert got.shape == (2, 120, 160, 3) and np.array_equal(np.load(tmp_path / "out.npy"), got)
    for t in range(2):
        np.save(tmp_path / f"f{t}.npy", frames[t])
        run.main(dp_args(tmp_path, tmp_path / f"f{t}.npy") + ["--color", str(tmp_path / f"c{t}.npy")])
        assert np.load(tmp_path / f"c{t}.npy").tobytes() == got[t].tobytes(), t
    assert got[0].tobytes() != got[1].tobytes()
    fixed = dp_stream.main(engine + ["--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "fixed.npy"),
                                     "--color-range", "0.5", "20"])
    run.main(dp_args(tmp_path, tmp_path / "f1.npy") + ["--color", str(tmp_path / "cf.npy"), "--color-range", "0.5", "20"])
    assert np.load(tmp_path / "cf.npy").tobytes() == fixed[1].tobytes()
