"""Robust display range on the device (csrc/depth_quantiles.hip, mde_op_depth_colorize_ranged in
csrc/depth_colorize.hip) through the C ABI, the Python classes and the drivers, against
visualize.quantiles_np and visualize.colorize_ranged_np.  Rows are compared as float64 values with NaN
equal to NaN, pictures byte for byte: selection is exact and the lerp is IEEE float64, so there is no
tolerance.

Shapes.  A workgroup owns a tile of 4096 pixels of one image, a wave 256 of them per pass: 1 x 1, 3 x 5
and 7 x 9 are under one wave; 37 x 53 = 1961 is read from a map pointer 4 bytes off its 16-byte
alignment (the scalar loads); 100 x 131 = 13100 is three tiles and a partial one of 812; the later
images of (3, 5, 7) and (2, 37, 53) start inside a float4; 640 x 640 at the reference's cap of 200000
is stride 2 over 100 tiles.  sample_cap 64 reaches strides up to 204 on these shapes.  Harness checks,
on every call, that nothing outside out[rows][8] and the first mde_op_depth_quantiles_ws_bytes of
scratch changed, hands the scratch over dirty and calls twice for identical bytes.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import quantile_cases as qc
from gpu_util import op, ptr, stream

from monocular_depth_estimation_trt_amd import _lib
from monocular_depth_estimation_trt_amd import preprocess as pre
from monocular_depth_estimation_trt_amd import visualize as vz

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64
TILE = 4096  # MDE_DEPTH_QUANTILES_TILE


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@functools.lru_cache(maxsize=None)
def lut_dev(bad=vz.BAD_VIZ):
    return torch.from_numpy(vz.lut("turbo", bad).copy()).cuda()


class Quantiles:
    """mde_op_depth_quantiles on [B][h][w] maps held on the device; `map_off` floats shift the map off
    its 16-byte alignment.  out and ws sit inside 0xA5-filled buffers; ws stays dirty between calls."""

    def __init__(self, maps, map_off=0):
        maps = np.asarray(maps, np.float32)
        self.maps = maps[None] if maps.ndim == 2 else maps
        self.B, self.h, self.w = self.maps.shape
        n = self.maps.size
        self.d_map_all = torch.zeros(n + map_off + 4, dtype=torch.float32, device="cuda")
        self.d_map_all[map_off:map_off + n] = torch.from_numpy(self.maps.reshape(-1).copy())
        self.d_map = self.d_map_all.data_ptr() + 4 * map_off
        self.need = vz.quantiles_ws_bytes(self.B, self.h, self.w)
        tiles = -(-self.h * self.w // TILE)
        assert 0 < self.need <= self.B * (8 * 256 + 64 + tiles) * 4 and self.need % 4 == 0
        self.d_out = torch.full((PAD + 64 * self.B + PAD,), FILL, dtype=torch.uint8, device="cuda")
        self.d_ws = torch.full((self.need + PAD,), FILL, dtype=torch.uint8, device="cuda")
        assert self.d_map_all.data_ptr() % 16 == 0 and self.d_out.data_ptr() % 8 == 0 and self.d_ws.data_ptr() % 8 == 0

    def range_ptr(self):
        """Where row 0's display range is: what mde_op_depth_colorize_ranged reads with stride 8."""
        return self.d_out.data_ptr() + PAD + 8 * vz.Q_VMIN

    def call(self, q, positive_only=False, reciprocal=False, pooled=False, sample_cap=0):
        rows = 1 if pooled else self.B
        self.d_out.fill_(FILL)
        runs = []
        for _ in range(2):
            op("mde_op_depth_quantiles", C.c_void_p(self.d_map), self.B, self.h, self.w, int(positive_only),
               int(reciprocal), int(pooled), int(sample_cap), (C.c_double * len(q))(*q), len(q),
               C.c_void_p(self.d_out.data_ptr() + PAD), ptr(self.d_ws), self.need, stream())
            out = self.d_out.cpu().numpy()
            assert (out[:PAD] == FILL).all() and (out[PAD + 64 * rows:] == FILL).all(), "bytes outside out written"
            assert (self.d_ws[self.need:].cpu().numpy() == FILL).all(), "scratch written past ws_bytes"
            runs.append(out[PAD:PAD + 64 * rows].tobytes())
        assert runs[0] == runs[1], "two runs, the second on the first one's scratch, differ"
        return np.frombuffer(runs[0], np.float64).reshape(rows, 8)

    def check(self, q, **kw):
        got = self.call(q, **kw)
        want = vz.quantiles_np(self.maps, q, **kw)
        assert same(got, want), (self.maps.shape, q, kw, got, want)
        return got


FLAGS = [dict(positive_only=p, reciprocal=r, pooled=pooled, sample_cap=cap)
         for p in (False, True) for r in (False, True) for pooled in (False, True) for cap in (0, 64)]


@pytest.mark.parametrize("regime", qc.REGIMES)
def test_rows_equal_quantiles_np(gpu, regime):
    for B, h, w, map_off in qc.SHAPES:
        dev = Quantiles(qc.maps(regime, B, h, w), map_off)
        for kw in FLAGS:
            for q in qc.QS:
                dev.check(q, **kw)


def test_reference_cap_at_640(gpu):
    """409600 valid pixels, 100 tiles, stride 409600 // 200000 = 2."""
    dev = Quantiles(qc.maps("lognormal", 1, 640, 640))
    row = dev.check((2.0, 98.0), positive_only=True, sample_cap=vz.SAMPLE_CAP)[0]
    assert row[0] == 409600 and row[1] == 204800
    assert tuple(row[6:]) == vz.robust_range_np(dev.maps)


@pytest.mark.parametrize("n_valid", [64, 65, 127, 128, 129, 200])
def test_stride_thresholds(gpu, n_valid):
    dev = Quantiles(qc.with_n_valid(n_valid))
    row = dev.check((2.0, 50.0, 98.0), positive_only=True, sample_cap=64)[0]
    assert row[0] == n_valid and row[1] == -(-n_valid // max(1, n_valid // 64 if n_valid > 64 else 1))


def test_extremes_in_the_first_and_the_last_partial_tile(gpu):
    """13100 pixels are tiles of 4096, 4096, 4096 and 812: min and max (ranks 0 and n - 1) sit once in
    the first tile and once in the partial one."""
    x = qc.maps("lognormal", 1, 100, 131).reshape(-1)
    for lo_at, hi_at in ((17, 4001), (3 * TILE + 5, 13099), (13099, 0)):
        y = x.copy()
        y[lo_at], y[hi_at] = 1e-6, 1e6
        row = Quantiles(y.reshape(1, 100, 131)).check((0.0, 100.0))[0]
        assert row[2] == row[4] == np.float32(1e-6) and row[3] == row[5] == np.float32(1e6)


def test_refused_arguments_launch_nothing(gpu):
    h, w = 37, 53
    d_map = torch.from_numpy(qc.maps("lognormal", 1, h, w)).cuda()
    need = vz.quantiles_ws_bytes(1, h, w)
    d_out = torch.full((64 + 8,), FILL, dtype=torch.uint8, device="cuda")
    d_ws = torch.full((need + 8,), FILL, dtype=torch.uint8, device="cuda")
    d_pic = torch.full((3 * h * w,), FILL, dtype=torch.uint8, device="cuda")
    nan = float("nan")
    good = dict(map=d_map.data_ptr(), batch=1, h=h, w=w, pos=0, rec=0, pooled=0, cap=0, q=(2.0, 98.0), nq=2,
                out=d_out.data_ptr(), ws=d_ws.data_ptr(), ws_bytes=need)
    bad = [dict(map=0), dict(out=0), dict(q=None), dict(batch=0), dict(h=0), dict(w=-1), dict(nq=0), dict(nq=4),
           dict(q=(-0.5, 98.0)), dict(q=(2.0, 100.5)), dict(q=(nan, 98.0)), dict(cap=-1), dict(batch=65536),
           dict(h=1 << 16, w=1 << 15), dict(pooled=1, batch=1 << 15, h=1 << 8, w=1 << 8, ws_bytes=1 << 40),
           dict(ws=0), dict(ws_bytes=need - 1), dict(ws=d_ws.data_ptr() + 4), dict(out=d_out.data_ptr() + 4)]
    for change in bad:
        a = dict(good, **change)
        q = None if a["q"] is None else (C.c_double * 3)(*a["q"], 0.0)
        with pytest.raises(_lib.MDEError) as e:
            op("mde_op_depth_quantiles", C.c_void_p(a["map"]), a["batch"], a["h"], a["w"], a["pos"], a["rec"],
               a["pooled"], a["cap"], q, a["nq"], C.c_void_p(a["out"]), C.c_void_p(a["ws"]), a["ws_bytes"], stream())
        assert e.value.code == 1, (change, e.value)
    lut = lut_dev()
    good = dict(map=d_map.data_ptr(), batch=1, h=h, w=w, rng=d_out.data_ptr(), stride=8, lut=lut.data_ptr(),
                out=d_pic.data_ptr())
    for change in (dict(map=0), dict(rng=0), dict(lut=0), dict(out=0), dict(batch=0), dict(h=0), dict(w=-1),
                   dict(stride=-1), dict(rng=d_out.data_ptr() + 4), dict(batch=65536), dict(h=1 << 16, w=1 << 15)):
        a = dict(good, **change)
        with pytest.raises(_lib.MDEError) as e:
            op("mde_op_depth_colorize_ranged", C.c_void_p(a["map"]), a["batch"], a["h"], a["w"], 0, 0,
               C.c_void_p(a["rng"]), a["stride"], C.c_void_p(a["lut"]), 1, C.c_void_p(a["out"]), stream())
        assert e.value.code == 1, (change, e.value)
    torch.cuda.synchronize()
    for t in (d_out, d_ws, d_pic):
        assert (t.cpu().numpy() == FILL).all()
    assert vz.quantiles_ws_bytes(65536, 8, 8) == 0 and vz.quantiles_ws_bytes(1, 1 << 16, 1 << 15) == 0
    assert vz.quantiles_ws_bytes(1, 0, 8) == 0


# ---- the ranged colour op -------------------------------------------------------------------------

def device_ranged(maps, d_range, range_stride, positive_only=False, reciprocal=False, swap_rb=True, map_off=0,
                  out_off=0):
    """mde_op_depth_colorize_ranged on [B][h][w] maps with the axis at device pointer `d_range`; checks
    that nothing outside the picture changed; returns it [B, h, w, 3]."""
    maps = np.asarray(maps, np.float32)
    maps = maps[None] if maps.ndim == 2 else maps
    B, h, w = maps.shape
    n = maps.size
    d_map_all = torch.zeros(n + map_off, dtype=torch.float32, device="cuda")
    d_map_all[map_off:] = torch.from_numpy(maps.reshape(-1).copy())
    d_out = torch.full((PAD + out_off + 3 * n + PAD,), FILL, dtype=torch.uint8, device="cuda")
    first = PAD + out_off
    op("mde_op_depth_colorize_ranged", C.c_void_p(d_map_all.data_ptr() + 4 * map_off), B, h, w, int(positive_only),
       int(reciprocal), C.c_void_p(d_range), int(range_stride), ptr(lut_dev()), int(swap_rb),
       C.c_void_p(d_out.data_ptr() + first), stream())
    del d_map_all
    out = d_out.cpu().numpy()
    assert (out[:first] == FILL).all() and (out[first + 3 * n:] == FILL).all(), "bytes outside out_u8 written"
    return out[first:first + 3 * n].reshape(B, h, w, 3).copy()


def device_fixed(maps, vmin, vmax, swap_rb=True):
    """mde_op_depth_colorize mode 2."""
    maps = np.asarray(maps, np.float32)
    B, h, w = maps.shape
    d_map = torch.from_numpy(maps.copy()).cuda()
    d_out = torch.empty(maps.size * 3, dtype=torch.uint8, device="cuda")
    op("mde_op_depth_colorize", ptr(d_map), B, h, w, 2, 0, 0.0, float(vmin), float(vmax), ptr(lut_dev()), int(swap_rb),
       ptr(d_out), C.c_void_p(0), C.c_void_p(0), 0, stream())
    return d_out.cpu().numpy().reshape(B, h, w, 3)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5), (2, 37, 53), (3, 5, 7), (1, 100, 131)])
def test_ranged_equals_colorize_ranged_np(gpu, shape):
    x = qc.maps("sprinkled", *shape)
    B = shape[0]
    ranges = np.array([[0.5, 20.0], [1.0, 3.0], [2.5, 2.5]])[:B]
    d_rng = torch.from_numpy(np.concatenate([ranges, np.full((B, 6), np.nan)], axis=1)).cuda()  # rows of 8
    for positive_only in (False, True):
        for reciprocal in (False, True):
            for swap_rb in (True, False):
                kw = dict(positive_only=positive_only, reciprocal=reciprocal, swap_rb=swap_rb)
                got = device_ranged(x, d_rng.data_ptr(), 8, **kw)
                assert got.tobytes() == vz.colorize_ranged_np(x, ranges, **kw).tobytes(), (shape, kw)
                got = device_ranged(x, d_rng.data_ptr(), 0, **kw)  # one shared axis
                assert got.tobytes() == vz.colorize_ranged_np(x, ranges[0], **kw).tobytes(), (shape, kw)
    for vmin, vmax in ((0.5, 20.0), (5.0, 1.0), (2.5, 2.5), (-np.inf, np.inf), (np.nan, 1.0)):
        d_one = torch.tensor([vmin, vmax], dtype=torch.float64, device="cuda")
        got = device_ranged(x, d_one.data_ptr(), 0)
        assert got.tobytes() == vz.colorize_ranged_np(x, (vmin, vmax)).tobytes()
        if vmin == vmin:  # mode 2 refuses a NaN bound on the host; on the device it makes every pixel bad
            assert got.tobytes() == device_fixed(x, vmin, vmax).tobytes(), (vmin, vmax)
        else:
            assert (got == np.array(vz.BAD_VIZ[::-1], np.uint8)).all()


def test_ranged_misaligned_buffers(gpu):
    x = qc.maps("sprinkled", 2, 37, 53)
    ranges = np.array([[0.5, 20.0], [0.1, 3.0]])
    d_rng = torch.from_numpy(ranges.copy()).cuda()
    for out_off in (0, 1, 6, 13):
        for map_off in (0, 2, 3):
            got = device_ranged(x, d_rng.data_ptr(), 2, True, True, out_off=out_off, map_off=map_off)
            assert got.tobytes() == vz.colorize_ranged_np(x, ranges, True, True).tobytes(), (out_off, map_off)


@pytest.mark.parametrize("pooled", [False, True])
def test_chained_from_the_quantile_rows(gpu, pooled):
    """The quantile op's rows feed the colour op from device memory: out + 6, stride 8 (0 when pooled)."""
    x = np.concatenate([qc.maps("sprinkled", 1, 37, 53), qc.maps("lognormal", 1, 37, 53) * np.float32(3)])
    for reciprocal in (False, True):
        dev = Quantiles(x)
        rows = dev.check((2.0, 98.0), positive_only=True, reciprocal=reciprocal, pooled=pooled, sample_cap=vz.SAMPLE_CAP)
        got = device_ranged(x, dev.range_ptr(), 0 if pooled else 8, True, reciprocal)
        want = vz.colorize_ranged_np(x, rows[:, 6:], True, reciprocal)
        assert got.tobytes() == want.tobytes()
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 8
        if not pooled:
            assert tuple(rows[0, 6:]) != tuple(rows[1, 6:])


def robust_np(maps, q=(2.0, 98.0), reciprocal=False, pooled=False):
    """The numpy chain of DeviceColorize's mode 'robust': (picture, ranges [B, 2])."""
    rows = vz.quantiles_np(maps, q, True, reciprocal, pooled, vz.SAMPLE_CAP)
    return vz.colorize_ranged_np(maps, rows[:, 6:], True, reciprocal), np.broadcast_to(rows[:, 6:], (len(maps), 2))


def test_device_colorize_robust(gpu):
    maps = np.concatenate([qc.maps("sprinkled", 1, 37, 53), qc.maps("lognormal", 1, 37, 53)])
    d_map = torch.from_numpy(maps.copy()).cuda()
    torch.cuda.synchronize()
    with vz.DeviceColorize(2, 37, 53) as dc:
        for kw in ({}, dict(reciprocal=True), dict(pooled=True), dict(q_percent=(10.0, 60.0))):
            pic = dc.run(d_map.data_ptr(), 0, "robust", **kw)
            want, rng = robust_np(maps, kw.get("q_percent", (2.0, 98.0)), kw.get("reciprocal", False),
                                  kw.get("pooled", False))
            assert pic.tobytes() == want.tobytes(), kw
            assert dc.range().dtype == np.float64 and same(dc.range(), rng), kw
        # the other modes are what they were, on the same object
        pic = dc.run(d_map.data_ptr(), 0, "fixed", vmin=0.5, vmax=20.0)
        want, want_rng = vz.colorize_np(maps, "fixed", vmin=0.5, vmax=20.0)
        assert pic.tobytes() == want.tobytes() and np.array_equal(dc.range(), want_rng)
    with vz.DeviceQuantiles(2, 37, 53) as dq:
        assert same(dq.run(d_map.data_ptr(), 0, vz.DISTRIBUTION_Q), vz.quantiles_np(maps, vz.DISTRIBUTION_Q))
        assert same(dq.run(d_map.data_ptr(), 0, (50.0,), pooled=True), vz.quantiles_np(maps, (50.0,), pooled=True))
    with pytest.raises(RuntimeError):
        dq.result()  # freed
    assert vz.device_distribution(d_map.data_ptr(), 37, 53, 0) == vz.distribution_np(maps[0])


def test_robust_in_a_captured_graph(gpu):
    """One robust enqueue (the eleven quantile kernels, the colour pass) captured into a
    torch.cuda.graph on a side stream, replayed on a changed map."""
    h, w = 37, 53
    pa, pb = qc.maps("lognormal", 1, h, w)[0], qc.maps("sprinkled", 1, h, w)[0]
    d_map = torch.from_numpy(pa.copy()).cuda()
    with vz.DeviceColorize(1, h, w, robust=True) as dc:
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dc.enqueue(d_map.data_ptr(), s.cuda_stream, "robust")  # warm: the kernels are loaded
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            dc.enqueue(d_map.data_ptr(), s.cuda_stream, "robust")
        for p in (pa, pb):
            d_map.copy_(torch.from_numpy(p.copy()))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            dc.download(0)
            want, rng = robust_np(p[None])
            assert dc.result().tobytes() == want.tobytes() and same(dc.range(), rng)


# ---- the drivers' --color-robust ------------------------------------------------------------------

def photo(h, w, seed=7):
    return np.random.Generator(np.random.PCG64(h * 131 + w + seed)).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def depth_lines(out):
    return [l for l in out.splitlines() if l.startswith("[MDET] depth : ")]


def check_depth_line(line, depth):
    d = vz.distribution_np(depth)
    assert line == vz.format_distribution(d), (line, d)
    words = line.split()
    assert [float(words[i]) for i in (4, 6, 8)] == [d["p02"], d["median"], d["p98"]]
    assert float(words[10][:-1]) == d["valid_pct"]


def check_driver_robust(run_main, args, tmp_path, capsys, reciprocal_when_near, first_of=lambda r: r):
    """--color-robust draws the returned map on its own 2..98 range; --color-robust-near draws proximity;
    without the options nothing of this is printed."""
    capsys.readouterr()
    path = str(tmp_path / "robust.npy")
    depth = first_of(run_main(args + ["--color", path, "--color-robust"]))
    out = capsys.readouterr().out
    want, rng = robust_np(depth[None])
    assert np.load(path).tobytes() == want[0].tobytes()
    line = [l for l in out.splitlines() if l.startswith("[MDET] color : ")]
    assert len(line) == 1 and f"mode robust range {rng[0, 0]:0.6g}..{rng[0, 1]:0.6g} " in line[0], out
    assert len(depth_lines(out)) == 1
    check_depth_line(depth_lines(out)[0], depth)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 8
    path2 = str(tmp_path / "near.npy")
    run_main(args + ["--color", path2, "--color-robust", "5", "90", "--color-robust-near"])
    want2, _ = robust_np(depth[None], (5.0, 90.0), reciprocal_when_near)
    assert np.load(path2).tobytes() == want2[0].tobytes() and want2.tobytes() != want.tobytes()
    capsys.readouterr()
    for more, msg in ((["--color-robust"], "goes with --color"),
                      (["--color", path, "--color-robust", "--color-range", "1", "2"], "exclude"),
                      (["--color", path, "--color-robust", "2"], "LO HI")):
        with pytest.raises(SystemExit, match=msg):
            run_main(args + more)
    return depth


def test_dav2_driver_robust(gpu, tmp_path, capsys):
    """depth_anything_v2 (spec: metric, a depth output: near is 1 / depth) on a 37 x 53 photo."""
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    np.save(tmp_path / "src.npy", photo(37, 53))
    args = ["--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--image",
            str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench"), "--source", "synthetic:vits:metric:1234"]
    check_driver_robust(run.main, args, tmp_path, capsys, True)
    run.main(args + ["--color", str(tmp_path / "plain.npy")])
    assert not depth_lines(capsys.readouterr().out)  # as it was without the new options


def test_depth_anything_ac_driver_robust(gpu, tmp_path, capsys):
    """depth_anything_ac's spec says relative: reciprocal stays off."""
    from monocular_depth_estimation_trt_amd.models.depth_anything_ac import run
    np.save(tmp_path / "src.npy", photo(37, 53))
    args = ["--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--image",
            str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench")]
    check_driver_robust(run.main, args, tmp_path, capsys, False)


def dp_args(tmp_path, image):
    return ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations",
            "2", "--warmup", "1", "--image", str(image), "--out-dir", str(tmp_path / "bench")]


def test_depth_pro_driver_and_stream_robust(gpu, tmp_path, capsys):
    from monocular_depth_estimation_trt_amd.models.depth_pro import run, stream as dp_stream
    frames = np.stack([photo(37, 53), photo(37, 53, seed=8)])
    np.save(tmp_path / "f0.npy", frames[0])
    np.save(tmp_path / "f1.npy", frames[1])
    np.save(tmp_path / "frames.npy", frames)
    d0 = check_driver_robust(run.main, dp_args(tmp_path, tmp_path / "f0.npy"), tmp_path, capsys, True,
                             first_of=lambda r: r[0])
    d1 = run.main(dp_args(tmp_path, tmp_path / "f1.npy"))[0]
    capsys.readouterr()
    engine = ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(tmp_path / "e_fp16.mdeng")]
    got = dp_stream.main(engine + ["--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "out.npy"),
                                   "--color-robust"])
    lines = depth_lines(capsys.readouterr().out)
    for t, d in enumerate((d0, d1)):  # each frame on its own range
        assert got[t].tobytes() == robust_np(d[None])[0][0].tobytes(), t
    assert len(lines) == 1
    check_depth_line(lines[0], d1)  # the last frame's
    with pytest.raises(SystemExit, match="exclude"):
        dp_stream.main(engine + ["--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "o.npy"),
                                 "--color-robust", "--color-range", "1", "2"])


def test_vggt_driver_robust_shares_one_axis(gpu, tmp_path, capsys):
    """S = 2: both views are drawn on the range pooled over the two cropped maps."""
    from monocular_depth_estimation_trt_amd.models.vggt import run
    np.save(tmp_path / "a.npy", photo(37, 53))
    np.save(tmp_path / "b.npy", photo(37, 53, seed=8))
    args = ["--source", "synthetic:vggt:tiny", "--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2",
            "--warmup", "1", "--image", str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), "--out-dir",
            str(tmp_path / "bench")]
    capsys.readouterr()
    depth = run.main(args + ["--color", str(tmp_path / "out.npy"), "--color-robust"])
    out = capsys.readouterr().out
    assert depth.ndim == 3 and depth.shape[0] == 2
    small, rng = robust_np(depth, pooled=True)
    assert tuple(rng[0]) == tuple(rng[1]) == vz.robust_range_np(depth)
    own = [vz.robust_range_np(d) for d in depth]
    assert own[0] != own[1]  # on their own ranges the two views would differ
    lines = [l for l in out.splitlines() if l.startswith("[MDET] color : ")]
    assert len(lines) == 2 and len(depth_lines(out)) == 2
    for i, name in enumerate(("out.npy", "out_1.npy")):
        pic = np.load(tmp_path / name)
        assert pic.shape == (37, 53, 3) and np.array_equal(pic, pre.resize_linear_u8(small[i], 37, 53))
        assert f"mode robust range {rng[0, 0]:0.6g}..{rng[0, 1]:0.6g} " in lines[i]
        check_depth_line(depth_lines(out)[i], depth[i])
