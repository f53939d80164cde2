"""Point clouds without a GPU: the numpy restatement of the mde_op_point_cloud contract
(pointcloud.unproject_np) against the reference's formula, the compaction semantics, the PLY
writer / reader and the ABI wrapper's argument checks.

The bar of the restatement: the reference (models/depth_pro/onnx2trt_pointcloud.py:172-184)
computes x = (u - w/2) / f_px * z in float64.  From the same float32 z, f, cx, cy the contract
rounds three times (subtract, divide, multiply), each within 2^-24 relative, so X and Y are
within 3 * 2^-24 to first order; the bar is 4 * 2^-24 = 2^-22, which leaves room for the
second-order terms (worst case measured over the cases below: 2.01 * 2^-24).  Where u == cx the
result is exactly 0.
"""

import ctypes
import functools
import os

import numpy as np
import pytest

from monocular_depth_estimation_trt_amd import pointcloud as pc

BAR = 2.0 ** -22
SHAPES = [(37, 53), (9, 5), (2268, 3024)]
FOCALS = [3.7, 511.9, 2875.123]


@functools.lru_cache(maxsize=None)
def depth_map(h, w):
    """z uniform in [1e-4, 1e4]; cached, never written."""
    rng = np.random.Generator(np.random.PCG64(h * 10007 + w))
    z = rng.uniform(1e-4, 1e4, size=(h, w)).astype(np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def photo(h, w):
    rng = np.random.Generator(np.random.PCG64(h * 131 + w))
    a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def reference_xy(z, f, cx, cy):
    """The reference's meshgrid arithmetic in float64 from float32 z, f, cx, cy."""
    h, w = z.shape
    f, cx, cy = (np.float64(np.float32(t)) for t in (f, cx, cy))
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    z = z.astype(np.float64)
    return (u - cx) / f * z, (v - cy) / f * z


@pytest.mark.parametrize("centre", ["half", "odd"])
@pytest.mark.parametrize("f", FOCALS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_unproject_np_against_the_reference_formula(shape, f, centre):
    h, w = shape
    cx, cy = (w / 2, h / 2) if centre == "half" else (w / 2 + 0.3, h / 2 - 0.7)
    z = depth_map(h, w)
    got = pc.unproject_np(z, f, f, cx, cy).reshape(h, w)
    assert got.dtype == pc.vertex_dtype(False)
    assert np.array_equal(got["z"].view(np.uint32), z.view(np.uint32))
    worst = 0.0
    for name, ref in zip("xy", reference_xy(z, f, cx, cy)):
        zero = ref == 0
        assert np.all(got[name][zero] == 0)
        err = np.abs(got[name].astype(np.float64) - ref)[~zero] / np.abs(ref[~zero])
        worst = max(worst, float(err.max()))
    print(f"{h}x{w} f={f} {centre}: worst relative error {worst / 2.0 ** -24:.3f} * 2^-24 (bar 4)")
    assert worst <= BAR
    # the column of u == cx (w even, the reference's own centre) is exactly 0
    if centre == "half" and w % 2 == 0:
        assert np.all(got["x"][:, w // 2] == 0)
    if centre == "half" and h % 2 == 0:
        assert np.all(got["y"][h // 2, :] == 0)


def test_unproject_np_separate_focal_lengths_and_colour():
    h, w = 9, 5
    z = depth_map(h, w)
    got = pc.unproject_np(z, 3.7, 511.9, 2.5, 4.5, photo=photo(h, w)).reshape(h, w)
    f32 = np.float32
    for v, u in [(0, 0), (8, 4), (3, 2)]:
        assert got["x"][v, u] == (f32(u) - f32(2.5)) / f32(3.7) * z[v, u]
        assert got["y"][v, u] == (f32(v) - f32(4.5)) / f32(511.9) * z[v, u]
    assert got.dtype.itemsize == 15
    rgb = np.stack([got["red"], got["green"], got["blue"]], axis=-1)
    assert np.array_equal(rgb, photo(h, w))
    swapped = pc.unproject_np(z, 3.7, 511.9, 2.5, 4.5, photo=photo(h, w), swap_rb=True).reshape(h, w)
    assert np.array_equal(np.stack([swapped["red"], swapped["green"], swapped["blue"]], axis=-1),
                          photo(h, w)[..., ::-1])
    assert np.array_equal(swapped[["x", "y", "z"]], got[["x", "y", "z"]])


def test_organized_keeps_nan_and_every_pixel():
    h, w = 9, 5
    z = depth_map(h, w).copy()
    z[4, 1] = np.nan
    z[0, 0] = np.inf
    got = pc.unproject_np(z, 3.7, 3.7, w / 2, h / 2)
    assert got.shape == (h * w,)
    r = got[4 * w + 1]
    assert np.isnan(r["x"]) and np.isnan(r["y"]) and np.isnan(r["z"])
    assert np.isinf(got[0]["z"])


@pytest.mark.parametrize("step", [1, 2, 3])
def test_compact_semantics(step):
    """Order, inclusive bounds, NaN / +-inf dropped, on a size no step divides."""
    h, w = 37, 53
    z_lo, z_hi = np.float32(1e-4), np.float32(1e4)
    z = depth_map(h, w).copy()
    rng = np.random.Generator(np.random.PCG64(step))
    z[rng.random((h, w)) < 0.3] = 0.0          # below the range
    z[0, 0], z[0, step] = z_lo, z_hi           # exactly at both bounds: kept
    z[step, 0] = np.nextafter(z_lo, np.float32(0))
    z[step, step] = np.nextafter(z_hi, np.float32(np.inf))
    z[2 * step, 0], z[2 * step, step], z[2 * step, 2 * step] = np.nan, np.inf, -np.inf
    z[36 - 36 % step, 52 - 52 % step] = 7.0    # the last sample: kept
    full = pc.unproject_np(z, 60.0, 61.0, w / 2, h / 2, photo=photo(h, w), step=step)
    got = pc.unproject_np(z, 60.0, 61.0, w / 2, h / 2, photo=photo(h, w), step=step, compact=True, z_lo=z_lo,
                          z_hi=z_hi)
    hs, ws = pc.grid(h, w, step)
    assert (hs, ws) == (-(-h // step), -(-w // step)) and full.shape == (hs * ws,)
    # a literal loop over the samples in row-major order
    want = [full[i * ws + j] for i in range(hs) for j in range(ws)
            if z[i * step, j * step] == z[i * step, j * step] and z_lo <= z[i * step, j * step] <= z_hi]
    assert got.shape == (len(want),) and 0 < len(want) < hs * ws
    assert got.tobytes() == b"".join(r.tobytes() for r in want)
    zs = got["z"]
    assert zs[0] == z_lo and zs[1] == z_hi and zs[-1] == 7.0
    assert np.isfinite(zs).all() and zs.min() >= z_lo and zs.max() <= z_hi
    for bad in (z[step, 0], z[step, step]):
        assert bad not in zs
    # each kept record is the organized record of its pixel
    i, j = 0, 1
    assert got[1] == full[i * ws + j] and got[1]["x"] == (np.float32(j * step) - np.float32(w / 2)) / np.float32(60) * z_hi


@pytest.mark.parametrize("colour", [True, False])
def test_ply_round_trip(tmp_path, colour):
    h, w = 9, 5
    rec = pc.unproject_np(depth_map(h, w), 3.7, 3.7, w / 2, h / 2, photo=photo(h, w) if colour else None)
    path = tmp_path / "cloud.ply"
    pc.write_ply(path, rec)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 45\n"
              "property float x\nproperty float y\nproperty float z\n")
    if colour:
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += "end_header\n"
    data = path.read_bytes()
    assert data.startswith(header.encode("ascii"))
    assert len(data) == len(header) + 45 * (15 if colour else 12)
    assert data[len(header):] == rec.tobytes()
    back = pc.read_ply(path)
    assert back.dtype == pc.vertex_dtype(colour) and back.dtype.itemsize == (15 if colour else 12)
    assert back.tobytes() == rec.tobytes()
    # an empty cloud is a header and nothing else
    pc.write_ply(path, rec[:0])
    assert pc.read_ply(path).shape == (0,) and b"element vertex 0\n" in path.read_bytes()


def test_ply_refuses_other_input(tmp_path):
    with pytest.raises(ValueError):
        pc.write_ply(tmp_path / "a.ply", np.zeros((3, 3), np.float32))
    (tmp_path / "b.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        pc.read_ply(tmp_path / "b.ply")
    rec = pc.unproject_np(depth_map(9, 5), 3.7, 3.7, 2.5, 4.5)
    pc.write_ply(tmp_path / "c.ply", rec)
    (tmp_path / "c.ply").write_bytes((tmp_path / "c.ply").read_bytes()[:-1])
    with pytest.raises(ValueError):
        pc.read_ply(tmp_path / "c.ply")


def test_vertex_dtype_is_packed():
    c, n = pc.vertex_dtype(True), pc.vertex_dtype(False)
    assert c.itemsize == 15 and n.itemsize == 12
    assert c.names == ("x", "y", "z", "red", "green", "blue") and n.names == ("x", "y", "z")
    assert [c.fields[k][1] for k in c.names] == [0, 4, 8, 12, 13, 14]
    assert all(c.fields[k][0] == np.dtype("<f4") for k in "xyz")


@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


P = ctypes.c_void_p(4096)  # never dereferenced: the checks run first
BIG = 2 ** 31 - 256        # a sampled grid of this many samples is refused


@pytest.mark.parametrize("kw, msg", [
    (dict(depth=None), b"null"), (dict(records=None), b"null"), (dict(counts=None), b"null"),
    (dict(batch=0), b"positive"), (dict(h=0), b"positive"), (dict(w=-1), b"positive"), (dict(step=0), b"step"),
    (dict(step=-2), b"step"),
    (dict(photo=P, pitch=23), b"pitch"),
    (dict(f=None, fx=0.0), b"fx"), (dict(f=None, fy=-1.0), b"fx"), (dict(f=None, fx=float("nan")), b"fx"),
    (dict(h=1, w=BIG, nbytes=1 << 62), b"2^31"), (dict(h=65536, w=32768, nbytes=1 << 62), b"2^31"),
    (dict(batch=65536, nbytes=1 << 40), b"65535"),
    (dict(nbytes=8 * 8 * 12 - 1), b"records_bytes"), (dict(photo=P, pitch=24, nbytes=8 * 8 * 15 - 1), b"records_bytes"),
    (dict(batch=2, nbytes=2 * 8 * 8 * 12 - 1), b"records_bytes"),
    (dict(step=3, nbytes=3 * 3 * 12 - 1), b"records_bytes"),
    (dict(compact=1, ws=None), b"ws"), (dict(compact=1, ws_bytes=3), b"ws"),
    (dict(compact=1, h=40, w=40, nbytes=1 << 20, ws_bytes=4), b"ws"),
    (dict(compact=1, z_lo=2.0, z_hi=1.0), b"z_lo"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_point_cloud_checks_arguments_before_any_device_call(lib, kw, msg):
    def call(depth=P, batch=1, h=8, w=8, step=1, photo=None, pitch=0, f=P, fx=0.0, fy=0.0, compact=0, z_lo=1e-4,
             z_hi=1e4, records=P, nbytes=8 * 8 * 15, counts=P, ws=P, ws_bytes=1 << 20):
        return lib.mde_op_point_cloud(depth, batch, h, w, step, photo, pitch, 0, f, fx, fy, 4.0, 4.0, compact, z_lo,
                                      z_hi, records, nbytes, counts, ws, ws_bytes, None)

    if "fy" in kw:
        kw = dict(kw, fx=1.0)
    elif "fx" in kw:
        kw = dict(kw, fy=1.0)
    assert call(**kw) == 1, kw
    err = lib.mde_last_error()
    assert b"mde_op_point_cloud:" in err and msg in err, (kw, err)


def test_point_cloud_ws_bytes(lib):
    """One int per workgroup of 1024 samples and image; 0 for what the op refuses."""
    f = lib.mde_op_point_cloud_ws_bytes
    assert f(1, 8, 8, 1) == 4 and f(1, 32, 32, 1) == 4 and f(1, 32, 33, 1) == 8
    assert f(2, 600, 800, 1) == 2 * 469 * 4 and f(1, 600, 800, 2) == 4 * -(-300 * 400 // 1024)
    assert f(0, 8, 8, 1) == 0 and f(1, 8, 8, 0) == 0 and f(1, 1, BIG, 1) == 0 and f(65536, 8, 8, 1) == 0


def test_driver_parsers_accept_the_ply_flags():
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run as dav2
    from monocular_depth_estimation_trt_amd.models.depth_pro import run as dp
    a = dp.build_parser().parse_args(["--ply", "out.ply", "--ply-step", "2"])
    assert a.ply == "out.ply" and a.ply_step == 2
    d = dp.build_parser().parse_args([])
    assert d.ply == "" and d.ply_step == 1
    a = dav2.build_parser().parse_args(["--ply", "out.ply", "--f-px", "500"])
    assert a.ply == "out.ply" and a.ply_step == 1 and a.f_px == 500.0


def test_drivers_refuse_ply_they_cannot_serve():
    from monocular_depth_estimation_trt_amd.models.depth_anything_ac import run as ac
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run as dav2
    from monocular_depth_estimation_trt_amd.models.depth_pro import run as dp
    from monocular_depth_estimation_trt_amd.models.distill_any_depth import run as distill
    with pytest.raises(SystemExit) as e:
        dp.main(["--ply", "out.ply", "--host-postprocess"])
    assert "--ply" in str(e.value) and "device post-process" in str(e.value)
    with pytest.raises(SystemExit) as e:
        dp.main(["--ply", "out.ply", "--ply-step", "0"])
    assert "--ply-step" in str(e.value)
    with pytest.raises(SystemExit) as e:
        dav2.main(["--source", "synthetic:vits:metric:1234", "--ply", "out.ply"])
    assert "--f-px" in str(e.value)
    with pytest.raises(SystemExit) as e:
        dav2.main(["--source", "synthetic:vits:relative:1234", "--ply", "out.ply", "--f-px", "500"])
    assert "metric" in str(e.value)
    for relative in (ac, distill):
        with pytest.raises(SystemExit) as e:
            relative.main(["--ply", "out.ply", "--f-px", "500"])
        assert "metric" in str(e.value)
