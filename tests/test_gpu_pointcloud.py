"""Point clouds on the device (csrc/point_cloud.hip) through the C ABI, the Python owner
(pointcloud.DevicePointCloud) and the two drivers' --ply.

Every comparison is bit-exact: the record bytes the device wrote, as uint8, against the bytes of
pointcloud.unproject_np (held to the reference's formula in tests/test_pointcloud_cpu.py).  Every
call writes into a buffer filled with 0xA5 and the helper checks that nothing but the counted
records of each image's region changed: the bytes before the base pointer, the bytes of a region
past counts[b] records, and the bytes after the last region.

Workgroup sizes, for the shapes below: point_cloud.hip gives one workgroup of 256 threads a tile
of 1024 samples, and scans the tiles' counts with one workgroup of 256 threads per image, 256
tiles at a time.  9 x 5 = 45 samples is less than one wave; 37 x 53 = 1961 is 2 tiles, the second
partly filled; 100 x 76 = 7600 is 8 tiles; 600 x 800 = 480000 is 469 tiles, more than the scan
workgroup's 256 threads, so its scan takes two rounds with a carry.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_util import op, ptr, stream

from monocular_depth_estimation_trt_amd import _lib
from monocular_depth_estimation_trt_amd import pointcloud as pc

pytestmark = pytest.mark.gpu

SHAPES = [(9, 5), (37, 53), (100, 76), (600, 800)]
FILL = 0xA5
PAD = 64          # guard bytes before the base pointer and after the last region
Z_LO, Z_HI = np.float32(0.25), np.float32(80.0)
PATTERNS = ["all", "none", "last", "first", "checker", "random", "run64", "nonfinite", "bounds"]


@functools.lru_cache(maxsize=None)
def base_depth(h, w, batch=1):
    """[batch][h][w] uniform in [1, 50], inside [Z_LO, Z_HI]; cached, never written."""
    rng = np.random.Generator(np.random.PCG64(h * 10007 + w))
    z = rng.uniform(1.0, 50.0, size=(batch, h, w)).astype(np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def photo(h, w, batch=1):
    rng = np.random.Generator(np.random.PCG64(h * 131 + w + 7))
    a = rng.integers(0, 256, size=(batch, h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def pattern_depth(name, h, w, seed=0):
    """One [h][w] map whose validity under [Z_LO, Z_HI] follows `name`; invalid = 0 unless said."""
    z = np.array(base_depth(h, w)[0])
    flat = z.reshape(-1)
    n = flat.size
    if name == "none":
        flat[:] = 0.0
    elif name == "last":
        flat[:-1] = 0.0
    elif name == "first":
        flat[1:] = 0.0
    elif name == "checker":
        vv, uu = np.mgrid[0:h, 0:w]
        z[(vv + uu) % 2 == 1] = 0.0
    elif name == "random":
        rng = np.random.Generator(np.random.PCG64(1000 + seed))
        flat[rng.random(n) < 0.5] = 0.0
    elif name == "run64":     # one whole wave's samples of a pass, and one run across two waves
        for start in (min(320, max(n - 64, 0)), min(1024 + 37, max(n - 64, 0))):
            flat[start:start + 64] = 0.0
    elif name == "nonfinite":
        for i, bad in zip((n // 3, n // 3 + 1, n // 2, n - 2), (np.nan, np.inf, -np.inf, np.nan)):
            flat[i] = bad
    elif name == "bounds":
        flat[0], flat[1] = Z_LO, Z_HI
        flat[2], flat[3] = np.nextafter(Z_LO, np.float32(0)), np.nextafter(Z_HI, np.float32(np.inf))
        flat[n - 1], flat[n - 2] = Z_HI, Z_LO
    else:
        assert name == "all"
    return z


def device_cloud(depth, img=None, pitch=None, swap_rb=0, step=1, f_dev=None, fx=0.0, fy=0.0, cx=None, cy=None,
                 compact=1, z_lo=Z_LO, z_hi=Z_HI, offset=0):
    """Run mde_op_point_cloud on depth [B][h][w] (and img [B][h][w][3], rows padded with 0xFF to
    `pitch`) with the records at `offset` bytes past a 16-byte boundary.  Checks the guards and
    returns (counts [B], [the bytes of image b's region]); `f_dev`: per-image focal lengths."""
    B, h, w = depth.shape
    hs, ws = pc.grid(h, w, step)
    rec = 15 if img is not None else 12
    region = hs * ws * rec
    d_depth = torch.from_numpy(np.array(depth)).cuda()
    d_photo = None
    if img is not None:
        pitch = pitch or 3 * w
        rows = np.full((B, h, pitch), 0xFF, np.uint8)
        rows[:, :, :3 * w] = img.reshape(B, h, 3 * w)
        d_photo = torch.from_numpy(rows).cuda()
    d_f = None if f_dev is None else torch.from_numpy(np.asarray(f_dev, np.float32)).cuda()
    d_rec = torch.full((PAD + offset + B * region + PAD,), FILL, dtype=torch.uint8, device="cuda")
    assert d_rec.data_ptr() % 16 == 0
    d_cnt = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    need = pc.ws_bytes(B, h, w, step)
    assert need == B * -(-hs * ws // 1024) * 4
    d_ws = torch.full((need + 16,), FILL, dtype=torch.uint8, device="cuda")
    op("mde_op_point_cloud", ptr(d_depth), B, h, w, step, ptr(d_photo), pitch or 0, swap_rb, ptr(d_f), float(fx),
       float(fy), float(w / 2 if cx is None else cx), float(h / 2 if cy is None else cy), compact, float(z_lo),
       float(z_hi), C.c_void_p(d_rec.data_ptr() + PAD + offset), B * region, ptr(d_cnt),
       ptr(d_ws) if compact else None, need if compact else 0, stream())
    out, cnt, wsb = d_rec.cpu().numpy(), d_cnt.cpu().numpy(), d_ws.cpu().numpy()
    assert cnt[B] == -7
    assert (wsb[need:] == FILL).all(), "scratch written past mde_op_point_cloud_ws_bytes"
    assert (out[:PAD + offset] == FILL).all(), "bytes before the base pointer written"
    assert (out[PAD + offset + B * region:] == FILL).all(), "bytes after the last region written"
    body = out[PAD + offset:PAD + offset + B * region]
    regions = [body[b * region:(b + 1) * region] for b in range(B)]
    for b in range(B):
        assert 0 <= cnt[b] <= hs * ws, cnt
        assert (regions[b][int(cnt[b]) * rec:] == FILL).all(), f"image {b}: bytes past counts[b] records written"
    return cnt[:B], regions


def expect(depth, fx, fy, img=None, swap_rb=0, step=1, cx=None, cy=None, compact=1, z_lo=Z_LO, z_hi=Z_HI):
    h, w = depth.shape
    return pc.unproject_np(depth, fx, fy, w / 2 if cx is None else cx, h / 2 if cy is None else cy, photo=img,
                           swap_rb=bool(swap_rb), step=step, compact=bool(compact), z_lo=z_lo, z_hi=z_hi)


def same_bytes(region, want, count):
    """The first `count` records of the region against the restatement's bytes."""
    assert int(count) == want.shape[0], (int(count), want.shape[0])
    got = region[:want.nbytes]
    ref = np.frombuffer(want.tobytes(), np.uint8)
    bad = got != ref
    assert not bad.any(), (int(bad.sum()), (np.flatnonzero(bad)[:6] // want.dtype.itemsize).tolist())


@pytest.mark.parametrize("colour", [True, False], ids=["rgb", "xyz"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_organized_bit_exact(gpu, shape, colour):
    """Every sample written, a NaN depth giving NaN x, y, z; counts = hs * ws."""
    h, w = shape
    z = np.array(base_depth(h, w))
    z[0, h // 2, w // 3] = np.nan
    img = photo(h, w) if colour else None
    cnt, regions = device_cloud(z, img, fx=0.8 * w + 0.37, fy=0.7 * w + 0.11, compact=0)
    want = expect(z[0], 0.8 * w + 0.37, 0.7 * w + 0.11, None if img is None else img[0], compact=0)
    assert cnt[0] == h * w and np.isnan(want["x"]).sum() == 1
    same_bytes(regions[0], want, cnt[0])


@pytest.mark.parametrize("colour", [True, False], ids=["rgb", "xyz"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_compact_random_bit_exact(gpu, shape, colour):
    h, w = shape
    z = pattern_depth("random", h, w)[None]
    img = photo(h, w) if colour else None
    cnt, regions = device_cloud(z, img, fx=0.8 * w + 0.37, fy=0.8 * w + 0.37, cx=w / 2 + 0.3, cy=h / 2 - 0.7)
    want = expect(z[0], 0.8 * w + 0.37, 0.8 * w + 0.37, None if img is None else img[0], cx=w / 2 + 0.3,
                  cy=h / 2 - 0.7)
    assert 0 < cnt[0] < h * w
    same_bytes(regions[0], want, cnt[0])


@pytest.mark.parametrize("swap_rb", [0, 1])
@pytest.mark.parametrize("compact", [0, 1], ids=["organized", "compact"])
@pytest.mark.parametrize("step", [1, 2, 3])
def test_step_swap_and_padded_pitch(gpu, step, compact, swap_rb):
    """37 x 53, which no step divides; rows 5 bytes longer than 3 * w, the padding 0xFF."""
    h, w = 37, 53
    z = pattern_depth("checker" if step == 1 else "random", h, w, seed=step)[None]
    cnt, regions = device_cloud(z, photo(h, w), pitch=3 * w + 5, swap_rb=swap_rb, step=step, fx=61.5, fy=60.25,
                                compact=compact)
    want = expect(z[0], 61.5, 60.25, photo(h, w)[0], swap_rb=swap_rb, step=step, compact=compact)
    hs, ws = pc.grid(h, w, step)
    assert (cnt[0] == hs * ws) if not compact else (0 < cnt[0] < hs * ws)
    same_bytes(regions[0], want, cnt[0])


@pytest.mark.parametrize("shape", [(37, 53), (100, 76)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", PATTERNS)
def test_validity_patterns(gpu, name, shape):
    h, w = shape
    z = pattern_depth(name, h, w)[None]
    cnt, regions = device_cloud(z, photo(h, w), fx=61.5, fy=61.5)
    want = expect(z[0], 61.5, 61.5, photo(h, w)[0])
    n = h * w
    fixed = {"all": n, "none": 0, "last": 1, "first": 1, "checker": (n + 1) // 2, "run64": n - 128,
             "nonfinite": n - 4, "bounds": n - 2}
    if name in fixed:
        assert cnt[0] == fixed[name]
    if name == "none":
        assert (regions[0] == FILL).all()  # not one byte
    same_bytes(regions[0], want, cnt[0])


@pytest.mark.parametrize("name", ["all", "none", "last", "first", "run64"])
def test_validity_patterns_many_tiles(gpu, name):
    """469 tiles: the scan of the tile counts takes two rounds of its 256 threads."""
    h, w = 600, 800
    z = pattern_depth(name, h, w)[None]
    cnt, regions = device_cloud(z, photo(h, w), fx=700.0, fy=700.0)
    same_bytes(regions[0], expect(z[0], 700.0, 700.0, photo(h, w)[0]), cnt[0])


@pytest.mark.parametrize("colour", [True, False], ids=["rgb", "xyz"])
@pytest.mark.parametrize("compact", [0, 1], ids=["organized", "compact"])
def test_batch2_device_focal_lengths(gpu, compact, colour):
    """Two images, different validity and different device focal lengths; image 1's region starts
    at byte hs * ws * rec, an odd offset with 15-byte records (1961 * 15)."""
    h, w = 37, 53
    z = np.stack([pattern_depth("random", h, w, seed=1), pattern_depth("checker", h, w)])
    img = photo(h, w, 2) if colour else None
    f = np.array([61.5, 47.125], np.float32)
    cnt, regions = device_cloud(z, img, f_dev=f, fx=-1.0, fy=-1.0, compact=compact)
    for b in range(2):
        want = expect(z[b], f[b], f[b], None if img is None else img[b], compact=compact)
        same_bytes(regions[b], want, cnt[b])
    if compact:
        assert cnt[0] != cnt[1]
    if colour:
        assert (h * w * 15) % 2 == 1
    assert not np.array_equal(regions[0][:1200], regions[1][:1200])


@pytest.mark.parametrize("compact", [0, 1], ids=["organized", "compact"])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_unaligned_base_and_guards(gpu, offset, compact):
    """The base pointer 0..3 bytes past a 16-byte boundary, two images of 15-byte records
    (device_cloud holds every byte outside the counted records to the 0xA5 fill)."""
    h, w = 37, 53
    z = np.stack([pattern_depth("random", h, w, seed=2), pattern_depth("last", h, w)])
    cnt, regions = device_cloud(z, photo(h, w, 2), fx=61.5, fy=61.5, compact=compact, offset=offset)
    for b in range(2):
        same_bytes(regions[b], expect(z[b], 61.5, 61.5, photo(h, w, 2)[b], compact=compact), cnt[b])


def test_deterministic(gpu):
    h, w = 600, 800
    z = pattern_depth("random", h, w)[None]
    a_cnt, a = device_cloud(z, photo(h, w), fx=700.0, fy=700.0)
    b_cnt, b = device_cloud(z, photo(h, w), fx=700.0, fy=700.0)
    assert np.array_equal(a_cnt, b_cnt) and np.array_equal(a[0], b[0])


def test_device_point_cloud_in_a_captured_graph(gpu):
    """One DevicePointCloud.enqueue (compact: three kernels) captured into a torch.cuda.graph on a
    side stream, replayed twice with the depth changed in between."""
    h, w = 100, 76
    za, zb = pattern_depth("random", h, w, seed=3), pattern_depth("checker", h, w)
    img = photo(h, w)[0]
    d_depth = torch.from_numpy(za).cuda()
    d_photo = torch.from_numpy(np.array(img)).cuda()
    with pc.DevicePointCloud(1, h, w, colour=True) as cloud:
        kw = dict(d_photo=d_photo.data_ptr(), pitch=3 * w, swap_rb=True, fx=61.5, z_lo=Z_LO, z_hi=Z_HI)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            cloud.enqueue(d_depth.data_ptr(), s.cuda_stream, **kw)  # warm: the kernels are loaded
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            cloud.enqueue(d_depth.data_ptr(), s.cuda_stream, **kw)
        for z in (za, zb):
            d_depth.copy_(torch.from_numpy(z))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            cloud.download(0)
            got = cloud.result()[0]
            want = expect(z, 61.5, 61.5, img, swap_rb=1)
            assert got.dtype == pc.vertex_dtype(True) and got.shape == want.shape
            assert got.tobytes() == want.tobytes()
    with pytest.raises(RuntimeError):
        cloud.result()  # freed


def test_device_point_cloud_run_batch2(gpu):
    """run() = enqueue, counts, the counted bytes: per-image views, organized and compact."""
    h, w = 37, 53
    z = np.stack([pattern_depth("random", h, w, seed=4), pattern_depth("first", h, w)])
    d_depth = torch.from_numpy(z).cuda()
    d_f = torch.tensor([61.5, 47.125], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pc.DevicePointCloud(2, h, w, colour=False, step=2) as cloud:
        for compact in (True, False):
            got = cloud.run(d_depth.data_ptr(), 0, d_f_px=d_f.data_ptr(), compact=compact, z_lo=Z_LO, z_hi=Z_HI)
            for b, f in enumerate((61.5, 47.125)):
                want = expect(z[b], f, f, step=2, compact=compact)
                assert got[b].tobytes() == want.tobytes(), (compact, b)
        with pytest.raises(ValueError):
            cloud.enqueue(d_depth.data_ptr(), 0, d_photo=d_depth.data_ptr(), fx=1.0)  # built without colour
        with pytest.raises(ValueError):
            cloud.enqueue(d_depth.data_ptr(), 0)  # no focal length
    with pytest.raises(_lib.MDEError):
        pc.point_cloud(d_depth.data_ptr(), 1, h, w, 1, 0, 0, False, 0, 0.0, 0.0, 1.0, 1.0, False, 0.0, 1.0,
                       d_depth.data_ptr(), 1 << 20, d_f.data_ptr(), 0, 0)


@pytest.fixture(scope="module")
def dp_driver(gpu, tmp_path_factory):
    """Depth Pro run.main on a 300 x 400 photo with extra flags -> ((depth, f_px), stdout part)."""
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    td = tmp_path_factory.mktemp("pc_dp")
    np.save(td / "src.npy", photo(300, 400)[0])
    args = ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(td / "e_fp16.mdeng"), "--iterations", "2",
            "--warmup", "1", "--image", str(td / "src.npy"), "--out-dir", str(td / "bench")]

    def call(*extra):
        return run.main(args + list(extra))

    return call, td


def check_driver_cloud(path, depth, f_px, bgr, step, z_lo, z_hi):
    cloud = pc.read_ply(path)
    want = pc.unproject_np(depth, f_px, f_px, depth.shape[1] / 2, depth.shape[0] / 2, photo=bgr, swap_rb=True,
                           step=step, compact=True, z_lo=z_lo, z_hi=z_hi)
    assert cloud.dtype == pc.vertex_dtype(True)
    assert cloud.shape == want.shape and cloud.tobytes() == want.tobytes()
    return cloud


def test_depth_pro_driver_ply(dp_driver, capsys):
    call, td = dp_driver
    bgr = photo(300, 400)[0]
    depth, f_px = call("--ply", str(td / "full.ply"))
    out = capsys.readouterr().out
    assert "[MDET] point cloud (device, kernels + D2H, hipEvents)" in out and "120000 points" in out
    cloud = check_driver_cloud(td / "full.ply", depth, np.float32(f_px), bgr, 1, 1e-4, 1e4)
    assert cloud.shape == (300 * 400,)  # the depth is already clamped into the range
    assert np.array_equal(cloud["z"].view(np.uint32), depth.reshape(-1).view(np.uint32))
    rgb = np.stack([cloud["red"], cloud["green"], cloud["blue"]], axis=-1)
    assert np.array_equal(rgb, bgr.reshape(-1, 3)[:, ::-1])
    depth2, f2 = call("--ply", str(td / "half.ply"), "--ply-step", "2")
    assert np.array_equal(depth2, depth) and f2 == f_px
    assert check_driver_cloud(td / "half.ply", depth, np.float32(f_px), bgr, 2, 1e-4, 1e4).shape == (150 * 200,)


def test_depth_pro_driver_ply_given_focal_length(dp_driver):
    call, td = dp_driver
    depth, f_px = call("--ply", str(td / "f.ply"), "--f-px", "500", "--ply-step", "3")
    assert f_px == 500.0
    check_driver_cloud(td / "f.ply", depth, 500.0, photo(300, 400)[0], 3, 1e-4, 1e4)


def test_dav2_driver_ply(gpu, tmp_path, capsys):
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    bgr = photo(300, 400)[0]
    np.save(tmp_path / "src.npy", bgr)
    args = ["--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--image",
            str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench"), "--f-px", "500"]
    depth = run.main(args + ["--source", "synthetic:vits:metric:1234", "--ply", str(tmp_path / "m.ply")])
    out = capsys.readouterr().out
    assert "[MDET] point cloud (device, kernels + D2H, hipEvents)" in out
    cloud = check_driver_cloud(tmp_path / "m.ply", depth, 500.0, bgr, 1, 1e-3, 1e3)
    assert cloud.shape == (300 * 400,)  # clamped to [1e-3, 1e3] by the post-process
    with pytest.raises(SystemExit) as e:
        run.main(args + ["--source", "synthetic:vits:relative:1234", "--ply", str(tmp_path / "r.ply")])
    assert "metric" in str(e.value) and not (tmp_path / "r.ply").exists()
