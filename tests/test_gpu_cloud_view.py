"""The point-cloud preview on the device (csrc/cloud_view.hip) through the C ABI, the Python owner
(pointcloud.DeviceCloudView), the two drivers' --cloud-view and the stream driver's --cloud-view-out.

Every comparison is exact: the picture byte for byte and the view row as float64 with NaN equal to NaN,
against pointcloud.render_np (held to the reference's render_points in tests/test_cloud_view_cpu.py).
device_view() puts the picture, the view rows and the scratch inside 0xA5-filled guards that must survive,
hands the scratch over dirty (0xA5 everywhere) and makes every call twice: the bytes must be identical.

Sizes, for the shapes below: cloud_view.hip gives a thread one sample (256 per workgroup) and the quantile
kernels a workgroup 4096 values.  9 x 5 = 45 samples is less than a wave; 37 x 53 = 1961 is 8 workgroups,
the last partly filled, and one quantile tile; 100 x 131 = 13100 is three quantile tiles and a partial one.
On the 64 x 80 picture of the 100 x 131 map 2.5 samples fall on a pixel on average and on the 7 x 9 and 1 x 1
pictures hundreds to thousands, so the 64-bit minimum and the index rule decide nearly every pixel.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cloud_view_cases as cases
from gpu_util import ptr, stream

from monocular_depth_estimation_trt_amd import _lib
from monocular_depth_estimation_trt_amd import pointcloud as pc

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64  # guard bytes; a multiple of 8, so the pointers behind it stay 8-byte aligned
SHAPES = [(9, 5), (37, 53), (100, 131)]
SIZES = [(1, 1), (7, 9), (41, 41), (64, 80)]
BG = np.array(pc.VIEW_BG, np.uint8)


def guarded(nbytes):
    t = torch.full((PAD + nbytes + PAD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t


def body(t, nbytes, what):
    a = t.cpu().numpy()
    assert (a[:PAD] == FILL).all(), f"{what}: bytes before the buffer written"
    assert (a[PAD + nbytes:] == FILL).all(), f"{what}: bytes after the buffer written"
    return a[PAD:PAD + nbytes].copy()


def device_view(depth, img=None, pitch=None, swap_rb=0, step=1, f_dev=None, cam=None, size=(41, 41),
                angles=pc.VIEW_ANGLES, view_in=None, bg=pc.VIEW_BG, out_swap_rb=0, depth_off=0):
    """mde_op_cloud_view on depth [B][h][w] (and img [B][h][w][3], rows padded with 0xFF to `pitch`), twice,
    inside guards; `depth_off`: floats the depth pointer sits past a 16-byte boundary; `f_dev`: per-image
    device focal lengths; `view_in`: [B][8] rows.  Returns (pictures [B, out_h, out_w, 3], rows [B, 8])."""
    B, h, w = depth.shape
    out_h, out_w = size
    fx, fy, cx, cy = cam or cases.camera(h, w)
    d_depth = torch.zeros(B * h * w + 4, dtype=torch.float32, device="cuda")
    d_depth[depth_off:depth_off + B * h * w] = torch.from_numpy(np.array(depth).reshape(-1))
    assert (d_depth.data_ptr() + 4 * depth_off) % 16 == (4 * depth_off) % 16
    d_photo = None
    if img is not None:
        pitch = pitch or 3 * w
        rows = np.full((B, h, pitch), 0xFF, np.uint8)
        rows[:, :, :3 * w] = img.reshape(B, h, 3 * w)
        d_photo = torch.from_numpy(rows).cuda()
    d_f = None if f_dev is None else torch.from_numpy(np.asarray(f_dev, np.float32)).cuda()
    d_vin = None if view_in is None else torch.from_numpy(np.ascontiguousarray(view_in, np.float64).reshape(B, 8)).cuda()
    need = pc.cloud_view_ws_bytes(B, h, w, step, out_h, out_w)
    assert need > B * out_h * out_w * 8 and need % 8 == 0
    runs = []
    for _ in range(2):
        d_out, d_view, d_ws = guarded(B * out_h * out_w * 3), guarded(B * 64), guarded(need)
        pc.cloud_view(d_depth.data_ptr() + 4 * depth_off, B, h, w, step, 0 if d_photo is None else d_photo.data_ptr(),
                      pitch or 0, swap_rb, 0 if d_f is None else d_f.data_ptr(), -1.0 if f_dev is not None else fx,
                      -1.0 if f_dev is not None else fy, cx, cy, pc.view_trig(*angles),
                      0 if d_vin is None else d_vin.data_ptr(), bg, out_swap_rb, d_out.data_ptr() + PAD, out_h, out_w,
                      d_view.data_ptr() + PAD, d_ws.data_ptr() + PAD, need, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        body(d_ws, need, "scratch")
        runs.append((body(d_out, B * out_h * out_w * 3, "picture"), body(d_view, B * 64, "view rows")))
    assert runs[0][0].tobytes() == runs[1][0].tobytes(), "the picture differs between two runs"
    assert runs[0][1].tobytes() == runs[1][1].tobytes(), "the view rows differ between two runs"
    return runs[0][0].reshape(B, out_h, out_w, 3), runs[0][1].view(np.float64).reshape(B, 8)


def expect(depth, img=None, swap_rb=0, step=1, f=None, cam=None, size=(41, 41), angles=pc.VIEW_ANGLES, view=None,
           bg=pc.VIEW_BG, out_swap_rb=0):
    h, w = depth.shape
    fx, fy, cx, cy = cam or cases.camera(h, w)
    if f is not None:
        fx = fy = f
    pic, row = pc.render_np(depth, fx, fy, cx, cy, size=size, elev_deg=angles[0], azim_deg=angles[1], photo=img,
                            swap_rb=bool(swap_rb), step=step, view=view, bg=bg)
    return (pic[..., ::-1] if out_swap_rb else pic), row


def same(got_pic, got_row, want_pic, want_row):
    assert got_pic.shape == want_pic.shape
    bad = (got_pic != want_pic).any(axis=-1)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.array_equal(got_row, want_row, equal_nan=True), (got_row.tolist(), want_row.tolist())


@functools.lru_cache(maxsize=None)
def scene(h, w, seed=0):
    return cases.scene(h, w, seed)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_picture_sizes(gpu, shape, size):
    h, w = shape
    depth, photo = scene(h, w)
    off = 1 if shape == (37, 53) else 0  # the depth pointer 4 bytes off 16-byte alignment
    pics, rows = device_view(depth[None], photo[None], size=size, depth_off=off)
    want = expect(depth, photo, size=size)
    same(pics[0], rows[0], *want)
    if size == (64, 80) and shape == (100, 131):
        assert want[1][pc.V_INSIDE] > 2 * (want[0] != BG).any(axis=-1).sum()  # pixels are shared


@pytest.mark.parametrize("angles", cases.ANGLES, ids=lambda a: "%g_%g" % a)
def test_angles(gpu, angles):
    h, w = 37, 53
    depth, photo = scene(h, w)
    pics, rows = device_view(depth[None], photo[None], size=(41, 41), angles=angles)
    same(pics[0], rows[0], *expect(depth, photo, size=(41, 41), angles=angles))


@pytest.mark.parametrize("out_swap_rb", [0, 1])
@pytest.mark.parametrize("swap_rb", [0, 1])
@pytest.mark.parametrize("step", [1, 2, 3])
def test_step_swaps_and_padded_pitch(gpu, step, swap_rb, out_swap_rb):
    """37 x 53, which no step divides; rows 5 bytes longer than 3 * w, the padding 0xFF."""
    h, w = 37, 53
    depth, photo = scene(h, w, seed=step)
    pics, rows = device_view(depth[None], photo[None], pitch=3 * w + 5, swap_rb=swap_rb, step=step, size=(41, 41),
                             out_swap_rb=out_swap_rb, bg=(1, 2, 3))
    want = expect(depth, photo, swap_rb=swap_rb, step=step, size=(41, 41), out_swap_rb=out_swap_rb, bg=(1, 2, 3))
    same(pics[0], rows[0], *want)
    assert (want[0] == np.array((3, 2, 1) if out_swap_rb else (1, 2, 3), np.uint8)).all(axis=-1).any()


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "%dx%d" % s)
def test_without_a_photo(gpu, shape):
    h, w = shape
    depth, _ = scene(h, w)
    pics, rows = device_view(depth[None], size=(7, 9))
    want = expect(depth, size=(7, 9))
    same(pics[0], rows[0], *want)
    assert (pics[0] == pc.VIEW_GREY).all(axis=-1).any()


@pytest.mark.parametrize("angles", [(0.0, 0.0), pc.VIEW_ANGLES], ids=["front", "default"])
@pytest.mark.parametrize("name", cases.DEGENERATE)
def test_degenerate_maps(gpu, name, angles):
    z, cam = cases.degenerate(name)
    col = cases.colours(9, 5)
    for size in ((7, 9), (3, 3)):
        pics, rows = device_view(z[None], col[None], cam=cam, size=size, angles=angles)
        same(pics[0], rows[0], *expect(z, col, cam=cam, size=size, angles=angles))
    if name == "all_invalid":
        assert (pics[0] == BG).all() and rows[0].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 0.46 * 3, 0.0, 0.0]
    if name == "two_on_one_pixel" and angles == (0.0, 0.0):
        assert rows[0][pc.V_INSIDE] == 2 and (pics[0] != BG).any(axis=-1).sum() == 1
        assert pics[0][(pics[0] != BG).any(axis=-1)][0].tolist() == col[4, 4].tolist()  # the nearer, later sample


def test_batch2_device_focal_lengths(gpu):
    h, w = 37, 53
    depth = np.stack([scene(h, w)[0], scene(h, w, seed=5)[0]])
    photo = np.stack([scene(h, w)[1], scene(h, w, seed=5)[1]])
    f = np.array([47.5, 61.125], np.float32)
    pics, rows = device_view(depth, photo, f_dev=f, size=(41, 41))
    for b in range(2):
        same(pics[b], rows[b], *expect(depth[b], photo[b], f=f[b], size=(41, 41)))
    assert not np.array_equal(rows[0], rows[1])


def test_view_in_round_half_even(gpu):
    """elev = azim = 0, centre 0, scale 1, X and Y on multiples of 0.5: x1 * scale + out_w / 2 lands exactly
    on k + 0.5 and round-half-even decides."""
    z, fx, fy, cx, cy, view = cases.half_grid()
    col = cases.colours(*z.shape)
    pics, rows = device_view(z[None], col[None], cam=(fx, fy, cx, cy), size=(8, 10), angles=(0.0, 0.0),
                             view_in=view[None])
    want = expect(z, col, cam=(fx, fy, cx, cy), size=(8, 10), angles=(0.0, 0.0), view=view)
    same(pics[0], rows[0], *want)
    assert rows[0][pc.V_INSIDE] > 0 and rows[0][1:6].tolist() == view[1:6].tolist()


def test_view_in_small_span_and_two_cameras(gpu):
    """A scale so large that most samples fall outside (slot 6 of the view row), and image 2 of a batch on
    another camera than image 1."""
    h, w = 37, 53
    depth = np.stack([scene(h, w)[0], scene(h, w, seed=5)[0]])
    photo = np.stack([scene(h, w)[1], scene(h, w, seed=5)[1]])
    _, auto = expect(depth[0], photo[0], size=(41, 41))
    tight, other = auto.copy(), auto.copy()
    tight[pc.V_SCALE] *= 8
    other[pc.V_C0] += 0.25
    other[pc.V_SCALE] *= 0.5
    views = np.stack([tight, other])
    pics, rows = device_view(depth, photo, size=(41, 41), view_in=views)
    for b in range(2):
        same(pics[b], rows[b], *expect(depth[b], photo[b], size=(41, 41), view=views[b]))
    assert 0 < rows[0][pc.V_INSIDE] < rows[0][pc.V_NVALID] / 4
    assert rows[1][pc.V_INSIDE] > rows[1][pc.V_NVALID] / 2


def test_device_cloud_view_in_a_captured_graph(gpu):
    """One DeviceCloudView.enqueue captured into a torch.cuda.graph on a side stream, replayed with the depth
    map changed in between."""
    h, w = 100, 131
    (za, img), zb = scene(h, w), scene(h, w, seed=5)[0]
    d_depth = torch.from_numpy(np.array(za)).cuda()
    d_photo = torch.from_numpy(np.array(img)).cuda()
    fx, fy, cx, cy = cases.camera(h, w)
    with pc.DeviceCloudView(1, h, w, (64, 80), colour=True) as cv:
        kw = dict(d_photo=d_photo.data_ptr(), pitch=3 * w, swap_rb=True, fx=fx, out_swap_rb=True)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            cv.enqueue(d_depth.data_ptr(), s.cuda_stream, **kw)  # warm: the kernels are loaded
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            cv.enqueue(d_depth.data_ptr(), s.cuda_stream, **kw)
        for z in (za, zb):
            d_depth.copy_(torch.from_numpy(np.array(z)))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            cv.download(0)
            want = expect(z, img, swap_rb=1, size=(64, 80), out_swap_rb=1)
            same(cv.result()[0], cv.view()[0], *want)


def test_device_cloud_view_class(gpu):
    """run(), a fixed camera from host rows and from the previous call's device rows, and the lifetime errors."""
    h, w = 37, 53
    depth = np.stack([scene(h, w)[0], scene(h, w, seed=5)[0]])
    d_depth = torch.from_numpy(depth).cuda()
    d_f = torch.tensor([47.5, 61.125], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pc.DeviceCloudView(2, h, w, (7, 9), colour=False, step=2) as cv:
        got = cv.run(d_depth.data_ptr(), 0, d_f_px=d_f.data_ptr(), elev_deg=30.0, azim_deg=-50.0)
        rows = cv.view().copy()
        for b, f in enumerate((47.5, 61.125)):
            same(got[b], rows[b], *expect(depth[b], f=f, step=2, size=(7, 9), angles=(30.0, -50.0)))
        # image 1 on image 0's camera, given from the host; then both kept from the device rows
        got = cv.run(d_depth.data_ptr(), 0, d_f_px=d_f.data_ptr(), view=rows[0]).copy()
        same(got[1], cv.view()[1], *expect(depth[1], f=61.125, step=2, size=(7, 9), view=rows[0]))
        again = cv.run(d_depth.data_ptr(), 0, d_f_px=d_f.data_ptr(), d_view=cv.views.device)
        assert again.tobytes() == got.tobytes()
        with pytest.raises(ValueError):
            cv.enqueue(d_depth.data_ptr(), 0, d_photo=d_depth.data_ptr(), fx=1.0)  # built without colour
        with pytest.raises(ValueError):
            cv.enqueue(d_depth.data_ptr(), 0)  # no focal length
        with pytest.raises(ValueError):
            cv.enqueue(d_depth.data_ptr(), 0, fx=1.0, view=rows, d_view=cv.views.device)
    for call in (cv.result, cv.view, lambda: cv.download(0), lambda: cv.enqueue(d_depth.data_ptr(), 0, fx=1.0)):
        with pytest.raises(RuntimeError, match="freed"):
            call()
    cv.free()  # twice is fine
    with pytest.raises(ValueError):
        pc.DeviceCloudView(1, h, w, (0, 9))


def test_bad_arguments_are_refused_before_any_device_call(gpu):
    h, w, size = 9, 5, (7, 9)
    z, _ = cases.degenerate("constant")
    d_depth = torch.from_numpy(np.array(z)).cuda()
    d_photo = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
    need = pc.cloud_view_ws_bytes(1, h, w, 1, *size)
    d_out, d_view, d_ws = guarded(size[0] * size[1] * 3), guarded(64), guarded(need)
    torch.cuda.synchronize()
    good = dict(d_depth=d_depth.data_ptr(), batch=1, h=h, w=w, step=1, d_photo=d_photo.data_ptr(), pitch=3 * w,
                swap_rb=False, d_f_px=0, fx=4.0, fy=4.0, cx=2.5, cy=4.5, trig=pc.view_trig(0.0, 0.0), d_view_in=0,
                bg=pc.VIEW_BG, out_swap_rb=False, d_out=d_out.data_ptr() + PAD, out_h=size[0], out_w=size[1],
                d_view_out=d_view.data_ptr() + PAD, d_ws=d_ws.data_ptr() + PAD, ws_nbytes=need,
                stream=torch.cuda.current_stream().cuda_stream)
    nan, inf = float("nan"), float("inf")
    bad = [dict(d_depth=0), dict(d_out=0), dict(d_view_out=0), dict(batch=0), dict(h=0), dict(w=-1), dict(step=0),
           dict(batch=65536), dict(batch=21846), dict(pitch=3 * w - 1), dict(fx=0.0), dict(fy=-1.0), dict(fx=nan),
           dict(cx=nan), dict(cy=nan), dict(out_h=0), dict(out_w=-3), dict(out_h=46341, out_w=46341),
           dict(h=32768, w=32768, step=1), dict(trig=(nan, 0.0, 1.0, 0.0)), dict(trig=(1.0, inf, 1.0, 0.0)),
           dict(trig=(1.0, 0.0, nan, 0.0)), dict(trig=(1.0, 0.0, 1.0, -inf)), dict(bg=(0, 256, 0)),
           dict(bg=(-1, 0, 0)), dict(d_ws=0), dict(ws_nbytes=need - 1), dict(d_ws=d_ws.data_ptr() + PAD + 4),
           dict(d_view_out=d_view.data_ptr() + PAD + 4), dict(d_view_in=d_view.data_ptr() + PAD + 4)]
    for change in bad:
        with pytest.raises(_lib.MDEError, match="MDE_ERR_ARG") as e:
            pc.cloud_view(**{**good, **change})
        assert "mde_op_cloud_view: " in str(e.value), change
    torch.cuda.synchronize()
    for t in (d_out, d_view, d_ws):
        assert (t.cpu().numpy() == FILL).all(), "a refused call wrote to the device"
    for args in ((0, h, w, 1, 7, 9), (1, h, w, 0, 7, 9), (1, h, w, 1, 0, 9), (1, 32768, 32768, 1, 7, 9),
                 (21846, h, w, 1, 7, 9), (1, h, w, 1, 46341, 46341)):
        assert pc.cloud_view_ws_bytes(*args) == 0, args
    pc.cloud_view(**good)  # and the unchanged arguments are taken
    torch.cuda.synchronize()
    pic = body(d_out, size[0] * size[1] * 3, "picture").reshape(*size, 3)
    want, _ = pc.render_np(z, 4.0, 4.0, 2.5, 4.5, size=size, elev_deg=0.0, azim_deg=0.0, photo=np.zeros((h, w, 3), np.uint8))
    assert np.array_equal(pic, want)


def dp_args(td, image):
    return ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(td / "e_fp16.mdeng"), "--iterations", "2",
            "--warmup", "1", "--image", str(image), "--out-dir", str(td / "bench")]


def driver_picture(depth, f, bgr, size=pc.VIEW_SIZE, angles=pc.VIEW_ANGLES, step=1, view=None):
    """What a driver's --cloud-view must have written: BGR, colours from the BGR photo."""
    h, w = depth.shape
    pic, row = pc.render_np(depth, f, f, w / 2, h / 2, size=size, elev_deg=angles[0], azim_deg=angles[1], photo=bgr,
                            swap_rb=True, step=step, view=view)
    return pic[..., ::-1], row


def test_depth_pro_driver_cloud_view(gpu, tmp_path, capsys):
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    bgr = cases.colours(60, 80)
    np.save(tmp_path / "src.npy", bgr)
    depth, f_px = run.main(dp_args(tmp_path, tmp_path / "src.npy") + ["--cloud-view", str(tmp_path / "v.npy")])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("[MDET] cloud view (device, ")]
    want, row = driver_picture(depth, np.float32(f_px), bgr)
    assert len(lines) == 1 and f"{int(row[0])} valid points, {int(row[6])} inside the picture" in lines[0], out
    got = np.load(tmp_path / "v.npy")
    assert got.shape == (320, 420, 3) and got.tobytes() == want.tobytes()
    depth2, _ = run.main(dp_args(tmp_path, tmp_path / "src.npy") + [
        "--cloud-view", str(tmp_path / "s.npy"), "--cloud-view-size", "48", "64", "--cloud-view-angles", "30", "-50",
        "--cloud-view-step", "2", "--f-px", "70"])
    assert np.array_equal(depth2.shape, depth.shape)
    want, _ = driver_picture(depth2, 70.0, bgr, size=(48, 64), angles=(30.0, -50.0), step=2)
    assert np.load(tmp_path / "s.npy").tobytes() == want.tobytes()
    with pytest.raises(SystemExit, match="host-postprocess"):
        run.main(dp_args(tmp_path, tmp_path / "src.npy") + ["--cloud-view", str(tmp_path / "n.npy"),
                                                            "--host-postprocess"])
    with pytest.raises(SystemExit, match="cloud-view-size"):
        run.main(dp_args(tmp_path, tmp_path / "src.npy") + ["--cloud-view", str(tmp_path / "n.npy"),
                                                            "--cloud-view-size", "0", "4"])
    assert not (tmp_path / "n.npy").exists()


def test_dav2_driver_cloud_view(gpu, tmp_path, capsys):
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    bgr = cases.colours(60, 80)
    np.save(tmp_path / "src.npy", bgr)
    args = ["--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2", "--warmup", "1", "--image",
            str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench")]
    depth = run.main(args + ["--source", "synthetic:vits:metric:1234", "--f-px", "70", "--cloud-view",
                             str(tmp_path / "m.npy"), "--cloud-view-size", "48", "64"])
    out = capsys.readouterr().out
    assert sum(l.startswith("[MDET] cloud view (device, ") for l in out.splitlines()) == 1, out
    want, row = driver_picture(depth, 70.0, bgr, size=(48, 64))
    assert np.load(tmp_path / "m.npy").tobytes() == want.tobytes() and row[pc.V_NVALID] == 60 * 80
    with pytest.raises(SystemExit, match="--cloud-view needs --f-px"):
        run.main(args + ["--source", "synthetic:vits:metric:1234", "--cloud-view", str(tmp_path / "n.npy")])
    with pytest.raises(SystemExit) as e:
        run.main(args + ["--source", "synthetic:vits:relative:1234", "--f-px", "70", "--cloud-view",
                         str(tmp_path / "r.npy")])
    assert "metric" in str(e.value) and not (tmp_path / "r.npy").exists() and not (tmp_path / "n.npy").exists()


def test_depth_pro_stream_cloud_view_out(gpu, tmp_path, capsys):
    """One preview per frame; frame 0 is run.py --cloud-view's picture, frame 1 is drawn with frame 0's camera."""
    from monocular_depth_estimation_trt_amd.models.depth_pro import run, stream as dp_stream
    frames = np.stack([cases.colours(37, 53), cases.colours(37, 53, seed=8)])
    np.save(tmp_path / "frames.npy", frames)
    maps = []
    for t in range(2):
        np.save(tmp_path / f"f{t}.npy", frames[t])
        maps.append(run.main(dp_args(tmp_path, tmp_path / f"f{t}.npy")))
    capsys.readouterr()
    engine = ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(tmp_path / "e_fp16.mdeng")]
    colour = dp_stream.main(engine + ["--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "out.npy"),
                                      "--cloud-view-out", str(tmp_path / "views.npy"), "--cloud-view-size", "41", "41"])
    out = capsys.readouterr().out
    assert sum(l.startswith("[MDET] cloud view (device; 2 previews") for l in out.splitlines()) == 1, out
    views = np.load(tmp_path / "views.npy")
    assert views.shape == (2, 41, 41, 3) and colour.shape == (2, 37, 53, 3)
    want0, row0 = driver_picture(maps[0][0], np.float32(maps[0][1]), frames[0], size=(41, 41))
    want1, row1 = driver_picture(maps[1][0], np.float32(maps[1][1]), frames[1], size=(41, 41), view=row0)
    assert views[0].tobytes() == want0.tobytes() and views[1].tobytes() == want1.tobytes()
    assert row1[1:6].tolist() == row0[1:6].tolist()
    plain = dp_stream.main(engine + ["--frames", str(tmp_path / "frames.npy"), "--out", str(tmp_path / "out2.npy")])
    assert plain.tobytes() == colour.tobytes()  # the previews change nothing else
