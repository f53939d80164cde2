"""Meshes on the device (csrc/depth_mesh.hip) through the C ABI, the Python owner (pointcloud.DeviceMesh)
and the two drivers' --mesh and --ply-edge-rtol.

Every comparison is bit-exact: the vertex and face record bytes the device wrote, as uint8, against the
bytes of pointcloud.mesh_np (held to the max-filter statement of the edge rule and to a per-sample loop in
tests/test_mesh_cpu.py).  Every call writes into buffers filled with 0xA5 and the helper checks that nothing
but the counted records of each image's two regions changed: the bytes before the base pointers, the bytes
of a region past its count, the bytes after the last region, and the scratch past ws_bytes.

Sizes, for the shapes of mesh_cases.SHAPES: the mark kernel works on 2D tiles of 16 x 64 samples with a
two-sample halo; counts, scan and the two write kernels on tiles of 1024 consecutive samples, the scan with
one workgroup of 256 threads per image.  9 x 5 is less than a wave and less than any tile; 37 x 53 is 3 x 1
mark tiles and 2 count tiles; 100 x 76 and 130 x 150 cross the mark tile on both axes (7 x 2 and 9 x 3 tiles);
600 x 800 is 469 count tiles, two rounds of the scan for vertices and for triangles.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_util import op, ptr, stream
from mesh_cases import RTOL, SHAPES, Z_HI, Z_LO, camera, photo, scene, steps_of

from monocular_depth_estimation_trt_amd import _lib
from monocular_depth_estimation_trt_amd import pointcloud as pc

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64  # guard bytes before the base pointers and after the last regions
CASES = [(s, k) for s in SHAPES for k in steps_of(s)]
case_id = lambda c: "%dx%d-step%d" % (*c[0], c[1])  # noqa: E731
# colour, padded pitch, swap_rb, faces, rtol, atol: every value of each, not their product
OPTIONS = [(True, 5, 1, 1, RTOL, 0.0), (False, 0, 0, 0, 0.0, 0.3), (True, 0, 0, 1, RTOL, 0.3),
           (True, 7, 1, 0, 0.0, 0.0), (False, 0, 0, 1, 0.0, 0.0), (True, 0, 0, 0, RTOL, 0.0)]
option_id = lambda o: "%s-pad%d-swap%d-faces%d-rtol%g-atol%g" % (("rgb" if o[0] else "xyz",) + o[1:])  # noqa: E731
PATTERNS = ["none", "patch", "last_block", "checker"]


def pattern_depth(name, h, w, step):
    """The scene with a validity pattern laid over its sampled grid (invalid = 0 unless said)."""
    z = np.array(scene(h, w, step))
    hs, ws = pc.grid(h, w, step)
    if name == "none":
        z[:] = 0.0
    elif name == "patch":  # NaN / +-inf / out-of-range, on sampled pixels
        i, j = (hs // 2) * step, (ws // 2) * step
        i1, j1 = min(i + step, (hs - 1) * step), min(j + step, (ws - 1) * step)
        z[i, j] = z[i - step, j] = z[i, j - step] = np.nan
        z[i1, j], z[i1, j - step] = np.inf, -np.inf
        z[i - step, j - step], z[i - step, j1] = Z_HI * np.float32(1.5), Z_LO * np.float32(0.5)
        z[(hs - 1) * step, (ws - 1) * step] = np.nan
        z[0, 0] = -1.0
    elif name == "last_block":  # the last 2 x 2 samples, made flat so that they are a quad
        keep = np.zeros((h, w), bool)
        keep[(hs - 2) * step::step, (ws - 2) * step::step] = True
        z[keep] = 2.5
        z[~keep] = 0.0
    elif name == "checker":
        ii, jj = np.mgrid[0:h, 0:w] // step
        z[(ii + jj) % 2 == 1] = np.nan
    else:
        assert name == "scene"
    return z


def device_mesh(depth, img=None, pad=0, swap_rb=0, step=1, f_dev=None, cam=None, faces=1, rtol=RTOL, atol=0.0,
                v_offset=0, f_offset=0, z_lo=Z_LO, z_hi=Z_HI):
    """Run mde_op_depth_mesh on depth [B][h][w] (and img [B][h][w][3], rows padded with `pad` bytes of 0xFF)
    with the vertex / face records at v_offset / f_offset bytes past a 16-byte boundary.  Checks the guards
    and returns (vertex counts, vertex regions, face counts, face regions); `f_dev`: per-image focal lengths
    instead of the camera's."""
    B, h, w = depth.shape
    hs, ws = pc.grid(h, w, step)
    rec = 15 if img is not None else 12
    region, fregion = hs * ws * rec, 2 * (hs - 1) * (ws - 1) * 13
    fx, fy, cx, cy = cam or camera(h, w)
    d_depth = torch.from_numpy(np.array(depth)).cuda()
    d_photo, pitch = None, 0
    if img is not None:
        pitch = 3 * w + pad
        rows = np.full((B, h, pitch), 0xFF, np.uint8)
        rows[:, :, :3 * w] = img.reshape(B, h, 3 * w)
        d_photo = torch.from_numpy(rows).cuda()
    d_f = None if f_dev is None else torch.from_numpy(np.asarray(f_dev, np.float32)).cuda()
    d_v = torch.full((PAD + v_offset + B * region + PAD,), FILL, dtype=torch.uint8, device="cuda")
    d_t = torch.full((PAD + f_offset + B * fregion + PAD,), FILL, dtype=torch.uint8, device="cuda")
    assert d_v.data_ptr() % 16 == 0 and d_t.data_ptr() % 16 == 0
    d_cnt = torch.full((2, B + 1), -7, dtype=torch.int32, device="cuda")
    need = pc.mesh_ws_bytes(B, h, w, step)
    assert need == B * (-(-hs * ws // 1024) * 8 + hs * ws * 5)
    d_ws = torch.full((need + 16,), FILL, dtype=torch.uint8, device="cuda")
    op("mde_op_depth_mesh", ptr(d_depth), B, h, w, step, ptr(d_photo), pitch, swap_rb, ptr(d_f),
       -1.0 if f_dev is not None else float(fx), -1.0 if f_dev is not None else float(fy), float(cx), float(cy),
       float(z_lo), float(z_hi), float(rtol), float(atol), faces, C.c_void_p(d_v.data_ptr() + PAD + v_offset),
       B * region, ptr(d_cnt), C.c_void_p(d_t.data_ptr() + PAD + f_offset) if faces else None,
       B * fregion if faces else 0, C.c_void_p(d_cnt.data_ptr() + 4 * (B + 1)) if faces else None, ptr(d_ws), need,
       stream())
    v, t, cnt, wsb = d_v.cpu().numpy(), d_t.cpu().numpy(), d_cnt.cpu().numpy(), d_ws.cpu().numpy()
    assert cnt[0, B] == -7 and cnt[1, B] == -7
    assert (wsb[need:] == FILL).all(), "scratch written past mde_op_depth_mesh_ws_bytes"
    if not faces:
        assert (cnt[1] == -7).all() and (t == FILL).all(), "faces == 0 wrote a face or a face count"
        cnt[1, :B] = 0
    out = []
    for buf, off, size, item, n, what in ((v, v_offset, region, rec, cnt[0], "vertex"),
                                          (t, f_offset, fregion, 13, cnt[1], "face")):
        assert (buf[:PAD + off] == FILL).all(), f"bytes before the {what} base pointer written"
        assert (buf[PAD + off + B * size:] == FILL).all(), f"bytes after the last {what} region written"
        body = buf[PAD + off:PAD + off + B * size]
        regions = [body[b * size:(b + 1) * size] for b in range(B)]
        for b in range(B):
            assert 0 <= n[b] * item <= size, (what, n)
            assert (regions[b][int(n[b]) * item:] == FILL).all(), f"image {b}: {what} bytes past the count written"
        out += [n[:B], regions]
    return out


@functools.lru_cache(maxsize=None)
def expect(shape, step, pattern="scene", colour=True, swap_rb=0, faces=1, rtol=RTOL, atol=0.0, f=None, b=0, batch=1):
    """mesh_np of one case; computed once and shared (keyed by the case, never written)."""
    h, w = shape
    fx, fy, cx, cy = camera(h, w)
    if f is not None:
        fx = fy = f
    return pc.mesh_np(pattern_depth(pattern, h, w, step), fx, fy, cx, cy, photo=photo(h, w, batch)[b] if colour else None,
                      swap_rb=bool(swap_rb), step=step, z_lo=Z_LO, z_hi=Z_HI, edge_rtol=rtol, edge_atol=atol,
                      faces=bool(faces))


def same_bytes(region, want, count, what):
    """The first `count` records of the region against the restatement's bytes."""
    assert int(count) == want.shape[0], (what, int(count), want.shape[0])
    got = region[:want.nbytes]
    ref = np.frombuffer(want.tobytes(), np.uint8)
    bad = got != ref
    assert not bad.any(), (what, int(bad.sum()), (np.flatnonzero(bad)[:6] // want.dtype.itemsize).tolist())


def same_mesh(got, want, b=0):
    nv, vr, nt, tr = got
    same_bytes(vr[b], want[0], nv[b], "vertices")
    same_bytes(tr[b], want[1], nt[b], "faces")


@pytest.mark.parametrize("option", OPTIONS, ids=option_id)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scene_bit_exact(gpu, case, option):
    (h, w), step = case
    colour, pad, swap, faces, rtol, atol = option
    z = pattern_depth("scene", h, w, step)[None]
    got = device_mesh(z, photo(h, w) if colour else None, pad=pad, swap_rb=swap, step=step, faces=faces, rtol=rtol,
                      atol=atol)
    want = expect((h, w), step, "scene", colour, swap, faces, rtol, atol)
    same_mesh(got, want)
    if (h, w) != (9, 5):
        clean = int(((want[2] & pc.F_CLEAN) != 0).sum())
        assert 0 < got[0][0] <= clean and (got[2][0] > 0) == bool(faces)
        if (rtol, atol) == (RTOL, 0.0):  # with faces some clean sample is no vertex; without, every one is
            assert (got[0][0] < clean) == bool(faces)


@pytest.mark.parametrize("faces", [1, 0], ids=["faces", "cloud"])
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_validity_patterns(gpu, case, name, faces):
    (h, w), step = case
    z = pattern_depth(name, h, w, step)[None]
    got = device_mesh(z, photo(h, w), step=step, faces=faces)
    nv, vr, nt, tr = got
    want = expect((h, w), step, name, True, 0, faces)
    same_mesh(got, want)
    hs, ws = pc.grid(h, w, step)
    if name == "none":
        assert nv[0] == 0 and nt[0] == 0 and (vr[0] == FILL).all() and (tr[0] == FILL).all()  # not one byte
    elif name == "last_block":
        assert (nv[0], nt[0]) == ((4, 2) if faces else (4, 0))
        if faces:
            assert want[1]["i0"].tolist() in ([0, 0], [0, 1]) and want[1].tobytes() == tr[0][:26].tobytes()
    elif name == "checker":  # no 2 x 2 block is whole: no quad, so no vertex with faces
        assert nt[0] == 0 and (nv[0] == 0 if faces else 0 < nv[0] <= (hs * ws + 1) // 2)
    else:  # on 9 x 5 the patch leaves no whole block at steps 2 and 3
        assert nv[0] < hs * ws and (nv[0] > 0 or (h, w) == (9, 5))


@pytest.mark.parametrize("faces", [1, 0], ids=["faces", "cloud"])
@pytest.mark.parametrize("colour", [True, False], ids=["rgb", "xyz"])
def test_batch2_device_focal_lengths(gpu, colour, faces):
    """Two images, different validity and different device focal lengths; image 1's vertex region starts at
    byte hs * ws * rec (odd with 15-byte records) and its face region at byte 2 * 36 * 52 * 13."""
    h, w = 37, 53
    z = np.stack([pattern_depth("scene", h, w, 1), pattern_depth("patch", h, w, 1)])
    f = (61.5, 47.125)
    got = device_mesh(z, photo(h, w, 2) if colour else None, f_dev=np.array(f, np.float32), faces=faces)
    for b, name in enumerate(("scene", "patch")):
        same_mesh(got, expect((h, w), 1, name, colour, 0, faces, f=f[b], b=b, batch=2), b)
    assert got[0][0] != got[0][1] and (not faces or got[2][0] != got[2][1])


@pytest.mark.parametrize("offsets", [(0, 0), (1, 3), (2, 1), (3, 2)], ids=lambda o: "v%d-f%d" % o)
def test_unaligned_bases_and_guards(gpu, offsets):
    """Vertex and face base pointers 0..3 bytes past a 16-byte boundary, two images (device_mesh holds every
    byte outside the counted records to the 0xA5 fill)."""
    h, w = 37, 53
    z = np.stack([pattern_depth("patch", h, w, 2), pattern_depth("last_block", h, w, 2)])
    got = device_mesh(z, photo(h, w, 2), step=2, swap_rb=1, v_offset=offsets[0], f_offset=offsets[1])
    for b, name in enumerate(("patch", "last_block")):
        same_mesh(got, expect((h, w), 2, name, True, 1, 1, b=b, batch=2), b)


@pytest.mark.parametrize("faces", [1, 0], ids=["faces", "cloud"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (5, 4)], ids=lambda s: "%dx%d" % s)
def test_a_grid_without_quads(gpu, shape, faces):
    """hs < 2 or ws < 2 (5 x 4 at step 4 is 2 x 1): legal, an empty face region, no vertex with faces."""
    h, w = shape
    step = 4 if shape == (5, 4) else 1
    z = np.full((1, h, w), 2.5, np.float32)
    nv, vr, nt, tr = device_mesh(z, photo(h, w), step=step, faces=faces)
    hs, ws = pc.grid(h, w, step)
    assert min(hs, ws) == 1 and tr[0].size == 0 and nt[0] == 0
    want = pc.mesh_np(z[0], *camera(h, w), photo=photo(h, w)[0], step=step, z_lo=Z_LO, z_hi=Z_HI, faces=bool(faces))
    assert want[0].shape[0] == (0 if faces else hs * ws)
    same_bytes(vr[0], want[0], nv[0], "vertices")


def test_deterministic(gpu):
    h, w = 600, 800
    z = pattern_depth("patch", h, w, 1)[None]
    a, b = device_mesh(z, photo(h, w)), device_mesh(z, photo(h, w))
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0])
    same_mesh(a, expect((h, w), 1, "patch"))


def test_device_mesh_in_a_captured_graph(gpu):
    """One DeviceMesh.enqueue (six kernels) captured into a torch.cuda.graph on a side stream, replayed
    twice with the depth changed in between."""
    h, w = 100, 76
    img = photo(h, w)[0]
    names = ("scene", "patch")
    d_depth = torch.from_numpy(pattern_depth(names[0], h, w, 1)).cuda()
    d_photo = torch.from_numpy(np.array(img)).cuda()
    fx, fy, cx, cy = camera(h, w)
    with pc.DeviceMesh(1, h, w, colour=True) as mesh:
        kw = dict(d_photo=d_photo.data_ptr(), pitch=3 * w, swap_rb=True, fx=fx, fy=fy, cx=cx, cy=cy, z_lo=Z_LO,
                  z_hi=Z_HI, edge_rtol=RTOL)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            mesh.enqueue(d_depth.data_ptr(), s.cuda_stream, **kw)  # warm: the kernels are loaded
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            mesh.enqueue(d_depth.data_ptr(), s.cuda_stream, **kw)
        for name in reversed(names):
            d_depth.copy_(torch.from_numpy(pattern_depth(name, h, w, 1)))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            mesh.download(0)
            v, t = mesh.result()[0]
            want = expect((h, w), 1, name, True, 1, 1)
            assert v.dtype == pc.vertex_dtype(True) and t.dtype == pc.FACE_DTYPE
            assert v.tobytes() == want[0].tobytes() and t.tobytes() == want[1].tobytes() and t.shape[0] > 0
    with pytest.raises(RuntimeError):
        mesh.result()  # freed


def test_device_mesh_run_batch2_and_cloud(gpu):
    """run() = enqueue, both counts, the counted bytes: per-image views, with faces and without."""
    h, w = 37, 53
    names = ("scene", "last_block")
    z = np.stack([pattern_depth(n, h, w, 2) for n in names])
    d_depth = torch.from_numpy(z).cuda()
    f = (61.5, 47.125)
    d_f = torch.tensor(f, dtype=torch.float32, device="cuda")
    fx, fy, cx, cy = camera(h, w)
    torch.cuda.synchronize()
    for faces in (True, False):
        with pc.DeviceMesh(2, h, w, colour=False, step=2, faces=faces) as mesh:
            got = mesh.run(d_depth.data_ptr(), 0, d_f_px=d_f.data_ptr(), cx=cx, cy=cy, z_lo=Z_LO, z_hi=Z_HI)
            for b, name in enumerate(names):
                want = expect((h, w), 2, name, False, 0, int(faces), f=f[b])
                assert got[b][0].tobytes() == want[0].tobytes() and got[b][1].tobytes() == want[1].tobytes(), (faces, b)
            with pytest.raises(ValueError):
                mesh.enqueue(d_depth.data_ptr(), 0, d_photo=d_depth.data_ptr(), fx=1.0)  # built without colour
            with pytest.raises(ValueError):
                mesh.enqueue(d_depth.data_ptr(), 0)  # no focal length
    with pytest.raises(_lib.MDEError):
        pc.depth_mesh(d_depth.data_ptr(), 1, h, w, 1, 0, 0, False, 0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, -0.1, 0.0, False,
                      d_depth.data_ptr(), 1 << 20, d_f.data_ptr(), 0, 0, 0, d_depth.data_ptr(), 1 << 20)


def check_driver_mesh(path, depth, f_px, bgr, step, z_lo, z_hi, rtol, atol=0.0):
    v, t = pc.read_ply_mesh(path)
    want = pc.mesh_np(depth, f_px, f_px, depth.shape[1] / 2, depth.shape[0] / 2, photo=bgr, swap_rb=True, step=step,
                      z_lo=z_lo, z_hi=z_hi, edge_rtol=rtol, edge_atol=atol)
    assert v.dtype == pc.vertex_dtype(True)
    assert v.tobytes() == want[0].tobytes() and t.tobytes() == want[1].tobytes()
    return v, t, want[2]


def check_driver_cloud(path, depth, f_px, bgr, step, z_lo, z_hi, rtol):
    cloud = pc.read_ply(path)
    want = pc.mesh_np(depth, f_px, f_px, depth.shape[1] / 2, depth.shape[0] / 2, photo=bgr, swap_rb=True, step=step,
                      z_lo=z_lo, z_hi=z_hi, edge_rtol=rtol, faces=False)[0]
    assert cloud.dtype == pc.vertex_dtype(True) and cloud.tobytes() == want.tobytes()
    return cloud


def spread_quantile(depth, step, q):
    """The q-quantile, as a float32, of the 3 x 3 relative depth spread over the sampled grid: a tolerance
    that makes about 1 - q of this map's samples edges, whatever the synthetic weights made of it."""
    z = np.asarray(depth, np.float32)[::step, ::step]
    ratio = (pc._max3x3(z) + pc._max3x3(-z)) / z
    return np.float32(np.quantile(ratio, q))


def mixed(flags, t):
    """Neither everything nor nothing is an edge, and some quad survived."""
    edge = (flags & pc.F_EDGE) != 0
    print("edge share", float(edge.mean()), "triangles", t.shape[0])
    return 0 < edge.sum() < edge.size and t.shape[0] > 0


def test_depth_pro_driver_mesh_and_filtered_ply(gpu, tmp_path, capsys):
    """--mesh and --ply --ply-edge-rtol in one run, with the focal length the device post-process left.  A
    first run without either gives the map, from which the tolerances are chosen."""
    from monocular_depth_estimation_trt_amd.models.depth_pro import run
    bgr = photo(300, 400)[0]
    np.save(tmp_path / "src.npy", bgr)
    args = ["--source", "synthetic:depth_pro:tiny:4321", "--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations",
            "2", "--warmup", "1", "--image", str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench")]
    depth, f_px = run.main(args)
    rtol, ply_rtol = spread_quantile(depth, 2, 0.7), spread_quantile(depth, 1, 0.5)
    capsys.readouterr()
    depth2, f2 = run.main(args + ["--mesh", str(tmp_path / "m.ply"), "--mesh-step", "2", "--edge-rtol",
                                  repr(float(rtol)), "--ply", str(tmp_path / "c.ply"), "--ply-edge-rtol",
                                  repr(float(ply_rtol))])
    out = capsys.readouterr().out
    assert np.array_equal(depth2, depth) and f2 == f_px
    assert f"[MDET] mesh (device, kernels + D2H, hipEvents) 300x400 step 2 rtol {float(rtol):g} atol 0" in out
    assert "[MDET] point cloud (device, kernels + D2H, hipEvents)" in out
    v, t, flags = check_driver_mesh(tmp_path / "m.ply", depth, np.float32(f_px), bgr, 2, 1e-4, 1e4, rtol)
    assert f"{v.shape[0]} vertices, {t.shape[0]} triangles" in out
    assert mixed(flags, t)
    cloud = check_driver_cloud(tmp_path / "c.ply", depth, np.float32(f_px), bgr, 1, 1e-4, 1e4, ply_rtol)
    assert 0 < cloud.shape[0] < 300 * 400 and f"{cloud.shape[0]} points" in out


def test_dav2_driver_mesh_and_filtered_ply(gpu, tmp_path, capsys):
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run
    bgr = photo(300, 400)[0]
    np.save(tmp_path / "src.npy", bgr)
    args = ["--source", "synthetic:vits:metric:1234", "--engine", str(tmp_path / "e_fp16.mdeng"), "--iterations", "2",
            "--warmup", "1", "--image", str(tmp_path / "src.npy"), "--out-dir", str(tmp_path / "bench"), "--f-px", "500"]
    depth = run.main(args)
    rtol, ply_rtol = spread_quantile(depth, 1, 0.7), spread_quantile(depth, 3, 0.5)
    capsys.readouterr()
    depth2 = run.main(args + ["--mesh", str(tmp_path / "m.ply"), "--edge-rtol", repr(float(rtol)), "--edge-atol", "100",
                              "--ply", str(tmp_path / "c.ply"), "--ply-step", "3", "--ply-edge-rtol",
                              repr(float(ply_rtol))])
    out = capsys.readouterr().out
    assert np.array_equal(depth2, depth)
    assert f"[MDET] mesh (device, kernels + D2H, hipEvents) 300x400 step 1 rtol {float(rtol):g} atol 100" in out
    v, t, flags = check_driver_mesh(tmp_path / "m.ply", depth, 500.0, bgr, 1, 1e-3, 1e3, rtol, 100.0)
    assert f"{v.shape[0]} vertices, {t.shape[0]} triangles" in out
    assert mixed(flags, t)
    cloud = check_driver_cloud(tmp_path / "c.ply", depth, 500.0, bgr, 3, 1e-3, 1e3, ply_rtol)
    assert 0 < cloud.shape[0] < 100 * 134 and f"{cloud.shape[0]} points" in out
