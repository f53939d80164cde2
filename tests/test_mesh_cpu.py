"""Meshes without a GPU: pointcloud.mesh_np, the numpy restatement of the mde_op_depth_mesh contract
(include/mde.h), the PLY mesh files, the ABI's argument checks and the drivers' flags.

`utils3d` (the reference's depth_map_edge and build_mesh_from_map, models/metric_anything/
demo_pointcloud.py:142-149) is not a file of the reference, so the edge rule is pinned against its
max-filter statement written with scipy.ndimage, and the whole of mesh_np against a per-sample Python loop
written from the contract's text.
"""

import ctypes
import os

import numpy as np
import pytest

from mesh_cases import RTOL, Z_HI, Z_LO, camera, photo, scene

from monocular_depth_estimation_trt_amd import _lib, pointcloud as pc

f32 = np.float32


def with_bad_patch(z):
    """A copy with a NaN / +-inf / out-of-range patch in the middle and one in a corner."""
    z = np.array(z)
    h, w = z.shape
    i, j = h // 2, w // 2
    z[i - 2:i + 1, j - 1:j + 1] = np.nan
    z[i + 1, j - 1], z[i + 1, j] = np.inf, -np.inf
    z[max(i - 3, 0), j - 1], z[max(i - 3, 0), j] = Z_HI * f32(1.5), Z_LO * f32(0.5)
    z[h - 1, w - 1] = np.nan
    z[0, 0] = 0.0
    return z


# ---- the edge rule -------------------------------------------------------------------------------------

@pytest.mark.parametrize("tol", [(0.1, 0.0), (0.0, 0.3), (0.1, 0.3), (0.0, 0.0), (0.05, 0.0)],
                         ids=lambda t: "rtol%g-atol%g" % t)
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("shape", [(9, 5), (37, 53), (100, 76)], ids=lambda s: "%dx%d" % s)
def test_edge_flags_equal_the_max_filter_statement(shape, step, tol):
    from scipy import ndimage
    rtol, atol = f32(tol[0]), f32(tol[1])
    z = with_bad_patch(scene(*shape, step))
    flags = pc.mesh_np(z, *camera(*shape), step=step, z_lo=Z_LO, z_hi=Z_HI, edge_rtol=rtol, edge_atol=atol)[2]
    zs = z[::step, ::step]
    with np.errstate(all="ignore"):
        valid = (zs == zs) & (zs >= Z_LO) & (zs <= Z_HI)
        ninf = f32(-np.inf)
        diff = (ndimage.maximum_filter(np.where(valid, zs, ninf), 3, mode="constant", cval=-np.inf)
                + ndimage.maximum_filter(np.where(valid, -zs, ninf), 3, mode="constant", cval=-np.inf))
        assert diff.dtype == np.float32
        ratio = diff / zs
        edge = valid & (((atol > 0) & (diff > atol)) | ((rtol > 0) & (ratio > rtol)))
    assert np.array_equal((flags & pc.F_VALID) != 0, valid)
    assert np.array_equal((flags & pc.F_EDGE) != 0, edge)
    assert np.array_equal((flags & pc.F_CLEAN) != 0, valid & ~edge)
    assert valid.sum() < valid.size
    if tol == (0.0, 0.0):
        assert not edge.any()
    elif shape != (9, 5):
        assert 0 < edge.sum() < valid.sum()


def test_threshold_ties_are_not_edges():
    """rtol = 0.125, a power of two: 0.125 / 1.0 is exact.  A neighbour at exactly 1.125 leaves the
    centre at the threshold -- no edge; one ulp more makes it one.  The same with atol."""
    z = np.ones((5, 5), f32)
    z[2, 3] = f32(1.125)
    kw = dict(z_lo=0.5, z_hi=10.0, faces=False)
    flags = pc.mesh_np(z, 5, 5, 2, 2, edge_rtol=0.125, **kw)[2]
    # the neighbour itself: diff / 1.125 < 0.125
    assert not (flags & pc.F_EDGE).any() and ((flags & pc.F_CLEAN) != 0).all()
    assert not (pc.mesh_np(z, 5, 5, 2, 2, edge_rtol=0.0, edge_atol=0.125, **kw)[2] & pc.F_EDGE).any()
    z[2, 3] = np.nextafter(f32(1.125), f32(2))
    for tol in (dict(edge_rtol=0.125), dict(edge_rtol=0.0, edge_atol=0.125)):
        edge = (pc.mesh_np(z, 5, 5, 2, 2, **tol, **kw)[2] & pc.F_EDGE) != 0
        want = np.zeros((5, 5), bool)
        want[1:4, 2:5] = True  # the 3 x 3 windows that hold (2, 3)
        if "edge_atol" not in tol:
            want[2, 3] = False  # (1.125 + ulp - 1) / (1.125 + ulp) < 0.125
        assert np.array_equal(edge, want), tol


# ---- the whole contract, sample by sample --------------------------------------------------------------

def brute_mesh(depth, fx, fy, cx, cy, img, swap_rb, step, z_lo, z_hi, rtol, atol, faces):
    """mde_op_depth_mesh's contract (include/mde.h) as loops over samples, np.float32 scalars throughout."""
    h, w = depth.shape
    hs, ws = -(-h // step), -(-w // step)
    fx, fy, cx, cy, z_lo, z_hi, rtol, atol = (f32(t) for t in (fx, fy, cx, cy, z_lo, z_hi, rtol, atol))
    z = [[f32(depth[i * step, j * step]) for j in range(ws)] for i in range(hs)]
    valid = [[bool(z[i][j] == z[i][j] and z[i][j] >= z_lo and z[i][j] <= z_hi) for j in range(ws)] for i in range(hs)]
    clean = [[False] * ws for _ in range(hs)]
    with np.errstate(all="ignore"):
        for i in range(hs):
            for j in range(ws):
                if not valid[i][j]:
                    continue
                near = [z[a][b] for a in range(max(i - 1, 0), min(i + 2, hs)) for b in range(max(j - 1, 0), min(j + 2, ws))
                        if valid[a][b]]
                diff = f32(max(near) - min(near))
                edge = bool((atol > 0 and diff > atol) or (rtol > 0 and f32(diff / z[i][j]) > rtol))
                clean[i][j] = not edge
        kept = [[i < hs - 1 and j < ws - 1 and clean[i][j] and clean[i][j + 1] and clean[i + 1][j + 1] and clean[i + 1][j]
                 for j in range(ws)] for i in range(hs)]
        vertex, index, n = [[False] * ws for _ in range(hs)], {}, 0
        body = bytearray()
        for i in range(hs):
            for j in range(ws):
                if faces:
                    vertex[i][j] = any(kept[a][b] for a in (i - 1, i) for b in (j - 1, j) if a >= 0 and b >= 0)
                else:
                    vertex[i][j] = clean[i][j]
                if not vertex[i][j]:
                    continue
                index[i, j], n = n, n + 1
                u, v = j * step, i * step
                xn, yn = f32(f32(f32(u) - cx) / fx), f32(f32(f32(v) - cy) / fy)
                body += np.array([xn * z[i][j], yn * z[i][j], z[i][j]], "<f4").tobytes()
                if img is not None:
                    px = img[v, u]
                    body += bytes([px[2], px[1], px[0]] if swap_rb else [px[0], px[1], px[2]])
        tri = bytearray()
        for i in range(hs):
            for j in range(ws):
                if not (faces and kept[i][j]):
                    continue
                a, b, c, d = index[i, j], index[i, j + 1], index[i + 1, j + 1], index[i + 1, j]
                if abs(f32(z[i][j] - z[i + 1][j + 1])) <= abs(f32(z[i][j + 1] - z[i + 1][j])):
                    two = ((a, d, c), (a, c, b))
                else:
                    two = ((a, d, b), (b, d, c))
                for t in two:
                    tri += bytes([3]) + np.array(t, "<i4").tobytes()
    return bytes(body), bytes(tri), n


@pytest.mark.parametrize("faces", [True, False], ids=["faces", "cloud"])
@pytest.mark.parametrize("case", [((9, 5), 1, 0.1, 0.0), ((9, 5), 2, 0.0, 0.0), ((37, 53), 1, 0.1, 0.0),
                                  ((37, 53), 2, 0.1, 0.3), ((37, 53), 3, 0.0, 0.25)],
                         ids=lambda c: "%dx%d-step%d-rtol%g-atol%g" % (*c[0], *c[1:]))
def test_mesh_np_equals_the_per_sample_loop(case, faces):
    (h, w), step, rtol, atol = case
    z = with_bad_patch(scene(h, w, step))
    img = photo(h, w)[0]
    swap = bool(step % 2)
    v, t, _ = pc.mesh_np(z, *camera(h, w), photo=img, swap_rb=swap, step=step, z_lo=Z_LO, z_hi=Z_HI, edge_rtol=rtol,
                         edge_atol=atol, faces=faces)
    body, tri, n = brute_mesh(z, *camera(h, w), img, swap, step, Z_LO, Z_HI, rtol, atol, faces)
    assert v.dtype == pc.vertex_dtype(True) and t.dtype == pc.FACE_DTYPE and pc.FACE_DTYPE.itemsize == 13
    assert v.shape == (n,) and v.tobytes() == body
    assert t.tobytes() == tri
    assert n > 0 and (len(tri) > 0) == faces


# ---- properties of the mesh ----------------------------------------------------------------------------

@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("shape", [(37, 53), (100, 76), (130, 150)], ids=lambda s: "%dx%d" % s)
def test_mesh_properties(shape, step):
    h, w = shape
    z = with_bad_patch(scene(h, w, step))
    cam = camera(h, w)
    v, t, flags = pc.mesh_np(z, *cam, step=step, z_lo=Z_LO, z_hi=Z_HI, edge_rtol=RTOL)
    idx = np.stack([t["i0"], t["i1"], t["i2"]], axis=-1)
    assert (t["n"] == 3).all() and idx.min() >= 0 and idx.max() < v.shape[0]
    assert np.array_equal(np.unique(idx), np.arange(v.shape[0])), "an unreferenced vertex"
    assert t.shape[0] == 2 * int(((flags & pc.F_QUAD) != 0).sum()) > 0
    assert v.shape[0] == int(((flags & pc.F_VERTEX) != 0).sum())
    # no face touches a sample that is not clean: every vertex is one
    assert (flags[(flags & pc.F_VERTEX) != 0] & pc.F_CLEAN).all()
    assert (((flags & pc.F_CLEAN) != 0) & ((flags & pc.F_VERTEX) == 0)).any(), "no clean sample left out"
    both = (flags[(flags & pc.F_QUAD) != 0] & pc.F_DIAG_BD) != 0
    assert both.any() and not both.all(), "only one diagonal occurs"
    # the vertices are the organized cloud's records of the flagged samples
    cloud = pc.unproject_np(z, *cam, step=step)
    assert v.tobytes() == cloud[((flags & pc.F_VERTEX) != 0).reshape(-1)].tobytes()
    # every face faces the origin of the camera frame (X right, Y down, Z forward), in float64
    p = np.stack([v["x"], v["y"], v["z"]], axis=-1).astype(np.float64)
    A, B, Cc = p[idx[:, 0]], p[idx[:, 1]], p[idx[:, 2]]
    assert (np.einsum("ij,ij->i", np.cross(B - A, Cc - A), A + B + Cc) < 0).all()
    # faces off: exactly the clean samples, and the same flags but for the vertex bit
    v0, t0, flags0 = pc.mesh_np(z, *cam, step=step, z_lo=Z_LO, z_hi=Z_HI, edge_rtol=RTOL, faces=False)
    assert t0.shape == (0,) and v0.tobytes() == cloud[((flags & pc.F_CLEAN) != 0).reshape(-1)].tobytes()
    assert np.array_equal(flags0 & ~np.uint8(pc.F_VERTEX), flags & ~np.uint8(pc.F_VERTEX))
    assert np.array_equal((flags0 & pc.F_VERTEX) != 0, (flags0 & pc.F_CLEAN) != 0)


@pytest.mark.parametrize("step", [1, 2])
def test_no_tolerance_makes_every_valid_block_a_quad(step):
    h, w = 37, 53
    z = with_bad_patch(scene(h, w, step))
    v, t, flags = pc.mesh_np(z, *camera(h, w), step=step, z_lo=Z_LO, z_hi=Z_HI, edge_rtol=0.0, edge_atol=0.0)
    valid = (flags & pc.F_VALID) != 0
    assert not (flags & pc.F_EDGE).any()
    want = valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, 1:] & valid[1:, :-1]
    assert np.array_equal((flags[:-1, :-1] & pc.F_QUAD) != 0, want) and 0 < want.sum() < want.size
    assert not (flags[-1] & pc.F_QUAD).any() and not (flags[:, -1] & pc.F_QUAD).any()
    assert t.shape[0] == 2 * want.sum()


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)], ids=lambda s: "%dx%d" % s)
def test_a_grid_without_quads(shape):
    z = np.full(shape, 2.0, f32)
    v, t, _ = pc.mesh_np(z, 5, 5, 0, 0, edge_rtol=RTOL)
    assert v.shape == (0,) and t.shape == (0,)
    v, t, _ = pc.mesh_np(z, 5, 5, 0, 0, edge_rtol=RTOL, faces=False)
    assert v.shape == (shape[0] * shape[1],) and t.shape == (0,)
    with pytest.raises(ValueError):
        pc.mesh_np(z, 5, 5, 0, 0, edge_rtol=-0.1)
    with pytest.raises(ValueError):
        pc.mesh_np(z, 5, 5, 0, 0, edge_atol=float("nan"))


# ---- PLY -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [True, False], ids=["rgb", "xyz"])
def test_ply_mesh_round_trip_and_header(tmp_path, colour):
    h, w = 37, 53
    v, t, _ = pc.mesh_np(scene(h, w), *camera(h, w), photo=photo(h, w)[0] if colour else None, z_lo=Z_LO, z_hi=Z_HI)
    path = tmp_path / "mesh.ply"
    pc.write_ply_mesh(path, v, t)
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {v.shape[0]}\n"
              "property float x\nproperty float y\nproperty float z\n"
              + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if colour else "")
              + f"element face {t.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    data = path.read_bytes()
    assert data[:len(header)] == header == pc.mesh_header(v.shape[0], t.shape[0], colour)
    assert data[len(header):] == v.tobytes() + t.tobytes()
    assert len(data) == len(header) + v.shape[0] * (15 if colour else 12) + t.shape[0] * 13
    v2, t2 = pc.read_ply_mesh(path)
    assert v2.dtype == v.dtype and v2.tobytes() == v.tobytes()
    assert t2.dtype == pc.FACE_DTYPE and t2.tobytes() == t.tobytes()
    # an empty mesh is a file too
    pc.write_ply_mesh(tmp_path / "e.ply", v[:0], t[:0])
    v3, t3 = pc.read_ply_mesh(tmp_path / "e.ply")
    assert v3.shape == (0,) and t3.shape == (0,)


def test_ply_mesh_refusals(tmp_path):
    h, w = 9, 5
    v, t, _ = pc.mesh_np(scene(h, w), *camera(h, w), z_lo=Z_LO, z_hi=Z_HI)
    with pytest.raises(ValueError):
        pc.write_ply_mesh(tmp_path / "a.ply", v, np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError):
        pc.write_ply_mesh(tmp_path / "a.ply", np.zeros(3, np.float32), t)
    pc.write_ply(tmp_path / "cloud.ply", v)
    with pytest.raises(ValueError):
        pc.read_ply_mesh(tmp_path / "cloud.ply")  # no face element
    pc.write_ply_mesh(tmp_path / "b.ply", v, t)
    (tmp_path / "b.ply").write_bytes((tmp_path / "b.ply").read_bytes()[:-1])
    with pytest.raises(ValueError):
        pc.read_ply_mesh(tmp_path / "b.ply")
    bad = t.copy()
    bad["n"][0] = 4
    pc.write_ply_mesh(tmp_path / "c.ply", v, bad)
    with pytest.raises(ValueError):
        pc.read_ply_mesh(tmp_path / "c.ply")


# ---- the ABI's argument checks: no device call ---------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


P = ctypes.c_void_p(4096)  # never dereferenced: the checks run first
BIG = 2 ** 31 - 256
WS88 = 2 * 4 + 8 * 8 * 5   # mde_op_depth_mesh_ws_bytes(1, 8, 8, 1)


def test_prototypes_and_ws_bytes(lib):
    assert "mde_op_depth_mesh" in _lib.PROTOTYPES and "mde_op_depth_mesh_ws_bytes" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["mde_op_depth_mesh"]) == 27
    assert lib.mde_version() == 12
    f = lib.mde_op_depth_mesh_ws_bytes
    # two ints per tile of 1024 samples, an int32 index and a flag byte per sample
    assert f(1, 8, 8, 1) == WS88 == pc.mesh_ws_bytes(1, 8, 8)
    assert f(1, 32, 33, 1) == 2 * 2 * 4 + 32 * 33 * 5
    assert f(2, 600, 800, 1) == 2 * (469 * 8 + 480000 * 5) and f(1, 600, 800, 2) == 118 * 8 + 120000 * 5
    assert f(0, 8, 8, 1) == 0 and f(1, 8, 8, 0) == 0 and f(1, 1, BIG, 1) == 0 and f(65536, 8, 8, 1) == 0


@pytest.mark.parametrize("kw, msg", [
    (dict(depth=None), b"null"), (dict(vertices=None), b"null"), (dict(vcounts=None), b"null"),
    (dict(batch=0), b"positive"), (dict(h=0), b"positive"), (dict(w=-1), b"positive"), (dict(step=0), b"step"),
    (dict(photo=P, pitch=23), b"pitch"),
    (dict(f=None, fx=0.0), b"fx"), (dict(f=None, fy=-1.0), b"fx"), (dict(f=None, fx=float("nan")), b"fx"),
    (dict(cx=float("nan")), b"cx"),
    (dict(h=1, w=BIG, vbytes=1 << 62, fbytes=1 << 62, ws_bytes=1 << 62), b"2^31"),
    (dict(batch=65536, vbytes=1 << 40, fbytes=1 << 40, ws_bytes=1 << 40), b"65535"),
    (dict(vbytes=8 * 8 * 12 - 1), b"vertices_bytes"), (dict(photo=P, pitch=24, vbytes=8 * 8 * 15 - 1), b"vertices_bytes"),
    (dict(batch=2, vbytes=2 * 8 * 8 * 12 - 1, ws_bytes=1 << 20), b"vertices_bytes"),
    (dict(z_lo=2.0, z_hi=1.0), b"z_lo"), (dict(z_lo=float("nan")), b"z_lo"),
    (dict(rtol=-0.1), b"edge_rtol"), (dict(atol=-1.0), b"edge_rtol"), (dict(rtol=float("nan")), b"edge_rtol"),
    (dict(atol=float("nan")), b"edge_rtol"),
    (dict(faces=1, frecords=None), b"face"), (dict(faces=1, fcounts=None), b"face"),
    (dict(faces=1, fbytes=2 * 7 * 7 * 13 - 1), b"faces_bytes"),
    (dict(faces=1, step=3, fbytes=2 * 2 * 2 * 13 - 1), b"faces_bytes"),
    (dict(faces=1, h=40000, w=40000, step=1, vbytes=1 << 62, fbytes=1 << 62, ws_bytes=1 << 62), b"2 * (hs - 1)"),
    (dict(ws=None), b"ws"), (dict(ws_bytes=WS88 - 1), b"ws"), (dict(ws=ctypes.c_void_p(4098)), b"aligned"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_depth_mesh_checks_arguments_before_any_device_call(lib, kw, msg):
    def call(depth=P, batch=1, h=8, w=8, step=1, photo=None, pitch=0, f=P, fx=0.0, fy=0.0, cx=4.0, cy=4.0, z_lo=1e-4,
             z_hi=1e4, rtol=0.1, atol=0.0, faces=0, vertices=P, vbytes=8 * 8 * 15, vcounts=P, frecords=P,
             fbytes=2 * 7 * 7 * 13, fcounts=P, ws=P, ws_bytes=WS88):
        return lib.mde_op_depth_mesh(depth, batch, h, w, step, photo, pitch, 0, f, fx, fy, cx, cy, z_lo, z_hi, rtol,
                                     atol, faces, vertices, vbytes, vcounts, frecords, fbytes, fcounts, ws, ws_bytes,
                                     None)

    if "fy" in kw:
        kw = dict(kw, fx=1.0)
    elif "fx" in kw:
        kw = dict(kw, fy=1.0)
    assert call(**kw) == 1, kw
    err = lib.mde_last_error()
    assert b"mde_op_depth_mesh:" in err and msg in err, (kw, err)


# ---- the drivers' flags --------------------------------------------------------------------------------

def test_driver_parsers_accept_the_mesh_flags():
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run as dav2
    from monocular_depth_estimation_trt_amd.models.depth_pro import run as dp
    for mod, extra in ((dp, []), (dav2, ["--f-px", "500"])):
        a = mod.build_parser().parse_args(["--mesh", "m.ply", "--mesh-step", "2", "--edge-atol", "0.5"] + extra)
        assert a.mesh == "m.ply" and a.mesh_step == 2 and a.edge_rtol == 0.1 and a.edge_atol == 0.5
        assert a.ply_edge_rtol is None
        d = mod.build_parser().parse_args(["--ply", "c.ply", "--ply-edge-rtol", "0.05"])
        assert d.mesh == "" and d.mesh_step == 1 and d.ply_edge_rtol == 0.05


def test_drivers_refuse_a_mesh_they_cannot_serve():
    from monocular_depth_estimation_trt_amd.models.depth_anything_ac import run as ac
    from monocular_depth_estimation_trt_amd.models.depth_anything_v2 import run as dav2
    from monocular_depth_estimation_trt_amd.models.depth_pro import run as dp
    for argv, word in ((["--mesh", "m.ply", "--host-postprocess"], "device post-process"),
                       (["--mesh", "m.ply", "--mesh-step", "0"], "--mesh-step"),
                       (["--mesh", "m.ply", "--edge-rtol", "-1"], "--edge-rtol"),
                       (["--ply-edge-rtol", "0.1"], "needs --ply"),
                       (["--ply", "c.ply", "--ply-edge-rtol", "-0.1"], "--ply-edge-rtol")):
        with pytest.raises(SystemExit) as e:
            dp.main(argv)
        assert word in str(e.value), argv
    with pytest.raises(SystemExit) as e:
        dav2.main(["--source", "synthetic:vits:metric:1234", "--mesh", "m.ply"])
    assert "--f-px" in str(e.value) and "--mesh" in str(e.value)
    with pytest.raises(SystemExit) as e:
        dav2.main(["--source", "synthetic:vits:relative:1234", "--mesh", "m.ply", "--f-px", "500"])
    assert "metric" in str(e.value)
    with pytest.raises(SystemExit) as e:
        ac.main(["--mesh", "m.ply", "--f-px", "500"])
    assert "metric" in str(e.value)
