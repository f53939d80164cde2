"""The refusals of the three ops that take a cloud source -- mde_op_point_cloud, mde_op_depth_mesh and
mde_op_cloud_view -- as one table: an argument set with one thing wrong, or two to pin which check comes
first, and the text the caller sees.  The texts were recorded from the library before the three wrappers
shared their checks (csrc/ops_abi.hip: cloud_source_error); they are part of the ABI's behaviour.

No GPU: every call returns MDE_ERR_ARG before any HIP call, so the fake pointers are never dereferenced.
"""

import ctypes
import os

import pytest

from monocular_depth_estimation_trt_amd import _lib

P = ctypes.c_void_p(4096)     # never dereferenced: the checks run first
ODD = ctypes.c_void_p(4100)   # 4-byte but not 8-byte aligned
NAN = float("nan")
H = W = 8
REC = 12                      # bytes per vertex without a photo
MESH_WS = 2 * 4 + H * W * 5   # mde_op_depth_mesh_ws_bytes(1, 8, 8, 1)
SIZE = (7, 9)                 # the picture of the cloud-view calls


@pytest.fixture(scope="module")
def lib():
    from monocular_depth_estimation_trt_amd import _build
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.lib()


def source(kw):
    """The cloud-source arguments, the same thirteen for the three ops."""
    g = dict(depth=P, batch=1, h=H, w=W, step=1, photo=None, pitch=0, f=P, fx=0.0, fy=0.0, cx=4.0, cy=4.0)
    g.update({k: kw.pop(k) for k in list(kw) if k in g})
    return (g["depth"], g["batch"], g["h"], g["w"], g["step"], g["photo"], g["pitch"], 0, g["f"], g["fx"], g["fy"],
            g["cx"], g["cy"])


def point_cloud(lib, **kw):
    src = source(kw)
    o = dict(compact=1, records=P, nbytes=H * W * REC, counts=P, ws=P, ws_bytes=4)
    o.update(kw)
    return lib.mde_op_point_cloud(*src, o["compact"], 1e-4, 1e4, o["records"], o["nbytes"], o["counts"], o["ws"],
                                  o["ws_bytes"], None)


def depth_mesh(lib, **kw):
    src = source(kw)
    o = dict(faces=1, records=P, nbytes=H * W * REC, counts=P, frecords=P, fbytes=2 * 7 * 7 * 13, fcounts=P, ws=P,
             ws_bytes=MESH_WS)
    o.update(kw)
    return lib.mde_op_depth_mesh(*src, 1e-4, 1e4, 0.1, 0.0, o["faces"], o["records"], o["nbytes"], o["counts"],
                                 o["frecords"], o["fbytes"], o["fcounts"], o["ws"], o["ws_bytes"], None)


def cloud_view(lib, **kw):
    src = source(kw)
    o = dict(records=P, counts=P, view_in=None, out_h=SIZE[0], out_w=SIZE[1], ws=P,
             ws_bytes=lib.mde_op_cloud_view_ws_bytes(1, H, W, 1, *SIZE))
    o.update(kw)
    return lib.mde_op_cloud_view(*src, 1.0, 0.0, 1.0, 0.0, o["view_in"], (ctypes.c_int * 3)(22, 22, 26), 0,
                                 o["records"], o["out_h"], o["out_w"], o["counts"], o["ws"], o["ws_bytes"], None)


OPS = {"mde_op_point_cloud": point_cloud, "mde_op_depth_mesh": depth_mesh, "mde_op_cloud_view": cloud_view}
HUGE = 1 << 40

NULL = "null pointer"
STEP = "step must be positive"
BATCH = "batch > 65535"
PITCH = "pitch < 3 * w"
FOCAL = "f_px_dev is null and fx <= 0 or fy <= 0"
CENTRE = "cx or cy is NaN"
WS = {"mde_op_point_cloud": "compact mode needs ws of mde_op_point_cloud_ws_bytes()",
      "mde_op_depth_mesh": "needs ws of mde_op_depth_mesh_ws_bytes()",
      "mde_op_cloud_view": "needs ws of mde_op_cloud_view_ws_bytes()"}
SHORT = {"mde_op_point_cloud": "records_bytes < batch * hs * ws * record size",
         "mde_op_depth_mesh": "vertices_bytes < batch * hs * ws * record size"}

# `records` / `counts` are each op's first two output pointers (the picture and the view rows for the view)
SHARED = [
    (dict(depth=None), NULL),
    (dict(records=None), NULL),
    (dict(counts=None), NULL),
    (dict(step=0), STEP),
    (dict(batch=65536, nbytes=HUGE, fbytes=HUGE, ws_bytes=HUGE), BATCH),
    (dict(photo=P, pitch=3 * W - 1), PITCH),
    (dict(f=None), FOCAL),
    (dict(f=None, fx=1.0, fy=-1.0), FOCAL),
    (dict(cx=NAN), CENTRE),
    (dict(ws_bytes="one short"), WS),
    # two things wrong: the first check of today's order speaks
    (dict(depth=None, step=0), NULL),
    (dict(records=None, step=0), NULL),
    (dict(step=0, batch=0), "batch and sizes must be positive"),
    (dict(step=0, batch=65536), STEP),
    (dict(batch=65536, photo=P, pitch=3 * W - 1), BATCH),
    (dict(photo=P, pitch=3 * W - 1, f=None), PITCH),
    (dict(f=None, cx=NAN), FOCAL),
    (dict(cx=NAN, ws_bytes=0), CENTRE),
]
OWN = {
    "mde_op_point_cloud": [
        (dict(nbytes=H * W * REC - 1), SHORT["mde_op_point_cloud"]),
        (dict(photo=P, pitch=3 * W, nbytes=H * W * 15 - 1), SHORT["mde_op_point_cloud"]),
        (dict(cx=NAN, nbytes=0), CENTRE),
        (dict(nbytes=0, ws_bytes=0), SHORT["mde_op_point_cloud"]),
        (dict(compact=0, ws=None, ws_bytes=0, step=0), STEP),
    ],
    "mde_op_depth_mesh": [
        (dict(nbytes=H * W * REC - 1), SHORT["mde_op_depth_mesh"]),
        (dict(photo=P, pitch=3 * W, nbytes=H * W * 15 - 1), SHORT["mde_op_depth_mesh"]),
        (dict(cx=NAN, nbytes=0), CENTRE),
        (dict(frecords=None), "faces with a null face_records or face_counts"),
        (dict(frecords=None, nbytes=0), SHORT["mde_op_depth_mesh"]),
        (dict(frecords=None, ws_bytes=0), "faces with a null face_records or face_counts"),
        (dict(frecords=None, step=0), STEP),
        (dict(faces=0, frecords=None, fcounts=None, ws_bytes=MESH_WS - 1), WS["mde_op_depth_mesh"]),
    ],
    "mde_op_cloud_view": [
        (dict(batch=21846, ws_bytes=HUGE), "batch > 21845"),
        (dict(batch=21846, photo=P, pitch=3 * W - 1, ws_bytes=HUGE), "batch > 21845"),
        (dict(batch=65536, out_h=0), BATCH),
        (dict(step=0, out_h=0), STEP),
        (dict(out_h=0, f=None), "the picture's sizes must be positive"),
        (dict(counts=ODD), "ws, view_in and view_out must be 8-byte aligned"),
        (dict(view_in=ODD), "ws, view_in and view_out must be 8-byte aligned"),
        (dict(counts=ODD, ws_bytes=0), WS["mde_op_cloud_view"]),
        (dict(counts=ODD, cx=NAN), CENTRE),
    ],
}


def cases():
    for op in OPS:
        for kw, text in SHARED + OWN[op]:
            yield pytest.param(op, kw, text[op] if isinstance(text, dict) else text,
                               id=op[7:] + "-" + "-".join(f"{k}={v}" for k, v in kw.items()))


@pytest.mark.parametrize("op, kw, text", list(cases()))
def test_refusal_text(lib, op, kw, text):
    kw = dict(kw)
    if kw.get("ws_bytes") == "one short":  # what the op asks for, less one byte
        need = {"mde_op_point_cloud": 4, "mde_op_depth_mesh": MESH_WS,
                "mde_op_cloud_view": lib.mde_op_cloud_view_ws_bytes(1, H, W, 1, *SIZE)}[op]
        kw["ws_bytes"] = need - 1
    assert OPS[op](lib, **kw) == 1, (op, kw)  # MDE_ERR_ARG
    assert lib.mde_last_error().decode() == f"{op}: {text}", (op, kw)


def test_the_good_arguments_are_not_what_is_refused(lib):
    """Every row above changes these defaults: the sizes they rest on are the ops' own."""
    assert lib.mde_op_point_cloud_ws_bytes(1, H, W, 1) == 4
    assert lib.mde_op_depth_mesh_ws_bytes(1, H, W, 1) == MESH_WS
    assert lib.mde_op_cloud_view_ws_bytes(1, H, W, 1, *SIZE) > 0


@pytest.mark.parametrize("geometry", [(1, H, W, 0), (65536, H, W, 1), (0, H, W, 1), (1, 1, 2 ** 31 - 256, 1)])
def test_ws_bytes_is_zero_for_a_refused_geometry(lib, geometry):
    assert lib.mde_op_point_cloud_ws_bytes(*geometry) == 0
    assert lib.mde_op_depth_mesh_ws_bytes(*geometry) == 0
    assert lib.mde_op_cloud_view_ws_bytes(*geometry, *SIZE) == 0


def test_cloud_view_ws_bytes_has_the_stricter_limits(lib):
    assert lib.mde_op_cloud_view_ws_bytes(21846, H, W, 1, *SIZE) == 0
    assert lib.mde_op_cloud_view_ws_bytes(21845, H, W, 1, *SIZE) > 0
    assert lib.mde_op_cloud_view_ws_bytes(1, H, W, 1, 0, 9) == 0
    assert lib.mde_op_point_cloud_ws_bytes(21846, H, W, 1) > 0 and lib.mde_op_depth_mesh_ws_bytes(21846, H, W, 1) > 0
