"""The C-ABI library loads and exports every symbol include/mde.h declares
(no compute calls: runs without a GPU)."""

import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mde.h")


def declared_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mde_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib_path():
    from monocular_depth_estimation_trt_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build_library()
    return _lib.LIB_PATH


def test_header_declares_the_api():
    fns = declared_functions()
    for must in ("mde_engine_load", "mde_context_create", "mde_context_enqueue", "mde_context_set_tensor_address",
                 "mde_rt_malloc_host", "mde_op_attention", "mde_last_error", "mde_version"):
        assert must in fns


def test_every_declared_symbol_is_exported(lib_path):
    from monocular_depth_estimation_trt_amd import _lib
    lib = _lib.lib()  # (a bare ctypes.CDLL before torch would map a second HIP runtime)
    missing = [f for f in declared_functions() if not hasattr(lib, f)]
    assert not missing, missing


def test_python_binding_covers_the_header(lib_path):
    from monocular_depth_estimation_trt_amd import _lib
    assert set(declared_functions()) == set(_lib.PROTOTYPES), \
        set(declared_functions()) ^ set(_lib.PROTOTYPES)
    L = _lib.lib()
    ver = int(re.search(r"#define MDE_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert L.mde_version() == ver


def test_info_struct_matches_header():
    """ctypes mirror of mde_engine_info / mde_io_desc has every header field, in order."""
    from monocular_depth_estimation_trt_amd import _lib
    txt = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} mde_engine_info;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"([a-z_0-9]+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [f[0] for f in _lib.mde_engine_info._fields_]


def test_errors_without_gpu_are_reported_not_crashed(lib_path):
    """Host-side argument checks answer before any device call."""
    from monocular_depth_estimation_trt_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.mde_engine_load(b"/nonexistent/engine.mdeng", 0, ctypes.byref(h))
    assert rc == 2 and b"cannot open" in L.mde_last_error()
    rc = L.mde_engine_load_memory(b"NOTAPACK" + b"\0" * 400, 408, 0, ctypes.byref(h))
    assert rc == 3 and b"magic" in L.mde_last_error()
    rc = L.mde_op_linear(None, 8, None, 64, 4, 4, 8, None, 0, None, 4, None)
    assert rc == 1


def test_tuning_switches(lib_path):
    """The library's dispatch switches (include/mde.h mde_tuning_set/_get):
    defaults, range and name checks, and the context manager restores."""
    from monocular_depth_estimation_trt_amd import _lib
    L = _lib.lib()
    for name in _lib.TUNING:
        assert _lib.get_tuning(name) == _lib.TUNING_DEFAULT.get(name, 1), name
    v = ctypes.c_int()
    assert L.mde_tuning_get(b"no_such_switch", ctypes.byref(v)) == 5
    assert L.mde_tuning_set(b"splitk", 2) == 1
    assert L.mde_tuning_set(b"gemm256", 2) == 0 and _lib.get_tuning("gemm256") == 2
    _lib.set_tuning("gemm256", 1)
    with _lib.tuning(splitk=0, deep64=0):
        assert _lib.get_tuning("splitk") == 0 and _lib.get_tuning("deep64") == 0
    assert _lib.get_tuning("splitk") == 1 and _lib.get_tuning("deep64") == 1
    with pytest.raises(ValueError):
        _lib.set_tuning("lnfold", 7)


def test_last_gemm_route_before_any_launch(lib_path):
    """mde_debug_last_gemm_route on a new thread (the record is per thread):
    no launch yet, and the buffer checks (include/mde.h)."""
    import threading
    from monocular_depth_estimation_trt_amd import _lib
    got = {}

    def fresh_thread():
        got["route"] = _lib.last_gemm_route()
        got["rc"] = (_lib.lib().mde_debug_last_gemm_route(ctypes.create_string_buffer(4), 4),
                     _lib.lib().mde_debug_last_gemm_route(None, 0))

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert got == {"route": {"kind": "none"}, "rc": (1, 1)}, got


def test_last_attention_route_before_any_launch(lib_path):
    """mde_debug_last_attention_route on a new thread (the record is per
    thread): no launch yet, and the same buffer checks."""
    import threading
    from monocular_depth_estimation_trt_amd import _lib
    got = {}

    def fresh_thread():
        got["route"] = _lib.last_attention_route()
        got["rc"] = (_lib.lib().mde_debug_last_attention_route(ctypes.create_string_buffer(4), 4),
                     _lib.lib().mde_debug_last_attention_route(None, 0))
        got["route32"] = _lib.last_attention32_route()
        got["rc32"] = (_lib.lib().mde_debug_last_attention32_route(ctypes.create_string_buffer(4), 4),
                       _lib.lib().mde_debug_last_attention32_route(None, 0))

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert got == {"route": {"kernel": "none"}, "rc": (1, 1), "route32": {"kernel": "none"}, "rc32": (1, 1)}, got


def _run_py(code, env=None):
    import subprocess
    import sys
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600, env=e)
    return r.returncode, r.stdout + r.stderr


def test_tuning_reads_environment_once(lib_path):
    rc, out = _run_py("from monocular_depth_estimation_trt_amd import _lib\n"
                      "print('VALS', _lib.get_tuning('splitk'), _lib.get_tuning('gemm256'), _lib.get_tuning('w8small'))",
                      {"MDE_SPLITK": "0", "MDE_GEMM256": "2", "MDE_W8SMALL": "bogus"})
    assert rc == 0, out
    # a marked line: the GPU driver stack may write lines of its own to stderr
    vals = [l for l in out.splitlines() if l.startswith("VALS ")][-1]
    assert vals.split()[1:] == ["0", "2", "1"], out
    assert "MDE_W8SMALL=bogus ignored" in out, out


def test_one_hip_runtime_when_torch_comes_first(lib_path):
    """_lib.lib() brings torch's bundled HIP runtime up first; libmde_hip then
    binds to it (same SONAME), so exactly one runtime is mapped and it is
    torch's -- the runtime that owns the streams torch passes in."""
    rc, out = _run_py("from monocular_depth_estimation_trt_amd import _lib\n"
                      "_lib.lib()\n"
                      "print('RT', _lib.hip_runtimes())")
    assert rc == 0, out
    line = [l for l in out.splitlines() if l.startswith("RT ")][-1]
    rts = eval(line[3:])
    assert len(rts) == 1 and "torch" in rts[0], out


def test_two_hip_runtimes_are_refused(lib_path):
    """libmde_hip loaded before torch maps ROCm's runtime; a later torch
    import maps its own second copy (the r3 smoke failure).  The binding
    refuses that state with an explanation instead of failing in hipSetDevice."""
    rc, out = _run_py("import ctypes\n"
                      f"ctypes.CDLL({lib_path!r})\n"
                      "import torch\n"
                      "torch.cuda.is_available()\n"
                      "from monocular_depth_estimation_trt_amd import _lib\n"
                      "try:\n"
                      "    _lib.lib()\n"
                      "except ImportError as e:\n"
                      "    print('REFUSED', e)\n")
    assert rc == 0, out
    assert "REFUSED two HIP runtimes" in out, out


@pytest.mark.parametrize("tpad, heads, msg", [(40, 6, b"% 16"), (36, 6, b"tokens_pad < tokens"), (48, 0, b"> 0")])
def test_qkv_ops_reject_bad_geometry(lib_path, tpad, heads, msg):
    """V^T stores key t at vt_pos(t) (bits 2 and 3 swapped), so a
    tokens_pad that is not a multiple of 16 would spill the last key group into
    the next row.  Both qkv entry points refuse it before touching the device."""
    from monocular_depth_estimation_trt_amd import _lib
    lib = _lib.lib()
    p = 4096  # never dereferenced: the geometry check runs first
    rc = lib.mde_op_qkv(p, p, 384, p, 1, 37, heads, tpad, 0.125, p, p, p, None)
    assert rc != 0 and msg in lib.mde_last_error()
    rc = lib.mde_op_qkv_lnfold(p, p, 1e-6, p, 384, p, p, 1, 37, heads, tpad, 0.125, p, p, p, None)
    assert rc != 0 and msg in lib.mde_last_error()


def test_engine_path_wrappers_reject_bad_arguments(lib_path):
    """The ABI 11 wrappers (mde_op_linear_res, ..., mde_op_linear_residual_split) answer null
    pointers, tokens < 2, a misaligned ConvT slot and fused split-K operands that do not fit before
    any kernel launch (the pointers below are never dereferenced)."""
    from monocular_depth_estimation_trt_amd import _lib
    L = _lib.lib()
    p = 4096

    def err(rc, msg):
        assert rc == 1, (rc, L.mde_last_error())
        assert msg in L.mde_last_error(), L.mde_last_error()

    err(L.mde_op_linear_res(None, 72, p, 128, 185, 96, 72, p, 0, None, 0, 0, None, p, 96, None, 0, None, None, 0, 0,
                            None), b"null")
    err(L.mde_op_linear_res(p, 72, p, 128, 185, 96, 72, p, 0, None, 37, 0, None, p, 96, None, 0, None, None, 0, 0,
                            None), b"without res0")
    # 185 x 96 has 3 x 2 tiles of 64^2: one counter is too few; slots past the workspace
    err(L.mde_op_linear_res(p, 768, p, 768, 185, 96, 768, p, 0, None, 0, 0, None, p, 96, p, 1 << 18, None, p, 1, 1 << 18,
                            None), b"fewer counters")
    err(L.mde_op_linear_res(p, 768, p, 768, 185, 96, 768, p, 0, None, 0, 0, None, p, 96, p, 1 << 10, None, p, 64,
                            1 << 18, None), b"exceeds the workspace")
    err(L.mde_op_conv3x3_res(p, 1, 19, 19, 384, p, 3456, 64, 1, 0, p, 0, None, 0, None, None, 0, 0, None, None, 0, None,
                             None, 0, 0, None), b"null")
    err(L.mde_op_conv3x3_res(p, 1, 19, 19, 384, p, 3456, 64, 1, 0, p, 0, None, 1, None, None, 0, 0, p, None, 0, None,
                             None, 0, 0, None), b"res0_relu without res0")
    err(L.mde_op_conv3x3_res(p, 1, 19, 19, 384, p, 3456, 64, 1, 0, p, 0, None, 0, None, p, 10, 10, p, None, 0, None,
                             None, 0, 0, None), b"res1_up needs res1")
    err(L.mde_op_conv3x3_res(p, 1, 19, 19, 384, p, 3456, 64, 1, 0, p, 0, None, 0, None, None, 0, 0, p, p, 1 << 20, None,
                             p, 5, 1 << 20, None), b"fewer counters")
    err(L.mde_op_linear_lnfold_tok(p, None, 1e-6, p, 384, p, p, 7, 38, 48, 384, 0, p, 48, None), b"null")
    err(L.mde_op_linear_lnfold_tok(p, p, 1e-6, p, 384, p, p, 7, 1, 48, 384, 0, p, 48, None), b"tokens >= 2")
    err(L.mde_op_depth_head_pe(p, 1, 8, 8, 32, 16, 16, p, 320, p, p, 0.0, 2, 1.0, p, 0, p, None), b"hpe_pix")
    err(L.mde_op_depth_head_pe(p, 1, 8, 8, 32, 16, 16, p, 320, p, None, 0.0, 2, 1.0, None, 0, p, None), b"null")
    err(L.mde_op_conv_transpose_ld(p, 1, 7, 9, 64, p, 64, 64, 2, p, None, 80, None), b"null")
    # a slot 8 bytes into the pixel (every store is 16 B), a stride below cout, a stride off 8
    err(L.mde_op_conv_transpose_ld(p, 1, 7, 9, 64, p, 64, 64, 2, p, p + 8, 80, None), b"conv_transpose_ld")
    err(L.mde_op_conv_transpose_ld(p, 1, 7, 9, 64, p, 64, 64, 2, p, p, 56, None), b"conv_transpose_ld")
    err(L.mde_op_conv_transpose_ld(p, 1, 7, 9, 64, p, 64, 64, 2, p, p, 84, None), b"conv_transpose_ld")
    rs = L.mde_op_linear_residual_split
    err(rs(p, 1536, p, 1536, 300, 384, 1536, p, p, p, p, 384, None, 4, p, 1 << 22, None, 0, 0, None), b"one of x32 / xh")
    err(rs(p, 1536, p, 1536, 300, 384, 1536, p, p, None, None, 384, None, 4, p, 1 << 22, None, 0, 0, None),
        b"one of x32 / xh")
    err(rs(p, 1536, p, 1536, 300, 384, 1536, p, p, p, None, 384, p, 4, p, 1 << 22, None, 0, 0, None), b"ln_partials")
    # 2 slices asked: the workspace must still hold 4 x 300 x 384 floats
    err(rs(p, 1536, p, 1536, 300, 384, 1536, p, p, p, None, 384, None, 2, p, 2 * 300 * 384, None, 0, 0, None),
        b"max(splitk, 4)")
    err(rs(p, 1536, p, 1536, 300, 384, 1536, p, p, p, None, 384, None, 4, p, 1 << 22, p, 29, 1 << 22, None),
        b"fewer counters")


def test_row_and_head_wrappers_reject_bad_arguments(lib_path):
    """The ABI 12 wrappers (mde_op_layernorm32 ... mde_op_patch_embed32) answer null pointers and sizes
    their kernels cannot take before any launch (the pointers below are never dereferenced)."""
    from monocular_depth_estimation_trt_amd import _lib
    L = _lib.lib()
    p = 4096

    def err(rc, msg):
        assert rc == 1, (rc, L.mde_last_error())
        assert msg in L.mde_last_error(), L.mde_last_error()

    err(L.mde_op_layernorm32(p, None, p, p, 21, 384, 1e-6, 7, 0, None), b"mde_op_layernorm32: null")
    err(L.mde_op_layernorm32(p, p, p, p, 21, 384, 1e-6, 1, 1, None), b"tokens >= 2")
    err(L.mde_op_layernorm32(p, p, p, p, 20, 384, 1e-6, 7, 1, None), b"rows % tokens")
    err(L.mde_op_layernorm32(p, p, p, p, 21, 512, 1e-6, 7, 0, None), b"invalid shape")      # not a layernorm width
    err(L.mde_op_rows_layernorm(None, p, p, 3, 9, 5, 384, 1e-5, None), b"mde_op_rows_layernorm: null")
    err(L.mde_op_rows_layernorm(p, p, p, 3, 9, 9, 384, 1e-5, None), b"row0 outside")
    err(L.mde_op_rows_layernorm(p, p, p, 3, 9, 5, 320, 1e-5, None), b"invalid shape")
    err(L.mde_op_prefix_rows(p, None, 6, 9, 5, 384, 3, 2, None), b"mde_op_prefix_rows: null")
    err(L.mde_op_prefix_rows(p, p, 6, 9, 10, 384, 3, 2, None), b"npre outside")
    err(L.mde_op_prefix_rows(p, p, 6, 9, 5, 382, 3, 2, None), b"dim % 4")
    err(L.mde_op_prefix_rows(p, p, 6, 9, 5, 384, 3, 3, None), b"sets must be")
    err(L.mde_op_prefix_rows(p, p, 6, 9, 5, 384, 0, 2, None), b"frames")
    err(L.mde_op_prefix_rows(p + 4, p, 6, 9, 5, 384, 3, 2, None), b"16-byte")
    err(L.mde_op_cls_rows(p, None, 3, 7, 384, None), b"mde_op_cls_rows: null")
    err(L.mde_op_cls_rows(p, p, 0, 7, 384, None), b"must be positive")
    err(L.mde_op_fov_final(None, p, 0.5, 1000, 3, p, None), b"mde_op_fov_final: null")
    err(L.mde_op_fov_final(p, p, 0.5, 0, 3, p, None), b"must be positive")
    err(L.mde_op_head32(p, None, 0.1, 300, 1, 20.0, p, None), b"mde_op_head32: null")
    err(L.mde_op_head32(p, p, 0.1, 300, 3, 20.0, p, None), b"metric must be")
    err(L.mde_op_head32(p + 4, p, 0.1, 300, 1, 20.0, p, None), b"16-byte")
    pes = L.mde_op_patch_embed_stream
    err(pes(p, 2, 98, 98, p, 704, p, p, p, 384, 50, 1, None, p, None, None, None, None), b"null")
    err(pes(p, 2, 98, 98, p, 704, p, p, p, 384, 50, 1, p, p, p, None, None, None), b"exactly one of")
    err(pes(p, 2, 98, 98, p, 704, p, p, p, 384, 49, 1, p, p, None, None, None, None), b"exceeds tokens")
    err(pes(p, 2, 98, 13, p, 704, p, p, p, 384, 50, 1, p, p, None, None, None, None), b"at least 14")
    err(pes(p, 2, 98, 98, p, 704, p, p, p, 384, 49, 0, p, p, None, None, None, None), b"tok0 >= 1")
    err(pes(p, 2, 98, 98, p, 704, p, p, p, 384, 50, 1, p, p, None, p, p, None), b"come together")     # partials need xh
    err(pes(p, 2, 98, 98, p, 704, p, p, None, 384, 54, 5, p, None, p, p, p, None), b"come together")  # and a cls row
    err(pes(p, 2, 98, 98, p, 704, p, p, p, 400, 50, 1, p, None, p, p, p, None), b"dim % 32")
    err(L.mde_op_patch_embed32(p, 2, 98, 98, p, 672, p, p, None, 384, p, p, None), b"mde_op_patch_embed32: null")
    err(L.mde_op_patch_embed32(p, 0, 98, 98, p, 672, p, p, p, 384, p, p, None), b"positive")
