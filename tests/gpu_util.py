"""Helpers for the gpu-marked tests: torch device tensors in, C ABI calls."""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from monocular_depth_estimation_trt_amd import _lib


_KEEP = []  # tensors whose pointers are in flight: freed only after op() syncs


def ptr(t) -> C.c_void_p:
    """Device pointer of t; keeps t alive until the next op() has synchronized
    (a temporary passed inline would otherwise go back to the caching
    allocator and be reused by the next argument's allocation)."""
    if t is None:
        return C.c_void_p(0)
    _KEEP.append(t)
    return C.c_void_p(t.data_ptr())


def stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def op(name: str, *args) -> None:
    try:
        _lib.call(name, *args)
        torch.cuda.synchronize()
    finally:
        _KEEP.clear()


def vt_pos(t):
    """Key permutation of the V^T layout (csrc/mde_device.h vt_pos): bits 2
    and 3 of t swapped."""
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def vt_perm(T: int) -> torch.Tensor:
    """Index tensor: storage column of key t, t in [0, T)."""
    return torch.tensor([vt_pos(t) for t in range(T)], dtype=torch.long)


def pad_w(w: torch.Tensor, n_mult: int = 128, k_mult: int = 64) -> torch.Tensor:
    """[N][K] -> f16 [Npad][Kpad] zero-padded device tensor (the packer's layout)."""
    n, k = w.shape
    N = -(-n // n_mult) * n_mult
    K = -(-k // k_mult) * k_mult
    out = torch.zeros(N, K, dtype=torch.float16, device=w.device)
    out[:n, :k] = w.half()
    return out


def conv_w(w: torch.Tensor) -> torch.Tensor:
    """[Cout][Cin][3][3] -> packed [Cout][ky][kx][Cin]."""
    co, ci = w.shape[:2]
    return pad_w(w.permute(0, 2, 3, 1).reshape(co, 9 * ci))


def nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2).contiguous()


def close(got: torch.Tensor, ref: torch.Tensor, rtol: float, atol: float, what: str = "") -> None:
    g = got.float().cpu()
    r = ref.float().cpu()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    err = (g - r).abs()
    bound = atol + rtol * r.abs()
    bad = ~(err <= bound)  # NaN counts as bad
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements out of tolerance; "
                             f"max_abs {err.max():.4e}; first bad idx {i}: got {g.flatten()[i]:.6f} "
                             f"ref {r.flatten()[i]:.6f}")


def depth_metrics(got: np.ndarray, ref: np.ndarray) -> dict:
    g = np.asarray(got, np.float64).ravel()
    r = np.asarray(ref, np.float64).ravel()
    d = np.abs(g - r)
    return dict(max_abs=float(d.max()), mean_abs=float(d.mean()),
                rel_mean=float(d.mean() / max(np.abs(r).mean(), 1e-12)),
                corr=float(np.corrcoef(g, r)[0, 1]) if g.size > 1 else 1.0)


# ---- exact comparisons and the route record (test_gpu_exact.py, test_gpu_bilinear.py) ----

def ordinal16(t):
    """f16 -> int32, monotone in the value (+0 and -0 both 0): differences are ulps."""
    b = t.contiguous().view(torch.int16).int()
    return torch.where(b < 0, -(b & 0x7FFF), b)


def assert_equal(got, ref, what):
    """torch.equal(got, ref) by value (zeros of either sign agree, NaN never
    does); on failure the count, the bounding box and the largest difference."""
    g = got.detach().cpu()
    assert g.shape == ref.shape and g.dtype == ref.dtype, (what, g.shape, ref.shape, g.dtype, ref.dtype)
    if torch.equal(g, ref):
        return
    g2, r2 = g.reshape(-1, g.shape[-1]), ref.reshape(-1, ref.shape[-1])
    bad = g2 != r2
    rows, cols = bad.any(1).nonzero().flatten(), bad.any(0).nonzero().flatten()
    if g.dtype == torch.float16:
        d = (ordinal16(g2) - ordinal16(r2)).abs()[bad]
        worst = f"max {int(d.max())} f16 ulp"
    else:
        worst = f"max |d| {float((g2.double() - r2.double()).abs()[bad].nan_to_num(float('inf')).max()):.3e}"
    i = int(bad.flatten().nonzero()[0])
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from float64, rows {int(rows[0])}..{int(rows[-1])} "
        f"cols {int(cols[0])}..{int(cols[-1])} of {tuple(g2.shape)}, {worst}, {int(torch.isnan(g2).sum())} NaN; "
        f"first [{i // g2.shape[1]}][{i % g2.shape[1]}] got {float(g2.flatten()[i])!r} ref {float(r2.flatten()[i])!r}")


def assert_route(want, what):
    r = _lib.last_gemm_route()
    assert {f: r.get(f) for f in want} == want, (what, want, r)
    return r


def assert_attn_route(want, what):
    """The fields of _lib.last_attention_route() named in want."""
    r = _lib.last_attention_route()
    assert {f: r.get(f) for f in want} == want, (what, want, r)
    return r


def run_attention(gpu, launch, cfg, tail, q, k, v, B, H, T):
    """q, k, v [B H][T][64] f16 -> o [B T][H 64]: V^T through vt_perm, the
    pad of q, k and vt zero (the kernel's contract), o prefilled with NaN.
    launch: "policy" (mde_op_attention), "ws" (mde_op_attention_ws) or a name
    for cfg through mde_op_attention_cfg, with "attn_tail" = tail if given."""
    Tp = -(-T // 64) * 64
    qg = torch.zeros(B * H, Tp, 64, dtype=torch.float16, device=gpu)
    kg = torch.zeros_like(qg)
    vtg = torch.zeros(B * H, 64, Tp, dtype=torch.float16, device=gpu)
    qg[:, :T], kg[:, :T] = q.to(gpu), k.to(gpu)
    vtg[:, :, vt_perm(T).to(gpu)] = v.transpose(1, 2).to(gpu)
    o = torch.full((B * T, H * 64), float("nan"), dtype=torch.float16, device=gpu)
    nbytes = _lib.lib().mde_op_attention_ws_bytes(B, H, T)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=gpu)
    if launch == "policy":
        op("mde_op_attention", ptr(qg), ptr(kg), ptr(vtg), ptr(o), B, H, T, Tp, H * 64, stream())
    elif launch == "ws":
        op("mde_op_attention_ws", ptr(qg), ptr(kg), ptr(vtg), ptr(o), B, H, T, Tp, H * 64, ptr(ws), nbytes, stream())
    else:
        with _lib.tuning(**({"attn_tail": tail} if tail is not None else {})):
            op("mde_op_attention_cfg", ptr(qg), ptr(kg), ptr(vtg), ptr(o), B, H, T, Tp, H * 64, cfg.encode(), ptr(ws),
               nbytes, stream())
    return o


def to16(ref64):
    """float64 (exact in fp32) -> f16, one rounding."""
    return ref64.float().half()
