"""AOT weight packer: DA-V2 state dict -> packed engine file for libmde_hip.

Replaces the reference's export/build stage -- `run.py export` ->
`models/depth_anything_v2/onnx_export.py:19-100` (ONNX opset 20 + onnxsim)
and `run.py build` -> `core/common.py:166-274` (TensorRT builder) -- with one
deterministic host-side pass that lays the weights out for the gfx950 kernels:

* every matrix operand becomes f16 [Npad][Kpad] (K contiguous; N padded to a
  multiple of 128 and K to a multiple of 64 with zeros) -- the B-operand
  layout of the MFMA GEMM (csrc/gemm.hip);
* 3x3 conv weights [Cout][Cin][3][3] -> [Cout][ky][kx][Cin] (the implicit
  im2col K order over an NHWC map);
* ConvTranspose(k == s) weights [Cin][Cout][s][s] -> [(dy*s+dx)*Cout+co][Cin]
  (a plain GEMM whose epilogue pixel-shuffles);
* patch-embed [D][3][14][14] -> [D][3*14*16] (kx padded to 16 so every 8-wide
  K chunk of the im2col row is 16-byte aligned);
* the positional table is interpolated ONCE for the packed input size with
  upstream DINOv2's bicubic + 0.1-offset rule, and cls + pos[0] is folded;
* LayerNorm / LayerScale / bias vectors stay fp32.

File layout: csrc/pack_format.h.  A packed file is specific to one model
variant and one input size, like a TensorRT engine is to its profile.
"""

from __future__ import annotations

import hashlib
import math
import os
import struct
from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np

from . import weights as W

PACK_VERSION = 1
PACKER_VERSION = "mde-pack-1"
ALIGN = 256


def f32(a) -> np.ndarray:
    """LayerNorm / LayerScale / bias vectors: flat fp32."""
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def check_keys(sd: dict, keys, label: str = "") -> None:
    """Raise if the state dict lacks a key the packer reads (`label`: the family, for the message)."""
    missing = [k for k in keys if k not in sd and not k.endswith("mask_token")]
    if missing:
        raise KeyError(f"{label + ' ' if label else ''}state dict lacks {len(missing)} keys, e.g. {missing[:4]}")


def _pad2(a: np.ndarray, dtype=np.float16) -> np.ndarray:
    """[n][k] -> zero-padded [n -> x128][k -> x64 (f16) / x32 (fp32)]: the
    weight operand of the MFMA GEMM (csrc/gemm.hip) / the exact-fp32 GEMM
    (csrc/fp32.hip)."""
    n, k = a.shape
    k_mult = 64 if dtype == np.float16 else 32
    out = np.zeros((-(-n // 128) * 128, -(-k // k_mult) * k_mult), dtype)
    out[:n, :k] = a
    return out


def _1x1(w: np.ndarray, dtype=np.float16) -> np.ndarray:
    return _pad2(w.reshape(w.shape[0], -1), dtype)


def _conv3(w: np.ndarray, dtype=np.float16, cin_pad: int = 0) -> np.ndarray:
    """[Cout][Cin][3][3] -> [Cout_pad][9*Cin' padded] in (ky, kx, ci) order,
    Cin' = cin_pad (zero input channels appended) when given."""
    co, ci, kh, kw = w.shape
    assert kh == 3 and kw == 3, w.shape
    if cin_pad and cin_pad > ci:
        w = np.concatenate([w, np.zeros((co, cin_pad - ci, 3, 3), w.dtype)], axis=1)
        ci = cin_pad
    return _pad2(np.ascontiguousarray(w.transpose(0, 2, 3, 1)).reshape(co, 9 * ci), dtype)


def _convT(w: np.ndarray, dtype=np.float16) -> np.ndarray:
    """ConvTranspose2d weight [Cin][Cout][s][s] (k == s) -> [(dy*s+dx)*Cout+co][Cin]."""
    ci, co, s, s2 = w.shape
    assert s == s2
    return _pad2(np.ascontiguousarray(w.transpose(2, 3, 1, 0)).reshape(s * s * co, ci), dtype)


def interpolate_pos_embed(pos: np.ndarray, ph: int, pw: int) -> np.ndarray:
    """Upstream DINOv2 interpolate_pos_encoding (bicubic, scale_factor with the
    0.1 offset, antialias False).  [1, 1+M*M, D] -> [1, 1+ph*pw, D] fp32."""
    N = pos.shape[1] - 1
    if N == ph * pw and ph == pw:
        return pos.astype(np.float32)
    import torch
    import torch.nn.functional as F
    M = int(math.isqrt(N))
    if M * M != N:
        raise ValueError(f"pos_embed has {N} patch positions, not a square grid")
    D = pos.shape[-1]
    t = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32))
    patch = t[:, 1:].reshape(1, M, M, D).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, scale_factor=(float(ph + 0.1) / M, float(pw + 0.1) / M),
                          mode="bicubic", antialias=False)
    if tuple(patch.shape[-2:]) != (ph, pw):
        raise ValueError(f"pos-embed interpolation produced {tuple(patch.shape[-2:])}, wanted {(ph, pw)}")
    patch = patch.permute(0, 2, 3, 1).reshape(1, ph * pw, D)
    return torch.cat([t[:, :1], patch], 1).numpy()


def normalize_keys(sd: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Accept upstream checkpoints as saved (optionally 'module.'-prefixed)."""
    out = {}
    for k, v in sd.items():
        if k.startswith("module."):
            k = k[len("module."):]
        out[k] = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
    return out


def _fold_ln(w: np.ndarray, bias: np.ndarray, g: np.ndarray, beta: np.ndarray):
    """LayerNorm folded into the linear that follows it (the f16-residual
    engines' norm1 -> qkv and norm2 -> fc1, engine.hip): with x the raw
    residual row, LN(x) W^T + b = rstd * (x (W*g)^T - mean * c1) + c2, where
    W*g scales input column k by gamma[k], c1[n] = sum_k f16(W*g)[n][k] (the
    operand the MFMAs see) and c2 = b + f16(W) beta.  Returns the padded f16
    W*g, c1 and c2 (fp32, sums in fp64)."""
    w = np.asarray(w, np.float32)
    wg = (w.astype(np.float64) * np.asarray(g, np.float64)[None, :]).astype(np.float32)
    c1 = wg.astype(np.float16).astype(np.float64).sum(axis=1)
    c2 = np.asarray(bias, np.float64) + w.astype(np.float16).astype(np.float64) @ np.asarray(beta, np.float64)
    return _pad2(wg), c1.astype(np.float32), c2.astype(np.float32)


def _slice_partials(v: np.ndarray) -> np.ndarray:
    """Per 32-column slice, (sum, sum of squared deviations from the slice
    mean) of the f16-rounded row v -- the LayerNorm partials the fold's
    producers write (GemmParams::lnst_out)."""
    h = np.asarray(v, np.float32).astype(np.float16).astype(np.float64).reshape(-1, 32)
    m2 = ((h - h.mean(1, keepdims=True)) ** 2).sum(1)
    return np.stack([h.sum(1), m2], 1).astype(np.float32).reshape(-1)


def pack_block(o, sd, src: str, dst: str, hf: bool = False, qk_norm: bool = False, fold_ln: bool = False,
               dtype=np.float16) -> None:
    """One pre-LN ViT block's tensors, state-dict prefix `src` -> packed
    prefix `dst`, in file order.  hf: transformers' DINOv2 key names with
    split q / k / v (stored fused, rows [q; k; v]); qk_norm: VGGT's per-head
    q/k LayerNorm; fold_ln: also the LayerNorm-folded qkv / fc1 (_fold_ln);
    dtype float32: the exact-fp32 encoder's `.w32` linears."""
    if hf:
        qkv = [f"{src}attention.attention.{n}" for n in ("query", "key", "value")]
        qkv_w = np.concatenate([sd[k + ".weight"] for k in qkv], 0)
        qkv_b = np.concatenate([sd[k + ".bias"] for k in qkv], 0)
        proj, ls1, ls2 = src + "attention.output.dense", "layer_scale1.lambda1", "layer_scale2.lambda1"
    else:
        qkv_w, qkv_b = sd[src + "attn.qkv.weight"], sd[src + "attn.qkv.bias"]
        proj, ls1, ls2 = src + "attn.proj", "ls1.gamma", "ls2.gamma"
    w = ".w32" if dtype == np.float32 else ".w"
    o[dst + "ln1.g"] = f32(sd[src + "norm1.weight"])
    o[dst + "ln1.b"] = f32(sd[src + "norm1.bias"])
    o[dst + "qkv" + w] = _pad2(qkv_w, dtype)
    o[dst + "qkv.b"] = f32(qkv_b)
    if qk_norm:
        o[dst + "qn.g"] = f32(sd[src + "attn.q_norm.weight"])
        o[dst + "qn.b"] = f32(sd[src + "attn.q_norm.bias"])
        o[dst + "kn.g"] = f32(sd[src + "attn.k_norm.weight"])
        o[dst + "kn.b"] = f32(sd[src + "attn.k_norm.bias"])
    o[dst + "proj" + w] = _pad2(sd[proj + ".weight"], dtype)
    o[dst + "proj.b"] = f32(sd[proj + ".bias"])
    o[dst + "ls1"] = f32(sd[src + ls1])
    o[dst + "ln2.g"] = f32(sd[src + "norm2.weight"])
    o[dst + "ln2.b"] = f32(sd[src + "norm2.bias"])
    o[dst + "fc1" + w] = _pad2(sd[src + "mlp.fc1.weight"], dtype)
    o[dst + "fc1.b"] = f32(sd[src + "mlp.fc1.bias"])
    if fold_ln:
        o[dst + "qkv.wf"], o[dst + "qkv.c1"], o[dst + "qkv.c2"] = _fold_ln(
            qkv_w, qkv_b, sd[src + "norm1.weight"], sd[src + "norm1.bias"])
        o[dst + "fc1.wf"], o[dst + "fc1.c1"], o[dst + "fc1.c2"] = _fold_ln(
            sd[src + "mlp.fc1.weight"], sd[src + "mlp.fc1.bias"], sd[src + "norm2.weight"], sd[src + "norm2.bias"])
    o[dst + "fc2" + w] = _pad2(sd[src + "mlp.fc2.weight"], dtype)
    o[dst + "fc2.b"] = f32(sd[src + "mlp.fc2.bias"])
    o[dst + "ls2"] = f32(sd[src + ls2])


def pack_dpt_head(o, sd, cfg: dict, dtype=np.float16, fold_norm=None, pe=None, rf4_unit1: bool = True,
                  depth_only: bool = False) -> None:
    """The upstream DPT head ("depth_head.") in file order.  dtype float32:
    the exact-fp32 engine's `.w32` weights, no channel padding (the fp32 conv
    takes any channel count % 4).  fold_norm = (gamma, beta): the taps' final
    LayerNorm folded into the projects (`projN.wf/.c1/.c2`, engine.hip).
    VGGT: pe = (4 per-projection tables `peN`, `head.pe`), no resConfUnit1 in
    refinenet4, output_conv2's last 1x1 reduced to its depth channel."""
    h = "depth_head."
    w = ".w32" if dtype == np.float32 else ".w"
    for i in range(4):
        pw = sd[f"{h}projects.{i}.weight"]
        pw = pw.reshape(pw.shape[0], pw.shape[1])
        o[f"proj{i}{w}"] = _pad2(pw, dtype)
        o[f"proj{i}.b"] = f32(sd[f"{h}projects.{i}.bias"])
        if fold_norm is not None:
            o[f"proj{i}.wf"], o[f"proj{i}.c1"], o[f"proj{i}.c2"] = _fold_ln(pw, sd[f"{h}projects.{i}.bias"], *fold_norm)
        if pe is not None:
            o[f"pe{i}"] = pe[0][i]
    o["rs0" + w] = _convT(sd[h + "resize_layers.0.weight"], dtype)
    o["rs0.b"] = f32(sd[h + "resize_layers.0.bias"])
    o["rs1" + w] = _convT(sd[h + "resize_layers.1.weight"], dtype)
    o["rs1.b"] = f32(sd[h + "resize_layers.1.bias"])
    o["rs3" + w] = _conv3(sd[h + "resize_layers.3.weight"], dtype)
    o["rs3.b"] = f32(sd[h + "resize_layers.3.bias"])
    for i in range(4):
        # f16 DPT maps feeding the direct conv carry channels padded to x32 (48 -> 64)
        cin_pad = -(-cfg["out_channels"][i] // 32) * 32 if dtype == np.float16 else 0
        o[f"rn{i + 1}{w}"] = _conv3(sd[f"{h}scratch.layer{i + 1}_rn.weight"], dtype, cin_pad)
    for r in range(1, 5):
        s = f"{h}scratch.refinenet{r}."
        o[f"rf{r}.out{w}"] = _1x1(sd[s + "out_conv.weight"], dtype)
        o[f"rf{r}.out.b"] = f32(sd[s + "out_conv.bias"])
        for u in ((1, 2) if r < 4 or rf4_unit1 else (2,)):
            for c in (1, 2):
                o[f"rf{r}.rcu{u}.c{c}{w}"] = _conv3(sd[f"{s}resConfUnit{u}.conv{c}.weight"], dtype)
                o[f"rf{r}.rcu{u}.c{c}.b"] = f32(sd[f"{s}resConfUnit{u}.conv{c}.bias"])
    s = h + "scratch."
    o["head.c1" + w] = _conv3(sd[s + "output_conv1.weight"], dtype)
    o["head.c1.b"] = f32(sd[s + "output_conv1.bias"])
    o["head.c2" + w] = _conv3(sd[s + "output_conv2.0.weight"], dtype)
    o["head.c2.b"] = f32(sd[s + "output_conv2.0.bias"])
    if pe is not None:
        o["head.pe"] = pe[1]
    rows = slice(0, 1) if depth_only else slice(None)
    o["head.c3.w"] = f32(sd[s + "output_conv2.2.weight"][rows])
    o["head.c3.b"] = f32(sd[s + "output_conv2.2.bias"][rows])


def packed_tensors(sd: Dict[str, np.ndarray], cfg: dict, img_h: int, img_w: int,
                   fold_ln: bool = False, enc_f32: bool = False) -> "OrderedDict[str, np.ndarray]":
    """The packed tensors (name -> f16/f32 numpy array) for one input size.
    fold_ln (precision "fp16" engines) adds the LayerNorm-folded qkv / fc1 /
    DPT project weights (`*.wf`, `*.c1`, `*.c2`) and the cls row's partials
    (`pos.cls.st`).  enc_f32 (precision "fp32" engines) stores every conv /
    linear weight as fp32 (`*.w32`) in place of f16: the exact-fp32 encoder
    and the head run on fp32 maps (engine.hip dav2_head32)."""
    sd = normalize_keys(sd)
    check_keys(sd, W.expected_keys(cfg))
    P = cfg["patch"]
    if img_h % P or img_w % P:
        raise ValueError(f"input size {img_h}x{img_w} is not a multiple of the patch size {P}")
    ph, pw = img_h // P, img_w // P
    D = cfg["embed_dim"]
    dtype = np.float32 if enc_f32 else np.float16
    o: "OrderedDict[str, np.ndarray]" = OrderedDict()
    p = "pretrained."
    pe16 = np.zeros((D, 3, 14, 16), np.float32)
    pe16[..., :14] = sd[p + "patch_embed.proj.weight"]      # [D,3,14,14]
    o["patch.w32" if enc_f32 else "patch.w"] = _pad2(pe16.reshape(D, 3 * 14 * 16), dtype)
    o["patch.b"] = f32(sd[p + "patch_embed.proj.bias"])
    pos = interpolate_pos_embed(sd[p + "pos_embed"], ph, pw)
    o["pos.patch"] = np.ascontiguousarray(pos[0, 1:], dtype=np.float32)
    o["pos.cls"] = f32(sd[p + "cls_token"].reshape(-1) + pos[0, 0])
    if fold_ln and D % 32 == 0:
        o["pos.cls.st"] = _slice_partials(o["pos.cls"])
    for i in range(cfg["depth"]):
        pack_block(o, sd, f"{p}blocks.{i}.", f"b{i}.", fold_ln=fold_ln, dtype=dtype)
    o["norm.g"] = f32(sd[p + "norm.weight"])
    o["norm.b"] = f32(sd[p + "norm.bias"])
    fold = fold_ln and not enc_f32
    pack_dpt_head(o, sd, cfg, dtype, fold_norm=(sd[p + "norm.weight"], sd[p + "norm.bias"]) if fold else None)
    return o


INPUT_FORMATS = ("float32_nchw", "uint8_nhwc")
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


PRECISIONS = ("fp16", "fp32")

# PackConfig (csrc/pack_format.h) in struct order: (field, struct format); `reserved` pads it to 256 bytes
_CONFIG_FIELDS = (
    ("embed_dim", "i"), ("depth", "i"), ("num_heads", "i"), ("mlp_hidden", "i"), ("patch", "i"),
    ("img_h", "i"), ("img_w", "i"), ("features", "i"), ("out_channels", "4i"), ("taps", "4i"),
    ("head_hidden", "i"), ("metric", "i"), ("max_depth", "f"), ("ln_eps", "f"), ("encoder", "16s"),
    ("input_u8", "i"), ("in_scale", "f"), ("in_mean", "3f"), ("in_std", "3f"),
    ("family", "i"), ("vit_size", "i"), ("merge_pad", "i"), ("use_fov", "i"), ("fov_layers", "i"), ("fov_k", "i"),
    ("hooks", "2i"), ("inter_dims", "2i"), ("scaled_dims", "3i"),
    ("frames", "i"), ("npre", "i"), ("aa_depth", "i"), ("agg_eps", "f"), ("resid_f16", "i"), ("enc_f32", "i"))
_CONFIG_STRUCT = struct.Struct("<" + "".join(fmt for _, fmt in _CONFIG_FIELDS))
assert _CONFIG_STRUCT.size == 256 - 52, _CONFIG_STRUCT.size     # sizeof(PackConfig) - sizeof(reserved)


def pack_config(cfg: dict, **fields) -> bytes:
    """The 256 PackConfig bytes: the ViT geometry every family stores
    (embed_dim, depth, num_heads, mlp_hidden, patch, head_hidden, ln_eps,
    encoder) from cfg, the other fields by name; what is not named is zero."""
    fields.update({k: cfg[k] for k in ("embed_dim", "depth", "num_heads", "mlp_hidden", "patch", "head_hidden",
                                       "ln_eps")}, encoder=cfg["encoder"].encode()[:15])
    vals = []
    for name, fmt in _CONFIG_FIELDS:
        v = fields.pop(name, None)
        if len(fmt) == 1 or fmt[-1] == "s":
            vals.append(v if v is not None else (b"" if fmt[-1] == "s" else 0))
        else:
            v = list(v) if v is not None else [0] * int(fmt[:-1])
            assert len(v) == int(fmt[:-1]), (name, v)
            vals += v
    if fields:
        raise TypeError(f"no PackConfig field named {sorted(fields)}")
    return _CONFIG_STRUCT.pack(*vals) + b"\0" * 52


def _config_bytes(cfg: dict, img_h: int, img_w: int, input_format: str = "float32_nchw",
                  mean=IMAGENET_MEAN, std=IMAGENET_STD, scale: float = 255.0, precision: str = "fp16") -> bytes:
    """PackConfig (csrc/pack_format.h).  input_format "uint8_nhwc" stores the
    preamble constants of the reference's add_uint8_input
    (core/onnx_tools.py:87-219): ((u8 / scale) - mean) / std, fp32.
    precision "fp16" keeps the residual stream in f16 (resid_f16 = 1, the
    reference's fp16 TensorRT engine); "fp32" (the reference's default) runs
    the encoder exactly in fp32 (enc_f32 = 1: fp32 weights, activations and
    MFMA, csrc/fp32.hip)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    if input_format not in INPUT_FORMATS:
        raise ValueError(f"input_format must be one of {INPUT_FORMATS}, got {input_format!r}")
    u8 = input_format == "uint8_nhwc"
    if u8 and (len(mean) != 3 or len(std) != 3 or float(scale) == 0.0 or any(float(v) == 0.0 for v in std)):
        raise ValueError("uint8 preamble needs 3 means, 3 non-zero stds and a non-zero scale")
    pre = dict(input_u8=1, in_scale=float(scale), in_mean=[float(v) for v in mean],
               in_std=[float(v) for v in std]) if u8 else {}
    return pack_config(cfg, img_h=img_h, img_w=img_w, features=cfg["features"], out_channels=cfg["out_channels"],
                       taps=cfg["taps"], metric=1 if cfg["depth_type"] == "metric" else 0,
                       max_depth=float(cfg["max_depth"]), resid_f16=1 if precision == "fp16" else 0,
                       enc_f32=1 if precision == "fp32" else 0, **pre)


def container(tens: "OrderedDict[str, np.ndarray]", cfg_bytes: bytes) -> bytes:
    """Header + PackConfig + tensor table + 256-byte aligned data."""
    assert len(cfg_bytes) == 256, len(cfg_bytes)
    n = len(tens)
    table = bytearray()
    data = bytearray()
    for name, a in tens.items():
        a = np.ascontiguousarray(a)
        dtype = {np.dtype(np.float32): 0, np.dtype(np.float16): 1}[a.dtype]
        if len(name) >= 80:
            raise ValueError(f"tensor name too long: {name}")
        dims = list(a.shape) + [0] * (4 - a.ndim)
        off = len(data)
        raw = a.tobytes()
        data += raw
        data += b"\0" * ((-len(data)) % ALIGN)
        table += struct.pack("<80sii4iQQ8s", name.encode(), dtype, a.ndim, *dims, off, len(raw), b"")
    head_len = 32 + 256 + len(table)
    data_offset = -(-head_len // ALIGN) * ALIGN
    header = struct.pack("<8sIIQQ", b"MDEPACK1", PACK_VERSION, n, data_offset, len(data))
    blob = header + cfg_bytes + bytes(table)
    blob += b"\0" * (data_offset - len(blob))
    return blob + bytes(data)


def pack_bytes(sd: Dict[str, np.ndarray], cfg: dict, img_h: int = 518, img_w: int = 518,
               input_format: str = "float32_nchw", precision: str = "fp16") -> bytes:
    return container(packed_tensors(sd, cfg, img_h, img_w, fold_ln=precision == "fp16", enc_f32=precision == "fp32"),
                     _config_bytes(cfg, img_h, img_w, input_format, precision=precision))


def write_packed(path: str, blob: bytes) -> str:
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(blob)
    os.replace(tmp, path)
    return path


def synthetic_blob(encoder: str = "vits", depth_type: str = "metric", img_h: int = 518, img_w: int = 518,
                   seed: int = 1234, input_format: str = "float32_nchw") -> Tuple[bytes, dict]:
    cfg = W.model_config(encoder, depth_type)
    sd = W.synthetic_state_dict(cfg, seed)
    return pack_bytes(sd, cfg, img_h, img_w, input_format), cfg


def fingerprint(blob: bytes, arch: str = "gfx950") -> str:
    return "\n".join([hashlib.sha256(blob).hexdigest(), f"packer={PACKER_VERSION}", f"arch={arch}"])
