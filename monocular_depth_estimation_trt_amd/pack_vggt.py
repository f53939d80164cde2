"""AOT weight packer for VGGT's depth path: upstream-keyed state dict ->
packed engine (family 2).

Replaces the reference's `models/vggt/onnx_export.py:78-131` (ONNX export of
`VGGTDepthOnlyWrapper` at 518x518 under fp16 autocast, with the export
patches of `core/export_compat.py`) and the TensorRT build of
`models/vggt/onnx2trt.py` for this model.  Same container as pack.py
(csrc/pack_format.h); what is folded at pack time:

* the aggregator's ImageNet normalisation into the patch-embed weights
  (W' = W / std_c, b' = b - sum W mean_c / std_c: the 14x14 stride-14 conv
  has no padding, so the fold is exact) -- the engine reads the [0, 1] images;
* cls + pos[0] and the 4 DINOv2 register tokens -> "pre.dino" [5][D]; the
  aggregator's camera + register tokens -> "pre.agg" [2][5][D] (set 0 =
  first frame of each batch item, set 1 = the others);
* the 2D RoPE tables cos/sin [max(gh, gw) + 2][16] (base 100, 32 features
  per axis, upstream _compute_frequency_components in fp32);
* the DPT head's UV sin/cos embeddings (ratio 0.1): after each 1x1
  projection as an f16 [np][oc_i] table the projection epilogue adds, and
  -- because output_conv2's first 3x3 conv is linear and zero-padded --
  the full-resolution one as conv(pe) without bias, an f16 [H*W][32] table
  the head epilogue adds before its ReLU (exact in real arithmetic,
  computed in float64);
* output_conv2's last 1x1 conv reduced to its depth channel (channel 1 is
  the confidence the wrapper drops, onnx_export.py:49-52).

A packed file is specific to one input size and one frame count S (the
global-attention length S * 1374 at 518^2), as the reference's engine is to
its static [1, S, 3, 518, 518] profile.
"""

from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np

from . import pack as PK
from . import weights_vggt as WV
from .pack import f32

FAMILY_VGGT = 2
NPRE = 1 + WV.NUM_REG      # camera + 4 register tokens ahead of the patch tokens


# ---- tables -----------------------------------------------------------------
def uv_grid(width: int, height: int, aspect: float) -> np.ndarray:
    """upstream heads/utils.create_uv_grid -> [height*width, 2] (u, v), float64."""
    diag = (aspect ** 2 + 1.0) ** 0.5
    sx, sy = aspect / diag, 1.0 / diag
    xs = np.linspace(-sx * (width - 1) / width, sx * (width - 1) / width, width)
    ys = np.linspace(-sy * (height - 1) / height, sy * (height - 1) / height, height)
    uu, vv = np.meshgrid(xs, ys, indexing="xy")
    return np.stack([uu.reshape(-1), vv.reshape(-1)], -1)


def _sincos(dim: int, pos: np.ndarray, omega_0: float) -> np.ndarray:
    omega = np.arange(dim // 2, dtype=np.float64) / (dim / 2.0)
    omega = 1.0 / omega_0 ** omega
    out = pos[:, None] * omega[None, :]
    return np.concatenate([np.sin(out), np.cos(out)], 1)


def uv_embed(channels: int, h: int, w: int, aspect: float, ratio: float = 0.1, omega_0: float = 100.0) -> np.ndarray:
    """ratio * position_grid_to_embed(create_uv_grid(w, h, aspect), C) -> [h*w, C] float64
    (token-major: row = y*w + x)."""
    g = uv_grid(w, h, aspect)
    return ratio * np.concatenate([_sincos(channels // 2, g[:, 0], omega_0),
                                   _sincos(channels // 2, g[:, 1], omega_0)], 1)


def rope_tables(npos: int, dim: int = 32, base: float = 100.0) -> Tuple[np.ndarray, np.ndarray]:
    """cos/sin [npos][dim/2] fp32: angle(p, j) = p * base^-(2j/dim), the
    non-duplicated half of upstream _compute_frequency_components (fp32)."""
    exps = (np.arange(0, dim, 2, dtype=np.float32) / np.float32(dim)).astype(np.float32)
    inv = (np.float32(1.0) / (np.float32(base) ** exps)).astype(np.float32)
    ang = (np.arange(npos, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def fold_patch_embed(w: np.ndarray, b: np.ndarray, mean=WV.RESNET_MEAN, std=WV.RESNET_STD):
    """Patch-embed conv over (x - mean) / std == conv with W' = W / std, b' =
    b - sum W mean / std (float64, returned float32)."""
    w64 = w.astype(np.float64)
    m = np.asarray(mean, np.float64)[None, :, None, None]
    s = np.asarray(std, np.float64)[None, :, None, None]
    wf = w64 / s
    bf = b.astype(np.float64) - (w64 * m / s).sum(axis=(1, 2, 3))
    return wf.astype(np.float32), bf.astype(np.float32)


def head_pe(w_conv: np.ndarray, h: int, w: int, ratio: float = 0.1, omega_0: float = 100.0) -> np.ndarray:
    """conv3x3(pad 1, no bias) of the full-resolution embedding through
    output_conv2.0 -> [h*w, Cout] float64."""
    import torch
    import torch.nn.functional as F
    cin = w_conv.shape[1]
    pe = uv_embed(cin, h, w, float(w) / float(h), ratio, omega_0).T.reshape(1, cin, h, w)
    with torch.no_grad():
        y = F.conv2d(torch.from_numpy(np.ascontiguousarray(pe)), torch.from_numpy(w_conv.astype(np.float64)),
                     padding=1)
    return y[0].reshape(w_conv.shape[0], h * w).T.numpy()


# ---- packing ----------------------------------------------------------------
def packed_tensors(sd: Dict[str, np.ndarray], cfg: dict) -> "OrderedDict[str, np.ndarray]":
    sd = PK.normalize_keys(sd)
    PK.check_keys(sd, WV.expected_keys(cfg), "VGGT")
    D, P, S = cfg["embed_dim"], cfg["patch"], cfg["img"]
    g = S // P
    np_ = g * g
    oc = cfg["out_channels"]
    o: "OrderedDict[str, np.ndarray]" = OrderedDict()
    p = "aggregator.patch_embed."
    pw, pb = fold_patch_embed(sd[p + "patch_embed.proj.weight"], sd[p + "patch_embed.proj.bias"])
    pe16 = np.zeros((D, 3, P, 16), np.float32)
    pe16[..., :P] = pw
    o["patch.w"] = PK._pad2(pe16.reshape(D, 3 * P * 16))
    o["patch.b"] = f32(pb)
    pos = sd[p + "pos_embed"]
    if pos.shape[1] != 1 + np_:
        raise ValueError(f"pos_embed holds {pos.shape[1] - 1} positions; the packed size {S} needs {np_} "
                         "(pack at the checkpoint's 518x518 grid)")
    o["pos.patch"] = np.ascontiguousarray(pos[0, 1:], dtype=np.float32)
    o["pre.dino"] = np.ascontiguousarray(np.concatenate(
        [sd[p + "cls_token"].reshape(1, D) + pos[0, :1], sd[p + "register_tokens"].reshape(WV.NUM_REG, D)], 0),
        dtype=np.float32)
    for i in range(cfg["depth"]):
        PK.pack_block(o, sd, f"{p}blocks.{i}.", f"db{i}.")
    o["norm.g"] = f32(sd[p + "norm.weight"])
    o["norm.b"] = f32(sd[p + "norm.bias"])
    a = "aggregator."
    cam = sd[a + "camera_token"].reshape(2, 1, D)
    reg = sd[a + "register_token"].reshape(2, WV.NUM_REG, D)
    o["pre.agg"] = np.ascontiguousarray(np.concatenate([cam, reg], 1), dtype=np.float32)   # [2][5][D]
    for i in range(cfg["aa_depth"]):
        PK.pack_block(o, sd, f"{a}frame_blocks.{i}.", f"fb{i}.", qk_norm=True)
        PK.pack_block(o, sd, f"{a}global_blocks.{i}.", f"gb{i}.", qk_norm=True)
    cos, sin = rope_tables(g + 2, 32, cfg["rope_freq"])
    o["rope.cos"] = cos
    o["rope.sin"] = sin
    h = "depth_head."
    o["dh.norm.g"] = f32(sd[h + "norm.weight"])
    o["dh.norm.b"] = f32(sd[h + "norm.bias"])
    pe = [uv_embed(oc[i], g, g, 1.0, cfg["pe_ratio"], cfg["pe_omega"]).astype(np.float16) for i in range(4)]
    pe_head = head_pe(sd[h + "scratch.output_conv2.0.weight"], S, S, cfg["pe_ratio"], cfg["pe_omega"])
    PK.pack_dpt_head(o, sd, cfg, pe=(pe, pe_head.astype(np.float16)), rf4_unit1=False, depth_only=True)
    return o


def config_bytes(cfg: dict, frames: int) -> bytes:
    """PackConfig (csrc/pack_format.h) with family = 2: the DA-V2 fields carry
    the DINOv2 geometry (depth = DINOv2 blocks, ln_eps its eps, metric = 2:
    exp head), then the family block (zeros but family) and the VGGT fields
    (frames, special tokens, aggregator depth, aggregator LayerNorm eps)."""
    if frames < 1:
        raise ValueError(f"frames must be >= 1, got {frames}")
    return PK.pack_config(cfg, img_h=cfg["img"], img_w=cfg["img"], features=cfg["features"],
                          out_channels=cfg["out_channels"], taps=cfg["taps"], metric=2, family=FAMILY_VGGT,
                          frames=int(frames), npre=NPRE, aa_depth=cfg["aa_depth"], agg_eps=float(cfg["agg_eps"]))


def pack_bytes(sd: Dict[str, np.ndarray], cfg: dict, frames: int = 1) -> bytes:
    return PK.container(packed_tensors(sd, cfg), config_bytes(cfg, frames))


def synthetic_blob(preset: str = "vggt_1b", frames: int = 1, seed: int = 2468):
    cfg = WV.vggt_config(preset)
    return pack_bytes(WV.synthetic_state_dict(cfg, seed), cfg, frames), cfg
