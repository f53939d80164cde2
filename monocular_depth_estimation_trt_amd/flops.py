"""Algorithmic work of the DA-V2 forward, per layer (2 FLOP per MAC).

Counts the REFERENCE graph (upstream DepthAnythingV2 / the TensorRT engine
of SURVEY.md 2.3), not what the HIP schedule happens to execute: e.g. the
fusion out_conv is counted at the post-resize resolution even though the
engine runs it before the resize (4x fewer MACs, exact by linearity).  These
are the numbers roofline fractions are quoted against (ViT-S
115.27 GFLOP/img, ViT-L 1304.22 GFLOP/img at 518^2).

Omission: where the engine runs a fusion block's out_conv inside rcu2's second
conv (switch "outconv_fold" on a persistent-conv grid: no rfN.out step), the
1x1's work is still listed under rfN.out, not under rfN.rcu2.c2 -- whether
the fold is active depends on the library's dispatch switches as well as on
the grid, and layer_flops() takes neither.  The totals are unaffected; a
per-layer table of such a run shows rfN.rcu2.c2 without the 1x1's FLOPs and
no rfN.out row.

Layer names match the engine's profiler names (csrc/engine.hip: Runner::forward_dav2 and the
shared vit_block / dpt_* steps; pinned by tests/golden/layer_schedule.json).
"""

from __future__ import annotations

from collections import OrderedDict
from typing import Dict


def block_flops(o, pfx: str, seqs: int, L: int, D: int, M4: int) -> None:
    """One ViT block over `seqs` sequences of `L` tokens, as `pfx`.qkv/.attn/.proj/.fc1/.fc2."""
    o[pfx + ".qkv"] = 2.0 * seqs * L * 3 * D * D
    o[pfx + ".attn"] = 4.0 * seqs * L * L * D
    o[pfx + ".proj"] = 2.0 * seqs * L * D * D
    o[pfx + ".fc1"] = 2.0 * seqs * L * M4 * D
    o[pfx + ".fc2"] = 2.0 * seqs * L * D * M4


def dpt_flops(o, cfg: dict, ph: int, pw: int, img_px: int, n: int, in_dim: int, out_dim: int = 1) -> None:
    """The DPT decoder (reassemble, layerN_rn, refinenets, head) on `n` frames
    of a ph x pw token grid: projections from `in_dim` channels, the head at
    `img_px` pixels with `out_dim` 1x1 outputs."""
    F, oc = cfg["features"], cfg["out_channels"]
    npch = ph * pw
    s = [(4 * ph) * (4 * pw), (2 * ph) * (2 * pw), npch, ((ph + 1) // 2) * ((pw + 1) // 2)]
    for i in range(4):
        o[f"reassemble{i}.project"] = 2.0 * n * npch * in_dim * oc[i]
    o["reassemble0.convT4"] = 2.0 * n * npch * oc[0] * oc[0] * 16
    o["reassemble1.convT2"] = 2.0 * n * npch * oc[1] * oc[1] * 4
    o["reassemble3.conv_s2"] = 2.0 * n * s[3] * oc[3] * oc[3] * 9
    for i in range(4):
        o[f"layer{i + 1}_rn"] = 2.0 * n * s[i] * F * oc[i] * 9
    # refinenet r works at scale index r-1; out_conv after the resize
    target = {4: s[2], 3: s[1], 2: s[0], 1: 4 * s[0]}
    for r in (4, 3, 2, 1):
        for u in ((2,) if r == 4 else (1, 2)):
            o[f"rf{r}.rcu{u}.c1"] = 2.0 * n * s[r - 1] * F * F * 9
            o[f"rf{r}.rcu{u}.c2"] = 2.0 * n * s[r - 1] * F * F * 9
        o[f"rf{r}.out"] = 2.0 * n * target[r] * F * F
    o["head.output_conv1"] = 2.0 * n * (8 * ph) * (8 * pw) * (F // 2) * F * 9
    o["head.output_conv2"] = 2.0 * n * img_px * (cfg["head_hidden"] * (F // 2) * 9 + cfg["head_hidden"] * out_dim)


def layer_flops(cfg: dict, img_h: int = 518, img_w: int = 518, batch: int = 1) -> "OrderedDict[str, float]":
    P, D = cfg["patch"], cfg["embed_dim"]
    ph, pw = img_h // P, img_w // P
    o: "OrderedDict[str, float]" = OrderedDict()
    o["patch_embed"] = 2.0 * batch * ph * pw * D * 3 * P * P
    for i in range(cfg["depth"]):
        block_flops(o, f"block{i}", batch, ph * pw + 1, D, cfg["mlp_hidden"])
    dpt_flops(o, cfg, ph, pw, img_h * img_w, batch, D)
    return o


def total_flops(cfg: dict, img_h: int = 518, img_w: int = 518, batch: int = 1) -> float:
    return float(sum(layer_flops(cfg, img_h, img_w, batch).values()))


def layer_class(name: str) -> str:
    """'block7.fc1' -> 'fc1'; 'rf3.rcu1.c2' -> 'rcu.conv'; others unchanged."""
    if name.startswith("block"):
        return name.split(".", 1)[1]
    if name.startswith("rf") and ".rcu" in name:
        return "rcu.conv"
    if name.startswith("rf") and name.endswith(".out"):
        return "fusion.out_conv"
    if name.startswith("rf") and name.endswith(".resize"):
        return "fusion.resize"
    if name.startswith("tap"):
        return "tap.norm"
    if name.startswith("layer") and name.endswith("_rn"):
        return "layer_rn"
    if name.startswith("reassemble") and name.endswith(".project"):
        return "reassemble.project"
    return name


def sum_classes(layers: Dict[str, float], layer_class) -> Dict[str, float]:
    """A layer_flops table summed per layer_class, in first-seen order."""
    out: Dict[str, float] = {}
    for k, v in layers.items():
        c = layer_class(k)
        out[c] = out.get(c, 0.0) + v
    return out


def class_flops(cfg: dict, img_h: int = 518, img_w: int = 518, batch: int = 1) -> Dict[str, float]:
    return sum_classes(layer_flops(cfg, img_h, img_w, batch), layer_class)
