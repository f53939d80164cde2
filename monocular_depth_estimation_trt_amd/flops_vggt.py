"""Algorithmic work of the VGGT depth path, per layer (2 FLOP per MAC).

Counts the REFERENCE graph (`VGGTDepthOnlyWrapper`, models/vggt/onnx_export.py:
38-52: aggregator + depth head), not what the HIP schedule executes: the
fusion out_conv is counted after the resize although the engine runs it
before (exact by linearity), output_conv2's 1x1 is counted with both of its
output channels although the engine computes only the depth channel, and the
UV embedding convolution the packer folds into a table is not counted at all
(it is input-independent).  Global attention is counted over the whole
S * T sequence of each batch item.

Layer names match the engine's profiler names (csrc/vggt.hip Runner::forward_vggt; the
block and DPT decoder steps it shares with DA-V2 are in csrc/engine.hip).
"""

from __future__ import annotations

import re
from collections import OrderedDict
from typing import Dict

from .flops import block_flops, dpt_flops, sum_classes
from .flops import layer_class as dav2_class

NPRE = 5   # camera + 4 register tokens (aggregator); cls + 4 registers (DINOv2)


def layer_flops(cfg: dict, batch: int = 1, frames: int = 1) -> "OrderedDict[str, float]":
    P, D, M4 = cfg["patch"], cfg["embed_dim"], cfg["mlp_hidden"]
    g = cfg["img"] // P
    T = g * g + NPRE
    n = batch * frames                      # frames in the batch
    o: "OrderedDict[str, float]" = OrderedDict()
    o["patch_embed"] = 2.0 * n * g * g * D * 3 * P * P
    for i in range(cfg["depth"]):
        block_flops(o, f"db{i}", n, T, D, M4)
    for i in range(cfg["aa_depth"]):
        block_flops(o, f"fb{i}", n, T, D, M4)
        block_flops(o, f"gb{i}", batch, frames * T, D, M4)
    dpt_flops(o, cfg, g, g, cfg["img"] ** 2, n, 2 * D, out_dim=2)
    return o


def total_flops(cfg: dict, batch: int = 1, frames: int = 1) -> float:
    return float(sum(layer_flops(cfg, batch, frames).values()))


_BLK = re.compile(r"^(db|fb|gb)\d+\.(.+)$")


def layer_class(name: str) -> str:
    """'gb7.attn' -> 'gb.attn'; 'rf3.rcu1.c2' -> 'rcu.conv'; others as flops.layer_class."""
    m = _BLK.match(name)
    if m:
        return f"{m.group(1)}.{m.group(2)}"
    return dav2_class(name)


def class_flops(cfg: dict, batch: int = 1, frames: int = 1) -> Dict[str, float]:
    return sum_classes(layer_flops(cfg, batch, frames), layer_class)
