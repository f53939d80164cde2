"""The forward-schedule cases of tests/test_gpu_schedule.py and
tests/golden/make_layer_schedule.py: the smallest synthetic engines that take
each branch of the three families' schedules, run once eagerly with a
profiler attached.

run(name) -> (profiler step names in launch order, {output name: array},
workspace bytes of the context).
"""

from __future__ import annotations

import contextlib

import numpy as np
import torch

from monocular_depth_estimation_trt_amd import _lib, pack, pack_depth_pro, pack_vggt, weights
from monocular_depth_estimation_trt_amd import weights_depth_pro as WD, weights_vggt as WV
from monocular_depth_estimation_trt_amd.engine import Engine

# name -> (family, options).  DA-V2 options: depth_type, size, batch,
# max_batch, precision, input_format, tuning switches (set before the context
# is created: the arena reads "lnfold").
CASES = {
    # fold + tap fold, fc2 split-K active (B*T = 50 rows, K = 1536)
    "dav2_vits_metric_98_b1": ("dav2", {}),
    "dav2_vits_metric_98_b1_lnfold0": ("dav2", dict(tuning=dict(lnfold=0))),
    "dav2_vits_metric_98_b1_splitk0": ("dav2", dict(tuning=dict(splitk=0))),
    "dav2_vits_metric_98_b1_resize_fold0": ("dav2", dict(tuning=dict(resize_fold=0))),
    "dav2_vits_metric_98_b1_u8": ("dav2", dict(input_format="uint8_nhwc")),
    "dav2_vits_relative_98_b2": ("dav2", dict(depth_type="relative", batch=2)),
    "dav2_vits_metric_98_b1_fp32": ("dav2", dict(precision="fp32")),
    # B*T = 4110 > 4096: the context has no fc2 split-K workspace
    "dav2_vits_metric_518_b3": ("dav2", dict(size=518, batch=3)),
    "depth_pro_tiny_b1": ("depth_pro", dict(batch=1)),
    "vggt_tiny_b2_s1": ("vggt", dict(batch=2, frames=1)),
    "vggt_tiny_b1_s2": ("vggt", dict(batch=1, frames=2)),
}


class _Names:
    def __init__(self):
        self.names = []

    def report_layer_time(self, name, ms):
        self.names.append(name)


def _dav2(depth_type="metric", size=98, batch=1, precision="fp16", input_format="float32_nchw", tuning=None):
    cfg = weights.model_config("vits", depth_type)
    sd = weights.synthetic_state_dict(cfg, 1234)
    blob = pack.pack_bytes(sd, cfg, size, size, input_format=input_format, precision=precision)
    if input_format == "uint8_nhwc":
        x = weights.synthetic_images_u8(batch, size, size, first_seed=5)
    else:
        x = weights.synthetic_images(batch, size, size, first_seed=3)
    out = torch.full((batch, size, size), float("nan"), device="cuda")
    return blob, x, {"output": out}, tuning or {}


def _depth_pro(batch=1):
    cfg = WD.depth_pro_config("tiny")
    sd = WD.synthetic_state_dict(cfg, 4321)
    x = WD.synthetic_images(batch, cfg["img"], first_seed=200)
    out = torch.full((batch, 1, cfg["img"], cfg["img"]), float("nan"), device="cuda")
    fov = torch.full((batch,), float("nan"), device="cuda")
    return pack_depth_pro.pack_bytes(sd, cfg), x, {"canonical_inverse_depth": out, "fov_deg": fov}, {}


def _vggt(batch=1, frames=1):
    cfg = WV.vggt_config("tiny")
    sd = WV.synthetic_state_dict(cfg, 2468)
    x = WV.synthetic_images(batch, frames, cfg["img"], first_seed=300)
    out = torch.full(x.shape[:2] + x.shape[3:] + (1,), float("nan"), device="cuda")
    return pack_vggt.pack_bytes(sd, cfg, frames), x, {"depth": out}, {}


def run(name: str):
    family, opts = CASES[name]
    blob, x, outs, switches = {"dav2": _dav2, "depth_pro": _depth_pro, "vggt": _vggt}[family](**opts)
    x = np.ascontiguousarray(x)
    shape1 = (1,) + x.shape[1:]
    prof = _Names()
    with Engine.from_bytes(blob, 0, profile=(shape1, x.shape, x.shape)) as eng:
        with (_lib.tuning(**switches) if switches else contextlib.nullcontext()):
            with eng.create_execution_context() as ctx:
                ctx.set_graph_mode(False)
                xin = torch.from_numpy(x).cuda()
                ctx.set_input_shape(eng.input_name, x.shape)
                ctx.set_tensor_address(eng.input_name, xin.data_ptr())
                for n, t in outs.items():
                    ctx.set_tensor_address(n, t.data_ptr())
                ctx.profiler = prof
                ctx.execute_async_v3(torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                ctx.profiler = None
                nbytes = ctx.workspace_bytes
    return prof.names, {n: t.cpu().numpy() for n, t in outs.items()}, nbytes
