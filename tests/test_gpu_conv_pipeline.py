"""The persistent 64-channel RCU conv (conv.hip conv64p_kernel) with the next
patch's DMA in flight under the epilogue (MODE 0 and 3: counted wait behind
the row stores, rows outside the map stored to a sink line, the input ReLU on
the wave's own landed rows) and with the waves that have no valid output row
skipping the tap loop and the epilogue (every MODE): bit for bit against the
per-tile kernel (conv_persist = 0).  And the fusion blocks' 1x1 out_conv run
inside rcu2's second conv (switch "outconv_fold"): the engine forward bit for
bit against the switch off, and the ".out" step gone exactly where the
persistent conv takes that conv.

Shapes, each >= 1024 tiles of 16 x 16 (the persistent kernel's threshold):
  B = 12, 148 x 148  bottom tile row with 4 valid rows (waves 0-1 work), 4 valid columns
  B =  9, 177 x 161  bottom tile row with 1 valid row (wave 0 alone, half of it), 1 valid column
  B =  8, 176 x 192  no partial tile, no idle wave
"""

import numpy as np
import pytest
import torch

from gpu_util import conv_w, depth_metrics, nhwc, op, ptr, stream
from monocular_depth_estimation_trt_amd import _lib, pack, weights
from monocular_depth_estimation_trt_amd.engine import Engine

pytestmark = pytest.mark.gpu

SHAPES = [(12, 148, 148), (9, 177, 161), (8, 176, 192)]
# (relu_in, act, nres): MODE 0 (conv1), 1, 2 (conv2 with one / two residuals), 3 (plain)
MODES = [(1, 1, 0), (0, 0, 1), (0, 0, 2), (0, 0, 0)]


@pytest.mark.parametrize("relu_in,act,nres", MODES)
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_conv_pipeline_bit_exact(gpu, B, h, w, relu_in, act, nres):
    g = torch.Generator().manual_seed(1000 * h + 10 * w + 4 * relu_in + nres)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    x = rn(B, 64, h, w)
    wt, b = rn(64, 64, 3, 3, scale=(9 * 64) ** -0.5), rn(64, scale=0.02)
    wp = conv_w(wt).to(gpu)
    rg = [nhwc(rn(B, 64, h, w)).half().to(gpu) for _ in range(nres)] + [None, None]
    xg, bg = nhwc(x).half().to(gpu), b.to(gpu)
    assert B * ((h + 15) // 16) * ((w + 15) // 16) >= 1024, "the persistent kernel must take this grid"

    def run(flag, fill):
        # (a row the kernel does not write keeps the fill, which differs per run)
        out = torch.full((B, h, w, 64), fill, dtype=torch.float16, device=gpu)
        with _lib.tuning(conv_persist=flag):
            op("mde_op_conv3x3", ptr(xg), B, h, w, 64, ptr(wp), wp.shape[1], 64, 1, relu_in, ptr(bg), act,
               ptr(rg[0]), ptr(rg[1]), ptr(out), stream())
        torch.cuda.synchronize()
        return out

    ref = run(0, 1001.0)
    got = run(1, 2002.0)
    again = run(1, 3003.0)
    got8 = run(2, 4004.0)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) < 100.0
    assert torch.equal(got, ref), "persistent conv (16 x 16 tiles) differs from the per-tile kernel"
    assert torch.equal(again, ref), "persistent conv (16 x 16 tiles): second run differs"
    assert torch.equal(got8, ref), "persistent conv (8 x 16 tiles) differs from the per-tile kernel"


class _Names:
    def __init__(self):
        self.names = []

    def report_layer_time(self, name, ms):
        self.names.append(name)


def _forward_with_steps(blob, x):
    """One eager forward with the profiler attached: (depth map, step names)."""
    prof = _Names()
    out = torch.full((x.shape[0],) + x.shape[2:], float("nan"), device="cuda")
    with Engine.from_bytes(blob, 0, profile=((1,) + x.shape[1:], x.shape, x.shape)) as eng:
        with eng.create_execution_context() as ctx:
            ctx.set_graph_mode(False)
            xin = torch.from_numpy(x).cuda()
            ctx.set_input_shape("input", x.shape)
            ctx.set_tensor_address("input", xin.data_ptr())
            ctx.set_tensor_address("output", out.data_ptr())
            ctx.profiler = prof
            ctx.execute_async_v3(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ctx.profiler = None
    return out.cpu().numpy(), prof.names


# ViT-S 518^2: the fusion blocks run at 148^2 (rf1), 74^2 (rf2), 37^2 and 19^2;
# the persistent conv takes grids of >= 1024 16 x 16 tiles.  B = 12: 1200 tiles
# at 148^2, 300 at 74^2 -- rf1 folds, rf2 keeps its GEMM.  B = 41 is the
# smallest batch whose 74^2 grid (25 tiles per image) reaches 1024: rf1 and
# rf2 fold.  rf3 and rf4 never do.
@pytest.mark.parametrize("B,folded", [(12, ("rf1",)), (41, ("rf1", "rf2"))])
def test_outconv_fold_bit_exact(gpu, B, folded):
    cfg = weights.model_config("vits", "metric")
    sd = weights.synthetic_state_dict(cfg, 77)
    blob = pack.pack_bytes(sd, cfg, 518, 518)
    x = np.ascontiguousarray(weights.synthetic_images(B, 518, 518, first_seed=31))
    with _lib.tuning(outconv_fold=1):
        y_on, steps_on = _forward_with_steps(blob, x)
    with _lib.tuning(outconv_fold=0):
        y_off, steps_off = _forward_with_steps(blob, x)
    assert np.isfinite(y_on).all()
    assert np.array_equal(y_on, y_off), depth_metrics(y_on, y_off)
    for r in ("rf1", "rf2", "rf3", "rf4"):
        assert (r + ".out") in steps_off, (r, "switch off: the 1x1 is a launch")
        assert ((r + ".out") in steps_on) == (r not in folded), (r, B, "switch on")
        assert (r + ".rcu2.c2") in steps_on and (r + ".rcu2.c2") in steps_off
    assert [s for s in steps_on if not s.endswith(".out")] == [s for s in steps_off if not s.endswith(".out")]
