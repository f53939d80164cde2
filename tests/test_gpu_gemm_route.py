"""One small launch per row of launch_gemm's tile table (csrc/gemm.hip kTiles,
DESIGN.md section 4b) that the route assertions of test_gpu_ops.py and
test_gpu_ops_engine_paths.py do not reach.  Every shape is the smallest that
crosses the rule's threshold (derived beside each case from the constant in
gemm.hip); every result is compared with a float64 torch reference over the
f16-rounded operands at the bar of the same op's test in test_gpu_ops.py, and
every case asserts the route it is here for (_lib.last_gemm_route)."""

import zlib

import pytest
import torch
import torch.nn.functional as F

from gpu_util import close, conv_w, nhwc, op, pad_w, ptr, stream
from monocular_depth_estimation_trt_amd import _lib

pytestmark = pytest.mark.gpu


def rn(key, *shape, scale=1.0):
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    return torch.randn(*shape, generator=g) * scale


def assert_route(**want):
    r = _lib.last_gemm_route()
    assert {f: r.get(f) for f in want} == want, r


def linear_operands(m, n, k):
    a16, w16 = rn(("a", m, n, k), m, k).half(), rn(("w", m, n, k), n, k, scale=k ** -0.5).half()
    b = rn(("b", m, n, k), n, scale=0.1)
    return a16, w16, b, a16.double() @ w16.double().T + b.double()


@pytest.mark.parametrize("m,n,k,tile", [
    # N <= 32: 128 x 32 tiles whatever M (two row tiles, the second of 2 rows; N = 24 leaves columns unused)
    (130, 24, 40, (128, 32, 4, 1)),
    # N <= 64 and M >= 128 * 256 = 32768: 128 x 64 tiles (one row less runs 64^2 tiles)
    (32768, 64, 40, (128, 64, 4, 1)),
], ids=["t128x32", "t128x64"])
def test_store_narrow_n_tiles(gpu, m, n, k, tile):
    a16, w16, b, ref = linear_operands(m, n, k)
    wp = pad_w(w16.float()).to(gpu)
    out = torch.empty(m, n, dtype=torch.float16, device=gpu)
    op("mde_op_linear", ptr(a16.to(gpu)), k, ptr(wp), wp.shape[1], m, n, k, ptr(b.to(gpu)), 0, ptr(out), n, stream())
    assert_route(kind="tile", bm=tile[0], bn=tile[1], wm=tile[2], wn=tile[3], slices=1)
    close(out, ref, 1e-2, 1e-2, f"linear {m}x{n}x{k}")


@pytest.mark.parametrize("m,n,k,want", [
    # t256 = ceil(M / 256) * ceil(N / 128) >= 512: N = 384 gives 3 columns, so 171 row tiles, M = 170 * 256 + 1
    (43521, 384, 64, dict(bm=256, bn=128, wm=4, wn=2, bk=32, stages=3)),
    # K <= 384 and ceil(M / 128) * ceil(N / 128) >= kBigTileMin = 240: 80 x 3 tiles, M = 79 * 128 + 1 (t256 = 120)
    (10113, 384, 40, dict(bm=128, bn=64, wm=4, wn=1, bk=64)),
    # narrow_resid: 64^2 tiles < 256 and 192 <= 32 x 64 tiles <= 512: 32 x 6 = 192 tiles, M = 31 * 32 + 1
    (993, 384, 72, dict(bm=32, bn=64, wm=2, wn=2, stages=4)),
], ids=["t256x128", "t128x64_short_k", "t32x64_narrow"])
def test_residual_tiles(gpu, m, n, k, want):
    a16, w16, b, acc = linear_operands(m, n, k)
    ls, x = 0.5 + 0.05 * rn(("ls", m, n, k), n), rn(("x", m, n, k), m, n)
    ref = x.double() + ls.double() * acc
    wp = pad_w(w16.float()).to(gpu)
    xg = x.clone().to(gpu)
    op("mde_op_linear_residual", ptr(a16.to(gpu)), k, ptr(wp), wp.shape[1], m, n, k, ptr(b.to(gpu)), ptr(ls.to(gpu)),
       ptr(xg), n, stream())
    assert_route(kind="tile", slices=1, **want)
    close(xg, ref, 2e-3, 2e-3, f"linear_residual {m}x{n}x{k}")


def test_patch_embed_bk32(gpu):
    """E_PATCH on the 128^2 BK 32 tiles: K = 672 <= kBk32Kmax = 768 and 30 x 8
    = 240 = kBigTileMin tiles -- D = 1024 gives 8 columns, 30 row tiles need
    more than 29 * 128 = 3712 patches: 619 images of 2 x 3 patches = 3714."""
    B, Hh, Ww, D = 619, 28, 42, 1024
    ph, pw = Hh // 14, Ww // 14
    img = rn("img", B, 3, Hh, Ww)
    w, b = rn("pw", D, 3, 14, 14, scale=588 ** -0.5), rn("pb", D, scale=0.02)
    pos, cls_pos = rn("pos", ph * pw, D, scale=0.5), rn("cls", D, scale=0.5)
    t = F.conv2d(img.half().double(), w.half().double(), b.double(), stride=14).flatten(2).transpose(1, 2) + pos.double()
    ref = torch.cat([cls_pos.double().expand(B, 1, D), t], 1).reshape(B * (ph * pw + 1), D)
    w16 = torch.zeros(D, 3, 14, 16)
    w16[..., :14] = w
    wp = pad_w(w16.reshape(D, 672)).to(gpu)
    scratch = torch.empty(B * ph * pw, 672, dtype=torch.float16, device=gpu)
    x = torch.empty(B * (ph * pw + 1), D, device=gpu)
    op("mde_op_patch_embed", ptr(img.to(gpu)), B, Hh, Ww, ptr(wp), wp.shape[1], ptr(b.to(gpu)), ptr(pos.to(gpu)),
       ptr(cls_pos.to(gpu)), D, ptr(scratch), ptr(x), stream())
    assert_route(kind="tile", bm=128, bn=128, wm=2, wn=2, bk=32, stages=3)
    close(x, ref, 1e-3, 2e-3, "patch_embed")


def test_conv_transpose_bk32(gpu):
    """E_CONVT on the 128^2 BK 32 tiles: K = 48, N = 4 * 4 * 48 = 768 gives 6
    columns, kBigTileMin = 240 tiles need 40 row tiles, more than 39 * 128 =
    4992 input pixels: one 71 x 71 map (5041)."""
    s, cin, B, h, w = 4, 48, 1, 71, 71
    x16 = rn("tx", B, cin, h, w).half()
    wt, b = rn("tw", cin, cin, s, s, scale=cin ** -0.5), rn("tb", cin, scale=0.02)
    ref = F.conv_transpose2d(x16.double(), wt.half().double(), b.double(), stride=s).permute(0, 2, 3, 1)
    wp = pad_w(wt.permute(2, 3, 1, 0).reshape(s * s * cin, cin)).to(gpu)
    out = torch.empty(B, h * s, w * s, cin, dtype=torch.float16, device=gpu)
    op("mde_op_conv_transpose", ptr(nhwc(x16).to(gpu)), B, h, w, cin, ptr(wp), wp.shape[1], cin, s, ptr(b.to(gpu)),
       ptr(out), stream())
    assert_route(kind="tile", bm=128, bn=128, wm=2, wn=2, bk=32, stages=3)
    close(out, ref, 1e-2, 1e-2, "conv_transpose")


def conv_operands(B, h, w, cin, cout, stride):
    x16 = rn(("cx", B, h, w, cin), B, cin, h, w).half()
    wt, b = rn(("cw", cin, cout), cout, cin, 3, 3, scale=(9 * cin) ** -0.5), rn(("cb", cout), cout, scale=0.02)
    ref = F.conv2d(x16.double(), wt.half().double(), b.double(), stride=stride, padding=1).permute(0, 2, 3, 1)
    return nhwc(x16), conv_w(wt), b, ref


def test_stride2_conv_takes_the_gemm(gpu):
    """prefer_im2col: a stride-2 conv the direct conv supports (32 channels)
    runs as the implicit-im2col GEMM -- here its 128 x 32 tile (N = 32), one
    workgroup of 25 output pixels."""
    x, wp, b, ref = conv_operands(1, 9, 9, 32, 32, 2)
    out = torch.empty(1, 5, 5, 32, dtype=torch.float16, device=gpu)
    op("mde_op_conv3x3", ptr(x.to(gpu)), 1, 9, 9, 32, ptr(wp.to(gpu)), wp.shape[1], 32, 2, 0, ptr(b.to(gpu)), 0, None,
       None, ptr(out), stream())
    assert_route(kind="tile", bm=128, bn=32, slices=1)
    close(out, ref, 1e-2, 1e-2, "conv3x3 stride 2")


def test_resize_first(gpu):
    """res1_up on a conv whose epilogue does not read it (128 output channels:
    conv3_takes_res1_up stops at 64): the upsample is written into res1 by a
    resize launch, then the direct conv adds res1."""
    B, h, w, cin, cout, sh, sw = 1, 9, 9, 32, 128, 5, 5
    x, wp, b, base = conv_operands(B, h, w, cin, cout, 1)
    u16 = rn("up", B, cout, sh, sw).half()
    up = F.interpolate(u16.double(), size=(h, w), mode="bilinear", align_corners=True).half().double()
    ref = base + up.permute(0, 2, 3, 1)
    out = torch.empty(B, h, w, cout, dtype=torch.float16, device=gpu)
    res1 = torch.empty_like(out)
    op("mde_op_conv3x3_res", ptr(x.to(gpu)), B, h, w, cin, ptr(wp.to(gpu)), wp.shape[1], cout, 1, 0, ptr(b.to(gpu)), 0,
       None, 0, ptr(res1), ptr(nhwc(u16).to(gpu)), sh, sw, ptr(out), None, 0, None, None, 0, 0, stream())
    assert_route(kind="conv_direct", resize_first=1)
    close(out, ref, 1e-2, 1e-2, "conv3x3 res1_up, resized first")


def test_deep64_ring(gpu):
    """Switch "deep64" at op level: a grid of 4 64^2 tiles runs the 4-deep ring
    with the switch on and the 2-stage kernel with it off -- two routes, the
    same K order per tile, the same bits."""
    m, n, k = 77, 96, 40
    a16, w16, b, ref = linear_operands(m, n, k)
    wp, ag, bg = pad_w(w16.float()).to(gpu), a16.to(gpu), b.to(gpu)
    outs = []
    for deep, stages in ((1, 4), (0, 2)):
        out = torch.empty(m, n, dtype=torch.float16, device=gpu)
        with _lib.tuning(deep64=deep):
            op("mde_op_linear", ptr(ag), k, ptr(wp), wp.shape[1], m, n, k, ptr(bg), 0, ptr(out), n, stream())
        assert_route(kind="tile", bm=64, bn=64, stages=stages)
        close(out, ref, 1e-2, 1e-2, f"linear deep64={deep}")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
