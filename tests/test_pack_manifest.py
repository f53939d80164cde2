"""The packed layout of the three families and their FLOP tables, against
tests/golden/pack_manifest.json (tests/golden/make_pack_manifest.py).

The weights / pack / flops modules of Depth Anything V2, Depth Pro and VGGT
share their ViT-block and DPT-head descriptions.  A change there that moves
the tensor order inside a block, the channel padding of `rnN.w`, which
refinenet lacks unit 1, or a PackConfig offset fails here: per case the 256
PackConfig bytes, the tensor names in file order, every dtype and shape, and
the sha256 (over dtype, shape and raw bytes) of every tensor that is a pure
relayout of drawn weights (cast, pad, transpose, concatenate) are compared for
equality.  A change that means to alter the layout bumps pack.PACKER_VERSION
and regenerates the manifest.

Tensors whose values pass through floating-point kernels that may differ in
the last bit between CPU builds of numpy or torch (sums, matrix products,
einsum, bicubic interpolation, sin / cos / pow, conv2d) are exempt from the
sha256 comparison only; EXEMPT names them, and the number of tensors each
pattern matches in each case is held to the count the manifest records.
"""

import fnmatch
import functools
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN

from monocular_depth_estimation_trt_amd import flops, flops_depth_pro, flops_vggt
from monocular_depth_estimation_trt_amd import pack, pack_depth_pro, pack_vggt
from monocular_depth_estimation_trt_amd import weights, weights_depth_pro, weights_vggt

# (fnmatch pattern, the cases it applies to, why the bytes may differ between CPU builds)
EXEMPT = [
    ("*.wf", "all", "LayerNorm fold: fp64 product W * gamma"),
    ("*.c1", "all", "LayerNorm fold: fp64 row sums"),
    ("*.c2", "all", "LayerNorm fold: fp64 matrix-vector product"),
    ("pos.cls.st", "all", "LayerNorm partials of the cls row: fp64 sums"),
    ("pos.patch", "interpolated", "bicubic interpolation (torch)"),
    ("pos.cls", "interpolated", "row 0 of the interpolated table (torch.cat output)"),
    ("rope.*", "all", "fp32 pow / cos / sin"),
    ("pe[0-3]", "all", "UV embedding: fp64 pow / sin / cos"),
    ("head.pe", "all", "UV embedding through torch conv2d"),
    ("fs*.up.w", "all", "deconv x projection fold: fp64 einsum"),
    ("patch.w", "vggt", "ImageNet normalisation fold: fp64 divide"),
    ("patch.b", "vggt", "ImageNet normalisation fold: fp64 sum"),
]

# name -> (family, arguments); the smallest cases that reach every branch of the packers
CASES = {
    "dav2_vits_metric_98x126_fp16": ("dav2", dict(encoder="vits", depth_type="metric", seed=7, hw=(98, 126),
                                                  precision="fp16", input_format="float32_nchw")),
    "dav2_vits_metric_98x126_fp16_u8": ("dav2", dict(encoder="vits", depth_type="metric", seed=7, hw=(98, 126),
                                                     precision="fp16", input_format="uint8_nhwc")),
    "dav2_vits_metric_98x126_fp32": ("dav2", dict(encoder="vits", depth_type="metric", seed=7, hw=(98, 126),
                                                  precision="fp32", input_format="float32_nchw")),
    "dav2_vitb_relative_518_fp16": ("dav2", dict(encoder="vitb", depth_type="relative", seed=7, hw=(518, 518),
                                                 precision="fp16", input_format="float32_nchw")),
    "depth_pro_tiny_fov": ("depth_pro", dict(preset="tiny", seed=4321, use_fov=True)),
    "depth_pro_tiny_nofov": ("depth_pro", dict(preset="tiny", seed=4321, use_fov=False)),
    "vggt_tiny_s1": ("vggt", dict(preset="tiny", seed=2468, frames=1)),
    "vggt_tiny_s3": ("vggt", dict(preset="tiny", seed=2468, frames=3)),
}

FLOP_CASES = {
    "dav2_vits_518_b1": lambda: flops.layer_flops(weights.model_config("vits"), 518, 518, 1),
    "dav2_vitl_518_b3": lambda: flops.layer_flops(weights.model_config("vitl"), 518, 518, 3),
    "depth_pro_full_b2_fov": lambda: flops_depth_pro.layer_flops(
        weights_depth_pro.depth_pro_config("dinov2l16_384", use_fov=True), 2),
    "depth_pro_full_b2_nofov": lambda: flops_depth_pro.layer_flops(
        weights_depth_pro.depth_pro_config("dinov2l16_384", use_fov=False), 2),
    "vggt_1b_b2_s3": lambda: flops_vggt.layer_flops(weights_vggt.vggt_config("vggt_1b"), 2, 3),
}


@functools.lru_cache(maxsize=None)
def _dav2_sd(encoder, depth_type, seed):
    cfg = weights.model_config(encoder, depth_type)
    return cfg, weights.synthetic_state_dict(cfg, seed)


@functools.lru_cache(maxsize=None)
def _vggt_sd(preset, seed):
    cfg = weights_vggt.vggt_config(preset)
    return cfg, weights_vggt.synthetic_state_dict(cfg, seed)


def _applies(where, family, interpolated):
    return where == "all" or (where == "interpolated" and interpolated) or where == family


def _tensors(blob):
    """The tensor table of a packed file (csrc/pack_format.h) in file order:
    [name, dtype, shape, sha256 over dtype, shape and the raw bytes]."""
    magic, _, n, data_offset, _ = struct.unpack_from("<8sIIQQ", blob, 0)
    assert magic == b"MDEPACK1"
    out = []
    for i in range(n):
        name, dtype, ndim, *rest = struct.unpack_from("<80sii4iQQ8s", blob, 288 + 128 * i)
        dims, off, nbytes = list(rest[:ndim]), rest[4], rest[5]
        dtype = ("float32", "float16")[dtype]
        assert nbytes == int(np.prod(dims)) * np.dtype(dtype).itemsize
        h = hashlib.sha256()
        h.update(dtype.encode())
        h.update(str(tuple(dims)).encode())
        h.update(blob[data_offset + off:data_offset + off + nbytes])
        out.append([name.rstrip(b"\0").decode(), dtype, dims, h.hexdigest()])
    return out


def describe(name):
    """One case as the manifest records it: the PackConfig bytes, the tensors
    of the packed file in file order, and the EXEMPT patterns that apply."""
    family, a = CASES[name]
    interpolated = False
    if family == "dav2":
        cfg, sd = _dav2_sd(a["encoder"], a["depth_type"], a["seed"])
        h, w = a["hw"]
        interpolated = (h // cfg["patch"], w // cfg["patch"]) != (cfg["pos_grid"], cfg["pos_grid"])
        blob = pack.pack_bytes(sd, cfg, h, w, a["input_format"], a["precision"])
    elif family == "depth_pro":
        cfg = weights_depth_pro.depth_pro_config(a["preset"], use_fov=a["use_fov"])
        blob = pack_depth_pro.pack_bytes(weights_depth_pro.synthetic_state_dict(cfg, a["seed"]), cfg)
    else:
        cfg, sd = _vggt_sd(a["preset"], a["seed"])
        blob = pack_vggt.pack_bytes(sd, cfg, a["frames"])
    patterns = [p for p, where, _ in EXEMPT if _applies(where, family, interpolated)]
    return dict(config=blob[32:288].hex(), patterns=patterns, tensors=_tensors(blob))


def exempt_counts(names, patterns):
    return {p: sum(fnmatch.fnmatchcase(n, p) for n in names) for p in patterns}


@functools.lru_cache(maxsize=None)
def _manifest():
    with open(os.path.join(GOLDEN, "pack_manifest.json")) as f:
        return json.load(f)


def test_manifest_covers_the_cases():
    assert sorted(_manifest()["packs"]) == sorted(CASES)
    assert sorted(_manifest()["flops"]) == sorted(FLOP_CASES)
    assert _manifest()["packer_version"] == pack.PACKER_VERSION


@pytest.mark.parametrize("name", list(CASES))
def test_packed_layout(name):
    want, got = _manifest()["packs"][name], describe(name)
    assert got["config"] == want["config"]
    assert [t[0] for t in got["tensors"]] == [t[0] for t in want["tensors"]]
    assert [t[:3] for t in got["tensors"]] == [t[:3] for t in want["tensors"]]
    # the exemptions: the patterns of this case, each matching as many tensors as when the manifest was made,
    # and no tensor matched twice
    names = [t[0] for t in got["tensors"]]
    assert got["patterns"] == want["patterns"]
    assert exempt_counts(names, got["patterns"]) == want["exempt_counts"]
    exempt = {n for n in names if any(fnmatch.fnmatchcase(n, p) for p in got["patterns"])}
    assert len(exempt) == sum(want["exempt_counts"].values())
    differ = [g[0] for g, w in zip(got["tensors"], want["tensors"]) if g[0] not in exempt and g[3] != w[3]]
    assert not differ, f"{name}: {len(differ)} relayout tensors changed bytes, e.g. {differ[:4]}"


@pytest.mark.parametrize("name", list(FLOP_CASES))
def test_layer_flops(name):
    got = [[k, v] for k, v in FLOP_CASES[name]().items()]
    want = _manifest()["flops"][name]
    assert [k for k, _ in got] == [k for k, _ in want]
    assert got == want
