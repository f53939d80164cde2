"""The scenes the mesh tests share (tests/test_mesh_cpu.py, tests/test_gpu_mesh.py).

One float32 depth map: a gently slanted plane (about 2 m, +0.004 per pixel in x, +0.006 per pixel in
y), multiplied by 1.25 on alternating blocks whose borders are slanted -- block parity
((v + u // 2) // (7 * step) + (u + v // 3) // (9 * step)) % 2, so that the sampled grid of every step
sees blocks 7 by 9 samples large -- with +-0.5 % of noise.  At the reference's rtol = 0.1 a block border
(a 25 % step) is a depth edge and the noise (1 % at most between neighbours, plus the slant) is not.

`scene` asserts on pointcloud.mesh_np's flags what keeps a test on it from passing vacuously: every
sampled row and column holds an edge sample, every row and column but the last holds a kept quad, and
the kept quads are at least 10 % of all quads.  The block pattern is fixed by the formula, not by the
noise, so what a small grid cannot hold is named in EXEMPT, case by case, and everything else is
asserted: 9 x 5 lies inside one or two blocks (at steps 2 and 3 it has no edge at all: those cases
check the grid smaller than a tile, and the validity patterns laid over it), and the 19 x 27 and
13 x 18 grids of 37 x 53 at steps 2 and 3 have two columns that an edge band covers from top to bottom.
"""

import functools

import numpy as np

from monocular_depth_estimation_trt_amd import pointcloud as pc

RTOL = 0.1   # the reference's depth_map_edge(rtol=0.1)
Z_LO, Z_HI = np.float32(0.25), np.float32(80.0)
SHAPES = [(9, 5), (37, 53), (100, 76), (130, 150), (600, 800)]
STEPS = {(600, 800): (1,)}  # every other shape: 1, 2, 3


def steps_of(shape):
    return STEPS.get(tuple(shape), (1, 2, 3))


def raw_scene(h, w, step=1):
    """The scene without the checks (bench_mesh scales it up; the CPU tests build their own cases on it)."""
    rng = np.random.Generator(np.random.PCG64(h * 10007 + w * 31 + step))
    v, u = np.mgrid[0:h, 0:w]
    z = 2.0 + 0.004 * u + 0.006 * v
    block = ((v + u // 2) // (7 * step) + (u + v // 3) // (9 * step)) % 2
    z = z * np.where(block == 1, 1.25, 1.0) * (1.0 + rng.uniform(-0.005, 0.005, size=(h, w)))
    return z.astype(np.float32)


def camera(h, w):
    """(fx, fy, cx, cy): an off-centre camera with different focal lengths on the two axes."""
    return 0.8 * w + 0.37, 0.7 * w + 0.11, w / 2 + 0.3, h / 2 - 0.7


ROWS_EDGE, COLS_EDGE, ROWS_QUAD, COLS_QUAD, SHARE = "rows_edge", "cols_edge", "rows_quad", "cols_quad", "share"
EXEMPT = {(9, 5, 1): {ROWS_EDGE, ROWS_QUAD}, (9, 5, 2): {ROWS_EDGE, COLS_EDGE}, (9, 5, 3): {ROWS_EDGE, COLS_EDGE},
          (37, 53, 2): {COLS_QUAD}, (37, 53, 3): {COLS_QUAD}}


def check_not_vacuous(flags, exempt=()):
    edge, quad = (flags & pc.F_EDGE) != 0, (flags & pc.F_QUAD) != 0
    hold = {ROWS_EDGE: edge.any(axis=1).all(), COLS_EDGE: edge.any(axis=0).all(),
            ROWS_QUAD: quad[:-1].any(axis=1).all(), COLS_QUAD: quad[:, :-1].any(axis=0).all(),
            SHARE: quad.sum() >= 0.1 * (flags.shape[0] - 1) * (flags.shape[1] - 1)}
    for name, ok in hold.items():
        # an exemption that is not needed is a mistake too: the case then asserts less than it could
        assert bool(ok) != (name in exempt), (name, flags.shape, "exempt" if name in exempt else "does not hold")


@functools.lru_cache(maxsize=None)
def scene(h, w, step=1):
    """[h][w] float32, checked at rtol = 0.1 on the sampled grid of `step`; cached, never written."""
    z = raw_scene(h, w, step)
    flags = pc.mesh_np(z, *camera(h, w), step=step, z_lo=Z_LO, z_hi=Z_HI, edge_rtol=RTOL)[2]
    check_not_vacuous(flags, EXEMPT.get((h, w, step), ()))
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def photo(h, w, batch=1):
    rng = np.random.Generator(np.random.PCG64(h * 131 + w + 11))
    a = rng.integers(0, 256, size=(batch, h, w, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a
