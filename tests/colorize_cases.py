"""What the colour-frame tests share: the seeded maps of tests/golden/colorize_cases.npz
(tests/golden/make_colorize_golden.py writes it; test_colorize_cpu.py and test_gpu_colorize.py read
it) and the inputs with planted values.  The fixture holds only what matplotlib drew; the maps are
regenerated here from their seeds."""

import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "colorize_cases.npz")
H, W = 37, 53
FIXED_RANGE = (0.5, 20.0)  # mode 2's axis in the fixture, metres
# the four clipping regimes of mode 0 (inverse depth against [1/250, 10]): name -> (seed, draw)
REGIMES = {
    "neither": (11, lambda rng, s: rng.uniform(0.5, 20.0, s)),         # 1/d in [0.05, 2]
    "high": (12, lambda rng, s: rng.uniform(0.02, 20.0, s)),           # 1/d up to 50: the top clips
    "low": (13, lambda rng, s: rng.uniform(0.5, 900.0, s)),            # 1/d down to 1/900: the bottom clips
    "both": (14, lambda rng, s: np.exp(rng.uniform(np.log(1e-3), np.log(1e3), s))),
}
# case name -> (mode, map_is_inverse, denom_eps); every regime has every case
VARIANTS = {
    "inverse_auto": (0, False, 0.0),
    "inverse_auto_eps": (0, False, 1e-6),
    "inverse_auto_inv": (0, True, 0.0),
    "inverse_auto_inv_eps": (0, True, 1e-6),
    "minmax_u8": (1, False, 0.0),
    "fixed": (2, False, 0.0),
}


@functools.lru_cache(maxsize=None)
def depth_map(regime: str, h: int = H, w: int = W) -> np.ndarray:
    """The regime's depth map, float32 [h, w], never written."""
    seed, draw = REGIMES[regime]
    d = draw(np.random.Generator(np.random.PCG64(seed)), (h, w)).astype(np.float32)
    d.setflags(write=False)
    return d


def case_input(regime: str, variant: str) -> np.ndarray:
    """What the op is given: depth, or its float32 reciprocal for the inverse-input variants."""
    d = depth_map(regime)
    return (np.float32(1.0) / d) if VARIANTS[variant][1] else d


def case_kwargs(variant: str) -> dict:
    mode, inverse, eps = VARIANTS[variant]
    kw = dict(mode=mode, map_is_inverse=inverse, denom_eps=eps)
    if mode == 2:
        kw.update(vmin=FIXED_RANGE[0], vmax=FIXED_RANGE[1])
    return kw


@functools.lru_cache(maxsize=None)
def load_fixture() -> dict:
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def sprinkled(regime: str, h: int = H, w: int = W, seed: int = 5) -> np.ndarray:
    """The regime's map with NaN, +-inf, +-0 and negative pixels planted at seeded places."""
    x = np.array(depth_map(regime, h, w))
    rng = np.random.Generator(np.random.PCG64(seed))
    flat = x.reshape(-1)
    vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.5, -1e-3], dtype=np.float32)
    where = rng.choice(flat.size, size=min(flat.size, 4 * len(vals)), replace=False)
    flat[where] = np.resize(vals, where.size)
    return x
