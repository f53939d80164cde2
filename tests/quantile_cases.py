"""Seeded maps for the robust-range tests (test_quantiles_cpu.py, test_gpu_quantiles.py): every regime
at which an exact selection by radix digits can go wrong, at any [batch, h, w]."""

import numpy as np

FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)  # the smallest denormal

REGIMES = ("lognormal", "constant", "two_values", "ladder", "power_of_two", "denormal_fltmax", "sprinkled",
           "all_invalid", "one_valid")
# (batch, h, w, floats the map pointer is shifted off its 16-byte alignment)
SHAPES = ((1, 1, 1, 0), (1, 3, 5, 0), (1, 7, 9, 0), (1, 37, 53, 1), (1, 100, 131, 0), (3, 5, 7, 0), (2, 37, 53, 0))
QS = ((2.0, 98.0), (2.0, 50.0, 98.0), (0.0,), (100.0,))


def rng_of(regime, shape, seed=0):
    return np.random.Generator(np.random.PCG64([REGIMES.index(regime), *shape, seed]))


def maps(regime, batch, h, w, seed=0):
    """float32 [batch, h, w]."""
    shape = (batch, h, w)
    n = batch * h * w
    g = rng_of(regime, shape, seed)
    if regime == "lognormal":
        x = np.exp(g.normal(1.0, 0.8, n)).astype(np.float32)
    elif regime == "constant":
        x = np.full(n, 2.5, np.float32)
    elif regime == "two_values":
        x = np.where(g.random(n) < 0.3, np.float32(1.25), np.float32(7.0)).astype(np.float32)
    elif regime == "ladder":
        # nextafter neighbours around 3: the keys differ in the last digit only (and across 3's own bits)
        steps = g.integers(-100, 100, n)
        x = (np.float32(3.0).view(np.int32) + steps.astype(np.int32)).view(np.float32)
    elif regime == "power_of_two":
        # half just below 2, half from 2 up: the median's prev and next sit in different top digits
        lo = np.nextafter(np.float32(2.0), np.float32(0.0)) - g.random(n).astype(np.float32) * np.float32(0.5)
        hi = np.float32(2.0) + g.random(n).astype(np.float32)
        x = np.where(np.arange(n) % 2 == 0, lo, hi).astype(np.float32)
        x = g.permutation(x)
    elif regime == "denormal_fltmax":
        pool = np.array([DENORM, 3 * DENORM, np.float32(1e-39), np.finfo(np.float32).tiny, 1.0, FLT_MAX,
                         np.nextafter(FLT_MAX, np.float32(0))], np.float32)
        x = pool[g.integers(0, len(pool), n)]
    elif regime == "sprinkled":
        # NaN, +-inf, 0, -0 and negatives in runs of 1..300 pixels: they cross waves (64 x 4 pixels) and
        # tiles (4096) wherever the map is long enough
        x = np.exp(g.normal(0.5, 1.0, n)).astype(np.float32)
        odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, -40.0, -1e-30], np.float32)
        i = 0
        while i < n:
            run = int(g.integers(1, 301))
            if g.random() < 0.45:
                x[i:i + run] = odd[g.integers(0, len(odd))]
            elif g.random() < 0.2:
                x[i:i + run] = -x[i:i + run]
            i += run
    elif regime == "all_invalid":
        x = np.array([np.nan, np.inf, -np.inf], np.float32)[g.integers(0, 3, n)]
    elif regime == "one_valid":
        x = np.full(n, np.nan, np.float32)
        x[int(g.integers(0, n))] = 4.0
    else:
        raise KeyError(regime)
    return np.ascontiguousarray(x.reshape(shape))


def with_n_valid(n_valid, h=16, w=16, seed=0):
    """[h, w] with exactly n_valid finite positive pixels, the others NaN, 0 or negative."""
    g = np.random.Generator(np.random.PCG64([n_valid, h, w, seed]))
    x = np.array([np.nan, 0.0, -2.0], np.float32)[g.integers(0, 3, h * w)]
    at = g.permutation(h * w)[:n_valid]
    x[at] = np.exp(g.normal(1.0, 0.8, n_valid)).astype(np.float32)
    return x.reshape(h, w)
