"""Write tests/golden/colorize_cases.npz: what matplotlib's `turbo` draws for the seeded maps of
tests/colorize_cases.py under the three recipes the reference drivers end with.  Needs matplotlib
(the product does not); run where it is installed:

    python tests/golden/make_colorize_golden.py

The recipes are stated here the way the reference's lines compute them, Python scalars and all, so
that NumPy's promotion rules decide the float types as they do there:

  inverse_auto   inverse depth against the display range [1/250, 1/0.1]: the ends are Python's
                 min / max of a float32 extreme and a Python float; the normalised map goes to the
                 colour map as floats.  `eps` adds the VGGT driver's 1e-6 to the denominator.
  minmax_u8      (d - min) / (max - min) * 255.0 cast to uint8; the colour map is indexed.
  fixed          float64, a given axis, clipped to [0, 1]; non-finite pixels get (60, 60, 66).

Every picture is stored BGR (the drivers' cvtColor(RGB2BGR)), with the range it was drawn on.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import colorize_cases as cc  # noqa: E402


def to_bgr_u8(rgba) -> np.ndarray:
    return np.ascontiguousarray((rgba[..., :3] * 255).astype(np.uint8)[..., ::-1])


def draw_inverse_auto(cmap, inverse_depth, eps):
    top = min(inverse_depth.max(), 1 / 0.1)
    bottom = max(1 / 250, inverse_depth.min())
    denom = (top - bottom + eps) if eps else (top - bottom)
    return to_bgr_u8(cmap((inverse_depth - bottom) / denom)), (bottom, top)


def draw_minmax_u8(cmap, depth):
    q = (depth - depth.min()) / (depth.max() - depth.min()) * 255.0
    return to_bgr_u8(cmap(q.astype(np.uint8))), (depth.min(), depth.max())


def draw_fixed(cmap, depth, vmin, vmax):
    a = np.asarray(depth, dtype=np.float64)
    bad = ~np.isfinite(a)
    t = np.clip((np.nan_to_num(a, nan=vmin) - vmin) / (vmax - vmin), 0.0, 1.0)
    rgb = (cmap(t)[..., :3] * 255.0).astype(np.uint8)
    rgb[bad] = np.asarray((60, 60, 66), np.uint8)
    return np.ascontiguousarray(rgb[..., ::-1]), (vmin, vmax)


def main():
    import matplotlib
    cmap = matplotlib.colormaps["turbo"]
    out = {}
    for regime in cc.REGIMES:
        for variant, (mode, inverse, eps) in cc.VARIANTS.items():
            x = cc.case_input(regime, variant)
            if mode == 0:
                pic, rng = draw_inverse_auto(cmap, x if inverse else 1 / x, eps)
            elif mode == 1:
                pic, rng = draw_minmax_u8(cmap, x)
            else:
                pic, rng = draw_fixed(cmap, x, *cc.FIXED_RANGE)
            out[f"{regime}/{variant}/bgr"] = pic
            out[f"{regime}/{variant}/range"] = np.array(rng, dtype=np.float32)
    np.savez_compressed(cc.FIXTURE, **out)
    print(f"wrote {cc.FIXTURE}: {len(out) // 2} cases, {os.path.getsize(cc.FIXTURE)} bytes "
          f"(matplotlib {matplotlib.__version__}, numpy {np.__version__})")


if __name__ == "__main__":
    main()
