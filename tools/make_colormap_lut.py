"""Write monocular_depth_estimation_trt_amd/colormaps.py: matplotlib's 256-entry `turbo` and `magma`
tables as uint8 R, G, B literals, entry i = (cmap(i)[:3] * 255).astype(uint8) -- what the reference
drivers' `(cmap(x)[..., :3] * 255).astype(np.uint8)` yields for table index i.  The product does not
import matplotlib; this tool does, once, where it is installed:

    python tools/make_colormap_lut.py [--out monocular_depth_estimation_trt_amd/colormaps.py]

tests/test_colorize_cpu.py compares the committed tables with the installed matplotlib's.
"""

import argparse
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("turbo", "magma")

HEADER = '''"""matplotlib's 256-entry colour tables as uint8 R, G, B: entry i is
(cmap(i)[:3] * 255).astype(uint8).  Written by tools/make_colormap_lut.py from
matplotlib {version}; do not edit.  visualize.lut() appends the bad colour."""

import numpy as np


def _table(hex_rows: str) -> np.ndarray:
    t = np.frombuffer(bytes.fromhex("".join(hex_rows.split())), dtype=np.uint8).reshape(256, 3).copy()
    t.setflags(write=False)
    return t

'''


def table(name: str) -> np.ndarray:
    import matplotlib
    cmap = matplotlib.colormaps[name]
    return np.array([(np.asarray(cmap(i)[:3]) * 255).astype(np.uint8) for i in range(256)], dtype=np.uint8)


def render() -> str:
    import matplotlib
    out = [HEADER.format(version=matplotlib.__version__)]
    for name in NAMES:
        t = table(name)
        rows = [" ".join(bytes(t[i]).hex() for i in range(r, r + 16)) for r in range(0, 256, 16)]
        out.append(f'\n{name.upper()} = _table("""\n' + "\n".join(rows) + '\n""")\n')
    out.append('\nTABLES = {' + ", ".join(f'"{n}": {n.upper()}' for n in NAMES) + '}\n')
    return "".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "monocular_depth_estimation_trt_amd", "colormaps.py"))
    a = ap.parse_args(argv)
    with open(a.out, "w") as f:
        f.write(render())
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
