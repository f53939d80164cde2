"""Generate tests/golden/pack_manifest.json (CPU only):

    python tests/golden/make_pack_manifest.py

For every case of tests/test_pack_manifest.py: the 256 PackConfig bytes, the
tensors of the packed file in file order (name, dtype, shape, sha256 over
dtype + shape + raw bytes), and how many tensors each sha256-exempt pattern
matches; and the layer_flops tables of its FLOP cases (names in order, exact
values).  tests/test_pack_manifest.py holds every later tree to it.

Regenerate only with a change that means to alter the packed layout or a FLOP
table.  Such a change also bumps pack.PACKER_VERSION (it is part of the
engine-cache fingerprint: an unchanged version would reuse stale cached
engines).  Where the change is a refactor, do not regenerate: the manifest of
the commit before it is the check.
"""

from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_pack_manifest as T  # noqa: E402
from monocular_depth_estimation_trt_amd import pack  # noqa: E402


def _rows(rows) -> str:
    """One JSON row per line."""
    return "[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]"


def main():
    packs = []
    for name in T.CASES:
        d = T.describe(name)
        counts = T.exempt_counts([t[0] for t in d["tensors"]], d["patterns"])
        packs.append(f'{json.dumps(name)}: {{\n"config": {json.dumps(d["config"])},\n'
                     f'"patterns": {json.dumps(d["patterns"])},\n"exempt_counts": {json.dumps(counts)},\n'
                     f'"tensors": {_rows(d["tensors"])}\n}}')
        print(name, len(d["tensors"]), "tensors,", sum(counts.values()), "exempt from the sha256", flush=True)
    fl = [f"{json.dumps(name)}: {_rows([[k, v] for k, v in fn().items()])}" for name, fn in T.FLOP_CASES.items()]
    with open(os.path.join(HERE, "pack_manifest.json"), "w") as f:
        f.write('{\n"packer_version": ' + json.dumps(pack.PACKER_VERSION) + ',\n"packs": {\n' + ",\n".join(packs)
                + '\n},\n"flops": {\n' + ",\n".join(fl) + "\n}\n}\n")


if __name__ == "__main__":
    main()
