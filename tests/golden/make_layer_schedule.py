"""Generate tests/golden/layer_schedule.json (run on an MI355X with the
library built):

    python tests/golden/make_layer_schedule.py

For every case of tests/schedule_cases.py: the profiler step names of one
eager forward, in launch order.  tests/test_gpu_schedule.py holds every later
build to these lists; flops*.py, bench.py's roofline and tools/pmc_traffic.py
key on the names.  Regenerate only with a change that means to alter a
schedule, from the commit before it where the change is a refactor.
"""

from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import schedule_cases  # noqa: E402


def main():
    rec = {}
    for name in schedule_cases.CASES:
        names, outs, _ = schedule_cases.run(name)
        assert all((o == o).all() for o in outs.values()), name   # every output written, no NaN
        rec[name] = names
        print(name, len(names), "steps", flush=True)
    with open(os.path.join(HERE, "layer_schedule.json"), "w") as f:
        json.dump(rec, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
