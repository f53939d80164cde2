"""The profiler step names of every forward schedule, in launch order, against
tests/golden/layer_schedule.json (tests/golden/make_layer_schedule.py).

flops.py, flops_depth_pro.py, flops_vggt.py, bench.py's roofline and
tools/pmc_traffic.py key on these names, and the three families share the
block and decoder helpers that emit them: a reordered, renamed, missing or
extra step in any case fails here (list equality).
"""

import json
import os

import pytest

from conftest import GOLDEN
import schedule_cases

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "layer_schedule.json")) as _f:
    SCHEDULE = json.load(_f)


def test_fixture_covers_the_cases():
    assert sorted(SCHEDULE) == sorted(schedule_cases.CASES)


@pytest.mark.parametrize("name", list(schedule_cases.CASES))
def test_layer_schedule(gpu, name):
    names, outs, _ = schedule_cases.run(name)
    want = SCHEDULE[name]
    diff = next((i for i, (a, b) in enumerate(zip(names, want)) if a != b), min(len(names), len(want)))
    assert names == want, (f"{name}: {len(names)} steps, expected {len(want)}; first difference at step {diff}: "
                           f"{names[diff:diff + 3]} vs {want[diff:diff + 3]}")
