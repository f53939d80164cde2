"""What the drivers answer when --ply, --mesh or --cloud-view cannot be served: one table over {Depth Pro,
DA-V2 and its family} x the three options.  Every case ends in SystemExit before an engine is built (no
GPU), with the text the drivers printed before the options moved into pointcloud.py's one stage, and
writes no file.
"""

import os

import numpy as np
import pytest

STEP = {"--ply": "--ply-step", "--mesh": "--mesh-step", "--cloud-view": "--cloud-view-step"}
METRIC = ["--source", "synthetic:vits:metric:1234", "--f-px", "500"]
NO_MAP_DP = "{opt} runs on the device post-process's depth map: do not combine it with --host-postprocess"
NO_MAP_DAV2 = ("{opt} runs on the device post-process's depth map: not with --host-postprocess or a model without a "
               "post-process")
STEP_TEXT = "{step} must be positive"
PHOTO_SIZE = "{opt} takes its colours from the --image photo: --src-hw must be the photo's size"
NO_FOCAL = "{opt} needs --f-px (a positive focal length in pixels): this model predicts none"
NOT_METRIC = "{opt} needs a metric model: relative depth is not turned into metres"

# (driver, arguments around the option, the text)
CASES = [
    ("depth_pro", ["--host-postprocess"], NO_MAP_DP),
    ("depth_pro", ["{step}", "0"], STEP_TEXT),
    ("depth_pro", ["{step}", "-3"], STEP_TEXT),
    ("depth_pro", ["--image", "{photo}", "--src-hw", "5", "8"], PHOTO_SIZE),
    ("depth_anything_v2", METRIC + ["--host-postprocess"], NO_MAP_DAV2),
    ("depth_anything_v2", METRIC + ["{step}", "0"], STEP_TEXT),
    ("depth_anything_v2", METRIC + ["--image", "{photo}", "--src-hw", "6", "9"], PHOTO_SIZE),
    ("depth_anything_v2", METRIC[:2], NO_FOCAL),
    ("depth_anything_v2", METRIC[:2] + ["--f-px", "0"], NO_FOCAL),
    ("depth_anything_v2", ["--source", "synthetic:vits:relative:1234", "--f-px", "500"], NOT_METRIC),
    ("depth_anything_ac", ["--f-px", "500"], NOT_METRIC),
    ("depth_anything_ac", [], NO_FOCAL),
    ("distill_any_depth", ["--f-px", "500"], NOT_METRIC),
    ("distill_any_depth", [], NO_FOCAL),
]


@pytest.fixture(scope="module")
def photo(tmp_path_factory):
    path = tmp_path_factory.mktemp("photo") / "p.npy"
    np.save(path, np.zeros((6, 8, 3), np.uint8))
    return str(path)


@pytest.mark.parametrize("opt", list(STEP))
@pytest.mark.parametrize("driver, argv, text", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_refusal_text(driver, argv, text, opt, photo, tmp_path, monkeypatch):
    import importlib
    run = importlib.import_module(f"monocular_depth_estimation_trt_amd.models.{driver}.run")
    monkeypatch.chdir(tmp_path)  # the default --out-dir and engine paths are not reached; were they, it shows here
    out = tmp_path / "out.bin"
    fill = dict(opt=opt, step=STEP[opt], photo=photo)
    with pytest.raises(SystemExit) as e:
        run.main([opt, str(out)] + [x.format(**fill) for x in argv])
    assert str(e.value) == text.format(**fill)
    assert os.listdir(tmp_path) == []
