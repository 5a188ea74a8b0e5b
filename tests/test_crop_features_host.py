"""Crop features (the association head on mask-cropped RoI features) on a machine without a GPU: the new C ABI entries refuse a
NULL context, C4 configurations are refused in Python with a sentence, the switch defaults to off, and the tools list the flag."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entries_refuse_a_null_context():
    from apse_uav_amd import _lib
    lib = _lib.load()
    assert "apse_set_crop_features" in _lib.EXPORTS and "apse_roi_features_windows" in _lib.EXPORTS
    assert lib.apse_set_crop_features(None, 1) < 0
    assert lib.apse_set_crop_features(None, 0) < 0
    assert lib.apse_roi_features_windows(None, 0, None, None, 0, 10, None, None) < 0
    assert lib.apse_roi_features_windows(None, 0, None, None, 4, 10, None, None) < 0


def test_crop_features_defaults_to_off():
    from apse_uav_amd.config import setup_cfg
    cfg = setup_cfg(device="cpu")
    assert cfg.APSE.CROP_FEATURES is False
    assert setup_cfg(arch="C4", device="cpu").APSE.CROP_FEATURES is False


def test_c4_refuses_crop_features_with_a_sentence():
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.utils.MOT_utils import MOTSloader
    from apse_uav_amd.weights import synthetic_association_state
    cfg = setup_cfg(arch="C4", device="cpu")
    with pytest.raises(NotImplementedError, match="C4"):
        RcnnTracker(cfg, (270, 480), synthetic_association_state(1), crop_features=True)
    on = setup_cfg(arch="C4", device="cpu")
    on.APSE.CROP_FEATURES = True
    with pytest.raises(NotImplementedError, match="C4"):
        RcnnTracker(on, (270, 480), synthetic_association_state(1))
    with pytest.raises(NotImplementedError, match="C4"):
        MOTSloader(cfg, "/nonexistent/dataset", "/nonexistent/seqmap", crop_features=True)


@pytest.mark.parametrize("tool", ["train_association_head.py", "track_mots.py", "run_sequence.py"])
def test_tools_list_the_flag(tool):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert "--crop-features" in out.stdout
