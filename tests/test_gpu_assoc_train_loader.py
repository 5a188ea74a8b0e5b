"""-m gpu: MOTSloader (utils/MOT_utils.py) on a synthetic KITTI MOTS-layout dataset with seeded BLOCKS=(1,1,1,1) weights, the
feature cache, 6- vs 7-column object rows, and tools/train_association_head.py --synthetic end to end into RcnnTracker."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = (1, 1, 1, 1)


def _cfg(weights):
    from apse_uav_amd.config import setup_cfg
    cfg = setup_cfg(weights=weights)
    cfg.INPUT.MIN_SIZE_TEST = 256
    cfg.INPUT.MAX_SIZE_TEST = 448
    return cfg


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from apse_uav_amd.synthetic import write_synthetic_mots
    from apse_uav_amd.weights import synthetic_detector_state
    root = tmp_path_factory.mktemp("mots")
    seqmap = write_synthetic_mots(str(root / "ds"))
    weights = str(root / "det.pth")
    torch.save(synthetic_detector_state(0, BLOCKS), weights)
    return dict(root=str(root / "ds"), seqmap=seqmap, weights=weights)


def test_batch_equals_direct_generator_calls(data):
    from apse_uav_amd.engines.roi_features_generator import RoiFeaturesGenerator
    from apse_uav_amd.utils.MOT_utils import MOTSloader
    dl = MOTSloader(_cfg(data["weights"]), data["root"], data["seqmap"], frames_in_batch=6, roi_size=10)
    assert dl.num_of_sequences == 2 and dl.batches_per_sequence == [2, 2] and dl.num_of_batches == 4
    assert 1 not in list(dl.frames_with_objects_per_seq["0000"])
    gen = RoiFeaturesGenerator(_cfg(data["weights"]), roi_size=10)
    ids, rois = dl.get_training_batch(1, 1)
    seq = dl.seqmap_names[1]
    frames = dl.frames_with_objects_per_seq[seq][6:12]
    ri, rr = [], []
    for f in frames:
        objs, _ = dl.objects_masks_from_frame(seq, f)
        assert objs.shape[1] == 6 and not (objs[:, 1] == 10000).any()
        a, b = gen.get_rois_features(dl.frame_from_sequence(seq, f), objs)
        ri.append(a)
        rr.append(b)
    assert torch.equal(ids, torch.cat(ri)) and torch.equal(rois, torch.cat(rr))
    assert tuple(rois.shape[1:]) == (256, 10, 10) and float(rois.abs().max()) > 0
    # the same objects as 7-column rows (conf appended) give the same RoIs
    objs, _ = dl.objects_masks_from_frame(seq, frames[0])
    seven = np.concatenate([objs, np.ones((len(objs), 1), objs.dtype)], 1)
    a6, b6 = gen.get_rois_features(dl.frame_from_sequence(seq, frames[0]), objs)
    a7, b7 = gen.get_rois_features(dl.frame_from_sequence(seq, frames[0]), seven)
    assert torch.equal(a6, a7) and torch.equal(b6, b7)


def _two_epochs(data, cache):
    from apse_uav_amd.networks.association_head import AssociationHead
    from apse_uav_amd.online_triplet_loss import batch_hard_triplet_loss
    from apse_uav_amd.optim import SGD
    from apse_uav_amd.utils.MOT_utils import MOTSloader
    dl = MOTSloader(_cfg(data["weights"]), data["root"], data["seqmap"], frames_in_batch=6, roi_size=10, cache_features=cache)
    torch.manual_seed(0)
    head = AssociationHead(roi_size=10, input_depth=dl.roi_generator.get_features_depth()).to("cuda")
    head.train()
    opt = SGD(head.parameters(), lr=0.01, momentum=0.9)
    losses = []
    for _ in range(2):
        for s in range(dl.num_of_sequences):
            for b in range(dl.batches_per_sequence[s]):
                ids, rois = dl.get_training_batch(s, b)
                opt.zero_grad()
                loss = batch_hard_triplet_loss(ids, head(rois), margin=0.2, device="cuda:0")
                loss.backward()
                opt.step()
                losses.append(loss.item())
    return losses, head.state_dict()["fc.weight"].cpu()


def test_cache_gives_identical_epochs(data):
    a, wa = _two_epochs(data, False)
    b, wb = _two_epochs(data, True)
    assert a == b and torch.equal(wa, wb)
    assert all(np.isfinite(a))


def test_train_script_checkpoint_loads_into_tracker(data, tmp_path):
    out = tmp_path / "ah"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_association_head.py"), "--synthetic", "--epochs", "2",
                        "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for f in ("association_head_EP0.pth", "association_head_EP1.pth", "association_head.pth", "train_info.txt"):
        assert (out / f).exists(), f
    info = (out / "train_info.txt").read_text()
    assert info.startswith("FRAMES_IN_BATCH: 6\nNUM_EPOCH: 2\nROI_SIZE: 10\nLEARNING_RATE: 0.01\nMOMENTUM: 0.9\n")
    from apse_uav_amd.config import setup_cfg
    from apse_uav_amd.engines.rcnn_tracker import RcnnTracker
    from apse_uav_amd.synthetic import SyntheticSequence
    from apse_uav_amd.weights import synthetic_detector_state
    cfg = setup_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 256, 448
    tracker = RcnnTracker(cfg, (270, 480), str(out / "association_head.pth"), detector_state=synthetic_detector_state(0, BLOCKS))
    sd = torch.load(str(out / "association_head.pth"), map_location="cpu", weights_only=True)
    assert torch.equal(tracker.association_head.fc.weight, sd["fc.weight"])
    objs = tracker.next_frame(SyntheticSequence("static", 270, 480).frame(0))
    torch.cuda.synchronize()
    assert len(objs) >= 0
