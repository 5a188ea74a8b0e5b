"""SelectivePredictor -- counterpart of /root/reference/dcnn/engines/selective_predictor.py:11-51:
``predictor(bgr_u8) -> predictions`` (no feature dict) from ``SelectiveMaskRCNN.scan``."""
import torch

from ..config import is_c4
from ..networks.selective_rcnn import LAST_LEVEL_ONLY, SelectiveMaskRCNN
from .track_predictor import TrackPredictor


class SelectivePredictor(TrackPredictor):
    model_class = SelectiveMaskRCNN

    def __init__(self, cfg, state_dict=None):
        if is_c4(cfg):
            raise NotImplementedError("SelectivePredictor selects FPN levels (p6 only): not available for C4 (Res5ROIHeads) models")
        super().__init__(cfg, state_dict=state_dict)

    def __call__(self, original_image, upcoming=None):
        with torch.no_grad():
            insts, _ = self._predict([original_image], upcoming=upcoming, rpn_levels=LAST_LEVEL_ONLY)
            return {"instances": insts[0]}
