"""Configuration node for the dcnn hot path.

The reference configures the path through detectron2's yacs ``CfgNode``
(/root/reference/dcnn/scripts/tests/visualize_uav.py:43-53 ``setup_cfg``;
YAML files dcnn/configs/Base-RCNN-FPN.yaml, dcnn/configs/mask_rcnn_R_101_FPN_3x.yaml).
yacs/detectron2 are not dependencies of this build, so this module provides a
small attribute-style node with the same surface the engines use
(``get_cfg``, ``merge_from_file`` with ``_BASE_``, ``clone``, ``freeze``) and only
the keys that define results on this path.
"""
import copy
import os

import yaml


class CfgNode(dict):
    def __init__(self, init=None):
        super().__init__()
        self.__dict__["_frozen"] = False
        for k, v in (init or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        if self.__dict__.get("_frozen"):
            raise AttributeError("attempt to modify frozen CfgNode key %r" % k)
        self[k] = v

    def freeze(self):
        self.__dict__["_frozen"] = True
        for v in self.values():
            if isinstance(v, CfgNode):
                v.freeze()

    def defrost(self):
        self.__dict__["_frozen"] = False
        for v in self.values():
            if isinstance(v, CfgNode):
                v.defrost()

    def clone(self):
        c = CfgNode(copy.deepcopy(_plain(self)))
        return c

    def _merge(self, other):
        for k, v in other.items():
            if isinstance(v, dict) and isinstance(self.get(k), CfgNode):
                self[k]._merge(v)
            else:
                self[k] = CfgNode(v) if isinstance(v, dict) else (tuple(v) if isinstance(v, list) else v)

    def merge_from_file(self, path):
        data = _load_yaml_chain(path)
        # a C4 YAML (Base-RCNN-C4 sets ROI_HEADS.NAME: Res5ROIHeads) switches every FPN default this path reads to detectron2's
        # C4 one first, so keys the YAML chain leaves alone do not stay FPN values (no FPN/C4 hybrid); the chain then wins
        if (data.get("MODEL", {}).get("ROI_HEADS", {}).get("NAME") == C4_ROI_HEADS and "MODEL" in self
                and not is_c4(self)):
            _apply_c4_defaults(self)
        self._merge(data)

    def merge_from_list(self, kv):
        for k, v in zip(kv[0::2], kv[1::2]):
            node = self
            parts = k.split(".")
            for p in parts[:-1]:
                node = node[p]
            node[parts[-1]] = v


def _deep_update(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _deep_update(dst[k], v)
        else:
            dst[k] = v
    return dst


def _load_yaml_chain(path):
    """A YAML file with its ``_BASE_`` chain resolved into one nested dict (the file's keys over its base's)."""
    with open(path) as f:
        data = yaml.safe_load(f) or {}
    base = data.pop("_BASE_", None)
    if not base:
        return data
    if not os.path.isabs(base):
        base = os.path.join(os.path.dirname(path), base)
    return _deep_update(_load_yaml_chain(base), data)


def _plain(n):
    return {k: (_plain(v) if isinstance(v, CfgNode) else v) for k, v in n.items()}


def get_cfg():
    """detectron2 0.1.2 defaults for the keys this path reads, with the R-101-FPN mask
    settings of the reference YAMLs already merged (so no YAML file is needed)."""
    return CfgNode({
        "VERSION": 2,
        "MODEL": {
            "DEVICE": "cuda",
            "META_ARCHITECTURE": "GeneralizedRCNN",
            "WEIGHTS": "",
            "MASK_ON": True,
            "PIXEL_MEAN": (103.530, 116.280, 123.675),
            "PIXEL_STD": (1.0, 1.0, 1.0),
            "BACKBONE": {"NAME": "build_resnet_fpn_backbone"},
            "RESNETS": {"DEPTH": 101, "OUT_FEATURES": ("res2", "res3", "res4", "res5"),
                        "STRIDE_IN_1X1": True, "NORM": "FrozenBN", "RES2_OUT_CHANNELS": 256, "STEM_OUT_CHANNELS": 64},
            "FPN": {"IN_FEATURES": ("res2", "res3", "res4", "res5"), "OUT_CHANNELS": 256, "FUSE_TYPE": "sum", "NORM": ""},
            "ANCHOR_GENERATOR": {"SIZES": ((32,), (64,), (128,), (256,), (512,)),
                                 "ASPECT_RATIOS": ((0.5, 1.0, 2.0),), "OFFSET": 0.0},
            "RPN": {"IN_FEATURES": ("p2", "p3", "p4", "p5", "p6"), "PRE_NMS_TOPK_TEST": 1000,
                    "POST_NMS_TOPK_TEST": 1000, "NMS_THRESH": 0.7, "BBOX_REG_WEIGHTS": (1.0, 1.0, 1.0, 1.0),
                    "MIN_SIZE": 0,
                    # the reference's Base-RCNN-FPN.yaml; read by the training path only (TrackRCNN.train_proposals)
                    "PRE_NMS_TOPK_TRAIN": 2000, "POST_NMS_TOPK_TRAIN": 1000},
            "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": ("p2", "p3", "p4", "p5"), "NUM_CLASSES": 80,
                          "SCORE_THRESH_TEST": 0.05, "NMS_THRESH_TEST": 0.5},
            "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "FC_DIM": 1024, "POOLER_RESOLUTION": 7,
                             "POOLER_SAMPLING_RATIO": 0, "POOLER_TYPE": "ROIAlignV2",
                             "BBOX_REG_WEIGHTS": (10.0, 10.0, 5.0, 5.0)},
            "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 4, "CONV_DIM": 256,
                              "POOLER_RESOLUTION": 14, "POOLER_SAMPLING_RATIO": 0, "POOLER_TYPE": "ROIAlignV2"},
        },
        # the *_TRAIN keys are detectron2's defaults; the reference's Base-RCNN-FPN.yaml, when merged, gives
        # MIN_SIZE_TRAIN (640, 672, 704, 736, 768, 800)
        "INPUT": {"MIN_SIZE_TEST": 800, "MAX_SIZE_TEST": 1333, "FORMAT": "BGR", "MIN_SIZE_TRAIN": (800,), "MAX_SIZE_TRAIN": 1333,
                  "MIN_SIZE_TRAIN_SAMPLING": "choice"},
        "TEST": {"DETECTIONS_PER_IMAGE": 100},
        "DATASETS": {"TRAIN": ("coco_2017_train",), "TEST": ("coco_2017_val",)},
        # build-specific knobs (not in the reference): storage dtype and batch of the HIP path
        # CONTEXT_CACHE: live contexts TrackRCNN keeps, one per (frame size, image size); 1 = rebuild at every size change
        # TAIL_LANE: a forward's selection / heads / results copy on the context's second stream, beside the next frame's trunk
        # (apse_config.tail_lane; the environment variable APSE_TAIL_LANE=0 switches it off for every context)
        # YUV_MATRIX: the conversion of INPUT.FORMAT "NV12" / "I420" frames (structures/yuv_frame.py): cv601 (OpenCV's
        # COLOR_YUV2BGR_NV12 constants), bt601, bt709, bt601-full, bt709-full
        # CROP_FEATURES: the association head's RoI features are cut from p2 * the instance mask with roi_align (the reference's
        # crop_features=True branch, rcnn_tracker.py:166-180) instead of roi_pool at the box (apse_set_crop_features; FPN only)
        "APSE": {"DTYPE": "f32", "MAX_BATCH": 1, "FUSED_PREPROC": True, "STORAGE16": True, "CONTEXT_CACHE": 1, "TAIL_LANE": True,
                 "YUV_MATRIX": "cv601", "CROP_FEATURES": False},
    })


C4_ROI_HEADS = "Res5ROIHeads"
C4_ANCHOR_SIZES = ((32, 64, 128, 256, 512),)
C4_ANCHOR_RATIOS = ((0.5, 1.0, 2.0),)


def is_c4(cfg):
    """True for a C4 model (detectron2 Base-RCNN-C4: ``MODEL.ROI_HEADS.NAME == "Res5ROIHeads"``)."""
    return cfg.MODEL.ROI_HEADS.NAME == C4_ROI_HEADS


def _apply_c4_defaults(cfg):
    """detectron2 0.1.2's values, for a C4 model, of the keys this path reads (Base-RCNN-C4.yaml over the library defaults)."""
    m = cfg.MODEL
    m.BACKBONE.NAME = "build_resnet_backbone"
    m.RESNETS.OUT_FEATURES = ("res4",)
    m.RESNETS.RES5_DILATION = 1
    m.ANCHOR_GENERATOR.SIZES = C4_ANCHOR_SIZES
    m.ANCHOR_GENERATOR.ASPECT_RATIOS = C4_ANCHOR_RATIOS
    m.RPN.IN_FEATURES = ("res4",)
    m.RPN.PRE_NMS_TOPK_TEST = 6000
    m.RPN.POST_NMS_TOPK_TEST = 1000
    m.ROI_HEADS.NAME = C4_ROI_HEADS
    m.ROI_HEADS.IN_FEATURES = ("res4",)
    m.ROI_BOX_HEAD.NAME = ""
    m.ROI_BOX_HEAD.NUM_FC = 0
    m.ROI_BOX_HEAD.POOLER_RESOLUTION = 14
    m.ROI_MASK_HEAD.NUM_CONV = 0
    m.ROI_MASK_HEAD.POOLER_RESOLUTION = 14


def check_c4_supported(cfg):
    """Refuses C4 settings the HIP path does not restate (raises ValueError)."""
    m = cfg.MODEL
    if tuple(tuple(s) for s in m.ANCHOR_GENERATOR.SIZES) != C4_ANCHOR_SIZES or \
            tuple(tuple(r) for r in m.ANCHOR_GENERATOR.ASPECT_RATIOS) != C4_ANCHOR_RATIOS or \
            float(m.ANCHOR_GENERATOR.get("OFFSET", 0.0)) != 0.0:
        raise ValueError("C4: only detectron2's default anchors are supported (sizes %s, ratios %s, offset 0)"
                         % (C4_ANCHOR_SIZES, C4_ANCHOR_RATIOS))
    if int(m.RESNETS.get("RES5_DILATION", 1)) != 1:
        raise ValueError("C4: RES5_DILATION 2 is not supported")
    if not m.MASK_ON:
        raise ValueError("C4: box-only models (MASK_ON False) are not supported")
    if tuple(m.RPN.IN_FEATURES) != ("res4",) or tuple(m.ROI_HEADS.IN_FEATURES) != ("res4",):
        raise ValueError("C4: the RPN and the ROI heads read res4")
    if int(m.ROI_BOX_HEAD.POOLER_RESOLUTION) != 14 or int(m.ROI_MASK_HEAD.POOLER_RESOLUTION) != 14 or \
            int(m.ROI_MASK_HEAD.NUM_CONV) != 0:
        raise ValueError("C4: pooler resolution 14 and no mask convolutions (NUM_CONV 0) are required")


CLASSES_NAMES = ["car", "truck", "bus", "person"]          # visualize_uav.py:31


def setup_cfg(weights="", score_thresh=0.5, num_classes=4, device="cuda", arch="FPN"):
    """Counterpart of visualize_uav.py:43-53.  ``arch="C4"``: detectron2's C4 values (Base-RCNN-C4) for a
    Res5ROIHeads checkpoint such as mask_rcnn_R_50_C4_3x."""
    if arch not in ("FPN", "C4"):
        raise ValueError("arch must be 'FPN' or 'C4'")
    cfg = get_cfg()
    if arch == "C4":
        _apply_c4_defaults(cfg)
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = score_thresh
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = num_classes
    cfg.MODEL.WEIGHTS = weights
    cfg.MODEL.MASK_ON = True
    cfg.MODEL.DEVICE = device
    return cfg
