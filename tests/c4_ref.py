"""CPU reference of detectron2 0.1.2's C4 Mask R-CNN (Base-RCNN-C4 / Res5ROIHeads) for the C4 tests.

Composes what ``oracle/`` provides: ``DetectorOracle._conv`` / ``stem`` / ``bottleneck`` on a key-remapped state dict, and
``oracle.ops`` for anchors, box coding, NMS, ROIAlignV2 and mask pasting.  What C4 computes:
  * the image is normalised and NOT padded (size_divisibility 0); stem + res2..res4 -> res4 (stride 16);
  * StandardRPNHead on res4 (conv 3x3 + ReLU, 15 objectness, 60 deltas); anchors: sizes (32..512) x ratios (0.5, 1, 2), cell
    order size-major (a = 3 * size + ratio), flattening (H, W, A); top min(6000, H W 15) logits (ties: ascending index),
    decode, clip, nonempty, NMS 0.7, keep 1000;
  * Res5ROIHeads: ROIAlignV2 14x14 (1/16) on res4 -> res5 (first block stride 2 in its 1x1) -> mean over 7x7 -> predictor;
  * mask branch: ROIAlignV2 14x14 of the detections -> res5 -> deconv 2x2 + ReLU -> 1x1 predictor -> sigmoid (14x14 masks);
  * association: roi_pool 10x10 of res4 at the frame boxes, scale = res4 width / frame width.
"""
import torch
import torch.nn.functional as F

from oracle import ops
from oracle.detector import DetectorOracle

C4_SIZES = (32, 64, 128, 256, 512)
C4_RATIOS = (0.5, 1.0, 2.0)


def remap_c4_state(sd):
    """C4 keys -> the names DetectorOracle reads (backbone.X -> backbone.bottom_up.X); roi_heads.res5 stays."""
    out = {}
    for k, v in sd.items():
        if k.startswith("backbone."):
            out["backbone.bottom_up." + k[len("backbone."):]] = v
        else:
            out[k] = v
    return out


def c4_cell_anchors():
    """[15, 4]: DefaultAnchorGenerator with one group of five sizes, sizes outer, ratios inner."""
    return torch.cat([ops.cell_anchors(s, C4_RATIOS) for s in C4_SIZES])


def c4_grid_anchors(h, w, stride=16):
    """Anchors in (y, x, a) order, offset 0."""
    base = c4_cell_anchors()
    sx = torch.arange(0, w * stride, step=stride, dtype=torch.float32)
    sy = torch.arange(0, h * stride, step=stride, dtype=torch.float32)
    yy, xx = torch.meshgrid(sy, sx, indexing="ij")
    shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), dim=1)
    return (shifts.view(-1, 1, 4) + base.view(1, -1, 4)).reshape(-1, 4)


class C4Oracle(DetectorOracle):
    def __init__(self, state_dict, cfg=None):
        c = dict(size_divisibility=1, rpn_pre_topk=6000, rpn_post_topk=1000, mask_pool=14)
        c.update(cfg or {})
        super().__init__(remap_c4_state(state_dict), c)
        self.res5_blocks = 0
        while ("roi_heads.res5.%d.conv1.weight" % self.res5_blocks) in self.sd:
            self.res5_blocks += 1

    def backbone(self, x):
        feats = {}
        x = self.stem(x)
        feats["stem"] = x
        for si, nblk in enumerate(self.cfg["depth_blocks"][:3]):
            stage = "res%d" % (si + 2)
            for bi in range(nblk):
                x = self.bottleneck(x, "backbone.bottom_up.%s.%d" % (stage, bi), 2 if (bi == 0 and si > 0) else 1)
            feats[stage] = x
        return feats

    def res5(self, x):
        for bi in range(self.res5_blocks):
            x = self.bottleneck(x, "roi_heads.res5.%d" % bi, 2 if bi == 0 else 1)
        return x

    def rpn_c4(self, res4, image_size):
        c = self.cfg
        t = self._conv(res4, "proposal_generator.rpn_head.conv", padding=1, relu=True)
        lg = self._conv(t, "proposal_generator.rpn_head.objectness_logits")
        dl = self._conv(t, "proposal_generator.rpn_head.anchor_deltas")
        _, A, H, W = lg.shape
        lg_f = lg.permute(0, 2, 3, 1).reshape(-1)
        dl_f = dl.view(1, A, 4, H, W).permute(0, 3, 4, 1, 2).reshape(-1, 4)
        anchors = c4_grid_anchors(H, W)
        k = min(c["rpn_pre_topk"], lg_f.numel())
        order = torch.sort(lg_f, descending=True, stable=True).indices[:k]
        boxes = ops.clip_boxes(ops.apply_deltas(dl_f[order], anchors[order], (1.0, 1.0, 1.0, 1.0)), *image_size)
        scores = lg_f[order]
        keep = ops.nonempty(boxes, 0.0)
        bk, sk = boxes[keep], scores[keep]
        kept = ops.batched_nms(bk, sk, torch.zeros(bk.shape[0], dtype=torch.int64), c["rpn_nms"])
        kept_t = torch.from_numpy(kept[: c["rpn_post_topk"]])
        return dict(boxes=bk[kept_t], logits=sk[kept_t], n_anchors=lg_f.numel(), n_valid=int(keep.sum()), n_nms_kept=len(kept),
                    topk_idx=order, topk_scores=scores, decoded=boxes, valid=keep)

    def pooled(self, res4, boxes):
        if boxes.shape[0] == 0:
            return torch.zeros((0, res4.shape[1], 14, 14))
        return ops.roi_align_v2(res4[0], boxes, 1.0 / 16.0, 14)

    def box_features_c4(self, res4, proposals):
        x = self.res5(self.pooled(res4, proposals)).mean(dim=[2, 3])
        cls = F.linear(x, self.sd["roi_heads.box_predictor.cls_score.weight"], self.sd["roi_heads.box_predictor.cls_score.bias"])
        reg = F.linear(x, self.sd["roi_heads.box_predictor.bbox_pred.weight"], self.sd["roi_heads.box_predictor.bbox_pred.bias"])
        return dict(cls_logits=cls, deltas=reg)

    def mask_head_c4(self, res4, boxes, classes):
        n = boxes.shape[0]
        if n == 0:
            return dict(probs=torch.zeros((0, 14, 14)))
        x = self.res5(self.pooled(res4, boxes))
        x = F.relu(F.conv_transpose2d(x, self.sd["roi_heads.mask_head.deconv.weight"], self.sd["roi_heads.mask_head.deconv.bias"],
                                      stride=2))
        logits = self._conv(x, "roi_heads.mask_head.predictor")
        return dict(probs=logits.sigmoid()[torch.arange(n), classes])

    def inference(self, image_chw, out_h, out_w, given_boxes=None, given_classes=None, rpn_levels=None):
        image_size = tuple(image_chw.shape[-2:])
        feats = self.backbone(self.preprocess(image_chw))
        res4 = feats["res4"]
        prop = None
        if given_boxes is None:
            prop = self.rpn_c4(res4, image_size)
            bf = self.box_features_c4(res4, prop["boxes"])
            det = self.box_inference(bf["cls_logits"], bf["deltas"], prop["boxes"], image_size)
            boxes, scores, classes = det["boxes"], det["scores"], det["classes"]
        else:
            det = None
            boxes = given_boxes.to(torch.float32)
            classes = given_classes.to(torch.int64)
            scores = torch.ones((boxes.shape[0],), dtype=torch.float32)
        mh = self.mask_head_c4(res4, boxes, classes)
        post = self.postprocess(boxes, scores, classes, mh["probs"], image_size, out_h, out_w)
        post.update(features=feats, proposals=prop, box_det=det, image_size=image_size)
        return post
