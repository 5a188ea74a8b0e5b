#!/usr/bin/env python
"""Fine-tune the RPN head and the box branch of a detector jointly on the GPU -- dcnn/scripts/train/finetune_uav.py and
finetune_faster_rcnn_aerial.py with ``to_train=['proposal_generator', 'roi_heads']``: one loop, one optimiser.

Everything is frozen except ``proposal_generator.rpn_head.{conv,objectness_logits,anchor_deltas}``, ``roi_heads.box_head.fc{1,2}``
and ``roi_heads.box_predictor.{cls_score,bbox_pred}`` (14 tensors).  Per step and image the frozen backbone runs once; the anchors
are labelled and sampled as ``RPNOutputs._get_ground_truth`` does (256 per image); the box head's proposals come from the RPN
head AS IT IS AT THAT STEP, selected with detectron2's training limits (2000 per level before NMS, 1000 after), the ground truths
are appended, and 512 per image are sampled as ``ROIHeads.label_and_sample_proposals`` does.  ``loss_rpn_cls + loss_rpn_loc +
loss_cls + loss_box_reg`` is optimised with one momentum SGD under detectron2's WarmupMultiStepLR, and after every optimiser step
the new RPN head is written into the live detector contexts (``TrackRCNN.set_rpn_head``: no rebuild).  At most 4 images per batch
(4 x 256 RPN rows is one step's limit); their up to 2048 box rows go through the box head in chunks of whole images
(utils/joint_train.py box_losses_chunked).  Every CHECKPOINT_PERIOD iterations the held-out images are scored (bbox AP / AR, and
the recall of the proposals at 100 and 1000) and a checkpoint with the merged full detector is written.

  python tools/finetune_uav.py --images DIR --annotations FILE.json --weights detector.pth --classes car truck bus --out DIR
  python tools/finetune_uav.py --synthetic 6 --iters 12 --checkpoint-period 4 --out DIR     # dry run on generated data
  python tools/finetune_uav.py ... --resume                                                 # continue from DIR/<name>_last.pth

Checkpoint keys: model, optimizer, scheduler, iteration, kfold_split, k_folds, best_precision, best_recall, training_results,
loader (the image order, the augmentation draws and both sampling generators), so that a resumed run repeats the uninterrupted
one bit for bit.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RESULTS_FILE = "results.txt"
HEADER = "\t\tAP\tAP_05\tAP0.75\tAP_s\tAP_m\tAP_l\tAR_1\tAR_10\tAR_100\tAR_s\tAR_m\tAR_l\tprop_AR@100\tprop_AR@1000\n"
MAX_IMS = 4


def merged_state(detector, rpn_head, box_head):
    from apse_uav_amd.networks.box_head import merge_box_head
    from apse_uav_amd.networks.rpn_head import merge_rpn_head
    return merge_box_head(merge_rpn_head(detector, rpn_head.state_dict()), box_head.state_dict())


def do_test(pred, dicts, coco_gt):
    """The 12 bbox COCOeval numbers (zeros when nothing was detected) followed by the proposal recall at 100 and 1000 (IoU 0.5)
    of the predictor on ``dicts``; None when there is no ground truth."""
    import finetune_box_head
    import finetune_rpn
    recall = finetune_rpn.do_test(pred, dicts)
    if recall is None:
        return None
    ap = finetune_box_head.do_test(pred, dicts, coco_gt)
    return (ap if ap is not None else [0.0] * 12) + recall


def main(argv=None):
    from finetune_box_head import adapt_detector
    from finetune_segmentation import holdout_split
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", default="")
    ap.add_argument("--annotations", default="")
    ap.add_argument("--weights", default="", help="detector (.pth / converted model-zoo file); its two heads are the start")
    ap.add_argument("--classes", nargs="*", default=None, help="category names to train on (default: all)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="R_50_FPN_UAV")
    ap.add_argument("--iters", type=int, default=20000, help="MAX_ITER")
    ap.add_argument("--checkpoint-period", type=int, default=10)
    ap.add_argument("--ims-per-batch", type=int, default=2, help="at most %d, the reference yaml's value" % MAX_IMS)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--steps", type=int, nargs="*", default=[30000])
    ap.add_argument("--gamma", type=float, default=0.1)
    ap.add_argument("--warmup-iters", type=int, default=1000)
    ap.add_argument("--warmup-factor", type=float, default=0.001)
    ap.add_argument("--optimizer", choices=("apse", "torch"), default="apse", help="apse_uav_amd.optim.SGD (HIP) or torch.optim.SGD")
    ap.add_argument("--k-folds", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--flip", action="store_true", help="random horizontal flip")
    ap.add_argument("--augment", action="store_true",
                    help="the reference mapper's colour chain on the GPU: random brightness, saturation, contrast (0.9 .. 1.1 each) "
                         "and lighting (0.2); the held-out images stay unaugmented")
    ap.add_argument("--min-sizes", default="", metavar="S1,S2,...",
                    help="multi-scale training: the short edge of every training image is drawn from these sizes "
                         "(default: the test size)")
    ap.add_argument("--max-size", type=int, default=0, help="cap of the long edge with --min-sizes / --augment (default: the test one)")
    ap.add_argument("--stop-at", type=int, default=0, help="stop after this iteration's checkpoint (an interrupted run, for --resume)")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--test-on-train", action="store_true", help="score the training images instead of the held-out ones")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    args = ap.parse_args(argv)
    if not 1 <= args.ims_per_batch <= MAX_IMS:
        ap.error("--ims-per-batch must be 1 .. %d (%d x 256 RPN rows is the limit of one step)" % (MAX_IMS, MAX_IMS))

    import torch
    from apse_uav_amd import optim
    from apse_uav_amd.config import is_c4, setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.networks.box_head import BoxHead
    from apse_uav_amd.networks.rpn_head import RPNHead
    from apse_uav_amd.utils import COCO_utils
    from apse_uav_amd.utils.coco import COCO
    from apse_uav_amd.utils.joint_train import JointTrainLoader, box_losses_chunked
    from apse_uav_amd.weights import load_detector_file, synthetic_detector_state

    os.makedirs(args.out, exist_ok=True)
    if args.synthetic:
        from eval_detector import synthetic_dataset
        args.images = os.path.join(args.out, "synthetic")
        args.annotations = synthetic_dataset(args.images, args.synthetic)
        detector = synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)
    elif args.images and args.annotations and args.weights:
        detector = load_detector_file(args.weights)
    else:
        ap.error("--images, --annotations and --weights are required (or --synthetic N)")

    dicts = COCO_utils.generate_coco_dataset_dictionaries(args.annotations, args.images, args.classes, None, False)
    have = int(detector["roi_heads.box_predictor.cls_score.weight"].shape[0]) - 1
    K = len(args.classes) if args.classes else have
    if max(a["category_id"] for d in dicts for a in d["annotations"]) >= K:
        raise ValueError("the annotations map to more classes than the %d being trained" % K)
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    # the loop alternates between images of several sizes and every size has a context of its own: keep a few alive
    cfg.APSE.CONTEXT_CACHE = max(int(cfg.APSE.get("CONTEXT_CACHE", 1)), 4)
    if is_c4(cfg):
        raise NotImplementedError("joint detection-head training covers FPN models")
    last_path = os.path.join(args.out, args.name + "_last.pth")
    results_path = os.path.join(args.out, RESULTS_FILE)

    torch.manual_seed(args.seed)
    detector, changed = adapt_detector(detector, K)
    rpn_head = RPNHead.from_cfg(cfg, "cuda")
    rpn_head.load_state_dict(detector)
    box_head = BoxHead(K, "cuda")
    box_head.load_state_dict(detector, keep_predictor=changed)      # another class count: fc1 / fc2 only, fresh predictors
    params = list(rpn_head.parameters()) + list(box_head.parameters())
    if args.optimizer == "torch":
        opt = torch.optim.SGD(params, lr=args.lr, momentum=args.momentum)
    else:
        opt = optim.SGD(params, lr=args.lr, momentum=args.momentum)
    sched = optim.WarmupMultiStepLR(opt, args.steps, args.gamma, args.warmup_factor, args.warmup_iters)
    start_iter, best_p, best_r = 0, 0.0, 0.0
    chk = None
    if args.resume:
        chk = torch.load(last_path, map_location="cpu", weights_only=False)
        detector = {k: v for k, v in chk["model"].items()}           # the frozen part as the interrupted run had it
        rpn_head.load_state_dict(chk["model"])
        box_head.load_state_dict(chk["model"])
        opt.load_state_dict(chk["optimizer"])
        sched.load_state_dict(chk["scheduler"])
        start_iter = int(chk["iteration"]) + 1
        split, k_folds = chk["kfold_split"], chk["k_folds"]
        best_p, best_r = chk["best_precision"], chk["best_recall"]
        with open(results_path, "w") as fh:
            fh.write(chk["training_results"])
    else:
        k_folds = args.k_folds
        split = holdout_split(len(dicts), k_folds, args.seed)
        with open(results_path, "w") as fh:
            fh.write(HEADER)
    train_ids, test_ids = split
    train_dicts = [dicts[i] for i in train_ids]
    test_dicts = train_dicts if args.test_on_train else [dicts[i] for i in test_ids]
    gt = COCO.from_dataset(COCO_utils.detectron2_dataset_to_coco(test_dicts), verbose=False)

    pred = TrackPredictor(cfg, state_dict=merged_state(detector, rpn_head, box_head))
    min_sizes = tuple(int(v) for v in args.min_sizes.split(",")) if args.min_sizes else None
    loader = JointTrainLoader(train_dicts, pred.model, args.ims_per_batch, args.seed, args.flip, augment=args.augment,
                              min_sizes=min_sizes, max_size=args.max_size or None, num_classes=K)
    if chk is not None:
        loader.load_state_dict(chk["loader"])

    def push_heads():
        """Both heads into the predictor: the box branch rebuilds the contexts (from a state that holds the current RPN head)."""
        pred.model.set_rpn_head(rpn_head)
        box_head.push_into(pred)

    names = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg")
    summary = {"losses": [], "tests": [], "num_classes": K}
    summary["before"] = do_test(pred, test_dicts, gt) if not args.resume else None
    print("Training for {} iterations started".format(args.iters))
    for iteration in range(start_iter, args.iters):
        rpn, box = next(loader)
        losses = dict(rpn_head(*rpn, args.ims_per_batch))
        losses.update(box_losses_chunked(box_head, *box, loader.last_box_rows))
        loss = losses["loss_rpn_cls"] + losses["loss_rpn_loc"] + losses["loss_cls"] + losses["loss_box_reg"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        pred.model.set_rpn_head(rpn_head)                            # the next step's proposals come from this head
        summary["losses"].append(tuple(float(losses[k].detach()) for k in names))
        print("Iter. {}/{}:\t".format(iteration, args.iters) + "\t".join("{}: {}".format(k, v) for k, v in zip(names, summary["losses"][-1]))
              + "\tpos/neg: {}\tfg/bg: {}".format(loader.last_rpn_counts, loader.last_box_counts))
        if iteration != 0 and iteration % args.checkpoint_period == 0:
            push_heads()
            res = do_test(pred, test_dicts, gt)
            print("test results:", res)
            if res is not None:
                line = "{}/{}:\t".format(iteration, args.iters) + "\t".join("{:.3f}".format(v) for v in res)
                if res[0] > best_p:
                    best_p = res[0]
                    line += " Best precision!"
                if res[12] > best_r:
                    best_r = res[12]
                    line += " Best recall!"
                with open(results_path, "a") as fh:
                    fh.write(line + "\n")
                summary["tests"].append((iteration, res))
            with open(results_path) as fh:
                chkpt = {"model": merged_state(detector, rpn_head, box_head), "optimizer": opt.state_dict(),
                         "scheduler": sched.state_dict(), "iteration": iteration, "kfold_split": split, "k_folds": k_folds,
                         "best_precision": best_p, "best_recall": best_r, "training_results": fh.read(),
                         "loader": loader.state_dict()}
            torch.save(chkpt, last_path)
            if res is None or res[0] == best_p or not os.path.exists(os.path.join(args.out, args.name + "_bestAP.pth")):
                torch.save(chkpt, os.path.join(args.out, args.name + "_bestAP.pth"))
            if res is None or res[12] == best_r or not os.path.exists(os.path.join(args.out, args.name + "_bestAR.pth")):
                torch.save(chkpt, os.path.join(args.out, args.name + "_bestAR.pth"))
            if args.stop_at and iteration >= args.stop_at:
                break
    push_heads()
    summary["after"] = do_test(pred, test_dicts, gt)
    summary["checkpoint"] = last_path
    summary["state"] = {k: v.cpu() for k, v in list(rpn_head.state_dict("proposal_generator.rpn_head.").items())
                        + list(box_head.state_dict("roi_heads.").items())}
    summary["predictor"] = pred
    return summary


if __name__ == "__main__":
    main()
