#!/usr/bin/env python
"""Fine-tune the RPN head of a detector on the GPU -- the ``proposal_generator`` half of dcnn/scripts/train/finetune_uav.py and
finetune_faster_rcnn_aerial.py.

Everything is frozen except ``proposal_generator.rpn_head.{conv,objectness_logits,anchor_deltas}``; the anchors of p2 .. p6 are
labelled against the ground-truth boxes and sampled as detectron2's ``RPNOutputs._get_ground_truth`` does (IoU 0.3 / 0.7 with
low-quality matches, 256 per image, half positive); ``loss_rpn_cls + loss_rpn_loc`` is optimised with momentum SGD under
detectron2's WarmupMultiStepLR; every CHECKPOINT_PERIOD iterations the recall of the detector's proposals on the held-out images
(at 100 and at 1000 proposals, IoU 0.5) is written to results.txt and a checkpoint with the merged full detector is written.
``--classes`` only filters the annotations: the RPN is class-agnostic and the detector keeps its class count.  Run
tools/finetune_box_head.py on the resulting checkpoint to adapt the box head to the new proposals.

  python tools/finetune_rpn.py --images DIR --annotations FILE.json --weights detector.pth --out DIR
  python tools/finetune_rpn.py --synthetic 6 --iters 12 --checkpoint-period 4 --out DIR     # dry run on generated data
  python tools/finetune_rpn.py ... --resume                                                 # continue from DIR/<name>_last.pth

Checkpoint keys: model, optimizer, scheduler, iteration, kfold_split, k_folds, best_recall, training_results, loader (the image
order, the augmentation draws and the sampling generator), so that a resumed run repeats the uninterrupted one bit for bit.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RESULTS_FILE = "results.txt"
HEADER = "\t\tAR@100\tAR@1000\n"
LIMITS = (100, 1000)


def do_test(pred, dicts):
    """[recall@100, recall@1000] (IoU 0.5) of the predictor's proposals on ``dicts``; None when there is no ground truth."""
    from apse_uav_amd.utils.rpn_train import proposal_recall
    res = proposal_recall(pred.model, dicts, 0.5, LIMITS)
    return None if res is None else [float(res[k]) for k in LIMITS]


def main(argv=None):
    from finetune_segmentation import holdout_split
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", default="")
    ap.add_argument("--annotations", default="")
    ap.add_argument("--weights", default="", help="detector (.pth / converted model-zoo file); its RPN head is the start")
    ap.add_argument("--classes", nargs="*", default=None, help="category names whose annotations are used (default: all)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="R_50_FPN_UAV_RPN")
    ap.add_argument("--iters", type=int, default=20000, help="MAX_ITER")
    ap.add_argument("--checkpoint-period", type=int, default=10)
    ap.add_argument("--ims-per-batch", type=int, default=2)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--steps", type=int, nargs="*", default=[30000])
    ap.add_argument("--gamma", type=float, default=0.1)
    ap.add_argument("--warmup-iters", type=int, default=1000)
    ap.add_argument("--warmup-factor", type=float, default=0.001)
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

    import torch
    from apse_uav_amd import optim
    from apse_uav_amd.config import is_c4, setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.networks.rpn_head import RPNHead, merge_rpn_head
    from apse_uav_amd.utils import COCO_utils
    from apse_uav_amd.utils.rpn_train import RpnTrainLoader
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
    K = int(detector["roi_heads.box_predictor.cls_score.weight"].shape[0]) - 1
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    # the loop alternates between images of several sizes and every size has a context of its own: keep a few alive
    cfg.APSE.CONTEXT_CACHE = max(int(cfg.APSE.get("CONTEXT_CACHE", 1)), 4)
    if is_c4(cfg):
        raise NotImplementedError("RPN-head training covers FPN models")
    last_path = os.path.join(args.out, args.name + "_last.pth")
    results_path = os.path.join(args.out, RESULTS_FILE)

    torch.manual_seed(args.seed)
    head = RPNHead.from_cfg(cfg, "cuda")
    head.load_state_dict(detector)
    params = list(head.parameters())
    opt = optim.SGD(params, lr=args.lr, momentum=args.momentum)
    sched = optim.WarmupMultiStepLR(opt, args.steps, args.gamma, args.warmup_factor, args.warmup_iters)
    start_iter, best_r = 0, 0.0
    chk = None
    if args.resume:
        chk = torch.load(last_path, map_location="cpu", weights_only=False)
        detector = {k: v for k, v in chk["model"].items()}           # the frozen part as the interrupted run had it
        head.load_state_dict(chk["model"])
        opt.load_state_dict(chk["optimizer"])
        sched.load_state_dict(chk["scheduler"])
        start_iter = int(chk["iteration"]) + 1
        split, k_folds = chk["kfold_split"], chk["k_folds"]
        best_r = chk["best_recall"]
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

    pred = TrackPredictor(cfg, state_dict=merge_rpn_head(detector, head.state_dict()))
    min_sizes = tuple(int(v) for v in args.min_sizes.split(",")) if args.min_sizes else None
    loader = RpnTrainLoader(train_dicts, pred.model, args.ims_per_batch, args.seed, args.flip, augment=args.augment,
                            min_sizes=min_sizes, max_size=args.max_size or None)
    if chk is not None:
        loader.load_state_dict(chk["loader"])

    summary = {"losses": [], "tests": []}
    summary["recall_before"] = do_test(pred, test_dicts) if not args.resume else None
    print("Training for {} iterations started".format(args.iters))
    for iteration in range(start_iter, args.iters):
        patches, slots, labels, anchor_boxes, gt_boxes = next(loader)
        losses = head(patches, slots, labels, anchor_boxes, gt_boxes, args.ims_per_batch)
        loss = losses["loss_rpn_cls"] + losses["loss_rpn_loc"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        summary["losses"].append((float(losses["loss_rpn_cls"].detach()), float(losses["loss_rpn_loc"].detach())))
        print("Iter. {}/{}:\tloss_rpn_cls: {}\tloss_rpn_loc: {}\tpos/neg: {}".format(iteration, args.iters, summary["losses"][-1][0],
                                                                                   summary["losses"][-1][1], loader.last_counts))
        if iteration != 0 and iteration % args.checkpoint_period == 0:
            head.push_into(pred)
            res = do_test(pred, test_dicts)
            print("test results:", res)
            if res is not None:
                line = "{}/{}:\t".format(iteration, args.iters) + "\t".join("{:.3f}".format(v) for v in res)
                if res[0] > best_r:
                    best_r = res[0]
                    line += " Best recall!"
                with open(results_path, "a") as fh:
                    fh.write(line + "\n")
                summary["tests"].append((iteration, res))
            with open(results_path) as fh:
                chkpt = {"model": merge_rpn_head(detector, head.state_dict()), "optimizer": opt.state_dict(),
                         "scheduler": sched.state_dict(), "iteration": iteration, "kfold_split": split, "k_folds": k_folds,
                         "best_recall": best_r, "training_results": fh.read(), "loader": loader.state_dict()}
            torch.save(chkpt, last_path)
            if res is None or res[0] == best_r or not os.path.exists(os.path.join(args.out, args.name + "_bestAR.pth")):
                torch.save(chkpt, os.path.join(args.out, args.name + "_bestAR.pth"))
            if args.stop_at and iteration >= args.stop_at:
                break
    head.push_into(pred)
    summary["recall_after"] = do_test(pred, test_dicts)
    summary["checkpoint"] = last_path
    summary["state"] = {k: v.cpu() for k, v in head.state_dict().items()}
    summary["predictor"] = pred
    return summary


if __name__ == "__main__":
    main()
