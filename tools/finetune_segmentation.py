#!/usr/bin/env python
"""Fine-tune the mask head of a box detector on the GPU -- counterpart of dcnn/scripts/train/finetune_segmentation.py.

Everything is frozen except ``roi_heads.mask_head.*``; the ground-truth boxes are the proposals; ``loss_mask`` is optimised with
momentum SGD (lr 0.02, momentum 0.9) under detectron2's WarmupMultiStepLR; every CHECKPOINT_PERIOD iterations the held-out
images are scored (segm AP / AR, ground-truth boxes and classes given to the detector with score 1) and a checkpoint with the
merged full detector is written.  The reference passes the boxes through its box head as proposals; this project has no
proposals-given box head, so the boxes go straight to the mask branch (``detected_instances``).

  python tools/finetune_segmentation.py --images DIR --annotations FILE.json --weights detector.pth --classes car truck bus person --out DIR
  python tools/finetune_segmentation.py --synthetic 12 --iters 40 --out DIR          # dry run on generated data, seeded weights
  python tools/finetune_segmentation.py ... --resume                                 # continue from DIR/<name>_last.pth

Checkpoint keys (the reference's): model, optimizer, scheduler, iteration, kfold_split, k_folds, best_precision, best_recall,
training_results -- plus ``loader`` (the sampling state) so that a resumed run repeats the uninterrupted one bit for bit.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RESULTS_FILE = "results.txt"
HEADER = "\t\tAP\tAP_05\tAP0.75\tAP_s\tAP_m\tAP_l\tAR_1\tAR_10\tAR_100\tAR_s\tAR_m\tAR_l\n"


def holdout_split(n, k_folds, seed):
    """First fold of a seeded shuffle split into ``k_folds`` parts (the reference takes KFold(shuffle=True)'s first fold):
    (train indices, test indices), both sorted."""
    k = max(2, min(int(k_folds), n))
    order = np.random.default_rng(seed).permutation(n)
    n_test = max(1, n // k)
    return sorted(int(i) for i in order[n_test:]), sorted(int(i) for i in order[:n_test])


def do_test(pred, dicts, coco_gt):
    """segm COCOeval stats (12 numbers) of the predictor's masks for the ground-truth boxes and classes of ``dicts``; None
    when there is nothing to score."""
    import torch
    from PIL import Image
    from apse_uav_amd.utils import resample
    from apse_uav_amd.utils.coco_eval import CocoEvaluator
    ev = CocoEvaluator(coco_gt)
    total = 0
    cap = int(pred.cfg.TEST.DETECTIONS_PER_IMAGE)
    for d in dicts:
        frame = np.asarray(Image.open(d["file_name"]).convert("RGB"))[:, :, ::-1].copy()
        H, W = frame.shape[:2]
        ih, iw = resample.resize_shortest_edge(H, W, pred.cfg.INPUT.MIN_SIZE_TEST, pred.cfg.INPUT.MAX_SIZE_TEST)
        anns = d["annotations"][:cap]
        b = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in anns],
                     np.float64).reshape(-1, 4) * np.array([iw / W, ih / H, iw / W, ih / H])
        classes = np.array([a["category_id"] for a in anns], np.int32)
        with torch.no_grad():
            insts, _ = pred.model.inference_frames(torch.from_numpy(frame[None]).to(pred.model.device),
                                                   given=(b.astype(np.float32), classes, np.array([len(anns)], np.int32)))
        ev.add(d["image_id"], insts[0])
        total += len(insts[0])
    if total == 0:
        return None
    return [float(v) for v in ev.evaluate("segm").stats]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", default="")
    ap.add_argument("--annotations", default="")
    ap.add_argument("--weights", default="", help="box detector (.pth / converted model-zoo file); its mask head, if any, is the start")
    ap.add_argument("--classes", nargs="*", default=None, help="category names to train on (default: all)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="R_50_FPN_UAV_SEGM")
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
                    help="multi-scale training: the short edge of every training image is drawn from these sizes, e.g. "
                         "640,672,704,736,768,800 (default: the test size)")
    ap.add_argument("--max-size", type=int, default=0, help="cap of the long edge with --min-sizes / --augment (default: the test one)")
    ap.add_argument("--cache-features", action="store_true")
    ap.add_argument("--stop-at", type=int, default=0, help="stop after this iteration's checkpoint (an interrupted run, for --resume)")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--test-on-train", action="store_true", help="score the training images instead of the held-out ones")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    args = ap.parse_args(argv)

    import torch
    from apse_uav_amd import optim
    from apse_uav_amd.config import is_c4, setup_cfg
    from apse_uav_amd.engines.track_predictor import TrackPredictor
    from apse_uav_amd.networks.mask_head import PREFIX, MaskHead, merge_full_mask_rcnn
    from apse_uav_amd.utils import COCO_utils
    from apse_uav_amd.utils.coco import COCO
    from apse_uav_amd.weights import load_detector_file, synthetic_detector_state

    os.makedirs(args.out, exist_ok=True)
    if args.synthetic:
        from eval_detector import synthetic_dataset
        args.images = os.path.join(args.out, "synthetic")
        args.annotations = synthetic_dataset(args.images, args.synthetic)
        detector = synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)
        detector = {k: v for k, v in detector.items() if not k.startswith(PREFIX)}          # a box detector: no mask head
    elif args.images and args.annotations and args.weights:
        detector = load_detector_file(args.weights)
    else:
        ap.error("--images, --annotations and --weights are required (or --synthetic N)")

    dicts = COCO_utils.generate_coco_dataset_dictionaries(args.annotations, args.images, args.classes, None, True)
    K = int(detector["roi_heads.box_predictor.cls_score.weight"].shape[0]) - 1        # the detector's classes (+ background)
    if max(a["category_id"] for d in dicts for a in d["annotations"]) >= K:
        raise ValueError("the annotations map to more classes than the detector's %d" % K)
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    if is_c4(cfg):
        raise NotImplementedError("mask-head training covers FPN models")
    last_path = os.path.join(args.out, args.name + "_last.pth")
    results_path = os.path.join(args.out, RESULTS_FILE)

    torch.manual_seed(args.seed)
    head = MaskHead(K, "cuda")
    if any(k.startswith(PREFIX) for k in detector):
        head.load_state_dict(detector)
    params = list(head.parameters())
    opt = optim.SGD(params, lr=args.lr, momentum=args.momentum)
    sched = optim.WarmupMultiStepLR(opt, args.steps, args.gamma, args.warmup_factor, args.warmup_iters)
    start_iter, best_p, best_r = 0, 0.0, 0.0
    chk = None
    if args.resume:
        chk = torch.load(last_path, map_location="cpu", weights_only=False)
        head.load_state_dict(chk["model"])
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

    full = merge_full_mask_rcnn(detector, head.state_dict())
    pred = TrackPredictor(cfg, state_dict=full)
    min_sizes = tuple(int(v) for v in args.min_sizes.split(",")) if args.min_sizes else None
    loader = COCO_utils.MaskTrainLoader(train_dicts, pred.model, args.ims_per_batch, args.seed, args.flip, args.cache_features,
                                        augment=args.augment, min_sizes=min_sizes, max_size=args.max_size or None)
    if chk is not None and "loader" in chk:
        loader.load_state_dict(chk["loader"])

    summary = {"losses": [], "tests": [], "num_classes": K}
    summary["ap_before"] = do_test(pred, test_dicts, gt) if not args.resume else None
    print("Training for {} iterations started".format(args.iters))
    for iteration in range(start_iter, args.iters):
        feats, classes, targets = next(loader)
        loss = head(feats, classes, targets)["loss_mask"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        summary["losses"].append(float(loss))
        print("Iter. {}/{}:\tloss: {}".format(iteration, args.iters, float(loss)))
        if iteration != 0 and iteration % args.checkpoint_period == 0:
            head.push_into(pred)
            res = do_test(pred, test_dicts, gt)
            print("test results:", res)
            if res is not None:
                line = "{}/{}:\t".format(iteration, args.iters) + "\t".join("{:.3f}".format(v) for v in res)
                if res[0] > best_p:
                    best_p = res[0]
                    line += " Best precision!"
                if res[8] > best_r:
                    best_r = res[8]
                    line += " Best recall!"
                with open(results_path, "a") as fh:
                    fh.write(line + "\n")
                summary["tests"].append((iteration, res))
            with open(results_path) as fh:
                chkpt = {"model": merge_full_mask_rcnn(detector, head.state_dict()), "optimizer": opt.state_dict(),
                         "scheduler": sched.state_dict(), "iteration": iteration, "kfold_split": split, "k_folds": k_folds,
                         "best_precision": best_p, "best_recall": best_r, "training_results": fh.read(),
                         "loader": loader.state_dict()}
            torch.save(chkpt, last_path)
            if res is not None and res[0] == best_p:
                torch.save(chkpt, os.path.join(args.out, args.name + "_bestAP.pth"))
            if res is not None and res[8] == best_r:
                torch.save(chkpt, os.path.join(args.out, args.name + "_bestAR.pth"))
            if args.stop_at and iteration >= args.stop_at:
                break
    head.push_into(pred)
    summary["ap_after"] = do_test(pred, test_dicts, gt)
    summary["checkpoint"] = last_path
    summary["state"] = {k: v.cpu() for k, v in head.state_dict().items()}
    return summary


if __name__ == "__main__":
    main()
