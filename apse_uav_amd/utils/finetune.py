"""The fine-tune loop that tools/finetune_segmentation.py, finetune_box_head.py, finetune_rpn.py and finetune_uav.py share --
dcnn/scripts/train/finetune_uav.py and finetune_segmentation.py are one loop too: frozen detector, some trainable heads, momentum
SGD under WarmupMultiStepLR, every CHECKPOINT_PERIOD iterations a score of the held-out images, a line in results.txt and a
checkpoint with the merged full detector, and ``--resume`` that repeats the uninterrupted run bit for bit.

A tool parses ``add_common_arguments`` plus its own, loads the start detector (``load_start``) and calls ``run`` with a ``Task``
that says what differs: which heads, which loader, which losses, which score.
"""
import functools
import operator
import os

import numpy as np
import torch

RESULTS_FILE = "results.txt"
AP_COLUMNS = "\t\tAP\tAP_05\tAP0.75\tAP_s\tAP_m\tAP_l\tAR_1\tAR_10\tAR_100\tAR_s\tAR_m\tAR_l"
RECALL_LIMITS = (100, 1000)
MASK_PREDICTOR = "roi_heads.mask_head.predictor."
CLS_SCORE = "roi_heads.box_predictor.cls_score.weight"
SYNTHETIC_MOTS = "<generated>"          # --mots without a DATASET (with --synthetic N)


def add_common_arguments(ap, name_default, start="heads"):
    """The arguments every fine-tune tool takes.  ``start``: what of the --weights file the training starts from (help text)."""
    ap.add_argument("--images", default="")
    ap.add_argument("--annotations", default="")
    ap.add_argument("--weights", default="", help="detector (.pth / converted model-zoo file); its %s is the start" % start)
    ap.add_argument("--classes", nargs="*", default=None, help="category names whose annotations are used (default: all)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default=name_default)
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
    ap.add_argument("--stop-at", type=int, default=0, help="stop after this iteration's checkpoint (an interrupted run, for --resume)")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--test-on-train", action="store_true", help="score the training images instead of the held-out ones")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N")
    ap.add_argument("--mask-format", choices=("polygon", "bitmask"), default="polygon",
                    help="ground truth of the mask head: polygon lists only, or (detectron2's INPUT.MASK_FORMAT = bitmask) RLE "
                         "segmentations as well, with BitMasks.crop_and_resize targets; with --synthetic N the generated "
                         "polygons are converted to RLE annotations")
    ap.add_argument("--mots", nargs="?", const=SYNTHETIC_MOTS, default="", metavar="DATASET",
                    help="train on a KITTI MOTS / MOTSChallenge layout (instances_txt/ or instances/, training/image_02/) with "
                         "--seqmap FILE instead of --images / --annotations; implies --mask-format bitmask; with --synthetic N "
                         "and no DATASET a generated one")
    ap.add_argument("--seqmap", default="", help="the sequence map of --mots")


def mask_format(args):
    """The mask ground-truth format of a parsed command line: --mots implies bitmask."""
    return "bitmask" if getattr(args, "mots", "") else getattr(args, "mask_format", "polygon")


def annotations_to_rle(annotations, out_path):
    """A COCO annotation file with every polygon segmentation replaced by its compressed RLE (the rasterisation of
    utils/coco.py on the device) -> ``out_path``."""
    import json
    from .coco import COCO
    coco = COCO.from_dataset(json.load(open(annotations)), verbose=False)
    for ann in coco.dataset["annotations"]:
        if isinstance(ann.get("segmentation"), list) and ann["segmentation"]:
            r = coco.annToRLE(ann)
            ann["segmentation"] = {"size": [int(v) for v in r["size"]], "counts": r["counts"].decode("ascii")}
    with open(out_path, "w") as fh:
        json.dump(coco.dataset, fh)
    return out_path


def holdout_split(n, k_folds, seed):
    """First fold of a seeded shuffle split into ``k_folds`` parts (the reference takes KFold(shuffle=True)'s first fold):
    (train indices, test indices), both sorted."""
    k = max(2, min(int(k_folds), n))
    order = np.random.default_rng(seed).permutation(n)
    n_test = max(1, n // k)
    return sorted(int(i) for i in order[n_test:]), sorted(int(i) for i in order[:n_test])


def load_start(args, ap):
    """The start detector's state: the --weights file, or with --synthetic N a seeded detector and N generated images with
    their annotations under --out (``args.images`` / ``args.annotations`` then point there)."""
    from ..synthetic import synthetic_dataset
    from ..weights import load_detector_file, synthetic_detector_state
    os.makedirs(args.out, exist_ok=True)
    mots = getattr(args, "mots", "")
    if args.synthetic and mots:
        if mots != SYNTHETIC_MOTS:
            ap.error("--synthetic N --mots takes no DATASET: it generates one")
        from ..synthetic import write_synthetic_mots
        args.mots = os.path.join(args.out, "synthetic_mots")
        args.seqmap = write_synthetic_mots(args.mots, seqs=("0000", "0001"), frames=args.synthetic // 2 + 2)
        return synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)
    if args.synthetic:
        args.images = os.path.join(args.out, "synthetic")
        args.annotations = synthetic_dataset(args.images, args.synthetic)
        if mask_format(args) == "bitmask":
            args.annotations = annotations_to_rle(args.annotations, os.path.join(args.images, "annotations_rle.json"))
        return synthetic_detector_state(0, (1, 1, 1, 1), num_classes=4)
    if mots:
        if mots == SYNTHETIC_MOTS or not args.seqmap or not args.weights:
            ap.error("--mots DATASET needs --seqmap FILE and --weights (or --synthetic N --mots)")
        return load_detector_file(args.weights)
    if args.images and args.annotations and args.weights:
        return load_detector_file(args.weights)
    ap.error("--images, --annotations and --weights are required (or --mots DATASET --seqmap FILE, or --synthetic N)")


def training_cfg(K, context_cache):
    """The f32 batch-1 configuration the loops train under.  ``context_cache``: the loop alternates between images of several
    sizes and every size has a context of its own, so at least this many are kept alive (None: the configuration's own)."""
    from ..config import setup_cfg
    cfg = setup_cfg(num_classes=K)
    cfg.APSE.MAX_BATCH = 1
    cfg.APSE.DTYPE = "f32"
    if context_cache:
        cfg.APSE.CONTEXT_CACHE = max(int(cfg.APSE.get("CONTEXT_CACHE", 1)), context_cache)
    return cfg


def detector_classes(detector):
    """The detector's class count (its cls_score has one more row, the background)."""
    return int(detector[CLS_SCORE].shape[0]) - 1


def trained_classes(args, detector, dicts):
    """The class count of a box branch trained on ``--classes``: their number (the detector's without them); annotations beyond
    it are refused."""
    K = len(args.classes) if args.classes else detector_classes(detector)
    if max(a["category_id"] for d in dicts for a in d["annotations"]) >= K:
        raise ValueError("the annotations map to more classes than the %d being trained" % K)
    return K


def adapt_detector(detector, K):
    """The frozen detector for K classes: when the checkpoint's class count differs, the per-class tensors outside the trained
    layers (the mask predictor) are re-initialised as detectron2 leaves shape-mismatched keys (normal(std = 0.001), bias 0).
    -> (state, True when the class count changed)."""
    if detector_classes(detector) == K:
        return detector, False
    out = dict(detector)
    if MASK_PREDICTOR + "weight" in out:
        cin = int(out[MASK_PREDICTOR + "weight"].shape[1])
        out[MASK_PREDICTOR + "weight"] = torch.nn.init.normal_(torch.zeros(K, cin, 1, 1), std=0.001)
        out[MASK_PREDICTOR + "bias"] = torch.zeros(K)
    return out, True


def detection_scores(pred, dicts, coco_gt, iou_types=("bbox",)):
    """COCOeval stats (12 numbers per entry of ``iou_types``: "bbox", "segm") of the predictor's detections on ``dicts``, from
    one pass over the images -- the masks are those of the predictor's own boxes; None when there is nothing to score."""
    from PIL import Image
    from .coco_eval import CocoEvaluator
    ev = CocoEvaluator(coco_gt)
    total = 0
    for d in dicts:
        frame = np.asarray(Image.open(d["file_name"]).convert("RGB"))[:, :, ::-1].copy()
        inst = pred(frame)[0]["instances"]
        ev.add(d["image_id"], inst)
        total += len(inst)
    if total == 0:
        return None
    return [[float(v) for v in ev.evaluate(t).stats] for t in iou_types]


def bbox_scores(pred, dicts, coco_gt):
    """bbox COCOeval stats (12 numbers) of the predictor's detections on ``dicts``; None when there is nothing to score."""
    res = detection_scores(pred, dicts, coco_gt)
    return None if res is None else res[0]


def proposal_scores(pred, dicts):
    """[recall@100, recall@1000] (IoU 0.5) of the predictor's proposals on ``dicts``; None when there is no ground truth."""
    from .rpn_train import proposal_recall
    res = proposal_recall(pred.model, dicts, 0.5, RECALL_LIMITS)
    return None if res is None else [float(res[k]) for k in RECALL_LIMITS]


class Task:
    """What one fine-tune tool adds to ``run``.  The class attributes are the tools' differences that are settings; the methods
    below ``build_heads`` have the behaviour most tools share."""
    what = None                         # "box-head": the training's name in messages
    header = AP_COLUMNS + "\n"          # first line of results.txt
    precision_index = 0                 # the score that earns "Best precision!" / _bestAP (None: no such score, no best_precision key)
    recall_index = 8                    # the score that earns "Best recall!" / _bestAR
    summary_keys = ("ap_before", "ap_after")
    summary_num_classes = True          # the summary has "num_classes"
    summary_predictor = False           # the summary has "predictor"
    coco_ground_truth = True            # do_test gets the held-out images as a COCO object (else None)
    precomputed_proposals = False       # generate_coco_dataset_dictionaries' precomputed_proposals
    keep_box_only = False               # ... and its keep_box_only: annotations without a segmentation stay
    context_cache = 4                   # training_cfg's
    best_needs_score = False            # _bestAP / _bestAR: False = also written when nothing was scored or the file is missing
    resume_takes_detector = True        # --resume: the frozen part comes from the checkpoint, not from the start detector
    loader_state_optional = False       # --resume: a checkpoint without "loader" is accepted

    heads = ()                          # the trainable heads, set by build_heads

    def num_classes(self, args, detector, dicts):
        return detector_classes(detector)

    def build_heads(self, args, cfg, detector, K):
        """Sets ``self.heads`` from the start detector (torch is seeded just before) -> the detector the run freezes."""
        raise NotImplementedError

    def merged_state(self, detector):
        raise NotImplementedError

    def make_loader(self, args, dicts, model, K, sizes):
        """``sizes``: the min_sizes / max_size keyword arguments from the command line."""
        raise NotImplementedError

    def losses(self, batch, loader, args):
        """-> {name: loss tensor}; ``run`` optimises their sum, taken in this order."""
        raise NotImplementedError

    def do_test(self, pred, dicts, coco_gt):
        raise NotImplementedError

    def optimizer(self, args, params):
        from .. import optim
        return optim.SGD(params, lr=args.lr, momentum=args.momentum)

    def predictor(self, cfg, state):
        from ..engines.track_predictor import TrackPredictor
        return TrackPredictor(cfg, state_dict=state)

    def after_step(self, pred):
        pass

    def counts(self, loader):
        """What the loader sampled for the last batch, for the iteration's line."""
        return ""

    def report(self, losses, loader):
        """-> (the iteration's entry in the summary's "losses", the rest of its printed line)."""
        values = tuple(float(v.detach()) for v in losses.values())
        return values, "\t".join("{}: {}".format(k, v) for k, v in zip(losses, values)) + self.counts(loader)

    def push(self, pred):
        for head in self.heads:
            head.push_into(pred)

    def state(self):
        return {k: v.cpu() for head in self.heads for k, v in head.state_dict().items()}


def run(task, args, detector):
    """The loop.  ``detector``: the start state (``load_start``).  -> the summary dictionary the tools' ``main`` returns."""
    from ..config import is_c4
    from ..optim import WarmupMultiStepLR
    from . import COCO_utils
    from .coco import COCO

    if getattr(args, "mots", ""):
        from .MOT_utils import generate_mots_dataset_dictionaries
        dicts = generate_mots_dataset_dictionaries(args.mots, args.seqmap, tuple(args.classes) if args.classes else ("car", "pedestrian"))
    else:
        dicts = COCO_utils.generate_coco_dataset_dictionaries(args.annotations, args.images, args.classes, None,
                                                              task.precomputed_proposals, task.keep_box_only, mask_format(args))
    K = task.num_classes(args, detector, dicts)
    cfg = training_cfg(K, task.context_cache)
    if is_c4(cfg):
        raise NotImplementedError("%s training covers FPN models" % task.what)
    last_path = os.path.join(args.out, args.name + "_last.pth")
    results_path = os.path.join(args.out, RESULTS_FILE)
    p_idx, r_idx = task.precision_index, task.recall_index

    torch.manual_seed(args.seed)
    detector = task.build_heads(args, cfg, detector, K)
    params = [p for head in task.heads for p in head.parameters()]
    opt = task.optimizer(args, params)
    sched = WarmupMultiStepLR(opt, args.steps, args.gamma, args.warmup_factor, args.warmup_iters)
    start_iter, best_p, best_r = 0, 0.0, 0.0
    chk = None
    if args.resume:
        chk = torch.load(last_path, map_location="cpu", weights_only=False)
        if task.resume_takes_detector:
            detector = {k: v for k, v in chk["model"].items()}       # the frozen part as the interrupted run had it
        for head in task.heads:
            head.load_state_dict(chk["model"])
        opt.load_state_dict(chk["optimizer"])
        sched.load_state_dict(chk["scheduler"])
        start_iter = int(chk["iteration"]) + 1
        split, k_folds = chk["kfold_split"], chk["k_folds"]
        if p_idx is not None:
            best_p = chk["best_precision"]
        best_r = chk["best_recall"]
        with open(results_path, "w") as fh:
            fh.write(chk["training_results"])
    else:
        k_folds = args.k_folds
        split = holdout_split(len(dicts), k_folds, args.seed)
        with open(results_path, "w") as fh:
            fh.write(task.header)
    train_ids, test_ids = split
    train_dicts = [dicts[i] for i in train_ids]
    test_dicts = train_dicts if args.test_on_train else [dicts[i] for i in test_ids]
    gt = COCO.from_dataset(COCO_utils.detectron2_dataset_to_coco(test_dicts), verbose=False) if task.coco_ground_truth else None

    pred = task.predictor(cfg, task.merged_state(detector))
    sizes = dict(min_sizes=tuple(int(v) for v in args.min_sizes.split(",")) if args.min_sizes else None, max_size=args.max_size or None)
    loader = task.make_loader(args, train_dicts, pred.model, K, sizes)
    loader.mask_format = mask_format(args)       # the box and RPN loaders read RLE annotations too (they make no mask targets)
    if chk is not None and ("loader" in chk or not task.loader_state_optional):
        loader.load_state_dict(chk["loader"])

    summary = {"losses": [], "tests": []}
    if task.summary_num_classes:
        summary["num_classes"] = K
    summary[task.summary_keys[0]] = task.do_test(pred, test_dicts, gt) if not args.resume else None
    print("Training for {} iterations started".format(args.iters))
    for iteration in range(start_iter, args.iters):
        losses = task.losses(next(loader), loader, args)
        loss = functools.reduce(operator.add, losses.values())
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        task.after_step(pred)
        entry, text = task.report(losses, loader)
        summary["losses"].append(entry)
        print("Iter. {}/{}:\t".format(iteration, args.iters) + text)
        if iteration != 0 and iteration % args.checkpoint_period == 0:
            task.push(pred)
            res = task.do_test(pred, test_dicts, gt)
            print("test results:", res)
            if res is not None:
                line = "{}/{}:\t".format(iteration, args.iters) + "\t".join("{:.3f}".format(v) for v in res)
                if p_idx is not None and res[p_idx] > best_p:
                    best_p = res[p_idx]
                    line += " Best precision!"
                if res[r_idx] > best_r:
                    best_r = res[r_idx]
                    line += " Best recall!"
                with open(results_path, "a") as fh:
                    fh.write(line + "\n")
                summary["tests"].append((iteration, res))
            chkpt = {"model": task.merged_state(detector), "optimizer": opt.state_dict(), "scheduler": sched.state_dict(),
                     "iteration": iteration, "kfold_split": split, "k_folds": k_folds}
            if p_idx is not None:
                chkpt["best_precision"] = best_p
            chkpt["best_recall"] = best_r
            with open(results_path) as fh:
                chkpt["training_results"] = fh.read()
            chkpt["loader"] = loader.state_dict()
            torch.save(chkpt, last_path)
            for idx, best, suffix in ((p_idx, best_p, "_bestAP.pth"), (r_idx, best_r, "_bestAR.pth")):
                path = os.path.join(args.out, args.name + suffix)
                if idx is None:
                    continue
                if (res is not None and res[idx] == best) or (not task.best_needs_score and (res is None or not os.path.exists(path))):
                    torch.save(chkpt, path)
            if args.stop_at and iteration >= args.stop_at:
                break
    task.push(pred)
    summary[task.summary_keys[1]] = task.do_test(pred, test_dicts, gt)
    summary["checkpoint"] = last_path
    summary["state"] = task.state()
    if task.summary_predictor:
        summary["predictor"] = pred
    return summary
