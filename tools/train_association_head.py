#!/usr/bin/env python3
"""Association-head training -- the loop of dcnn/scripts/train/train_association_head.py on the HIP path.

MOTSloader (frozen backbone + roi_pool features of the ground-truth boxes), AssociationHead in training mode,
batch_hard_triplet_loss(margin=0.2) and momentum SGD (apse_uav_amd.optim.SGD, torch.optim.SGD's rule on apse_sgd_step).
Same defaults (6 frames per batch, 10 epochs, roi 10, lr 0.01, momentum 0.9), the same --checkpoint resume, per-epoch
association_head_EP{k}.pth, final association_head.pth and train_info.txt.  The checkpoint is a plain state_dict that
RcnnTracker loads (weights.load_association_file).

    python tools/train_association_head.py --dataset DATA --seqmap train.seqmap --weights R_101_FPN.pth [--out DIR]
    python tools/train_association_head.py --synthetic --epochs 2 --out /tmp/ah      # dry run, no download
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from apse_uav_amd.config import setup_cfg  # noqa: E402
from apse_uav_amd.networks.association_head import AssociationHead  # noqa: E402
from apse_uav_amd.online_triplet_loss.losses import batch_hard_triplet_loss  # noqa: E402
from apse_uav_amd.optim import SGD  # noqa: E402
from apse_uav_amd.utils.MOT_utils import MOTSloader  # noqa: E402

NETWORK = 'R_101_FPN_3x'
FRAMES_IN_BATCH = 6
NUM_EPOCH = 10
ROI_SIZE = 10
LEARNING_RATE = 0.01
MOMENTUM = 0.9
MARGIN = 0.2


def get_parser():
    p = argparse.ArgumentParser(description="Association head training")
    p.add_argument('--checkpoint', help='Path to pretrained association_head.pth checkpoint')
    p.add_argument('--dataset', default=os.path.join(ROOT, 'datasets', 'data_tracking_image_2'),
                   help='KITTI MOTS root: instances_txt/<seq>.txt and training/image_02/<seq>/%%06d.png')
    p.add_argument('--seqmap', default=None, help='seqmap file (default: <dataset>/train.seqmap)')
    p.add_argument('--weights', default=os.path.join(ROOT, 'pretrained', 'R_101_FPN_UAV_SEGM_bestAP.pth'),
                   help='detector checkpoint whose backbone produces the RoI features')
    p.add_argument('--out', default=None, help='output directory (default: pretrained/<checkpoint name>)')
    p.add_argument('--epochs', type=int, default=NUM_EPOCH)
    p.add_argument('--cache-features', action='store_true',
                   help='keep every batch\'s RoI features on the device after epoch 1 (100 KB per object at roi 10)')
    p.add_argument('--crop-features', action='store_true',
                   help='train on mask-cropped RoI features: p2 * the ground-truth mask, roi_align (the tracker then needs '
                        'cfg.APSE.CROP_FEATURES / --crop-features too)')
    p.add_argument('--synthetic', action='store_true',
                   help='write a tiny MOTS-layout dataset and seeded detector weights to a temporary directory and train on them')
    return p


def synthetic_setup(tmp):
    from apse_uav_amd.synthetic import write_synthetic_mots
    from apse_uav_amd.weights import synthetic_detector_state
    seqmap = write_synthetic_mots(os.path.join(tmp, "mots"))
    weights = os.path.join(tmp, "detector_seeded.pth")
    torch.save(synthetic_detector_state(0, (1, 1, 1, 1)), weights)
    return os.path.join(tmp, "mots"), seqmap, weights


def main(argv=None):
    args = get_parser().parse_args(argv)
    num_epoch = args.epochs
    tmp = None
    if args.synthetic:
        tmp = tempfile.TemporaryDirectory(prefix="assoc_synth_")
        dataset_path, seqmap_path, weights = synthetic_setup(tmp.name)
    else:
        dataset_path, weights = args.dataset, args.weights
        seqmap_path = args.seqmap or os.path.join(dataset_path, 'train.seqmap')
    config = setup_cfg(weights=weights)
    if args.synthetic:
        config.INPUT.MIN_SIZE_TEST, config.INPUT.MAX_SIZE_TEST = 256, 448

    dataloader = MOTSloader(config=config, dataset_path=dataset_path, seqmap_path=seqmap_path,
                            frames_in_batch=FRAMES_IN_BATCH, roi_size=ROI_SIZE, cache_features=args.cache_features,
                            crop_features=args.crop_features)
    print('Dataset loaded with {} batches and {} sequences'.format(dataloader.num_of_batches, len(dataloader.seqmap_names)))
    print('Training for', num_epoch, 'epochs')
    training_start_time = time.time()

    if args.checkpoint:
        checkpoint_name = 'association_head_UAV' + 'CHECKPOINT_' + NETWORK
    else:
        checkpoint_name = 'association_head_UAV_' + 'roi' + str(ROI_SIZE) + '_' + str(num_epoch) + 'ep_' + NETWORK
    path = args.out or os.path.join(ROOT, 'pretrained', checkpoint_name)
    print('Checkpoint will be saved as', path)
    os.makedirs(path, exist_ok=True)

    association_head = AssociationHead(roi_size=ROI_SIZE, input_depth=dataloader.roi_generator.get_features_depth())
    if args.checkpoint:
        association_head.load_state_dict(torch.load(args.checkpoint, map_location='cpu', weights_only=True))
        print('checkpoint {} loaded'.format(args.checkpoint))
    association_head.to(torch.device(config.MODEL.DEVICE))
    association_head.train()
    optimizer = SGD(association_head.parameters(), lr=LEARNING_RATE, momentum=MOMENTUM)
    avglosses_per_epoch = []

    for epoch in range(num_epoch):
        print('EPOCH:', epoch)
        epoch_loss = 0
        for sequence_idx in range(dataloader.num_of_sequences):
            print('Sequence:', dataloader.seqmap_names[sequence_idx])
            sequence_loss = 0
            for batch_idx in range(dataloader.batches_per_sequence[sequence_idx]):
                ids, rois = dataloader.get_training_batch(sequence_idx, batch_idx)
                optimizer.zero_grad()
                embeddings = association_head(rois)
                loss = batch_hard_triplet_loss(ids, embeddings, margin=MARGIN, device=config.MODEL.DEVICE)
                loss.backward()
                optimizer.step()
                epoch_loss += loss.item()
                sequence_loss += loss.item()
            nb = dataloader.batches_per_sequence[sequence_idx]
            print('\taverage loss in sequence:', sequence_loss / nb if nb else float('nan'))
        avg = epoch_loss / dataloader.num_of_batches if dataloader.num_of_batches else float('nan')
        print('epoch {} finished, average loss: {}'.format(epoch, avg))
        avglosses_per_epoch.append(avg)
        torch.save(association_head.state_dict(), os.path.join(path, 'association_head_EP{}.pth'.format(epoch)))

    print('Training finished')
    torch.save(association_head.state_dict(), os.path.join(path, 'association_head.pth'))
    total_time = time.time() - training_start_time
    total_time = str(total_time // 3600) + 'h' + str((total_time % 3600) / 60) + 'm'
    with open(os.path.join(path, 'train_info.txt'), 'w+') as f:
        s = 'FRAMES_IN_BATCH: ' + str(FRAMES_IN_BATCH) + '\n'
        s += 'NUM_EPOCH: ' + str(num_epoch) + '\n'
        s += 'ROI_SIZE: ' + str(ROI_SIZE) + '\n'
        s += 'LEARNING_RATE: ' + str(LEARNING_RATE) + '\n'
        s += 'MOMENTUM: ' + str(MOMENTUM) + '\n'
        s += 'training time: ' + total_time + '\n'
        for loss in avglosses_per_epoch:
            s += str(loss) + ','
        f.write(s)
    if tmp is not None:
        tmp.cleanup()
    return avglosses_per_epoch


if __name__ == '__main__':
    main()
