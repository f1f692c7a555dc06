#!/usr/bin/env python
"""Train an SSN: the counterpart of the reference's ssn_train.py on the kernels of this project.

Flags are those of ssn_opts.py that the loop reads.  ``--train-list`` / ``--val-list`` stand in for its YAML lookup of the
proposal lists, ``--frame-root`` for the frame folders the lists name.  ``--synthetic N`` replaces the data set by N seeded batches
per epoch (and per validation), so the whole driver -- prefetcher, device augmentation, loop, validation, checkpoint -- runs with
no data:

    python tools/train_ssn.py thumos14 RGB --synthetic 4 --epochs 1 -b 2
    python tools/train_ssn.py thumos14 RGB --train-list data/thumos14_tag_val_normalized_proposal_list.txt \\
        --val-list data/thumos14_tag_test_normalized_proposal_list.txt --frame-root /data/frames -b 16 --snapshot_pref runs/thumos

``-b`` counts videos (8 proposals x 9 snippets each), as the reference's loader does.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NUM_CLASS = {"thumos14": 20, "activitynet1.2": 100}


def parse(argv=None):
    p = argparse.ArgumentParser(description="Train Structured Segment Networks (SSN) on the MI355X")
    p.add_argument("dataset", choices=sorted(NUM_CLASS))
    p.add_argument("modality", choices=["RGB", "Flow"])
    p.add_argument("--arch", default="BNInception")
    p.add_argument("--num_aug_segments", type=int, default=2)
    p.add_argument("--num_body_segments", type=int, default=5)
    p.add_argument("--dropout", "--do", type=float, default=0.8)
    p.add_argument("--epochs", type=int, default=7)
    p.add_argument("--training_epoch_multiplier", "--tem", type=int, default=10)
    p.add_argument("-b", "--batch-size", type=int, default=16)
    p.add_argument("-i", "--iter-size", type=int, default=1)
    p.add_argument("--lr", "--learning-rate", type=float, default=0.001)
    p.add_argument("--lr_steps", type=float, nargs="+", default=[3, 6])
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--weight-decay", "--wd", type=float, default=5e-4)
    p.add_argument("--clip-gradient", "--gd", type=float, default=None)
    p.add_argument("--bn_mode", "--bn", default="frozen")
    p.add_argument("--comp_loss_weight", "--lw", type=float, default=0.1)
    p.add_argument("--reg_loss_weight", "--rw", type=float, default=0.1)
    p.add_argument("--print-freq", "-p", type=int, default=20)
    p.add_argument("--eval-freq", "-ef", type=int, default=1)
    p.add_argument("--resume", default="")
    p.add_argument("--init_weights", default="")
    p.add_argument("-e", "--evaluate", action="store_true")
    p.add_argument("--snapshot_pref", default="")
    p.add_argument("--start-epoch", type=int, default=0)
    p.add_argument("--flow_prefix", default="")
    p.add_argument("--train-list", default="")
    p.add_argument("--val-list", default="")
    p.add_argument("--frame-root", default="")
    p.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded batches instead of a data set")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--gpu-decode", action="store_true",
                   help="upload the frames' JPEG files and decode them on the device (jpeg_decode.py) instead of PIL on the host"
                        "; files rewritten with tools/transcode_frames.py (restart markers, same pixels) decode on one lane per interval instead of one per file")
    p.add_argument("--device-index", action="store_true",
                   help="with --gpu-decode: find the restart intervals on the device too (JpegDecoder(index=\"device\")): no host work per interval or per byte")
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    import numpy as np
    import torch
    import action_detection_amd as pkg
    from action_detection_amd import train_data as D
    from action_detection_amd.input_pipeline import TrainingBatchPrefetcher
    from action_detection_amd.ops.ssn_ops import SSNObjective
    from action_detection_amd.optim import SSNSGD
    from action_detection_amd.proposal_sampling import ProposalSampler
    from action_detection_amd.ssn_models import SSN
    from action_detection_amd.training import SSNTrainer, checkpoint_names, fit, load_checkpoint

    pkg.build()
    num_class = NUM_CLASS[args.dataset]
    new_length = 1 if args.modality == "RGB" else 5
    model = SSN(num_class, args.num_aug_segments, args.num_body_segments, args.num_aug_segments, args.modality,
                base_model=args.arch, dropout=args.dropout, bn_mode=args.bn_mode)
    if args.init_weights:
        model.base_model.load_state_dict(torch.load(args.init_weights, map_location="cpu", weights_only=False)["state_dict"])
        print("=> loaded init weights from '{}'".format(args.init_weights))
    elif args.synthetic:
        from action_detection_amd.synthetic import init_backbone_synthetic
        init_backbone_synthetic(model.base_model)       # no checkpoint to start from: activations stay O(1)
    start_epoch, best_loss = args.start_epoch, math.inf
    if args.resume:
        ck = load_checkpoint(args.resume, model)
        start_epoch, best_loss = ck["epoch"], ck["best_loss"]
        print("=> loaded checkpoint '{}' (epoch {}) best loss {}".format(args.resume, start_epoch, best_loss))
    policies = model.get_optim_policies()
    for group in policies:
        print("group: {} has {} params, lr_mult: {}, decay_mult: {}".format(group["name"], len(group["params"]), group["lr_mult"],
                                                                            group["decay_mult"]))
    model.to(args.device)
    optimizer = SSNSGD(policies, args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    train_tf, val_tf = D.make_transforms(model, args.device)
    snippets = (2 * args.num_aug_segments + args.num_body_segments) * new_length * (1 if args.modality == "RGB" else 2)

    Prefetcher, batches = TrainingBatchPrefetcher, D.ssn_batches
    if args.synthetic:
        reg_stats = np.array([[0.0, 0.0], [1.0, 1.0]])
        split, group_size = 1, 7
        n_train = n_val = args.synthetic

        def train_source(epoch):
            return D.synthetic_ssn_source(args.synthetic, args.batch_size, num_class, args.modality, new_length, seed=epoch)

        def val_source(epoch):
            return D.synthetic_ssn_source(args.synthetic, args.batch_size, num_class, args.modality, new_length, seed=1000)
    else:
        if not (args.train_list and args.val_list and args.frame_root):
            raise SystemExit("--train-list, --val-list and --frame-root are needed without --synthetic")
        if args.gpu_decode:
            from action_detection_amd.jpeg_decode import CompressedBatchPrefetcher
            import functools
            Prefetcher = functools.partial(CompressedBatchPrefetcher, index="device" if args.device_index else "host")
            batches = D.compressed_ssn_batches
            reader = D.CompressedFrameDirReader(args.frame_root, args.modality, args.flow_prefix)
        else:
            reader = D.FrameDirReader(args.frame_root, args.modality, args.flow_prefix)
        common = dict(body_seg=args.num_body_segments, aug_seg=args.num_aug_segments, new_length=new_length)
        train_sampler = ProposalSampler(args.train_list, **common)
        val_sampler = ProposalSampler(args.val_list, random_shift=False, reg_stats=train_sampler.stats, **common)
        reg_stats = train_sampler.stats
        split, group_size = train_sampler.fg_per_video, train_sampler.fg_per_video + train_sampler.incomplete_per_video
        n_train = len(train_sampler) * args.training_epoch_multiplier // args.batch_size
        n_val = -(-len(val_sampler) // args.batch_size)

        def train_source(epoch):
            order = np.random.permutation(len(train_sampler) * args.training_epoch_multiplier)
            return batches(train_sampler, reader, args.batch_size, order)

        def val_source(epoch):
            return batches(val_sampler, reader, args.batch_size, drop_last=False)

    def train_batches(epoch):
        return D.Counted(D.closing(Prefetcher(train_source(epoch), train_tf, group_size=snippets)), n_train)

    def val_batches(epoch):
        return D.Counted(D.closing(Prefetcher(val_source(epoch), val_tf, group_size=snippets)), n_val)

    trainer = SSNTrainer(model, optimizer, SSNObjective(args.comp_loss_weight, args.reg_loss_weight), sample_split=split,
                         sample_group_size=group_size, lr_steps=args.lr_steps, iter_size=args.iter_size,
                         clip_gradient=args.clip_gradient, print_freq=args.print_freq)
    if args.evaluate:
        trainer.validate(val_batches(0))
        return None
    names = checkpoint_names("ssn", args.snapshot_pref, args.dataset, args.arch, args.modality)
    best = fit(trainer, train_batches, val_batches, args.epochs, args.arch, names, start_epoch, best_loss, args.eval_freq, reg_stats)
    print("best loss {:.5f}; checkpoint {}".format(best, names[0]))
    return names[0]


if __name__ == "__main__":
    main()
