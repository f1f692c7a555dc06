#!/usr/bin/env python
"""Train the actionness classifier: the counterpart of the reference's binary_train.py on the kernels of this project.

Flags are those of ssn_opts.py that the loop reads; ``--train-list`` / ``--val-list`` / ``--frame-root`` / ``--synthetic N`` as in
tools/train_ssn.py.  ``-b`` counts videos (3 foreground + 9 background proposals x 5 snippets each; the reference fixes 4):

    python tools/train_binary.py thumos14 RGB --synthetic 4 --epochs 1 -b 2
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse(argv=None):
    p = argparse.ArgumentParser(description="Train the binary actionness classifier on the MI355X")
    p.add_argument("dataset", choices=["activitynet1.2", "thumos14"])
    p.add_argument("modality", choices=["RGB", "Flow"])
    p.add_argument("--arch", default="BNInception")
    p.add_argument("--num_body_segments", type=int, default=5)
    p.add_argument("--epochs", type=int, default=7)
    p.add_argument("--training_epoch_multiplier", "--tem", type=int, default=10)
    p.add_argument("-b", "--batch-size", type=int, default=4)
    p.add_argument("-i", "--iter-size", type=int, default=1)
    p.add_argument("--lr", "--learning-rate", type=float, default=0.001)
    p.add_argument("--lr_steps", type=float, nargs="+", default=[3, 6])
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--weight-decay", "--wd", type=float, default=5e-4)
    p.add_argument("--clip-gradient", "--gd", type=float, default=None)
    p.add_argument("--bn_mode", "--bn", default="frozen")
    p.add_argument("--print-freq", "-p", type=int, default=20)
    p.add_argument("--eval-freq", "-ef", type=int, default=1)
    p.add_argument("--resume", default="")
    p.add_argument("--init_weights", default="")
    p.add_argument("--snapshot_pref", default="")
    p.add_argument("--start-epoch", type=int, default=0)
    p.add_argument("--flow_prefix", default="")
    p.add_argument("--train-list", default="")
    p.add_argument("--val-list", default="")
    p.add_argument("--frame-root", default="")
    p.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded batches instead of a data set")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--num-class", type=int, default=2,
                   help="outputs of the classifier (2: actionness; K: the video-level classifier tools/classify_videos.py scores with; "
                        "the targets are whatever the data source yields)")
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
    from action_detection_amd.actionness_sampling import ActionnessSampler
    from action_detection_amd.binary_model import BinaryClassifier
    from action_detection_amd.input_pipeline import TrainingBatchPrefetcher
    from action_detection_amd.optim import SSNSGD
    from action_detection_amd.training import BinaryTrainer, checkpoint_names, fit, load_checkpoint

    pkg.build()
    new_length = 1 if args.modality == "RGB" else 5
    model = BinaryClassifier(args.num_class, args.num_body_segments, args.modality, new_length=new_length, base_model=args.arch, dropout=0.8,
                             bn_mode=args.bn_mode)      # (binary_train.py:25 fixes the dropout)
    if args.init_weights:
        model.base_model.load_state_dict(torch.load(args.init_weights, map_location="cpu", weights_only=False)["state_dict"])
        print("=> loaded init weights from '{}'".format(args.init_weights))
    elif args.synthetic:
        from action_detection_amd.synthetic import init_backbone_synthetic
        init_backbone_synthetic(model.base_model)
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
    snippets = args.num_body_segments * new_length * (1 if args.modality == "RGB" else 2)

    Prefetcher, batches = TrainingBatchPrefetcher, D.binary_batches
    if args.synthetic:
        n_train = n_val = args.synthetic

        def train_source(epoch):
            return D.synthetic_binary_source(args.synthetic, args.batch_size, args.modality, new_length, seed=epoch,
                                             body_seg=args.num_body_segments)

        def val_source(epoch):
            return D.synthetic_binary_source(args.synthetic, args.batch_size, args.modality, new_length, seed=1000, fg=6, bg=6,
                                             body_seg=args.num_body_segments)
    else:
        if not (args.train_list and args.val_list and args.frame_root):
            raise SystemExit("--train-list, --val-list and --frame-root are needed without --synthetic")
        if args.gpu_decode:
            from action_detection_amd.jpeg_decode import CompressedBatchPrefetcher
            import functools
            Prefetcher = functools.partial(CompressedBatchPrefetcher, index="device" if args.device_index else "host")
            batches = D.compressed_binary_batches
            reader = D.CompressedFrameDirReader(args.frame_root, args.modality, args.flow_prefix)
        else:
            reader = D.FrameDirReader(args.frame_root, args.modality, args.flow_prefix)
        common = dict(body_seg=args.num_body_segments, new_length=new_length)
        train_sampler = ActionnessSampler(args.train_list, epoch_multiplier=args.training_epoch_multiplier, **common)
        val_sampler = ActionnessSampler(args.val_list, random_shift=False, fg_ratio=6, bg_ratio=6, **common)
        n_train, n_val = len(train_sampler) // args.batch_size, -(-len(val_sampler) // args.batch_size)

        def train_source(epoch):
            return batches(train_sampler, reader, args.batch_size, np.random.permutation(len(train_sampler)))

        def val_source(epoch):
            return batches(val_sampler, reader, args.batch_size, drop_last=False)

    def train_batches(epoch):
        return D.Counted(D.binary_view(D.closing(Prefetcher(train_source(epoch), train_tf, group_size=snippets))), n_train)

    def val_batches(epoch):
        return D.Counted(D.binary_view(D.closing(Prefetcher(val_source(epoch), val_tf, group_size=snippets))), n_val)

    trainer = BinaryTrainer(model, optimizer, lr_steps=args.lr_steps, iter_size=args.iter_size, clip_gradient=args.clip_gradient,
                            print_freq=args.print_freq)
    names = checkpoint_names("binaryclassifier", args.snapshot_pref, args.dataset, args.arch, args.modality)
    best = fit(trainer, train_batches, val_batches, args.epochs, args.arch, names, start_epoch, best_loss, args.eval_freq)
    print("best loss {:.5f}; checkpoint {}".format(best, names[0]))
    return names[0]


if __name__ == "__main__":
    main()
