#!/usr/bin/env python
"""Video-level classification: the ``{video: scores[C]}`` file ``tools/eval_detections.py --cls_scores`` reads.

A trained K-class ``BinaryClassifier`` (a TSN with a segment consensus; ``tools/train_binary.py`` trains it) scores every
``--frame_interval``-th frame of every video of a proposal list (``ActionnessTester(grouping="tick")``), the per-tick scores
are aggregated per video on the device (``video_cls.VideoScoreAggregator``), the file is written and top-1 / top-3
accuracy, video mAP and mean class accuracy against the labels of the list are printed.

    python tools/classify_videos.py activitynet1.2 RGB weights.pth.tar cls_rgb.pc --frame-root /data/frames \\
        --proposal-list data/activitynet1.2_tag_val_normalized_proposal_list.txt --agg sliding_window

``--from-scores`` skips the network: it reads ``[T, crops, C]`` score pickles in the ``ActionnessScores.save`` format (one per
stream), aggregates each stream without the softmax and fuses them, ``stream 0 + sum_i (w_i / w_0) * stream i``, softmax at
the end (WEIGHTS is not read then; give ``-``):

    python tools/classify_videos.py activitynet1.2 RGB - cls.pc --proposal-list LIST --from-scores rgb.pc flow.pc --weights 1 1.5

One process; the GPU is opened here and no workers are spawned.
"""
import argparse
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NUM_CLASS = {"activitynet1.2": 100, "activitynet1.3": 200, "thumos14": 20}


def base_id(vid):
    vid = vid.decode("utf-8") if isinstance(vid, bytes) else str(vid)
    return vid.split("/")[-1]


def labels_of(proposal_list):
    """{video (last path component): sorted class indices} from the ground truth of a processed proposal list"""
    from action_detection_amd.proposal_sampling import ProposalSampler
    out = {}
    for vid, label, _, _ in ProposalSampler(proposal_list).all_gt():
        out.setdefault(base_id(vid), set()).add(int(label))
    return {k: sorted(v) for k, v in out.items()}


def build_net(arch, num_class, modality, checkpoint, device):
    import torch  # noqa: F401
    from action_detection_amd.binary_model import BinaryClassifier
    from action_detection_amd.training import load_checkpoint
    data_length = 1 if modality == "RGB" else 5
    net = BinaryClassifier(num_class, 5, modality, test_mode=True, new_length=data_length, base_model=arch)
    ckpt = load_checkpoint(checkpoint, model=net)
    print("model epoch {} loss: {}".format(ckpt.get("epoch"), ckpt.get("best_loss")))
    net.prepare_test_fc()
    return net.to(device).eval()


def load_tick_scores(path, device):
    """A score pickle {video: float32 [T, crops, C]} -> {last path component: device tensor}"""
    import numpy as np
    import torch
    with open(path, "rb") as f:
        raw = pickle.load(f, encoding="bytes")
    return {base_id(k): torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32))).to(device) for k, v in raw.items()}


def aggregate_streams(streams, weights, agg_kw, softmax):
    """streams: [{video: [T, crops, C] device tensor}] -> VideoClassScores"""
    from action_detection_amd.video_cls import VideoScoreAggregator, fuse_scores
    if len(streams) == 1:
        return VideoScoreAggregator(normalization=softmax, **agg_kw).aggregate(streams[0])
    if weights is None:
        weights = [1.0] * len(streams)
    if len(weights) != len(streams):
        raise ValueError("{} weights for {} score files".format(len(weights), len(streams)))
    agg = VideoScoreAggregator(normalization=False, **agg_kw)
    parts = [agg.aggregate(s) for s in streams]
    return fuse_scores(parts[0], parts[1:], [w / weights[0] for w in weights[1:]], norm=softmax)


def report(cls, labels):
    """Prints the metrics of the videos that have both scores and labels -> ClassificationMetrics (None without any)."""
    from action_detection_amd.video_cls import classification_metrics
    known = {k: v for k, v in labels.items() if k in set(cls.ids)}
    if not known:
        print("no labelled video among the {} scored ones".format(len(cls)))
        return None
    single = all(len(v) == 1 for v in known.values())
    m = classification_metrics(cls, known, top_k=(1, 3), class_accuracy=single)
    print("videos scored: {}".format(m.videos_scored))
    print("top-1 accuracy: {:.6f}".format(m.top_k_accuracy[1]))
    print("top-3 accuracy: {:.6f}".format(m.top_k_accuracy[3]))
    print("video mAP: {:.6f}".format(m.mean_ap))
    print("mean class accuracy: {}".format("{:.6f}".format(m.mean_class_accuracy) if single else "n/a (multi-label videos)"))
    return m


def main(argv=None):
    import action_detection_amd as pkg
    from action_detection_amd.ssn_models import SSN
    ap = argparse.ArgumentParser(description="video-level classification scores and metrics")
    ap.add_argument("dataset", type=str)
    ap.add_argument("modality", type=str, choices=["RGB", "Flow"])
    ap.add_argument("checkpoint", metavar="weights", type=str)
    ap.add_argument("save_scores", type=str)
    ap.add_argument("--proposal-list", required=True, help="the processed proposal list of the subset (videos and labels)")
    ap.add_argument("--frame-root", type=str, default="")
    ap.add_argument("--arch", type=str, default="BNInception", choices=sorted(SSN._BACKBONES))
    ap.add_argument("--num-class", type=int, default=None)
    ap.add_argument("--frame_interval", type=int, default=6)
    ap.add_argument("--test_crops", type=int, default=10, choices=[1, 10])
    ap.add_argument("--tick_batch", type=int, default=32)
    ap.add_argument("--input_size", type=int, default=None)
    ap.add_argument("--flow_pref", type=str, default="")
    ap.add_argument("--max_num", type=int, default=-1)
    ap.add_argument("--agg", type=str, default="sliding_window", choices=["default", "top_k", "sliding_window"])
    ap.add_argument("--k", type=int, default=None, help="ticks averaged per class with --agg top_k")
    ap.add_argument("--fps", type=int, default=1, help="ticks per second, for the sliding-window spans")
    ap.add_argument("--no-softmax", action="store_true")
    ap.add_argument("--gpu-decode", action="store_true", help="decode the frames on the device (10 crops, frames at scale_size)")
    ap.add_argument("--from-scores", type=str, nargs="+", default=None, help="tick score pickles, one per stream; skips the network")
    ap.add_argument("--weights", dest="fusion_weights", type=float, nargs="+", default=None, help="one weight per score file")
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args(argv)

    num_class = args.num_class if args.num_class is not None else NUM_CLASS.get(args.dataset)
    if num_class is None:
        ap.error("--num-class is needed for dataset {!r}".format(args.dataset))
    agg_kw = dict(mode=args.agg, k=args.k, fps=args.fps)
    if args.agg == "top_k" and args.k is None:
        ap.error("--agg top_k needs --k")
    pkg.build()
    if args.from_scores:
        streams = [load_tick_scores(p, args.device) for p in args.from_scores]
    else:
        import extract_actionness as EA
        from action_detection_amd.actionness_sampling import ActionnessSampler
        net = build_net(args.arch, num_class, args.modality, args.checkpoint, args.device)
        sampler = ActionnessSampler(args.proposal_list, new_length=net.new_length, test_interval=args.frame_interval)
        if args.gpu_decode:
            scores = EA.extract(net, sampler, EA.file_reader(args.frame_root, args.modality, args.flow_pref), args.test_crops,
                                args.input_size, args.tick_batch, "tick", args.max_num,
                                transform=EA.device_transform(net, args.modality, args.device, args.input_size))
        else:
            scores = EA.extract(net, sampler, EA.pil_loader(args.frame_root, args.modality, args.flow_pref), args.test_crops,
                                args.input_size, args.tick_batch, "tick", args.max_num)
        streams = [scores.raw]
    for s in streams:
        for vid, t in s.items():
            if t.dim() != 3 or t.shape[2] != num_class:
                raise ValueError("scores of video {!r} are {}, expected [T, crops, {}]".format(vid, tuple(t.shape), num_class))
    cls = aggregate_streams(streams, args.fusion_weights, agg_kw, not args.no_softmax)
    cls.save(args.save_scores)
    print("wrote {} videos to {}".format(len(cls), args.save_scores))
    metrics = report(cls, labels_of(args.proposal_list))
    return cls, metrics


if __name__ == "__main__":
    main()
