#!/usr/bin/env python
"""Detect actions in videos that have no annotations: frame folders in, ActivityNet-style detection JSON out.

Every folder under FRAME_ROOT is a video (``proposal_io.parse_directory``).  Trained actionness networks score its frames, TAG
turns the scores into proposals, trained SSNs score the proposals, and the fused scores go through the detection post-processing
(``detect.ActionDetector``): no proposal list, no ground truth and no file between two stages.

    python tools/detect_videos.py /data/frames detections.json --dataset thumos14 \\
        --ssn RGB:ssn_rgb.pth.tar:1 Flow:ssn_flow.pth.tar:1.2 --actionness RGB:bin_rgb.pth.tar Flow:bin_flow.pth.tar \\
        --flow_pref flow_ --gpu-decode --save-scores scores.pc

``--ssn`` / ``--actionness`` take MODALITY:WEIGHTS[:WEIGHT] once per stream (give every stream of a kind a weight or none: equal
weights).  ``--proposals sliding`` replaces actionness + TAG by exponential sliding windows.  A video's frame count is the smallest
count over the modalities in use; its duration is frames / ``--fps`` unless ``--durations`` (lines of ``video seconds``) gives it.
NMS threshold, top-k and the softmax flag are those the data set is evaluated with (``tools/eval_detections.py --nms_threshold
--top_k --softmax_before_filter``).  Flow streams read the images ``tools/extract_flow.py`` wrote.  The networks are built by the
code of ``tools/test_ssn.py`` and ``tools/extract_actionness.py``.  One process, one device.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# top_k / nms_threshold / softmax_before_filter of the data sets' evaluation
EVALUATION = {"thumos14": dict(nms_threshold=0.2, top_k=2000, softmax_before_filter=True),
              "activitynet1.2": dict(nms_threshold=0.6, top_k=60, softmax_before_filter=False)}


def parse_stream(text):
    """MODALITY:WEIGHTS[:WEIGHT] -> (modality, checkpoint path, weight or None)"""
    parts = text.split(":")
    if len(parts) not in (2, 3) or parts[0] not in ("RGB", "Flow") or not parts[1]:
        raise argparse.ArgumentTypeError("expected RGB|Flow:WEIGHTS[:WEIGHT], got %r" % text)
    return parts[0], parts[1], (float(parts[2]) if len(parts) == 3 else None)


def parse(argv=None):
    import test_ssn
    ap = argparse.ArgumentParser(description="detect actions in videos without annotations")
    ap.add_argument("frame_root", type=str)
    ap.add_argument("out_json", type=str)
    ap.add_argument("--dataset", type=str, required=True, choices=sorted(EVALUATION))
    ap.add_argument("--ssn", type=parse_stream, nargs="+", required=True, metavar="MODALITY:WEIGHTS[:WEIGHT]")
    ap.add_argument("--actionness", type=parse_stream, nargs="+", default=[], metavar="MODALITY:WEIGHTS[:WEIGHT]")
    ap.add_argument("--proposals", type=str, default="tag", choices=["tag", "sliding"])
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--durations", type=str, default=None, help="a file of 'video seconds' lines")
    ap.add_argument("--class-names", type=str, default=None, help="one class name per line (default: the class index)")
    ap.add_argument("--arch", type=str, default="BNInception")
    ap.add_argument("--test_crops", type=int, default=10, choices=[1, 10])
    ap.add_argument("--frame_interval", type=int, default=6)
    ap.add_argument("--actionness_interval", type=int, default=5)
    ap.add_argument("--tick_batch", type=int, default=32)
    ap.add_argument("--gpu-decode", action="store_true", help="decode, scale and crop the frames on the device")
    ap.add_argument("--flow_pref", type=str, default="")
    ap.add_argument("--save-scores", type=str, default=None, help="also write the score pickle tools/eval_detections.py reads")
    ap.add_argument("--device", type=str, default="cuda:0")
    args = ap.parse_args(argv)
    if args.proposals == "tag" and not args.actionness:
        ap.error("--proposals tag needs --actionness streams (or use --proposals sliding)")
    args.num_class = test_ssn.NUM_CLASS[args.dataset]
    return args


def find_videos(args):
    """-> [(video id, frame count, duration)] of the folders under FRAME_ROOT, alphabetical."""
    from action_detection_amd.proposal_io import parse_directory
    frame_dict = parse_directory(args.frame_root, key_func=lambda x: x.split("/")[-1], flow_x_prefix=args.flow_pref + "x_",
                                 flow_y_prefix=args.flow_pref + "y_")
    modalities = {m for m, _, _ in list(args.ssn) + list(args.actionness)}
    durations = {}
    if args.durations:
        with open(args.durations) as f:
            for line in f:
                if line.strip():
                    vid, seconds = line.split()
                    durations[vid] = float(seconds)
    videos = []
    for vid in sorted(frame_dict):
        _, rgb, flow = frame_dict[vid]
        frames = min(([rgb] if "RGB" in modalities else []) + ([flow] if "Flow" in modalities else []))
        if frames < 1:
            raise ValueError("video {} has no frames of {}".format(vid, sorted(modalities)))
        videos.append((vid, frames, durations.get(vid, frames / args.fps)))
    if not videos:
        raise ValueError("no video folder under {}".format(args.frame_root))
    return videos


def make_ssn_stream(args, modality, weights, weight):
    """One SSN of the detector, built as tools/test_ssn.py builds its tester."""
    import test_ssn
    from action_detection_amd.detect import Stream
    # (the driver's per-video tester builds the network, the DenseTester and the frame source; its proposal list is not used here:
    # an empty one)
    ns = argparse.Namespace(dataset=args.dataset, modality=modality, weights=weights, arch=args.arch, no_regression=False,
                            tick_batch=args.tick_batch, input_size=None, gpu_decode=args.gpu_decode, frame_root=args.frame_root,
                            flow_pref=args.flow_pref, test_crops=args.test_crops, frame_interval=args.frame_interval,
                            proposal_list=os.devnull)
    built = test_ssn.SSNVideoTester(ns, args.device)
    tester, reader, transform = built.tester, built.reader, built.transform
    return Stream(tester, reader, transform, 1 if modality == "RGB" else 5, weight)


def make_actionness_stream(args, modality, weights, weight):
    """One actionness network of the detector, built as tools/extract_actionness.py builds it, with that tool's transforms."""
    import extract_actionness as EA
    from action_detection_amd import test_data as TD
    from action_detection_amd import train_data as D
    from action_detection_amd.actionness_test import ActionnessTester
    from action_detection_amd.detect import Stream
    net = EA.build_net(modality, weights, args.arch, args.device)
    if args.gpu_decode:
        if args.test_crops != 10:
            raise ValueError("--gpu-decode scores the actionness streams with 10 crops, got --test_crops {}".format(args.test_crops))
        reader = D.CompressedFrameDirReader(args.frame_root, modality, args.flow_pref)
        transform = EA.device_transform(net, modality, args.device, scale=True)
    else:
        # binary_test.py's host chain: ten crops are GroupOverSample as in the SSN tester's chain (the same transforms); one crop is
        # taken as that chain takes it, GroupScale + GroupCenterCrop (the backbone here takes square inputs only)
        reader = D.FrameDirReader(args.frame_root, modality, args.flow_pref)
        transform = TD.host_test_chain(net.input_size, net.scale_size, net.input_mean, net.input_std, args.test_crops)
    return Stream(ActionnessTester(net, tick_batch=args.tick_batch), reader, transform,
                  1 if modality == "RGB" else 5, weight)


def main(argv=None, make_ssn=make_ssn_stream, make_actionness=make_actionness_stream):
    args = parse(argv)
    import test_ssn
    from action_detection_amd.detect import ActionDetector
    from action_detection_amd.detection_post import DetectionPostProcessor
    from action_detection_amd.tag_proposals import TagProposalGenerator, sliding_window_proposals
    import numpy as np
    if make_ssn is make_ssn_stream:
        import torch
        import action_detection_amd as pkg
        pkg.build()
        if torch.device(args.device).type == "cuda":
            torch.cuda.set_device(torch.device(args.device))
    videos = find_videos(args)
    print("{} videos under {}".format(len(videos), args.frame_root))
    ssn = [make_ssn(args, *s) for s in args.ssn]
    sliding = args.proposals == "sliding"
    actionness = [] if sliding else [make_actionness(args, *s) for s in args.actionness]
    post = DetectionPostProcessor(args.num_class, **EVALUATION[args.dataset])
    detector = ActionDetector(ssn, actionness, None if sliding else TagProposalGenerator(device=args.device), post,
                              frame_interval=args.frame_interval, actionness_interval=args.actionness_interval,
                              test_crops=args.test_crops, tick_batch=args.tick_batch, stpp_cfg=test_ssn.STPP[args.dataset],
                              device=args.device)
    proposals = [np.asarray(sliding_window_proposals(v[2]), dtype=np.float64).reshape(-1, 2) for v in videos] if sliding else None
    result = detector.detect(videos, proposals=proposals)
    if args.class_names:
        with open(args.class_names) as f:
            names = [line.strip() for line in f if line.strip()]
    else:
        names = [str(c) for c in range(args.num_class)]
    out = result.to_activitynet(names)
    with open(args.out_json, "w") as f:
        json.dump(out, f)
    if args.save_scores:
        result.save_scores(args.save_scores)
    print("{} detections of {} videos written to {}".format(len(result.detections.rows), len(videos), args.out_json))
    return result


if __name__ == "__main__":
    main()
