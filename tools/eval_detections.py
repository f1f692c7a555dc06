#!/usr/bin/env python
"""Evaluate detection results: score pickles in the ssn_test.py format + a proposal list -> the mAP table.

The counterpart of the reference's eval_detection_results.py with the GPU stages of this project: the weighted merge of
the pickles (detection_eval.merge_detection_scores), score fusion / top-k / NMS / regression of all videos in one batched
pass (detection_post.DetectionPostProcessor.process_videos; --per-video runs the same stage video by video), then one
batched evaluation of all classes and thresholds (detection_eval.DetectionEvaluator).  Flags are named as the
reference's; --num-class and --tiou stand in for its YAML lookup, --proposal-list for the list file the YAML names.

    python tools/eval_detections.py scores_rgb.pc scores_flow.pc --proposal-list data/thumos14_tag_test_normalized_proposal_list.txt \\
        --num-class 20 --tiou thumos14 --nms_threshold 0.2 --top_k 2000 --score_weights 1 1.2 --ap-out ap.npy
"""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_tiou(text):
    from action_detection_amd.detection_eval import tiou_thresholds
    if text in ("thumos14", "activitynet1.2"):
        return tiou_thresholds(text)
    return np.asarray([float(x) for x in text.split(",")], dtype=np.float64)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate detection performance metrics")
    ap.add_argument("detection_pickles", type=str, nargs="+")
    ap.add_argument("--proposal-list", required=True, help="the test proposal list (ground truth comes from it)")
    ap.add_argument("--num-class", type=int, required=True)
    ap.add_argument("--tiou", type=str, required=True, help="thumos14 | activitynet1.2 | comma-separated thresholds")
    ap.add_argument("--nms_threshold", type=float, required=True)
    ap.add_argument("--no_regression", default=False, action="store_true")
    ap.add_argument("--softmax_before_filter", default=False, action="store_true")
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--cls_scores", type=str, default=None)
    ap.add_argument("--cls_top_k", type=int, default=1)
    ap.add_argument("--score_weights", type=float, default=None, nargs="+")
    ap.add_argument("--ap-out", type=str, default=None, help="write the AP array [class, threshold] as .npy")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--per-video", default=False, action="store_true",
                    help="post-process video by video instead of all videos in one batched pass (same results; for A/B runs)")
    args = ap.parse_args(argv)

    import torch
    from action_detection_amd.detection_eval import (DetectionEvaluator, _default_device, format_map_table,
                                                     merge_detection_scores)
    from action_detection_amd.detection_post import DetectionPostProcessor
    from action_detection_amd.proposal_sampling import ProposalSampler

    dev = torch.device(args.device) if args.device else _default_device()
    thresholds = parse_tiou(args.tiou)
    print("initiating evaluation of detection results {}".format(args.detection_pickles))
    score_dicts = []
    for pc in args.detection_pickles:
        with open(pc, "rb") as f:
            score_dicts.append(pickle.load(f))
    print("Merge detection scores from {} sources...".format(len(score_dicts)))
    scores = merge_detection_scores(score_dicts, args.score_weights)
    cls_scores = None
    if args.cls_scores:
        print("Using classifier scores from {}".format(args.cls_scores))
        with open(args.cls_scores, "rb") as f:
            raw = pickle.load(f, encoding="bytes")
        cls_scores = {os.path.splitext(os.path.basename(k.decode("utf-8") if isinstance(k, bytes) else k))[0]: v
                      for k, v in raw.items()}

    post = DetectionPostProcessor(args.num_class, args.nms_threshold, args.top_k, args.no_regression, args.cls_top_k,
                                  args.softmax_before_filter)
    evaluator = DetectionEvaluator(args.num_class, thresholds, device=dev)
    vcls = None if cls_scores is None else {vid: cls_scores[os.path.splitext(os.path.basename(vid))[0]] for vid in scores}
    if args.per_video:
        for vid, (rel_prop, act, comp, reg) in scores.items():
            dets, _ = post.process_video_device(np.asarray(rel_prop), torch.as_tensor(np.asarray(act)).to(dev),
                                                torch.as_tensor(np.asarray(comp)).to(dev),
                                                None if reg is None else torch.as_tensor(np.asarray(reg)).to(dev),
                                                device=dev, video_cls_score=None if vcls is None else vcls[vid])
            evaluator.add_video(vid, dets)
    else:
        evaluator.add_batch(post.process_videos(scores, device=dev, video_cls_scores=vcls))
    all_gt = ProposalSampler(args.proposal_list).all_gt()
    result = evaluator.evaluate(all_gt)
    if result.classes_without_gt:
        print("classes without ground truth (AP NaN): {}".format(result.classes_without_gt))
    print("Evaluation done.\n\n")
    print(format_map_table(thresholds, result.map_per_iou, "Detection Performance on {}".format(args.tiou)))
    if args.ap_out:
        np.save(args.ap_out, result.ap)
    return result


if __name__ == "__main__":
    main()
