#!/usr/bin/env python
"""Bottom-up (TAG) proposals of one subset from actionness score pickles: recall report and, with --write_proposals, the
proposal list the trainers and the tester read.

The counterpart of the reference's gen_bottom_up_proposals.py with the stages of this project chained on the GPU:
tag_proposals.merge_scores -> TagProposalGenerator.generate (all videos in one batch) -> ProposalListBuilder.from_spans
-> ProposalListBuilder.build (-> proposal_eval.proposal_ar_an_batch with --ar_an, on the same device batch).  Flags are named as the reference's; --annotations stands in for its fixed data/ paths and
--frame_path is used for both the folder lookup and the written paths (the reference hard-codes the former).  Not
offered: --cls_scores and --iou_thresh (parsed there and never used), --reg_score_files (reaches an undefined name
there).  Videos without instances are left out as in the reference, so its `allow_empty` case (ActivityNet `testing`)
cannot arise; videos without scores are left out and counted.

    python tools/gen_bottom_up_proposals.py thumos14_rgb_actionness.pc thumos14_flow_actionness.pc --dataset thumos14 \\
        --subset testing --annotations data/thumos_14 --frame_path /data/thumos14_frames \\
        --write_proposals thumos14_tag_test_proposal_list.txt
"""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None, db=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('score_files', type=str, nargs='+')
    ap.add_argument("--anet_version", type=str, default='1.2', help='names the release; the file is --annotations')
    ap.add_argument("--dataset", type=str, default='activitynet', choices=['activitynet', 'thumos14'])
    ap.add_argument("--subset", type=str, default='validation', choices=['training', 'validation', 'testing'])
    ap.add_argument("--score_weights", type=float, nargs='+', default=None)
    ap.add_argument("--write_proposals", type=str, default=None)
    ap.add_argument("--minimum_len", type=float, default=0, help='minimum length of a proposal, in second')
    ap.add_argument("--frame_path", type=str, default=None, help='folder of the frame folders (needed with --write_proposals)')
    ap.add_argument("--annotations", default=None, help="THUMOS14 annotation folder / ActivityNet JSON file")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--device-text", action="store_true",
                    help="with --write_proposals: form the bytes of the list file on the device too; the same file")
    ap.add_argument("--ar_an", type=float, nargs='?', const=0.0, default=None, metavar='N',
                    help='also print the AR-AN report (proposal_eval); N: the maximum average number of proposals per '
                         'video, without a value the mean')
    args = ap.parse_args(argv)
    if args.write_proposals and not args.frame_path:
        ap.error("--write_proposals needs --frame_path")
    if args.score_weights is not None and len(args.score_weights) != len(args.score_files):
        ap.error("--score_weights: one weight per score file")

    import glob
    from action_detection_amd.datasets import open_database
    from action_detection_amd.proposal_io import format_window_list_rows, write_proposal_bytes, write_proposal_file
    from action_detection_amd.proposal_lists import ProposalListBuilder
    from action_detection_amd.tag_proposals import TagProposalGenerator, merge_scores

    if db is None:
        if args.annotations is None:
            ap.error("--annotations is required")
        db = open_database(args.dataset, args.annotations)
    if args.frame_path:
        print("loaded {} video folders".format(db.try_load_file_path(args.frame_path)))
    if args.dataset == 'thumos14' and args.subset == 'testing':
        args.subset = 'test'

    video_list = [v for v in db.get_subset_videos(args.subset) if v.instances != []]
    print("video list size: {}".format(len(video_list)))
    print('loading scores...')
    score_list = []
    for fname in args.score_files:
        with open(fname, 'rb') as f:
            score_list.append(pickle.load(f))
    print('load {} piles of scores'.format(len(score_list)))
    print('merging scores')
    score_dict = merge_scores(score_list, args.score_weights)
    print('done')

    videos = [v for v in video_list if v.id in score_dict]
    if len(videos) < len(video_list):
        print('{} videos without scores left out'.format(len(video_list) - len(videos)))
    if not videos:
        raise ValueError("no video of subset {} has both instances and scores".format(args.subset))

    print('generating proposals')
    generator = TagProposalGenerator(minimum_len=args.minimum_len, device=args.device)
    tag = generator.generate([np.ascontiguousarray(score_dict[v.id], dtype=np.float32) for v in videos],
                             [v.duration for v in videos])
    frame_counts = None
    if args.write_proposals:          # (a video without a frame folder raises here, naming it)
        names = [v.path.split('/')[-1].split('.')[0] for v in videos]
        frame_counts = [len(glob.glob(os.path.join(args.frame_path, n, 'img_*.jpg'))) for n in names]
    builder = ProposalListBuilder(device=args.device)
    batch = builder.from_spans(videos, [r.seconds for r in tag])
    thresholds = np.arange(0.5, 1, 0.2)
    device_text = bool(args.write_proposals) and args.device_text
    if device_text:
        result = builder.build_text(batch, frame_counts, [os.path.join(args.frame_path, n) for n in names],
                                    recall_thresholds=thresholds)
    else:
        result = builder.build(batch, frame_counts, recall_thresholds=thresholds)

    print('{} groundtruth boxes from'.format(int(result.totals.sum())))
    print('average # of proposals: {}'.format(result.mean_proposals))
    for th, (pv, pi) in zip(thresholds, result.recall):
        print('IOU threshold {}. per video recall: {:02f}, per instance recall: {:02f}'.format(th, pv * 100, pi * 100))
    print('Average Recall: {:.04f} {:.04f}'.format(*(np.mean(result.recall, axis=0) * 100)))
    if args.ar_an is not None:          # (TagResult.seconds is in NMS order, descending score: the batch's order is the rank)
        from action_detection_amd.proposal_eval import format_ar_an_report, proposal_ar_an_batch
        result.ar_an = proposal_ar_an_batch(batch, max_avg_nr_proposals=args.ar_an or None)
        print(format_ar_an_report(result.ar_an))

    if args.write_proposals:
        bad = [v.id for v, s in zip(videos, result.status) if s & 3]      # (bit 2, device text only: formatted on the host)
        if bad:
            raise ValueError("positions of {} are not finite or do not fit int32 (duration 0?)".format(", ".join(bad)))
        if device_text:
            write_proposal_bytes(args.write_proposals, result.data)
        else:
            records = [format_window_list_rows(os.path.join(args.frame_path, n), c, *result.rows(i))
                       for i, (n, c) in enumerate(zip(names, frame_counts))]
            write_proposal_file(args.write_proposals, records)
        print('list written. got {} videos'.format(len(videos)))
    return result


if __name__ == "__main__":
    main()
