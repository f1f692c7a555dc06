#!/usr/bin/env python
"""AR-AN of a proposal-list file: average recall against the average number of proposals per video, recall per tIoU and
the area under the curve (action_detection_amd.proposal_eval), for all videos of the file in one GPU pass.

Reads any list ``proposal_io.load_proposal_file`` reads -- normalised positions or frame numbers, the measure is
unit-free -- and takes of each record the ground-truth spans and the proposals; the order of the proposals in the file
is their rank (a TAG list is in NMS order, best first; a sliding-window list has no score and its order is arbitrary).

    python tools/eval_proposals.py data/activitynet1.2_tag_val_normalized_proposal_list.txt --max-avg 100
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def read_lists(list_file):
    """-> (video ids, proposals per video [m, 2], ground truth per video [n, 2]) of a proposal-list file."""
    from action_detection_amd.proposal_io import load_proposal_file
    records = load_proposal_file(list_file)
    ids = [r[0] for r in records]
    gt = [np.asarray([[float(g[1]), float(g[2])] for g in r[2]], dtype=np.float64).reshape(-1, 2) for r in records]
    pr = [np.asarray([[float(p[3]), float(p[4])] for p in r[3]], dtype=np.float64).reshape(-1, 2) for r in records]
    return ids, pr, gt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("list_file")
    ap.add_argument("--max-avg", type=float, default=None, metavar="N",
                    help="maximum average number of proposals per video (default: the file's mean)")
    ap.add_argument("--tiou", type=float, nargs=3, default=(0.5, 0.95, 10), metavar=("LO", "HI", "N"),
                    help="tIoU thresholds np.linspace(LO, HI, N)")
    ap.add_argument("--points", type=int, default=100, help="points of the curve")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--out", type=str, default=None, metavar="FILE.npz", help="store the arrays of the result")
    args = ap.parse_args(argv)

    from action_detection_amd.proposal_eval import format_ar_an_report, proposal_ar_an

    ids, pr, gt = read_lists(args.list_file)
    print("{}: {} videos, {} proposals, {} groundtruth boxes".format(args.list_file, len(ids), sum(len(p) for p in pr),
                                                                     sum(len(g) for g in gt)))
    thresholds = np.linspace(args.tiou[0], args.tiou[1], int(args.tiou[2]))
    result = proposal_ar_an(pr, gt, max_avg_nr_proposals=args.max_avg, thresholds=thresholds, points=args.points,
                            device=args.device)
    print(format_ar_an_report(result))
    if args.out:
        np.savez(args.out, recall=result.recall, avg_recall=result.avg_recall, proposals_per_video=result.proposals_per_video,
                 auc=result.auc, matches=result.matches, positives=result.positives, total_proposals=result.total_proposals,
                 thresholds=result.thresholds, first_hit=result.first_hit, video_ids=np.asarray(ids))
        print("arrays written to {}".format(args.out))
    return result


if __name__ == "__main__":
    main()
