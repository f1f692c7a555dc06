#!/usr/bin/env python
"""Sliding-window proposal list of one subset: annotations + frame folders -> the list file the trainers and the tester read.

The counterpart of the reference's gen_sliding_window_proposals.py, same positionals and flags, with the stage run as
ONE batch on the GPU (proposal_lists.ProposalListBuilder: windows made on the device, named, converted to frame numbers
and checked for recall there; the text is formatted on the host, or with --device-text on the device as well).  --annotations stands in for the reference's
fixed data/ paths: the THUMOS14 annotation folder (data/thumos_14 layout) or the ActivityNet release JSON.

    python tools/gen_sliding_window_proposals.py testing rgb /data/thumos14_frames thumos14_sw_test_proposal_list.txt \\
        --dataset thumos14 --annotations data/thumos_14
"""
import argparse
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def frame_folder_name(video):
    """The folder name the reference derives from a video's path (ops/io.py:99)."""
    return video.path.split('/')[-1].split('.')[0]


def count_frames(frame_path, video, name_pattern):
    return len(glob.glob(os.path.join(frame_path, frame_folder_name(video), name_pattern)))


def main(argv=None, db=None):
    ap = argparse.ArgumentParser(description="Make window file used for detection")
    ap.add_argument("subset")
    ap.add_argument("modality", choices=['rgb', 'flow'])
    ap.add_argument("frame_path")
    ap.add_argument("output_file")
    ap.add_argument("--overlap", type=float, default=0.7)
    ap.add_argument("--max_level", type=int, default=8)
    ap.add_argument("--time_step", type=float, default=1)
    ap.add_argument("--version", default="1.2", help="ActivityNet version (names the release; the file is --annotations)")
    ap.add_argument("--avoid", default=None, type=str, help="file of video ids left out of the written list")
    ap.add_argument("--dataset", default="activitynet", choices=['thumos14', 'activitynet'])
    ap.add_argument("--annotations", default=None, help="THUMOS14 annotation folder / ActivityNet JSON file")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--device-text", action="store_true",
                    help="form the bytes of the list file on the device too (ProposalListBuilder.build_text); the same file")
    args = ap.parse_args(argv)

    from action_detection_amd.datasets import open_database
    from action_detection_amd.proposal_io import format_window_list_rows, write_proposal_bytes, write_proposal_file
    from action_detection_amd.proposal_lists import ProposalListBuilder

    name_pattern = 'img_*.jpg' if args.modality == 'rgb' else 'flow_x_*.jpg'
    if db is None:
        if args.annotations is None:
            ap.error("--annotations is required")
        db = open_database(args.dataset, args.annotations)
    print("loaded {} video folders".format(db.try_load_file_path(args.frame_path)))
    if args.dataset == 'thumos14' and args.subset == 'testing':
        args.subset = 'test'
    if args.avoid:
        with open(args.avoid) as f:
            avoid_list = [x.strip() for x in f]
    else:
        avoid_list = []

    videos = db.get_subset_videos(args.subset)
    written = [i for i, v in enumerate(videos) if v.id not in avoid_list]
    frame_counts = np.zeros(len(videos), dtype=np.int64)
    for i in written:          # (a video without a frame folder raises here, naming it)
        frame_counts[i] = count_frames(args.frame_path, videos[i], name_pattern)

    builder = ProposalListBuilder(device=args.device)
    batch = builder.sliding_windows(videos, overlap=args.overlap, max_level=args.max_level, time_step=args.time_step)
    if args.device_text:
        paths = [""] * len(videos)
        for i in written:
            paths[i] = os.path.join(args.frame_path, frame_folder_name(videos[i]))
        result = builder.build_text(batch, frame_counts, paths, write=written, recall_thresholds=[0.5, 0.7, 0.9])
    else:
        result = builder.build(batch, frame_counts, recall_thresholds=[0.5, 0.7, 0.9])
    print('average # of proposals: {} at overlap param {}'.format(result.mean_proposals, args.overlap))
    for th, (pv, pi) in zip([0.5, 0.7, 0.9], result.recall):
        print('IOU threshold {}. per video recall: {:02f}, per instance recall: {:02f}'.format(th, pv * 100, pi * 100))
    print("average per video recall: {:.2f}, average per instance recall: {:.2f}".format(
        np.mean([r[0] for r in result.recall]), np.mean([r[1] for r in result.recall])))
    bad = [videos[i].id for i in written if result.status[i] & 3]      # (bit 2, device text only: formatted on the host)
    if bad:
        raise ValueError("positions of {} are not finite or do not fit int32 (duration 0?)".format(", ".join(bad)))

    if args.device_text:
        write_proposal_bytes(args.output_file, result.data)
    else:
        records = [format_window_list_rows(os.path.join(args.frame_path, frame_folder_name(videos[i])), int(frame_counts[i]),
                                           *result.rows(i)) for i in written]
        write_proposal_file(args.output_file, records)
    print('list written. got {} videos'.format(len(written)))
    return result


if __name__ == "__main__":
    main()
