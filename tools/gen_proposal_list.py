#!/usr/bin/env python
"""Normalised proposal lists + extracted frames -> the proposal lists used for training and testing.

The counterpart of the reference's gen_proposal_list.py: the frame folders are counted (proposal_io.parse_directory, keyed
by the dataset's rule) and every normalised list is rewritten with frame numbers (proposal_io.process_proposal_list).
The reference takes the list names from its YAML; here they are given, in pairs:

    python tools/gen_proposal_list.py thumos14 /data/thumos14_frames \\
        --norm-list data/thumos14_tag_val_normalized_proposal_list.txt --out-list data/thumos14_tag_val_proposal_list.txt \\
        --norm-list data/thumos14_tag_test_normalized_proposal_list.txt --out-list data/thumos14_tag_test_proposal_list.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEY_FUNCS = {'activitynet1.2': lambda x: x[-11:], 'thumos14': lambda x: x.split('/')[-1]}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Generate proposal list to be used for training")
    ap.add_argument('dataset', type=str, choices=sorted(KEY_FUNCS))
    ap.add_argument('frame_path', type=str)
    ap.add_argument('--norm-list', action='append', required=True, help='a normalised proposal list (repeatable)')
    ap.add_argument('--out-list', action='append', required=True, help='where its processed list is written (repeatable)')
    args = ap.parse_args(argv)
    if len(args.norm_list) != len(args.out_list):
        ap.error("one --out-list per --norm-list")

    from action_detection_amd.proposal_io import parse_directory, process_proposal_list

    print('parse frames under folder {}'.format(args.frame_path))
    frame_dict = parse_directory(args.frame_path, key_func=KEY_FUNCS[args.dataset])
    print('frame folder analysis done')
    for norm, out in zip(args.norm_list, args.out_list):
        process_proposal_list(norm, out, frame_dict)
    print("proposal lists for dataset {} are ready for training.".format(args.dataset))
    return frame_dict


if __name__ == "__main__":
    main()
