#!/usr/bin/env python
"""``tools/test_ssn.py`` with two more flags; every other argument, the worker plumbing and the pickles are that tool's.

    python tools/score_ssn.py thumos14 RGB weights.pth.tar scores_rgb.pc --proposal-list LIST --frame-root /data/frames \\
        --gpu-decode --include-empty --device-ticks

``--include-empty`` also scores the videos of the list that have no ground truth (the reference, and ``test_ssn.py``, leave them
out).  ``--device-ticks`` forms the proposal ticks, scalings and STPP row ranges of ALL videos of the list in one batched pass on
the device up front (``detect.build_test_table``) and scores through ``detect.score_video_ranges``: the same pickles, byte for
byte, without the per-proposal host loops between the backbone and the pooling launch of every video.  Without the two flags the
output is ``test_ssn.py``'s.
"""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_ssn  # noqa: E402


def parse(argv=None):
    """The two flags of this command, then ``test_ssn.parse`` on everything else."""
    import argparse
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--include-empty", action="store_true")
    ap.add_argument("--device-ticks", action="store_true")
    own, rest = ap.parse_known_args(argv)
    args = test_ssn.parse(rest)
    args.include_empty, args.device_ticks = own.include_empty, own.device_ticks
    return args


def load_videos(args, records=None):
    """``test_ssn.load_videos`` with the videos without ground truth kept when ``--include-empty`` is given."""
    if records is None and not getattr(args, "include_empty", False):
        return test_ssn.load_videos(args)
    import numpy as np
    from action_detection_amd.proposal_sampling import ProposalSampler
    return ProposalSampler(args.proposal_list, records=records, new_length=1 if args.modality == "RGB" else 5,
                           test_interval=args.frame_interval, reg_stats=np.zeros((2, 2)),
                           exclude_empty=not getattr(args, "include_empty", False))


def build_list_table(args, records, sampler, stpp_cfg, device):
    """The test table of the sampler's videos from the frame-number columns of the list's records as they stand (the table applies
    the record's filters itself)."""
    import numpy as np
    from action_detection_amd.detect import build_test_table
    records = {r[0]: r for r in records}
    videos = sampler.video_list
    props = [np.asarray([[int(x[3]), int(x[4])] for x in records[v.id][3]], dtype=np.int64).reshape(-1, 2) for v in videos]
    p_off = np.concatenate([[0], np.cumsum([len(p) for p in props])])
    return build_test_table(np.concatenate(props), p_off, np.asarray([v.num_frames for v in videos], dtype=np.int64),
                            sampler.new_length, args.frame_interval, stpp_cfg, device=device, video_ids=[v.id for v in videos])


class RangeVideoTester(test_ssn.SSNVideoTester):
    """``SSNVideoTester`` over the videos of ``load_videos`` above, scoring from the table with ``--device-ticks``.  ``tester`` /
    ``reader`` / ``transform``: stand-ins for the DenseTester built from ``args.weights`` and its frame source (tests inject
    deterministic ones)."""

    def __init__(self, args, device, tester=None, reader=None, transform=None):
        if tester is None:
            super(RangeVideoTester, self).__init__(args, device)
        else:
            from action_detection_amd import test_data as TD
            self.tester, self.reader, self.transform = tester, reader, transform
            self.test_crops, self.tick_batch = args.test_crops, args.tick_batch
            self.host_scaled_videos = self.host_decoded_files = 0
            self._batches = TD.test_frame_batches
        self.table = None
        if getattr(args, "device_ticks", False):
            from action_detection_amd.proposal_io import load_proposal_file
            records = load_proposal_file(args.proposal_list)          # (read once for the sampler and the table)
            self.sampler = load_videos(args, records)
            if len(self.sampler.video_list):
                self.table = build_list_table(args, records, self.sampler, test_ssn.STPP[args.dataset], device)
        elif getattr(args, "include_empty", False) or tester is not None:
            self.sampler = load_videos(args)

    def __call__(self, index):
        if self.table is None:
            return super(RangeVideoTester, self).__call__(index)
        from action_detection_amd.detect import score_video_ranges
        video = self.sampler.video_list[index]
        rows = self.table.video(index)
        before = getattr(self.transform, "host_scaled", 0)
        gen = self._batches(self.sampler, video, self.reader, self.transform, self.tick_batch)
        act, comp, reg, output = score_video_ranges(self.tester, gen, int(self.table.n_rows[index]), rows.ranges, rows.act,
                                                    rows.scaling, num_crop=self.test_crops)
        self.host_scaled_videos += int(getattr(self.transform, "host_scaled", 0) > before)
        self.host_decoded_files = getattr(self.transform, "host_decoded", 0)
        return (video.id, rows.rel.cpu().numpy(), act.cpu().numpy(), comp.cpu().numpy(), None if reg is None else reg.cpu().numpy(),
                output.cpu().numpy())


def make_range_tester(args, device):
    return RangeVideoTester(args, device)


def main(argv=None, make_tester=make_range_tester):
    """``test_ssn.main`` over the videos of ``load_videos`` above (that function counts the videos with its own ``load_videos``, so
    its few lines behind ``run`` are restated here, word for word)."""
    args = parse(argv)
    if make_tester is make_range_tester:
        import action_detection_amd as pkg
        pkg.build()                                  # once, before any worker starts (compiles; does not touch a GPU)
    n_videos = len(load_videos(args))
    if args.max_num > 0:
        n_videos = min(n_videos, args.max_num)
    out, (host_scaled, host_decoded) = test_ssn.run(args, n_videos, make_tester)
    if args.save_scores is not None:
        with open(args.save_scores, "wb") as f:
            pickle.dump({k: v[:-1] for k, v in out.items()}, f, pickle.HIGHEST_PROTOCOL)
    if args.save_raw_scores is not None:
        with open(args.save_raw_scores, "wb") as f:
            pickle.dump({k: v[-1] for k, v in out.items()}, f, pickle.HIGHEST_PROTOCOL)
    if args.gpu_decode:
        print("{} of {} videos were scaled with PIL on the host (frames more than 6x the scale size); {} files were decoded with PIL "
              "on the host (not baseline JPEG)".format(host_scaled, n_videos, host_decoded))
    return out


if __name__ == "__main__":
    main()
