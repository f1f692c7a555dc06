"""Which frames the actionness classifier trains and tests on: the index / label side of the reference's ``BinaryDataSet``
(/root/reference/load_binary_score.py:38-76 records, :120-146 pools, :179-195 frames of a proposal, :208-219 per-proposal
data, :223-241 sampling, :265-306 test ticks), without the image I/O -- the counterpart of ``proposal_sampling`` for
``binary_model.BinaryClassifier``.

``ActionnessSampler.sample_video(i)`` returns, for the 12 proposals the reference draws from video ``i`` (3 foreground, 9
background by default), the frame indices of the ``body_seg`` snippets and the type (1 foreground, 0 background), issuing
the same calls to numpy's global RNG in the same order as the reference: after ``np.random.seed(s)`` the picks are
identical.  ``test_ticks(video)`` gives the frames ``binary_test.py`` scores.
"""
from collections import namedtuple

import numpy as np
from numpy.random import randint

from .proposal_io import load_proposal_file

FG, BG = 1, 0

SampledActionness = namedtuple("SampledActionness", "video_id frame_indices prop_type")


class BinaryInstance(object):
    """A ground-truth instance or a proposal of one video, frame units (load_binary_score.py:12-31)."""

    def __init__(self, start_frame, end_frame, video_frame_count, label=None, overlap_self=None, iou=1.0):
        self.start_frame = start_frame
        self.end_frame = min(end_frame, video_frame_count)
        self.label = label if label is not None else -1
        self.iou = iou
        self.coverage = (end_frame - start_frame) / video_frame_count
        self.overlap_self = overlap_self


class BinaryVideoRecord(object):
    """One record of a processed proposal list with the filters of load_binary_score.py:47-58: empty spans and spans that
    start behind the last frame are dropped."""

    def __init__(self, record):
        self.id, n = record[0], int(record[1])
        self.num_frames = n
        self.gt = [BinaryInstance(int(x[1]), int(x[2]), n, label=int(x[0]), iou=1.0) for x in record[2] if int(x[2]) > int(x[1])]
        self.gt = [g for g in self.gt if g.start_frame < n]
        self.proposals = [BinaryInstance(int(x[3]), int(x[4]), n, label=int(x[0]), iou=float(x[1]), overlap_self=float(x[2]))
                          for x in record[3] if int(x[4]) > int(x[3])]
        self.proposals = [p for p in self.proposals if p.start_frame < n]

    def get_fg(self, fg_thresh, with_gt=True):
        fg = [p for p in self.proposals if p.iou > fg_thresh]
        if with_gt:
            fg.extend(self.gt)
        return fg

    def get_bg(self, bg_thresh):
        return [p for p in self.proposals if p.iou < bg_thresh]


class ActionnessSampler(object):
    def __init__(self, prop_file=None, records=None, body_seg=5, video_centric=True, new_length=1, random_shift=True,
                 prop_per_video=12, fg_ratio=3, bg_ratio=9, fg_iou_thresh=0.7, bg_iou_thresh=0.01, bg_coverage_thresh=0.02,
                 gt_as_fg=True, test_interval=6, exclude_empty=True, epoch_multiplier=1):
        self.body_seg, self.new_length = body_seg, new_length
        self.video_centric, self.random_shift, self.test_interval = video_centric, random_shift, test_interval
        self.fg_iou_thresh, self.bg_iou_thresh, self.bg_coverage_thresh = fg_iou_thresh, bg_iou_thresh, bg_coverage_thresh
        self.gt_as_fg = gt_as_fg
        self.epoch_multiplier = epoch_multiplier
        denum = fg_ratio + bg_ratio
        self.fg_per_video = int(prop_per_video * (fg_ratio / denum))
        self.bg_per_video = int(prop_per_video * (bg_ratio / denum))

        records = load_proposal_file(prop_file) if records is None else records
        self.video_list = [BinaryVideoRecord(r) for r in records]
        if exclude_empty:
            self.video_list = [v for v in self.video_list if len(v.gt) > 0]
        self.video_dict = {v.id: v for v in self.video_list}
        self.fg_pool, self.bg_pool = [], []
        for v in self.video_list:
            self.fg_pool.extend((v.id, p) for p in v.get_fg(fg_iou_thresh, gt_as_fg))
            self.bg_pool.extend((v.id, p) for p in v.get_bg(bg_iou_thresh))

    def __len__(self):
        return len(self.video_list) * self.epoch_multiplier

    # ---- which proposals (load_binary_score.py:223-241)
    def _draw(self, prop_type, video, pool, count, dataset_pool):
        if len(pool) == 0:      # nothing of this type in the video: borrow from the whole data set, without replacement
            return [(dataset_pool[x], prop_type) for x in np.random.choice(len(dataset_pool), count, replace=False)]
        picks = np.random.choice(len(pool), count, replace=len(pool) < count)
        return [((video.id, pool[x]), prop_type) for x in picks]

    def pick_proposals(self, video):
        fg = video.get_fg(self.fg_iou_thresh, self.gt_as_fg)
        bg = video.get_bg(self.bg_iou_thresh)
        return (self._draw(FG, video, fg, self.fg_per_video, self.fg_pool)
                + self._draw(BG, video, bg, self.bg_per_video, self.bg_pool))

    # ---- which frames (load_binary_score.py:179-195, 215-217)
    def _sample_frames(self, prop):
        start = prop.start_frame + 1
        duration = prop.end_frame - start + 1
        sample_duration = duration / self.body_seg
        if sample_duration < 1:
            return start + randint(prop.end_frame - prop.start_frame, size=self.body_seg)
        split = [int(np.round(i * sample_duration)) + start for i in range(self.body_seg + 1)]
        out = []
        for i in range(self.body_seg):
            out.extend(np.random.choice(range(split[i], split[i + 1]), 1))
        return out

    def snippet_indices(self, prop, frame_cnt):
        """-> the frames of the body_seg snippets of one proposal, new_length each, clamped to the last frame."""
        return [min(frame_cnt, int(idx) + x) for idx in self._sample_frames(prop) for x in range(self.new_length)]

    def describe(self, picked):
        (vid, inst), prop_type = picked
        return SampledActionness(vid, self.snippet_indices(inst, self.video_dict[vid].num_frames), prop_type)

    def sample_video(self, index):
        """The proposals of one training sample in the reference's order (foreground, then background) and the type array
        ``get_training_data`` returns besides the frames."""
        video = self.video_list[index % len(self.video_list)]
        props = [self.describe(p) for p in self.pick_proposals(video)]
        return props, {"prop_type": np.array([p.prop_type for p in props])}

    # ---- testing (load_binary_score.py:265-272)
    def test_ticks(self, video):
        """-> the frame every tick starts at (1-based); a tick is new_length frames from there, clamped to the last frame."""
        return np.arange(0, video.num_frames - self.new_length, self.test_interval, dtype=int) + 1

    def test_frames(self, video):
        """-> [T, new_length] frame numbers the test generator loads (load_binary_score.py:291-294)."""
        n = video.num_frames
        return np.array([[min(n, int(p) + x) for x in range(self.new_length)] for p in self.test_ticks(video)],
                        dtype=np.int64).reshape(-1, self.new_length)
