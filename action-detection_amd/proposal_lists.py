"""The proposal-list stage for a whole subset at once: from video records (``datasets``) and proposals -- exponential
sliding windows made on the device, or the spans of ``TagProposalGenerator`` -- to every number of the list file the
trainers and the tester read, in a constant number of launches and copies whatever the number of videos.

The reference does this per video in Python loops (/root/reference/gen_sliding_window_proposals.py:45-62,
gen_bottom_up_proposals.py:159-186: gen_exponential_sw_proposal, name_proposal, get_temporal_proposal_recall,
dump_window_list).  Here

    builder = ProposalListBuilder()
    batch = builder.sliding_windows(videos, overlap=0.7)          # csrc/proposal_list.hip; the windows stay on the device
    result = builder.build(batch, frame_counts)                   # naming, frame numbers, recall; one upload, one download
    text = format_window_list_rows(path, frame_cnt, *result.rows(i))

and the numbers are the reference's bit for bit: the chain is integer arithmetic and single IEEE float64 operations.
Quirks kept from the reference: ``time_step`` scales the step between windows but not their length; a video without
ground truth counts as recalled; a ground-truth span is hit only by an IoU strictly above the threshold.
"""
from collections import namedtuple

import numpy as np
import torch

from . import kernels as K
from .tag_proposals import _default_device

DEFAULT_RECALL_THRESHOLDS = (0.5, 0.7, 0.9)          # gen_sliding_window_proposals.py:54

ProposalBatch = namedtuple("ProposalBatch", "videos durations windows offsets d_offsets d_durations")
ProposalBatch.__doc__ = """Proposals of a list of videos, resident on the device: windows float64 [W, 2] (seconds), ragged
by offsets (host int64 [V + 1]; d_offsets: the int32 device copy); durations float64 [V] (host; d_durations: device)."""


class ProposalListResult(object):
    """What ``ProposalListBuilder.build`` brings back.  Per video (lists of numpy views in the order of the batch):
    ``labels`` int32 [K] (label + 1, or 0), ``iou`` and ``overlap_self`` float64 [K], ``frames`` int32 [K, 2], ``gt_labels``
    int32 [n] (label + 1, as written), ``gt_frames`` int32 [n, 2], ``status`` (bit 0: a ground-truth position, bit 1: a
    proposal position of the video was not finite or did not fit int32 and reads 0).  ``recall``: one (per video, per
    instance) pair per threshold; ``hits`` int [V, T] and ``totals`` [V] behind it; ``mean_proposals``."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def rows(self, i):
        """The arrays of video i in the argument order of ``proposal_io.format_window_list_rows`` (behind path, frame_cnt)."""
        return (self.gt_labels[i], self.gt_frames[i], self.labels[i], self.iou[i], self.overlap_self[i], self.frames[i])


def _pack(arrays):
    """Host arrays -> one uint8 buffer with every array at an 8-byte boundary, and the byte ranges."""
    ranges, pos = [], 0
    for a in arrays:
        ranges.append((pos, pos + a.nbytes))
        pos += (a.nbytes + 7) // 8 * 8
    buf = np.zeros(max(pos, 8), dtype=np.uint8)
    for a, (b, e) in zip(arrays, ranges):
        buf[b:e] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return buf, ranges


class ProposalListBuilder(object):
    def __init__(self, device=None):
        self.device = device

    def _device(self):
        return torch.device(self.device) if self.device is not None else _default_device()

    @staticmethod
    def _durations(videos, who):
        if len(videos) < 1:
            raise ValueError("%s: at least one video" % who)
        dur = np.asarray([float(v.duration) for v in videos], dtype=np.float64)
        if not np.isfinite(dur).all():
            raise ValueError("%s: the duration of %s is not finite" % (who, videos[int(np.flatnonzero(~np.isfinite(dur))[0])].id))
        return dur

    @torch.no_grad()
    def sliding_windows(self, videos, overlap=0.7, max_level=8, time_step=1):
        """``gen_exponential_sw_proposal`` (ops/sequence_funcs.py:37-54) for every video: per level l < max_level windows of
        2**l seconds every ``int(ceil(2**l * time_step * (1 - overlap)))`` seconds, kept while at least one second lies
        inside the video; per video level ascending, start ascending.  Count launch, one host read, fill launch."""
        max_level = int(max_level)
        if max_level < 1 or max_level > 31:
            raise ValueError("sliding_windows: max_level must lie in 1 ... 31, got %d" % max_level)
        spans = [2 ** x for x in range(max_level)]
        steps = [float(np.ceil(t * time_step * (1 - overlap))) for t in spans]
        for t, s in zip(spans, steps):
            if not s >= 1 or s >= 2 ** 31:
                raise ValueError("sliding_windows: overlap %r and time_step %r give a step of %r for the %d s windows; "
                                 "it must be at least 1" % (overlap, time_step, s, t))
        steps = [int(s) for s in steps]
        dur = self._durations(videos, "sliding_windows")
        if (dur / min(steps)).max() >= 2 ** 30:
            raise ValueError("sliding_windows: 2^30 windows or more in one level of one video")
        dev = self._device()
        d_dur = torch.from_numpy(dur).to(dev)
        counts = K.sw_count(d_dur, spans, steps).cpu().numpy().astype(np.int64)          # the one host read
        level_off = np.concatenate([[0], np.cumsum(counts.ravel())])
        total = int(level_off[-1])
        if total >= 2 ** 30:
            raise ValueError("sliding_windows: %d windows in one batch (2^30 or more), split it" % total)
        windows = K.sw_fill(torch.from_numpy(level_off.astype(np.int32)).to(dev), spans, steps, total)
        offsets = level_off[::max_level].copy()
        return ProposalBatch(list(videos), dur, windows, offsets, torch.from_numpy(offsets.astype(np.int32)).to(dev), d_dur)

    @torch.no_grad()
    def from_spans(self, videos, spans_per_video):
        """Proposals given in seconds, one [K, 2] array per video (``TagResult.seconds``): one concatenated upload."""
        if len(videos) != len(spans_per_video):
            raise ValueError("from_spans: one span array per video")
        dur = self._durations(videos, "from_spans")
        spans = [np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in spans_per_video]
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in spans])]).astype(np.int64)
        if offsets[-1] >= 2 ** 30:
            raise ValueError("from_spans: %d spans in one batch (2^30 or more), split it" % offsets[-1])
        buf, (r_span, r_off, r_dur) = _pack([np.concatenate(spans), offsets.astype(np.int32), dur])
        d = torch.from_numpy(buf).to(self._device())
        return ProposalBatch(list(videos), dur, d[r_span[0]:r_span[1]].view(torch.float64).reshape(-1, 2), offsets,
                             d[r_off[0]:r_off[1]].view(torch.int32), d[r_dur[0]:r_dur[1]].view(torch.float64))

    @torch.no_grad()
    def build(self, batch, frame_counts=None, recall_thresholds=DEFAULT_RECALL_THRESHOLDS, thresh=0.0):
        """Name the proposals of every video (``name_proposal``), convert all spans to frame numbers at ``frame_counts[i] /
        duration`` frames per second (``dump_window_list``) and count the recalled ground truth at every threshold
        (``get_temporal_proposal_recall``).  One upload (ground truth, frame counts, thresholds), three launches, one
        download.  frame_counts None: zeros (the frame columns are then all 0)."""
        v = len(batch.videos)
        dev = batch.windows.device
        thr = np.ascontiguousarray(np.asarray(recall_thresholds, dtype=np.float64).reshape(-1))
        if thr.size < 1:
            raise ValueError("build: at least one recall threshold")
        fc = np.zeros(v, dtype=np.int64) if frame_counts is None else np.asarray(frame_counts)
        if fc.shape != (v,) or fc.dtype.kind not in "iu" or (fc < 0).any() or (fc >= 2 ** 31).any():
            raise ValueError("build: frame_counts must be one non-negative int32 per video")
        gt = [[(i.num_label, i.time_span) for i in video.instances] for video in batch.videos]
        for video, g in zip(batch.videos, gt):
            if any(l is None for l, _ in g):
                raise ValueError("build: an instance of video %s has no label index" % video.id)
        totals = np.asarray([len(g) for g in gt], dtype=np.int64)
        g_off = np.concatenate([[0], np.cumsum(totals)])
        n_gt, n_pr = int(g_off[-1]), int(batch.offsets[-1])
        gt_span = np.asarray([s for g in gt for _, s in g], dtype=np.float64).reshape(-1, 2)
        gt_label = np.asarray([l for g in gt for l, _ in g], dtype=np.int32)
        if not np.isfinite(gt_span).all():
            raise ValueError("build: a ground-truth span is not finite")
        buf, rng = _pack([gt_span, gt_label, g_off.astype(np.int32), fc.astype(np.int32), thr])
        d = torch.from_numpy(buf).to(dev)                                                # the one upload
        part = [d[b:e] for b, e in rng]
        d_span, d_label, d_goff = part[0].view(torch.float64).reshape(-1, 2), part[1].view(torch.int32), part[2].view(torch.int32)
        d_fc, d_thr = part[3].view(torch.int32), part[4].view(torch.float64)

        label, iou, own = K.tag_name_proposals(d_span, d_label, d_goff, batch.windows, batch.d_offsets, thresh)
        gt_frames, frames, status = K.proposal_list_rows(d_span, d_goff, batch.windows, batch.d_offsets, d_fc, batch.d_durations)
        hits = K.eval_recall(d_span, d_goff, batch.windows, batch.d_offsets, d_thr)

        outs = [iou, own, label, frames, gt_frames, status, hits]                        # (the float64 arrays first: alignment)
        sizes = [t.numel() * t.element_size() for t in outs]
        host = torch.cat([t.reshape(-1).view(torch.uint8) for t in outs]).cpu().numpy()  # the one download
        cut = np.concatenate([[0], np.cumsum(sizes)])
        h = [host[cut[i]:cut[i + 1]] for i in range(len(outs))]
        iou, own = h[0].view(np.float64), h[1].view(np.float64)
        label, frames, gt_frames = h[2].view(np.int32), h[3].view(np.int32).reshape(-1, 2), h[4].view(np.int32).reshape(-1, 2)
        status, hits = h[5].view(np.int32), h[6].view(np.int32).reshape(v, thr.size).astype(np.int64)

        po, go = batch.offsets, g_off
        per_video = [np.sum(hits[:, t] == totals) / float(v) for t in range(thr.size)]
        with np.errstate(divide="ignore", invalid="ignore"):                             # no ground truth at all: 0 / 0, as the reference's
            per_inst = [np.sum(hits[:, t]) / np.float64(n_gt) for t in range(thr.size)]
        written = gt_label + 1
        return ProposalListResult(
            labels=[label[po[i]:po[i + 1]] for i in range(v)], iou=[iou[po[i]:po[i + 1]] for i in range(v)],
            overlap_self=[own[po[i]:po[i + 1]] for i in range(v)], frames=[frames[po[i]:po[i + 1]] for i in range(v)],
            gt_labels=[written[go[i]:go[i + 1]] for i in range(v)], gt_frames=[gt_frames[go[i]:go[i + 1]] for i in range(v)],
            status=[int(s) for s in status], recall=list(zip(per_video, per_inst)), hits=hits, totals=totals,
            thresholds=thr, mean_proposals=np.mean(np.diff(po)), num_proposals=n_pr)


def windows_per_video(batch):
    """The batch's proposals on the host, one float64 [K, 2] array per video (a download of its own; ``build`` does not need it)."""
    host = batch.windows.cpu().numpy()
    return [host[batch.offsets[i]:batch.offsets[i + 1]] for i in range(len(batch.videos))]
