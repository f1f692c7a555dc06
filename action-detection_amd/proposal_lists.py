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
    listing = builder.build_text(batch, frame_counts, paths)      # or the bytes of the whole file from the device
    write_proposal_bytes("list.txt", listing.data)                # (csrc/proposal_text.hip)

and the numbers are the reference's bit for bit: the chain is integer arithmetic and single IEEE float64 operations.
Quirks kept from the reference: ``time_step`` scales the step between windows but not their length; a video without
ground truth counts as recalled; a ground-truth span is hit only by an IoU strictly above the threshold.
"""
from collections import namedtuple
from types import SimpleNamespace

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


class ProposalListText(object):
    """What ``ProposalListBuilder.build_text`` brings back: ``data`` (bytes: the whole list file, for
    ``proposal_io.write_proposal_bytes``), ``offsets`` (host int64 [n_written + 1]: where every record's '# <index>' line
    begins, and the end), ``host_formatted`` (records the host had to format: status bit 2, a float outside what the
    device prints); ``status``, ``recall``, ``hits``, ``totals``, ``thresholds``, ``mean_proposals``, ``num_proposals`` as
    ``ProposalListResult`` has them, over ALL videos of the batch."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def record(self, k):
        """Record k behind its '# <index>' line, as text: what ``proposal_io.format_window_list_rows`` returns."""
        text = self.data[self.offsets[k]:self.offsets[k + 1]]
        return text[text.index(b"\n") + 1:].decode("utf-8")


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

    def _device_part(self, who, batch, frame_counts, recall_thresholds, thresh, extra=()):
        """What ``build`` and ``build_text`` share: the checks, ONE upload (ground truth, frame counts, thresholds and the
        host arrays of ``extra`` behind them) and the three launches.  -> a namespace of the device tensors and host tables."""
        v = len(batch.videos)
        dev = batch.windows.device
        thr = np.ascontiguousarray(np.asarray(recall_thresholds, dtype=np.float64).reshape(-1))
        if thr.size < 1:
            raise ValueError("%s: at least one recall threshold" % who)
        fc = np.zeros(v, dtype=np.int64) if frame_counts is None else np.asarray(frame_counts)
        if fc.shape != (v,) or fc.dtype.kind not in "iu" or (fc < 0).any() or (fc >= 2 ** 31).any():
            raise ValueError("%s: frame_counts must be one non-negative int32 per video" % who)
        gt = [[(i.num_label, i.time_span) for i in video.instances] for video in batch.videos]
        for video, g in zip(batch.videos, gt):
            if any(l is None for l, _ in g):
                raise ValueError("%s: an instance of video %s has no label index" % (who, video.id))
        totals = np.asarray([len(g) for g in gt], dtype=np.int64)
        g_off = np.concatenate([[0], np.cumsum(totals)])
        n_gt, n_pr = int(g_off[-1]), int(batch.offsets[-1])
        gt_span = np.asarray([s for g in gt for _, s in g], dtype=np.float64).reshape(-1, 2)
        gt_label = np.asarray([l for g in gt for l, _ in g], dtype=np.int32)
        if not np.isfinite(gt_span).all():
            raise ValueError("%s: a ground-truth span is not finite" % who)
        buf, rng = _pack([gt_span, gt_label, g_off.astype(np.int32), fc.astype(np.int32), thr] + list(extra))
        d = torch.from_numpy(buf).to(dev)                                                # the one upload
        part = [d[b:e] for b, e in rng]
        d_span, d_label, d_goff = part[0].view(torch.float64).reshape(-1, 2), part[1].view(torch.int32), part[2].view(torch.int32)
        d_fc, d_thr = part[3].view(torch.int32), part[4].view(torch.float64)

        label, iou, own = K.tag_name_proposals(d_span, d_label, d_goff, batch.windows, batch.d_offsets, thresh)
        gt_frames, frames, status = K.proposal_list_rows(d_span, d_goff, batch.windows, batch.d_offsets, d_fc, batch.d_durations)
        hits = K.eval_recall(d_span, d_goff, batch.windows, batch.d_offsets, d_thr)
        return SimpleNamespace(v=v, thr=thr, fc=fc, totals=totals, g_off=g_off, n_gt=n_gt, n_pr=n_pr, gt_label=gt_label,
                               d_label=d_label, d_goff=d_goff, d_fc=d_fc, extra=part[5:], label=label, iou=iou, own=own,
                               gt_frames=gt_frames, frames=frames, status=status, hits=hits)

    @staticmethod
    def _recall(hits, totals, n_gt, n_thr):
        v = len(totals)
        per_video = [np.sum(hits[:, t] == totals) / float(v) for t in range(n_thr)]
        with np.errstate(divide="ignore", invalid="ignore"):                             # no ground truth at all: 0 / 0, as the reference's
            per_inst = [np.sum(hits[:, t]) / np.float64(n_gt) for t in range(n_thr)]
        return list(zip(per_video, per_inst))

    @torch.no_grad()
    def build(self, batch, frame_counts=None, recall_thresholds=DEFAULT_RECALL_THRESHOLDS, thresh=0.0):
        """Name the proposals of every video (``name_proposal``), convert all spans to frame numbers at ``frame_counts[i] /
        duration`` frames per second (``dump_window_list``) and count the recalled ground truth at every threshold
        (``get_temporal_proposal_recall``).  One upload (ground truth, frame counts, thresholds), three launches, one
        download.  frame_counts None: zeros (the frame columns are then all 0)."""
        p = self._device_part("build", batch, frame_counts, recall_thresholds, thresh)
        v, thr, totals, g_off = p.v, p.thr, p.totals, p.g_off

        outs = [p.iou, p.own, p.label, p.frames, p.gt_frames, p.status, p.hits]          # (the float64 arrays first: alignment)
        sizes = [t.numel() * t.element_size() for t in outs]
        host = torch.cat([t.reshape(-1).view(torch.uint8) for t in outs]).cpu().numpy()  # the one download
        cut = np.concatenate([[0], np.cumsum(sizes)])
        h = [host[cut[i]:cut[i + 1]] for i in range(len(outs))]
        iou, own = h[0].view(np.float64), h[1].view(np.float64)
        label, frames, gt_frames = h[2].view(np.int32), h[3].view(np.int32).reshape(-1, 2), h[4].view(np.int32).reshape(-1, 2)
        status, hits = h[5].view(np.int32), h[6].view(np.int32).reshape(v, thr.size).astype(np.int64)

        po, go = batch.offsets, g_off
        written = p.gt_label + 1
        return ProposalListResult(
            labels=[label[po[i]:po[i + 1]] for i in range(v)], iou=[iou[po[i]:po[i + 1]] for i in range(v)],
            overlap_self=[own[po[i]:po[i + 1]] for i in range(v)], frames=[frames[po[i]:po[i + 1]] for i in range(v)],
            gt_labels=[written[go[i]:go[i + 1]] for i in range(v)], gt_frames=[gt_frames[go[i]:go[i + 1]] for i in range(v)],
            status=[int(s) for s in status], recall=self._recall(hits, totals, p.n_gt, thr.size), hits=hits, totals=totals,
            thresholds=thr, mean_proposals=np.mean(np.diff(po)), num_proposals=p.n_pr)

    @torch.no_grad()
    def build_text(self, batch, frame_counts, paths, write=None, first_index=1, recall_thresholds=DEFAULT_RECALL_THRESHOLDS,
                   thresh=0.0):
        """``build`` with the list file formed on the device (csrc/proposal_text.hip): the records of the videos ``write``
        (indices into the batch, in the order given; None: all) under '# <first_index + k>' lines, ``paths[i]`` the path
        written for video i -- byte for byte what ``proposal_io.write_proposal_file`` writes from ``format_window_list_rows``.
        Recall counts every video of the batch, written or not.  One upload (the path bytes ride along), six launches, two
        host reads: the byte count, then text, hits and status; the per-row arrays stay on the device.  A written video
        with a float the device does not print (status bit 2: NaN, inf, 2^32 and beyond) is formatted on the host from its
        downloaded rows and spliced in (``host_formatted`` counts them)."""
        v = len(batch.videos)
        if len(paths) != v:
            raise ValueError("build_text: %d paths for %d videos" % (len(paths), v))
        write = np.arange(v, dtype=np.int64) if write is None else np.asarray(write).reshape(-1)
        if write.size and (write.dtype.kind not in "iu" or write.min() < 0 or write.max() >= v):
            raise ValueError("build_text: write holds indices into the %d videos of the batch" % v)
        write = write.astype(np.int64)
        first_index = int(first_index)
        if first_index < 0 or first_index + write.size >= 2 ** 31:
            raise ValueError("build_text: first_index %d" % first_index)
        raw = []
        for i in write:
            path = str(paths[i])
            if "\n" in path or "\r" in path:
                raise ValueError("build_text: the path of video %s holds a line break: %r" % (batch.videos[i].id, path))
            raw.append(path.encode("utf-8"))
        path_off = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
        if path_off[-1] >= 2 ** 30:
            raise ValueError("build_text: %d bytes of paths (2^30 or more), split the batch" % path_off[-1])
        totals = np.asarray([len(video.instances) for video in batch.videos], dtype=np.int64)
        item_off = K.proposal_text_items(np.concatenate([[0], np.cumsum(totals)]), batch.offsets, write)
        if item_off[-1] >= 2 ** 31:
            raise ValueError("build_text: %d rows to write (2^31 or more), split the batch" % item_off[-1])
        path_bytes = np.frombuffer(b"".join(raw), dtype=np.uint8)
        p = self._device_part("build_text", batch, frame_counts, recall_thresholds, thresh,
                              extra=[path_off.astype(np.int32), write.astype(np.int32), item_off.astype(np.int32), path_bytes])
        thr = p.thr
        small = [p.status, p.hits]
        data, offsets, host_formatted = b"", np.zeros(1, dtype=np.int64), 0
        if write.size:
            d_poff, d_write, d_ioff = (t.view(torch.int32) for t in p.extra[:3])
            d_paths = p.extra[3]
            inp = K.ProposalTextInputs(p.d_label + 1, p.gt_frames, p.d_goff, p.label, p.iou, p.own, p.frames, batch.d_offsets,
                                       p.d_fc, d_paths, d_poff, d_write, d_ioff, int(item_off[-1]), first_index)
            bp, _ = K.proposal_text_size(inp, p.status)
            total = int(bp[-1].item())                                                   # host read 1: the size of the text
            if total < 0:
                raise ValueError("build_text: the text has 2^31 bytes or more, split the batch")
            out = torch.zeros(max(total, 1), device=p.status.device, dtype=torch.uint8)
            small.append(K.proposal_text_fill(inp, bp, out))
        sizes = [t.numel() * 4 for t in small]
        host = torch.cat([t.reshape(-1).view(torch.uint8) for t in small] + ([out[:total]] if write.size else [])).cpu().numpy()
        cut = np.concatenate([[0], np.cumsum(sizes)])                                    # host read 2: status, hits, offsets, text
        status = host[cut[0]:cut[1]].view(np.int32)
        hits = host[cut[1]:cut[2]].view(np.int32).reshape(v, thr.size).astype(np.int64)
        if write.size:
            offsets = host[cut[2]:cut[3]].view(np.int32).astype(np.int64)
            data = host[cut[3]:].tobytes()
            flagged = [k for k, i in enumerate(write) if status[i] & 4]
            if flagged:
                data, offsets = self._reformat(data, offsets, flagged, lambda k: (
                    first_index + k, raw[k].decode("utf-8"), int(p.fc[write[k]])) + self._rows_of(p, batch, int(write[k])))
                host_formatted = len(flagged)
        return ProposalListText(
            data=data, offsets=offsets, host_formatted=host_formatted, status=[int(s) for s in status],
            recall=self._recall(hits, p.totals, p.n_gt, thr.size), hits=hits, totals=p.totals, thresholds=thr,
            mean_proposals=np.mean(np.diff(batch.offsets)), num_proposals=p.n_pr)

    @staticmethod
    def _rows_of(p, batch, i):
        """The rows of video i from the device (only a video the device could not print needs them):
        the arguments of ``format_window_list_rows`` behind path and frame count."""
        po, go = batch.offsets, p.g_off
        part = lambda t, off: t[int(off[i]):int(off[i + 1])].cpu().numpy()      # noqa: E731
        return ((p.gt_label + 1)[go[i]:go[i + 1]], part(p.gt_frames, go), part(p.label, po), part(p.iou, po), part(p.own, po),
                part(p.frames, po))

    @staticmethod
    def _reformat(data, offsets, flagged, record_of):
        """Replace the records ``flagged`` (positions in the written order) of the device's text by the host's:
        ``record_of(k)`` -> (index, path, frame_cnt, gt_labels, gt_frames, labels, iou, overlap_self, frames).
        -> (data, offsets)."""
        from .proposal_io import format_window_list_rows
        flagged = set(flagged)
        pieces = []
        for k in range(len(offsets) - 1):
            if k in flagged:
                rec = record_of(k)
                pieces.append(("# %d\n" % rec[0] + format_window_list_rows(*rec[1:])).encode("utf-8"))
            else:
                pieces.append(data[offsets[k]:offsets[k + 1]])
        return b"".join(pieces), np.concatenate([[0], np.cumsum([len(x) for x in pieces])]).astype(np.int64)


def windows_per_video(batch):
    """The batch's proposals on the host, one float64 [K, 2] array per video (a download of its own; ``build`` does not need it)."""
    host = batch.windows.cpu().numpy()
    return [host[batch.offsets[i]:batch.offsets[i + 1]] for i in range(len(batch.videos))]
