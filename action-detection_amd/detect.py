"""Annotation-free detection: frames in, detections out, with every stage's data staying on the device.

The file-based workflow goes actionness pickle -> ``gen_bottom_up_proposals`` -> list file -> ``load_proposal_file`` ->
``VideoRecord`` -> ``ProposalSampler.test_ticks`` -> ``STPPReorgainzed.host_ranges`` -> score pickle -> evaluation, needs
ground truth to write the list, and loops over every proposal in Python between the backbone and the pooling launch.  Here

    table = build_test_table(frames, p_off, frame_counts, new_length, test_interval, stpp_cfg)

turns the frame-number columns of ALL videos into everything ``score_video_ranges`` (``DenseTester.score_video`` without its host
part) takes (csrc/test_table.hip: a constant number of launches, one host read), and

    result = ActionDetector(ssn=[...], actionness=[...], tag=..., post=...).detect(videos)

chains actionness scoring, TAG, the test table, SSN scoring (one or more streams, fused on the device) and the batched
post-processing.  Every number equals what the file chain gives for the same videos with ``exclude_empty=False``: the stages
are the existing ones, the table restates the host arithmetic one IEEE operation at a time.
"""
import pickle
from collections import namedtuple

import numpy as np
import torch

from . import kernels as K
from .proposal_lists import ProposalListBuilder
from .tag_proposals import _default_device, merge_scores_device
from .test_data import test_frame_batches

TableRows = namedtuple("TableRows", "src rel ticks scaling ranges act")
TableRows.__doc__ = """The rows of one video in a TestTable (device views): src int32 [K] (index of the proposal in the
video's input, -1: the whole-video row), rel float64 [K, 2], ticks int32 [K, 4], scaling float64 [K, 2], ranges int32
[K, n_parts, 2], act int32 [K, 2]."""


class TestTable(object):
    """What ``build_test_table`` returns, on the device: ``src / rel / ticks / scaling / ranges / act`` for the K rows of all
    videos one after the other (see TableRows), ``k_off`` int32 [V + 1] (``h_k_off``: the host copy), ``keep`` int32 [P]
    (the input proposals the records keep), ``n_rows`` (host int64 [V]: ticks of every video)."""
    __test__ = False      # (a library class whose name starts with "Test": not a test case)

    def __init__(self, src, rel, ticks, scaling, ranges, act, k_off, h_k_off, keep, n_rows):
        self.src, self.rel, self.ticks, self.scaling, self.ranges, self.act = src, rel, ticks, scaling, ranges, act
        self.k_off, self.h_k_off, self.keep, self.n_rows = k_off, h_k_off, keep, n_rows

    def __len__(self):
        return len(self.n_rows)

    def video(self, i):
        b, e = int(self.h_k_off[i]), int(self.h_k_off[i + 1])
        return TableRows(self.src[b:e], self.rel[b:e], self.ticks[b:e], self.scaling[b:e], self.ranges[b:e], self.act[b:e])


def _name(video_ids, i):
    return "%r" % (video_ids[i],) if video_ids is not None else "#%d" % i


@torch.no_grad()
def build_test_table(frames, p_off, frame_counts, new_length, test_interval, stpp_cfg, device=None, video_ids=None):
    """frames: int [P, 2] (start, end) frame numbers as a list file holds them, a host array or a device tensor (the
    ``frames`` output of ``kernels.proposal_list_rows``); p_off: int [V + 1], the videos' shares of the rows (host array or
    device tensor); frame_counts: host ints [V].  -> TestTable for a tester with ``new_length`` frames per tick, a tick every
    ``test_interval`` frames, and the STPP configuration ``stpp_cfg``.

    A video of fewer than 2 frames or without a tick, and a negative frame number, raise ValueError naming the video (the
    host path divides by zero or raises there): host inputs are checked before any launch, device-resident frames by the
    marking launch, whose per-video counts -- the one host read -- carry the verdict."""
    fc = np.asarray(frame_counts)
    v = fc.shape[0] if fc.ndim == 1 else 0
    if v < 1 or fc.dtype.kind not in "iu":
        raise ValueError("build_test_table: frame_counts must be one int per video, at least one video")
    if video_ids is not None and len(video_ids) != v:
        raise ValueError("build_test_table: one id per video")
    new_length, test_interval = int(new_length), int(test_interval)
    if new_length < 1 or test_interval < 1:
        raise ValueError("build_test_table: new_length and test_interval must be at least 1")
    K.test_table_stages(stpp_cfg)                                       # (refuses more than 16 parts)
    fc = fc.astype(np.int64)
    n_rows = np.maximum(0, -((fc - new_length) // -test_interval))      # len(np.arange(0, frame_cnt - new_length, test_interval))
    for i in range(v):
        if fc[i] < 2 or fc[i] >= 2 ** 31:
            raise ValueError("build_test_table: video %s has %d frames, at least 2 are needed" % (_name(video_ids, i), fc[i]))
        if n_rows[i] < 1:
            raise ValueError("build_test_table: video %s (%d frames) has no tick for new_length %d"
                             % (_name(video_ids, i), fc[i], new_length))
    if torch.is_tensor(frames) and frames.device.type != "cpu":
        dev = frames.device
        d_frames = frames.to(torch.int32).reshape(-1, 2).contiguous()
        h_off = None if torch.is_tensor(p_off) and p_off.device.type != "cpu" else np.asarray(p_off)
    else:
        dev = torch.device(device) if device is not None else _default_device()
        h_frames = np.asarray(frames.numpy() if torch.is_tensor(frames) else frames).reshape(-1, 2)
        h_off = np.asarray(p_off.cpu().numpy() if torch.is_tensor(p_off) else p_off)
        if h_frames.size and h_frames.dtype.kind not in "iu":
            raise ValueError("build_test_table: frame numbers must be integers, got %s" % h_frames.dtype)
        if h_frames.size and (np.abs(h_frames.astype(np.int64)) >= 2 ** 31).any():
            raise ValueError("build_test_table: a frame number does not fit int32")
        d_frames = None
    if h_off is not None:
        h_off = h_off.astype(np.int64)
        n_p = d_frames.shape[0] if d_frames is not None else h_frames.shape[0]
        if h_off.shape != (v + 1,) or h_off[0] != 0 or (np.diff(h_off) < 0).any() or h_off[-1] != n_p:
            raise ValueError("build_test_table: p_off must be [V + 1] non-decreasing from 0 to the %d proposals" % n_p)
    if d_frames is None:
        neg = np.flatnonzero((h_frames < 0).any(axis=1))
        if neg.size:
            i = int(np.searchsorted(h_off, neg[0], side="right")) - 1
            raise ValueError("build_test_table: video %s holds a negative frame number" % _name(video_ids, i))
        d_frames = torch.from_numpy(np.ascontiguousarray(h_frames.astype(np.int32))).to(dev)
    d_off = torch.from_numpy(h_off.astype(np.int32)).to(dev) if h_off is not None else p_off.to(torch.int32).contiguous()
    if d_off.shape != (v + 1,):
        raise ValueError("build_test_table: p_off must be [V + 1]")
    small = torch.from_numpy(np.stack([fc, n_rows]).astype(np.int32)).to(dev)
    d_fc, d_rows = small[0], small[1]

    keep, pre, bp, counts = K.test_table_mark(d_frames, d_off, d_fc)
    counts = counts.cpu().numpy().astype(np.int64)                      # the one host read
    if (counts < 0).any():
        raise ValueError("build_test_table: video %s holds a negative frame number" % _name(video_ids, int(np.argmax(counts < 0))))
    h_k_off = np.concatenate([[0], np.cumsum(counts)])
    d_k_off = torch.from_numpy(h_k_off.astype(np.int32)).to(dev)
    src, rel, ticks, scaling, ranges, act = K.test_table_fill(d_frames, d_off, d_fc, d_rows, keep, pre, bp, d_k_off,
                                                              int(h_k_off[-1]), stpp_cfg)
    return TestTable(src, rel, ticks, scaling, ranges, act, d_k_off, h_k_off, keep, n_rows)


# ------------------------------------------------------------------------------------------------------------------ the tester's side
@torch.no_grad()
def score_video_ranges(tester, frames_gen, frame_cnt, ranges, act, scaling, num_crop=10):
    """``DenseTester.score_video`` of ``tester`` from the video's rows of a test table: ``ranges`` int32 [P, n_parts, 2], ``act`` int32
    [P, 2] and ``scaling`` [P, 2] on the device, pooled by ``STPPReorgainzed.forward_ranges`` in place of ``forward``.  No host work
    per proposal and no upload of ranges stand between the backbone's last launch and the pooling launch (``frame_scores`` keeps its
    one read per video, the poll of the range guard).  -> (act_scores, comp_scores, reg_scores or None, output)."""
    output = tester.frame_scores(frames_gen, frame_cnt, num_crop)
    act_s, comp_s, reg_s = tester.reorg.forward_ranges(output, ranges, act, scaling)
    if reg_s is not None:
        reg_s = reg_s.reshape(-1, tester.num_class, 2)
        if tester.stats is not None:
            K.reg_denorm(reg_s, tester.stats[0][0], tester.stats[1][0], tester.stats[0][1], tester.stats[1][1])
    return act_s, comp_s, reg_s, output


def _ranges_scorer(scorer):
    """The scorer's own ``score_video_ranges`` where it has one; otherwise the function above on it (a ``DenseTester``)."""
    return getattr(scorer, "score_video_ranges", None) or (lambda *a, **kw: score_video_ranges(scorer, *a, **kw))


# ------------------------------------------------------------------------------------------------------------------ the detector
class Stream(namedtuple("Stream", "scorer reader transform new_length weight")):
    """One network of the detector: ``scorer`` (a ``DenseTester`` / ``ActionnessTester`` or anything with the signature of
    ``score_video_ranges`` above without its first argument / of ``ActionnessTester.score_video``), the ``reader`` and ``transform`` pair ``test_data.test_frame_batches`` takes,
    the frames per tick, and the fusion weight (None for all streams: equal weights, as ``merge_detection_scores``)."""
    __slots__ = ()

    def __new__(cls, scorer, reader, transform, new_length=1, weight=None):
        return super(Stream, cls).__new__(cls, scorer, reader, transform, int(new_length), weight)


_Video = namedtuple("_Video", "id num_frames duration")


class _TickRule(object):
    """The two things ``test_frame_batches`` asks of a sampler: ``new_length`` and the frame ticks of ``test_ticks``."""

    def __init__(self, new_length, test_interval):
        self.new_length, self.test_interval = new_length, test_interval

    def test_ticks(self, video):
        return (np.arange(0, video.num_frames - self.new_length, self.test_interval, dtype=int) + 1,)


def _weights(streams):
    given = [s.weight for s in streams]
    if all(w is None for w in given):
        return None
    if any(w is None for w in given):
        raise ValueError("give every stream a weight or none")
    return [float(w) for w in given]


def fuse_scores(parts, weights=None):
    """``detection_eval.merge_detection_scores`` for one part (activity, completeness or regression scores) of one video, on
    the device: ``parts`` holds the streams' float32 tensors.  Its operations in its order and precision -- with weights
    ``np.array(weights) / sum(weights)``, float64, every product and the running sum in float64; without, the float32
    products with ``1.0 / len`` rounded to float32 and a float32 running sum -- so the result equals the host's bit for bit."""
    if parts[0] is None:
        return None
    if weights:
        w = np.array(weights) / sum(weights)
        out = parts[0].to(torch.float64) * float(w[0])
        for p, wi in zip(parts[1:], w[1:]):
            out = out + p.to(torch.float64) * float(wi)
        return out
    w = 1.0 / len(parts)
    out = parts[0] * w
    for p in parts[1:]:
        out = out + p * w
    return out


class ActionDetector(object):
    """``ssn`` / ``actionness``: lists of ``Stream`` (or tuples in its field order); ``tag``: a ``TagProposalGenerator``; ``post``:
    a ``DetectionPostProcessor``.  ``frame_interval`` / ``actionness_interval``: frames between two ticks of the SSN /
    actionness networks; ``stpp_cfg``: the testers' STPP configuration (default: that of the first scorer that has one)."""

    def __init__(self, ssn, actionness=None, tag=None, post=None, frame_interval=6, actionness_interval=5, test_crops=10,
                 tick_batch=32, stpp_cfg=None, device=None):
        self.ssn = [s if isinstance(s, Stream) else Stream(*s) for s in ssn]
        self.actionness = [s if isinstance(s, Stream) else Stream(*s) for s in (actionness or [])]
        if not self.ssn:
            raise ValueError("ActionDetector: at least one SSN stream")
        if post is None:
            raise ValueError("ActionDetector: a DetectionPostProcessor is needed")
        self.tag, self.post = tag, post
        self.frame_interval, self.actionness_interval = int(frame_interval), int(actionness_interval)
        self.test_crops, self.tick_batch = int(test_crops), int(tick_batch)
        if stpp_cfg is None:
            cfgs = [s.scorer.reorg.stpp_cfg for s in self.ssn if hasattr(s.scorer, "reorg")]
            stpp_cfg = cfgs[0] if cfgs else (1, 1, 1)
        self.stpp_cfg = stpp_cfg
        self.device = device

    def _device(self):
        return torch.device(self.device) if self.device is not None else _default_device()

    def _gen(self, stream, video, interval):
        return test_frame_batches(_TickRule(stream.new_length, interval), video, stream.reader, stream.transform, self.tick_batch)

    # ---- steps 1 and 2
    def score_actionness(self, videos):
        """-> one ``{video id: mean scores float32 [T, 2]}`` per actionness stream (device)."""
        if not self.actionness:
            raise ValueError("detect: no actionness stream, give proposals= or actionness_scores=")
        out = []
        for st in self.actionness:
            rule = _TickRule(st.new_length, self.actionness_interval)
            scores = {}
            for video in videos:
                n = len(rule.test_ticks(video)[0])
                if n < 1:
                    raise ValueError("detect: video %r (%d frames) has no tick for the actionness stream" % (video.id, video.num_frames))
                scores[video.id] = st.scorer.score_video(self._gen(st, video, self.actionness_interval), n, num_crop=self.test_crops)[1]
            out.append(scores)
        return out

    def _merged_actionness(self, videos, given):
        dev = self._device()
        if given is None:
            streams = self.score_actionness(videos)
            weights = _weights(self.actionness)
        else:
            streams = [given] if isinstance(given, dict) else list(given)
            weights = _weights(self.actionness) if len(self.actionness) == len(streams) else None
            streams = [{v.id: (s[v.id] if torch.is_tensor(s[v.id]) else torch.from_numpy(np.ascontiguousarray(s[v.id], dtype=np.float32))
                               ).to(dev, torch.float32) for v in videos} for s in streams]
        if len(streams) == 1:
            return streams[0]
        return merge_scores_device(streams, weights)

    # ---- steps 3 and 4
    def propose(self, videos, merged):
        if self.tag is None:
            raise ValueError("detect: no TagProposalGenerator, give proposals=")
        results = self.tag.generate([merged[v.id] for v in videos], [v.duration for v in videos])
        return [r.seconds for r in results]

    def tables_for(self, videos, spans):
        """Seconds -> frame numbers (what a list file would hold) -> one TestTable per distinct ``new_length`` of the SSN streams."""
        dev = self._device()
        batch = ProposalListBuilder(dev).from_spans(videos, spans)
        fc = np.asarray([v.num_frames for v in videos], dtype=np.int64)
        d_fc = torch.from_numpy(fc.astype(np.int32)).to(dev)
        no_gt = torch.zeros((0, 2), device=dev, dtype=torch.float64)
        no_off = torch.zeros(len(videos) + 1, device=dev, dtype=torch.int32)
        _, frames, _ = K.proposal_list_rows(no_gt, no_off, batch.windows.contiguous(), batch.d_offsets.contiguous(), d_fc,
                                            batch.d_durations.contiguous())
        ids = [v.id for v in videos]
        tables = {}
        for st in self.ssn:
            if st.new_length not in tables:
                tables[st.new_length] = build_test_table(frames, batch.offsets, fc, st.new_length, self.frame_interval,
                                                         self.stpp_cfg, video_ids=ids)
        return frames, batch.offsets, tables

    # ---- steps 5 and 6
    @torch.no_grad()
    def detect(self, videos, proposals=None, actionness_scores=None, video_cls_scores=None):
        """videos: ``[(video id, frame count, duration in seconds)]``.  proposals: one [K, 2] array of seconds per video (skips
        actionness scoring, merging and TAG); actionness_scores: ``{video id: [T, 2]}`` merged, or a list of such dictionaries
        per stream (skips the scoring); video_cls_scores: ``{video id: [C]}`` of an external classifier.  -> DetectionResult."""
        videos = [_Video(v[0], int(v[1]), float(v[2])) for v in videos]
        if not videos:
            raise ValueError("detect: no video")
        merged = None
        if proposals is None:
            merged = self._merged_actionness(videos, actionness_scores)
            spans = self.propose(videos, merged)
        else:
            if len(proposals) != len(videos):
                raise ValueError("detect: one proposal array per video")
            spans = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in proposals]
        frames, p_off, tables = self.tables_for(videos, spans)
        first = tables[self.ssn[0].new_length]
        per_stream = []
        for st in self.ssn:
            table, out, score = tables[st.new_length], [], _ranges_scorer(st.scorer)
            for i, video in enumerate(videos):
                rows = table.video(i)
                act, comp, reg, _ = score(self._gen(st, video, self.frame_interval), int(table.n_rows[i]), rows.ranges, rows.act,
                                          rows.scaling, num_crop=self.test_crops)
                out.append((act, comp, reg))
            per_stream.append(out)
        weights = _weights(self.ssn)
        scores = {}
        for i, video in enumerate(videos):
            parts = [ps[i] for ps in per_stream]
            if len(parts) == 1 and weights is None:
                act, comp, reg = parts[0]
            else:
                act, comp, reg = (fuse_scores([p[k] for p in parts], weights) for k in range(3))
            scores[video.id] = (first.video(i).rel, act, comp, reg)
        detections = self.post.process_videos(scores, video_cls_scores=video_cls_scores)
        return DetectionResult(videos, spans, frames, p_off, first, tables, merged, scores, detections)


class DetectionResult(object):
    """``videos`` (id, frames, duration); ``spans``: the proposals in seconds, one float64 [K, 2] array per video; ``frames`` int32
    [P, 2] (device) and ``p_off``: their frame numbers, as a list file would hold them; ``table``: the TestTable of the first
    SSN stream (``tables``: by new_length); ``actionness``: the merged actionness scores or None; ``scores``: ``{video id: (rel,
    act, comp, reg)}`` on the device; ``detections``: the BatchedDetections."""

    def __init__(self, videos, spans, frames, p_off, table, tables, actionness, scores, detections):
        self.videos, self.spans, self.frames, self.p_off = videos, spans, frames, p_off
        self.table, self.tables, self.actionness, self.scores, self.detections = table, tables, actionness, scores, detections

    def host_scores(self):
        """The dictionary of a score pickle: ``{video id: (rel float64 [K, 2], act, comp, reg or None)}`` as numpy arrays."""
        return {vid: tuple(None if t is None else t.cpu().numpy() for t in parts) for vid, parts in self.scores.items()}

    def save_scores(self, path):
        """The score pickle ``tools/eval_detections.py`` reads (the format ``tools/test_ssn.py`` writes)."""
        with open(path, "wb") as f:
            pickle.dump(self.host_scores(), f, pickle.HIGHEST_PROTOCOL)

    def to_activitynet(self, class_names, version="VERSION 1.3"):
        """The detections as the ActivityNet result dictionary: per video its rows in their order (class ascending, descending
        score), ``segment`` in seconds = the relative (start, end) times the video's duration."""
        d = self.detections
        rows, cls, vid = d.rows.cpu().numpy(), d.cls.cpu().numpy(), d.vid.cpu().numpy()
        if len(class_names) < d.num_class:
            raise ValueError("to_activitynet: %d class names for %d classes" % (len(class_names), d.num_class))
        results = {v.id: [] for v in self.videos}
        for r, c, i in zip(rows, cls, vid):
            video = self.videos[int(i)]
            results[video.id].append({"label": class_names[int(c)], "score": float(r[2]),
                                      "segment": [float(r[0] * video.duration), float(r[1] * video.duration)]})
        return {"version": version, "results": results, "external_data": {}}
