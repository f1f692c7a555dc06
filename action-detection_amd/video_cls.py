"""Video-level classification: dense per-tick scores -> one score vector per video, stream fusion, and the metrics.

The counterpart of the reference's ``ops/video_funcs.py`` (``default_aggregation_func``, ``top_k_aggregation_func``,
``sliding_window_aggregation_func`` -- the ActivityNet 2016 rule --, ``tpp_aggregation_func``, ``default_fusion_func``)
and ``ops/metrics.py`` (``top_k_accuracy``, ``video_mean_ap``, ``mean_class_accuracy``), as ONE batched pass over all
videos in the kernels of ``csrc/video_cls.hip``.  The input is what ``ActionnessTester`` leaves on the device
(``ActionnessScores``); the output is the ``{video: scores[C]}`` file ``tools/eval_detections.py --cls_scores`` reads
and the ``video_cls_score=`` argument of ``DetectionPostProcessor``.  Nothing is read back unless the caller asks
(``check`` / ``to_host`` / ``save``); the number of launches does not depend on the number of videos.

Rules this module fixes where the reference leaves them open:

* ``sliding_window`` takes the mean of the ``max(15, n // 4)`` largest of a span's ``n`` windows.  The reference writes
  ``len(local_agg) / 4``, Python 2's integer division; under Python 3 its function fails as soon as a span has more
  than 60 windows.
* top-k ranking is STABLE: of equal scores the higher class index ranks higher (numpy's default ``argsort`` leaves the
  order of ties open).
* the AP of a class without a positive video is NaN (sklearn versions differ there: 0, NaN or a warning), and so is
  then the macro mean.
* a video with a non-finite input score (status bit 1) or without ticks (status bit 2) gets a NaN row.
"""
import math
import pickle
from collections import OrderedDict

import numpy as np
import torch

from . import kernels as K

MODES = ("default", "top_k", "sliding_window", "tpp")


class VideoClassScores(object):
    """``scores`` float32 [V, C] and ``status`` int32 [V] on the device, ``ids`` the V video ids in row order, ``spans``
    float32 [V, S, C] (the per-span values of ``sliding_window`` before their mean) when it was asked for."""

    def __init__(self, ids, scores, status=None, spans=None):
        self.ids = list(ids)
        self.scores = scores
        self.status = status
        self.spans = spans
        if scores.dim() != 2 or scores.shape[0] != len(self.ids):
            raise ValueError("scores must be [%d, C], got %s" % (len(self.ids), tuple(scores.shape)))

    def __len__(self):
        return len(self.ids)

    def check(self):
        """The one optional host read: raises, naming the videos, if any was flagged."""
        if self.status is None:
            return self
        st = self.status.cpu().numpy()
        bad = [(self.ids[i], int(s)) for i, s in enumerate(st) if s]
        if bad:
            raise ValueError("video-level scores: %d flagged video(s) (1: non-finite input, 2: no ticks): %s"
                             % (len(bad), ", ".join("%s=%d" % b for b in bad[:20])))
        return self

    def to_host(self):
        """-> {video id: float32 numpy [C]}"""
        s = self.scores.cpu().numpy()
        return OrderedDict((vid, s[i].copy()) for i, vid in enumerate(self.ids))

    def save(self, path):
        """The classifier score file of ``eval_detection_results.py --cls_scores``: {str id: float32 [C]}, pickle protocol 2."""
        with open(path, "wb") as f:
            pickle.dump({str(k): v for k, v in self.to_host().items()}, f, 2)

    @classmethod
    def load(cls, path, device=None):
        with open(path, "rb") as f:
            raw = pickle.load(f, encoding="bytes")
        ids = [k.decode("utf-8") if isinstance(k, bytes) else k for k in raw]
        return _as_scores({i: raw[k] for i, k in zip(ids, raw)}, device)


def _default_device():
    from .detection_eval import _default_device as d
    return d()


def _as_scores(x, device=None):
    """VideoClassScores, or a mapping id -> [C] array / tensor, as VideoClassScores on the device."""
    if isinstance(x, VideoClassScores):
        return x
    if not hasattr(x, "items") or len(x) == 0:
        raise ValueError("scores must be VideoClassScores or a non-empty mapping of video id -> [C] scores")
    ids, rows = [], []
    for k, v in x.items():
        t = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))
        if t.dim() != 1 or t.dtype != torch.float32:
            raise ValueError("scores of video %r must be float32 [C], got %s %s" % (k, t.dtype, tuple(t.shape)))
        ids.append(k)
        rows.append(t)
    if device is None:
        device = rows[0].device if rows[0].is_cuda else _default_device()
    if len(set(r.shape[0] for r in rows)) != 1:
        raise ValueError("the videos' score vectors differ in length")
    return VideoClassScores(ids, torch.stack([r.to(device) for r in rows]).contiguous())


def window_plan(spans, overlap, fps):
    """(span, step) in ticks per temporal span, in Python floats exactly as the reference computes them
    (``span = t_span * fps``, ``step = int(ceil(span * (1 - overlap)))``): 0.8 -> 1, 1.6 -> 2, 3.2 -> 4, 6.4 -> 7, 12.8 -> 13."""
    out = []
    for t_span in spans:
        span = t_span * fps
        if int(span) != span or span < 1:
            raise ValueError("span %r x fps %r is not a positive whole number of ticks" % (t_span, fps))
        step = int(math.ceil(span * (1 - overlap)))
        if step < 1:
            raise ValueError("overlap %r leaves no step for span %r" % (overlap, t_span))
        out.append((int(span), step))
    return out


class VideoScoreAggregator(object):
    """``mode``: ``"default"`` (mean over ticks), ``"top_k"`` (mean of the ``k`` largest ticks per class),
    ``"sliding_window"`` (per span: window maxima, mean of the ``max(15, n // 4)`` largest; then the mean over spans) or
    ``"tpp"`` (stage-wise mean of ``stages * num_class`` columns; no softmax, as in the reference).  ``normalization``:
    softmax over the classes at the end.  ``crop_agg``: how ``[T, crops, C]`` input becomes ``[T, C]``."""

    def __init__(self, mode="default", k=None, spans=(1, 2, 4, 8, 16), overlap=0.2, fps=1, normalization=True, crop_agg="mean",
                 num_class=None):
        if mode not in MODES:
            raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
        if crop_agg not in ("mean", "max"):
            raise ValueError("crop_agg must be 'mean' or 'max', got %r" % (crop_agg,))
        if mode == "top_k" and (k is None or int(k) != k or int(k) < 1):
            raise ValueError("top_k needs an integer k >= 1, got %r" % (k,))
        if mode == "tpp" and (num_class is None or int(num_class) < 1):
            raise ValueError("tpp needs num_class >= 1")
        self.mode = mode
        self.k = None if k is None else int(k)
        self.normalization = bool(normalization)
        self.crop_agg = crop_agg
        self.num_class = None if num_class is None else int(num_class)
        self.plan = window_plan(spans, overlap, fps) if mode == "sliding_window" else []
        if mode == "sliding_window" and not self.plan:
            raise ValueError("sliding_window needs at least one span")

    @staticmethod
    def _items(scores):
        if hasattr(scores, "raw") and hasattr(scores, "mean"):      # ActionnessScores
            scores = scores.raw if len(scores.raw) else scores.mean
        if hasattr(scores, "items"):
            return list(scores.keys()), list(scores.values())
        scores = list(scores)
        return list(range(len(scores))), scores

    def aggregate(self, scores, return_spans=False):
        """``scores``: ``ActionnessScores``, or a dict / list of float32 device tensors ``[T, crops, C]`` or ``[T, C]``
        (one rank, crop count and C for all) -> ``VideoClassScores``."""
        ids, tens = self._items(scores)
        if not tens:
            raise ValueError("no videos to aggregate")
        first = tens[0]
        for t in tens:
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() not in (2, 3):
                raise ValueError("every video's scores must be a float32 tensor [T, crops, C] or [T, C]")
            if t.dim() != first.dim() or t.shape[1:] != first.shape[1:] or t.device != first.device:
                raise ValueError("the videos' score tensors differ in rank, crops, C or device")
        if min(first.shape[1:]) < 1:
            raise ValueError("scores need crops >= 1 and C >= 1, got %s" % (tuple(first.shape),))
        width = first.shape[-1]
        if self.mode == "tpp" and width % self.num_class:
            raise ValueError("tpp: %d columns are not a multiple of num_class = %d" % (width, self.num_class))
        if return_spans and self.mode != "sliding_window":
            raise ValueError("return_spans belongs to the sliding_window mode")
        ts = [int(t.shape[0]) for t in tens]
        v = len(ts)
        h_off = torch.zeros(v + 1, dtype=torch.int32)
        h_off[1:] = torch.tensor(ts, dtype=torch.int64).cumsum(0).to(torch.int32)
        rows = (tens[0] if v == 1 else torch.cat(tens, 0)).contiguous()
        status = K.vcls_status(rows, h_off)
        frm = K.vcls_crop_reduce(rows, use_max=self.crop_agg == "max") if rows.dim() == 3 else rows
        spans_out = None
        if self.mode == "tpp":
            terms = K.vcls_tpp(frm, h_off, self.num_class).view(v, 1, self.num_class)
            out = K.vcls_finish(terms, 0, status=status)
        elif self.mode == "sliding_window":
            s = len(self.plan)
            counts = [(-(-t // step)) for t in ts for _, step in self.plan]
            h_win = torch.zeros(v * s + 1, dtype=torch.int32)
            h_win[1:] = torch.tensor(counts, dtype=torch.int64).cumsum(0).to(torch.int32)
            dev = frm.device
            d_spans = torch.tensor([p[0] for p in self.plan], dtype=torch.int32).to(dev)
            d_steps = torch.tensor([p[1] for p in self.plan], dtype=torch.int32).to(dev)
            win = K.vcls_window_max(frm, h_off, h_win, d_spans, d_steps)
            h_ks = torch.tensor([max(15, n // 4) for n in counts], dtype=torch.int32)
            spans_out = K.vcls_topk_mean(win, h_win, h_ks).view(v, s, width)
            out = K.vcls_finish(spans_out, 0, status=status, divide=True, softmax=self.normalization)
        else:
            h_ks = torch.tensor([max(t, 1) if self.mode == "default" else self.k for t in ts], dtype=torch.int32)
            terms = K.vcls_topk_mean(frm, h_off, h_ks).view(v, 1, width)
            out = K.vcls_finish(terms, 0, status=status, softmax=self.normalization)
        return VideoClassScores(ids, out, status, spans_out if return_spans else None)


def fuse_scores(major, others, weights, norm=True):
    """``default_fusion_func`` for all videos: ``major + sum_i weights[i] * others[i]``, added in the given order, then the
    softmax when ``norm``.  Streams are ``VideoClassScores`` or mappings id -> [C]; videos are matched by id (the rows
    follow ``major``), a video missing from a stream raises ``KeyError``."""
    others, weights = list(others), [float(w) for w in weights]
    if len(others) != len(weights):
        raise ValueError("fuse_scores: %d streams for %d weights" % (len(others), len(weights)))
    major = _as_scores(major)
    dev = major.scores.device
    planes, status = [major.scores], major.status
    for i, o in enumerate(others):
        o = _as_scores(o, dev)
        if o.scores.shape[1] != major.scores.shape[1]:
            raise ValueError("fuse_scores: stream %d has %d classes, the major stream %d" % (
                i + 1, o.scores.shape[1], major.scores.shape[1]))
        if o.ids != major.ids:
            where = {vid: j for j, vid in enumerate(o.ids)}
            missing = [vid for vid in major.ids if vid not in where]
            if missing:
                raise KeyError("fuse_scores: stream %d has no scores for %r" % (i + 1, missing[0]))
            idx = torch.tensor([where[vid] for vid in major.ids], dtype=torch.int64).to(dev)
            o = VideoClassScores(major.ids, o.scores.index_select(0, idx),
                                 None if o.status is None else o.status.index_select(0, idx))
        planes.append(o.scores)
        if o.status is not None:
            status = o.status if status is None else status | o.status
    terms = torch.stack(planes).contiguous()
    w = torch.tensor(weights, dtype=torch.float32).to(dev) if weights else None
    out = K.vcls_finish(terms, 1, weights=w, status=status, softmax=bool(norm))
    return VideoClassScores(major.ids, out, status)


class ClassificationMetrics(object):
    """``top_k_accuracy`` {k: float}, ``mean_ap``, ``ap`` float64 numpy [C], ``mean_class_accuracy`` (None when it was
    not asked for), ``videos_scored``."""

    def __init__(self, top_k_accuracy, mean_ap, ap, mean_class_accuracy, videos_scored):
        self.top_k_accuracy = top_k_accuracy
        self.mean_ap = mean_ap
        self.ap = ap
        self.mean_class_accuracy = mean_class_accuracy
        self.videos_scored = videos_scored

    def __repr__(self):
        return "ClassificationMetrics(%s, mean_ap=%r, mean_class_accuracy=%r, videos_scored=%d)" % (
            ", ".join("top%d=%r" % kv for kv in sorted(self.top_k_accuracy.items())), self.mean_ap, self.mean_class_accuracy,
            self.videos_scored)


def classification_metrics(scores, labels, top_k=(1, 3), class_accuracy=True):
    """``scores``: ``VideoClassScores`` or a mapping id -> [C]; ``labels``: {id: iterable of class indices}.  Videos of
    ``labels`` without scores are left out, as the reference leaves them out.  One call computes on the device

    * the top-k hit rate (``top_k_accuracy``): a video hits when its label set meets its k highest-ranked classes, ranked
      by a STABLE ascending sort (of equal scores the higher class index ranks higher);
    * the video mAP (``video_mean_ap``): per class ``sum_n (R_n - R_{n-1}) P_n`` over the DISTINCT score values in
      descending order (tied scores form one threshold, as sklearn's ``average_precision_score`` groups them), fp64, and
      the macro mean.  A class without a positive video gives NaN (and so does the mean); sklearn versions differ there;
    * the mean class accuracy (``mean_class_accuracy``): first argmax per video, hits / videos per class, mean over the
      classes that occur among labels OR predictions -- a class that is only predicted contributes 0 / 0 = NaN, as the
      reference's confusion-matrix arithmetic does.  It needs ONE label per video and raises ``ValueError`` otherwise;
      ``class_accuracy=False`` leaves it out (None)."""
    sc = _as_scores(scores)
    c = sc.scores.shape[1]
    ks = [int(k) for k in top_k]
    if any(k < 1 for k in ks):
        raise ValueError("classification_metrics: every top_k must be >= 1")
    where = {vid: i for i, vid in enumerate(sc.ids)}
    rows, sets = [], []
    for vid, lb in labels.items():
        if vid not in where:
            continue
        lb = sorted(set(int(x) for x in lb))
        if not lb or lb[0] < 0 or lb[-1] >= c:
            raise ValueError("classification_metrics: labels of video %r must lie in [0, %d), got %r" % (vid, c, lb))
        if class_accuracy and len(lb) != 1:
            raise ValueError("classification_metrics: mean class accuracy needs one label per video, %r has %r" % (vid, lb))
        rows.append(where[vid])
        sets.append(lb)
    if not rows:
        raise ValueError("classification_metrics: no labelled video has scores")
    dev = sc.scores.device
    gt = np.zeros((len(rows), c), dtype=np.uint8)
    for i, lb in enumerate(sets):
        gt[i, lb] = 1
    picked = sc.scores if rows == list(range(len(sc.ids))) else \
        sc.scores.index_select(0, torch.tensor(rows, dtype=torch.int64).to(dev))
    label = torch.tensor([lb[0] for lb in sets], dtype=torch.int32).to(dev) if class_accuracy else None
    _, ap, res = K.vcls_metrics(picked.contiguous(), torch.from_numpy(gt).to(dev), label,
                                torch.tensor(ks, dtype=torch.int32).to(dev))
    res = res.cpu().numpy()
    return ClassificationMetrics({k: float(res[i]) for i, k in enumerate(ks)}, float(res[len(ks)]), ap.cpu().numpy(),
                                 float(res[len(ks) + 1]) if class_accuracy else None, len(rows))
