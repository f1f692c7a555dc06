"""Detection evaluation: per-class average precision, the mAP table and proposal recall -- the last stage of the
reference's workflow (/root/reference/eval_detection_results.py:188-251, ops/detection_metrics.py:7-51, 79-83), after
``detection_post.DetectionPostProcessor``.

The reference ravels ``dataset_detections`` into one pandas frame per class and runs the ActivityNet toolkit's
``compute_average_precision_detection`` for every (class, tIoU) pair in a pool of 32 processes.  That function lives in
a git submodule that is EMPTY in the reference tree, so AP parity here is against a restatement of the public
algorithm (the numpy referee in tools/make_eval_golden.py), not against reference output; the threshold
ranges, the means, the table's number formats, the score merge and both recall functions are the reference's own.

``DetectionEvaluator.evaluate`` is ONE batched GPU pass through csrc/eval.hip for all classes, videos and thresholds:
a sizing pass with one host read, then sort / match / scan -- launches and host synchronisations do not depend on the
number of classes or videos.  Where the toolkit leaves the outcome open (numpy's default argsort is unstable) the
rule is: predictions of equal score in input order (lower flat index first), ground-truth rows of equal IoU lower
index first.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import kernels as K

MAX_THRESHOLDS = 32


def tiou_thresholds(dataset):
    """The tIoU ranges of eval_detection_results.py:209-212, by the same expressions (bit-equal float64 values)."""
    if dataset == "activitynet1.2":
        return np.arange(0.5, 1.0, 0.05)
    if dataset == "thumos14":
        return np.arange(0.1, 1.0, 0.1)
    raise ValueError("unknown dataset {}".format(dataset))


def _default_device():
    return torch.device("cpu") if _lib.emulator_active() else torch.device("cuda")


def _put(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


FlatAP = namedtuple("FlatAP", "ap tp order pred_off")
FlatAP.__doc__ = """ap float64 [C, T] (NaN: class without ground truth); with return_matches tp uint8 [T, N] and order
int64 [N]: the flat indices class by class in descending score (class c at pred_off[c]:pred_off[c + 1]), tp in that order."""


@torch.no_grad()
def average_precision_flat(pred_seg, pred_score, pred_cls, pred_vid, gt_seg, gt_cls, gt_vid, num_class, thresholds,
                           device=None, return_matches=False):
    """AP of every (class, threshold) from flat rows.  Predictions: pred_seg [N, 2] and pred_score [N] float64, pred_cls /
    pred_vid [N] int32, numpy or tensors (tensors on the device stay there).  Ground truth (host): gt_seg [G, 2], gt_cls,
    gt_vid [G]; videos are numbered by the caller.  -> FlatAP."""
    dev = torch.device(device) if device is not None else _default_device()
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size < 1 or thr.size > MAX_THRESHOLDS:
        raise ValueError("between 1 and %d tIoU thresholds in one call, got %d" % (MAX_THRESHOLDS, thr.size))
    c = int(num_class)
    gt_seg = np.asarray(gt_seg, dtype=np.float64).reshape(-1, 2)
    gt_cls = np.asarray(gt_cls, dtype=np.int64).reshape(-1)
    gt_vid = np.asarray(gt_vid, dtype=np.int64).reshape(-1)
    if not (len(gt_seg) == len(gt_cls) == len(gt_vid)):
        raise ValueError("ground truth: one class and one video per span")
    if not np.isfinite(gt_seg).all() or not (gt_seg[:, 1] > gt_seg[:, 0]).all():
        raise ValueError("ground-truth spans must be finite and of positive length")
    if len(gt_cls) and (gt_cls.min() < 0 or gt_cls.max() >= c):
        raise ValueError("ground-truth class outside [0, %d)" % c)

    def dev_tensor(x, dtype, shape):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        t = t.to(dev, dtype).reshape(shape).contiguous()
        return t
    seg = dev_tensor(pred_seg, torch.float64, (-1, 2))
    score = dev_tensor(pred_score, torch.float64, (-1,))
    cls = dev_tensor(pred_cls, torch.int32, (-1,))
    vid = dev_tensor(pred_vid, torch.int32, (-1,))
    n = score.shape[0]
    if seg.shape[0] != n or cls.shape[0] != n or vid.shape[0] != n:
        raise ValueError("predictions: one span, class and video per score")

    # ground-truth tables (host): rows grouped by (class, video), input order inside a group
    g_order = np.lexsort((gt_vid, gt_cls))                    # stable
    gc, gv = gt_cls[g_order], gt_vid[g_order]
    head = np.ones(len(gc), dtype=bool)
    head[1:] = (gc[1:] != gc[:-1]) | (gv[1:] != gv[:-1])
    first = np.flatnonzero(head)
    rows = np.diff(np.append(first, len(gc)))
    lds = K.eval_lds_gt()
    units = np.where(rows > lds, rows + 32 * ((rows + 63) // 64), 0)
    big_off = np.concatenate([[0], np.cumsum(units)])
    if big_off[-1] >= 2 ** 31:
        raise ValueError("ground-truth groups too large for one call")
    groups = np.stack([gc[first], gv[first], first, rows, big_off[:-1]], axis=1).astype(np.int32).reshape(-1, 5)
    npos = np.bincount(gt_cls, minlength=c).astype(np.int32)

    # sizing pass and its one host read
    counts = K.eval_count(score, cls, c).cpu().numpy().astype(np.int64)
    if counts[c]:
        raise ValueError("%d predictions with a class outside [0, %d) or a score that is not finite" % (counts[c], c))
    per_class = counts[:c]
    pred_off = np.concatenate([[0], np.cumsum(per_class)])
    pow2 = np.left_shift(np.int64(1), np.frexp(np.maximum(per_class - 1, 0).astype(np.float64))[1].astype(np.int64))
    sort_off = np.concatenate([[0], np.cumsum(np.where(per_class > 0, pow2, 0))])
    if sort_off[-1] >= 2 ** 31:
        raise ValueError("%d predictions in one evaluation, split it" % n)
    order, tp, ap = K.eval_ap(seg, score, cls, vid, _put(gt_seg[g_order], dev), _put(groups, dev), _put(npos, dev),
                              _put(thr, dev), _put(pred_off.astype(np.int32), dev), _put(sort_off.astype(np.int64), dev),
                              int(sort_off[-1]), int(big_off[-1]))
    ap = ap.cpu().numpy()
    if return_matches:
        return FlatAP(ap, tp.cpu().numpy(), order.cpu().numpy().astype(np.int64), pred_off)
    return FlatAP(ap, None, None, pred_off)


DetectionEvalResult = namedtuple("DetectionEvalResult", "ap map_per_iou average_map classes_without_gt thresholds tp order "
                                                        "pred_off rows")
DetectionEvalResult.__doc__ = """ap [C, T]; map_per_iou [T] = ap.mean(axis=0) and average_map = map_per_iou.mean(), the plain
means of eval_detection_results.py:237,247 (a class without ground truth has AP NaN, as the toolkit's 0 / 0, is listed in
classes_without_gt, and the means carry the NaN).  With return_matches: tp [T, N], order [N], pred_off [C + 1] as in
FlatAP, and rows = (video ids [N], class [N], span [N, 2], score [N]) of the evaluator's flat rows that order indexes."""


class DetectionEvaluator(object):
    def __init__(self, num_class, tiou_thresholds, device=None):
        self.num_class = int(num_class)
        self.thresholds = np.ascontiguousarray(np.asarray(tiou_thresholds, dtype=np.float64).reshape(-1))
        if self.thresholds.size < 1 or self.thresholds.size > MAX_THRESHOLDS:
            raise ValueError("between 1 and %d tIoU thresholds, got %d" % (MAX_THRESHOLDS, self.thresholds.size))
        self.device = device
        self._videos = {}            # video id -> index, in the order of add_video
        self._host = []              # (video index, class, rows [n, 3])
        self._dev = []               # (video index, dets [C, n_max, 5], counts [C]) on the device
        self._batches = []           # (index of the batch's first video, detection_post.BatchedDetections)

    def add_video(self, video_id, detections):
        """detections: what ``DetectionPostProcessor.process_video`` returns first, ``{class: rows [n, >= 3]}`` (start, end,
        score; further columns ignored, as ravel_detections' ``x[:3]``), or the pair ``(dets [C, n_max, 5], counts [C])``
        of ``process_video_device``, which stays on the device.  Flat row order (the tie rule's "input order"): the rows
        given on the host, then the per-video device entries, then the batches of ``add_batch``, each in the order added."""
        if video_id in self._videos:
            raise ValueError("video %r was added before" % (video_id,))
        index = len(self._videos)
        if isinstance(detections, dict):
            items = []
            for cls in sorted(detections):
                rows = np.asarray(detections[cls], dtype=np.float64)
                if not 0 <= int(cls) < self.num_class:
                    raise ValueError("class %r outside [0, %d)" % (cls, self.num_class))
                if rows.ndim != 2 or rows.shape[1] < 3:
                    raise ValueError("detections of class %r must be rows of (start, end, score, ...)" % (cls,))
                if not np.isfinite(rows[:, 2]).all():
                    raise ValueError("video %r: scores must be finite" % (video_id,))
                items.append((index, int(cls), rows[:, :3]))
            self._host.extend(items)
        else:
            dets, counts = detections
            if not (torch.is_tensor(dets) and torch.is_tensor(counts)) or dets.dim() != 3 \
                    or not 1 <= dets.shape[0] <= self.num_class or dets.shape[2] < 3 or counts.shape != (dets.shape[0],):
                raise ValueError("device detections must be (dets [C, n_max, >= 3], counts [C]) tensors, C <= num_class")
            self._dev.append((index, dets, counts))
        self._videos[video_id] = index

    def add_batch(self, batched):
        """batched: what ``DetectionPostProcessor.process_videos`` returns.  Its flat rows are appended as they are (no
        padding, nothing to compact); its videos count as added in the batch's order."""
        if batched.num_class > self.num_class:
            raise ValueError("a batch of %d classes for an evaluator of %d" % (batched.num_class, self.num_class))
        seen = set()
        for video_id in batched.video_ids:
            if video_id in self._videos or video_id in seen:
                raise ValueError("video %r was added before" % (video_id,))
            seen.add(video_id)
        base = len(self._videos)
        for video_id in batched.video_ids:
            self._videos[video_id] = len(self._videos)
        self._batches.append((base, batched))

    def _flat_rows(self, dev):
        """-> seg [N, 2], score [N] float64, cls, vid [N] int32 on `dev`.  A constant number of transfers and torch calls."""
        parts = []
        if self._host:
            rows = np.concatenate([r for _, _, r in self._host])
            lens = [len(r) for _, _, r in self._host]
            cls = np.repeat(np.asarray([c for _, c, _ in self._host], dtype=np.int32), lens)
            vid = np.repeat(np.asarray([v for v, _, _ in self._host], dtype=np.int32), lens)
            parts.append((_put(rows[:, :2], dev), _put(rows[:, 2], dev), _put(cls, dev), _put(vid, dev)))
        if self._dev:
            padded = torch.cat([d.to(dev, torch.float64).reshape(-1, d.shape[2])[:, :3] for _, d, _ in self._dev])
            counts = torch.cat([k.to(dev).reshape(-1) for _, _, k in self._dev]).to(torch.int64)
            # per padded row (host arithmetic on the shapes alone): its class, its video, its place among the n_max slots of
            # its class, and where its class's count stands in `counts`
            cls, vid, pos, cnt_at, base = [], [], [], [], 0
            for v, d, _ in self._dev:
                c, n_max = d.shape[0], d.shape[1]
                cls.append(np.repeat(np.arange(c, dtype=np.int32), n_max))
                vid.append(np.full(c * n_max, v, dtype=np.int32))
                pos.append(np.tile(np.arange(n_max, dtype=np.int64), c))
                cnt_at.append(base + np.repeat(np.arange(c, dtype=np.int64), n_max))
                base += c
            valid = _put(np.concatenate(pos), dev) < counts[_put(np.concatenate(cnt_at), dev)]
            keep = valid.nonzero().reshape(-1)                              # (the sizing read of the device form)
            padded = padded.index_select(0, keep)
            parts.append((padded[:, :2].contiguous(), padded[:, 2].contiguous(),
                          _put(np.concatenate(cls), dev).index_select(0, keep),
                          _put(np.concatenate(vid), dev).index_select(0, keep)))
        for base, b in self._batches:
            rows = b.rows.to(dev)
            parts.append((rows[:, :2].contiguous(), rows[:, 2].contiguous(), b.cls.to(dev), b.vid.to(dev) + base))
        if not parts:
            return (torch.zeros((0, 2), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev),
                    torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev))
        if len(parts) == 1:
            return parts[0]
        return tuple(torch.cat([p[i] for p in parts]) for i in range(4))

    @torch.no_grad()
    def evaluate(self, all_gt, return_matches=False):
        """all_gt: the rows ``[video id, class, start, end]`` of ``ProposalSampler.all_gt()`` (the reference's
        ``get_all_gt``).  -> DetectionEvalResult."""
        dev = torch.device(self.device) if self.device is not None else _default_device()
        videos = dict(self._videos)
        gt_vid = np.asarray([videos.setdefault(g[0], len(videos)) for g in all_gt], dtype=np.int64)
        gt_cls = np.asarray([g[1] for g in all_gt], dtype=np.int64)
        gt_seg = np.asarray([[g[2], g[3]] for g in all_gt], dtype=np.float64).reshape(-1, 2)
        seg, score, cls, vid = self._flat_rows(dev)
        flat = average_precision_flat(seg, score, cls, vid, gt_seg, gt_cls, gt_vid, self.num_class, self.thresholds, dev,
                                      return_matches)
        ap = flat.ap
        map_per_iou = ap.mean(axis=0)
        without = [c for c in range(self.num_class) if not (gt_cls == c).any()]
        rows = None
        if return_matches:
            names = list(videos)
            rows = ([names[v] for v in vid.cpu().numpy()], cls.cpu().numpy(), seg.cpu().numpy(), score.cpu().numpy())
        return DetectionEvalResult(ap, map_per_iou, map_per_iou.mean(), without, self.thresholds, flat.tp, flat.order,
                                   flat.pred_off, rows)


def map_table_rows(thresholds, map_per_iou):
    """The two rows of the reference's table (eval_detection_results.py:240-247), cell texts in its number formats."""
    rows = [["IoU thresh"], ["mean AP"]]
    for t, m in zip(thresholds, map_per_iou):
        rows[0].append("{:.02f}".format(t))
        rows[1].append("{:.04f}".format(m))
    rows[0].append("Average")
    rows[1].append("{:.04f}".format(np.asarray(map_per_iou).mean()))
    return rows


def format_map_table(thresholds, map_per_iou, title):
    """The table of :248-251 as text: the cells of ``map_table_rows`` in a plain ASCII frame, last column right-aligned.
    (The reference draws the frame with terminaltables; the cell texts are the same, the frame is this module's.)"""
    rows = map_table_rows(thresholds, map_per_iou)
    width = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    last = len(width) - 1

    def line(r):
        cells = [(x.rjust(w) if i == last else x.ljust(w)) for i, (x, w) in enumerate(zip(r, width))]
        return "| " + " | ".join(cells) + " |"
    rule = "+" + "+".join("-" * (w + 2) for w in width) + "+"
    head = "+" + title.center(len(rule) - 2, "-") + "+"
    return "\n".join([head, line(rows[0]), rule, line(rows[1]), rule])


RecallResult = namedtuple("RecallResult", "per_video_recall per_inst_recall hits totals")
RecallResult.__doc__ = """per_video_recall / per_inst_recall float64 [T] (get_temporal_proposal_recall, detection_metrics.py
:79-83, per threshold), hits int64 [V, T] and totals int64 [V]: temporal_recall's (hit, total) of every video."""


@torch.no_grad()
def proposal_recall(pr_list, gt_list, thresholds, device=None):
    """``get_temporal_proposal_recall`` for all thresholds in one launch.  pr_list / gt_list: per video the proposal and
    the ground-truth spans ``[(start, end), ...]``.  A ground-truth span is hit when some proposal's temporal_iou with it
    is strictly above the threshold; a video counts as recalled when all of its spans are (a video without ground
    truth does, as in the reference)."""
    if len(pr_list) != len(gt_list) or len(gt_list) < 1:
        raise ValueError("proposal_recall: one proposal list per ground-truth list, at least one video")
    dev = torch.device(device) if device is not None else _default_device()
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size < 1:
        raise ValueError("proposal_recall: at least one threshold")
    props = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in pr_list]
    spans = [np.asarray(g, dtype=np.float64).reshape(-1, 2) for g in gt_list]
    totals = np.asarray([len(s) for s in spans], dtype=np.int64)
    if totals.sum() == 0:
        raise ValueError("proposal_recall: no ground-truth span in any video (the reference divides by zero here)")
    p_off = np.concatenate([[0], np.cumsum([len(p) for p in props])]).astype(np.int32)
    g_off = np.concatenate([[0], np.cumsum(totals)]).astype(np.int32)
    hits = K.eval_recall(_put(np.concatenate(spans), dev), _put(g_off, dev), _put(np.concatenate(props), dev), _put(p_off, dev),
                         _put(thr, dev)).cpu().numpy().astype(np.int64)
    per_video = np.asarray([np.sum(hits[:, t] == totals) / float(len(totals)) for t in range(thr.size)])
    per_inst = np.asarray([np.sum(hits[:, t]) / float(np.sum(totals)) for t in range(thr.size)])
    return RecallResult(per_video, per_inst, hits, totals)


def merge_detection_scores(score_dicts, weights=None):
    """The weighted merge of several score pickles (eval_detection_results.py:50-75): per video of the FIRST source
    ``(rel_props of the first source, activity, completeness, regression)``, each part the sum over the sources of
    part * weight; weights are normalised by their sum (default: equal); a part that is None in the first source stays
    None.  Host arithmetic, numpy's own ``np.sum`` over the list as in the reference."""
    if weights:
        weights = np.array(weights) / sum(weights)
    else:
        weights = [1.0 / len(score_dicts) for _ in score_dicts]

    def merge_part(arrs, index):
        if arrs[0][index] is not None:
            return np.sum([a[index] * w for a, w in zip(arrs, weights)], axis=0)
        return None

    out = {}
    for vid in score_dicts[0]:
        arrays = [d[vid] for d in score_dicts]
        out[vid] = (score_dicts[0][vid][0], merge_part(arrays, 1), merge_part(arrays, 2), merge_part(arrays, 3))
    return out
