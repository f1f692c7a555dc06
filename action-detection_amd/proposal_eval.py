"""Proposal evaluation: average recall against the average number of proposals per video (AR-AN), its area under the
curve and recall against tIoU -- the measure the TAG / SSN papers and the ActivityNet proposal task report, and the one
that can compare two proposal generators: unlike ``detection_eval.proposal_recall`` it does not rise just because more
proposals are emitted.

The algorithm is the ActivityNet toolkit's public ``average_recall_vs_avg_nr_proposals``.  The toolkit is a git submodule
that is EMPTY in the reference tree, so parity here is against a restatement (tests/proposal_eval_referee.py),
not against toolkit output.  Where the toolkit leaves the outcome open (its ``argsort()[::-1]`` is unstable) the rule is
``DetectionEvaluator``'s: proposals of equal score rank in input order.

``proposal_ar_an`` is ONE batched GPU pass through csrc/proposal_eval.hip for all videos, thresholds and curve points:
one packed upload, a memset and two launches (four with ``scores``), one download, whatever the number of videos.  The host derives
the per-video truncation ``nr`` and the curve fractions ``pcn`` from the per-video COUNTS alone, with vectorised numpy;
nothing is read back from the device in between.  ``proposal_ar_an_batch`` reads the proposals where
``ProposalListBuilder`` left them on the device.  Spans are in any one unit.
"""
import numpy as np
import torch

from . import kernels as K
from .proposal_lists import _pack
from .tag_proposals import _default_device

MAX_THRESHOLDS = 32
MAX_POINTS = 4096          # curve points of one call (ssn_proposal_eval_max_points)


def default_thresholds():
    """The toolkit's tIoU thresholds, by its own expression."""
    return np.linspace(0.5, 0.95, 10)


class ArAnResult(object):
    """What ``proposal_ar_an`` returns.  ``recall`` float64 [T, J], ``avg_recall`` and ``proposals_per_video`` [J], ``auc``
    (area under avg_recall over proposals_per_video, divided by the last entry: a fraction), ``matches`` int64 [T, J]
    (ground-truth spans covered at threshold t by the proposals shown at point j), ``positives`` (ground-truth spans),
    ``total_proposals`` (proposals of the counted videos after the truncation), ``num_videos`` (videos with ground truth),
    ``thresholds`` [T], ``first_hit`` int [G, T]: per ground-truth span, in the order given, the best rank (from 0) of a
    proposal of its video whose tIoU reaches the threshold, -1 for never."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def ar_at(self, n):
        """avg_recall at `n` proposals per video, linearly interpolated between the curve points (clamped outside)."""
        return np.interp(n, self.proposals_per_video, self.avg_recall)

    def recall_vs_tiou(self, n):
        """The recall of every threshold at `n` proposals per video, interpolated in the same way -> [T]."""
        return np.asarray([np.interp(n, self.proposals_per_video, r) for r in self.recall])


def _thresholds(thresholds):
    thr = default_thresholds() if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    thr = np.ascontiguousarray(thr)
    if thr.size < 1 or thr.size > MAX_THRESHOLDS:
        raise ValueError("between 1 and %d tIoU thresholds in one call, got %d" % (MAX_THRESHOLDS, thr.size))
    if not np.isfinite(thr).all():
        raise ValueError("tIoU thresholds must be finite")
    return thr


def _plan(m, n, max_avg_nr_proposals, points):
    """The host part, from the per-video counts m (proposals) and n (ground-truth spans) alone: nr [V'] int32 (0 for a
    video without ground truth), pcn [J], total_nr, counted videos.  The expressions and their order are the toolkit's."""
    points = int(points)
    if points < 1 or points > MAX_POINTS:
        raise ValueError("between 1 and %d curve points in one call, got %d" % (MAX_POINTS, points))
    counted = n >= 1
    v = int(counted.sum())
    if v == 0:
        raise ValueError("no ground-truth span in any video")
    p_total = int(m.sum())
    if p_total == 0:
        raise ValueError("no proposal in any video")
    if max_avg_nr_proposals is None or max_avg_nr_proposals == 0:
        max_avg_nr_proposals = float(p_total) / v
    max_avg_nr_proposals = float(max_avg_nr_proposals)
    if not np.isfinite(max_avg_nr_proposals) or max_avg_nr_proposals < 0:
        raise ValueError("max_avg_nr_proposals must be a finite number above 0, or None")
    ratio = max_avg_nr_proposals * float(v) / p_total
    nr = np.where(counted, np.minimum(np.trunc(m.astype(np.float64) * ratio), m.astype(np.float64)), 0.0).astype(np.int64)
    total_nr = int(nr.sum())
    if total_nr == 0:
        raise ValueError("no proposal is left in a video with ground truth (max_avg_nr_proposals %r)" % max_avg_nr_proposals)
    pcn = np.arange(1, points + 1) / float(points) * (max_avg_nr_proposals * float(v) / total_nr)
    return nr.astype(np.int32), np.ascontiguousarray(pcn), total_nr, v


def _rank_tables(m):
    """sort_off [V' + 1] int64 of ssn_proposal_eval_rank: every video's count rounded up to a power of two (0 stays 0)."""
    pow2 = np.left_shift(np.int64(1), np.frexp(np.maximum(m - 1, 0).astype(np.float64))[1].astype(np.int64))
    sort_off = np.concatenate([[0], np.cumsum(np.where(m > 0, pow2, 0))]).astype(np.int64)
    if sort_off[-1] >= 2 ** 31:
        raise ValueError("%d proposals in one evaluation, split it" % int(m.sum()))
    return sort_off


def _gt_arrays(gt_list):
    spans = [np.asarray(g, dtype=np.float64).reshape(-1, 2) for g in gt_list]
    n = np.asarray([len(s) for s in spans], dtype=np.int64)
    flat = np.concatenate(spans) if spans else np.zeros((0, 2))
    if not np.isfinite(flat).all():
        raise ValueError("a ground-truth span is not finite")
    return np.ascontiguousarray(flat), n


def _run(dev, plan, d_prop, d_poff, gt_span, n, thr, head):
    """The launches and the one download.  `head`: host arrays that go up in front of the ground truth in the packed
    buffer -- nothing (the proposals are on the device: d_prop, d_poff), or (prop, p_off[, score, sort_off])."""
    nr, pcn, total_nr, v = plan
    g_off = np.concatenate([[0], np.cumsum(n)])
    if g_off[-1] * thr.size >= 2 ** 31:
        raise ValueError("%d ground-truth spans in one evaluation, split it" % g_off[-1])
    buf, rng = _pack(head + [gt_span, g_off.astype(np.int32), nr, thr, pcn])
    d = torch.from_numpy(buf).to(dev)                                                    # the one upload
    part = [d[b:e] for b, e in rng]
    k = len(head)
    d_span, d_goff = part[k].view(torch.float64).reshape(-1, 2), part[k + 1].view(torch.int32)
    d_nr, d_thr, d_pcn = part[k + 2].view(torch.int32), part[k + 3].view(torch.float64), part[k + 4].view(torch.float64)
    order = None
    if k:
        d_prop, d_poff = part[0].view(torch.float64).reshape(-1, 2), part[1].view(torch.int32)
    if k == 4:
        order = K.proposal_eval_rank(part[2].view(torch.float64), d_poff, part[3].view(torch.int64), int(head[3][-1]))
    first_hit, matches, curves = K.proposal_eval_ar_an(d_span, d_goff, d_prop, d_poff, d_nr, d_thr, d_pcn,
                                                       float(total_nr) / v, order)
    outs = [curves, first_hit, matches]                                                  # (the float64 array first: alignment)
    sizes = [t.numel() * t.element_size() for t in outs]
    host = torch.cat([t.reshape(-1).view(torch.uint8) for t in outs]).cpu().numpy()      # the one download
    cut = np.concatenate([[0], np.cumsum(sizes)])
    curves = host[cut[0]:cut[1]].view(np.float64)
    t, j = thr.size, pcn.size
    return ArAnResult(recall=curves[:t * j].reshape(t, j), avg_recall=curves[t * j:t * j + j],
                      proposals_per_video=curves[t * j + j:t * j + 2 * j], auc=float(curves[t * j + 2 * j]),
                      matches=host[cut[2]:cut[3]].view(np.int32).reshape(t, j).astype(np.int64), positives=int(g_off[-1]),
                      total_proposals=total_nr, num_videos=v, thresholds=thr,
                      first_hit=host[cut[1]:cut[2]].view(np.int32).reshape(-1, t).astype(np.int64))


@torch.no_grad()
def proposal_ar_an(pr_list, gt_list, scores=None, max_avg_nr_proposals=None, thresholds=None, points=100, device=None):
    """AR-AN of a subset.  pr_list / gt_list: per video the proposal and the ground-truth spans ``[(start, end), ...]``,
    the proposals in rank order, best first -- or in any order with ``scores`` (one list of scores per video; the rank is
    then descending score, equal scores in input order).  Only videos with ground truth count; the proposals of ALL
    videos enter the default ``max_avg_nr_proposals`` (None or 0: proposals / counted videos), as in the toolkit.
    -> ArAnResult.  Raises ValueError when there is no ground truth, when no proposal is left, and for spans or scores
    that are not finite."""
    if len(pr_list) != len(gt_list) or len(gt_list) < 1:
        raise ValueError("proposal_ar_an: one proposal list per ground-truth list, at least one video")
    if scores is not None and len(scores) != len(pr_list):
        raise ValueError("proposal_ar_an: one score list per proposal list")
    thr = _thresholds(thresholds)
    props = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in pr_list]
    m = np.asarray([len(p) for p in props], dtype=np.int64)
    prop = np.ascontiguousarray(np.concatenate(props))
    if not np.isfinite(prop).all():
        raise ValueError("a proposal span is not finite")
    gt_span, n = _gt_arrays(gt_list)
    p_off = np.concatenate([[0], np.cumsum(m)])
    if p_off[-1] >= 2 ** 30:
        raise ValueError("%d proposals in one evaluation (2^30 or more), split it" % p_off[-1])
    head = [prop, p_off.astype(np.int32)]
    if scores is not None:
        sc = [np.asarray(s, dtype=np.float64).reshape(-1) for s in scores]
        if [len(s) for s in sc] != list(m):
            raise ValueError("proposal_ar_an: one score per proposal")
        score = np.ascontiguousarray(np.concatenate(sc))
        if not np.isfinite(score).all():
            raise ValueError("a proposal score is not finite")
        head += [score, _rank_tables(m)]
    plan = _plan(m, n, max_avg_nr_proposals, points)           # (every argument error before anything touches the device)
    dev = torch.device(device) if device is not None else _default_device()
    return _run(dev, plan, None, None, gt_span, n, thr, head)


@torch.no_grad()
def proposal_ar_an_batch(batch, gt=None, max_avg_nr_proposals=None, thresholds=None, points=100):
    """The same on a ``proposal_lists.ProposalBatch``, whose proposals are already on the device (``sliding_windows``,
    ``from_spans``): only ground truth, nr, thresholds and pcn go up.  The batch's order within a video is the rank:
    NMS order for ``TagResult.seconds``; sliding windows have no score and their order (level, then start) is arbitrary
    as a rank.  gt: per video the ground-truth spans in the batch's unit (seconds); None: the ``time_span`` of the
    videos' instances.  Proposals that are not finite on the device never hit."""
    if gt is None:
        gt = [[i.time_span for i in video.instances] for video in batch.videos]
    if len(gt) != len(batch.videos):
        raise ValueError("proposal_ar_an_batch: one ground-truth list per video of the batch")
    thr = _thresholds(thresholds)
    gt_span, n = _gt_arrays(gt)
    m = np.diff(np.asarray(batch.offsets, dtype=np.int64))
    plan = _plan(m, n, max_avg_nr_proposals, points)
    return _run(batch.windows.device, plan, batch.windows, batch.d_offsets, gt_span, n, thr, [])


def format_ar_an_report(result, at=(1, 5, 10, 50, 100)):
    """The report as text: AR@n for every requested n inside the curve, recall per tIoU at the curve's last point, AUC."""
    ppv = result.proposals_per_video
    lines = ["AR-AN: {} videos, {} groundtruth boxes, {} proposals, {:.2f} per video at the last point".format(
        result.num_videos, result.positives, result.total_proposals, ppv[-1])]
    for n in at:
        if ppv[0] * (1 - 1e-9) <= n <= ppv[-1] * (1 + 1e-9):          # (the last point is max_avg_nr_proposals up to rounding)
            lines.append("AR@{}: {:.2f}".format(n, result.ar_at(n) * 100))
    for th, r in zip(result.thresholds, result.recall[:, -1]):
        lines.append("tIoU {:.2f}. recall@{:.2f}: {:.2f}".format(th, ppv[-1], r * 100))
    lines.append("AUC: {:.2f}".format(result.auc * 100))
    return "\n".join(lines)
