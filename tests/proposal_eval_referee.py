"""numpy referee for AR-AN (action_detection_amd.proposal_eval): a restatement of the ActivityNet toolkit's public
``average_recall_vs_avg_nr_proposals`` in float64 with its loops kept as they are -- over videos, thresholds and curve
points.  The toolkit itself is an empty submodule in the reference tree, so this file is what parity is measured against.
The one rule added: with scores, proposals of equal score rank in input order (a stable descending sort)."""
import numpy as np


def segment_iou(target_segment, candidate_segments):
    """tIoU of one span with an array of spans [m, 2], the toolkit's operations in their order."""
    tt1 = np.maximum(target_segment[0], candidate_segments[:, 0])
    tt2 = np.minimum(target_segment[1], candidate_segments[:, 1])
    segments_intersection = (tt2 - tt1).clip(0)
    segments_union = (candidate_segments[:, 1] - candidate_segments[:, 0]) + (target_segment[1] - target_segment[0]) \
        - segments_intersection
    with np.errstate(divide="ignore", invalid="ignore"):
        return segments_intersection.astype(float) / segments_union


def stable_descending(scores):
    """Positions by descending score, equal scores in input order."""
    scores = np.asarray(scores, dtype=np.float64)
    return np.asarray(sorted(range(len(scores)), key=lambda i: -scores[i]), dtype=np.int64)      # (sorted() is stable)


def ar_an(pr_list, gt_list, scores=None, max_avg_nr_proposals=None, thresholds=None, points=100):
    """-> dict with recall [T, J], avg_recall [J], proposals_per_video [J], auc, matches [T, J], positives,
    total_proposals, first_hit [G, T] (-1: never)."""
    thr = np.linspace(0.5, 0.95, 10) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    props = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in pr_list]
    gts = [np.asarray(g, dtype=np.float64).reshape(-1, 2) for g in gt_list]
    if scores is not None:
        for s in scores:
            if not np.isfinite(np.asarray(s, dtype=np.float64)).all():
                raise ValueError("score not finite")
        props = [p[stable_descending(s)] if len(p) else p for p, s in zip(props, scores)]
    for a in props + gts:
        if not np.isfinite(a).all():
            raise ValueError("span not finite")
    counted = [i for i in range(len(gts)) if len(gts[i]) >= 1]
    v = len(counted)
    p_total = sum(len(p) for p in props)
    positives = sum(len(gts[i]) for i in counted)
    if positives == 0:
        raise ValueError("no ground truth")
    if p_total == 0:
        raise ValueError("no proposals")
    if max_avg_nr_proposals is None or max_avg_nr_proposals == 0:
        max_avg_nr_proposals = float(p_total) / v
    ratio = max_avg_nr_proposals * float(v) / p_total

    # per counted video: the tIoU of the retained proposals with every ground-truth span, [nr, n]
    score_lst, nr_lst, total_nr = [], [], 0
    for i in counted:
        m_i = len(props[i])
        nr_i = min(int(m_i * ratio), m_i)
        nr_lst.append(nr_i)
        total_nr += nr_i
        if m_i == 0 or nr_i == 0:
            score_lst.append(np.zeros((0, len(gts[i]))))
            continue
        tiou = np.empty((nr_i, len(gts[i])))
        for g in range(len(gts[i])):
            tiou[:, g] = segment_iou(gts[i][g], props[i][:nr_i])
        score_lst.append(tiou)
    if total_nr == 0:
        raise ValueError("no proposals left")

    j_n = int(points)
    pcn = np.arange(1, j_n + 1) / float(j_n) * (max_avg_nr_proposals * float(v) / total_nr)
    matches = np.zeros((len(thr), j_n), dtype=np.int64)
    first_hit = np.full((positives, len(thr)), -1, dtype=np.int64)
    for t, th in enumerate(thr):
        row = 0
        for tiou, nr_i in zip(score_lst, nr_lst):
            for g in range(tiou.shape[1]):
                hits = np.flatnonzero(tiou[:, g] >= th)
                if len(hits):
                    first_hit[row + g, t] = hits[0]
            row += tiou.shape[1]
            if nr_i == 0:
                continue
            covered = np.logical_or.accumulate(tiou >= th, axis=0)      # [k - 1, g]: span g is hit by one of the first k
            for j in range(j_n):
                k = min(int(nr_i * pcn[j]), nr_i)
                if k == 0:
                    continue
                matches[t, j] += np.count_nonzero(covered[k - 1])
    recall = matches / float(positives)
    avg_recall = recall.mean(axis=0)
    ppv = pcn * (float(total_nr) / v)
    area = 0.0
    for j in range(j_n - 1):
        area += (ppv[j + 1] - ppv[j]) * (avg_recall[j + 1] + avg_recall[j]) / 2.0
    return dict(recall=recall, avg_recall=avg_recall, proposals_per_video=ppv, auc=area / ppv[-1], matches=matches,
                positives=positives, total_proposals=total_nr, first_hit=first_hit, thresholds=thr, num_videos=v)
