#!/usr/bin/env python
"""Generate tests/golden/ref_eval.npz: seeded detection rows / ground truth with the tp flags, score order and AP the
evaluation must give, and proposal-recall cases with the outputs of the REFERENCE's own functions (test infrastructure;
runs only where the reference tree exists, the fixture it writes is committed).

AP: the function the reference calls (compute_average_precision_detection of the ActivityNet toolkit) sits in a
submodule that is empty in the reference tree, so there is no reference program to run.  `referee_ap` below walks the
public algorithm literally in numpy -- predictions by descending score, per threshold a walk over the video's
ground-truth rows by descending IoU with a lock array, padded precision / recall arrays -- and is NOT how the kernels
compute it (free row of highest IoU; sum of the running-maximum precision at the true positives).  Where the toolkit's
unstable argsort leaves the outcome open the referee uses stable sorts: equal scores lower flat index first, equal IoU
lower row first.

Recall: ops.detection_metrics.temporal_recall / get_temporal_proposal_recall, imported from the reference tree.

Asserted here: scores inside a class are distinct in every case but `ties`; in `dup_gt` the flags do not depend on which
of two identical ground-truth rows is taken (the referee is run with both orders); the file stays below 200 KB.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_eval.npz")
RANGES = {"thumos14": np.arange(0.1, 1.0, 0.1), "activitynet1.2": np.arange(0.5, 1.0, 0.05)}


def segment_iou(seg, gts):
    """fp64, in the order the kernels use: inter / ((ge - gs) + (e - s) - inter)"""
    inter = np.maximum(0.0, np.minimum(seg[1], gts[:, 1]) - np.maximum(seg[0], gts[:, 0]))
    union = (gts[:, 1] - gts[:, 0]) + (seg[1] - seg[0]) - inter
    return inter / union


def interpolated_prec_rec(prec, rec):
    mprec = np.hstack([[0], prec, [0]])
    mrec = np.hstack([[0], rec, [1]])
    for i in range(len(mprec) - 1)[::-1]:
        mprec[i] = max(mprec[i], mprec[i + 1])
    idx = np.where(mrec[1::] != mrec[0:-1])[0] + 1
    return np.sum((mrec[idx] - mrec[idx - 1]) * mprec[idx])


def referee_ap(gt_vid, gt_seg, p_vid, p_seg, p_score, thresholds, reverse_gt_ties=False):
    """One class.  -> (order [n], tp [T, n] uint8 in that order, ap [T])"""
    T, n, npos = len(thresholds), len(p_score), len(gt_vid)
    order = np.argsort(-p_score, kind="stable")
    lock = np.ones((T, max(npos, 1))) * -1
    tp = np.zeros((T, n))
    fp = np.zeros((T, n))
    by_video = {}
    for g, v in enumerate(gt_vid):
        by_video.setdefault(int(v), []).append(g)
    for idx, p in enumerate(order):
        rows = by_video.get(int(p_vid[p]))
        if rows is None:
            fp[:, idx] = 1
            continue
        tiou = segment_iou(p_seg[p], gt_seg[rows])
        walk = np.argsort(-tiou, kind="stable")
        if reverse_gt_ties:
            walk = (len(tiou) - 1 - np.argsort(-tiou[::-1], kind="stable"))
        for t, thr in enumerate(thresholds):
            for j in walk:
                if tiou[j] < thr:
                    fp[t, idx] = 1
                    break
                if lock[t, rows[j]] >= 0:
                    continue
                tp[t, idx] = 1
                lock[t, rows[j]] = idx
                break
            if fp[t, idx] == 0 and tp[t, idx] == 0:
                fp[t, idx] = 1
    tp_cumsum = np.cumsum(tp, axis=1).astype(np.float64)
    fp_cumsum = np.cumsum(fp, axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rec = tp_cumsum / npos
        prec = tp_cumsum / (tp_cumsum + fp_cumsum)
        ap = np.array([interpolated_prec_rec(prec[t], rec[t]) for t in range(T)])
    if npos == 0:
        # the edge rule: a class without ground truth has AP NaN (the toolkit's 0 / 0) -- also when it has no predictions
        # either, where the padded arrays alone would give 0
        ap[:] = np.nan
    return order, tp.astype(np.uint8), ap


def referee_dataset(case, **kw):
    """All classes of a flat case -> (order [N] flat indices class by class, tp [T, N], ap [C, T])"""
    thr = RANGES[case["dataset"]]
    orders, tps, aps = [], [], []
    for c in range(case["num_class"]):
        rows = np.flatnonzero(case["pred_cls"] == c)
        g = np.flatnonzero(case["gt_cls"] == c)
        o, tp, ap = referee_ap(case["gt_vid"][g], case["gt_seg"][g], case["pred_vid"][rows], case["pred_seg"][rows],
                               case["pred_score"][rows], thr, **kw)
        orders.append(rows[o])
        tps.append(tp)
        aps.append(ap)
    return np.concatenate(orders), np.concatenate(tps, axis=1), np.stack(aps)


def spans(rs, n, grid=None, lo=0.02, hi=0.5):
    s = rs.uniform(0, 1 - lo, n)
    e = np.minimum(1.0, s + rs.uniform(lo, hi, n))
    seg = np.stack([s, e], axis=1)
    if grid:                      # rational end points: many IoUs are exact and some EQUAL a threshold
        seg = np.round(seg * grid) / grid
        seg[:, 1] = np.maximum(seg[:, 1], seg[:, 0] + 1.0 / grid)
    return seg


def around(rs, gt_seg, n, jitter):
    """predictions scattered around ground-truth spans (so that every threshold separates some of them)"""
    pick = gt_seg[rs.randint(0, len(gt_seg), n)]
    seg = pick + rs.uniform(-jitter, jitter, (n, 2)) * (pick[:, 1] - pick[:, 0])[:, None]
    seg = np.sort(np.clip(seg, 0, 1), axis=1)
    seg[:, 1] = np.maximum(seg[:, 1], seg[:, 0] + 1e-3)
    return seg


def random_case(seed, dataset, num_class, n_video, gt_per_group, pred_per_group, grid=None, quantised_scores=0,
                empty_pred_class=None, empty_gt_class=None):
    rs = np.random.RandomState(seed)
    gt, pred = [], []
    for c in range(num_class):
        for v in range(n_video):
            ng = 0 if c == empty_gt_class or rs.rand() < 0.25 else int(rs.randint(1, gt_per_group + 1))
            g = spans(rs, ng, grid)
            gt.extend((c, v, a, b) for a, b in g)
            if c == empty_pred_class or rs.rand() < 0.15:
                continue
            npred = 1 if rs.rand() < 0.1 else int(rs.randint(2, pred_per_group + 1))       # (groups with ONE prediction)
            near = around(rs, g, npred // 2, 0.35) if ng else np.zeros((0, 2))
            if grid and len(near):
                near = np.round(near * grid) / grid
                near[:, 1] = np.maximum(near[:, 1], near[:, 0] + 1.0 / grid)
            seg = np.concatenate([near, spans(rs, npred - len(near), grid)])
            pred.extend((c, v, a, b) for a, b in seg)
    # predictions whose video has no ground truth of ANY class (video index beyond the ground truth's)
    pred.extend((0, n_video, a, b) for a, b in spans(rs, 3, grid))
    pred = [pred[i] for i in rs.permutation(len(pred))]            # flat order: classes and videos interleaved
    n = len(pred)
    score = rs.randint(0, quantised_scores, n) / float(quantised_scores) if quantised_scores else rs.uniform(0, 1, n)
    gt, pred = np.array(gt).reshape(-1, 4), np.array(pred).reshape(-1, 4)
    return {"dataset": dataset, "num_class": num_class, "gt_cls": gt[:, 0].astype(np.int32), "gt_vid": gt[:, 1].astype(np.int32),
            "gt_seg": gt[:, 2:].copy(), "pred_cls": pred[:, 0].astype(np.int32), "pred_vid": pred[:, 1].astype(np.int32),
            "pred_seg": pred[:, 2:].copy(), "pred_score": score}


def big_group_case(seed):
    """class 0 / video 0 holds 320 ground-truth rows (more than the kernels match out of LDS) and 260 predictions"""
    rs = np.random.RandomState(seed)
    case = random_case(seed, "thumos14", 2, 4, 3, 10)
    start = np.sort(rs.uniform(0, 0.98, 320))
    g = np.stack([start, start + rs.uniform(0.002, 0.02, 320)], axis=1)
    p = around(rs, g, 260, 0.3)
    keep_g, keep_p = ~((case["gt_cls"] == 0) & (case["gt_vid"] == 0)), ~((case["pred_cls"] == 0) & (case["pred_vid"] == 0))
    for k in ("gt_cls", "gt_vid", "gt_seg"):
        case[k] = case[k][keep_g]
    for k in ("pred_cls", "pred_vid", "pred_seg", "pred_score"):
        case[k] = case[k][keep_p]
    case["gt_cls"] = np.concatenate([case["gt_cls"], np.zeros(320, np.int32)])
    case["gt_vid"] = np.concatenate([case["gt_vid"], np.zeros(320, np.int32)])
    case["gt_seg"] = np.concatenate([case["gt_seg"], g])
    case["pred_cls"] = np.concatenate([case["pred_cls"], np.zeros(260, np.int32)])
    case["pred_vid"] = np.concatenate([case["pred_vid"], np.zeros(260, np.int32)])
    case["pred_seg"] = np.concatenate([case["pred_seg"], p])
    case["pred_score"] = np.concatenate([case["pred_score"], rs.uniform(0, 1, 260)])
    return case


def dup_gt_case(seed):
    """every ground-truth row of class 0 twice (equal IoU with every prediction)"""
    case = random_case(seed, "thumos14", 2, 5, 3, 14)
    twin = np.flatnonzero(case["gt_cls"] == 0)
    for k in ("gt_cls", "gt_vid", "gt_seg"):
        case[k] = np.concatenate([case[k], case[k][twin]])
    return case


def excerpt_case(seed):
    """the committed ActivityNet excerpt: its ground truth, its proposals as predictions with seeded scores"""
    sys.path.insert(0, ROOT)
    from action_detection_amd.proposal_sampling import ProposalSampler
    s = ProposalSampler(os.path.join(ROOT, "tests", "golden", "proposal_list_processed.txt"))
    rs = np.random.RandomState(seed)
    ids = [v.id for v in s.video_list]
    gt = [(g[1], ids.index(g[0]), g[2], g[3]) for g in s.all_gt()]
    pred = []
    for i, v in enumerate(s.video_list):
        own = v.gt[0].label - 1
        for p in v.proposals:
            cls = own if rs.rand() < 0.7 else int(rs.randint(0, 100))
            pred.append((cls, i, p.start_frame / v.num_frames, p.end_frame / v.num_frames))
    gt, pred = np.array(gt).reshape(-1, 4), np.array(pred).reshape(-1, 4)
    return {"dataset": "activitynet1.2", "num_class": 100, "gt_cls": gt[:, 0].astype(np.int32),
            "gt_vid": gt[:, 1].astype(np.int32), "gt_seg": gt[:, 2:].copy(), "pred_cls": pred[:, 0].astype(np.int32),
            "pred_vid": pred[:, 1].astype(np.int32), "pred_seg": pred[:, 2:].copy(), "pred_score": rs.uniform(0, 1, len(pred))}


def recall_cases():
    sys.path.insert(0, REF)
    from ops.detection_metrics import get_temporal_proposal_recall, temporal_recall
    rs = np.random.RandomState(11)
    out = {}
    for name, n_video, grid in (("recall_random", 9, None), ("recall_grid", 12, 8)):
        gt_list, pr_list = [], []
        for v in range(n_video):
            g = spans(rs, 0 if v == 2 else int(rs.randint(1, 5)), grid)
            near = around(rs, g, 6, 0.3) if len(g) else np.zeros((0, 2))
            if grid and len(near):
                near = np.round(near * grid) / grid
                near[:, 1] = np.maximum(near[:, 1], near[:, 0] + 1.0 / grid)
            p = np.concatenate([near, spans(rs, 10, grid)]) if v != 4 else np.zeros((0, 2))
            gt_list.append(g)
            pr_list.append(p)
        # grid 8: hull IoUs are small rationals, and 0.5 / 0.75 are hit exactly by some (the comparison is strict)
        thr = np.array([0.25, 0.5, 0.75, 0.9]) if grid else np.arange(0.1, 1.0, 0.1)
        as_tuples = lambda a: [(float(x), float(y)) for x, y in a]
        gl, pl = [as_tuples(g) for g in gt_list], [as_tuples(p) for p in pr_list]
        hits = np.array([[temporal_recall(g, p, thresh=t)[0] for t in thr] for g, p in zip(gl, pl)], dtype=np.int64)
        rec = np.array([get_temporal_proposal_recall(pl, gl, t) for t in thr], dtype=np.float64)
        if grid:
            ious = [(min(a[1], b[1]) - max(a[0], b[0])) / (max(a[1], b[1]) - min(a[0], b[0]))
                    for g, p in zip(gl, pl) for a in g for b in p if max(a[0], b[0]) < min(a[1], b[1])]
            assert any(x == 0.5 for x in ious) and any(x == 0.75 for x in ious)
        out[name + "_thr"] = thr
        out[name + "_gt"] = np.concatenate(gt_list)
        out[name + "_gt_off"] = np.concatenate([[0], np.cumsum([len(g) for g in gt_list])]).astype(np.int32)
        out[name + "_pr"] = np.concatenate(pr_list)
        out[name + "_pr_off"] = np.concatenate([[0], np.cumsum([len(p) for p in pr_list])]).astype(np.int32)
        out[name + "_hits"] = hits
        out[name + "_recall"] = rec          # [T, 2]: per_video_recall, per_inst_recall
    return out


def main():
    assert os.path.isdir(REF), "the reference tree is needed for the recall expectations"
    cases = {
        # class 3 has ground truth and no predictions, class 4 predictions and no ground truth
        "thumos_mixed": random_case(1, "thumos14", 5, 12, 4, 30, empty_pred_class=3, empty_gt_class=4),
        "anet_grid": random_case(2, "activitynet1.2", 6, 10, 3, 14, grid=16),
        "big_group": big_group_case(3),
        "dup_gt": dup_gt_case(4),
        "ties": random_case(5, "thumos14", 3, 6, 3, 20, quantised_scores=12),
        "anet_excerpt": excerpt_case(6),
        # one class, one video (a seed whose single group has ground truth and a match)
        "one_by_one": random_case(8, "thumos14", 1, 1, 2, 5),
        # more than 2048 predictions in a class: the sort leaves LDS
        "long_class": random_case(8, "thumos14", 2, 32, 4, 200, grid=1024),
    }
    out = {"names": np.array(sorted(cases))}
    for name in sorted(cases):
        case = cases[name]
        thr = RANGES[case["dataset"]]
        for c in range(case["num_class"]):
            s = case["pred_score"][case["pred_cls"] == c]
            assert (len(np.unique(s)) == len(s)) == (name != "ties") or len(s) < 2, name
        assert np.isfinite(case["pred_score"]).all() and (case["gt_seg"][:, 1] > case["gt_seg"][:, 0]).all()
        order, tp, ap = referee_dataset(case)
        if name == "dup_gt":
            o2, tp2, ap2 = referee_dataset(case, reverse_gt_ties=True)
            assert np.array_equal(order, o2) and np.array_equal(tp, tp2) and np.array_equal(ap, ap2, equal_nan=True)
        if name == "anet_grid":     # some IoU EQUALS a threshold (`<` ends the walk: equal is a match)
            hit = 0
            for v in np.unique(case["gt_vid"]):
                for c in range(case["num_class"]):
                    g = case["gt_seg"][(case["gt_vid"] == v) & (case["gt_cls"] == c)]
                    for seg in case["pred_seg"][(case["pred_vid"] == v) & (case["pred_cls"] == c)]:
                        if len(g):
                            hit += int(np.isin(segment_iou(seg, g), thr).sum())
            assert hit > 0, "no IoU equal to a threshold"
        if name == "long_class":
            assert np.bincount(case["pred_cls"]).max() > 2048
        if name == "big_group":
            assert ((case["gt_cls"] == 0) & (case["gt_vid"] == 0)).sum() >= 300
        assert tp.any() and not tp.all(), name
        for k in ("gt_cls", "gt_vid", "gt_seg", "pred_cls", "pred_vid", "pred_seg", "pred_score"):
            out[name + "_" + k] = case[k]
        out[name + "_dataset"] = np.array(case["dataset"])
        out[name + "_num_class"] = np.array([case["num_class"]], dtype=np.int32)
        out[name + "_order"] = order.astype(np.int32)
        out[name + "_tp"] = np.packbits(tp, axis=1)
        out[name + "_ap"] = ap
        print("%-13s N %5d G %4d C %3d  mAP %s" % (name, len(case["pred_score"]), len(case["gt_cls"]), case["num_class"],
                                                    np.round(np.nanmean(ap, axis=0), 3)))
    out.update(recall_cases())
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 200 * 1024, size
    print("wrote", OUT, size, "bytes")


if __name__ == "__main__":
    main()
