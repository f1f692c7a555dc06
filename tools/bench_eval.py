#!/usr/bin/env python
"""Detection evaluation (detection_eval.average_precision_flat / csrc/eval.hip) on seeded synthetic datasets of the size of
THUMOS14 (20 classes x 213 videos x ~100 rows per class and video) and ActivityNet 1.2 (100 classes x 2383 videos, ~100
rows per video in its top class).

    python tools/bench_eval.py [--dataset thumos14|activitynet1.2|both] [--iters 5] [--referee-classes N]

Per dataset one JSON line: the median of `iters` evaluations end to end (host arrays in, AP on the host: uploads, the
sizing read, both C calls, the copy back; host clock around calls that end in a device-to-host copy), HIP-event medians
of the two C ABI calls on device-resident inputs (ssn_eval_count; ssn_eval_ap = memsets + fill + sort + match + AP
kernels, output allocation included), and the numpy referee of tools/make_eval_golden.py on the same inputs on this
machine's CPU (one process; `--referee-classes` classes are timed and the figure is scaled by rows, 0 skips it).  The
referee is the yardstick because the function the reference calls sits in an empty submodule.  Per-kernel times come
from running this script under ``rocprofv3 --kernel-trace --stats`` (kernel names eval_*_kernel), in a run of its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402


def make_dataset(name, seed):
    rs = np.random.RandomState(seed)
    if name == "thumos14":
        num_class, n_video = 20, 213
        classes_of = [rs.choice(num_class, int(rs.randint(1, 3)), replace=False) for _ in range(n_video)]
        pred_classes = [np.arange(num_class)] * n_video          # top_k over all pairs: rows in every class
        per = 100
        gt_per = 15
    else:
        num_class, n_video = 100, 2383
        classes_of = [rs.choice(num_class, 1) for _ in range(n_video)]
        pred_classes = [c if rs.rand() < 0.8 else rs.choice(num_class, 1) for c in classes_of]      # cls_top_k = 1
        per = 100
        gt_per = 2
    gt, pred = [], []
    for v in range(n_video):
        spans = {}
        for c in classes_of[v]:
            n = int(rs.randint(1, gt_per + 1))
            s = rs.uniform(0, 0.9, n)
            g = np.stack([s, s + rs.uniform(0.01, 0.1, n)], axis=1)
            spans[int(c)] = g
            gt.append(np.column_stack([np.full(n, c), np.full(n, v), g]))
        for c in pred_classes[v]:
            n = int(rs.randint(per // 2, per * 3 // 2))
            s = rs.uniform(0, 0.9, n)
            p = np.stack([s, s + rs.uniform(0.01, 0.1, n)], axis=1)
            if int(c) in spans:                                   # half of the rows near a ground-truth span
                g = spans[int(c)][rs.randint(0, len(spans[int(c)]), n // 2)]
                p[:n // 2] = np.sort(g + rs.uniform(-0.3, 0.3, g.shape) * (g[:, 1] - g[:, 0])[:, None], axis=1)
                p[:, 1] = np.maximum(p[:, 1], p[:, 0] + 1e-4)
            pred.append(np.column_stack([np.full(n, c), np.full(n, v), p]))
    gt, pred = np.concatenate(gt), np.concatenate(pred)
    return {"dataset": name, "num_class": num_class, "gt_cls": gt[:, 0].astype(np.int32), "gt_vid": gt[:, 1].astype(np.int32),
            "gt_seg": gt[:, 2:].copy(), "pred_cls": pred[:, 0].astype(np.int32), "pred_vid": pred[:, 1].astype(np.int32),
            "pred_seg": pred[:, 2:].copy(), "pred_score": rs.uniform(0, 1, len(pred))}


def run(case, iters, referee_classes):
    import torch
    import action_detection_amd as pkg
    from action_detection_amd import kernels as K
    from action_detection_amd.detection_eval import average_precision_flat, tiou_thresholds
    pkg.build()
    assert torch.cuda.is_available(), "bench_eval.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    thr = tiou_thresholds(case["dataset"])
    c = case["num_class"]

    def evaluate():
        return average_precision_flat(case["pred_seg"], case["pred_score"], case["pred_cls"], case["pred_vid"], case["gt_seg"],
                                      case["gt_cls"], case["gt_vid"], c, thr, device=dev)
    ap = evaluate().ap                                   # warm-up: code objects, allocator
    end_to_end = []
    for _ in range(iters):
        t0 = time.perf_counter()
        ap = evaluate().ap
        end_to_end.append(time.perf_counter() - t0)

    # the two C calls on device-resident inputs, HIP events (tables as average_precision_flat builds them)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    seg, score, cls, vid = put(case["pred_seg"]), put(case["pred_score"]), put(case["pred_cls"]), put(case["pred_vid"])
    g_order = np.lexsort((case["gt_vid"], case["gt_cls"]))
    gc, gv = case["gt_cls"][g_order], case["gt_vid"][g_order]
    head = np.ones(len(gc), dtype=bool)
    head[1:] = (gc[1:] != gc[:-1]) | (gv[1:] != gv[:-1])
    first = np.flatnonzero(head)
    rows = np.diff(np.append(first, len(gc)))
    assert rows.max() <= K.eval_lds_gt()
    groups = put(np.stack([gc[first], gv[first], first, rows, np.zeros_like(rows)], axis=1).astype(np.int32))
    gt_seg, npos, thr_d = put(case["gt_seg"][g_order]), put(np.bincount(case["gt_cls"], minlength=c).astype(np.int32)), put(thr)
    t_count, t_ap = [], []
    for _ in range(iters + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        counts = K.eval_count(score, cls, c)
        e[1].record()
        per_class = counts.cpu().numpy().astype(np.int64)[:c]
        pred_off = np.concatenate([[0], np.cumsum(per_class)])
        pow2 = np.left_shift(np.int64(1), np.frexp(np.maximum(per_class - 1, 0).astype(np.float64))[1].astype(np.int64))
        sort_off = np.concatenate([[0], np.cumsum(np.where(per_class > 0, pow2, 0))])
        po, so = put(pred_off.astype(np.int32)), put(sort_off.astype(np.int64))
        e[2].record()
        _, _, ap_d = K.eval_ap(seg, score, cls, vid, gt_seg, groups, npos, thr_d, po, so, int(sort_off[-1]), 0)
        e[3].record()
        torch.cuda.synchronize()
        t_count.append(e[0].elapsed_time(e[1]))
        t_ap.append(e[2].elapsed_time(e[3]))
    assert np.array_equal(ap_d.cpu().numpy(), ap, equal_nan=True)
    out = {"what": "average_precision_flat on one MI355X", "dataset": case["dataset"], "classes": c,
           "videos": int(case["pred_vid"].max()) + 1, "predictions": len(case["pred_score"]), "ground_truth": len(case["gt_cls"]),
           "gt_groups": len(rows), "thresholds": len(thr), "largest_class": int(per_class.max()),
           "end_to_end_ms_median": round(1e3 * float(np.median(end_to_end)), 3),
           "end_to_end_ms_all": [round(1e3 * x, 3) for x in end_to_end],
           "count_call_ms_median": round(float(np.median(t_count[1:])), 3),
           "ap_call_ms_median": round(float(np.median(t_ap[1:])), 3), "map_per_iou": [round(float(x), 4) for x in np.nanmean(ap, axis=0)]}
    if referee_classes:
        import make_eval_golden as G
        sub = [k for k in np.argsort(-per_class)[:referee_classes]]        # the largest classes (the slowest for both sides)
        t0 = time.perf_counter()
        worst = 0.0
        for k in sub:
            r, g = np.flatnonzero(case["pred_cls"] == k), np.flatnonzero(case["gt_cls"] == k)
            _, _, ref_ap = G.referee_ap(case["gt_vid"][g], case["gt_seg"][g], case["pred_vid"][r], case["pred_seg"][r],
                                        case["pred_score"][r], thr)
            with np.errstate(invalid="ignore"):
                worst = max(worst, float(np.nanmax(np.abs(ref_ap - ap[k]))) if len(g) else 0.0)
        dt = time.perf_counter() - t0
        covered = int(per_class[sub].sum())
        out.update({"referee": "numpy referee (tools/make_eval_golden.py), one process, this machine's CPU",
                    "referee_classes": len(sub), "referee_rows": covered, "referee_s": round(dt, 3),
                    "referee_s_scaled_to_all_rows": round(dt * len(case["pred_score"]) / max(covered, 1), 3),
                    "max_abs_ap_difference_to_referee": worst})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="both", choices=["thumos14", "activitynet1.2", "both"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--referee-classes", type=int, default=1000, help="classes the referee is timed on (largest first); 0: none")
    a = ap.parse_args()
    for name in (["thumos14", "activitynet1.2"] if a.dataset == "both" else [a.dataset]):
        out = run(make_dataset(name, a.seed), a.iters, a.referee_classes)
        out["seed"] = a.seed
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
