#!/usr/bin/env python
"""Video-level aggregation and metrics (video_cls.py / csrc/video_cls.hip) at the size of the ActivityNet 1.2 validation set:
2383 synthetic videos, tick counts drawn from the committed ActivityNet excerpt (tests/golden/proposal_list_processed.txt at
frame interval 6), 100 classes, 10 crops.

    python tools/bench_video_cls.py [--repeats 20] [--referee-videos 200] [--seed 0]

One JSON line.  Device times are HIP events around ``VideoScoreAggregator.aggregate`` (``sliding_window`` and ``default``)
and ``classification_metrics``' kernel call on device-resident inputs, after a warm-up call each: the median of
``--repeats`` calls and their spread (min ... max).  The yardstick is the numpy restatement of the same rules on this
machine's CPU (float64 aggregation of tests/video_cls_referee.py, one process) on the first ``--referee-videos`` videos,
scaled by rows; 0 skips it.  Nothing is gated on these figures.  Per-kernel times come from running this script under
``rocprofv3 --kernel-trace --stats`` (kernel names vcls_*_kernel), in a run of its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

VIDEOS, CLASSES, CROPS = 2383, 100, 10


def tick_counts(seed):
    from action_detection_amd.proposal_io import load_proposal_file
    frames = [r[1] for r in load_proposal_file(os.path.join(ROOT, "tests", "golden", "proposal_list_processed.txt"))]
    ticks = [len(range(0, n - 1, 6)) for n in frames]
    return np.random.RandomState(seed).choice(ticks, VIDEOS)


def timed(fn, repeats):
    import torch
    fn()                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--referee-videos", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    import torch
    import action_detection_amd as pkg
    from action_detection_amd import kernels as K
    from action_detection_amd.video_cls import VideoScoreAggregator
    pkg.build()
    assert torch.cuda.is_available(), "bench_video_cls.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    ts = tick_counts(a.seed)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    vids = [3 * torch.randn((int(t), CROPS, CLASSES), device=dev, generator=gen) for t in ts]
    out = {"what": "video-level aggregation + metrics on one MI355X", "videos": VIDEOS, "classes": CLASSES, "crops": CROPS,
           "ticks": int(ts.sum()), "input_MB": round(4e-6 * int(ts.sum()) * CROPS * CLASSES, 1), "repeats": a.repeats, "seed": a.seed}
    results = {}
    for mode in ("sliding_window", "default"):
        agg = VideoScoreAggregator(mode)
        results[mode], out[mode] = timed(lambda: agg.aggregate(vids), a.repeats)
    # aggregate() includes the torch.cat of the 2383 tensors into one [N, crops, C] block and the upload of the offset tables;
    # the cat alone, for its share:
    _, out["torch_cat_alone"] = timed(lambda: torch.cat(vids, 0), a.repeats)
    rs = np.random.RandomState(a.seed + 1)
    labels = rs.randint(0, CLASSES, VIDEOS)
    labels[:CLASSES] = np.arange(CLASSES)
    gt = np.zeros((VIDEOS, CLASSES), dtype=np.uint8)
    gt[np.arange(VIDEOS), labels] = 1
    scores = results["sliding_window"].scores
    gt_d, lab_d = torch.from_numpy(gt).to(dev), torch.from_numpy(labels.astype(np.int32)).to(dev)
    ks = torch.tensor([1, 3], dtype=torch.int32).to(dev)
    (_, _, res), out["metrics"] = timed(lambda: K.vcls_metrics(scores, gt_d, lab_d, ks), a.repeats)
    res = res.cpu().numpy()
    out["top1"], out["top3"], out["mean_ap"], out["mean_class_accuracy"] = [round(float(x), 6) for x in res]
    assert results["sliding_window"].status.count_nonzero().item() == 0
    if a.referee_videos:
        import video_cls_referee as R
        n = min(a.referee_videos, VIDEOS)
        host = [v.cpu().numpy() for v in vids[:n]]
        share = float(ts[:n].sum()) / float(ts.sum())
        for mode, fn in (("sliding_window", lambda v: R.agg_sliding(v, 1, True)), ("default", lambda v: R.agg_default(v, True))):
            t0 = time.perf_counter()
            ref = np.stack([fn(v) for v in host])
            dt = time.perf_counter() - t0
            err = float(np.abs(results[mode].scores[:n].cpu().numpy() - ref).max())
            out[mode].update({"referee_videos": n, "referee_s": round(dt, 3), "referee_s_scaled_to_all_rows": round(dt / share, 3),
                              "max_abs_difference_to_referee": err})
        s_h = scores.cpu().numpy()
        t0 = time.perf_counter()
        top1 = float((np.argmax(s_h, axis=1) == labels).mean())
        try:
            from sklearn.metrics import average_precision_score      # (host yardstick of the mAP, where it is installed)
            m_ap = float(average_precision_score(gt, s_h, average="macro"))
            out["metrics"].update({"referee": "sklearn average_precision_score + numpy argmax", "mean_ap_difference": abs(m_ap - float(res[2]))})
        except ImportError:
            out["metrics"]["referee"] = "numpy argmax (sklearn is not installed: mAP not compared)"
        out["metrics"].update({"referee_s": round(time.perf_counter() - t0, 3), "top1_difference": abs(top1 - float(res[0]))})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
