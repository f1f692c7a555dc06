#!/usr/bin/env python
"""Detection post-processing of a whole subset: the batched pass (DetectionPostProcessor.process_videos, csrc/detect_batch.hip)
against the per-video loop of the same tree (process_video_device, csrc/detect.hip), on seeded synthetic score dicts of
the size of the two benchmarks:

    thumos14         213 videos, P around 1000, C = 20, top_k 2000, NMS 0.2
    activitynet      2383 videos, P around 50 (at most 187), C = 100, top_k 60, NMS 0.6
    activitynet_cls  the same scores in the --cls_scores branch with cls_top_k 1

    python tools/bench_detection_post.py [--config all] [--repeats 7] [--scale 1] [--out profiles/detection_post_measured.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_detection_post.py --config activitynet --scale 2 --trace-only

Per configuration: (1) the rows of both paths are compared bit for bit; (2) after a warm-up of both, `repeats` alternating
timed runs of each: score dict in -> evaluator-ready flat rows on the device (the evaluator's add_* calls and its
_flat_rows included; host clock around work that ends in a device synchronise), median and min-max; (3) HIP-event medians
of the two C calls of the batched path on device-resident inputs (output allocation included); (4) the host merge of two
score sources (detection_eval.merge_detection_scores) beside them.  --trace-only runs ONE batched pass and nothing else,
for a kernel trace of its own: the launch counts for --scale 1 and 2 show that they do not depend on the number of videos.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CONFIGS = {
    "thumos14": dict(videos=213, p_mean=1000, p_max=4000, classes=20, top_k=2000, nms=0.2, cls=False),
    "activitynet": dict(videos=2383, p_mean=50, p_max=187, classes=100, top_k=60, nms=0.6, cls=False),
    "activitynet_cls": dict(videos=2383, p_mean=50, p_max=187, classes=100, top_k=60, nms=0.6, cls=True),
}


def make_scores(cfg, scale, seed):
    """Two score sources (as two modalities' pickles) for the merge, and classifier scores."""
    rs = np.random.RandomState(seed)
    v, c = cfg["videos"] * scale, cfg["classes"]
    sizes = np.clip(rs.poisson(cfg["p_mean"], v) + rs.randint(-cfg["p_mean"] // 2, cfg["p_mean"] // 2 + 1, v), 1, cfg["p_max"])
    sizes[rs.randint(0, v)] = cfg["p_max"]
    sources, cls_scores = [{}, {}], {}
    for i, p in enumerate(sizes):
        vid = "video_%05d" % i
        start = rs.uniform(0, 0.8, p)
        rel = np.stack([start, np.minimum(start + rs.uniform(0.02, 0.5, p), 1.0)], axis=1)[None]
        for s in sources:
            s[vid] = (rel, rs.standard_normal((p, c + 1)).astype(np.float32) * 2, rs.standard_normal((p, c)).astype(np.float32),
                      (rs.standard_normal((p, c, 2)) * 0.3).astype(np.float32))
        cls_scores[vid] = rs.standard_normal(c).astype(np.float32)
    return sources, cls_scores, sizes


def spread(xs, scale=1e3):
    xs = np.asarray(xs) * scale
    return {"median": round(float(np.median(xs)), 3), "min": round(float(xs.min()), 3), "max": round(float(xs.max()), 3)}


def run(name, cfg, a):
    import torch
    import action_detection_amd as pkg
    from action_detection_amd import kernels as K
    from action_detection_amd.detection_eval import DetectionEvaluator, merge_detection_scores
    from action_detection_amd.detection_post import DetectionPostProcessor
    pkg.build()
    assert torch.cuda.is_available(), "bench_detection_post.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    sources, cls_scores, sizes = make_scores(cfg, a.scale, a.seed)
    c = cfg["classes"]
    post = DetectionPostProcessor(c, cfg["nms"], cfg["top_k"], cls_top_k=1)
    vcls = cls_scores if cfg["cls"] else None
    t_merge = []
    for _ in range(3):
        t0 = time.perf_counter()
        scores = merge_detection_scores(sources, [1.0, 1.2])
        t_merge.append(time.perf_counter() - t0)

    def batched():
        ev = DetectionEvaluator(c, [0.5], device=dev)
        ev.add_batch(post.process_videos(scores, device=dev, video_cls_scores=vcls))
        rows = ev._flat_rows(dev)
        torch.cuda.synchronize()
        return rows

    if a.trace_only:
        batched()
        return {"config": name, "videos": len(sizes), "trace_only": True}

    def per_video():
        ev = DetectionEvaluator(c, [0.5], device=dev)
        for vid, (rel, act, comp, reg) in scores.items():
            dets, _ = post.process_video_device(np.asarray(rel), torch.as_tensor(np.asarray(act)).to(dev),
                                                torch.as_tensor(np.asarray(comp)).to(dev),
                                                torch.as_tensor(np.asarray(reg)).to(dev), device=dev,
                                                video_cls_score=None if vcls is None else vcls[vid])
            ev.add_video(vid, dets)
        rows = ev._flat_rows(dev)
        torch.cuda.synchronize()
        return rows

    got, want = batched(), per_video()                   # warm-up of both paths, and the comparison
    for g, w in zip(got, want):
        view = torch.int64 if g.dtype == torch.float64 else torch.int32
        assert g.shape == w.shape and torch.equal(g.contiguous().view(view), w.contiguous().view(view)), "the two paths differ"
    t_b, t_p = [], []
    for _ in range(a.repeats):
        for fn, dst in ((batched, t_b), (per_video, t_p)):
            t0 = time.perf_counter()
            fn()
            dst.append(time.perf_counter() - t0)

    # the two C calls on device-resident inputs, HIP events
    b = post.process_videos(scores, device=dev, video_cls_scores=vcls)
    put = lambda xs, dt, shape: torch.from_numpy(np.concatenate([np.asarray(x).reshape(shape) for x in xs])).to(dev, dt)  # noqa: E731
    vals = list(scores.values())
    rel = put([x[0] for x in vals], torch.float64, (-1, 2))
    act = put([x[1] for x in vals], torch.float32, (-1, c + 1))
    comp = put([x[2] for x in vals], torch.float32, (-1, c))
    reg = put([x[3] for x in vals], torch.float32, (-1, c, 2))
    h_off = b.p_off.cpu()
    report = None
    if cfg["cls"]:
        mask = np.zeros((len(vals), c), dtype=np.uint8)
        for i, vid in enumerate(scores):
            mask[i, np.argsort(vcls[vid],)[-1:]] = 1
        report = torch.from_numpy(mask).to(dev)
    top_k, mode = (0, 2) if cfg["cls"] else (cfg["top_k"], 0)
    t_call, t_fill = [], []
    for _ in range(a.repeats + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        combined, kept, row_off = K.detections_batch(act, comp, rel, h_off, b.p_off, report, top_k, mode, cfg["nms"])
        e[1].record()
        n = int(row_off[-1])
        e[2].record()
        rows = K.detections_batch_fill(rel, combined, reg, b.p_off, kept, row_off, n, True)[0]
        e[3].record()
        torch.cuda.synchronize()
        t_call.append(e[0].elapsed_time(e[1]))
        t_fill.append(e[2].elapsed_time(e[3]))
    assert torch.equal(rows.view(torch.int64), b.rows.view(torch.int64))
    return {"config": name, "videos": len(sizes), "classes": c, "proposals": int(sizes.sum()), "largest_video": int(sizes.max()),
            "top_k": cfg["top_k"], "nms": cfg["nms"], "cls_scores_branch": cfg["cls"], "rows": int(got[1].shape[0]),
            "repeats": a.repeats, "rows_bit_equal": True,
            "batched_ms": spread(t_b), "per_video_ms": spread(t_p),
            "per_video_over_batched": round(float(np.median(t_p) / np.median(t_b)), 2),
            "ssn_detections_batch_ms": spread(t_call[1:], 1.0), "ssn_detections_batch_fill_ms": spread(t_fill[1:], 1.0),
            "host_merge_ms": spread(t_merge)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=sorted(CONFIGS) + ["all"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=int, default=1, help="multiply the number of videos (launch counts for V and 2 V)")
    ap.add_argument("--trace-only", action="store_true", help="one batched pass and nothing else (for a kernel trace)")
    ap.add_argument("--out", type=str, default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for name in (["thumos14", "activitynet", "activitynet_cls"] if a.config == "all" else [a.config]):
        line = json.dumps(run(name, CONFIGS[name], a))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
