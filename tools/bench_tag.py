#!/usr/bin/env python
"""TAG proposal generation (tag_proposals.TagProposalGenerator / csrc/tag.hip) on a seeded batch of synthetic videos.

    python tools/bench_tag.py [--videos 2000] [--seed 0] [--iters 5]      on the GPU: one JSON line
    python tools/bench_tag.py --reference 16                              where the reference tree exists: the reference's
                                                                           gen_prop arithmetic on the first 16 videos of the
                                                                           same seeded batch, one process, one JSON line

GPU figures: HIP-event medians of the two C ABI phases (ssn_tag_count: softmax, smoothing, run counting -- three
kernels; ssn_tag_generate: grouping + NMS -- two or three kernels) on device-resident inputs, and videos/s of
``generate`` end to end (host concatenation, one upload, the host read between the phases, results back on the host)
timed with a host clock around calls that end in device-to-host copies.  Per-kernel times come from running this script
under ``rocprofv3 --kernel-trace --stats`` (kernel names tag_*_kernel), in a run of its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def make_batch(n, seed):
    """n videos with lengths spread over 100 ... 4000 frames: foreground segments on noisy logits (about one per 150 frames)"""
    rs = np.random.RandomState(seed)
    vids, durs = [], []
    for _ in range(n):
        T = int(rs.randint(100, 4001))
        base = -np.ones(T)
        for _ in range(max(2, T // 150)):
            ln = int(rs.randint(8, 80))
            s = int(rs.randint(0, max(1, T - ln)))
            base[s:s + ln] = 1.0
        logit = base * 1.5 + rs.standard_normal(T) * 2.0
        common = rs.standard_normal(T) * 0.5
        vids.append(np.stack([common - logit / 2, common + logit / 2], axis=1).astype(np.float32))
        durs.append(T / 6.0)
    return vids, durs


def run_reference(vids, durs, n):
    sys.path.insert(0, "/root/reference")
    from ops import sequence_funcs as SF
    from action_detection_amd.tag_proposals import DEFAULT_THRESHOLDS, DEFAULT_TOLERANCES
    t0 = time.perf_counter()
    kept = cands = 0
    for s, d in zip(vids[:n], durs[:n]):
        rows = SF.label_frame_by_threshold(s, [0], bw=3, thresh=list(DEFAULT_THRESHOLDS), multicrop=False)
        boxes = SF.build_box_by_search(rows, np.array(DEFAULT_TOLERANCES))
        cands += len(boxes)
        if boxes:
            kept += len(SF.temporal_nms(boxes, 0.9))
    dt = time.perf_counter() - t0
    return {"what": "reference gen_prop arithmetic (numpy, one process, CPU)", "videos": n,
            "frames": int(sum(len(s) for s in vids[:n])), "candidates": cands, "kept": kept,
            "seconds": round(dt, 3), "videos_per_s": round(n / dt, 3)}


def run_gpu(vids, durs, iters):
    import torch
    import action_detection_amd as pkg
    from action_detection_amd import kernels as K
    from action_detection_amd.tag_proposals import TagProposalGenerator
    pkg.build()
    assert torch.cuda.is_available(), "bench_tag.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    gen = TagProposalGenerator(device=dev)
    res = gen.generate(vids, durs)                      # warm-up: code objects, allocator
    end_to_end = []
    for _ in range(iters):
        t0 = time.perf_counter()
        res = gen.generate(vids, durs)
        end_to_end.append(time.perf_counter() - t0)
    # the two ABI phases on device-resident inputs, HIP events
    lens = np.array([len(s) for s in vids])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    h_off = torch.from_numpy(offsets)
    d_off = h_off.to(dev)
    cat = torch.from_numpy(np.concatenate(vids)).to(dev)
    thr = torch.from_numpy(gen.thresholds).to(dev)
    tol = torch.from_numpy(gen.tolerances).to(dev)
    dur = torch.tensor(durs, dtype=torch.float64).to(dev)
    n_thr, n_tol = gen.thresholds.size, gen.tolerances.size
    t_count, t_gen = [], []
    for _ in range(iters + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        smoothed, _, runs = K.tag_count(cat, h_off, d_off, thr, gen.bw)
        e[1].record()
        runs_h = runs.cpu().numpy().astype(np.int64).ravel()
        run_off = np.concatenate([[0], np.cumsum(runs_h)])
        n_cand = np.diff(2 * n_tol * run_off[::n_thr])
        pow2 = np.left_shift(np.int64(1), np.frexp(np.maximum(n_cand - 1, 0).astype(np.float64))[1].astype(np.int64))
        sort_off = np.concatenate([[0], np.cumsum(np.where(n_cand > K.tag_lds_candidates(), pow2, 0))])
        ro, so = torch.from_numpy(run_off.astype(np.int32)).to(dev), torch.from_numpy(sort_off.astype(np.int64)).to(dev)
        e[2].record()
        K.tag_generate(cat, smoothed, d_off, dur, thr, tol, ro, so, int(run_off[-1]), int(sort_off[-1]), 0.9, 0.0)
        e[3].record()
        torch.cuda.synchronize()
        t_count.append(e[0].elapsed_time(e[1]))
        t_gen.append(e[2].elapsed_time(e[3]))
    med = float(np.median(end_to_end))
    return {"what": "TagProposalGenerator.generate on one MI355X", "videos": len(vids), "frames": int(lens.sum()),
            "candidates": int(n_cand.sum()), "videos_over_lds_capacity": int((n_cand > K.tag_lds_candidates()).sum()),
            "kept": int(sum(len(r.boxes) for r in res)),
            "count_phase_ms_median": round(float(np.median(t_count[1:])), 3),
            "generate_phase_ms_median": round(float(np.median(t_gen[1:])), 3),
            "generate_phase_includes": "output + workspace allocation (torch.zeros) and the grouping / NMS kernels",
            "end_to_end_s_median": round(med, 4), "end_to_end_s_all": [round(x, 4) for x in end_to_end],
            "videos_per_s": round(len(vids) / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reference", type=int, default=0, help="time the reference's functions on the first N videos instead")
    a = ap.parse_args()
    vids, durs = make_batch(a.videos, a.seed)
    out = run_reference(vids, durs, a.reference) if a.reference else run_gpu(vids, durs, a.iters)
    out.update({"seed": a.seed, "batch": a.videos})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
