#!/usr/bin/env python
"""Measure TV-L1 flow extraction on one MI355X (optical_flow.FlowExtractor, csrc/flow.hip): one JSON line, and with --out the
text of profiles/flow_measured.txt.

    timeout -k 10 540 python tools/bench_flow.py [--pairs 32] [--pair-batch 16] [--iters 3] [--out profiles/flow_measured.txt]

A seeded synthetic clip at 340 x 256 (a smooth texture under a slow rotation and drift, plus sensor noise) runs through
FlowExtractor.extract with the default parameters.  The parent commit has no flow extraction to compare with, so the baseline is
the same run with ssn_tvl1_iterate limited to ONE iteration per launch (state through HBM every iteration, ten times the
launches); the two alternate inside one process and their outputs are compared.  Whole calls, host clock around work that ends
in a device synchronise; a warm-up call first.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic_clip(frames, h, w, seed):
    """uint8 [frames, h, w, 3]: a blurred-noise texture sampled under a rotation of 0.15 degrees and a drift of (1.2, -0.6) px
    per frame about the image centre, plus Gaussian noise of sigma 1.5."""
    import numpy as np
    rs = np.random.RandomState(seed)
    m = 24
    tex = rs.uniform(0, 1, (3, h + 2 * m, w + 2 * m))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for _ in range(3):
        tex = np.apply_along_axis(lambda r: np.convolve(np.pad(r, 2, mode="edge"), k, mode="valid"), 2, tex)
        tex = np.apply_along_axis(lambda r: np.convolve(np.pad(r, 2, mode="edge"), k, mode="valid"), 1, tex)
    tex = (tex - tex.min()) * (255.0 / (tex.max() - tex.min()))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((frames, h, w, 3), dtype=np.uint8)
    for t in range(frames):
        a = np.deg2rad(0.15 * t)
        cx = (xs - w / 2) * np.cos(a) - (ys - h / 2) * np.sin(a) + w / 2 + m - 1.2 * t
        cy = (xs - w / 2) * np.sin(a) + (ys - h / 2) * np.cos(a) + h / 2 + m + 0.6 * t
        cx, cy = np.clip(cx, 0, w + 2 * m - 1.001), np.clip(cy, 0, h + 2 * m - 1.001)
        x0, y0 = cx.astype(np.int64), cy.astype(np.int64)
        fx, fy = cx - x0, cy - y0
        img = ((1 - fy) * ((1 - fx) * tex[:, y0, x0] + fx * tex[:, y0, x0 + 1])
               + fy * ((1 - fx) * tex[:, y0 + 1, x0] + fx * tex[:, y0 + 1, x0 + 1]))
        img = img + rs.normal(0, 1.5, img.shape)
        out[t] = np.clip(np.rint(img), 0, 255).astype(np.uint8).transpose(1, 2, 0)
    return out


def commit_name():
    if os.environ.get("BENCH_COMMIT"):
        return os.environ["BENCH_COMMIT"]
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain"], stderr=subprocess.DEVNULL).decode().strip()
        return head + (" + the working tree of this change" if dirty else "")
    except Exception:
        return "unknown (no git metadata where this ran; set BENCH_COMMIT)"


def report(r):
    return """TV-L1 flow extraction: tools/bench_flow.py on one {device} (host {host}), commit measured: {commit}.
Method: a warm-up call of each version first, then {iters} timed repetitions alternating the two versions, medians; whole
FlowExtractor.extract calls (gray, pyramid, warps, iterations, quantiser) with a host clock around work that ends in a device
synchronise; frames resident on the device.  No profiler attached.  Input: seeded synthetic clip, {pairs} consecutive pairs at
{w} x {h}, pair_batch {pair_batch}; defaults of cuda::OpticalFlowDual_TVL1 (5 scales, 5 warps, up to 300 iterations, epsilon 0.01),
error tested every 10 iterations.  Iterations the pairs ran: mean {mean_it:.0f}, min {min_it}, max {max_it} of at most {worst_it}
(levels: {levels}).

1. ssn_tvl1_iterate advancing up to {halo} iterations per launch on LDS-resident tiles ({launches_tiled} launches enqueued per batch):
     median {t_tiled:.4f} s = {pps_tiled:.1f} pairs/s        (all calls: {all_tiled})
2. the same kernel limited to one iteration per launch ({launches_single} launches enqueued per batch) -- the baseline:
     median {t_single:.4f} s = {pps_single:.1f} pairs/s        (all calls: {all_single})
   ratio 2 / 1: {ratio:.2f} x
   outputs of 1 and 2 bit-equal: {equal}

Nothing here is a pass/fail condition.
To repeat: timeout -k 10 540 python tools/bench_flow.py --out profiles/flow_measured.txt
""".format(**r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--pair-batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import action_detection_amd as pkg
    from action_detection_amd import kernels as K
    from action_detection_amd.optical_flow import TVL1, FlowExtractor, rgb_to_gray
    assert torch.cuda.is_available(), "bench_flow.py measures on the GPU; there is nothing to measure without one"
    pkg.build()
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(synthetic_clip(a.pairs + 1, a.height, a.width, seed=0)).to(dev)
    halo = K.tvl1_tile_shape()[2]
    tiled = FlowExtractor(TVL1(), pair_batch=a.pair_batch)
    single = FlowExtractor(TVL1(iterations_per_launch=1), pair_batch=a.pair_batch)

    def timed(ex):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ex.extract(frames)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    _, out_tiled = timed(tiled)
    _, out_single = timed(single)
    t_tiled, t_single = [], []
    for _ in range(a.iters):
        t_tiled.append(timed(tiled)[0])
        t_single.append(timed(single)[0])
    gray = rgb_to_gray(frames)
    res = tiled.tvl1(gray[:a.pair_batch], gray[1:a.pair_batch + 1])
    per_pair = res.iterations.sum(dim=(0, 1)).cpu().numpy()
    levels, warps = res.iterations.shape[:2]
    med = lambda ts: float(np.median(ts))
    r = {"what": "TV-L1 flow extraction on one MI355X", "device": torch.cuda.get_device_name(0), "host": socket.gethostname(),
         "commit": commit_name(), "iters": a.iters, "pairs": a.pairs, "pair_batch": a.pair_batch, "h": a.height, "w": a.width,
         "halo": halo, "levels": levels, "mean_it": float(per_pair.mean()), "min_it": int(per_pair.min()), "max_it": int(per_pair.max()),
         "worst_it": levels * warps * tiled.tvl1.iterations,
         "launches_tiled": levels * warps * len(tiled.tvl1.launch_plan()), "launches_single": levels * warps * len(single.tvl1.launch_plan()),
         "t_tiled": med(t_tiled), "t_single": med(t_single), "pps_tiled": a.pairs / med(t_tiled), "pps_single": a.pairs / med(t_single),
         "all_tiled": [round(t, 4) for t in t_tiled], "all_single": [round(t, 4) for t in t_single],
         "ratio": med(t_single) / med(t_tiled), "equal": bool(torch.equal(out_tiled, out_single))}
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report(r))


if __name__ == "__main__":
    main()
