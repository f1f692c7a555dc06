#!/usr/bin/env python
"""AR-AN (proposal_eval.proposal_ar_an) on two synthetic subsets, against the only other thing that computes it: the numpy
referee of tests/proposal_eval_referee.py on the host (the toolkit's loops over videos, thresholds and curve points).

  activitynet   2383 videos x ~100 proposals x 1-2 ground truths      (the ActivityNet-1.2 validation set's shape)
  thumos14      210 videos x ~1000 proposals x ~15 ground truths      (the THUMOS14 test set's shape)

    python tools/bench_proposal_eval.py [--repeats 7] [--out profiles/proposal_eval_measured.txt]

Proposals are ground-truth spans jittered at random plus uniform spans, with random scores and in score order; 10 tIoU
thresholds, 100 curve points, the default truncation.  Timed: lists in to result out (`proposal_ar_an`, which packs, uploads,
launches and downloads), the same with `scores` (the device ranks), the launches and the download alone on a resident
ProposalBatch (`proposal_ar_an_batch`), and the referee.  The paths alternate inside every repeat; medians with
[min .. max]; host clock around calls that end in a device-to-host copy.  The results of the paths are compared at the
tests' bars.  Needs the GPU: there is no CPU fallback.
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

SETS = {"activitynet": dict(videos=2383, proposals=100, gt=(1, 2), duration=120.0),
        "thumos14": dict(videos=210, proposals=1000, gt=(10, 20), duration=220.0)}


def make_set(videos, proposals, gt, duration, seed):
    rs = np.random.RandomState(seed)
    pr, gts, scores = [], [], []
    for _ in range(videos):
        n = int(rs.randint(gt[0], gt[1] + 1))
        m = int(max(1, round(proposals * rs.uniform(0.5, 1.5))))
        s = rs.uniform(0, duration * 0.9, n)
        g = np.stack([s, np.minimum(duration, s + rs.uniform(1.0, duration * 0.3, n))], axis=1)
        near = g[rs.randint(0, n, m // 2)] + rs.normal(0, duration * 0.03, (m // 2, 2))
        a = rs.uniform(0, duration, (m - m // 2, 2))
        p = np.concatenate([near, a])
        p = np.stack([p.min(axis=1), p.max(axis=1) + 0.01], axis=1)
        sc = rs.uniform(0, 1, m)
        o = np.argsort(-sc, kind="stable")
        pr.append(p[o])
        scores.append(sc[o])
        gts.append(g)
    return pr, gts, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sets", nargs="+", default=list(SETS), choices=list(SETS))
    ap.add_argument("--scale", type=float, default=1.0, help="scale the number of videos (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposal_eval_measured.txt"))
    a = ap.parse_args()

    import torch
    import action_detection_amd as pkg
    from action_detection_amd import _lib
    from action_detection_amd.proposal_eval import proposal_ar_an, proposal_ar_an_batch
    from action_detection_amd.proposal_lists import ProposalListBuilder
    import proposal_eval_referee as referee
    pkg.build()
    if _lib.emulator_active():          # (a rehearsal of the script through the tests' host emulator; its times mean nothing)
        dev = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench_proposal_eval.py measures on the GPU; there is no CPU fallback"
        dev = torch.device("cuda:0")

    def stat(x):
        x = np.asarray(x) * 1e3
        return "%9.2f [%8.2f .. %8.2f]" % (np.median(x), x.min(), x.max())

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    lines = ["AR-AN, device pass and numpy referee, %s, torch %s" % (
        torch.cuda.get_device_name(0) if dev.type == "cuda" else "HOST EMULATOR (rehearsal)", torch.__version__),
        "10 tIoU thresholds, 100 curve points, default truncation; the paths alternate inside each of %d repeats after one "
        "warm-up each; host clock, ms, median [min .. max]" % a.repeats]
    agree = True
    for name in a.sets:
        cfg = dict(SETS[name])
        cfg["videos"] = max(1, int(round(cfg["videos"] * a.scale)))
        pr, gts, scores = make_set(seed=a.seed, **cfg)
        rs = np.random.RandomState(a.seed + 1)
        perm = [rs.permutation(len(p)) for p in pr]
        pr_shuffled, sc_shuffled = [p[o] for p, o in zip(pr, perm)], [s[o] for s, o in zip(scores, perm)]
        vids = [SimpleNamespace(id=str(i), duration=cfg["duration"]) for i in range(len(pr))]
        batch = ProposalListBuilder(device=dev).from_spans(vids, pr)
        paths = [("lists in, result out (proposal_ar_an)", lambda: proposal_ar_an(pr, gts, device=dev)),
                 ("the same with scores, shuffled input", lambda: proposal_ar_an(pr_shuffled, gts, scores=sc_shuffled, device=dev)),
                 ("resident batch (proposal_ar_an_batch)", lambda: proposal_ar_an_batch(batch, gt=gts)),
                 ("numpy referee on the host", lambda: referee.ar_an(pr, gts))]
        first = [fn() for _, fn in paths]          # warm-up of all: code objects, allocator
        ref = first[3]
        for r in first[:3]:
            ok = (np.array_equal(r.first_hit, ref["first_hit"]) and np.array_equal(r.matches, ref["matches"])
                  and np.array_equal(r.recall, ref["recall"]) and np.array_equal(r.proposals_per_video, ref["proposals_per_video"])
                  and np.allclose(r.avg_recall, ref["avg_recall"], rtol=1e-12, atol=0) and abs(r.auc - ref["auc"]) <= 1e-12 * ref["auc"])
            agree = agree and ok
        times = [[] for _ in paths]
        for _ in range(a.repeats):
            for k, (_, fn) in enumerate(paths):
                times[k].append(timed(fn)[1])
        lines += ["", "%s-like: %d videos, %d proposals (%d after the truncation), %d ground-truth spans; AUC %.4f, AR@last %.4f"
                  % (name, len(pr), sum(len(p) for p in pr), ref["total_proposals"], ref["positives"], ref["auc"],
                     ref["avg_recall"][-1])]
        for (label, _), t in zip(paths, times):
            lines.append("  %-40s %s" % (label, stat(t)))
        med = [np.median(t) for t in times]
        lines.append("  referee / lists-in: %.1f x; referee / resident batch: %.1f x" % (med[3] / med[0], med[3] / med[2]))
    lines += ["", "device results equal to the referee's at the tests' bars on every set: %s" % agree]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert agree, "the device pass and the referee disagree"


if __name__ == "__main__":
    main()
