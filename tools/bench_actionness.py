#!/usr/bin/env python
"""The actionness scoring stage on one MI355X (actionness_test.ActionnessTester, csrc/actionness.hip,
tag_proposals.merge_scores_device): one JSON line, and with --out the text of profiles/actionness_measured.txt.

    timeout -k 10 540 python tools/bench_actionness.py [--ticks 1000] [--videos 200] [--iters 5] [--out profiles/actionness_measured.txt]

Three measurements, all on seeded synthetic data:
  * tester: frames/s of ActionnessTester.score_video on a video of --ticks ticks (BN-Inception, RGB, 10 crops, 224 x 224,
    tick_batch 32, synthetic weights), frame batches resident on the device; host clock around a call that ends in a
    device synchronise, median over --iters calls after a warm-up call.
  * tail: the scoring tail of that video -- ssn_actionness_fc per backbone call + ssn_actionness_group -- on stored
    features, next to the same tail written with what the library had before (HipLinear + torch view / index / mean),
    alternating, device events around each whole tail, medians; the outputs are compared.
  * merge: merge_scores_device on --videos videos x 2 streams resident on the device, against the host merge_scores with
    the transfers it needs when the scores live on the device (download both streams, upload the result), alternating.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def median_ms(samples):
    return round(float(np.median(samples)), 4)


def bench_tester(torch, net, ticks, iters, tick_batch=32, crops=10, size=224):
    from action_detection_amd.actionness_test import ActionnessTester
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    # 4 ticks per source batch as the reference's generator; the same 8 batches are cycled (the frames are not the subject)
    pool = [(torch.randint(0, 256, (crops * 4 * 3, size, size), generator=g).float() - 110.0).to(dev) for _ in range(8)]

    def source():
        for i in range(ticks // 4):
            yield pool[i % len(pool)]
        if ticks % 4:
            yield pool[0].reshape(crops, 4, 3, size, size)[:, :ticks % 4].reshape(-1, size, size)
    tester = ActionnessTester(net, tick_batch=tick_batch)
    tester.score_video(source(), ticks, num_crop=crops)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        tester.score_video(source(), ticks, num_crop=crops)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    med = float(np.median(times))
    return {"ticks": ticks, "crops": crops, "tick_batch": tick_batch, "frames": ticks * crops,
            "seconds_median": round(med, 4), "seconds_all": [round(t, 4) for t in times],
            "frames_per_s": round(ticks * crops / med, 1), "repeated_calls": tester.repeated_calls}


def bench_tail(torch, net, ticks, iters, tick_batch=32, crops=10):
    from action_detection_amd import kernels as K
    dev = torch.device("cuda:0")
    fc = net.test_fc
    w, b = fc.weight.detach().contiguous(), fc.bias.detach().contiguous()
    d, c = w.shape[1], w.shape[0]
    g = torch.Generator().manual_seed(2)
    calls = [(t0, min(tick_batch, ticks - t0)) for t0 in range(0, ticks, tick_batch)]
    feats = [torch.rand((crops * n, d), generator=g).to(dev) for _, n in calls]
    # the reference grouping as a gather of the true layout (what a torch tail needs; built once, outside the timing)
    i = np.arange(ticks)[:, None]
    j = np.arange(crops)[None, :]
    q = i // 4
    bsz = np.minimum(4, ticks - 4 * q)
    r = (i - 4 * q) * crops + j
    gather = torch.from_numpy(((4 * q + r % bsz) * crops + r // bsz).ravel().astype(np.int64)).to(dev)

    def new_tail():
        raw_true = torch.empty((ticks, crops, c), device=dev)
        for (t0, _), f in zip(calls, feats):
            K.actionness_fc(f, w, b, raw_true, t0, crops)
        return K.actionness_group(raw_true, 4)

    def old_tail():
        raw_true = torch.empty((ticks, crops, c), device=dev)
        for (t0, n), f in zip(calls, feats):
            raw_true[t0:t0 + n] = fc(f).view(crops, n, c).transpose(0, 1)
        raw = raw_true.view(-1, c).index_select(0, gather).view(ticks, crops, c)
        return raw, raw.mean(dim=1)
    with torch.no_grad():
        a, b_ = new_tail(), old_tail()
        torch.cuda.synchronize()
        same_rows = bool(torch.equal(a[0], b_[0]))
        max_diff = float((a[0] - b_[0]).abs().max())
        mean_diff = float((a[1] - b_[1]).abs().max())
        t_new, t_old = [], []
        for _ in range(iters + 1):
            for fn, acc in ((new_tail, t_new), (old_tail, t_old)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                acc.append(e0.elapsed_time(e1))
    return {"ticks": ticks, "backbone_calls": len(calls), "feature_dim": d,
            "fc_group_ms_median": median_ms(t_new[1:]), "fc_group_ms_all": [round(t, 4) for t in t_new[1:]],
            "hiplinear_torch_ms_median": median_ms(t_old[1:]), "hiplinear_torch_ms_all": [round(t, 4) for t in t_old[1:]],
            "launches_new": len(calls) + 1, "rows_bit_equal": same_rows, "max_abs_diff_raw": max_diff,
            "max_abs_diff_mean": mean_diff}


def bench_merge(torch, videos, iters):
    from action_detection_amd.tag_proposals import merge_scores, merge_scores_device
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(3)
    streams = [{}, {}]
    for v in range(videos):
        t = int(rs.randint(100, 4001))
        t2 = max(1, t + int(rs.randint(-5, 6)))
        streams[0]["v%d" % v] = torch.from_numpy(rs.standard_normal((t, 2)).astype(np.float32)).to(dev)
        streams[1]["v%d" % v] = torch.from_numpy(rs.standard_normal((t2, 2)).astype(np.float32)).to(dev)
    weights = [1.0, 1.5]

    def device_path():
        return merge_scores_device(streams, weights)

    def host_path():
        files = [{k: v.cpu().numpy()[:, None, :] for k, v in s.items()} for s in streams]      # (one crop: the mean is the row)
        return {k: torch.from_numpy(v).to(dev) for k, v in merge_scores(files, weights).items()}
    a, b = device_path(), host_path()
    torch.cuda.synchronize()
    equal = all(torch.equal(a[k], b[k]) for k in a)
    t_dev, t_host = [], []
    for _ in range(iters + 1):
        for fn, acc in ((device_path, t_dev), (host_path, t_host)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
    return {"videos": videos, "streams": 2, "rows": int(sum(v.shape[0] for s in streams for v in s.values())),
            "device_ms_median": median_ms(t_dev[1:]), "device_ms_all": [round(t, 3) for t in t_dev[1:]],
            "host_with_transfers_ms_median": median_ms(t_host[1:]), "host_ms_all": [round(t, 3) for t in t_host[1:]],
            "bit_equal": equal}


def commit_name():
    if os.environ.get("BENCH_COMMIT"):
        return os.environ["BENCH_COMMIT"]
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain"], stderr=subprocess.DEVNULL).decode().strip()
        return head + (" + the working tree of this change" if dirty else "")
    except Exception:
        return "unknown (no git metadata where this ran; set BENCH_COMMIT)"


def report(res):
    t, tl, m = res["tester"], res["tail"], res["merge"]
    return """Actionness scoring stage: tools/bench_actionness.py on one MI355X, commit measured: {commit}.
Method: warm-up call first, then {iters} timed repetitions, medians; whole calls with a host clock around work that ends in a
device synchronise, the scoring tail with device events; the two versions of a comparison alternate inside one process; seeded
synthetic inputs at the sizes of a real run; outputs of old and new compared on the same inputs.  No profiler attached.

1. ActionnessTester.score_video, BN-Inception, RGB, {crops} crops, 224 x 224, tick_batch {tb}, one video of {ticks} ticks
   ({frames} frames, batches of 4 ticks resident on the device, synthetic weights):
     median {sec} s = {fps} frames/s        (all calls: {sec_all}; backbone calls repeated by the range guard: {rep})

2. The scoring tail of that video on stored features [{rows_per_call} x {d}] per backbone call, {calls} calls:
     ssn_actionness_fc x {calls} + ssn_actionness_group x 1   median {new} ms   ({new_all})
     HipLinear + torch view / copy / index_select / mean    median {old} ms   ({old_all})
   rows bit-equal between the two: {same}; max |difference| raw {dr:.3g}, mean {dm:.3g} (HipLinear sums in another order;
   torch's mean is not numpy's sequential sum).  Both include the allocation of the staging tensor.
   The tail is {share:.2f} % of the video's time in 1.

3. merge_scores_device, {videos} videos x 2 streams ({rows} rows of 2 scores, lengths 100 ... 4000, second stream up to 5 rows
   shorter or longer), scores resident on the device:
     one ssn_actionness_merge launch (host: offsets, one concatenation)          median {dev} ms   ({dev_all})
     host merge_scores with the transfers it needs (2 downloads per video, upload)  median {host} ms   ({host_all})
   results bit-equal: {eq}

Not gated: the backbone dominates the stage.
To repeat: timeout -k 10 540 python tools/bench_actionness.py --out profiles/actionness_measured.txt
""".format(commit=res["commit"], iters=res["iters"], crops=t["crops"], tb=t["tick_batch"], ticks=t["ticks"], frames=t["frames"],
           sec=t["seconds_median"], fps=t["frames_per_s"], sec_all=t["seconds_all"], rep=t["repeated_calls"],
           rows_per_call=t["crops"] * t["tick_batch"], d=tl["feature_dim"], calls=tl["backbone_calls"],
           new=tl["fc_group_ms_median"], new_all=tl["fc_group_ms_all"], old=tl["hiplinear_torch_ms_median"],
           old_all=tl["hiplinear_torch_ms_all"], same=tl["rows_bit_equal"], dr=tl["max_abs_diff_raw"], dm=tl["max_abs_diff_mean"],
           share=100.0 * tl["fc_group_ms_median"] / (1e3 * t["seconds_median"]), videos=m["videos"], rows=m["rows"],
           dev=m["device_ms_median"], dev_all=m["device_ms_all"], host=m["host_with_transfers_ms_median"], host_all=m["host_ms_all"],
           eq=m["bit_equal"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--videos", type=int, default=200)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    import action_detection_amd as pkg
    from action_detection_amd.binary_model import BinaryClassifier
    from action_detection_amd.synthetic import init_backbone_synthetic
    pkg.build()
    assert torch.cuda.is_available(), "bench_actionness.py measures on the GPU; there is no CPU fallback"
    torch.manual_seed(0)
    net = BinaryClassifier(2, 5, "RGB", base_model="BNInception", test_mode=True)
    init_backbone_synthetic(net.base_model)
    with torch.no_grad():
        net.classifier_fc.weight.normal_(0, 0.05)
    net.prepare_test_fc()
    net.to("cuda:0").eval()
    res = {"what": "actionness scoring stage on one MI355X", "commit": commit_name(), "iters": a.iters,
           "tester": bench_tester(torch, net, a.ticks, a.iters), "tail": bench_tail(torch, net, a.ticks, a.iters),
           "merge": bench_merge(torch, a.videos, a.iters)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
