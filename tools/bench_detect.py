#!/usr/bin/env python
"""The test table against the host path it replaces, and the dense tester with and without the per-proposal host work.

  table    detect.build_test_table (host frame numbers in, table on the device, synchronised) against VideoRecord +
           ProposalSampler.test_ticks + STPPReorgainzed.host_ranges for the same records, on a THUMOS14-like batch (213 videos of
           about 1000 proposals) and an ActivityNet-like one (2383 videos of about 50)
  tester   detect.score_video_ranges (rows of the table) against DenseTester.score_video (proposal ticks from the host) for one
           video of 900 ticks and about 1000 proposals (948 with the fixed seed) on synthetic frames that are resident on the device (BNInception, RGB, 1 crop)

    python tools/bench_detect.py [--repeats 7] [--out profiles/detect_measured.txt]

The two sides alternate inside every repeat after one warm-up each; host clock around calls that end synchronised; medians with
[min .. max].  The results of the two sides are compared.  Needs the GPU: there is no CPU fallback.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def make_batch(n_videos, mean_props, frames_lo, frames_hi, seed):
    """-> (records in load_proposal_file's layout, frame counts, one int [n, 2] array per video); about 3 % of the rows are ones a
    record drops, a few end past the last frame."""
    rs = np.random.RandomState(seed)
    fcs = rs.randint(frames_lo, frames_hi, size=n_videos)
    props = []
    for fc in fcs:
        n = max(1, int(mean_props * rs.uniform(0.6, 1.4)))
        s = rs.randint(0, fc - 1, size=n)
        e = np.minimum(s + rs.randint(1, max(2, fc // 3), size=n), fc + 20)
        bad = rs.rand(n) < 0.03
        e[bad] = s[bad]
        props.append(np.stack([s, e], axis=1))
    records = [("v%d" % i, str(fc), [], [["0", "0.0", "0.0", str(a), str(b)] for a, b in p.tolist()])
               for i, (fc, p) in enumerate(zip(fcs, props))]
    return records, fcs, props


def stat(x):
    x = np.asarray(x) * 1e3
    return "%9.2f [%8.2f .. %8.2f]" % (np.median(x), x.min(), x.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_measured.txt"))
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--videos-scale", type=float, default=1.0, help="fraction of the videos of either batch (rehearsals)")
    a = ap.parse_args()

    import torch
    import action_detection_amd as pkg
    from action_detection_amd import _lib
    from action_detection_amd.detect import build_test_table, score_video_ranges
    from action_detection_amd.ops.ssn_ops import STPPReorgainzed
    from action_detection_amd.proposal_sampling import ProposalSampler, VideoRecord
    pkg.build()
    if _lib.emulator_active():          # (a rehearsal of the script through the tests' host emulator; its times mean nothing)
        dev = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench_detect.py measures on the GPU; there is no CPU fallback"
        dev = torch.device("cuda:0")

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    name = torch.cuda.get_device_name(0) if dev.type == "cuda" else "HOST EMULATOR (rehearsal)"
    lines = ["The test table and the dense tester's proposal path, %s, torch %s" % (name, torch.__version__),
             "the two sides alternate inside each of %d repeats after one warm-up each; host clock, ms, median [min .. max]" % a.repeats, ""]
    sampler = ProposalSampler(records=[], reg_stats=np.zeros((2, 2)), new_length=1, test_interval=6)
    all_equal = True
    for title, shape in (("THUMOS14-like", (213, 1000, 3000, 8000, 0)), ("ActivityNet-like", (2383, 50, 1500, 6000, 1))):
        records, fcs, props = make_batch(max(41, int(shape[0] * a.videos_scale)), *shape[1:])
        frames = np.concatenate(props).astype(np.int32)
        p_off = np.concatenate([[0], np.cumsum([len(p) for p in props])])
        for cfg in ((1, 1, 1), (1, (1, 2), 1)):
            reorg = STPPReorgainzed(10, 2, 1, 2, True, stpp_cfg=cfg)

            def host():
                t = [time.perf_counter()]
                videos = [VideoRecord(r) for r in records]
                t.append(time.perf_counter())
                ticks = [sampler.test_ticks(v) for v in videos]
                t.append(time.perf_counter())
                ranges = [reorg.host_ranges(tk[2], len(tk[0])) for tk in ticks]
                t.append(time.perf_counter())
                return (ticks, ranges), np.diff(t)

            def device():
                t0 = time.perf_counter()
                table = build_test_table(frames, p_off, fcs, 1, 6, cfg, device=dev)
                sync()
                return table, time.perf_counter() - t0

            (ticks, ranges), _ = host()
            table, _ = device()
            equal = True
            for i in range(len(records)):
                rows = table.video(i)
                n = len(ticks[i][0])
                rg, act = ranges[i][0].copy(), ranges[i][1].copy()      # + the clamps of STPPReorgainzed.forward (no -1 rows arise here)
                np.minimum(rg[..., 1], n, out=rg[..., 1])
                np.minimum(act[:, 1], n, out=act[:, 1])
                equal &= np.array_equal(rows.rel.cpu().numpy(), ticks[i][1]) and np.array_equal(rows.ticks.cpu().numpy(), ticks[i][2]) \
                    and np.array_equal(rows.scaling.cpu().numpy(), ticks[i][3]) and np.array_equal(rows.ranges.cpu().numpy(), rg) \
                    and np.array_equal(rows.act.cpu().numpy(), act)
                if i >= 40:
                    break
            all_equal &= bool(equal)
            th, td = [], []
            for _ in range(a.repeats):
                th.append(host()[1])
                td.append(device()[1])
            th = np.asarray(th)
            lines += ["%s: %d videos, %d proposals, %d rows kept, stpp_cfg %r; first 41 videos equal: %s"
                      % (title, len(records), len(frames), int(table.h_k_off[-1]), cfg, equal),
                      "  host  VideoRecord                  %s" % stat(th[:, 0]),
                      "        test_ticks                   %s" % stat(th[:, 1]),
                      "        host_ranges                  %s" % stat(th[:, 2]),
                      "        total                        %s" % stat(th.sum(axis=1)),
                      "  build_test_table (upload .. sync)  %s" % stat(td),
                      "  host / table, medians: %.0f x" % (np.median(th.sum(axis=1)) / np.median(td)), ""]

    if not a.skip_tester and dev.type == "cuda":
        from action_detection_amd.dense_test import DenseTester
        from action_detection_amd.ssn_models import SSN
        from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic
        torch.manual_seed(0)
        net = SSN(20, 2, 5, 2, "RGB", test_mode=True, stpp_cfg=(1, 1, 1))
        init_backbone_synthetic(net.base_model)
        init_heads_synthetic(net, std=0.05)
        net.prepare_test_fc()
        net.to(dev).eval()
        tester = DenseTester(net, 20, stats=np.array([[0.1, -0.3], [1.5, 0.7]]), tick_batch=128)
        fc, n_ticks = 5401, 900
        records, _, props = make_batch(1, 1000, fc, fc + 1, 2)
        video = VideoRecord(records[0])
        _, rel, pticks, scaling = sampler.test_ticks(video)
        assert len(np.arange(0, fc - 1, 6)) == n_ticks
        table = build_test_table(props[0], np.array([0, len(props[0])]), np.array([fc]), 1, 6, (1, 1, 1), device=dev)
        rows = table.video(0)
        resident = torch.randn(128, 3, 224, 224, device=dev)

        def gen():
            for b in range(0, n_ticks, 128):
                yield resident[:min(128, n_ticks - b)]

        def via_host():
            t0 = time.perf_counter()
            out = tester.score_video(gen(), n_ticks, torch.from_numpy(pticks), torch.from_numpy(scaling), num_crop=1)
            sync()
            return out, time.perf_counter() - t0

        def via_table():
            t0 = time.perf_counter()
            out = score_video_ranges(tester, gen(), n_ticks, rows.ranges, rows.act, rows.scaling, num_crop=1)
            sync()
            return out, time.perf_counter() - t0

        for _ in range(2):                                  # (the first calls calibrate the backbone's scales)
            ref, _ = via_host()
            got, _ = via_table()
        equal = all(torch.equal(x, y) for x, y in zip(ref[:3], got[:3]))
        all_equal &= equal
        t_host, t_table = [], []
        for _ in range(a.repeats):
            t_host.append(via_host()[1])
            t_table.append(via_table()[1])
        lines += ["dense tester, one video of %d ticks and %d proposals (%d rows), BNInception RGB, 1 crop, tick_batch 128, resident frames; "
                  "outputs equal: %s" % (n_ticks, len(props[0]), len(pticks), equal),
                  "  score_video (proposal ticks from the host)   %s" % stat(t_host),
                  "  score_video_ranges (rows of the table)       %s" % stat(t_table),
                  "  difference of the medians: %.2f ms" % ((np.median(t_host) - np.median(t_table)) * 1e3), ""]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    assert all_equal, "the two sides disagree"


if __name__ == "__main__":
    main()
