#!/usr/bin/env python
"""The proposal-list stage on a synthetic subset shaped like the THUMOS14 test set, three ways in one process:

  per video   what the tree offered before proposal_lists.py: per video tag_proposals.sliding_window_proposals (host
              tuples), name_proposals (one upload, one launch, one download each), proposal_io.format_window_list_record;
              detection_eval.proposal_recall once over all videos
  batched     ProposalListBuilder.sliding_windows + build (a constant number of launches and copies), then
              proposal_io.format_window_list_rows per video
  device text ProposalListBuilder.sliding_windows + build_text: the bytes of the file formed on the device
              (csrc/proposal_text.hip), one download of text, hits and status

    python tools/bench_proposal_lists.py [--videos 210] [--repeats 7] [--out profiles/proposal_lists_measured.txt]

The subset is written to a temporary folder in the THUMOS14 layout (durations, class files, avoid files, frame folders of
empty files) and read back through datasets.ThumosDB, so both paths start from the same records and frame counts; that
reading is timed once and reported on its own.  Durations are log-uniform over the range of the annotated THUMOS14 videos
(8.932 ... 1673.428 s), instance counts 1 ... 73 growing with the duration, overlap 0.7.  The three paths alternate inside
every repeat; medians with [min .. max]; host clock around calls that end in device-to-host copies.  The texts of the
three paths are compared (under the '# <index>' lines write_proposal_file adds).  After the repeats one more device-text
pass times its three text launches with device events.  Needs the GPU: there is no CPU fallback.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CLASSES = ["Ambiguous", "BaseballPitch", "BasketballDunk", "Billiards", "CleanAndJerk", "CliffDiving", "CricketBowling",
           "CricketShot", "Diving", "FrisbeeCatch", "GolfSwing", "HammerThrow", "HighJump", "JavelinThrow", "LongJump",
           "PoleVault", "Shotput", "SoccerPenalty", "TennisSwing", "ThrowDiscus", "VolleyballSpiking"]


def write_subset(folder, n, seed):
    """n annotated test videos (and a token validation subset) in the THUMOS14 layout + frame folders; -> frame path"""
    rs = np.random.RandomState(seed)
    durations = np.round(np.exp(rs.uniform(np.log(8.932), np.log(1673.428), n)), 3)
    rows = {c: [] for c in CLASSES}
    for i, d in enumerate(durations):
        k = int(min(73, max(1, round(d / 23.0 * rs.uniform(0.3, 1.7)))))
        cls = CLASSES[1 + int(rs.randint(0, 20))]
        starts = np.sort(rs.uniform(0, d * 0.95, k))
        for s in starts:
            e = min(d, s + rs.uniform(0.5, 12.0))
            rows[cls].append("video_test_%07d %.1f %.1f\n" % (i, s, e))
    ann = os.path.join(folder, "annotations")
    for subset, tag in (("test", "test"), ("validation", "val")):
        os.makedirs(os.path.join(ann, "temporal_annotations_%s" % subset))
        for c in CLASSES:
            with open(os.path.join(ann, "temporal_annotations_%s" % subset, "%s_%s.txt" % (c, tag)), "w") as f:
                f.write("".join(rows[c]) if subset == "test" else "")
        with open(os.path.join(ann, "%s_avoid_videos.txt" % subset), "w") as f:
            f.write("")
        with open(os.path.join(ann, "%s_durations.txt" % subset), "w") as f:
            if subset == "test":
                f.write("".join("video_test_%07d.mp4\n%.3f\n" % (i, d) for i, d in enumerate(durations)))
    frames = os.path.join(folder, "frames")
    for i, d in enumerate(durations):
        os.makedirs(os.path.join(frames, "video_test_%07d" % i))
        for f in range(int(d / 4) + 1):
            open(os.path.join(frames, "video_test_%07d" % i, "img_%05d.jpg" % (f + 1)), "w").close()
    return ann, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=210)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--overlap", type=float, default=0.7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposal_lists_measured.txt"))
    a = ap.parse_args()

    import glob
    import torch
    import action_detection_amd as pkg
    from action_detection_amd import _lib
    from action_detection_amd.datasets import ThumosDB
    from action_detection_amd.detection_eval import proposal_recall
    from action_detection_amd.proposal_io import format_window_list_record, format_window_list_rows
    from action_detection_amd.proposal_lists import ProposalListBuilder
    from action_detection_amd.tag_proposals import name_proposals, sliding_window_proposals
    pkg.build()
    if _lib.emulator_active():          # (a rehearsal of the script through the tests' host emulator; its times mean nothing)
        dev = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench_proposal_lists.py measures on the GPU; there is no CPU fallback"
        dev = torch.device("cuda:0")
    thresholds = [0.5, 0.7, 0.9]

    tmp = tempfile.mkdtemp()
    try:
        ann, frame_path = write_subset(tmp, a.videos, a.seed)
        t0 = time.perf_counter()
        db = ThumosDB.from_folder(ann)
        db.try_load_file_path(frame_path)
        videos = db.get_subset_videos("test")
        paths = [os.path.join(frame_path, v.path.split("/")[-1].split(".")[0]) for v in videos]
        counts = [len(glob.glob(os.path.join(p, "img_*.jpg"))) for p in paths]
        t_read = time.perf_counter() - t0
    finally:
        shutil.rmtree(tmp)
    gts = [[(i.num_label, i.time_span) for i in v.instances] for v in videos]
    builder = ProposalListBuilder(device=dev)

    def per_video():
        t = [time.perf_counter()]
        props = [sliding_window_proposals(v.duration, overlap=a.overlap) for v in videos]
        t.append(time.perf_counter())
        named = [name_proposals([g], [p], device=dev)[0] for g, p in zip(gts, props)]
        t.append(time.perf_counter())
        recall = proposal_recall(props, [[s for _, s in g] for g in gts], thresholds, device=dev)
        t.append(time.perf_counter())
        text = [format_window_list_record(p, c, v.duration, g, n) for p, c, v, g, n in zip(paths, counts, videos, gts, named)]
        t.append(time.perf_counter())
        return text, list(zip(recall.per_video_recall, recall.per_inst_recall)), np.diff(t)

    def batched():
        t = [time.perf_counter()]
        batch = builder.sliding_windows(videos, overlap=a.overlap)
        t.append(time.perf_counter())
        result = builder.build(batch, counts, recall_thresholds=thresholds)      # (ends in the one download)
        t.append(time.perf_counter())
        text = [format_window_list_rows(p, c, *result.rows(i)) for i, (p, c) in enumerate(zip(paths, counts))]
        t.append(time.perf_counter())
        return text, result.recall, np.diff(t), result.num_proposals

    def device_text():
        t = [time.perf_counter()]
        batch = builder.sliding_windows(videos, overlap=a.overlap)
        t.append(time.perf_counter())
        result = builder.build_text(batch, counts, paths, recall_thresholds=thresholds)      # (ends in the one large download)
        t.append(time.perf_counter())
        return result, result.recall, np.diff(t)

    text_a, recall_a, _ = per_video()                     # warm-up of all three: code objects, allocator
    text_b, recall_b, _, windows = batched()
    res_c, recall_c, _ = device_text()
    whole = "".join("# %d\n%s" % (i + 1, x) for i, x in enumerate(text_b)).encode("utf-8")
    equal = text_a == text_b and np.array_equal(np.asarray(recall_a), np.asarray(recall_b)) and res_c.data == whole \
        and np.array_equal(np.asarray(recall_b), np.asarray(recall_c)) and res_c.host_formatted == 0
    ta, tb, tc = [], [], []
    for _ in range(a.repeats):
        ta.append(per_video()[2])
        tb.append(batched()[2])
        tc.append(device_text()[2])
    ta, tb, tc = np.asarray(ta) * 1e3, np.asarray(tb) * 1e3, np.asarray(tc) * 1e3

    # one more device-text pass with device events around the two text entries (size: two launches, fill: one)
    from action_detection_amd import kernels as K
    launches = {}

    def timed(name, fn):
        def call(*args, **kwargs):
            if dev.type != "cuda":
                return fn(*args, **kwargs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kwargs)
            e1.record()
            launches[name] = (e0, e1)
            return out
        return call

    size_fn, fill_fn = K.proposal_text_size, K.proposal_text_fill
    K.proposal_text_size, K.proposal_text_fill = timed("size", size_fn), timed("fill", fill_fn)
    try:
        device_text()
    finally:
        K.proposal_text_size, K.proposal_text_fill = size_fn, fill_fn
    if dev.type == "cuda":
        torch.cuda.synchronize()
    dev_ms = {k: e0.elapsed_time(e1) for k, (e0, e1) in launches.items()}
    n_v, n_t, n_g = len(videos), len(thresholds), sum(len(g) for g in gts)
    down_b = windows * (8 + 8 + 4 + 8) + n_g * 8 + n_v * 4 + n_v * n_t * 4
    down_c = len(res_c.data) + 4 * (n_v + 1) + n_v * 4 + n_v * n_t * 4 + 4

    def stat(x):
        return "%9.1f [%8.1f .. %8.1f]" % (np.median(x), x.min(), x.max())

    tot_a, tot_b, tot_c = ta.sum(axis=1), tb.sum(axis=1), tc.sum(axis=1)
    gain = np.median(tot_b) - np.median(tot_c)
    spreads = (tot_b.max() - tot_b.min()) + (tot_c.max() - tot_c.min())
    lines = [
        "The proposal-list stage, per video, batched and batched with device text, %s, torch %s" % (torch.cuda.get_device_name(0) if dev.type == "cuda" else "HOST EMULATOR (rehearsal)", torch.__version__),
        "%d synthetic videos shaped like the THUMOS14 test set (seed %d): durations %.1f .. %.1f s, %d instances, overlap %g, "
        "%d windows, %d characters of list text" % (len(videos), a.seed, min(v.duration for v in videos),
                                                     max(v.duration for v in videos), sum(len(g) for g in gts), a.overlap,
                                                     windows, sum(len(x) for x in text_b)),
        "records and frame counts in, list text out; the three paths alternate inside each of %d repeats after one warm-up "
        "each; host clock, ms, median [min .. max]" % a.repeats,
        "texts and recall of the three paths equal: %s" % equal,
        "",
        "reading the annotations and counting the frame files (datasets.ThumosDB + glob; once, before both): %.1f ms" % (t_read * 1e3),
        "",
        "per video (sliding_window_proposals + name_proposals per video, proposal_recall once, format_window_list_record)",
        "  windows on the host            %s" % stat(ta[:, 0]),
        "  naming, one call per video     %s" % stat(ta[:, 1]),
        "  recall, one call               %s" % stat(ta[:, 2]),
        "  text                           %s" % stat(ta[:, 3]),
        "  total                          %s" % stat(tot_a),
        "batched (ProposalListBuilder + format_window_list_rows)",
        "  windows: count, read, fill     %s" % stat(tb[:, 0]),
        "  build: upload .. download      %s" % stat(tb[:, 1]),
        "  text                           %s" % stat(tb[:, 2]),
        "  total                          %s" % stat(tot_b),
        "  share of the text formatting in the batched total: %.0f %%" % (100 * np.median(tb[:, 2] / tot_b)),
        "batched + device text (ProposalListBuilder.build_text: the file's bytes from the device)",
        "  windows: count, read, fill     %s" % stat(tc[:, 0]),
        "  build_text: upload .. download %s" % stat(tc[:, 1]),
        "  total                          %s" % stat(tot_c),
        "  text launches, device events, one pass: size + scan %s ms, fill %s ms"
        % tuple("%.3f" % dev_ms[k] if k in dev_ms else "not measured" for k in ("size", "fill")),
        "  bytes downloaded: batched %d (7 arrays), device text %d (the size word; status, hits, record offsets, text)"
        % (down_b, down_c),
        "",
        "per video / batched, medians of the totals: %.1f x (min-max spread of the totals: %.1f ms and %.1f ms)"
        % (np.median(tot_a) / np.median(tot_b), tot_a.max() - tot_a.min(), tot_b.max() - tot_b.min()),
        "batched / device text, medians of the totals: %.1f x; batched - device text = %.1f ms against %.1f ms, the sum of "
        "the two min-max spreads (%.1f ms and %.1f ms): margin %s"
        % (np.median(tot_b) / np.median(tot_c), gain, spreads, tot_b.max() - tot_b.min(), tot_c.max() - tot_c.min(),
           "met" if gain > spreads else "NOT met"),
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert equal, "the paths disagree"


if __name__ == "__main__":
    main()
