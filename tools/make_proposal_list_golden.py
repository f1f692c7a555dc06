#!/usr/bin/env python
"""Generate the fixtures of the proposal-list stage (test infrastructure; runs only where the reference tree exists,
what it writes under tests/golden/ is committed as data):

  thumos14_excerpt.json     {relative path: text}: a trimmed copy of the reference's data/thumos_14 -- all 21 + 21 class
                            file names (they define the label indices), annotation lines and durations of the CHOSEN
                            videos only, the two avoid files as they are
  ref_proposal_lists.npz    what the REFERENCE's own classes and functions make of that excerpt and of the hand-written
                            anet_tiny.json: video order, labels and spans per subset (ops/thumos_db.py, ops/anet_db.py);
                            for overlap 0.7 and 0.4 the windows (gen_exponential_sw_proposal), the name_proposal rows,
                            get_temporal_proposal_recall at 0.5 / 0.7 / 0.9 and the dump_window_list text per video,
                            against temporary frame folders with seeded file counts (one of them 0); the list file and
                            the report lines of gen_sliding_window_proposals.py, run as a script

The reference reads the class files in the order glob lists them, which the file system decides; glob.glob is wrapped to
sort here, the order datasets.ThumosDB fixes.  The conditions the tests rely on are asserted before anything is written:
every one of the three THUMOS rules removes an annotation line, some (video, level) keeps no window, some duration is an
exact multiple of a step.  (IoUs that lie exactly ON a recall threshold do occur on these videos, see main.)
"""
import contextlib
import glob
import io
import json
import os
import runpy
import shutil
import sys
import tempfile
import warnings

import numpy as np

from make_tag_golden import REF, ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
CHOSEN = {"validation": ["video_validation_0000364",      # two HighJump instances start behind the duration
                         "video_validation_0000178",      # CricketShot on the avoid list
                         "video_validation_0000190",      # the shortest annotated video, 8.932 s
                         "video_validation_0000201",      # Ambiguous lines
                         "video_validation_0000885"],     # no instances
          "test": ["video_test_0000814", "video_test_0000364",      # the latter: integral duration (213 s), no instances
                   "video_test_0000793",                  # the longest annotated video, 1673.428 s
                   "video_test_0001433",                  # Ambiguous lines
                   "video_test_0000062", "video_test_0000764", "video_test_0000367"]}      # ...0367: HighJump on the avoid list
OVERLAPS = (0.7, 0.4)
THRESHOLDS = (0.5, 0.7, 0.9)
IOU_MARGIN = 1e-9


def make_excerpt():
    src = os.path.join(REF, "data", "thumos_14")
    out = {}
    for subset, chosen in CHOSEN.items():
        lines = open(os.path.join(src, "%s_durations.txt" % subset)).read().split("\n")
        kept = []
        for i in range(0, len(lines) - 1, 2):
            if lines[i].strip().split(".")[0] in chosen:
                kept += [lines[i], lines[i + 1]]
        assert len(kept) == 2 * len(chosen), subset
        out["%s_durations.txt" % subset] = "\n".join(kept) + "\n"
        out["%s_avoid_videos.txt" % subset] = open(os.path.join(src, "%s_avoid_videos.txt" % subset)).read()
        folder = "temporal_annotations_%s" % subset
        for name in sorted(os.listdir(os.path.join(src, folder))):
            rows = [l for l in open(os.path.join(src, folder, name)) if l.split() and l.split()[0] in chosen]
            out["%s/%s" % (folder, name)] = "".join(rows)
    return out


def dropped_by_rule(excerpt):
    """Annotation lines of the excerpt that each of the three rules removes, counted from the text alone."""
    n = {"avoid": 0, "behind": 0, "ambiguous": 0}
    for subset in CHOSEN:
        d = excerpt["%s_durations.txt" % subset].split("\n")
        dur = {d[i].split(".")[0]: float(d[i + 1]) for i in range(0, len(d) - 1, 2)}
        avoid = set(tuple(l.split()) for l in excerpt["%s_avoid_videos.txt" % subset].split("\n") if l.strip())
        for path, text in excerpt.items():
            if not path.startswith("temporal_annotations_%s/" % subset):
                continue
            cls = os.path.basename(path).split("_")[0]
            for l in text.split("\n"):
                if not l.strip():
                    continue
                vid, st = l.split()[0], float(l.split()[1])
                if (vid, cls) in avoid:
                    n["avoid"] += 1
                elif st > dur[vid]:
                    n["behind"] += 1
                elif cls == "Ambiguous":
                    n["ambiguous"] += 1
    return n


def main():
    assert os.path.isdir(REF), "this script needs the reference tree at %s" % REF
    excerpt = make_excerpt()
    rules = dropped_by_rule(excerpt)
    assert min(rules.values()) >= 1, rules
    assert sum(p.startswith("temporal_annotations_") for p in excerpt) == 42
    print("annotation lines removed by rule:", rules)

    tmp = tempfile.mkdtemp()
    for rel, text in excerpt.items():
        os.makedirs(os.path.dirname(os.path.join(tmp, "data", "thumos_14", rel)), exist_ok=True)
        with open(os.path.join(tmp, "data", "thumos_14", rel), "w") as f:
            f.write(text)
    shutil.copy(os.path.join(GOLDEN, "anet_tiny.json"), os.path.join(tmp, "data", "activity_net.v1-2.min.json"))
    cwd = os.getcwd()
    os.chdir(tmp)
    sys.path.insert(0, REF)
    real_glob = glob.glob
    glob.glob = lambda *a, **k: sorted(real_glob(*a, **k))
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        from ops.anet_db import ANetDB
        from ops.thumos_db import THUMOSDB
        from ops.detection_metrics import get_temporal_proposal_recall, name_proposal, temporal_recall
        from ops.io import dump_window_list
        from ops.sequence_funcs import gen_exponential_sw_proposal
        dbs = {"thumos": (THUMOSDB.get_db(), ("validation", "test"), lambda vid: vid),
               "anet": (ANetDB.get_db("1.2"), ("training", "validation", "testing"), lambda vid: "v_" + vid)}

    out = {"overlaps": np.asarray(OVERLAPS), "thresholds": np.asarray(THRESHOLDS)}
    rs = np.random.RandomState(2024)
    empty_level = exact_multiple = False
    margin, on_threshold = np.inf, []
    for name, (db, subsets, folder_of) in dbs.items():
        out["%s_labels" % name] = np.asarray(db.get_ordered_label_list())
        for s in subsets:
            videos = list(db.get_subset_videos(s))
            counts = [int(rs.randint(20, 400)) for _ in videos]
            if name == "thumos" and s == "test":
                counts[[v.id for v in videos].index("video_test_0001433")] = 0
            for v, c in zip(videos, counts):
                os.makedirs(os.path.join("frames", folder_of(v.id)))
                for f in range(c):
                    open(os.path.join("frames", folder_of(v.id), "img_%05d.jpg" % (f + 1)), "w").close()
            p = "%s_%s_" % (name, s)
            out[p + "ids"] = np.asarray([v.id for v in videos])
            out[p + "durations"] = np.asarray([v.duration for v in videos], dtype=np.float64)
            out[p + "integral"] = np.asarray([isinstance(v.duration, int) for v in videos])
            out[p + "gt_off"] = np.concatenate([[0], np.cumsum([len(v.instances) for v in videos])]).astype(np.int64)
            out[p + "gt_label"] = np.asarray([i.num_label for v in videos for i in v.instances], dtype=np.int32)
            out[p + "gt_span"] = np.asarray([i.time_span for v in videos for i in v.instances], dtype=np.float64).reshape(-1, 2)
            out[p + "frame_cnt"] = np.asarray(counts, dtype=np.int64)
        with contextlib.redirect_stdout(sink):
            db.try_load_file_path("frames")
        for s in subsets:
            videos = list(db.get_subset_videos(s))
            gt_spans = [[(x.num_label, x.time_span) for x in v.instances] for v in videos]
            for ov in OVERLAPS:
                p = "%s_%s_o%d_" % (name, s, round(ov * 100))
                props = [gen_exponential_sw_proposal(v, overlap=ov) for v in videos]
                named = [name_proposal(g, pr) for g, pr in zip(gt_spans, props)]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")          # (a subset without any ground truth: 0 / 0)
                    recall = [get_temporal_proposal_recall(props, [[y[1] for y in g] for g in gt_spans], th) for th in THRESHOLDS]
                out[p + "win_off"] = np.concatenate([[0], np.cumsum([len(pr) for pr in props])]).astype(np.int64)
                out[p + "windows"] = np.asarray([w for pr in props for w in pr], dtype=np.float64).reshape(-1, 2)
                out[p + "named"] = np.asarray([r for n in named for r in n], dtype=np.float64).reshape(-1, 5)
                out[p + "recall"] = np.asarray(recall, dtype=np.float64)
                out[p + "hits"] = np.asarray([[temporal_recall([y[1] for y in g], pr, th)[0] for th in THRESHOLDS]
                                              for g, pr in zip(gt_spans, props)], dtype=np.int64).reshape(-1, len(THRESHOLDS))
                out[p + "dump"] = np.asarray([dump_window_list(v, n, "frames", "img_*.jpg") for v, n in zip(videos, named)])
                # the conditions the tests rely on
                for v, pr, g in zip(videos, props, gt_spans):
                    for t_span in (2 ** x for x in range(8)):
                        step = int(np.ceil(t_span * (1 - ov)))
                        n_level = sum(1 for w in pr if w[1] - w[0] == t_span)
                        empty_level |= n_level == 0
                        exact_multiple |= float(v.duration) / step == int(float(v.duration) / step) and v.duration >= step
                    if g and pr:
                        a, b = np.asarray([x[1] for x in g], dtype=np.float64), np.asarray(pr, dtype=np.float64)
                        inter = np.minimum(a[:, None, 1], b[None, :, 1]) - np.maximum(a[:, None, 0], b[None, :, 0])
                        hull = np.maximum(a[:, None, 1], b[None, :, 1]) - np.minimum(a[:, None, 0], b[None, :, 0])
                        iou = np.where(inter > 0, inter / hull, 0.0)
                        here = float(np.abs(iou[..., None] - np.asarray(THRESHOLDS)).min())
                        if here < IOU_MARGIN:
                            on_threshold.append((v.id, ov, here))
                        margin = min(margin, here)
    assert empty_level, "no (video, level) without a window"
    assert exact_multiple, "no duration that is an exact multiple of a step"
    # NOT a condition: "no IoU within 1e-9 of a recall threshold" cannot hold on these videos.  THUMOS14 annotations have a
    # resolution of 0.1 s and the windows are whole seconds, so IoUs of exactly 1/2 occur (and one of video_test_0000814 lies
    # one ulp from a threshold).  The comparisons stay exact all the same -- an IoU is one IEEE division of two exact
    # differences on either side -- and the reference's per-video hit counts are recorded so that the tests pin exactly
    # these decisions.
    for vid, ov, here in on_threshold:
        print("  %s (overlap %g): an IoU within %g of a recall threshold" % (vid, ov, here))
    out["iou_margin_measured"] = np.asarray([margin])

    # the reference's script itself, on the THUMOS14 test subset (its own defaults: overlap 0.7)
    argv = sys.argv
    sys.argv = ["gen_sliding_window_proposals.py", "testing", "rgb", "frames", "list.txt", "--dataset", "thumos14"]
    report = io.StringIO()
    with contextlib.redirect_stdout(report):
        runpy.run_path(os.path.join(REF, "gen_sliding_window_proposals.py"), run_name="__main__")
    sys.argv = argv
    out["script_list"] = np.asarray(open("list.txt").read())
    out["script_report"] = np.asarray([l for l in report.getvalue().split("\n")
                                       if l.startswith(("average", "IOU threshold", "list written"))])
    assert len(out["script_report"]) == 6, report.getvalue()
    glob.glob = real_glob
    os.chdir(cwd)
    shutil.rmtree(tmp)

    with open(os.path.join(GOLDEN, "thumos14_excerpt.json"), "w") as f:
        json.dump(excerpt, f, indent=0, sort_keys=True)
        f.write("\n")
    path = os.path.join(GOLDEN, "ref_proposal_lists.npz")
    np.savez_compressed(path, **out)
    for f in ("thumos14_excerpt.json", "ref_proposal_lists.npz"):
        print("wrote %s (%d bytes)" % (f, os.path.getsize(os.path.join(GOLDEN, f))))
    print("windows per (db, subset) at overlap 0.7:",
          {k[:-12]: int(v[-1]) for k, v in out.items() if k.endswith("_o70_win_off")})


if __name__ == "__main__":
    main()
