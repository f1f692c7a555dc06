"""The commands that print the AR-AN report: tools/eval_proposals.py on an excerpt of the reference's published
ActivityNet 1.2 TAG list (tests/golden/anet12_tag_val_norm_first20.txt: its first 20 records, data), and
tools/gen_bottom_up_proposals.py with and without --ar_an on the records of tests/golden/ref_tag.npz.  Both against the
numpy referee of tests/proposal_eval_referee.py."""
import os
import pickle
from types import SimpleNamespace

import numpy as np

import proposal_eval_referee as R
from action_detection_amd.proposal_eval import ArAnResult, format_ar_an_report
from action_detection_amd.proposal_io import load_proposal_file
from test_proposal_drivers import GOLDEN, StubDB, tool

EXCERPT = os.path.join(GOLDEN, "anet12_tag_val_norm_first20.txt")


def check_arrays(got, ref):
    for name in ("first_hit", "matches", "recall", "proposals_per_video", "thresholds"):
        assert np.array_equal(got[name], ref[name]), name
    assert int(got["positives"]) == ref["positives"] and int(got["total_proposals"]) == ref["total_proposals"]
    assert (np.abs(got["avg_recall"] - ref["avg_recall"]) <= 1e-12 * np.abs(ref["avg_recall"])).all()
    assert abs(float(got["auc"]) - ref["auc"]) <= 1e-12 * abs(ref["auc"])


def test_eval_proposals_command_on_the_references_list(backend, tmp_path, capsys):
    records = load_proposal_file(EXCERPT)
    assert len(records) == 20 and records[0][0] == "nEOpfvJ7g_g" and len(records[0][3]) == 15
    gt = [[(float(g[1]), float(g[2])) for g in r[2]] for r in records]
    pr = [[(float(p[3]), float(p[4])) for p in r[3]] for r in records]
    cmd = tool("eval_proposals")
    out_file = str(tmp_path / "ar_an.npz")
    capsys.readouterr()
    cmd.main([EXCERPT, "--device", backend.device, "--out", out_file])
    printed = capsys.readouterr().out.split("\n")
    ref = R.ar_an(pr, gt)
    assert ref["positives"] == sum(len(g) for g in gt) >= 20 and 0.2 < ref["auc"] < 1.0
    assert printed[0] == "{}: 20 videos, {} proposals, {} groundtruth boxes".format(EXCERPT, sum(len(p) for p in pr), ref["positives"])
    report = format_ar_an_report(ArAnResult(**ref)).split("\n")
    assert printed[1:1 + len(report)] == report and printed[1 + len(report)] == "arrays written to " + out_file
    # AR@1, @5, @10, @50 lie inside this curve, @100 does not; one recall line per threshold; the area
    assert [l.split(":")[0] for l in report[1:5]] == ["AR@1", "AR@5", "AR@10", "AR@50"] and len(report) == 1 + 4 + 10 + 1
    assert report[-1] == "AUC: {:.2f}".format(ref["auc"] * 100)
    check_arrays(np.load(out_file), ref)
    assert [str(x) for x in np.load(out_file)["video_ids"]] == [r[0] for r in records]

    # the other options: a maximum, other thresholds, fewer points
    cmd.main([EXCERPT, "--device", backend.device, "--max-avg", "10", "--tiou", "0.3", "0.7", "3", "--points", "25",
              "--out", out_file])
    ref = R.ar_an(pr, gt, max_avg_nr_proposals=10, thresholds=np.linspace(0.3, 0.7, 3), points=25)
    check_arrays(np.load(out_file), ref)
    assert "AR@10: {:.2f}".format(ref["avg_recall"][-1] * 100) in capsys.readouterr().out


def run_bottom_up(backend, tmp_path, extra):
    d = np.load(os.path.join(GOLDEN, "ref_tag.npz"))
    videos, scores = [], {}
    for i, name in enumerate(str(n) for n in d["names"]):
        p = "v%d_" % i
        if bool(d[p + "gpu_only"][0]) and not backend.is_gpu:
            continue
        gt = [SimpleNamespace(num_label=int(l), time_span=(float(s), float(e))) for l, (s, e) in zip(d[p + "gt_label"], d[p + "gt_span"])]
        videos.append(SimpleNamespace(id=name, duration=float(d[p + "duration"][0]), instances=gt))
        scores[name] = d[p + "scores"][:, None, :]
    if not os.path.exists(str(tmp_path / "scores.pc")):
        with open(str(tmp_path / "scores.pc"), "wb") as f:
            pickle.dump(scores, f)
    result = tool("gen_bottom_up_proposals").main(
        [str(tmp_path / "scores.pc"), "--dataset", "thumos14", "--subset", "validation", "--minimum_len",
         str(float(d["minimum_len"][0])), "--device", backend.device] + extra, db=StubDB(videos))
    return result, [v for v in videos if v.instances]


def test_bottom_up_command_prints_the_report_only_when_asked(backend, tmp_path, capsys):
    capsys.readouterr()
    plain, _ = run_bottom_up(backend, tmp_path, [])
    before = capsys.readouterr().out
    assert "AR-AN" not in before and "AUC" not in before and not hasattr(plain, "ar_an")
    assert before.rstrip("\n").split("\n")[-1].startswith("Average Recall: ")

    with_mean, kept = run_bottom_up(backend, tmp_path, ["--ar_an"])
    after = capsys.readouterr().out
    assert after.startswith(before)                                        # the lines of today, byte for byte, then the report
    # the referee on what the generator made: TagResult.seconds per video, in NMS order
    from action_detection_amd.tag_proposals import TagProposalGenerator, merge_scores
    with open(str(tmp_path / "scores.pc"), "rb") as f:
        merged = merge_scores([pickle.load(f)], None)
    d = np.load(os.path.join(GOLDEN, "ref_tag.npz"))
    tag = TagProposalGenerator(minimum_len=float(d["minimum_len"][0]), device=backend.device).generate(
        [np.ascontiguousarray(merged[v.id], dtype=np.float32) for v in kept], [v.duration for v in kept])
    pr, gt = [r.seconds for r in tag], [[i.time_span for i in v.instances] for v in kept]
    ref = R.ar_an(pr, gt)
    assert after[len(before):] == format_ar_an_report(ArAnResult(**ref)) + "\n"
    check_arrays(with_mean.ar_an.__dict__, ref)

    with_max, _ = run_bottom_up(backend, tmp_path, ["--ar_an", "2"])
    again = capsys.readouterr().out
    ref2 = R.ar_an(pr, gt, max_avg_nr_proposals=2)
    assert again == before + format_ar_an_report(ArAnResult(**ref2)) + "\n"
    check_arrays(with_max.ar_an.__dict__, ref2)
    assert ref2["total_proposals"] < ref["total_proposals"] and abs(ref2["proposals_per_video"][-1] - 2.0) < 1e-9
