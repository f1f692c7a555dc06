"""The three commands of the proposal-list stage (tools/gen_sliding_window_proposals.py, gen_bottom_up_proposals.py,
gen_proposal_list.py), run in-process on small trees of empty frame files.

The sliding-window command is pinned against the list file and the report lines the REFERENCE's script wrote on the same
tree (tests/golden/ref_proposal_lists.npz, tools/make_proposal_list_golden.py); the bottom-up command against the dumped
records of tests/golden/ref_tag.npz; gen_proposal_list against tests/golden/proposal_list_processed.txt.
"""
import importlib.util
import json
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

from action_detection_amd.proposal_io import load_proposal_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_frames(folder, count, prefixes=("img_",)):
    os.makedirs(folder)
    for prefix in prefixes:
        for f in range(count):
            open(os.path.join(folder, "%s%05d.jpg" % (prefix, f + 1)), "w").close()


def materialise_thumos(tmp_path):
    with open(os.path.join(GOLDEN, "thumos14_excerpt.json")) as f:
        excerpt = json.load(f)
    for rel, text in excerpt.items():
        path = tmp_path / "data" / "thumos_14" / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(text)
    return str(tmp_path / "data" / "thumos_14")


def test_sliding_window_command_writes_the_references_list(backend, tmp_path, monkeypatch, capsys):
    ref = np.load(os.path.join(GOLDEN, "ref_proposal_lists.npz"))
    annotations = materialise_thumos(tmp_path)
    ids, counts = [str(x) for x in ref["thumos_test_ids"]], ref["thumos_test_frame_cnt"]
    for vid, c in zip(ids, counts):
        make_frames(str(tmp_path / "frames" / vid), int(c))
    monkeypatch.chdir(tmp_path)
    cmd = tool("gen_sliding_window_proposals")
    argv = ["testing", "rgb", "frames", "list.txt", "--dataset", "thumos14", "--annotations", annotations, "--device", backend.device]
    capsys.readouterr()
    cmd.main(argv)
    printed = capsys.readouterr().out.split("\n")
    assert (tmp_path / "list.txt").read_text() == str(ref["script_list"])
    report = [l for l in printed if l.startswith(("average", "IOU threshold", "list written"))]
    assert report == [str(x) for x in ref["script_report"]]
    back = load_proposal_file(str(tmp_path / "list.txt"))
    assert [b[0] for b in back] == [os.path.join("frames", v) for v in ids] and [b[1] for b in back] == [int(c) for c in counts]
    off = ref["thumos_test_o70_win_off"]
    assert [len(b[3]) for b in back] == list(np.diff(off)) and [len(b[2]) for b in back] == list(np.diff(ref["thumos_test_gt_off"]))

    # --avoid leaves videos out of the written list (and only there); flow counts flow_x_*.jpg
    left_out = ("video_test_0001433", ids[0])          # (the former: the folder without frames)
    (tmp_path / "avoid.txt").write_text("\n".join(left_out) + "\n")
    cmd.main(argv[:3] + ["list_avoid.txt"] + argv[4:] + ["--avoid", "avoid.txt"])
    avoided = load_proposal_file(str(tmp_path / "list_avoid.txt"))
    assert [b[0] for b in avoided] == [os.path.join("frames", v) for v in ids if v not in left_out]
    assert [b[1:] for b in avoided] == [b[1:] for b in back if b[0].split("/")[-1] not in left_out]
    # the samplers of tools/train_ssn.py and tools/train_binary.py load the written list
    from action_detection_amd.actionness_sampling import ActionnessSampler
    from action_detection_amd.proposal_sampling import ProposalSampler
    with_gt = sum(1 for b in avoided if b[2])          # (the samplers leave videos without ground truth out)
    assert len(ProposalSampler("list_avoid.txt").video_list) == with_gt >= 3
    assert len(ActionnessSampler("list_avoid.txt").video_list) >= 1
    cmd.main(["testing", "flow"] + argv[2:3] + ["list_flow.txt"] + argv[4:])
    assert all(b[1] == 0 for b in load_proposal_file(str(tmp_path / "list_flow.txt")))

    # a video of the subset without a frame folder ends the run with an error that names it
    os.rmdir(str(tmp_path / "frames" / "video_test_0001433"))      # (the fixture's folder without frames)
    with pytest.raises(ValueError, match="video_test_0001433"):
        cmd.main(argv)


def test_sliding_window_command_on_activitynet(backend, tmp_path, monkeypatch, capsys):
    ref = np.load(os.path.join(GOLDEN, "ref_proposal_lists.npz"))
    ids, counts = [str(x) for x in ref["anet_validation_ids"]], ref["anet_validation_frame_cnt"]
    for vid, c in zip(ids, counts):
        make_frames(str(tmp_path / "frames" / ("v_" + vid)), int(c))
    monkeypatch.chdir(tmp_path)
    tool("gen_sliding_window_proposals").main(["validation", "rgb", "frames", "anet.txt", "--overlap", "0.4", "--annotations",
                                               os.path.join(GOLDEN, "anet_tiny.json"), "--device", backend.device])
    want = "".join("# %d\n%s" % (i + 1, str(t)) for i, t in enumerate(ref["anet_validation_o40_dump"]))
    assert (tmp_path / "anet.txt").read_text() == want
    assert "average # of proposals: {} at overlap param 0.4".format(np.mean(np.diff(ref["anet_validation_o40_win_off"]))) \
        in capsys.readouterr().out


class StubDB(object):
    """The videos of ref_tag.npz as a database: every video has the id and folder of its name."""

    def __init__(self, videos):
        self.videos = videos

    def get_subset_videos(self, subset):
        assert subset == "validation"
        return self.videos

    def try_load_file_path(self, frame_path):
        for v in self.videos:
            v.path = os.path.join(frame_path, v.id)
        return len(self.videos)


def test_bottom_up_command_writes_the_references_records(backend, tmp_path, monkeypatch, capsys):
    d = np.load(os.path.join(GOLDEN, "ref_tag.npz"))
    videos, scores, dumps = [], {}, {}
    for i, name in enumerate(str(n) for n in d["names"]):
        p = "v%d_" % i
        if bool(d[p + "gpu_only"][0]) and not backend.is_gpu:
            continue
        gt = [SimpleNamespace(num_label=int(l), time_span=(float(s), float(e))) for l, (s, e) in zip(d[p + "gt_label"], d[p + "gt_span"])]
        videos.append(SimpleNamespace(id=name, duration=float(d[p + "duration"][0]), instances=gt))
        if gt:                                                            # (videos without instances are never looked up)
            make_frames(str(tmp_path / "frames" / name), int(d[p + "frame_cnt"][0]))
        scores[name] = d[p + "scores"][:, None, :]                       # [T, 1, 2]: one crop
        dumps[name] = str(d[p + "dump"])
    missing = videos[-1].id                                               # one annotated video has no scores
    assert videos[-1].instances
    del scores[missing]
    with open(str(tmp_path / "scores.pc"), "wb") as f:
        pickle.dump(scores, f)
    monkeypatch.chdir(tmp_path)
    result = tool("gen_bottom_up_proposals").main(
        ["scores.pc", "--dataset", "thumos14", "--subset", "validation", "--minimum_len", str(float(d["minimum_len"][0])),
         "--frame_path", "frames", "--write_proposals", "tag.txt", "--device", backend.device], db=StubDB(videos))
    out = capsys.readouterr().out
    kept = [v for v in videos if v.instances and v.id != missing]
    assert {len(v.instances) for v in videos} >= {0, 1, 3} and len(kept) >= 4
    assert "video list size: %d\n" % (len(kept) + 1) in out and "1 videos without scores left out" in out
    assert "%d groundtruth boxes from" % sum(len(v.instances) for v in kept) in out
    assert "list written. got %d videos" % len(kept) in out
    text = (tmp_path / "tag.txt").read_text()
    assert text == "".join("# %d\n%s" % (i + 1, dumps[v.id]) for i, v in enumerate(kept))
    assert [b[0] for b in load_proposal_file(str(tmp_path / "tag.txt"))] == ["frames/" + v.id for v in kept]
    assert list(result.thresholds) == list(np.arange(0.5, 1, 0.2)) and result.thresholds[2] != 0.9
    for th, (pv, pi) in zip(result.thresholds, result.recall):
        assert 'IOU threshold {}. per video recall: {:02f}, per instance recall: {:02f}'.format(th, pv * 100, pi * 100) in out
    assert 'Average Recall: {:.04f} {:.04f}'.format(*(np.mean(result.recall, axis=0) * 100)) in out


def test_gen_proposal_list_command(tmp_path, monkeypatch):
    with open(os.path.join(GOLDEN, "proposal_list_expected.json")) as f:
        frame_dict = json.load(f)["frame_dict"]
    for vid, (path, rgb, flow) in frame_dict.items():
        assert path == "frames/" + vid
        make_frames(str(tmp_path / path), rgb)
        for prefix in ("flow_x_", "flow_y_"):
            for f in range(min(flow, 3)):
                open(str(tmp_path / path / ("%s%05d.jpg" % (prefix, f + 1))), "w").close()
    monkeypatch.chdir(tmp_path)
    cmd = tool("gen_proposal_list")
    norm = os.path.join(GOLDEN, "proposal_list_norm.txt")
    parsed = cmd.main(["thumos14", "frames", "--norm-list", norm, "--out-list", "a.txt", "--norm-list", norm,
                       "--out-list", "b.txt"])
    want = open(os.path.join(GOLDEN, "proposal_list_processed.txt")).read()
    assert (tmp_path / "a.txt").read_text() == want and (tmp_path / "b.txt").read_text() == want
    assert {k: v[:2] for k, v in parsed.items()} == {k: (v[0], v[1]) for k, v in frame_dict.items()}
    # thumos14 keys by the folder name, activitynet1.2 by the path's last 11 characters; an x / y mismatch is an error
    # that names the folder
    from action_detection_amd.proposal_io import parse_directory
    by_tail = parse_directory("frames", key_func=cmd.KEY_FUNCS["activitynet1.2"])
    assert sorted(by_tail) == sorted(("frames/" + v)[-11:] for v in frame_dict) and any(len(v) != 11 for v in frame_dict)
    assert parse_directory("frames") == by_tail
    vid = sorted(frame_dict)[0]
    open(str(tmp_path / "frames" / vid / "flow_x_99999.jpg"), "w").close()
    with pytest.raises(ValueError, match=vid):
        cmd.main(["thumos14", "frames", "--norm-list", norm, "--out-list", "c.txt"])
    with pytest.raises(SystemExit):
        cmd.main(["thumos14", "frames", "--norm-list", norm])
