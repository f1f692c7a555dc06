"""TAG proposal generation (csrc/tag.hip, tag_proposals.py, the writer in proposal_io.py).

Pinned against tests/golden/ref_tag.npz: seeded actionness scores and the outputs of the REFERENCE's own functions
(tools/make_tag_golden.py: label_frame_by_threshold, build_box_by_search, gen_prop / temporal_nms, name_proposal,
dump_window_list, the score-merging loop, gen_exponential_sw_proposal).  Agreement is EXACT, for two reasons the
generator asserts on the inputs: no smoothed probability of a fixture video lies within 1e-5 of a threshold (softmax /
expf differ from numpy's by <= 3e-7 on a probability, so the label rows are the reference's), and the reference's kept
list does not depend on how equal scores are ordered.  With equal labels everything downstream is integer arithmetic,
single IEEE float64 operations and float32 adds in a fixed order.  Candidates are compared as a sorted multiset, kept
lists after ordering both sides by (score descending, start, end), scores as bit patterns.

The emulator runs every barrier through fibers: the CPU tier takes the fixture videos of at most 300 frames, the long
ones (two of them, noisy4000 and runs3000, with more candidates than fit in LDS: the global-memory sort) run under -m gpu
only."""
import ctypes
import os

import numpy as np
import pytest
import torch

import action_detection_amd as pkg
from action_detection_amd import _lib
from action_detection_amd import kernels as K
from action_detection_amd.proposal_io import format_window_list_record, load_proposal_file, write_proposal_file
from action_detection_amd.tag_proposals import (TagProposalGenerator, merge_scores, name_proposals,
                                                sliding_window_proposals)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tag.npz")


def fixture():
    d = np.load(GOLDEN)
    vids = []
    for i, name in enumerate(d["names"]):
        p = "v%d_" % i
        scores = d[p + "scores"]
        vids.append({"name": str(name), "scores": scores, "duration": float(d[p + "duration"][0]),
                     "gpu_only": bool(d[p + "gpu_only"][0]), "margin": float(d[p + "margin"][0]),
                     "labels": np.unpackbits(d[p + "labels"], axis=1)[:, :len(scores)].astype(bool),
                     "cand_box": d[p + "cand_box"], "cand_score": d[p + "cand_score"], "kept_box": d[p + "kept_box"],
                     "kept_score": d[p + "kept_score"], "seconds": d[p + "seconds"],
                     "gt": [(int(l), (float(s), float(e))) for l, (s, e) in zip(d[p + "gt_label"], d[p + "gt_span"])],
                     "named": d[p + "named"], "frame_cnt": int(d[p + "frame_cnt"][0]), "dump": str(d[p + "dump"])})
    return d, vids


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canonical(boxes, scores):
    """rows (start, end, score bits) ordered by (score descending, start, end)"""
    boxes, scores = np.asarray(boxes).reshape(-1, 2), np.asarray(scores, dtype=np.float32)
    order = np.lexsort((boxes[:, 1], boxes[:, 0], -scores.astype(np.float64)))
    return np.column_stack([boxes[order].astype(np.int64), bits(scores[order]).astype(np.int64)])


def multiset(boxes, scores):
    rows = np.column_stack([np.asarray(boxes).reshape(-1, 2).astype(np.int64), bits(scores).astype(np.int64)])
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


def selected(vids, backend):
    return [v for v in vids if backend.is_gpu or not v["gpu_only"]]


def check_video(v, r, minimum_len):
    assert np.array_equal(r.labels, v["labels"]), v["name"]
    assert np.array_equal(multiset(*r.candidates), multiset(v["cand_box"], v["cand_score"])), v["name"]
    assert np.array_equal(canonical(r.boxes, r.scores), canonical(v["kept_box"], v["kept_score"])), v["name"]
    assert r.boxes.dtype == np.int32 and r.scores.dtype == np.float32 and r.seconds.dtype == np.float64
    # the spans in seconds follow the product's kept order: the same set as the reference's, and the kept boxes' own
    T = len(v["scores"])
    assert sorted(map(tuple, r.seconds)) == sorted(map(tuple, v["seconds"])), v["name"]
    longer = [(a / float(T) * v["duration"], b / float(T) * v["duration"]) for a, b in r.boxes]
    assert [s for s in longer if s[1] - s[0] > minimum_len] == [tuple(s) for s in r.seconds]


def test_fixture_conditions():
    d, vids = fixture()
    assert float(d["margin_required"][0]) == 1e-5
    assert all(v["margin"] >= 1e-5 for v in vids)
    # all background, all foreground, T = 1 foreground / background, T = 5.  (The generator's T = 5 pattern and its
    # both-ends video are its own -- the latter faded on purpose, see both_ends_video there -- so their kept counts, 1
    # and 16, are not the 2 and 20 of the patterns the issue's author tried.)
    assert [len(v["kept_box"]) for v in vids[:5]] == [0, 1, 1, 0, 1]
    assert max(len(v["scores"]) for v in vids if not v["gpu_only"]) <= 300
    assert sum(len(v["cand_box"]) > 2048 for v in vids) == 2
    assert any(len(v["seconds"]) < len(v["kept_box"]) for v in vids)      # minimum_len removes some spans


def test_batch_matches_reference(backend):
    """All selected fixture videos in ONE batch (lengths 1 ... 300 on the emulator, 1 ... 4000 on the GPU, side by side)."""
    d, vids = fixture()
    vs = selected(vids, backend)
    gen = TagProposalGenerator(minimum_len=float(d["minimum_len"][0]), device=backend.device)
    res = gen.generate([v["scores"] for v in vs], [v["duration"] for v in vs], return_candidates=True, return_labels=True)
    assert len(res) == len(vs)
    for v, r in zip(vs, res):
        check_video(v, r, float(d["minimum_len"][0]))
    # the returned scores are NOT filtered by minimum_len (gen_bottom_up_proposals.py:142)
    assert any(len(r.seconds) < len(r.scores) for r in res)


def test_default_minimum_len_keeps_every_span(backend):
    _, vids = fixture()
    v = [x for x in vids if x["name"] == "noisy60"][0]
    r = TagProposalGenerator(device=backend.device).generate([v["scores"]], [v["duration"]])[0]
    assert len(r.seconds) == len(r.boxes) == len(v["kept_box"])
    T = len(v["scores"])
    assert np.array_equal(r.seconds, np.array([(a / float(T) * v["duration"], b / float(T) * v["duration"])
                                               for a, b in r.boxes]))


def test_batch_independence(backend):
    """Each video alone == the same video inside a batch of 64, bit for bit (kept order included)."""
    _, vids = fixture()
    pool = [v for v in selected(vids, backend) if len(v["scores"]) <= (4000 if backend.is_gpu else 60)]
    batch = [pool[i % len(pool)] for i in range(64)]
    gen = TagProposalGenerator(minimum_len=1.5, device=backend.device)
    together = gen.generate([v["scores"] for v in batch], [v["duration"] for v in batch], return_candidates=True)
    alone = {v["name"]: gen.generate([v["scores"]], [v["duration"]], return_candidates=True)[0] for v in pool}
    for v, r in zip(batch, together):
        a = alone[v["name"]]
        assert np.array_equal(r.boxes, a.boxes) and np.array_equal(bits(r.scores), bits(a.scores))
        assert np.array_equal(r.seconds, a.seconds)
        assert np.array_equal(r.candidates[0], a.candidates[0]) and np.array_equal(bits(r.candidates[1]), bits(a.candidates[1]))


def test_non_finite_scores_never_fault(backend):
    """inf / NaN / huge scores: the call returns, every kept box lies in [0, T + 1] and start < end."""
    rs = np.random.RandomState(3)
    vids = []
    for T, spoil in ((40, np.inf), (75, np.nan), (33, -np.inf), (64, 3e38), (1, np.nan), (50, None)):
        s = (rs.standard_normal((T, 2)) * 2).astype(np.float32)
        if spoil is not None:
            s[rs.randint(0, T, max(1, T // 5)), rs.randint(0, 2, max(1, T // 5))] = spoil
        else:
            s[:, 1] = 3e38                      # every box sum overflows to inf
            s[:, 0] = -3e38
        vids.append(s)
    res = TagProposalGenerator(device=backend.device).generate(vids, [10.0] * len(vids), return_candidates=True)
    for s, r in zip(vids, res):
        T = len(s)
        for boxes in (r.boxes, r.candidates[0]):
            assert ((boxes[:, 0] >= 0) & (boxes[:, 1] <= T + 1) & (boxes[:, 0] < boxes[:, 1])).all()
    assert len(res[-1].boxes) >= 1 and np.isinf(res[-1].scores).all()


def test_bad_arguments_are_rejected_before_any_launch():
    """Checkable without a GPU: the real library validates on the host before it launches anything."""
    lib = _lib.SsnLibrary(pkg.build())
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_tag_count", None, None, None, 1, 8, None, 1, 3.0, None, None, None, None, None)
    good = (ctypes.c_int * 3)(0, 3, 8)
    for bad in ((0, 5, 3), (0, 3, 3), (1, 3, 8), (0, 3, 7)):                 # decreasing, empty video, not from 0, wrong total
        arr = (ctypes.c_int * 3)(*bad)
        with pytest.raises(RuntimeError, match="offsets"):
            lib.call("ssn_tag_count", p, ctypes.addressof(arr), p, 2, 8, p, 1, 3.0, p, p, None, p, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("ssn_tag_count", p, ctypes.addressof(good), p, 0, 8, p, 1, 3.0, p, p, None, p, None)
    with pytest.raises(RuntimeError, match="bw out of range"):
        lib.call("ssn_tag_count", p, ctypes.addressof(good), p, 2, 8, p, 1, 100.0, p, p, None, p, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_tag_generate", *([None] * 4), 1, 8, None, 1, None, 1, None, None, 0, 0, 0.9, 0.0, *([None] * 8), 0, None)
    with pytest.raises(RuntimeError, match="bad table sizes"):
        lib.call("ssn_tag_generate", p, p, p, p, 1, 8, p, 1, p, 1, p, p, -1, 0, 0.9, 0.0, *([p] * 8), 0, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_tag_name_proposals", None, None, None, 0, None, None, 1, 0, 0.0, None, None, None, None)


def test_wrong_shapes_are_rejected(backend):
    gen = TagProposalGenerator(device=backend.device)
    ok = np.zeros((5, 2), dtype=np.float32)
    for bad in (np.zeros((5, 3), dtype=np.float32), np.zeros((0, 2), dtype=np.float32), np.zeros((5, 2), dtype=np.float64),
                np.zeros(5, dtype=np.float32)):
        with pytest.raises(ValueError):
            gen.generate([ok, bad], [1.0, 1.0])
    with pytest.raises(ValueError):
        gen.generate([ok], [1.0, 2.0])
    dev = backend.device
    h = torch.tensor([0, 5], dtype=torch.int32)
    with pytest.raises(ValueError):
        K.tag_count(torch.zeros(5, 3).to(dev), h, h.to(dev), torch.tensor([0.5]).to(dev), 3)
    with pytest.raises(ValueError):
        K.tag_count(torch.zeros(5, 2).to(dev), h.long(), h.to(dev), torch.tensor([0.5]).to(dev), 3)
    with pytest.raises(RuntimeError, match="offsets"):                       # non-monotone offsets: the library's own check
        bad = torch.tensor([0, 4, 2, 5], dtype=torch.int32)
        K.tag_count(torch.zeros(5, 2).to(dev), bad, bad.to(dev), torch.tensor([0.5]).to(dev), 3)


def test_named_proposals_and_dumped_text(backend, tmp_path):
    _, vids = fixture()
    vs = selected(vids, backend)
    named = name_proposals([v["gt"] for v in vs], [v["seconds"] for v in vs], device=backend.device)
    records = []
    for v, n in zip(vs, named):
        assert np.array_equal(np.asarray(n, dtype=np.float64).reshape(-1, 5), v["named"]), v["name"]
        rec = format_window_list_record("frames/" + v["name"], v["frame_cnt"], v["duration"], v["gt"], n)
        assert rec == v["dump"], v["name"]
        records.append(rec)
    assert {len(v["gt"]) for v in vs} >= {0, 1, 3}
    path = str(tmp_path / "tag_list.txt")
    write_proposal_file(path, records)
    back = load_proposal_file(path)
    assert len(back) == len(vs)
    for v, n, (vid, n_frame, gt_boxes, pr_boxes) in zip(vs, named, back):
        fps = v["frame_cnt"] / v["duration"]
        assert vid == "frames/" + v["name"] and n_frame == v["frame_cnt"]
        assert [[int(x) for x in g] for g in gt_boxes] == [[g[0] + 1, int(g[1][0] * fps), int(g[1][1] * fps)] for g in v["gt"]]
        assert len(pr_boxes) == len(n)
        for row, p in zip(pr_boxes, n):
            assert int(row[0]) == p[0] and row[1] == "%.4f" % p[1] and row[2] == "%.4f" % p[2]
            assert (int(row[3]), int(row[4])) == (int(p[3] * fps), int(p[4] * fps))


def test_merge_scores():
    d, _ = fixture()
    files = [{k: d["merge_in%d_%s" % (f, k)] for k in "ab"} for f in range(2)]
    assert files[1]["a"].shape[0] < files[0]["a"].shape[0] and files[1]["b"].shape[0] > files[0]["b"].shape[0]
    for tag, weights in (("w", [float(x) for x in d["merge_weights"]]), ("n", None)):
        got = merge_scores(files, weights)
        for k in "ab":
            assert got[k].dtype == np.float32 and np.array_equal(bits(got[k]), bits(d["merge_%s_%s" % (tag, k)])), (tag, k)


def test_sliding_window_proposals():
    d, _ = fixture()
    for j in range(3):
        dur = float(d["sw%d_duration" % j][0])
        dur = int(dur) if dur == int(dur) else dur
        got = np.asarray(sliding_window_proposals(dur), dtype=np.float64).reshape(-1, 2)
        assert np.array_equal(got, d["sw%d" % j]) and len(got) > 0
