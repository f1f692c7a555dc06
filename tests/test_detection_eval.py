"""Detection evaluation (csrc/eval.hip, detection_eval.py, tools/eval_detections.py).

Pinned against tests/golden/ref_eval.npz (tools/make_eval_golden.py).  The AP function the reference calls belongs to
the ActivityNet toolkit, a submodule that is empty in the reference tree: the AP expectations come from the generator's
numpy referee, a literal walk of the public algorithm (stable sorts where the toolkit's argsort leaves ties open), NOT
from reference output.  The recall expectations are the outputs of the reference's own temporal_recall /
get_temporal_proposal_recall; thresholds, means, table formats and the score merge are checked against the reference's
expressions.

What is exact and why: the IoU is float64 `inter / ((ge - gs) + (e - s) - inter)` in that order on both sides -- no
multiply, so nothing can be contracted, and IEEE subtraction / division round as numpy's do.  The tp flags and the score
order are therefore compared with array_equal on EVERY case, with no margin around a threshold (the `anet_grid` case
has IoUs that equal a threshold).  AP: |ap - expected| <= 1e-12 absolute, derived: tp is exact, each term is one float64
division of integers, the terms are non-negative and sum to at most npos, so another summation order moves the result
by at most n * 2^-53 with n a few thousand.

The chain test uses the five ref_detection.npz cases whose fused scores are finite; the sixth (overflowed: inf / NaN
scores) cannot be evaluated -- scores must be finite -- and is asserted to raise ValueError instead.
"""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import action_detection_amd as pkg
from action_detection_amd import _lib
from action_detection_amd import kernels as K
from action_detection_amd.detection_eval import (DetectionEvaluator, average_precision_flat, format_map_table, map_table_rows,
                                                 merge_detection_scores, proposal_recall, tiou_thresholds)
from action_detection_amd.detection_post import DetectionPostProcessor
from action_detection_amd.proposal_sampling import ProposalSampler

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "ref_eval.npz")
AP_TOL = 1e-12


def tools_module(name):
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    return __import__(name)


def fixture():
    d = np.load(GOLDEN)
    cases = {}
    for name in (str(n) for n in d["names"]):
        c = {k: d["%s_%s" % (name, k)] for k in ("gt_cls", "gt_vid", "gt_seg", "pred_cls", "pred_vid", "pred_seg", "pred_score",
                                                 "order", "ap")}
        c["dataset"] = str(d[name + "_dataset"])
        c["num_class"] = int(d[name + "_num_class"][0])
        c["thresholds"] = tiou_thresholds(c["dataset"])
        c["tp"] = np.unpackbits(d[name + "_tp"], axis=1)[:, :len(c["pred_score"])]
        cases[name] = c
    return d, cases


def run_flat(case, backend, **kw):
    return average_precision_flat(case["pred_seg"], case["pred_score"], case["pred_cls"], case["pred_vid"], case["gt_seg"],
                                  case["gt_cls"], case["gt_vid"], case["num_class"], case["thresholds"], device=backend.device, **kw)


def test_fixture_conditions():
    d, cases = fixture()
    assert os.path.getsize(GOLDEN) < 207109                        # below ref_tag.npz
    assert {c["dataset"] for c in cases.values()} == {"thumos14", "activitynet1.2"}
    for name, c in cases.items():
        for cls in range(c["num_class"]):
            s = c["pred_score"][c["pred_cls"] == cls]
            if name == "ties":
                assert len(np.unique(s)) < len(s)
            else:
                assert len(np.unique(s)) == len(s), (name, cls)
        assert c["pred_score"].dtype == np.float64 and c["tp"].shape == (len(c["thresholds"]), len(c["pred_score"]))
    m = cases["thumos_mixed"]
    assert (m["gt_cls"] == 3).any() and not (m["pred_cls"] == 3).any()             # ground truth, no predictions
    assert (m["pred_cls"] == 4).any() and not (m["gt_cls"] == 4).any()             # predictions, no ground truth
    assert np.isnan(m["ap"][4]).all() and (m["ap"][3] == 0).all() and not np.isnan(np.delete(m["ap"], 4, axis=0)).any()
    assert not np.isin(m["pred_vid"], m["gt_vid"]).all()                            # a video without any ground truth
    groups = {(c, v) for c, v in zip(m["pred_cls"], m["pred_vid"])}
    assert any(((m["pred_cls"] == c) & (m["pred_vid"] == v)).sum() == 1 for c, v in groups)      # a group with one prediction
    b = cases["big_group"]
    assert ((b["gt_cls"] == 0) & (b["gt_vid"] == 0)).sum() >= 300
    assert np.bincount(cases["long_class"]["pred_cls"]).max() > 2048
    g = cases["dup_gt"]
    rows = np.column_stack([g["gt_cls"], g["gt_vid"], g["gt_seg"]])
    assert len(np.unique(rows, axis=0)) < len(rows)
    # scores are not float32 values
    assert (cases["thumos_mixed"]["pred_score"].astype(np.float32).astype(np.float64) != cases["thumos_mixed"]["pred_score"]).any()
    x = cases["anet_excerpt"]
    s = ProposalSampler(os.path.join(HERE, "golden", "proposal_list_processed.txt"))
    assert [list(r) for r in zip(x["gt_cls"], x["gt_seg"][:, 0], x["gt_seg"][:, 1])] == [g[1:] for g in s.all_gt()]
    assert len(x["pred_score"]) == sum(len(v.proposals) for v in s.video_list)
    for name in ("recall_random", "recall_grid"):
        off_g, off_p = d[name + "_gt_off"], d[name + "_pr_off"]
        assert (np.diff(off_g) == 0).sum() == 1 and (np.diff(off_p) == 0).sum() == 1 and (np.diff(off_g) > 0).sum() > 5


def test_matching_is_exact_and_ap_within_bound(backend):
    """tp flags and score order equal the referee's on EVERY case; AP within 1e-12, NaN exactly where the referee has it."""
    _, cases = fixture()
    for name, c in sorted(cases.items()):
        r = run_flat(c, backend, return_matches=True)
        assert np.array_equal(r.order, c["order"]), name
        mism = int((r.tp != c["tp"]).sum())
        with np.errstate(invalid="ignore"):
            err = np.nanmax(np.abs(r.ap - c["ap"])) if not np.isnan(c["ap"]).all() else 0.0
        print("%s: %d flags differ, max |ap - expected| %.3g" % (name, mism, err))
        assert r.tp.dtype == np.uint8 and np.array_equal(r.tp, c["tp"]), name
        assert np.array_equal(np.isnan(r.ap), np.isnan(c["ap"])), name
        assert r.ap.shape == (c["num_class"], len(c["thresholds"])) and err <= AP_TOL, (name, err)


def test_tie_rule(backend):
    """Equal scores: lower flat index first.  Equal IoU (identical ground-truth rows): the flags do not depend on the twin."""
    _, cases = fixture()
    c = cases["ties"]
    r = run_flat(c, backend, return_matches=True)
    for cls in range(c["num_class"]):
        o = r.order[r.pred_off[cls]:r.pred_off[cls + 1]]
        s = c["pred_score"][o]
        assert (np.diff(s) <= 0).all() and (np.diff(o)[np.diff(s) == 0] > 0).all()
    g = cases["dup_gt"]
    flipped = dict(g)
    for k in ("gt_cls", "gt_vid", "gt_seg"):
        flipped[k] = g[k][::-1].copy()
    a, b = run_flat(g, backend, return_matches=True), run_flat(flipped, backend, return_matches=True)
    assert np.array_equal(a.tp, b.tp) and np.array_equal(a.order, b.order) and np.array_equal(a.tp, g["tp"])


def test_evaluator_means_and_classes_without_gt(backend):
    _, cases = fixture()
    c = cases["thumos_mixed"]
    ev = DetectionEvaluator(c["num_class"], c["thresholds"], device=backend.device)
    names = ["video_%d" % v for v in range(int(max(c["pred_vid"].max(), c["gt_vid"].max())) + 1)]
    for v in np.unique(c["pred_vid"]):
        rows = np.flatnonzero(c["pred_vid"] == v)
        dets = {int(k): np.column_stack([c["pred_seg"][rows[c["pred_cls"][rows] == k]], c["pred_score"][rows[c["pred_cls"][rows] == k]],
                                         np.zeros(((c["pred_cls"][rows] == k).sum(), 2))])
                for k in np.unique(c["pred_cls"][rows])}
        ev.add_video(names[v], dets)
    all_gt = [[names[v], int(k), float(s), float(e)] for k, v, (s, e) in zip(c["gt_cls"], c["gt_vid"], c["gt_seg"])]
    r = ev.evaluate(all_gt, return_matches=True)
    with np.errstate(invalid="ignore"):
        assert np.nanmax(np.abs(r.ap - c["ap"])) <= AP_TOL and np.array_equal(np.isnan(r.ap), np.isnan(c["ap"]))
    assert r.classes_without_gt == [4]
    # the plain means of the reference (:237, :247) carry the NaN of the class without ground truth
    assert np.isnan(r.map_per_iou).all() and np.isnan(r.average_map)
    assert np.array_equal(r.map_per_iou, r.ap.mean(axis=0), equal_nan=True)
    # the matches refer to the evaluator's own flat rows
    assert len(r.rows[0]) == len(c["pred_score"]) and r.tp.sum() == c["tp"].sum()
    assert sorted(zip(r.rows[0], r.rows[3])) == sorted(zip([names[v] for v in c["pred_vid"]], c["pred_score"]))
    with pytest.raises(ValueError):
        ev.add_video(names[0], {})


def test_invalid_inputs_raise_value_error(backend):
    _, cases = fixture()
    c = cases["one_by_one"]
    bad = dict(c)
    bad["gt_seg"] = c["gt_seg"].copy()
    bad["gt_seg"][0, 1] = bad["gt_seg"][0, 0]                       # zero-length ground truth
    with pytest.raises(ValueError, match="positive length"):
        run_flat(bad, backend)
    for spoil in (np.inf, np.nan, -np.inf):
        bad = dict(c)
        bad["pred_score"] = c["pred_score"].copy()
        bad["pred_score"][1] = spoil
        with pytest.raises(ValueError, match="not finite"):
            run_flat(bad, backend)
    bad = dict(c)
    bad["pred_cls"] = c["pred_cls"].copy()
    bad["pred_cls"][0] = 7
    with pytest.raises(ValueError):
        run_flat(bad, backend)
    with pytest.raises(ValueError, match="thresholds"):
        average_precision_flat(c["pred_seg"], c["pred_score"], c["pred_cls"], c["pred_vid"], c["gt_seg"], c["gt_cls"], c["gt_vid"],
                               1, np.linspace(0.1, 0.9, 33), device=backend.device)
    ev = DetectionEvaluator(3, [0.5], device=backend.device)
    with pytest.raises(ValueError, match="finite"):
        ev.add_video("v", {0: np.array([[0.0, 1.0, np.nan, 0, 0]])})
    # no predictions at all: AP 0 where there is ground truth, NaN elsewhere
    r = ev.evaluate([["v", 1, 0.1, 0.4]])
    assert np.array_equal(r.ap, np.array([[np.nan], [0.0], [np.nan]]), equal_nan=True) and r.classes_without_gt == [0, 2]


def test_bad_arguments_are_rejected_before_any_launch():
    """Checkable without a GPU: the real library validates on the host before it launches anything."""
    lib = _lib.SsnLibrary(pkg.build())
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert lib.cdll.ssn_eval_lds_gt() == 256
    with pytest.raises(RuntimeError, match="33 thresholds"):
        lib.call("ssn_eval_ap", p, p, p, p, 4, p, p, 1, 1, p, p, 33, 2, p, p, 4, 0, p, p, p, p, 1 << 20, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_eval_ap", None, None, None, None, 4, p, p, 1, 1, p, p, 3, 2, p, p, 4, 0, p, p, p, p, 1 << 20, None)
    with pytest.raises(RuntimeError, match="sort entries"):
        lib.call("ssn_eval_ap", p, p, p, p, 4, p, p, 1, 1, p, p, 3, 2, p, p, 2, 0, p, p, p, p, 1 << 20, None)
    with pytest.raises(RuntimeError, match="workspace"):
        lib.call("ssn_eval_ap", p, p, p, p, 4, p, p, 1, 1, p, p, 3, 2, p, p, 4, 0, p, p, p, p, 16, None)
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("ssn_eval_count", p, p, 4, 0, p, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("ssn_eval_recall", p, p, 1, p, p, 1, 0, p, 1, p, None)


def detection_cases():
    d = np.load(os.path.join(HERE, "golden", "ref_detection.npz"))
    for ci in range(int(d["n_cases"][0])):
        p, c, top_k, no_reg, with_reg = (int(v) for v in d["d%d_cfg" % ci])
        yield dict(rel=d["d%d_rel" % ci], act=d["d%d_act" % ci], comp=d["d%d_comp" % ci], reg=d["d%d_reg" % ci] if with_reg else None,
                   c=c, top_k=top_k, no_reg=bool(no_reg), thr=float(d["d%d_thr" % ci][0]),
                   finite=bool(np.isfinite(d["d%d_dets" % ci][:, 2]).all()))


def test_chain_from_post_processing(backend):
    """ref_detection.npz inputs as the videos of one dataset with seeded ground truth: process_video + add_video and
    process_video_device + add_video both give the AP the referee computes from process_video's rows on the host."""
    G = tools_module("make_eval_golden")
    cases = list(detection_cases())
    num_class = max(k["c"] for k in cases)
    thresholds = tiou_thresholds("thumos14")
    rs = np.random.RandomState(5)
    host_ev = DetectionEvaluator(num_class, thresholds, device=backend.device)
    dev_ev = DetectionEvaluator(num_class, thresholds, device=backend.device)
    flat, all_gt = [], []
    for vi, k in enumerate(cases):
        post = DetectionPostProcessor(k["c"], k["thr"], k["top_k"], k["no_reg"])
        args = (torch.from_numpy(k["rel"][None]), backend.put(torch.from_numpy(k["act"])), backend.put(torch.from_numpy(k["comp"])),
                backend.put(torch.from_numpy(k["reg"])) if k["reg"] is not None else None)
        dets, _ = post.process_video(*args, device=backend.device)
        (ddev, counts), _ = post.process_video_device(*args, device=backend.device)
        assert ddev.is_cuda == backend.is_gpu and counts.is_cuda == backend.is_gpu
        # the device rows equal the host rows exactly
        hd, hc = ddev.cpu().numpy(), counts.cpu().numpy()
        assert sorted(dets) == [c for c in range(k["c"]) if hc[c] > 0]
        for c, rows in dets.items():
            assert np.array_equal(hd[c, :hc[c]], rows, equal_nan=True)
        if not k["finite"]:
            with pytest.raises(ValueError, match="finite"):
                DetectionEvaluator(num_class, thresholds, device=backend.device).add_video("spoilt", dets)
            bad = DetectionEvaluator(num_class, thresholds, device=backend.device)
            bad.add_video("spoilt", (ddev, counts))
            with pytest.raises(ValueError, match="not finite"):
                bad.evaluate([["spoilt", 0, 0.1, 0.5]])
            continue
        vid = "video_%d" % vi
        host_ev.add_video(vid, dets)
        dev_ev.add_video(vid, (ddev, counts))
        for c, rows in sorted(dets.items()):
            flat.extend((c, vi, r[0], r[1], r[2]) for r in rows)
            # seeded ground truth: around some detections of the class, plus one span anywhere
            pick = rows[rs.randint(0, len(rows), 2), :2] + rs.uniform(-0.03, 0.03, (2, 2))
            for s, e in list(np.sort(np.clip(pick, 0, 1), axis=1)) + [np.sort(rs.uniform(0, 1, 2))]:
                if e > s:
                    all_gt.append([vid, c, float(s), float(e)])
    assert dev_ev._dev[0][1].is_cuda == backend.is_gpu                      # what the evaluator holds stayed on the device
    flat = np.array(flat)
    case = {"dataset": "thumos14", "num_class": num_class, "pred_cls": flat[:, 0].astype(np.int32),
            "pred_vid": flat[:, 1].astype(np.int32), "pred_seg": flat[:, 2:4].copy(), "pred_score": flat[:, 4].copy(),
            "gt_cls": np.array([g[1] for g in all_gt]), "gt_vid": np.array([int(g[0].split("_")[1]) for g in all_gt]),
            "gt_seg": np.array([g[2:] for g in all_gt])}
    for c in range(num_class):          # (the referee's order is only defined for distinct scores)
        s = case["pred_score"][case["pred_cls"] == c]
        assert len(np.unique(s)) == len(s)
    _, ref_tp, ref_ap = G.referee_dataset(case)
    assert ref_tp.any() and not np.isnan(ref_ap).all()
    for ev in (host_ev, dev_ev):
        r = ev.evaluate(all_gt, return_matches=True)
        with np.errstate(invalid="ignore"):
            err = np.nanmax(np.abs(r.ap - ref_ap))
        print("chain: max |ap - referee| %.3g" % err)
        assert np.array_equal(np.isnan(r.ap), np.isnan(ref_ap)) and err <= AP_TOL
        assert np.array_equal(r.tp, ref_tp)


def test_proposal_recall_matches_reference_functions(backend):
    d, _ = fixture()
    for name in ("recall_random", "recall_grid"):
        go, po = d[name + "_gt_off"], d[name + "_pr_off"]
        gt_list = [d[name + "_gt"][go[i]:go[i + 1]] for i in range(len(go) - 1)]
        pr_list = [d[name + "_pr"][po[i]:po[i + 1]] for i in range(len(po) - 1)]
        r = proposal_recall(pr_list, gt_list, d[name + "_thr"], device=backend.device)
        assert np.array_equal(r.hits, d[name + "_hits"]), name
        assert np.array_equal(r.totals, np.diff(go))
        assert (r.per_video_recall == d[name + "_recall"][:, 0]).all() and (r.per_inst_recall == d[name + "_recall"][:, 1]).all()
    # the comparison is strict: a proposal of IoU exactly 0.5 does not hit at 0.5
    r = proposal_recall([[(0.0, 1.0)]], [[(0.0, 2.0)]], [0.5, 0.49], device=backend.device)
    assert r.hits.tolist() == [[0, 1]]
    with pytest.raises(ValueError):
        proposal_recall([[(0.0, 1.0)], []], [[], []], [0.5], device=backend.device)


def test_calls_per_evaluate_do_not_grow(backend, monkeypatch):
    """The number of calls into the C library is the same for 1 class x 1 video and for the largest fixture case."""
    _, cases = fixture()
    calls = []
    for name in ("eval_count", "eval_ap", "eval_recall", "detections", "tag_count", "tag_generate", "tag_name_proposals"):
        def wrap(*a, _f=getattr(K, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, wrap)
    lib_calls = []
    lib = _lib.get_lib()
    real_call = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (lib_calls.append(name), real_call(name, *a))[1])
    seen = {}
    for name in ("one_by_one", max(cases, key=lambda n: len(cases[n]["pred_score"]))):
        del calls[:], lib_calls[:]
        run_flat(cases[name], backend)
        seen[name] = (list(calls), list(lib_calls))
    assert "one_by_one" in seen and len(seen) == 2
    a, b = seen.values()
    assert a == b and a[0] == ["eval_count", "eval_ap"] and a[1] == ["ssn_eval_count", "ssn_eval_ap"]


def test_thresholds_table_and_merge():
    assert np.array_equal(tiou_thresholds("activitynet1.2"), np.arange(0.5, 1.0, 0.05))
    assert np.array_equal(tiou_thresholds("thumos14"), np.arange(0.1, 1.0, 0.1))
    assert tiou_thresholds("thumos14").dtype == np.float64 and len(tiou_thresholds("activitynet1.2")) == 10
    with pytest.raises(ValueError):
        tiou_thresholds("thumos15")
    thr = tiou_thresholds("thumos14")
    m = np.array([0.66123, 0.6, 0.51237, 0.41, 0.29996, 0.2, 0.1, 0.05, 0.00004])
    rows = map_table_rows(thr, m)
    assert rows[0] == ["IoU thresh", "0.10", "0.20", "0.30", "0.40", "0.50", "0.60", "0.70", "0.80", "0.90", "Average"]
    assert rows[1] == ["mean AP", "0.6612", "0.6000", "0.5124", "0.4100", "0.3000", "0.2000", "0.1000", "0.0500", "0.0000",
                       "{:.04f}".format(m.mean())]
    text = format_map_table(thr, m, "Detection Performance on thumos14")
    lines = text.split("\n")
    assert "Detection Performance on thumos14" in lines[0] and len(lines) == 5
    assert [c.strip() for c in lines[1].strip("|").split("|")] == rows[0]
    assert [c.strip() for c in lines[3].strip("|").split("|")] == rows[1]
    assert lines[1].endswith("Average |") and lines[3].endswith(rows[1][-1] + " |")      # last column right-aligned

    # merge: against the loop of eval_detection_results.py:50-75
    rs = np.random.RandomState(0)
    files = []
    for f in range(3):
        files.append({v: (rs.uniform(0, 1, (1, 7, 2)), rs.standard_normal((7, 5)).astype(np.float32),
                          rs.standard_normal((7, 4)).astype(np.float32), None if v == "b" else rs.standard_normal((7, 4, 2)).astype(np.float32))
                      for v in ("a", "b")})
    for score_weights in (None, [1.0, 2.0, 0.5]):
        if score_weights:
            weights = np.array(score_weights) / sum(score_weights)
        else:
            weights = [1.0 / len(files) for _ in files]
        got = merge_detection_scores(files, score_weights)
        assert list(got) == ["a", "b"]
        for vid in ("a", "b"):
            arrays = [pc[vid] for pc in files]
            assert got[vid][0] is files[0][vid][0]
            for index in (1, 2, 3):
                if arrays[0][index] is not None:
                    want = np.sum([a[index] * w for a, w in zip(arrays, weights)], axis=0)
                    assert np.array_equal(got[vid][index], want)
                else:
                    assert got[vid][index] is None and vid == "b" and index == 3


def test_driver_end_to_end(emu, tmp_path, capsys):
    """tools/eval_detections.py on a two-video pickle (emulator tier): its table and its .npy equal the evaluator's output."""
    prop_file = os.path.join(HERE, "golden", "proposal_list_processed.txt")
    sampler = ProposalSampler(prop_file)
    rs = np.random.RandomState(3)
    num_class, scores = 100, []
    for f in range(2):
        pc = {}
        for v in sampler.video_list[:2]:
            p = 9
            start = rs.uniform(0, 0.6, p)
            rel = np.stack([start, start + rs.uniform(0.1, 0.4, p)], axis=1)
            rel[:3] = np.array([v.gt[0].start_frame, v.gt[0].end_frame]) / v.num_frames + rs.uniform(-0.02, 0.02, (3, 2))
            pc[v.id] = (np.clip(rel, 0, 1)[None], rs.standard_normal((p, num_class + 1)).astype(np.float32),
                        rs.standard_normal((p, num_class)).astype(np.float32), (rs.standard_normal((p, num_class, 2)) * 0.1).astype(np.float32))
            pc[v.id][1][:, v.gt[0].label] += 6.0                        # (the video's own class scores high)
        path = str(tmp_path / ("scores%d.pc" % f))
        with open(path, "wb") as fh:
            pickle.dump(pc, fh)
        scores.append(pc)
    out = str(tmp_path / "ap.npy")
    tool = tools_module("eval_detections")
    tool.main([str(tmp_path / "scores0.pc"), str(tmp_path / "scores1.pc"), "--proposal-list", prop_file, "--num-class", str(num_class),
               "--tiou", "activitynet1.2", "--nms_threshold", "0.6", "--top_k", "30", "--score_weights", "1", "3", "--ap-out", out])
    printed = capsys.readouterr().out
    merged = merge_detection_scores(scores, [1.0, 3.0])
    post = DetectionPostProcessor(num_class, 0.6, 30)
    ev = DetectionEvaluator(num_class, tiou_thresholds("activitynet1.2"), device="cpu")
    for vid, (rel, act, comp, reg) in merged.items():
        ev.add_video(vid, post.process_video(rel, torch.from_numpy(act), torch.from_numpy(comp), torch.from_numpy(reg))[0])
    want = ev.evaluate(sampler.all_gt())
    got = np.load(out)
    assert got.shape == (num_class, 10) and np.array_equal(got, want.ap, equal_nan=True)
    assert (~np.isnan(got)).any(axis=1).sum() == len({g[1] for g in sampler.all_gt()}) and np.nanmax(got) > 0
    for cell in map_table_rows(want.thresholds, want.map_per_iou)[1]:
        assert cell in printed
    assert "Average" in printed and "Detection Performance on activitynet1.2" in printed
