"""Video-level classification (csrc/video_cls.hip, video_cls.py) against tests/golden/ref_video_cls.npz, the outputs of the
reference's own ops.video_funcs / ops.metrics (tools/make_video_cls_golden.py), and the float64 restatement
tests/video_cls_referee.py.

Exact checks: on inputs whose entries are multiples of 2^-6 with |x| <= 8 every sum is exact in float32 in any order, so
selection, window maxima, crop means and the means over ticks must be bit-equal to the reference.  The reference's
sliding-window function only runs under Python 3 while no span has more than 60 windows (its ``n / 4`` is a float
there); those videos are compared with the ``max(15, n // 4)`` restatement, the Python 2 division the reference was
written for.  Tolerance checks: 4 x e_ref, e_ref = max |reference float32 - float64 restatement| measured by the
fixture generator on the same inputs (floor: one float32 ulp of the largest restatement value)."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import action_detection_amd  # noqa: F401
from action_detection_amd import kernels as K
from action_detection_amd.video_cls import (VideoClassScores, VideoScoreAggregator, classification_metrics, fuse_scores,
                                            window_plan)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import video_cls_referee as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_G = {}


def golden():
    if not _G:
        with np.load(os.path.join(ROOT, "tests", "golden", "ref_video_cls.npz")) as z:
            _G.update({k: z[k] for k in z.files})
    return _G


_BATCH = {}


def batch(kind, seed, c, crops):
    key = (kind, seed, c, crops)
    if key not in _BATCH:
        _BATCH[key] = (R.dyadic_batch if kind == "dyadic" else R.float_batch)(seed, c, crops)
    return _BATCH[key]


def put(backend, vids):
    return [backend.put(torch.from_numpy(v)) for v in vids]


def run(backend, vids, mode, **kw):
    return_spans = kw.pop("return_spans", False)
    return VideoScoreAggregator(mode, **kw).aggregate(put(backend, vids), return_spans=return_spans)


def same(t, ref):
    """torch.equal on values (the reference's float64 outputs are exact float32 values here)"""
    return torch.equal(t.cpu(), torch.from_numpy(np.asarray(ref, dtype=np.float32)))


def bound(e_ref, rest):
    return max(4 * float(e_ref), float(np.spacing(np.float32(np.abs(rest).max()))))


def mean_of_spans32(rows):
    """[V, S, C] -> [V, C]: the float32 rows added in order 0 ... S - 1 and divided once, as the reference's np.mean over
    its list of rows does"""
    acc = rows[:, 0].astype(np.float32)
    for s in range(1, rows.shape[1]):
        acc = acc + rows[:, s].astype(np.float32)
    return acc / np.float32(rows.shape[1])


def test_window_plan_is_the_reference_arithmetic():
    assert window_plan((1, 2, 4, 8, 16), 0.2, 1) == [(1, 1), (2, 2), (4, 4), (8, 7), (16, 13)] == R.plan(1)
    assert window_plan((1, 2, 4, 8, 16), 0.2, 3) == R.plan(3) == [(3, 3), (6, 5), (12, 10), (24, 20), (48, 39)]


@pytest.mark.parametrize("case", range(len(R.EXACT_CASES)), ids=["C%d_crops%d" % c for c in R.EXACT_CASES])
def test_exact_against_the_reference(backend, case):
    """default, top_k (k = 1, 5 and k >= every n), crop maximum and the sliding-window spans / results, bit for bit; the
    batch is ragged (T = 1 ... 1000) and its columns hold constant runs, three-valued columns, +-0.0 and negatives."""
    c, crops = R.EXACT_CASES[case]
    g, tag = golden(), "%d_%d" % R.EXACT_CASES[case]
    vids = batch("dyadic", 100 + case, c, crops)
    out = run(backend, vids, "default", normalization=False)
    assert same(out.scores, g["xd_" + tag]) and out.status.cpu().tolist() == [0] * len(vids)
    assert same(run(backend, vids, "top_k", k=1, normalization=False).scores, g["xk1_" + tag])
    assert same(run(backend, vids, "top_k", k=R.TOP_K, normalization=False).scores, g["xk_" + tag])
    assert same(run(backend, vids, "top_k", k=1000, normalization=False).scores, g["xd_" + tag])      # k = n and k > n
    if crops:
        assert same(run(backend, vids, "default", normalization=False, crop_agg="max").scores, g["xdmax_" + tag])
    for fps in (1, 3):
        out = run(backend, vids, "sliding_window", fps=fps, normalization=False, return_spans=True)
        ok = g["xok%d_%s" % (fps, tag)]
        assert ok.tolist() == [max(-(-t // step) for _, step in R.plan(fps)) <= 60 for t in R.TS]
        rows = np.where(ok[:, None, None], g["xs%d_%s" % (fps, tag)], np.stack([R.span_rows(v, fps) for v in vids]))
        assert same(out.spans, rows)
        res = mean_of_spans32(rows)
        assert same(out.scores, res) and np.array_equal(res[ok], g["xo%d_%s" % (fps, tag)][ok])


@pytest.mark.parametrize("case", range(len(R.TOL_CASES)), ids=["C%d_crops%d" % c for c in R.TOL_CASES])
def test_tolerance_against_float64(backend, case):
    """General floats, ten crops, softmax on: within 4 x e_ref of the float64 restatement.  Measured e_ref (fixture):
    default 8.8e-08, top_k 1.8e-07, sliding_window 9.3e-08."""
    c, crops = R.TOL_CASES[case]
    g = golden()
    vids = batch("float", 200 + case, c, crops)
    checks = [("default", {}, lambda v: R.agg_default(v, True)),
              ("top_k", dict(k=R.TOP_K), lambda v: R.agg_top_k(v, R.TOP_K, True)),
              ("sliding_window", dict(fps=1), lambda v: R.agg_sliding(v, 1, True)),
              ("sliding_window", dict(fps=3), lambda v: R.agg_sliding(v, 3, True))]
    for mode, kw, rest_fn in checks:
        out = run(backend, vids, mode, **kw).scores.cpu().numpy().astype(np.float64)
        rest = np.stack([rest_fn(v) for v in vids])
        err = np.abs(out - rest).max()
        print("%s %s: max error %.3e, bound %.3e" % (mode, kw, err, bound(g["e_" + mode], rest)))
        assert err <= bound(g["e_" + mode], rest), (mode, kw)


@pytest.mark.parametrize("mode,kw", [("top_k", dict(k=3)), ("sliding_window", dict(fps=1))])
def test_ties_at_the_cut_and_extreme_k(backend, mode, kw):
    """Hand-made columns: constant, a cut inside a run of equals, +-0.0 mixed, all negative, with n on both sides of the
    LDS tile; exactly min(k, n) entries are counted."""
    n = K.vcls_lds_rows()
    vids = []
    for t in (2, n, n + 1, 3 * n + 5):
        x = np.zeros((t, 4), dtype=np.float32)
        x[:, 0] = 1.25
        x[:, 1] = np.float32([2.0, -1.0, 2.0, 0.5])[np.arange(t) % 4]      # half the rows hold the maximum
        x[:, 2] = np.float32([0.0, -0.0, -3.0])[np.arange(t) % 3]
        x[:, 3] = -1 - (np.arange(t) % 7).astype(np.float32) / 8
        vids.append(x)
    res = run(backend, vids, mode, normalization=False, return_spans=mode == "sliding_window", **kw)
    if mode == "top_k":
        rest = np.stack([R.agg_top_k(v, 3, False) for v in vids]).astype(np.float32)
    else:
        rows = np.stack([R.span_rows(v, 1) for v in vids])
        assert same(res.spans, rows)
        rest = mean_of_spans32(rows)
    assert np.array_equal(res.scores.cpu().numpy(), rest)
    if mode == "top_k":
        for k in (1, n, 3 * n + 5):
            out = run(backend, vids, "top_k", k=k, normalization=False).scores.cpu().numpy()
            assert np.array_equal(out, np.stack([R.agg_top_k(v, k, False) for v in vids]).astype(np.float32)), k


def test_status_flags_only_the_bad_videos(backend):
    """A NaN and an Inf in one video, and an empty video: their rows are NaN and flagged, every other row equals the
    clean run bit for bit; two runs are bit-identical; check() names the videos."""
    vids = [v.copy() for v in batch("float", 200, 7, 1)]
    names = ["v%d" % i for i in range(len(vids))]
    for mode, kw in (("default", {}), ("top_k", dict(k=4)), ("sliding_window", {})):
        agg = VideoScoreAggregator(mode, **kw)
        clean = agg.aggregate(dict(zip(names, put(backend, vids))))
        again = agg.aggregate(dict(zip(names, put(backend, vids))))
        assert torch.equal(clean.scores, again.scores) and clean.check() is clean
        dirty = [v.copy() for v in vids]
        dirty[5][7, 0, 2] = np.nan
        dirty[5][9, 0, 3] = np.inf
        dirty[8] = dirty[8][:0]
        out = agg.aggregate(dict(zip(names, put(backend, dirty))))
        st = out.status.cpu().tolist()
        assert st == [1 if i == 5 else 2 if i == 8 else 0 for i in range(len(vids))]
        keep = torch.tensor([i not in (5, 8) for i in range(len(vids))])
        assert torch.equal(out.scores.cpu()[keep], clean.scores.cpu()[keep])
        assert bool(torch.isnan(out.scores.cpu()[~keep]).all())
        with pytest.raises(ValueError, match="v5=1, v8=2"):
            out.check()


def test_nothing_outside_the_results_is_written(backend):
    """Outputs and the window workspace sit between NaN-filled guards; the kernels write the result and nothing else."""
    vids = batch("dyadic", 100, 65, 2)[:8]
    ts = [v.shape[0] for v in vids]
    h_off = torch.tensor(np.concatenate([[0], np.cumsum(ts)]), dtype=torch.int32)
    raw = backend.put(torch.from_numpy(np.concatenate(vids)))
    guard = 300

    def guarded(rows, c):
        buf = torch.full((rows * c + 2 * guard,), float("nan"), dtype=torch.float32, device=raw.device)
        return buf, buf[guard:guard + rows * c].view(rows, c)

    def intact(buf):
        return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all())

    n = raw.shape[0]
    b_frm, frm = guarded(n, 65)
    K.vcls_crop_reduce(raw, out=frm)
    plan = R.plan(1)
    counts = [-(-t // step) for t in ts for _, step in plan]
    h_win = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    b_win, win = guarded(int(h_win[-1]), 65)
    dev = raw.device
    K.vcls_window_max(frm, h_off, h_win, torch.tensor([p[0] for p in plan], dtype=torch.int32).to(dev),
                      torch.tensor([p[1] for p in plan], dtype=torch.int32).to(dev), out=win)
    b_sp, sp = guarded(len(counts), 65)
    K.vcls_topk_mean(win, h_win, torch.tensor([max(15, x // 4) for x in counts], dtype=torch.int32), out=sp)
    b_out, out = guarded(len(ts), 65)
    K.vcls_finish(sp.view(len(ts), len(plan), 65), 0, divide=True, softmax=True, out=out)
    for buf in (b_frm, b_win, b_sp, b_out):
        assert intact(buf) and not bool(torch.isnan(buf[guard:-guard]).any())
    direct = VideoScoreAggregator("sliding_window").aggregate(put(backend, vids))
    assert torch.equal(direct.scores, out)


def test_calls_do_not_grow_with_the_videos(backend, monkeypatch):
    """The number of calls into the C library is the same for V = 1 and V = 12."""
    from action_detection_amd import _lib
    lib = _lib.get_lib()
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    vids = batch("float", 201, 65, 10)
    for mode, kw in (("default", {}), ("top_k", dict(k=3)), ("sliding_window", {})):
        seen = []
        for sub in (vids[5:6], vids):
            del calls[:]
            run(backend, sub, mode, **kw)
            seen.append(list(calls))
        assert seen[0] == seen[1] and 3 <= len(seen[0]) <= 5, seen


def test_argument_errors_raise_before_any_launch(backend, monkeypatch):
    from action_detection_amd import _lib
    lib = _lib.get_lib()
    calls = []
    monkeypatch.setattr(lib, "call", lambda name, *a: calls.append(name))
    x = backend.put(torch.zeros((6, 2, 4)))
    off = torch.tensor([0, 2, 6], dtype=torch.int32)
    with pytest.raises(ValueError):
        VideoScoreAggregator("median")
    with pytest.raises(ValueError):
        VideoScoreAggregator("top_k")
    with pytest.raises(ValueError):
        VideoScoreAggregator("top_k", k=0)
    with pytest.raises(ValueError):
        VideoScoreAggregator("default", crop_agg="median")
    with pytest.raises(ValueError):
        VideoScoreAggregator("tpp")
    with pytest.raises(ValueError, match="multiple"):
        VideoScoreAggregator("tpp", num_class=3).aggregate([x])
    with pytest.raises(ValueError):
        VideoScoreAggregator().aggregate([x.double()])
    with pytest.raises(ValueError):
        VideoScoreAggregator().aggregate([x[:, 0, 0]])
    with pytest.raises(ValueError):
        VideoScoreAggregator().aggregate([x, x[:, :1]])
    with pytest.raises(ValueError):
        VideoScoreAggregator().aggregate([x[:, :, :0]])
    with pytest.raises(ValueError):
        VideoScoreAggregator().aggregate([])
    with pytest.raises(ValueError, match="ascend"):
        K.vcls_status(x, torch.tensor([0, 4, 2, 6], dtype=torch.int32))
    with pytest.raises(ValueError, match="ascend"):
        K.vcls_topk_mean(x[:, 0].contiguous(), torch.tensor([0, 2, 5], dtype=torch.int32), torch.tensor([1, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        K.vcls_topk_mean(x[:, 0].contiguous(), off.long(), torch.tensor([1, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="k must be"):
        K.vcls_topk_mean(x[:, 0].contiguous(), off, torch.tensor([1, 0], dtype=torch.int32))
    with pytest.raises(ValueError):
        K.vcls_crop_reduce(x[:, 0].contiguous())
    with pytest.raises(ValueError, match="multiple"):
        K.vcls_tpp(x[:, 0].contiguous(), off, 3)
    s = {"a": np.zeros(4, np.float32), "b": np.ones(4, np.float32)}
    with pytest.raises(ValueError, match="weights"):
        fuse_scores(s, [s, s], [1.0])
    with pytest.raises(ValueError):
        classification_metrics(s, {"a": [0, 1], "b": [2]})
    with pytest.raises(ValueError):
        classification_metrics(s, {"a": [4]})
    with pytest.raises(ValueError):
        classification_metrics(s, {"a": [0]}, top_k=(0,))
    assert calls == []


def test_c_abi_refuses_bad_sizes(backend):
    from action_detection_amd import _lib
    lib = _lib.get_lib()
    p = backend.put(torch.zeros(64)).data_ptr()
    for name, args in (("ssn_vcls_status", (p, p, 0, 4, 1, p, None)), ("ssn_vcls_crop_reduce", (p, p, 4, 0, 1, 0, None)),
                       ("ssn_vcls_topk_mean", (p, p, p, 1, 4, 0, p, None)), ("ssn_vcls_tpp", (p, p, 1, 4, 1, 0, p, None)),
                       ("ssn_vcls_finish", (p, None, None, 1, 0, 1, 1, 1, 0, 0, p, None)),
                       ("ssn_vcls_window_max", (p, p, p, p, p, 1, 0, 4, 1, 1, p, None)),
                       ("ssn_vcls_metrics", (p, p, None, p, 1, 1, 1, p, p, p, p, 0, None))):
        with pytest.raises(RuntimeError):
            lib.call(name, *args)


def test_tpp_stage_indices(backend):
    """One-hot probes: entry i of the aggregate is k_i + 1, the stage index used for frame i, for every i -- equal to
    what the reference's tpp_aggregation_func used (int(t * (stages / T)) in float64)."""
    g = golden()
    for t, stages in R.TPP_PROBES:
        out = VideoScoreAggregator("tpp", num_class=t).aggregate([backend.put(torch.from_numpy(R.tpp_probe(t, stages)))])
        assert same(out.scores[0], g["tpp_%d_%d" % (t, stages)]), (t, stages)
    # a ragged batch in one call, [T, C] input, against the float64 restatement.  Bound: the kernel adds ceil(T / 4) + 2
    # float32 terms per class and divides once, each rounding at most 2^-24 of the running magnitude <= sum |x|.
    rs = np.random.RandomState(7)
    vids = [rs.randn(t, 3 * 7).astype(np.float32) for t in (1, 2, 5, 64, 257)]
    out = VideoScoreAggregator("tpp", num_class=7).aggregate(put(backend, vids)).scores.cpu().numpy()
    for o, v in zip(out, vids):
        t = v.shape[0]
        tol = (-(-t // 4) + 3) * 2.0 ** -24 * np.abs(v).sum(axis=0).reshape(3, 7).sum(axis=0).max() / t
        assert np.abs(o - R.agg_tpp(v, 7)).max() <= tol


@pytest.mark.parametrize("n_other", [1, 2])
def test_fusion(backend, n_other):
    g = golden()
    ids = ["v%d" % i for i in range(len(R.TS))]

    def stream(a, order=None):
        order = range(len(ids)) if order is None else order
        return VideoClassScores([ids[i] for i in order], backend.put(torch.from_numpy(np.ascontiguousarray(a[list(order)]))))

    dy, w = g["fuse_dyadic"], [float(x) for x in g["fuse_w_dyadic"][:n_other]]
    rev = list(reversed(range(len(ids))))
    out = fuse_scores(stream(dy[0]), [stream(dy[1 + i], rev if i == 0 else None) for i in range(n_other)], w, norm=False)
    assert out.ids == ids and same(out.scores, g["fuse_exact_%d" % n_other])      # (matched by id, not by row)
    st, w = g["fuse_streams"], [float(x) for x in g["fuse_w"][:n_other]]
    for norm in (False, True):
        out = fuse_scores(stream(st[0]), [stream(st[1 + i]) for i in range(n_other)], w, norm=norm)
        rest = np.stack([R.fuse(st[0][j], [s[j] for s in st[1:1 + n_other]], w, norm) for j in range(len(ids))])
        err = np.abs(out.scores.cpu().numpy() - rest).max()
        print("fusion %d norm %s: max error %.3e, bound %.3e" % (n_other, norm, err, bound(g["e_fusion"], rest)))
        assert err <= bound(g["e_fusion"], rest)
    short = VideoClassScores(ids[:-1], backend.put(torch.from_numpy(st[1][:-1].copy())))
    with pytest.raises(KeyError, match="v11"):
        fuse_scores(stream(st[0]), [short], [1.0])


@pytest.mark.parametrize("name,kw", [("m1", dict(seed=1, v=40, c=11)), ("m4", dict(seed=4, v=45, c=9, multi=True)),
                                     ("m5", dict(seed=5, v=300, c=140)), ("m2", dict(seed=2, v=30, c=6, ties=True))])
def test_metrics_against_the_reference(backend, name, kw):
    """top_k_accuracy and mean_class_accuracy equal the reference's functions exactly; the AP per class and the macro
    mean are within 1e-12 of sklearn's average_precision_score (m2: tied scores, which sklearn groups into one
    threshold; its top-k is checked against the stated stable rule)."""
    g = golden()
    s, sets = R.metric_case(**kw)
    scores = VideoClassScores(["v%d" % i for i in range(len(s))], backend.put(torch.from_numpy(s)))
    labels = {"v%d" % i: lb for i, lb in enumerate(sets)}
    labels["absent"] = [0]                                    # a labelled video without scores is left out
    m = classification_metrics(scores, labels, top_k=(1, 3, 5), class_accuracy=not kw.get("multi"))
    assert m.videos_scored == len(s)
    got = [m.top_k_accuracy[k] for k in (1, 3, 5)]
    if kw.get("ties"):
        assert got == [R.stable_top_k_hit_rate(s, sets, k) for k in (1, 3, 5)]
    else:
        assert got == g[name + "_topk"].tolist()
    assert np.abs(m.ap - g[name + "_ap"]).max() <= 1e-12 and abs(m.mean_ap - float(g[name + "_map"])) <= 1e-12
    if kw.get("multi"):
        assert m.mean_class_accuracy is None
        with pytest.raises(ValueError, match="one label"):
            classification_metrics(scores, labels)
    else:
        assert m.mean_class_accuracy == float(g[name + "_mca"])


def test_metrics_edge_rules(backend):
    """A class that is only predicted gives NaN (as the reference's confusion matrix does); a class without a positive
    video has AP NaN; equal scores: the higher class index ranks higher."""
    g = golden()
    s, sets = R.predicted_only_case()
    m = classification_metrics({i: s[i] for i in range(len(s))}, {i: lb for i, lb in enumerate(sets)})
    assert np.isnan(m.mean_class_accuracy) and np.isnan(g["m3_mca"])
    assert np.isnan(m.ap[8]) and np.isnan(m.mean_ap)
    tied = {"a": np.float32([1, 1, 1, 0]), "b": np.float32([0, 2, 2, 2])}
    m = classification_metrics(tied, {"a": [2], "b": [1]}, top_k=(1, 2, 3), class_accuracy=False)
    assert m.top_k_accuracy == {1: 0.5, 2: 0.5, 3: 1.0}      # a: 2 is top-1; b: ranks 3 > 2 > 1, class 1 is third


def test_save_load_and_the_detection_filter(backend, tmp_path):
    """save -> load round trip; the saved file given to tools/eval_detections.py --cls_scores on a two-video score pickle
    changes which classes get detections exactly as video_cls_score= does when it is given directly."""
    import importlib.util
    from action_detection_amd.detection_eval import DetectionEvaluator, tiou_thresholds
    from action_detection_amd.detection_post import DetectionPostProcessor
    from action_detection_amd.proposal_sampling import ProposalSampler
    spec = importlib.util.spec_from_file_location("eval_detections_tool", os.path.join(ROOT, "tools", "eval_detections.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    prop_file = os.path.join(ROOT, "tests", "golden", "proposal_list_processed.txt")
    sampler = ProposalSampler(prop_file)
    rs = np.random.RandomState(11)
    c, vids = 100, sampler.video_list[:2]
    ticks = {}
    for i, v in enumerate(vids):
        x = rs.randn(20 + 5 * i, 2, c).astype(np.float32)
        x[:, :, v.gt[0].label if i == 0 else (v.gt[0].label + 1) % c] += 4.0      # right for the first video, wrong for the second
        ticks[v.id] = backend.put(torch.from_numpy(x))
    cls = VideoScoreAggregator("top_k", k=3).aggregate(ticks)
    path = str(tmp_path / "cls.pc")
    cls.save(path)
    with open(path, "rb") as f:
        raw = pickle.load(f)
    assert sorted(raw) == sorted(str(v.id) for v in vids)
    assert all(isinstance(k, str) and a.dtype == np.float32 and a.shape == (c,) for k, a in raw.items())
    back = VideoClassScores.load(path, device=backend.device)
    assert back.ids == [str(i) for i in cls.ids] and torch.equal(back.scores.cpu(), cls.scores.cpu())
    det = {}
    for v in vids:
        p = 9
        start = rs.uniform(0, 0.6, p)
        rel = np.stack([start, start + rs.uniform(0.1, 0.4, p)], axis=1)
        rel[:3] = np.array([v.gt[0].start_frame, v.gt[0].end_frame]) / v.num_frames + rs.uniform(-0.02, 0.02, (3, 2))
        det[v.id] = (np.clip(rel, 0, 1)[None], rs.standard_normal((p, c + 1)).astype(np.float32),
                     rs.standard_normal((p, c)).astype(np.float32), (rs.standard_normal((p, c, 2)) * 0.1).astype(np.float32))
    det_path = str(tmp_path / "det.pc")
    with open(det_path, "wb") as f:
        pickle.dump(det, f, 2)
    argv = [det_path, "--proposal-list", prop_file, "--num-class", str(c), "--tiou", "activitynet1.2", "--nms_threshold", "0.6",
            "--device", str(backend.device)]
    with_file = tool.main(argv + ["--cls_scores", path])
    host = cls.to_host()
    dev = torch.device(backend.device)
    post = DetectionPostProcessor(c, 0.6, cls_top_k=1)
    ev = DetectionEvaluator(c, tiou_thresholds("activitynet1.2"), device=dev)
    for v in vids:
        rel, act, comp, reg = det[v.id]
        dets, _ = post.process_video_device(rel, torch.from_numpy(act).to(dev), torch.from_numpy(comp).to(dev),
                                            torch.from_numpy(reg).to(dev), device=dev, video_cls_score=host[v.id])
        assert [k for k in range(c) if int(dets[1][k]) > 0] == [int(np.argsort(host[v.id], kind="stable")[-1])]
        ev.add_video(v.id, dets)
        plain, _ = post.process_video_device(rel, torch.from_numpy(act).to(dev), torch.from_numpy(comp).to(dev),
                                             torch.from_numpy(reg).to(dev), device=dev)
        assert int((plain[1] > 0).sum()) > 1                      # (without the classifier every class reports)
    want = ev.evaluate(sampler.all_gt())
    assert np.array_equal(with_file.ap, want.ap, equal_nan=True)
