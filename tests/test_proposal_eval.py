"""AR-AN proposal evaluation (action_detection_amd.proposal_eval, csrc/proposal_eval.hip) against the numpy referee of
tests/proposal_eval_referee.py -- a restatement of the ActivityNet toolkit's average_recall_vs_avg_nr_proposals.

Bars: first_hit, matches, positives, total_proposals, recall and proposals_per_video EXACTLY (integers, an integer divided
by an integer in fp64, single IEEE operations); avg_recall and auc to 1e-12 relative (their sums' order is the kernel's
own -- the project's bar for AP).  Every kernel test runs on the host emulator and, marked gpu, on the MI355X.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import proposal_eval_referee as R
from action_detection_amd import kernels as K
from action_detection_amd import proposal_eval as PE
from action_detection_amd.proposal_lists import ProposalListBuilder, windows_per_video

_REFEREE = {}


def referee(key, make):
    """The referee's result of a case, computed once and shared by the emulator and the GPU run."""
    if key not in _REFEREE:
        _REFEREE[key] = make()
    return _REFEREE[key]


def assert_equal_to_referee(res, ref):
    assert np.array_equal(res.first_hit, ref["first_hit"])
    assert np.array_equal(res.matches, ref["matches"]) and res.matches.dtype == np.int64
    assert res.positives == ref["positives"] and res.total_proposals == ref["total_proposals"]
    assert np.array_equal(res.recall, ref["recall"])
    assert np.array_equal(res.proposals_per_video, ref["proposals_per_video"])
    assert np.array_equal(res.thresholds, ref["thresholds"])
    assert (np.abs(res.avg_recall - ref["avg_recall"]) <= 1e-12 * np.abs(ref["avg_recall"])).all()
    assert abs(res.auc - ref["auc"]) <= 1e-12 * abs(ref["auc"])


def dyadic_case(seed, ms, ns):
    """Videos with ms[i] proposals and ns[i] ground-truth spans on the grid of integers / 64.  Half of the proposals are
    the first half, the first three quarters or the whole of a ground-truth span of their video, or one shifted a
    little (tIoUs exactly on 0.5, 0.75 and 1, and near them); the rest lie anywhere."""
    rs = np.random.RandomState(seed)
    pr, gt = [], []
    for m, n in zip(ms, ns):
        s = rs.randint(0, 64 * 50, n)
        length = 8 * rs.randint(1, 64, n)
        g = np.stack([s, s + length], axis=1).astype(np.float64).reshape(-1, 2)
        p = np.zeros((m, 2))
        for k in range(m):
            if n and rs.rand() < 0.5:
                a, b = g[rs.randint(n)]
                frac = (0.5, 0.75, 1.0)[rs.randint(3)]
                shift = (0, 0, 1, -3)[rs.randint(4)]
                p[k] = (a + shift, a + shift + (b - a) * frac)
            else:
                a = rs.randint(0, 64 * 60)
                p[k] = (a, a + rs.randint(1, 64 * 8))
        pr.append(p / 64.0)
        gt.append(g / 64.0)
    return pr, gt


# ---------------------------------------------------------------------------------------------------------------- 1
WORKED_GT = [[(0, 10), (20, 30)], [(0, 8)], [], [(5, 6)]]
WORKED_PR = [[(0, 5), (0, 10), (21, 29), (40, 50)], [(0, 6), (1, 8)], [(0, 1), (2, 3)], []]


def test_worked_example(backend):
    """The example of DESIGN.md: tIoUs of exactly 0.5 and 0.75 (hence >=), a video without ground truth, a video without
    proposals and a truncated video; literal change points and area."""
    res = PE.proposal_ar_an(WORKED_PR, WORKED_GT, max_avg_nr_proposals=2, thresholds=[0.5, 0.75], device=backend.device)
    ref = referee("worked", lambda: R.ar_an(WORKED_PR, WORKED_GT, max_avg_nr_proposals=2, thresholds=[0.5, 0.75]))
    assert_equal_to_referee(res, ref)
    assert res.num_videos == 3 and res.positives == 4 and res.total_proposals == 4
    assert res.first_hit.tolist() == [[0, 1], [2, 2], [0, 0], [-1, -1]]
    want = np.zeros((2, 100))
    want[0, 22:] = 0.25
    want[1, 44:] = 0.25
    want[:, 66:] = 0.75
    assert np.array_equal(res.recall, want)
    assert np.array_equal(res.matches, (want * 4).astype(np.int64))
    assert res.proposals_per_video[99] == 2.0
    assert np.array_equal(res.proposals_per_video, (np.arange(1, 101) / 100.0 * 1.5) * (4.0 / 3))
    assert abs(res.auc - 0.33375) <= 1e-12 * 0.33375
    assert res.ar_at(2.0) == res.avg_recall[99] == 0.75 and res.ar_at(1e9) == 0.75
    assert np.array_equal(res.recall_vs_tiou(2.0), [0.75, 0.75])
    lo, hi = res.proposals_per_video[21], res.proposals_per_video[22]
    assert abs(res.recall_vs_tiou((lo + hi) / 2)[0] - 0.125) < 1e-12
    text = PE.format_ar_an_report(res)
    assert text.split("\n") == ["AR-AN: 3 videos, 4 groundtruth boxes, 4 proposals, 2.00 per video at the last point",
                                "AR@1: %.2f" % (res.ar_at(1) * 100), "tIoU 0.50. recall@2.00: 75.00",
                                "tIoU 0.75. recall@2.00: 75.00", "AUC: 33.38"]


# ---------------------------------------------------------------------------------------------------------------- 2
def edge_case(name):
    """-> (pr, gt, thresholds, points, pinned video or None)."""
    sizes_m = [0, 1, 63, 64, 65, 129]          # (with 0, 1, 2 and 65 ground-truth spans)
    if name == "v1_t1_j1":
        pr, gt = dyadic_case(1, [129], [65])
        return pr, gt, [0.5], 1, None
    if name == "v3_t32_j100":
        pr, gt = dyadic_case(2, [65, 0, 64], [2, 1, 0])
        return pr, gt, np.linspace(0.05, 0.98, 32), 100, None
    assert name == "v300_t10_j100"
    ms = [sizes_m[i % 6] for i in range(300)]
    ns = [65 if i in (4, 77, 203) else (1, 2, 0, 1, 2, 1, 1)[i % 7] for i in range(300)]
    assert {(m, n) for m, n in zip(ms, ns)} >= {(65, 65), (129, 65), (0, 1), (1, 2), (63, 0), (64, 1), (129, 2)}
    pr, gt = dyadic_case(3, ms, ns)
    # video 300: span 0 reaches the thresholds up to 0.6 at rank 5 and the others only at rank 128, in the third chunk of 64
    # ranks; span 1 is never hit
    p = np.stack([1000.0 + np.arange(140), 1001.0 + np.arange(140)], axis=1)
    p[5] = (0, 40)
    p[128] = (0, 64)
    pr.append(p)
    gt.append(np.asarray([(0.0, 64.0), (5000.0, 5001.0)]))
    return pr, gt, None, 100, 300


@pytest.mark.parametrize("name", ["v1_t1_j1", "v3_t32_j100", "v300_t10_j100"])
def test_chunk_and_staging_edges(backend, name):
    pr, gt, thr, points, pinned = edge_case(name)
    # (a maximum above the mean: no video is truncated, so the sizes are those the kernel's chunks see)
    ref = referee(name, lambda: R.ar_an(pr, gt, max_avg_nr_proposals=1000, thresholds=thr, points=points))
    res = PE.proposal_ar_an(pr, gt, max_avg_nr_proposals=1000, thresholds=thr, points=points, device=backend.device)
    assert_equal_to_referee(res, ref)
    assert res.total_proposals == sum(len(p) for p, g in zip(pr, gt) if len(g))
    assert res.recall.shape == (len(res.thresholds), points) and res.first_hit.shape == (res.positives, len(res.thresholds))
    assert (res.first_hit >= 0).any()
    if pinned is not None:
        rows = res.first_hit[-2:]
        assert rows[0].tolist() == [5, 5, 5] + [128] * 7          # 40 / 64 = 0.625: settles 0.5, 0.55, 0.6 in the first chunk
        assert rows[1].tolist() == [-1] * 10
        assert (res.first_hit >= 64).sum() >= 7 and (res.first_hit == -1).sum() >= 10


# ---------------------------------------------------------------------------------------------------------------- 3
TRUNC_MS = [40, 1, 2, 3, 8, 0, 25, 2, 17, 1, 64, 5]
TRUNC_NS = [2, 1, 1, 3, 0, 2, 1, 2, 4, 0, 3, 1]


@pytest.mark.parametrize("max_avg", [3, 100, None])
def test_truncation(backend, max_avg):
    pr, gt = dyadic_case(4, TRUNC_MS, TRUNC_NS)
    thr = [0.5, 0.75, 0.9]
    ties = 0
    for p, g in zip(pr, gt):
        for span in g:
            if len(p):
                iou = R.segment_iou(span, p)
                ties += int(((iou == 0.5) | (iou == 0.75)).sum())
    assert ties >= 5
    m, n = np.asarray(TRUNC_MS), np.asarray(TRUNC_NS)
    v, p_total = int((n >= 1).sum()), int(m.sum())
    use = float(p_total) / v if max_avg is None else max_avg
    ratio = use * float(v) / p_total
    nr = [min(int(mi * ratio), mi) for mi, ni in zip(m, n) if ni >= 1]
    kept = [mi for mi, ni in zip(m, n) if ni >= 1]
    if max_avg == 3:
        assert any(a == 0 and b > 0 for a, b in zip(nr, kept)) and any(0 < a < b for a, b in zip(nr, kept))
    elif max_avg == 100:
        assert ratio > 1 and nr == kept
    ref = referee(("trunc", max_avg), lambda: R.ar_an(pr, gt, max_avg_nr_proposals=max_avg, thresholds=thr))
    res = PE.proposal_ar_an(pr, gt, max_avg_nr_proposals=max_avg, thresholds=thr, device=backend.device)
    assert_equal_to_referee(res, ref)
    assert res.total_proposals == sum(nr)
    # a tie counts: with the thresholds moved up by one ulp the ties no longer do
    up = PE.proposal_ar_an(pr, gt, max_avg_nr_proposals=max_avg, thresholds=np.nextafter(thr, 1.0), device=backend.device)
    assert (up.matches <= res.matches).all() and (max_avg == 3 or (up.first_hit[:, :2] != res.first_hit[:, :2]).any())


# ---------------------------------------------------------------------------------------------------------------- 4
def scored_case():
    ms, ns = [2049, 70, 0, 5, 33], [2, 3, 1, 0, 1]
    pr, gt = dyadic_case(5, ms, ns)
    rs = np.random.RandomState(6)
    scores = [np.round(rs.uniform(-1, 1, m), 1) for m in ms]          # one decimal: many equal scores
    scores[1][:4] = [0.0, -0.0, 0.0, -0.0]                            # (-0.0 and 0.0 compare equal: input order)
    return pr, gt, scores


def test_scores_rank_the_proposals(backend):
    pr, gt, scores = scored_case()
    assert max(len(p) for p in pr) > 2048 and any(len(np.unique(s)) < len(s) / 2 for s in scores if len(s))
    ref = referee("scores", lambda: R.ar_an(pr, gt, scores=scores, max_avg_nr_proposals=600))
    res = PE.proposal_ar_an(pr, gt, scores=scores, max_avg_nr_proposals=600, device=backend.device)
    assert_equal_to_referee(res, ref)
    order = [R.stable_descending(s) for s in scores]
    presorted = PE.proposal_ar_an([p[o] for p, o in zip(pr, order)], gt, max_avg_nr_proposals=600, device=backend.device)
    for name in ("first_hit", "matches", "recall", "avg_recall", "proposals_per_video"):
        assert np.array_equal(getattr(res, name), getattr(presorted, name)), name
    assert res.auc == presorted.auc
    # the input order alone (no scores) ranks differently
    assert not np.array_equal(PE.proposal_ar_an(pr, gt, max_avg_nr_proposals=600, device=backend.device).first_hit, res.first_hit)


def test_rank_kernel_orders_by_score_then_index(backend):
    _, _, scores = scored_case()
    m = np.asarray([len(s) for s in scores], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(m)])
    sort_off = PE._rank_tables(m)
    assert sort_off.tolist() == [0, 4096, 4096 + 128, 4096 + 128, 4096 + 128 + 8, 4096 + 128 + 8 + 64]
    order = K.proposal_eval_rank(backend.put(torch.from_numpy(np.concatenate(scores))),
                                 backend.put(torch.from_numpy(off.astype(np.int32))),
                                 backend.put(torch.from_numpy(sort_off)), int(sort_off[-1])).cpu().numpy()
    want = np.concatenate([off[i] + R.stable_descending(s) for i, s in enumerate(scores)])
    assert np.array_equal(order, want)


# ---------------------------------------------------------------------------------------------------------------- 5
def batch_case():
    ms, ns = [65, 0, 129, 7, 64], [2, 1, 3, 0, 1]
    pr, gt = dyadic_case(7, ms, ns)
    videos = [SimpleNamespace(id="v%d" % i, duration=100.0,
                              instances=[SimpleNamespace(num_label=0, time_span=(float(a), float(b))) for a, b in g])
              for i, g in enumerate(gt)]
    return pr, gt, videos


def test_batch_form_equals_the_list_form(backend):
    pr, gt, videos = batch_case()
    builder = ProposalListBuilder(device=backend.device)
    batch = builder.from_spans(videos, pr)
    lists = PE.proposal_ar_an(pr, gt, device=backend.device)
    assert_equal_to_referee(lists, referee("batch", lambda: R.ar_an(pr, gt)))
    for res in (PE.proposal_ar_an_batch(batch), PE.proposal_ar_an_batch(batch, gt=gt), PE.proposal_ar_an_batch(batch)):
        for name in ("first_hit", "matches", "recall", "avg_recall", "proposals_per_video", "thresholds"):
            assert np.array_equal(getattr(res, name), getattr(lists, name)), name      # (bit-identical, repeats included)
        assert (res.auc, res.positives, res.total_proposals, res.num_videos) == \
            (lists.auc, lists.positives, lists.total_proposals, lists.num_videos)
    # a video's first_hit rows alone and inside the batch (no truncation in either: the maximum is far above the mean)
    whole = PE.proposal_ar_an_batch(batch, max_avg_nr_proposals=1e6, thresholds=[0.5, 0.75], points=7)
    g_off = np.concatenate([[0], np.cumsum([len(g) for g in gt])])
    for i in (0, 2, 4):
        alone = PE.proposal_ar_an_batch(builder.from_spans([videos[i]], [pr[i]]), max_avg_nr_proposals=1e6,
                                        thresholds=[0.5, 0.75], points=7)
        assert np.array_equal(alone.first_hit, whole.first_hit[g_off[i]:g_off[i + 1]])
    # sliding windows stay on the device too; their order is taken as the rank
    sw = builder.sliding_windows(videos, overlap=0.5, max_level=6)
    assert np.array_equal(PE.proposal_ar_an_batch(sw, points=20).matches,
                          PE.proposal_ar_an(windows_per_video(sw), gt, points=20, device=backend.device).matches)


# ---------------------------------------------------------------------------------------------------------------- 8
def test_argument_errors():
    """Everything the host refuses before it touches a device or the library."""
    pr, gt = [[(0, 1)], [(2, 3)]], [[(0, 1)], []]
    with pytest.raises(ValueError, match="no ground-truth span"):
        PE.proposal_ar_an(pr, [[], []])
    with pytest.raises(ValueError, match="no proposal in any video"):
        PE.proposal_ar_an([[], []], gt)
    with pytest.raises(ValueError, match="no proposal is left"):
        PE.proposal_ar_an([[], [(0, 1)]], gt)                      # (the only proposals belong to a video without ground truth)
    with pytest.raises(ValueError, match="no proposal is left"):
        PE.proposal_ar_an(pr, gt, max_avg_nr_proposals=0.1)        # (truncated to nothing)
    with pytest.raises(ValueError, match="one proposal list per ground-truth list"):
        PE.proposal_ar_an(pr, gt[:1])
    with pytest.raises(ValueError, match="one proposal list per ground-truth list"):
        PE.proposal_ar_an([], [])
    with pytest.raises(ValueError, match="one score list per proposal list"):
        PE.proposal_ar_an(pr, gt, scores=[[1.0]])
    with pytest.raises(ValueError, match="one score per proposal"):
        PE.proposal_ar_an(pr, gt, scores=[[1.0, 2.0], [1.0]])
    with pytest.raises(ValueError, match="between 1 and 32 tIoU thresholds"):
        PE.proposal_ar_an(pr, gt, thresholds=np.linspace(0.1, 0.9, 33))
    with pytest.raises(ValueError, match="between 1 and 32 tIoU thresholds"):
        PE.proposal_ar_an(pr, gt, thresholds=[])
    with pytest.raises(ValueError, match="between 1 and 4096 curve points"):
        PE.proposal_ar_an(pr, gt, points=PE.MAX_POINTS + 1)
    with pytest.raises(ValueError, match="between 1 and 4096 curve points"):
        PE.proposal_ar_an(pr, gt, points=0)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="proposal span is not finite"):
            PE.proposal_ar_an([[(0, bad)], [(2, 3)]], gt)
        with pytest.raises(ValueError, match="ground-truth span is not finite"):
            PE.proposal_ar_an(pr, [[(bad, 1)], []])
        with pytest.raises(ValueError, match="score is not finite"):
            PE.proposal_ar_an(pr, gt, scores=[[bad], [0.5]])
    with pytest.raises(ValueError, match="max_avg_nr_proposals"):
        PE.proposal_ar_an(pr, gt, max_avg_nr_proposals=-1)
    for args in ((pr, [[], []]), ([[], []], gt), ([[(0, np.nan)], []], gt)):
        with pytest.raises(ValueError):
            R.ar_an(*args)                                          # (the referee refuses the same)


def test_kernel_wrappers_check_shapes_and_dtypes(backend):
    assert K.proposal_eval_max_points() == PE.MAX_POINTS >= 1000

    def t(a, dtype):
        return backend.put(torch.from_numpy(np.asarray(a, dtype=dtype)))
    good = dict(gt_span=t([[0, 1]], np.float64), gt_off=t([0, 1], np.int32), prop=t([[0, 1], [0, 2]], np.float64),
                prop_off=t([0, 2], np.int32), nr=t([2], np.int32), thresholds=t([0.5], np.float64),
                pcn=t([0.5, 1.0], np.float64), per_video=2.0)
    first_hit, matches, curves = K.proposal_eval_ar_an(**good)
    assert first_hit.cpu().tolist() == [[0]] and matches.cpu().tolist() == [[1, 1]]
    assert curves.cpu().tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 0.5]
    for name, bad in (("gt_span", t([[0, 1]], np.float32)), ("gt_span", t([0, 1], np.float64)), ("gt_off", t([0, 1], np.int64)),
                      ("prop", t([[0, 1], [0, 2]], np.float32)), ("prop_off", t([0, 1, 2], np.int32)), ("nr", t([2], np.int64)),
                      ("nr", t([2, 2], np.int32)), ("thresholds", t([0.5], np.float32)), ("pcn", t([[0.5, 1.0]], np.float64)),
                      ("thresholds", t(np.linspace(0.1, 0.9, 33), np.float64)),
                      ("pcn", t(np.linspace(0.1, 1, PE.MAX_POINTS + 1), np.float64)), ("order", t([0, 1], np.int64)),
                      ("order", t([0], np.int32)), ("gt_span", t(np.zeros((0, 2)), np.float64))):
        with pytest.raises(ValueError, match="proposal_eval_ar_an"):
            K.proposal_eval_ar_an(**dict(good, **{name: bad}))
    rank = dict(score=t([0.5, 0.7], np.float64), prop_off=t([0, 2], np.int32), sort_off=t([0, 2], np.int64), sort_entries=2)
    assert K.proposal_eval_rank(**rank).cpu().tolist() == [1, 0]
    for name, bad in (("score", t([0.5, 0.7], np.float32)), ("prop_off", t([0, 2], np.int64)), ("sort_off", t([0, 2], np.int32)),
                      ("sort_off", t([0, 2, 2], np.int64)), ("sort_entries", 1)):
        with pytest.raises(ValueError, match="proposal_eval_rank"):
            K.proposal_eval_rank(**dict(rank, **{name: bad}))
    # the library refuses what is beyond its caps by itself, before any launch
    lib = backend_lib()
    with pytest.raises(RuntimeError, match="thresholds, at most 32"):
        lib.call("ssn_proposal_eval_ar_an", 1, 1, 1, 1, 1, 1, 1, 1, None, 1, 33, 1, 2, 1.0, 1, 1, 1, None)
    with pytest.raises(RuntimeError, match="curve points, at most 4096"):
        lib.call("ssn_proposal_eval_ar_an", 1, 1, 1, 1, 1, 1, 1, 1, None, 1, 1, 1, 4097, 1.0, 1, 1, 1, None)


def backend_lib():
    from action_detection_amd import _lib
    return _lib.get_lib()
