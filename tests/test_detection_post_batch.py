"""Batched detection post-processing (csrc/detect_batch.hip, DetectionPostProcessor.process_videos, BatchedDetections,
DetectionEvaluator.add_batch, tools/eval_detections.py).

The referee everywhere is the per-video path on the same inputs (process_video_device / process_video over
csrc/detect.hip): the batch must give the same BITS -- float64 rows are compared as int64, fused scores as int32, so a
NaN equals a NaN.  The reference's own outputs (tests/golden/ref_detection*.npz) are matched with the tolerance
tests/test_detection_post.py uses for them."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import action_detection_amd  # noqa: F401
from action_detection_amd.detection_eval import DetectionEvaluator, tiou_thresholds
from action_detection_amd.detection_post import DetectionPostProcessor
from action_detection_amd.proposal_sampling import ProposalSampler

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# (name, constructor arguments after num_class and the NMS threshold, with_reg, cls-branch)
SETTINGS = [
    ("top_k_0", dict(top_k=0), True, False),
    ("top_k_5", dict(top_k=5), True, False),
    ("top_k_40", dict(top_k=40), True, False),            # below P_v * C for some videos of a batch, above it for others
    ("top_k_1e6", dict(top_k=10 ** 6), True, False),
    ("no_regression", dict(top_k=40, no_regression=True), True, False),
    ("reg_none", dict(top_k=0), False, False),
    ("cls_raw_1", dict(top_k=7, cls_top_k=1, softmax_before_filter=False), True, True),
    ("cls_raw_3", dict(top_k=7, cls_top_k=3, softmax_before_filter=False), True, True),
    ("cls_softmax_1", dict(top_k=7, cls_top_k=1, softmax_before_filter=True), True, True),
    ("cls_softmax_3", dict(top_k=7, cls_top_k=3, softmax_before_filter=True), True, True),
]
NMS = 0.45


def batches_of(backend):
    """(sizes, classes) of the mixed batches of a tier.  The emulator runs every barrier through fibers: tiny batches."""
    if backend.is_gpu:
        big = [700, 0, 1, 2048, 2049, 64, 65, 187]      # both LDS forms, the workspace form, both sides of every threshold
        return [(big, 20), (big, 65), ([50, 0, 1, 42, 187], 100)]
    return [([0, 1, 2, 5, 17, 24, 3], 6), ([2100, 3], 2)]


def synthetic_video(rs, p, c):
    start = rs.uniform(0, 0.8, p)
    length = rs.uniform(0.02, 0.5, p)
    rel = np.stack([start, np.minimum(start + length, 1.0)], axis=1)            # float64, as in the pickles
    act = rs.standard_normal((p, c + 1)).astype(np.float32) * 2
    comp = rs.standard_normal((p, c)).astype(np.float32)
    reg = (rs.standard_normal((p, c, 2)) * 0.3).astype(np.float32)
    return rel[None], act, comp, reg


def make_videos(sizes, c, seed):
    rs = np.random.RandomState(seed)
    return [("video_%d" % i, synthetic_video(rs, p, c)) for i, p in enumerate(sizes)]


def classifier_scores(videos, c, seed):
    """Scores of an external classifier; those of the third video tie exactly (all equal)."""
    rs = np.random.RandomState(seed)
    out = {vid: rs.standard_normal(c).astype(np.float32) for vid, _ in videos}
    if len(videos) > 2:
        out[videos[2][0]] = np.full(c, 0.25, dtype=np.float32)
    return out


def drop_reg(videos):
    return [(vid, (rel, act, comp, None)) for vid, (rel, act, comp, _) in videos]


def per_video(backend, post, videos, vcls=None):
    """The referee: [(dets [C, n, 5], counts [C], combined [P, C])] as numpy, one process_video_device call per video."""
    out = []
    for vid, (rel, act, comp, reg) in videos:
        (dets, counts), comb = post.process_video_device(
            torch.from_numpy(rel), backend.put(torch.from_numpy(act)), backend.put(torch.from_numpy(comp)),
            backend.put(torch.from_numpy(reg)) if reg is not None else None, device=backend.device,
            video_cls_score=None if vcls is None else vcls[vid])
        out.append((dets.cpu().numpy(), counts.cpu().numpy(), comb.cpu().numpy()))
    return out


_REFEREE = {}


def referee(backend, key, post, videos, vcls=None):
    """per_video, computed once per (tier, case) and shared by the tests that need it (never modified)."""
    k = (backend.name,) + key
    if k not in _REFEREE:
        _REFEREE[k] = per_video(backend, post, videos, vcls)
    return _REFEREE[k]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def host(b):
    return dict(rows=b.rows.cpu().numpy(), cls=b.cls.cpu().numpy(), vid=b.vid.cpu().numpy(), prop=b.prop.cpu().numpy(),
                row_off=b.row_off.cpu().numpy(), combined=b.combined.cpu().numpy(), p_off=b.p_off.cpu().numpy())


def assert_equals_per_video(b, ref, videos, c, regress_from=None):
    """BatchedDetections `b` against the referee's per-video results: rows, cls, prop, counts, combined."""
    h = host(b)
    sizes = [v[1][1].shape[0] for v in videos]
    assert b.video_ids == [v[0] for v in videos]
    assert np.array_equal(h["p_off"], np.concatenate([[0], np.cumsum(sizes)]))
    assert h["row_off"].shape == (len(videos) * c + 1,) and h["row_off"][0] == 0
    assert h["rows"].shape == (h["row_off"][-1], 5)
    for i, ((vid, (rel, act, comp, reg)), (dets, counts, comb)) in enumerate(zip(videos, ref)):
        off = h["row_off"][i * c:(i + 1) * c + 1]
        assert np.array_equal(np.diff(off), counts), (vid, np.diff(off), counts)
        assert np.array_equal(bits(h["combined"][h["p_off"][i]:h["p_off"][i + 1]]), bits(comb)), vid
        for k in range(c):
            rows = h["rows"][off[k]:off[k + 1]]
            assert np.array_equal(bits(rows), bits(dets[k, :counts[k]])), (vid, k)
            assert (h["cls"][off[k]:off[k + 1]] == k).all() and (h["vid"][off[k]:off[k + 1]] == i).all()
            # prop names the proposal the row was made from: its fused score, its regression scores (or, without them,
            # nothing but the score) are that proposal's
            prop = h["prop"][off[k]:off[k + 1]]
            assert ((prop >= 0) & (prop < sizes[i])).all(), (vid, k)
            assert np.array_equal(bits(rows[:, 2]), bits(comb[prop, k].astype(np.float64)))
            if reg is not None:
                assert np.array_equal(bits(rows[:, 3:]), bits(reg.reshape(-1, c, 2)[prop, k].astype(np.float64)))
            assert len(set(prop.tolist())) == len(prop)


def mixed_case(backend, index, setting):
    """The `index`-th mixed batch of the tier under a setting: (post, videos, classifier scores, referee, classes)."""
    name, kwargs, with_reg, cls_branch = setting
    sizes, c = batches_of(backend)[index]
    videos = make_videos(sizes, c, 100 + index)
    if not with_reg:
        videos = drop_reg(videos)
    vcls = classifier_scores(videos, c, 7) if cls_branch else None
    post = DetectionPostProcessor(c, NMS, **kwargs)
    return post, videos, vcls, referee(backend, ("mixed", index, name), post, videos, vcls), c


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_mixed_batches_equal_the_per_video_path(backend, setting):
    for index in range(len(batches_of(backend))):
        post, videos, vcls, ref, c = mixed_case(backend, index, setting)
        b = post.process_videos(videos, device=backend.device, video_cls_scores=vcls)
        assert b.rows.is_cuda == backend.is_gpu and b.row_off.is_cuda == backend.is_gpu
        assert_equals_per_video(b, ref, videos, c)
        if setting[3]:          # only the reported classes have rows
            k = setting[1]["cls_top_k"]
            per = np.diff(b.row_off.cpu().numpy()).reshape(len(videos), c)
            assert ((per > 0).sum(axis=1) == [min(k, c) if v[1][1].shape[0] else 0 for v in videos]).all()
        # the two other views of the same rows
        first = b.to_host()
        for i, (vid, parts) in enumerate(videos[:3]):
            dets, counts, _ = ref[i]
            assert sorted(first[vid]) == [k for k in range(c) if counts[k] > 0]
            for k, rows in first[vid].items():
                assert np.array_equal(bits(rows), bits(dets[k, :counts[k]]))
            d, n = b.video(i)
            d = d.cpu().numpy()
            assert np.array_equal(n.cpu().numpy(), counts) and d.shape == dets.shape
            for k in range(c):      # (the per-video path leaves rows of classes it does not report behind their zero counts)
                assert np.array_equal(bits(d[k, :counts[k]]), bits(dets[k, :counts[k]])) and not d[k, counts[k]:].any()


def test_offsets_across_scan_tiles(backend):
    """More (video, class) pairs than one tile of the offset scan holds (16384): thousands of empty videos around a few
    small ones, one of them astride the tile boundary."""
    c = 20 if backend.is_gpu else 6
    sizes = [0] * 2800
    for v, p in ((0, 2), (1370, 3), (16384 // c, 4), (2799, 2)):
        sizes[v] = p
    assert len(sizes) * c > 16384 and (16384 // c) * c < 16384 < (16384 // c + 1) * c
    videos = make_videos(sizes, c, 31)
    post = DetectionPostProcessor(c, NMS, 0)
    b = post.process_videos(videos, device=backend.device)
    assert_equals_per_video(b, per_video(backend, post, videos), videos, c)
    assert int(b.row_off[-1]) == len(b.rows) > 0


def tie_videos(sizes, c, seed):
    """Many exactly equal fused scores (scores from four values) and IoUs exactly on the threshold 0.5 (spans on the grid
    k / 8, with duplicates)."""
    rs = np.random.RandomState(seed)
    out = []
    for i, p in enumerate(sizes):
        lo = rs.randint(0, 7, p)
        hi = lo + 1 + (rs.randint(0, 8, p) % (8 - lo))
        rel = np.stack([lo / 8.0, hi / 8.0], axis=1)
        values = np.array([-1, 0, 0.5, 1], dtype=np.float32)
        act = values[rs.randint(0, 4, (p, c + 1))]
        comp = values[rs.randint(0, 4, (p, c))]
        reg = (rs.standard_normal((p, c, 2)) * 0.3).astype(np.float32)
        out.append(("tie_%d" % i, (rel[None], act, comp, reg)))
    return out


@pytest.mark.parametrize("top_k", [0, 10, 37])
def test_ties_fall_as_in_the_per_video_path(backend, top_k):
    sizes, c = ([300, 16, 64], 20) if backend.is_gpu else ([9, 16, 1], 3)
    videos = tie_videos(sizes, c, 5)
    post = DetectionPostProcessor(c, 0.5, top_k)
    ref = referee(backend, ("ties", top_k), post, videos)
    comb = ref[0][2]
    assert len(np.unique(comb)) < comb.size                       # the scores do tie
    b = post.process_videos(videos, device=backend.device)
    assert_equals_per_video(b, ref, videos, c)
    vcls = classifier_scores(videos, c, 3)
    post = DetectionPostProcessor(c, 0.5, top_k, cls_top_k=2)
    assert_equals_per_video(post.process_videos(videos, device=backend.device, video_cls_scores=vcls),
                            referee(backend, ("ties_cls", top_k), post, videos, vcls), videos, c)


@pytest.mark.parametrize("top_k", [0, 15])
def test_non_finite_scores_stay_in_their_video(backend, top_k):
    sizes, c = ([64, 300, 65], 20) if backend.is_gpu else ([5, 12, 7], 4)
    videos = make_videos(sizes, c, 11)
    rel, act, comp, reg = videos[1][1]
    rs = np.random.RandomState(12)
    comp[:] = np.where(rs.uniform(size=comp.shape) < 0.5, 200.0, -200.0).astype(np.float32)   # exp -> inf and 0: inf, NaN fused
    act[1, 2] = np.nan
    post = DetectionPostProcessor(c, 0.4, top_k)
    ref = referee(backend, ("spoilt", top_k), post, videos)
    assert np.isinf(ref[1][2]).any() and np.isnan(ref[1][2]).any()
    b = post.process_videos(videos, device=backend.device)
    assert_equals_per_video(b, ref, videos, c)
    # the other videos' rows do not depend on the spoilt one being in the batch
    others = [videos[0], videos[2]]
    assert_equals_per_video(post.process_videos(others, device=backend.device), [ref[0], ref[2]], others, c)
    h = host(b)
    assert (h["prop"] < np.asarray(sizes)[h["vid"]]).all() and (h["prop"] >= 0).all()


def golden_groups():
    """The cases of the two fixture files, grouped by their settings: (post, [case, ...], cls-branch)."""
    groups = {}
    d = np.load(os.path.join(GOLDEN, "ref_detection.npz"))
    for ci in range(int(d["n_cases"][0])):
        p, c, top_k, no_reg, with_reg = (int(v) for v in d["d%d_cfg" % ci])
        thr = float(d["d%d_thr" % ci][0])
        case = dict(name="d%d" % ci, rel=d["d%d_rel" % ci], act=d["d%d_act" % ci], comp=d["d%d_comp" % ci],
                    reg=d["d%d_reg" % ci] if with_reg else None, counts=d["d%d_counts" % ci], dets=d["d%d_dets" % ci],
                    combined=d["d%d_combined" % ci], vcls=None)
        groups.setdefault(("d", c, thr, top_k, no_reg, with_reg), []).append(case)
    e = np.load(os.path.join(GOLDEN, "ref_detection_cls.npz"))
    for ci in range(int(e["n_cases"][0])):
        p, c, ktop, sbf, no_reg, with_reg = (int(v) for v in e["e%d_cfg" % ci])
        thr = float(e["e%d_thr" % ci][0])
        case = dict(name="e%d" % ci, rel=e["e%d_rel" % ci], act=e["e%d_act" % ci], comp=e["e%d_comp" % ci],
                    reg=e["e%d_reg" % ci] if with_reg else None, counts=e["e%d_counts" % ci], dets=e["e%d_dets" % ci],
                    combined=e["e%d_combined" % ci], vcls=e["e%d_vcls" % ci])
        groups.setdefault(("e", c, thr, ktop, sbf, no_reg, with_reg), []).append(case)
    for key, cases in sorted(groups.items()):
        if key[0] == "d":
            post = DetectionPostProcessor(key[1], key[2], key[3], bool(key[4]))
        else:
            post = DetectionPostProcessor(key[1], key[2], top_k=7, no_regression=bool(key[5]), cls_top_k=key[3],
                                          softmax_before_filter=bool(key[4]))
        yield post, cases, key[0] == "e", key[1], bool(key[-1])


def test_reference_fixtures_in_batches(backend):
    """Every group of fixture cases as ONE batch, each case in twice with another video between its copies: both copies match
    the reference's own outputs and are bit-equal to each other."""
    n_cases = 0
    for post, cases, cls_branch, c, with_reg in golden_groups():
        rs = np.random.RandomState(17)
        frel, fact, fcomp, freg = synthetic_video(rs, 7, c)
        filler = ("filler", (frel, fact, fcomp, freg if with_reg else None))
        videos = [("%s#0" % k["name"], (k["rel"][None], k["act"], k["comp"], k["reg"])) for k in cases] + [filler] \
            + [("%s#1" % k["name"], (k["rel"][None], k["act"], k["comp"], k["reg"])) for k in cases]
        vcls = None
        if cls_branch:
            vcls = {"filler": rs.standard_normal(c).astype(np.float32)}
            for k in cases:
                vcls["%s#0" % k["name"]] = vcls["%s#1" % k["name"]] = k["vcls"]
        b = post.process_videos(videos, device=backend.device, video_cls_scores=vcls)
        h = host(b)
        for j, k in enumerate(cases):
            copies = []
            for i in (j, len(cases) + 1 + j):
                off = h["row_off"][i * c:(i + 1) * c + 1]
                assert np.array_equal(np.diff(off), k["counts"]), k["name"]
                rows = h["rows"][off[0]:off[-1]]
                assert np.allclose(rows, k["dets"].reshape(-1, 5), rtol=2e-6, atol=1e-9, equal_nan=True), k["name"]
                comb = h["combined"][h["p_off"][i]:h["p_off"][i + 1]]
                assert np.allclose(comb, k["combined"], rtol=2e-6, atol=1e-30, equal_nan=True), k["name"]
                copies.append((rows, comb, h["prop"][off[0]:off[-1]], h["cls"][off[0]:off[-1]]))
            assert np.array_equal(bits(copies[0][0]), bits(copies[1][0])) and np.array_equal(bits(copies[0][1]), bits(copies[1][1]))
            assert np.array_equal(copies[0][2], copies[1][2]) and np.array_equal(copies[0][3], copies[1][3])
            n_cases += 1
    assert n_cases == 10


def seeded_ground_truth(videos, c, seed):
    rs = np.random.RandomState(seed)
    gt = []
    for vid, _ in videos:
        for k in rs.choice(c, 3, replace=False):
            s, e = np.sort(rs.uniform(0, 1, 2))
            if e - s > 0.02:
                gt.append([vid, int(k), float(s), float(e)])
    return gt


def test_evaluator_takes_the_batch_as_it_is(backend):
    setting = SETTINGS[2]
    post, videos, _, _, c = mixed_case(backend, 0, setting)
    thresholds = tiou_thresholds("thumos14")
    gt = seeded_ground_truth(videos, c, 23)
    batch_ev = DetectionEvaluator(c, thresholds, device=backend.device)
    batch_ev.add_batch(post.process_videos(videos, device=backend.device))
    loop_ev = DetectionEvaluator(c, thresholds, device=backend.device)
    for vid, (rel, act, comp, reg) in videos:
        dets, _ = post.process_video_device(torch.from_numpy(rel), backend.put(torch.from_numpy(act)),
                                            backend.put(torch.from_numpy(comp)), backend.put(torch.from_numpy(reg)),
                                            device=backend.device)
        loop_ev.add_video(vid, dets)
    got, want = batch_ev.evaluate(gt, return_matches=True), loop_ev.evaluate(gt, return_matches=True)
    assert len(want.order) > 0 and want.tp.any()
    assert np.array_equal(got.ap, want.ap, equal_nan=True)
    assert np.array_equal(got.tp, want.tp) and np.array_equal(got.order, want.order)
    assert np.array_equal(got.pred_off, want.pred_off)
    assert got.rows[0] == want.rows[0] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got.rows[1:], want.rows[1:]))


def test_order_and_repeatability(backend):
    setting = SETTINGS[2]
    post, videos, _, ref, c = mixed_case(backend, 0, setting)
    a, again = (host(post.process_videos(videos, device=backend.device)) for _ in range(2))
    for name in a:
        assert np.array_equal(bits(a[name]), bits(again[name])), name
    # reversed videos: the per-video blocks are permuted, nothing changes inside them
    rev = post.process_videos(videos[::-1], device=backend.device)
    assert rev.video_ids == [v[0] for v in videos[::-1]]
    assert_equals_per_video(rev, ref[::-1], videos[::-1], c)
    # a dict is taken in its own order
    d = post.process_videos(dict(videos), device=backend.device)
    assert np.array_equal(bits(host(d)["rows"]), bits(a["rows"]))


def tools_module(name):
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    return __import__(name)


def test_driver_batched_and_per_video_agree(backend, tmp_path, capsys):
    """tools/eval_detections.py on a three-video pickle: the batched default and --per-video give the same AP array and
    the same table, with and without --cls_scores."""
    prop_file = os.path.join(GOLDEN, "proposal_list_processed.txt")
    sampler = ProposalSampler(prop_file)
    rs = np.random.RandomState(3)
    num_class, pc, cls_scores = 100, {}, {}
    for v, p in zip(sampler.video_list[:3], (9, 4, 11)):
        start = rs.uniform(0, 0.6, p)
        rel = np.stack([start, start + rs.uniform(0.1, 0.4, p)], axis=1)
        rel[:3] = np.array([v.gt[0].start_frame, v.gt[0].end_frame]) / v.num_frames + rs.uniform(-0.02, 0.02, (3, 2))
        pc[v.id] = (np.clip(rel, 0, 1)[None], rs.standard_normal((p, num_class + 1)).astype(np.float32),
                    rs.standard_normal((p, num_class)).astype(np.float32),
                    (rs.standard_normal((p, num_class, 2)) * 0.1).astype(np.float32))
        pc[v.id][1][:, v.gt[0].label] += 6.0                        # (the video's own class scores high)
        cls_scores[os.path.basename(v.id) + ".avi"] = rs.standard_normal(num_class).astype(np.float32)
        cls_scores[os.path.basename(v.id) + ".avi"][v.gt[0].label - 1] += 8.0
    with open(str(tmp_path / "scores.pc"), "wb") as fh:
        pickle.dump(pc, fh)
    with open(str(tmp_path / "cls.pc"), "wb") as fh:
        pickle.dump(cls_scores, fh)
    tool = tools_module("eval_detections")
    base = [str(tmp_path / "scores.pc"), "--proposal-list", prop_file, "--num-class", str(num_class), "--tiou", "activitynet1.2",
            "--nms_threshold", "0.6", "--top_k", "30", "--device", str(backend.device)]
    for extra in ([], ["--cls_scores", str(tmp_path / "cls.pc"), "--cls_top_k", "2"]):
        tables, aps = [], []
        for mode in ([], ["--per-video"]):
            out = str(tmp_path / "ap.npy")
            result = tool.main(base + extra + mode + ["--ap-out", out])
            printed = capsys.readouterr().out
            tables.append(printed[printed.index("Evaluation done."):])
            aps.append((result.ap, np.load(out)))
        assert np.array_equal(bits(aps[0][0]), bits(aps[1][0])) and np.array_equal(bits(aps[0][1]), bits(aps[1][1]))
        assert np.array_equal(bits(aps[0][0]), bits(aps[0][1]))
        assert tables[0] == tables[1] and "Average" in tables[0]
        assert np.nanmax(aps[0][0]) > 0


def test_argument_errors(backend):
    c = 6
    post = DetectionPostProcessor(c, NMS, 10)
    videos = make_videos([3, 4], c, 1)
    run = lambda v: post.process_videos(v, device=backend.device)      # noqa: E731
    with pytest.raises(ValueError, match="all videos or for none"):
        run([videos[0], drop_reg(videos[1:])[0]])
    rel, act, comp, reg = synthetic_video(np.random.RandomState(2), 4, c + 1)
    with pytest.raises(ValueError, match="completeness"):
        run([videos[0], ("other_c", (rel, act, comp, reg))])
    rel, act, comp, reg = videos[1][1]
    with pytest.raises(ValueError, match="activity"):
        run([videos[0], ("bad_act", (rel, act[:, :c], comp, reg))])
    with pytest.raises(ValueError, match="activity"):
        run([videos[0], ("short_act", (rel, act[:3], comp, reg))])
    # too many (proposal, class) pairs for int32 indices: refused on the shapes alone (views of one element, nothing allocated)
    p = 2 ** 31 // c + 1
    huge = (np.broadcast_to(np.zeros(1), (1, p, 2)), np.broadcast_to(np.zeros(1, dtype=np.float32), (p, c + 1)),
            np.broadcast_to(np.zeros(1, dtype=np.float32), (p, c)), None)
    with pytest.raises(ValueError, match="split the batch"):
        run([("huge", huge)])
    half = tuple(None if x is None else x[..., :p // 2 + 1, :] if x.ndim == 3 else x[:p // 2 + 1] for x in huge)
    with pytest.raises(ValueError, match="split the batch"):
        run([("half_a", half), ("half_b", half)])
    with pytest.raises(ValueError):
        run([])
    b = run(videos)
    ev = DetectionEvaluator(c, [0.5], device=backend.device)
    ev.add_batch(b)
    with pytest.raises(ValueError, match="added before"):
        ev.add_batch(b)
    other = DetectionEvaluator(c, [0.5], device=backend.device)
    other.add_video(videos[1][0], {})
    with pytest.raises(ValueError, match="added before"):
        other.add_batch(b)
    with pytest.raises(ValueError, match="added before"):
        DetectionEvaluator(c, [0.5], device=backend.device).add_batch(run([videos[0], videos[0]]))
