"""The proposal-list stage: dataset readers (datasets.py), the batched builder (proposal_lists.py over
csrc/proposal_list.hip and the naming / recall kernels) and the text writer (proposal_io.format_window_list_rows).

Pinned against tests/golden/ref_proposal_lists.npz (tools/make_proposal_list_golden.py): what the REFERENCE's own classes
and functions make of tests/golden/thumos14_excerpt.json (a trimmed copy of its THUMOS14 annotations) and of the
hand-written tests/golden/anet_tiny.json.  Everything is EXACT: window positions are integers, the kept-window test and a
frame number are single IEEE float64 operations, IoU and overlap come from a kernel that is already pinned exactly.  The
fixture's videos have IoUs that lie exactly on a recall threshold and one a single ulp away (the generator lists them),
so the recall decisions are compared per video, not only as rates.
"""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import action_detection_amd as pkg
from action_detection_amd import _lib
from action_detection_amd import kernels as K
from action_detection_amd.datasets import ANetDB, ThumosDB
from action_detection_amd.proposal_io import format_window_list_record, format_window_list_rows
from action_detection_amd.proposal_lists import ProposalListBuilder, windows_per_video
from action_detection_amd.tag_proposals import sliding_window_proposals

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUBSETS = {"thumos": ("validation", "test"), "anet": ("training", "validation", "testing")}
_cache = {}


def reference():
    if "ref" not in _cache:
        _cache["ref"] = dict(np.load(os.path.join(GOLDEN, "ref_proposal_lists.npz")))
    return _cache["ref"]


def materialise_excerpt(folder):
    with open(os.path.join(GOLDEN, "thumos14_excerpt.json")) as f:
        excerpt = json.load(f)
    for rel, text in excerpt.items():
        os.makedirs(os.path.dirname(os.path.join(folder, rel)), exist_ok=True)
        with open(os.path.join(folder, rel), "w") as f:
            f.write(text)
    return folder


@pytest.fixture(scope="module")
def databases(tmp_path_factory):
    folder = materialise_excerpt(str(tmp_path_factory.mktemp("thumos_14")))
    return {"thumos": ThumosDB.from_folder(folder), "anet": ANetDB.from_json(os.path.join(GOLDEN, "anet_tiny.json"))}


def cases(databases):
    for name, subsets in SUBSETS.items():
        for s in subsets:
            yield name, s, databases[name].get_subset_videos(s)


def video(duration, gt=(), vid="synthetic"):
    return SimpleNamespace(id=vid, duration=duration,
                           instances=[SimpleNamespace(num_label=l, time_span=(s, e)) for l, s, e in gt])


def parse_dump(text):
    """-> (path, frame count, gt rows [n, 3] int, proposal rows as [label, iou text, overlap text, start, end])"""
    lines = text.split("\n")
    n_gt = int(lines[3])
    gt = np.asarray([[int(x) for x in l.split()] for l in lines[4:4 + n_gt]], dtype=np.int64).reshape(-1, 3)
    n_pr = int(lines[4 + n_gt])
    pr = [l.split() for l in lines[5 + n_gt:5 + n_gt + n_pr]]
    assert lines[5 + n_gt + n_pr:] in ([""], ["", ""]) and int(lines[2]) == 1
    return lines[0], int(lines[1]), gt, pr


def host_windows(duration, overlap, max_level=8, time_step=1):
    """the existing host enumeration (tag_proposals.sliding_window_proposals), the cross-check for synthetic durations"""
    return np.asarray(sliding_window_proposals(duration, time_step=time_step, max_level=max_level, overlap=overlap),
                      dtype=np.float64).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------ readers
def test_readers_match_reference(databases):
    ref = reference()
    for name, s, videos in cases(databases):
        p = "%s_%s_" % (name, s)
        assert [v.id for v in videos] == [str(x) for x in ref[p + "ids"]], p
        assert np.array_equal(np.asarray([v.duration for v in videos], dtype=np.float64), ref[p + "durations"]), p
        assert [isinstance(v.duration, int) for v in videos] == list(ref[p + "integral"])
        off = np.concatenate([[0], np.cumsum([len(v.instances) for v in videos])])
        assert np.array_equal(off, ref[p + "gt_off"]), p
        assert [i.num_label for v in videos for i in v.instances] == list(ref[p + "gt_label"]), p
        spans = np.asarray([i.time_span for v in videos for i in v.instances], dtype=np.float64).reshape(-1, 2)
        assert np.array_equal(spans, ref[p + "gt_span"]), p
    for name in SUBSETS:
        assert databases[name].get_ordered_label_list() == [str(x) for x in ref["%s_labels" % name]]
    assert len(databases["thumos"].get_ordered_label_list()) == 20 and "Ambiguous" not in databases["thumos"].get_ordered_label_list()
    # the taxonomy's alphabetical order is not its file order; subsets are ordered by id, not as the file lists them
    assert databases["anet"].get_ordered_label_list() == ["Archery", "Ballet", "Mowing the lawn", "Washing dishes", "Zumba"]
    assert [v.id for v in databases["anet"].get_subset_videos("validation")] == ["Bval0000004", "mVal_000003"]
    with pytest.raises(ValueError):
        databases["thumos"].get_subset_videos("testing")
    with pytest.raises(ValueError):
        databases["anet"].get_subset_videos("test")


def test_reader_rules_on_the_excerpt(databases):
    """Each THUMOS rule shows on the video chosen for it."""
    val = {v.id: v for v in databases["thumos"].get_subset_videos("validation")}
    test = {v.id: v for v in databases["thumos"].get_subset_videos("test")}
    with open(os.path.join(GOLDEN, "thumos14_excerpt.json")) as f:
        excerpt = json.load(f)
    lines = lambda path, vid: [l for l in excerpt[path].split("\n") if l.startswith(vid + " ")]      # noqa: E731
    hj = lines("temporal_annotations_validation/HighJump_val.txt", "video_validation_0000364")
    behind = [l for l in hj if float(l.split()[1]) > val["video_validation_0000364"].duration]
    assert len(behind) == 2 and len([i for i in val["video_validation_0000364"].instances if i.label == "HighJump"]) == len(hj) - 2
    assert lines("temporal_annotations_validation/CricketShot_val.txt", "video_validation_0000178")
    assert all(i.label != "CricketShot" for i in val["video_validation_0000178"].instances)
    assert lines("temporal_annotations_test/Ambiguous_test.txt", "video_test_0001433")
    assert all(i.label != "Ambiguous" and i.num_label is not None for v in test.values() for i in v.instances)
    assert test["video_test_0000364"].duration == 213.0 and test["video_test_0000764"].instances == []
    assert min(v.duration for v in val.values()) == 8.932 and max(v.duration for v in test.values()) == 1673.428


def test_frame_folders_attach_by_each_datasets_key(databases, tmp_path):
    thumos = ThumosDB.from_folder(materialise_excerpt(str(tmp_path / "t14")))
    anet = ANetDB.from_json(os.path.join(GOLDEN, "anet_tiny.json"))
    v = thumos.get_subset_videos("test")[0]
    a = anet.get_subset_videos("training")[0]
    for rec in (v, a):
        with pytest.raises(ValueError, match=rec.id):
            rec.path
    frames = tmp_path / "frames"
    for folder in (v.id, "v_" + a.id + ".mp4", "unrelated"):
        (frames / folder).mkdir(parents=True)
    assert thumos.try_load_file_path(str(frames)) == 1 and anet.try_load_file_path(str(frames)) == 1
    assert v.path == str(frames / v.id) and a.path == str(frames / ("v_" + a.id + ".mp4"))
    with pytest.raises(ValueError):
        thumos.get_subset_videos("test")[1].path


# ------------------------------------------------------------------------------------------------ fixture videos
@pytest.mark.parametrize("overlap", [0.7, 0.4])
def test_fixture_subsets_match_reference(backend, databases, overlap):
    """Windows, name_proposal rows, recall, frame columns and the dumped text of every subset, each subset one batch."""
    ref = reference()
    builder = ProposalListBuilder(device=backend.device)
    seen_zero_frames = False
    for name, s, videos in cases(databases):
        p = "%s_%s_o%d_" % (name, s, round(overlap * 100))
        batch = builder.sliding_windows(videos, overlap=overlap)
        assert batch.windows.dtype == torch.float64 and str(batch.windows.device).startswith(str(backend.device)[:4])
        assert np.array_equal(batch.offsets, ref[p + "win_off"]), p
        wins = windows_per_video(batch)
        assert np.array_equal(np.concatenate(wins), ref[p + "windows"]), p
        frame_cnt = ref["%s_%s_frame_cnt" % (name, s)]
        res = builder.build(batch, frame_cnt)
        named = ref[p + "named"]
        assert np.array_equal(np.concatenate(res.labels), named[:, 0].astype(np.int32)), p
        assert np.array_equal(np.concatenate(res.iou), named[:, 1]) and np.array_equal(np.concatenate(res.overlap_self), named[:, 2])
        assert np.array_equal(res.hits, ref[p + "hits"]), p
        assert np.array_equal(np.asarray(res.recall), ref[p + "recall"], equal_nan=True), p
        assert res.mean_proposals == np.mean(np.diff(ref[p + "win_off"]))
        assert res.status == [0] * len(videos)
        for i, v in enumerate(videos):
            text = str(ref[p + "dump"][i])
            path, fc, gt_rows, pr_rows = parse_dump(text)
            assert fc == frame_cnt[i]
            seen_zero_frames |= fc == 0
            assert res.frames[i].dtype == np.int32 and res.gt_frames[i].dtype == np.int32
            assert np.array_equal(res.gt_frames[i], gt_rows[:, 1:]) and np.array_equal(res.gt_labels[i], gt_rows[:, 0]), v.id
            assert np.array_equal(res.frames[i], np.asarray([[int(r[3]), int(r[4])] for r in pr_rows], dtype=np.int64).reshape(-1, 2)), v.id
            mine = format_window_list_rows(path, fc, *res.rows(i))
            assert mine == text, v.id
            gt = [(x.num_label, x.time_span) for x in v.instances]
            rows = [(int(l), float(o), float(a), float(w[0]), float(w[1]))
                    for l, o, a, w in zip(res.labels[i], res.iou[i], res.overlap_self[i], wins[i])]
            assert mine == format_window_list_record(path, fc, v.duration, gt, rows), v.id
    assert seen_zero_frames


def test_fixture_conditions():
    ref = reference()
    levels_without_window = multiples = 0
    for name, subsets in SUBSETS.items():
        for s in subsets:
            dur = ref["%s_%s_durations" % (name, s)]
            off, win = ref["%s_%s_o70_win_off" % (name, s)], ref["%s_%s_o70_windows" % (name, s)]
            for i, d in enumerate(dur):
                w = win[off[i]:off[i + 1]]
                for l in range(8):
                    step = int(np.ceil(2 ** l * (1 - 0.7)))
                    levels_without_window += int(not np.any(w[:, 1] - w[:, 0] == 2 ** l))
                    multiples += int(d >= step and d / step == int(d / step))
    assert levels_without_window >= 1 and multiples >= 1
    assert float(ref["iou_margin_measured"][0]) == 0.0      # IoUs exactly ON a threshold are part of the fixture
    assert 1000 < ref["thumos_test_o70_win_off"][-1] < 20000


# ------------------------------------------------------------------------------------------------ edge cases
def check_against_host(builder, durations, overlap, max_level=8, time_step=1):
    batch = builder.sliding_windows([video(d) for d in durations], overlap=overlap, max_level=max_level, time_step=time_step)
    got = windows_per_video(batch)
    for d, g in zip(durations, got):
        want = host_windows(d, overlap, max_level, time_step)
        assert np.array_equal(g, want), (d, overlap, len(g), len(want))
    return batch, got


def test_short_videos_have_no_windows(backend):
    builder = ProposalListBuilder(device=backend.device)
    batch, got = check_against_host(builder, [0.5, np.nextafter(1.0, 0.0), 0.0], 0.7)
    assert list(batch.offsets) == [0, 0, 0, 0] and batch.windows.shape == (0, 2)
    res = builder.build(batch, [10, 10, 10])
    assert [len(x) for x in res.labels] == [0, 0, 0] and res.mean_proposals == 0 and res.status == [0, 0, 0]
    _, got = check_against_host(builder, [1.0, 0.5], 0.7)          # exactly one second: the window (0, t_span) of every level
    assert len(got[0]) == 8 and len(got[1]) == 0


@pytest.mark.parametrize("overlap", [0.7, 0.4])
def test_durations_on_and_next_to_a_step_boundary(backend, overlap):
    builder = ProposalListBuilder(device=backend.device)
    for level in (0, 2, 3, 5, 7):
        t_span = 2 ** level
        step = int(np.ceil(t_span * (1 - overlap)))
        for n in (1, 7, 40):
            d = float(n * step)
            check_against_host(builder, [np.nextafter(d, 0.0), d, np.nextafter(d, np.inf), n * step, d + 1.0], overlap)
        t = float(t_span)
        check_against_host(builder, [t, np.nextafter(t, 0.0), np.nextafter(t, np.inf), t + 1.0, np.nextafter(t + 1.0, 0.0)], overlap)


def test_single_level_and_time_step(backend):
    builder = ProposalListBuilder(device=backend.device)
    batch, got = check_against_host(builder, [33.5, 7, 200.0], 0.7, max_level=1)
    assert all((g[:, 1] - g[:, 0] == 1).all() for g in got) and [len(g) for g in got] == [33, 7, 200]
    # time_step moves the step and not the window length (the reference's quirk)
    _, got = check_against_host(builder, [100.25], 0.7, max_level=4, time_step=2.5)
    assert set(np.unique(got[0][:, 1] - got[0][:, 0])) == {1.0, 2.0, 4.0, 8.0}
    assert got[0][1, 0] == np.ceil(1 * 2.5 * (1 - 0.7))


def test_many_windows_next_to_none(backend):
    """More than 256 windows in one level (more than one workgroup of the fill) next to a video without any."""
    builder = ProposalListBuilder(device=backend.device)
    batch, got = check_against_host(builder, [0.4, 700.3, 0.9, 300.0], 0.7)
    assert len(got[0]) == 0 and len(got[2]) == 0
    assert np.sum(got[1][:, 1] - got[1][:, 0] == 1) == 700 > 256


def test_video_without_ground_truth(backend):
    builder = ProposalListBuilder(device=backend.device)
    videos = [video(20.0, vid="none"), video(30.0, [(3, 2.5, 11.25), (7, 12.0, 29.0)], vid="two")]
    batch = builder.sliding_windows(videos, overlap=0.4)
    res = builder.build(batch, [100, 301])
    assert (res.labels[0] == 0).all() and (res.iou[0] == 0).all() and (res.overlap_self[0] == 0).all()
    assert len(res.gt_frames[0]) == 0 and res.gt_frames[1].shape == (2, 2) and list(res.gt_labels[1]) == [4, 8]
    assert list(res.totals) == [0, 2] and (res.hits[0] == 0).all()
    # the video without ground truth counts as recalled (0 hits of 0), as in the reference
    assert all(pv >= 0.5 for pv, _ in res.recall)
    assert format_window_list_rows("f/none", 100, *res.rows(0)).startswith("f/none\n100\n1\n0\n%d\n0 0.0000 0.0000 0 5\n" % len(res.labels[0]))
    alone = builder.build(builder.sliding_windows(videos[:1], overlap=0.4), [100])
    assert np.isnan([pi for _, pi in alone.recall]).all() and [pv for pv, _ in alone.recall] == [1.0, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------ rows
def test_overflowing_positions_set_only_their_own_status_bit(backend):
    builder = ProposalListBuilder(device=backend.device)
    videos = [video(10.0, [(1, 1.0, 4.5)], "ok"), video(1.0, [(2, 0.25, 0.5)], "proposal overflows"),
              video(1.0, [(2, 0.25, 2.0)], "gt overflows"), video(0.0, [(0, 0.0, 1.0)], "zero duration"),
              video(8.0, [(5, 0.5, 7.75)], "ok too")]
    spans = [[(0.0, 5.0), (2.5, 9.75)], [(0.5, 0.75), (0.5, 3.0)], [(0.125, 1.0)], [(0.0, 0.5), (0.25, 0.5)], [(1.0, 7.9)]]
    frame_cnt = [250, 2000000000, 2000000000, 100, 2 ** 31 - 1]
    batch = builder.from_spans(videos, spans)
    res = builder.build(batch, frame_cnt)
    assert res.status == [0, 2, 1, 3, 0]
    for i in (0, 4):
        fps = float(frame_cnt[i]) / videos[i].duration
        assert res.frames[i].tolist() == [[int(a * fps), int(b * fps)] for a, b in spans[i]]
        assert res.gt_frames[i].tolist() == [[int(x * fps) for x in videos[i].instances[0].time_span]]
    assert res.frames[4].max() > 2 ** 30                                     # large, and still inside int32
    assert res.frames[1].tolist() == [[1000000000, 1500000000], [1000000000, 0]]      # 3.0 * 2e9 does not fit: 0 in its place
    assert res.gt_frames[1].tolist() == [[500000000, 1000000000]]
    assert res.gt_frames[2].tolist() == [[500000000, 0]] and res.frames[2].tolist() == [[250000000, 2000000000]]
    assert res.frames[3].tolist() == [[0, 0], [0, 0]] and res.gt_frames[3].tolist() == [[0, 0]]      # 0 * inf, x * inf


def test_from_spans_equals_sliding_windows_given_as_spans(backend, databases):
    """The second way into build(): spans uploaded from the host give what the windows made on the device give."""
    builder = ProposalListBuilder(device=backend.device)
    videos = databases["thumos"].get_subset_videos("validation")
    a = builder.sliding_windows(videos, overlap=0.7)
    b = builder.from_spans(videos, windows_per_video(a))
    ra, rb = builder.build(a, range_counts(len(videos))), builder.build(b, range_counts(len(videos)))
    for i in range(len(videos)):
        for x, y in zip(ra.rows(i), rb.rows(i)):
            assert np.array_equal(x, y)
    assert np.array_equal(ra.hits, rb.hits)


def range_counts(n):
    return [37 + 101 * i for i in range(n)]


# ------------------------------------------------------------------------------------------------ batching
def test_batch_independence_and_repeats(backend, databases):
    builder = ProposalListBuilder(device=backend.device)
    pool = [v for v in databases["thumos"].get_subset_videos("validation") + databases["anet"].get_subset_videos("training")]
    videos = [pool[i % len(pool)] for i in range(17)]
    counts = range_counts(len(videos))
    batch = builder.sliding_windows(videos, overlap=0.7)
    together = builder.build(batch, counts)
    again = builder.build(builder.sliding_windows(videos, overlap=0.7), counts)
    wins = windows_per_video(batch)
    for i, v in enumerate(videos):
        one = builder.sliding_windows([v], overlap=0.7)
        alone = builder.build(one, [counts[i]])
        assert np.array_equal(windows_per_video(one)[0], wins[i])
        for x, y, z in zip(together.rows(i), alone.rows(0), again.rows(i)):
            assert np.array_equal(x, y) and np.array_equal(x, z) and x.dtype == y.dtype
        assert np.array_equal(together.hits[i], alone.hits[0]) and together.status[i] == alone.status[0]
    assert np.array_equal(together.hits, again.hits) and together.recall == again.recall


# ------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_are_rejected_before_any_launch():
    """Checkable without a GPU: the builder and the real library validate on the host before anything is launched."""
    builder = ProposalListBuilder(device="cpu")          # (never reached: every call below fails in front of the first tensor)
    v = [video(10.0)]
    for kwargs in ({"overlap": 1.0}, {"overlap": 1.5}, {"time_step": 0}, {"max_level": 0}, {"max_level": 32},
                   {"overlap": float("nan")}):
        with pytest.raises(ValueError):
            builder.sliding_windows(v, **kwargs)
    for bad in ([], [video(float("inf"))], [video(float("nan"))], [video(3e9)]):
        with pytest.raises(ValueError):
            builder.sliding_windows(bad)
    with pytest.raises(ValueError):
        builder.from_spans(v, [])
    lib = _lib.SsnLibrary(pkg.build())
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = (ctypes.c_int * 2)(1, 2)
    zero = (ctypes.c_int * 2)(1, 0)
    a = ctypes.addressof
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_sw_count", None, 1, a(ok), a(ok), 2, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_sw_count", p, 1, None, None, 2, p, None)
    with pytest.raises(RuntimeError, match="must be at least 1"):
        lib.call("ssn_sw_count", p, 1, a(ok), a(zero), 2, p, None)
    with pytest.raises(RuntimeError, match="levels"):
        lib.call("ssn_sw_count", p, 1, a(ok), a(ok), 0, p, None)
    with pytest.raises(RuntimeError, match="levels"):
        lib.call("ssn_sw_fill", p, 1, a(ok), a(ok), 32, 5, p, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("ssn_sw_count", p, 0, a(ok), a(ok), 2, p, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("ssn_sw_fill", p, 1, a(ok), a(ok), 2, -1, p, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("ssn_sw_fill", p, 1, a(ok), a(ok), 2, 2 ** 30, p, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_sw_fill", None, 1, a(ok), a(ok), 2, 5, p, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_proposal_list_rows", p, p, 1, p, p, 1, None, None, 1, p, p, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.call("ssn_proposal_list_rows", None, p, 1, p, p, 1, p, p, 1, p, p, p, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("ssn_proposal_list_rows", p, p, 1, p, p, 1, p, p, 0, p, p, p, None)


def test_wrong_shapes_are_rejected(backend):
    dev = backend.device
    builder = ProposalListBuilder(device=dev)
    dur = torch.tensor([5.0, 6.0], dtype=torch.float64).to(dev)
    with pytest.raises(ValueError):
        K.sw_count(dur.float(), [1, 2], [1, 1])
    with pytest.raises(ValueError):
        K.sw_count(dur, [1, 2], [1])
    with pytest.raises(ValueError):
        K.sw_count(dur, [1, 2], [1, 0])
    off = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32).to(dev)
    with pytest.raises(ValueError):
        K.sw_fill(off.long(), [1, 2], [1, 1], 4)
    with pytest.raises(ValueError):
        K.sw_fill(off[:4].contiguous(), [1, 2], [1, 1], 3)
    with pytest.raises(ValueError):
        K.sw_fill(off, [1, 2], [1, 1], 2 ** 30)
    span = torch.zeros((3, 2), dtype=torch.float64).to(dev)
    o3 = torch.tensor([0, 1, 3], dtype=torch.int32).to(dev)
    fc = torch.tensor([5, 6], dtype=torch.int32).to(dev)
    for args in ((span.float(), o3, span, o3, fc, dur), (span, o3.long(), span, o3, fc, dur), (span, o3, span, o3[:2].contiguous(), fc, dur),
                 (span, o3, span, o3, fc.long(), dur), (span, o3, span, o3, fc, dur[:1].contiguous()), (span, o3, span.reshape(2, 3), o3, fc, dur)):
        with pytest.raises(ValueError):
            K.proposal_list_rows(*args)
    batch = builder.sliding_windows([video(5.0), video(6.0)])
    for bad in ([1], [1, 2, 3], [1.5, 2.0], [-1, 2], [1, 2 ** 31]):
        with pytest.raises(ValueError):
            builder.build(batch, bad)
    with pytest.raises(ValueError):
        builder.build(batch, [1, 2], recall_thresholds=[])
