"""detect.ActionDetector against the file chain it replaces, step by step and bit for bit: actionness scores -> TAG ->
ProposalListBuilder.build -> list file text -> load_proposal_file -> ProposalSampler(exclude_empty=False).test_ticks ->
DenseTester.score_video -> DetectionPostProcessor.process_videos.

* CPU tier (emulator): the scorers are stubs whose per-tick scores are a fixed function of (video, frame number); the pooling,
  de-normalisation, TAG, list, table and post-processing kernels run as in the product.
* gpu: a real BinaryClassifier and SSN on JPEG frames.
"""
import json
import os
import pickle
from collections import namedtuple

import numpy as np
import pytest
import torch

import action_detection_amd  # noqa: F401
from action_detection_amd import detect as DT
from action_detection_amd import proposal_io
from action_detection_amd import test_data as TD
from action_detection_amd.dense_test import DenseTester
from action_detection_amd.detection_eval import merge_detection_scores
from action_detection_amd.detection_post import DetectionPostProcessor
from action_detection_amd.ops.ssn_ops import STPPReorgainzed
from action_detection_amd.proposal_lists import ProposalListBuilder
from action_detection_amd.proposal_sampling import ProposalSampler
from action_detection_amd.tag_proposals import TagProposalGenerator, merge_scores_device, sliding_window_proposals

NUM_CLASS = 3
ListVideo = namedtuple("ListVideo", "id duration instances")

# (video id, frames, duration in seconds); the stub actionness below gives v0 and v1 bursts, v2 one burst, v3 nothing
VIDEOS = [("v0", 300, 10.0), ("v1", 452, 15.5), ("v2", 120, 4.0), ("v3", 200, 7.0)]
NUMBER = {v[0]: i for i, v in enumerate(VIDEOS)}


def frame_reader(calls=None):
    """reader(video id, frame numbers) -> float32 [n, 2] of (video number, frame number): the 'pixels' of the CPU tier."""
    def read(vid, idx):
        if calls is not None:
            calls.append(vid)
        return torch.tensor([[NUMBER[vid], f] for f in idx], dtype=torch.float32)
    return read


def identity(frames):
    return frames


class StubActionness(object):
    """``ActionnessTester.score_video``'s signature: foreground in bursts whose length depends on the video, none in v3."""

    def __init__(self, device, new_length=1, phase=0):
        self.device, self.new_length, self.phase = device, new_length, phase

    def score_video(self, frames_gen, frame_cnt, num_crop=10):
        x = torch.cat(list(frames_gen))[::self.new_length]
        assert x.shape[0] == frame_cnt
        vid, f = x[:, 0].long(), x[:, 1].long() + self.phase
        burst = torch.tensor([35, 50, 60, 1])[vid]
        fg = torch.where(((f // burst) % 2 == 1) & (vid != 3), 0.9 - 0.001 * (f % 7).float(), torch.full_like(x[:, 0], 0.004))
        # (TAG takes the softmax of the two scores: a background score of 12 puts v3's foreground below its lowest threshold)
        mean = torch.stack([torch.where(vid == 3, 12.0, 1.0) - fg, fg], dim=1).float().to(self.device)
        return mean[:, None, :].expand(-1, num_crop, -1).contiguous(), mean


class StubTester(DenseTester):
    """A DenseTester whose backbone + test_fc is a fixed function of (video, frame number); ``score_video``,
    ``score_video_ranges`` and the tail behind them are the product's."""

    def __init__(self, device, stpp_cfg=(1, 1, 1), new_length=1, seed=0, regression=True, num_class=NUM_CLASS):
        mult = sum(c if isinstance(c, int) else sum(c) for c in stpp_cfg)
        self.num_class, self.with_regression = num_class, regression
        self.output_dim = num_class + 1 + (num_class + (2 * num_class if regression else 0)) * mult
        self.reorg = STPPReorgainzed(self.output_dim, num_class + 1, num_class, num_class * 2, True, with_regression=regression,
                                     stpp_cfg=stpp_cfg)
        self.stats = np.array([[0.1, -0.3], [1.5, 0.7]])
        self.device, self.new_length, self.seed = device, new_length, seed
        self.videos_scored = []

    def frame_scores(self, frames_gen, frame_cnt, num_crop):
        x = torch.cat(list(frames_gen))[::self.new_length]
        assert x.shape[0] == frame_cnt
        self.videos_scored.append(int(x[0, 0]))
        col = torch.arange(self.output_dim, dtype=torch.float32)
        out = torch.sin(x[:, 1:2] * (0.013 + 0.002 * self.seed) * (col + 1) + x[:, 0:1] + self.seed) * 2
        return out.to(self.device)


def make_detector(device, ssn=None, actionness=None, post=None, **kw):
    ssn = ssn or [DT.Stream(StubTester(device), frame_reader(), identity, 1)]
    actionness = actionness if actionness is not None else [DT.Stream(StubActionness(device), frame_reader(), identity, 1)]
    post = post or DetectionPostProcessor(NUM_CLASS, 0.4, top_k=50)
    return DT.ActionDetector(ssn, actionness, TagProposalGenerator(device=device), post, frame_interval=6, actionness_interval=5,
                             test_crops=1, tick_batch=16, device=device, **kw)


def file_chain(tmp_path, device, videos, spans, testers, readers, transforms, new_lengths, stpp_cfg, frame_interval=6, crops=1,
               tick_batch=16):
    """From the proposals in seconds on: list file -> records -> sampler -> score_video per stream.
    -> (records, one sampler per stream, one score dictionary (numpy, as in a pickle) per stream)."""
    builder = ProposalListBuilder(device)
    listed = [ListVideo(v[0], v[2], []) for v in videos]
    built = builder.build(builder.from_spans(listed, spans), [v[1] for v in videos])
    assert not any(built.status)
    path = str(tmp_path / "list.txt")
    proposal_io.write_proposal_file(path, [proposal_io.format_window_list_rows(v[0], v[1], *built.rows(i))
                                           for i, v in enumerate(videos)])
    records = proposal_io.load_proposal_file(path)
    samplers, dicts = [], []
    for tester, reader, transform, nl in zip(testers, readers, transforms, new_lengths):
        sampler = ProposalSampler(records=records, exclude_empty=False, reg_stats=np.zeros((2, 2)), new_length=nl,
                                  test_interval=frame_interval)
        assert [v.id for v in sampler.video_list] == [v[0] for v in videos]
        scores = {}
        for video in sampler.video_list:
            ticks, rel, pticks, scaling = sampler.test_ticks(video)
            gen = TD.test_frame_batches(sampler, video, reader, transform, tick_batch)
            act, comp, reg, _ = tester.score_video(gen, len(ticks), torch.from_numpy(pticks), torch.from_numpy(scaling), num_crop=crops)
            scores[video.id] = (rel, act.cpu().numpy(), comp.cpu().numpy(), None if reg is None else reg.cpu().numpy())
        samplers.append(sampler)
        dicts.append(scores)
    return records, samplers, dicts


def assert_table_equals_sampler(table, sampler):
    for i, video in enumerate(sampler.video_list):
        ticks, rel, pticks, scaling = sampler.test_ticks(video)
        rows = table.video(i)
        assert table.n_rows[i] == len(ticks)
        assert np.array_equal(rows.rel.cpu().numpy(), rel.reshape(-1, 2))
        assert np.array_equal(rows.ticks.cpu().numpy(), pticks)
        assert np.array_equal(rows.scaling.cpu().numpy(), scaling.reshape(-1, 2))


def assert_scores_equal(got, want):
    assert list(got) == list(want)
    for vid in want:
        for a, b in zip(got[vid], want[vid]):
            assert (a is None) == (b is None)
            if b is not None:
                a = a.cpu().numpy()
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), vid


def assert_detections_equal(got, want):
    for name in ("rows", "cls", "vid", "prop", "row_off", "combined", "p_off"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert got.video_ids == want.video_ids and len(got.rows) > 0


def check_against_file_chain(tmp_path, device, detector, videos, result, reference_actionness):
    """Every step of ``result`` against the file chain fed with the same videos."""
    # spans: generate's, from scores computed outside the detector
    want_spans = [r.seconds for r in detector.tag.generate([reference_actionness[v[0]] for v in videos], [v[2] for v in videos])]
    assert len(result.spans) == len(want_spans)
    for a, b in zip(result.spans, want_spans):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    streams = detector.ssn
    records, samplers, dicts = file_chain(tmp_path, device, videos, want_spans, [s.scorer for s in streams], [s.reader for s in streams],
                                          [s.transform for s in streams], [s.new_length for s in streams], detector.stpp_cfg,
                                          detector.frame_interval, detector.test_crops, detector.tick_batch)
    # frame numbers: those of the list file's text
    frames, p_off = result.frames.cpu().numpy(), result.p_off
    for i, rec in enumerate(records):
        listed = np.asarray([[int(x[3]), int(x[4])] for x in rec[3]], dtype=np.int32).reshape(-1, 2)
        assert rec[1] == videos[i][1] and np.array_equal(frames[p_off[i]:p_off[i + 1]], listed)
    # the table(s): test_ticks of the records
    for st, sampler in zip(streams, samplers):
        assert_table_equals_sampler(result.tables[st.new_length], sampler)
    return records, samplers, dicts


# ---------------------------------------------------------------------------------------------------------------------- CPU tier
def test_detect_equals_the_file_chain(emu, tmp_path):
    dev = "cpu"
    detector = make_detector(dev)
    result = detector.detect(VIDEOS)
    kept = [len(s) for s in result.spans]
    # TAG itself decides the proposals of two videos; one video has none and takes the whole-video row
    assert sum(k >= 5 for k in kept) >= 2 and kept[3] == 0, kept
    assert result.table.src[result.table.h_k_off[3]:result.table.h_k_off[4]].tolist() == [-1]
    reference = {v[0]: StubActionness(dev).score_video(
        TD.test_frame_batches(DT._TickRule(1, 5), DT._Video(*v), frame_reader(), identity, 16),
        len(np.arange(0, v[1] - 1, 5)), 1)[1] for v in VIDEOS}
    for vid in reference:
        assert torch.equal(result.actionness[vid], reference[vid])
    records, samplers, dicts = check_against_file_chain(tmp_path, dev, detector, VIDEOS, result, reference)
    assert_scores_equal(result.scores, dicts[0])
    want = detector.post.process_videos(dicts[0], device=dev)
    assert_detections_equal(result.detections, want)


@pytest.mark.parametrize("weights", [None, (1.0, 1.5)], ids=["equal-weights", "weights"])
def test_two_streams_fuse_as_merge_detection_scores(emu, tmp_path, weights):
    """A second stream with 5 frames per tick (its own table: the ticks differ), another STPP-compatible scorer, two actionness
    streams merged on the device."""
    dev = "cpu"
    cfg = (1, (1, 2), 1)
    w = weights or (None, None)
    ssn = [DT.Stream(StubTester(dev, cfg, 1, seed=0), frame_reader(), identity, 1, w[0]),
           DT.Stream(StubTester(dev, cfg, 5, seed=3), frame_reader(), identity, 5, w[1])]
    actionness = [DT.Stream(StubActionness(dev), frame_reader(), identity, 1, 1.0),
                  DT.Stream(StubActionness(dev, 5, phase=4), frame_reader(), identity, 5, 0.5)]
    detector = make_detector(dev, ssn, actionness, DetectionPostProcessor(NUM_CLASS, 0.4, top_k=0))
    videos = VIDEOS[:3]
    result = detector.detect(videos)
    assert detector.stpp_cfg == ((1,), (1, 2), (1,)) and set(result.tables) == {1, 5}
    per_stream = []
    for st in actionness:
        per_stream.append({v[0]: st.scorer.score_video(
            TD.test_frame_batches(DT._TickRule(st.new_length, 5), DT._Video(*v), st.reader, identity, 16),
            len(np.arange(0, v[1] - st.new_length, 5)), 1)[1] for v in videos})
    reference = merge_scores_device(per_stream, [1.0, 0.5])
    records, samplers, dicts = check_against_file_chain(tmp_path, dev, detector, videos, result, reference)
    assert any(not np.array_equal(result.tables[1].video(i).ticks.cpu().numpy(), result.tables[5].video(i).ticks.cpu().numpy())
               for i in range(len(videos)))
    merged = merge_detection_scores(dicts, list(weights) if weights else None)
    assert merged[videos[0][0]][1].dtype == (np.float64 if weights else np.float32)
    assert_scores_equal(result.scores, merged)
    assert_detections_equal(result.detections, detector.post.process_videos(merged, device=dev))


def test_given_proposals_and_scores_skip_their_steps(emu, tmp_path):
    dev = "cpu"
    a_calls, s_calls = [], []
    detector = make_detector(dev, [DT.Stream(StubTester(dev), frame_reader(s_calls), identity, 1)],
                             [DT.Stream(StubActionness(dev), frame_reader(a_calls), identity, 1)])
    full = detector.detect(VIDEOS)
    assert set(a_calls) == set(NUMBER) and set(s_calls) == set(NUMBER)
    # actionness_scores=: nothing is read for the actionness stream, everything else is as before (host arrays or tensors)
    del a_calls[:]
    given = detector.detect(VIDEOS, actionness_scores={k: v.numpy() for k, v in full.actionness.items()})
    assert a_calls == []
    for a, b in zip(given.spans, full.spans):
        assert np.array_equal(a, b)
    assert_detections_equal(given.detections, full.detections)
    # proposals=: neither actionness nor TAG (a detector without either)
    bare = DT.ActionDetector([DT.Stream(StubTester(dev), frame_reader(), identity, 1)], None, None, detector.post, test_crops=1,
                             tick_batch=16, device=dev)
    windows = [np.asarray(sliding_window_proposals(v[2]), dtype=np.float64) for v in VIDEOS]
    got = bare.detect(VIDEOS, proposals=windows)
    assert got.actionness is None and all(np.array_equal(a, b) for a, b in zip(got.spans, windows))
    records, samplers, dicts = file_chain(tmp_path, dev, VIDEOS, windows, [bare.ssn[0].scorer], [frame_reader()], [identity], [1],
                                          (1, 1, 1))
    assert_scores_equal(got.scores, dicts[0])
    assert_detections_equal(got.detections, bare.post.process_videos(dicts[0], device=dev))
    with pytest.raises(ValueError, match="proposals="):
        bare.detect(VIDEOS)
    # video_cls_scores= reaches the post-processor
    cls_scores = {v[0]: np.array([0.1, 0.7, 0.2]) for v in VIDEOS}
    filtered = bare.detect(VIDEOS, proposals=windows, video_cls_scores=cls_scores)
    assert_detections_equal(filtered.detections, bare.post.process_videos(dicts[0], device=dev, video_cls_scores=cls_scores))
    assert set(filtered.detections.cls.tolist()) == {1}


def test_results_round_trip(emu, tmp_path):
    dev = "cpu"
    result = make_detector(dev).detect(VIDEOS)
    path = str(tmp_path / "scores.pc")
    result.save_scores(path)
    with open(path, "rb") as f:
        loaded = pickle.load(f)
    assert list(loaded) == [v[0] for v in VIDEOS]
    for vid, parts in loaded.items():
        assert isinstance(parts, tuple) and len(parts) == 4 and parts[0].dtype == np.float64 and parts[1].dtype == np.float32
        for a, b in zip(parts, result.scores[vid]):
            assert np.array_equal(a, b.cpu().numpy())
    # the pickle is what the evaluation tool's post-processing takes
    assert_detections_equal(DetectionPostProcessor(NUM_CLASS, 0.4, top_k=50).process_videos(loaded, device=dev), result.detections)
    names = ["run", "jump", "throw"]
    out = json.loads(json.dumps(result.to_activitynet(names)))
    assert set(out) == {"version", "results", "external_data"} and out["external_data"] == {}
    assert list(out["results"]) == [v[0] for v in VIDEOS]
    host = result.detections.to_host()
    for vid, frames, duration in VIDEOS:
        rows = np.concatenate([host[vid][c] for c in sorted(host[vid])]) if host[vid] else np.zeros((0, 5))
        labels = [names[c] for c in sorted(host[vid]) for _ in range(len(host[vid][c]))]
        entries = out["results"][vid]
        assert len(entries) == len(rows) and [e["label"] for e in entries] == labels
        for e, r in zip(entries, rows):
            assert e["score"] == r[2] and e["segment"] == [r[0] * duration, r[1] * duration]
    assert sum(len(e) for e in out["results"].values()) == len(result.detections.rows) > 0
    with pytest.raises(ValueError):
        result.to_activitynet(names[:2])


# ---------------------------------------------------------------------------------------------------------------------- GPU tier
def write_frames(root, counts, h=256, w=340):
    from PIL import Image
    videos = []
    for v, n in enumerate(counts):
        folder = os.path.join(str(root), "vid%d" % v)
        os.makedirs(folder)
        rs = np.random.RandomState(50 + v)
        yy, xx = np.mgrid[0:h, 0:w]
        for i in range(1, n + 1):
            # a moving pattern whose contrast changes along the video: the scores of neighbouring ticks differ
            base = np.stack([127 + (40 + 60 * ((i // 9) % 2)) * np.sin(xx / (9.0 + c) + 0.3 * i + v) * np.cos(yy / 6.0 - c) for c in range(3)], axis=2)
            pic = np.clip(base + rs.randint(-10, 11, size=(h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(pic).save(os.path.join(folder, "img_%05d.jpg" % i), quality=85)
        videos.append(("vid%d" % v, n, n / 12.0))
    return videos


@pytest.mark.gpu
def test_detect_end_to_end_gpu(hip_library, tmp_path):
    from action_detection_amd import train_data as D
    from action_detection_amd.actionness_test import ActionnessTester
    from action_detection_amd.binary_model import BinaryClassifier
    from action_detection_amd.ssn_models import SSN
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic
    dev = "cuda:0"
    torch.manual_seed(0)
    binary = BinaryClassifier(2, 5, "RGB", base_model="BNInception", test_mode=True, new_length=1)
    init_backbone_synthetic(binary.base_model)
    rs = np.random.RandomState(7)
    with torch.no_grad():
        binary.classifier_fc.weight.copy_(torch.from_numpy((rs.standard_normal(tuple(binary.classifier_fc.weight.shape)) * 0.5).astype(np.float32)))
        binary.classifier_fc.bias.zero_()
    binary.prepare_test_fc()
    binary.to(dev).eval()
    net = SSN(NUM_CLASS, 2, 5, 2, "RGB", test_mode=True, stpp_cfg=(1, 1, 1))
    init_backbone_synthetic(net.base_model)
    init_heads_synthetic(net, std=0.05)
    net.prepare_test_fc()
    net.to(dev).eval()
    videos = write_frames(tmp_path, (61, 37, 25))
    reader = D.FrameDirReader(str(tmp_path), "RGB")
    chain = TD.host_test_chain(net.input_size, net.scale_size, net.input_mean, net.input_std, 1)
    tester = DenseTester(net, NUM_CLASS, stats=np.array([[0.1, -0.3], [1.5, 0.7]]), tick_batch=16)
    scorer = ActionnessTester(binary, tick_batch=16)
    detector = DT.ActionDetector([DT.Stream(tester, reader, chain, 1)], [DT.Stream(scorer, reader, chain, 1)],
                                 TagProposalGenerator(device=dev), DetectionPostProcessor(NUM_CLASS, 0.4, top_k=50),
                                 frame_interval=6, actionness_interval=5, test_crops=1, tick_batch=16, device=dev)
    # The backbone stores every activation with a power-of-two scale taken from the maxima its PREVIOUS pass recorded (planes_exec:
    # delayed scales), so the low bits of a pass depend on what ran before it.  One round over the videos first: from then on every
    # pass over a video follows the same predecessor in the detector's run and in the file chain's, and equality is exact.
    detector.detect(videos)
    scorer.score_video(TD.test_frame_batches(DT._TickRule(1, 5), DT._Video(*videos[-1]), reader, chain, 16),
                       len(np.arange(0, videos[-1][1] - 1, 5)), 1)
    result = detector.detect(videos)
    print("proposals per video:", [len(s) for s in result.spans], "detections:", len(result.detections.rows))
    assert any(len(s) for s in result.spans)            # (TAG's own proposals are scored, not whole-video fallback rows alone)
    reference = {v[0]: scorer.score_video(TD.test_frame_batches(DT._TickRule(1, 5), DT._Video(*v), reader, chain, 16),
                                          len(np.arange(0, v[1] - 1, 5)), 1)[1] for v in videos}
    for vid in reference:
        assert torch.equal(result.actionness[vid], reference[vid])
    records, samplers, dicts = check_against_file_chain(tmp_path, dev, detector, videos, result, reference)
    assert_scores_equal(result.scores, dicts[0])
    assert_detections_equal(result.detections, detector.post.process_videos(dicts[0], device=dev))
    out = result.to_activitynet(["a", "b", "c"])
    assert sum(len(e) for e in out["results"].values()) == len(result.detections.rows)
