"""``tools/detect_videos.py --flow on-the-fly`` against ``--flow files``: the same JSON and the same score pickle, byte for byte.

CPU tier: stub scorers through the command's ``make_ssn=`` / ``make_actionness=`` hooks whose scores are an exact integer function of
EVERY pixel they are handed, so that one differing flow pixel changes the output; everything else (the readers, the flow source, TAG,
the test table, pooling, post-processing, the grouping) is the product's, on the emulator.  Three tiny videos of 20 x 36 frames; their
flow files are written by the file chain (``FlowExtractor.extract`` -> ``tools/extract_flow.py``'s writer) with the TV-L1 parameters
the command is given.  GPU tier: the real ``BinaryClassifier`` and ``SSN`` of seeded checkpoints.
"""
import os
import sys

import numpy as np
import pytest
import torch

import action_detection_amd  # noqa: F401
from action_detection_amd import detect as DT
from action_detection_amd.optical_flow import TVL1, FlowExtractor
from test_detect import StubTester, identity
from test_flow_stream import clip, flow_tool, write_rgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import detect_videos as det  # noqa: E402

FRAMES = {"tiny_a": 26, "tiny_b": 32, "tiny_c": 20}      # RGB frames; flow bytes 2 * 20 * 36 * (T - 1): 36000, 44640, 27360
PAIRS = sum(t - 1 for t in FRAMES.values())
TVL1_FLAGS = ["--flow-nscales", "2", "--flow-warps", "2", "--flow-iterations", "10"]


def pixel_hash(frames, per_tick):
    """int64 [ticks]: an exact function of every pixel of the ``per_tick`` images of a tick (a host array or a tensor [n, H, W, 1])."""
    x = torch.as_tensor(np.asarray(frames.cpu() if torch.is_tensor(frames) else frames)).to(torch.int64)
    x = x.reshape(-1, per_tick, x.shape[1] * x.shape[2])
    weights = (torch.arange(x.shape[1] * x.shape[2], dtype=torch.int64).reshape(x.shape[1], -1) * 7919 + 13) % 1009
    return (x * weights).sum(dim=(1, 2))


class PixelTester(StubTester):
    """``StubTester`` whose frame scores depend on the pixels of the tick's ten flow images."""

    def frame_scores(self, frames_gen, frame_cnt, num_crop):
        h = torch.cat([pixel_hash(f, 10) for f in frames_gen])
        assert h.shape[0] == frame_cnt
        col = torch.arange(self.output_dim, dtype=torch.float64)
        phase = (h % 100003).to(torch.float64)[:, None] / 100003.0
        return (torch.sin(phase * 6.0 * (col + 1) + self.seed) * 2).float().to(self.device)


class PixelActionness(object):
    """``ActionnessTester.score_video``'s signature: foreground in bursts of four ticks, moved a little by the pixels."""

    def __init__(self, device):
        self.device = device

    def score_video(self, frames_gen, frame_cnt, num_crop=10):
        h = torch.cat([pixel_hash(f, 10) for f in frames_gen])
        assert h.shape[0] == frame_cnt
        tick = torch.arange(frame_cnt)
        fg = torch.where((tick // 4) % 2 == 1, 0.9, 0.004) + (h % 64).float() * 1e-4
        mean = torch.stack([1.0 - fg, fg], dim=1).float().to(self.device)
        return mean[:, None, :].expand(-1, num_crop, -1).contiguous(), mean


def stub_ssn(args, modality, weights, weight):
    assert modality == "Flow"
    return DT.Stream(PixelTester(args.device, num_class=args.num_class, seed=len(weights)), det.flow_reader(args), identity, 5, weight)


def stub_actionness(args, modality, weights, weight):
    assert modality == "Flow"
    return DT.Stream(PixelActionness(args.device), det.flow_reader(args), identity, 5, weight)


def write_videos(root, frames, device, extractor, h=20, w=36):
    """RGB frames and, by the file chain, their flow files."""
    tool = flow_tool()
    for k, (vid, t) in enumerate(sorted(frames.items())):
        write_rgb(root, vid, clip(20 + k, t=t, h=h, w=w))
        rgb = torch.from_numpy(tool.load_frames(os.path.join(root, vid), t)).to(device)
        tool.write_flow(os.path.join(root, vid), "flow_", extractor.extract(rgb).cpu().numpy(), 95)


def load(path):
    with open(path, "rb") as f:
        return f.read()


def run(tmp_path, root, name, extra, ssn=("Flow:a:1", "Flow:bb:1.5"), actionness=("Flow:c",)):
    out_json, scores = str(tmp_path / (name + ".json")), str(tmp_path / (name + ".pc"))
    argv = [root, out_json, "--dataset", "thumos14", "--ssn"] + list(ssn)
    argv += (["--actionness"] + list(actionness)) if actionness else ["--proposals", "sliding"]
    argv += ["--flow_pref", "flow_", "--fps", "5", "--test_crops", "1", "--tick_batch", "4", "--frame_interval", "2", "--actionness_interval",
             "1", "--device", "cpu", "--save-scores", scores] + list(extra)
    result = det.main(argv, make_ssn=stub_ssn, make_actionness=stub_actionness)
    return result, load(out_json), load(scores)


_MASTER = []


@pytest.fixture
def videos(emu, tmp_path, tmp_path_factory):
    """A copy of the frame root (one test removes files from it); the files are made once."""
    import shutil
    if not _MASTER:
        master = str(tmp_path_factory.mktemp("flow_driver") / "frames")
        write_videos(master, FRAMES, "cpu", FlowExtractor(TVL1(nscales=2, warps=2, iterations=10), bound=20))
        _MASTER.append(master)
    root = str(tmp_path / "frames")
    shutil.copytree(_MASTER[0], root)
    return root


def test_on_the_fly_writes_the_same_json_and_pickle(videos, tmp_path, capsys):
    files, files_json, files_pc = run(tmp_path, videos, "files", ["--flow", "files"])
    assert [v[1] for v in files.videos] == [t - 1 for _, t in sorted(FRAMES.items())]
    assert len(files.detections.rows) > 0
    # without the flag: the same bytes as with --flow files
    _, default_json, default_pc = run(tmp_path, videos, "default", [])
    assert default_json == files_json and default_pc == files_pc
    capsys.readouterr()
    fly, fly_json, fly_pc = run(tmp_path, videos, "fly", ["--flow", "on-the-fly"] + TVL1_FLAGS)
    assert fly_json == files_json and fly_pc == files_pc
    src = fly.flow_source
    assert len(fly.flow_groups) == 1 and (src.videos_computed, src.pairs_computed) == (3, PAIRS) and src.cache_hits > 0
    assert "1 groups of videos; 3 videos and %d pairs computed" % PAIRS in capsys.readouterr().out
    # the byte equality cannot pass by accident: one more TV-L1 iteration changes the output
    _, other_json, other_pc = run(tmp_path, videos, "other", ["--flow", "on-the-fly", "--flow-nscales", "2", "--flow-warps", "2",
                                                              "--flow-iterations", "11"])
    assert other_pc != files_pc


def test_on_the_fly_needs_no_flow_file(videos, tmp_path):
    _, files_json, files_pc = run(tmp_path, videos, "files", ["--flow", "files"])
    for vid in FRAMES:
        for name in os.listdir(os.path.join(videos, vid)):
            if name.startswith("flow_"):
                os.remove(os.path.join(videos, vid, name))
    _, fly_json, fly_pc = run(tmp_path, videos, "fly", ["--flow", "on-the-fly"] + TVL1_FLAGS)
    assert fly_json == files_json and fly_pc == files_pc


def test_two_groups_give_the_same_output_and_compute_every_pair_once(videos, tmp_path):
    _, files_json, files_pc = run(tmp_path, videos, "files", ["--flow", "files"])
    budget = 85000 / float(1 << 30)                                    # tiny_a + tiny_b fit (80640 bytes), tiny_c does not
    fly, fly_json, fly_pc = run(tmp_path, videos, "fly", ["--flow", "on-the-fly", "--flow-cache-gb", repr(budget)] + TVL1_FLAGS)
    assert fly.flow_groups == [[0, 1], [2]] and isinstance(fly, det.GroupedResults) and len(fly.results) == 2
    assert fly_json == files_json and fly_pc == files_pc
    src = fly.flow_source
    assert (src.videos_computed, src.pairs_computed) == (3, PAIRS)
    assert [v[0] for v in fly.videos] == sorted(FRAMES)
    # a budget below every video: one group per video, still every pair once
    one, one_json, one_pc = run(tmp_path, videos, "one", ["--flow", "on-the-fly", "--flow-cache-gb", "1e-9"] + TVL1_FLAGS)
    assert one.flow_groups == [[0], [1], [2]] and one_json == files_json and one_pc == files_pc
    assert one.flow_source.pairs_computed == PAIRS


def test_an_ssn_only_flow_stream_computes_only_the_pairs_it_reads(videos, tmp_path):
    """Sliding-window proposals, one SSN Flow stream at --frame_interval 6: five pairs of every six."""
    common = dict(ssn=("Flow:a",), actionness=())
    _, files_json, files_pc = run(tmp_path, videos, "files", ["--flow", "files", "--frame_interval", "6"], **common)
    fly, fly_json, fly_pc = run(tmp_path, videos, "fly", ["--flow", "on-the-fly", "--frame_interval", "6"] + TVL1_FLAGS, **common)
    assert fly_json == files_json and fly_pc == files_pc
    needed = sum(len(det.ssn_flow_pairs(5, 6, t - 1)) for t in FRAMES.values())
    assert fly.flow_source.pairs_computed == needed < PAIRS
    assert det.ssn_flow_pairs(5, 6, 25) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 18, 19, 20, 21, 22]


# ---------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_on_the_fly_with_real_networks_gpu(hip_library, tmp_path):
    """The command as a user runs it: Flow checkpoints on disk, RGB frames of 340 x 256, flow files of the file chain next to them.
    Spans exactly; scores to the tolerance tests/test_detect_driver.py allows between two runs of the backbone."""
    from action_detection_amd.binary_model import BinaryClassifier
    from action_detection_amd.ssn_models import SSN
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic
    from test_ssn_test_driver import compare_scores, load_scores, save_checkpoint
    torch.manual_seed(0)
    net = SSN(20, 2, 5, 2, "Flow", test_mode=True, stpp_cfg=(1, 1, 1))
    init_backbone_synthetic(net.base_model)
    init_heads_synthetic(net, std=0.05)
    ssn_weights = str(tmp_path / "ssn_flow.pth.tar")
    save_checkpoint(net, ssn_weights, np.array([[0.1, -0.3], [1.5, 0.7]]))
    binary = BinaryClassifier(2, 5, "Flow", base_model="BNInception", test_mode=True, new_length=5)
    init_backbone_synthetic(binary.base_model)
    bin_weights = str(tmp_path / "bin_flow.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.5, "state_dict": {"module." + k: v.detach().cpu().clone() for k, v in binary.state_dict().items()}},
               bin_weights)
    root = str(tmp_path / "frames")
    frames = {"vid0": 31, "vid1": 25}
    iterations = 30
    write_videos(root, frames, "cuda:0", FlowExtractor(TVL1(iterations=iterations), bound=20), h=256, w=340)
    outputs = {}
    for name, extra in (("files", ["--flow", "files"]), ("fly", ["--flow", "on-the-fly", "--flow-iterations", str(iterations)]),
                        ("fly_device", ["--flow", "on-the-fly", "--flow-iterations", str(iterations), "--gpu-decode", "--test_crops", "10"]),
                        ("files_device", ["--flow", "files", "--gpu-decode", "--test_crops", "10"])):
        out_json, pc = str(tmp_path / (name + ".json")), str(tmp_path / (name + ".pc"))
        result = det.main([root, out_json, "--dataset", "thumos14", "--ssn", "Flow:" + ssn_weights, "--actionness", "Flow:" + bin_weights,
                           "--flow_pref", "flow_", "--fps", "12", "--test_crops", "1", "--tick_batch", "16", "--save-scores", pc] + extra)
        outputs[name] = (result, load_scores(pc))
    for a, b in (("files", "fly"), ("files_device", "fly_device")):
        (want, want_scores), (got, got_scores) = outputs[a], outputs[b]
        assert [tuple(v) for v in got.videos] == [tuple(v) for v in want.videos] == [("vid0", 30, 2.5), ("vid1", 24, 2.0)]
        assert len(want.detections.rows) > 0
        for s, t in zip(got.spans, want.spans):
            assert np.array_equal(s, t)
        compare_scores(want_scores, got_scores)
        src = got.flow_source
        assert (src.videos_computed, src.pairs_computed) == (2, 30 + 24) and src.cache_hits > 0
