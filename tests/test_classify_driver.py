"""tools/classify_videos.py: the score-file path (--from-scores, two streams fused) and the network path (a five-class
BinaryClassifier on the five-layer backbone of tests/tiny_backbone.py) against the library calls it is made of."""
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest
import torch
from torch import nn

import action_detection_amd  # noqa: F401
from action_detection_amd.proposal_io import format_processed_record
from action_detection_amd.video_cls import VideoClassScores, VideoScoreAggregator, classification_metrics, fuse_scores

from tiny_backbone import TinyBackbone, init_tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CLASS = 5
VIDEOS = (("some/folder/vid_a", 8, 2), ("vid_b", 55, 5), ("vid_c", 14, 1))      # (frame folder, frames, label): 2, 9 and 3 ticks of 6


def tool():
    spec = importlib.util.spec_from_file_location("classify_videos_tool", os.path.join(ROOT, "tools", "classify_videos.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_list(path):
    with open(path, "w") as f:
        for i, (vid, frames, label) in enumerate(VIDEOS):
            f.write(format_processed_record(i + 1, vid, frames, [[label, 1, frames - 1]], [[label, 1.0, 1.0, 1, frames - 1]]))
    return {vid.split("/")[-1]: [label - 1] for vid, _, label in VIDEOS}


def printed_metrics(text):
    out = {}
    for key in ("top-1 accuracy", "top-3 accuracy", "video mAP", "mean class accuracy"):
        out[key] = float(re.search(re.escape(key) + r": (\S+)", text).group(1))
    return out


def same_metrics(printed, m):
    want = {"top-1 accuracy": m.top_k_accuracy[1], "top-3 accuracy": m.top_k_accuracy[3], "video mAP": m.mean_ap,
            "mean class accuracy": m.mean_class_accuracy}
    for key, val in want.items():
        assert "{:.6f}".format(val) == "{:.6f}".format(printed[key]), (key, val, printed[key])


def test_from_scores(backend, tmp_path, capsys):
    """Two synthetic tick-score pickles: the file is written, holds aggregate + fuse of the same data, and the printed
    metrics are classification_metrics of it."""
    labels = write_list(str(tmp_path / "list.txt"))
    rs = np.random.RandomState(0)
    files = []
    for s in range(2):
        pc = {vid: rs.randn(2 + 3 * i, 2, NUM_CLASS).astype(np.float32) for i, (vid, _, _) in enumerate(VIDEOS)}
        files.append(str(tmp_path / ("ticks%d.pc" % s)))
        with open(files[-1], "wb") as f:
            pickle.dump(pc, f, 2)
    out = str(tmp_path / "cls.pc")
    cls, m = tool().main(["thumos14", "RGB", "-", out, "--proposal-list", str(tmp_path / "list.txt"), "--num-class", str(NUM_CLASS),
                          "--agg", "top_k", "--k", "2", "--from-scores"] + files + ["--weights", "1", "1.5", "--device", str(backend.device)])
    text = capsys.readouterr().out
    agg = VideoScoreAggregator("top_k", k=2, normalization=False)
    parts = []
    for path in files:
        with open(path, "rb") as f:
            pc = pickle.load(f)
        parts.append(agg.aggregate({k.split("/")[-1]: backend.put(torch.from_numpy(v)) for k, v in pc.items()}))
    want = fuse_scores(parts[0], parts[1:], [1.5])
    assert cls.ids == want.ids == ["vid_a", "vid_b", "vid_c"] and torch.equal(cls.scores, want.scores)
    back = VideoClassScores.load(out, device=backend.device)
    assert back.ids == want.ids and torch.equal(back.scores.cpu(), want.scores.cpu())
    ref = classification_metrics(want, labels)
    assert m.videos_scored == 3 and "videos scored: 3" in text
    same_metrics(printed_metrics(text), ref)
    assert (m.top_k_accuracy, m.mean_ap) == (ref.top_k_accuracy, ref.mean_ap) or np.isnan(ref.mean_ap)


def tiny_classifier(monkeypatch, device):
    """BinaryClassifier(5 classes) whose backbone is the five-layer TinyBackbone, registered under the name 'Tiny'."""
    from action_detection_amd.binary_model import BinaryClassifier
    from action_detection_amd.ssn_models import SSN

    def ctor():
        b = init_tiny(TinyBackbone(3, 16))
        b.fc = nn.Linear(32, 1)      # (replaced by the classifier's dropout / identity; only in_features is read)
        return b
    monkeypatch.setitem(SSN._BACKBONES, "Tiny", (ctor, "fc", 16))
    torch.manual_seed(3)
    net = BinaryClassifier(NUM_CLASS, 5, "RGB", base_model="Tiny", test_mode=True, new_length=1)
    with torch.no_grad():
        net.classifier_fc.weight.copy_(torch.randn(NUM_CLASS, 32) * 0.5)
        net.classifier_fc.bias.copy_(torch.randn(NUM_CLASS) * 0.1)
    return net.to(device).eval()


def test_network_path(backend, monkeypatch, tmp_path, capsys):
    """Checkpoint -> BinaryClassifier -> ActionnessTester(grouping='tick') -> aggregation, on 3 videos of 2 to 9 ticks: the
    driver's scores equal the tester and the aggregator called directly."""
    from PIL import Image
    from action_detection_amd import transforms as T
    from action_detection_amd.actionness_sampling import ActionnessSampler
    from action_detection_amd.actionness_test import ActionnessTester
    from action_detection_amd.training import save_checkpoint
    mod = tool()
    labels = write_list(str(tmp_path / "list.txt"))
    net = tiny_classifier(monkeypatch, backend.device)
    save_checkpoint(net, 1, "Tiny", 0.5, False, str(tmp_path / "ckpt.pth.tar"), str(tmp_path / "best.pth.tar"))
    net.prepare_test_fc()      # (after the checkpoint: the trainer's file holds no test_fc)
    rs = np.random.RandomState(1)
    for vid, frames, _ in VIDEOS:
        os.makedirs(str(tmp_path / "frames" / vid))
        for idx in range(1, frames + 1):
            Image.fromarray(rs.randint(0, 256, (18, 18, 3)).astype(np.uint8)).save(
                str(tmp_path / "frames" / vid / "img_{:05d}.jpg".format(idx)), quality=95)
    out = str(tmp_path / "cls.pc")
    cls, m = mod.main(["thumos14", "RGB", str(tmp_path / "ckpt.pth.tar"), out, "--frame-root", str(tmp_path / "frames"),
                       "--proposal-list", str(tmp_path / "list.txt"), "--arch", "Tiny", "--num-class", str(NUM_CLASS),
                       "--test_crops", "1", "--tick_batch", "4", "--agg", "default", "--device", str(backend.device)])
    text = capsys.readouterr().out
    # the same, called directly
    sampler = ActionnessSampler(str(tmp_path / "list.txt"), new_length=1, test_interval=6)
    transform = T.Compose([T.GroupScale(net.scale_size), T.GroupScale(net.input_size), T.Stack(roll=True),
                           T.ToTorchFormatTensor(div=False), T.GroupNormalize(net.input_mean, net.input_std)])
    import extract_actionness as EA      # (tools/, on the path since the driver was loaded: the frame generator it uses)
    tester = ActionnessTester(net, tick_batch=4, grouping="tick")
    load = EA.pil_loader(str(tmp_path / "frames"), "RGB")
    raw = {}
    for video in sampler.video_list:
        n = len(sampler.test_ticks(video))
        assert 2 <= n <= 9
        raw[video.id.split("/")[-1]], _ = tester.score_video(EA.frame_batches(load, video, sampler, transform), n, num_crop=1)
    want = VideoScoreAggregator("default").aggregate(raw)
    assert cls.ids == want.ids == ["vid_a", "vid_b", "vid_c"]
    assert [raw[k].shape[0] for k in want.ids] == [2, 9, 3] and want.scores.shape == (3, NUM_CLASS)
    assert torch.equal(cls.scores, want.scores) and want.check() is want
    assert torch.equal(VideoClassScores.load(out, device=backend.device).scores.cpu(), want.scores.cpu())
    same_metrics(printed_metrics(text), classification_metrics(want, labels))
    assert m.videos_scored == 3
