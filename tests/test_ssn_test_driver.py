"""The SSN testing driver (tools/test_ssn.py) and its frame source (action_detection_amd/test_data.py).

* CPU tier, emulator: ``test_frame_batches`` with the device chain (compressed files -> JpegDecoder -> GroupScale -> ten crops) and
  with the PIL reader + host chain, both against a literal restatement of the reference's generator (ssn_dataset.py:434-450).
* CPU tier, no kernel library: the worker plumbing with a stub tester -- spawned workers against the in-process run, the pickles'
  layout, the worker limit, and a worker that dies (host processes only: nothing here opens a GPU).
* gpu: the whole driver on a synthetic-initialised SSN, host chain against ``--gpu-decode`` and against the oracle's reference loop.
"""
import os
import pickle
import signal
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import action_detection_amd  # noqa: F401
import ssn_oracle as O
from action_detection_amd import proposal_io
from action_detection_amd import test_data as TD
from action_detection_amd import train_data as D
from action_detection_amd import transforms as T
from action_detection_amd.proposal_sampling import ProposalSampler
from test_kernels import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))     # (by name, so that spawned workers can import it too)
import test_ssn as drv  # noqa: E402


def picture(h, w, seed):
    """A smooth picture with some texture (what a JPEG file of a video frame holds)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(xx / 7.0 + seed + c) * np.cos(yy / 5.0 - c) for c in range(3)], axis=2)
    return np.clip(base + rs.randint(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


def write_videos(root, frame_counts, h, w, modality):
    """<root>/v<i>/img_00001.jpg ... (RGB) or x_/y_ (Flow) and a proposal list naming them -> the list's path."""
    records = []
    for v, n in enumerate(frame_counts):
        folder = os.path.join(str(root), "v%d" % v)
        os.makedirs(folder, exist_ok=True)
        for i in range(1, n + 1):
            pic = picture(h, w, 100 * v + i)
            if modality == "RGB":
                Image.fromarray(pic).save(os.path.join(folder, "img_%05d.jpg" % i), quality=90)
            else:
                Image.fromarray(pic[:, :, 0]).save(os.path.join(folder, "x_%05d.jpg" % i), quality=90)
                Image.fromarray(pic[:, :, 1]).save(os.path.join(folder, "y_%05d.jpg" % i), quality=90)
        # one frame per second: spans in seconds are spans in frames
        props = [(1, 0.8, 0.9, 1, n - 3), (0, 0.0, 0.0, 0, 3), (1, 0.4, 0.5, n // 2, n - 1)]
        records.append(proposal_io.format_window_list_record("v%d" % v, n, n, [(0, (1, n - 2))], props))
    path = os.path.join(str(root), "proposal_list.txt")
    proposal_io.write_proposal_file(path, records)
    return path


def reference_frame_gen(folder, frame_cnt, frame_ticks, new_length, modality, transform, batchsize):
    """ssn_dataset.py:434-450 with _load_image (:208-215), literally."""
    def load_image(idx):
        if modality == "RGB":
            return [Image.open(os.path.join(folder, "img_{:05d}.jpg".format(idx))).convert("RGB")]
        return [Image.open(os.path.join(folder, "x_{:05d}.jpg".format(idx))).convert("L"),
                Image.open(os.path.join(folder, "y_{:05d}.jpg".format(idx))).convert("L")]
    frames = []
    cnt = 0
    for idx, seg_ind in enumerate(frame_ticks):
        p = int(seg_ind)
        for x in range(new_length):
            frames.extend(load_image(min(frame_cnt, p + x)))
        cnt += 1
        if cnt % batchsize == 0:
            frames = transform(frames)
            yield frames
            frames = []
    if len(frames):
        frames = transform(frames)
        yield frames


@pytest.mark.parametrize("modality,interval,crops", [("RGB", 2, 10), ("Flow", 1, 10), ("RGB", 3, 1)])
def test_frame_batches(emu, tmp_path, modality, interval, crops):
    """2 videos of 14 and 9 frames of 18 x 25 (GroupScale(24) upscales them to 24 x 33), tick_batch 4 with a tail.  The ticks stop at
    frame_cnt - new_length, so ``min(frame_cnt, p + x)`` reaches frame_cnt - 1 at most: the last frame read is asserted below."""
    new_length = 1 if modality == "RGB" else 5
    mean = [104, 117, 128] if modality == "RGB" else [128]
    plist = write_videos(tmp_path, (14, 9), 18, 25, modality)
    sampler = ProposalSampler(plist, new_length=new_length, test_interval=interval, reg_stats=np.zeros((2, 2)))
    assert [v.num_frames for v in sampler.video_list] == [14, 9]
    cropping = [T.GroupOverSample(20, 24)] if crops == 10 else [T.GroupScale(24), T.GroupCenterCrop(20)]
    ref_tf = T.Compose(cropping + [T.Stack(roll=True), T.ToTorchFormatTensor(div=False), T.GroupNormalize(mean, [1])])
    device_chain = TD.DeviceTestChain(20, 24, mean, [1], modality, crops, device="cpu")
    host_chain = TD.host_test_chain(20, 24, mean, [1], crops)
    length = (3 if modality == "RGB" else 2) * new_length
    tails = 0
    for video in sampler.video_list:
        ticks = sampler.test_ticks(video)[0]
        want = list(reference_frame_gen(os.path.join(str(tmp_path), video.id), video.num_frames, ticks, new_length, modality, ref_tf, 4))
        seen = []

        def spy(reader):
            def read(vid, idx):
                seen.extend(idx)
                return reader(vid, idx)
            return read
        dev = list(TD.test_frame_batches(sampler, video, spy(D.CompressedFrameDirReader(str(tmp_path), modality)), device_chain, 4))
        host = list(TD.test_frame_batches(sampler, video, D.FrameDirReader(str(tmp_path), modality), host_chain, tick_batch=4))
        assert len(dev) == len(host) == len(want) == -(-len(ticks) // 4)
        for a, b, w in zip(dev, host, want):
            assert a.shape == b.shape == w.shape and a.shape[1:] == (20, 20)
            assert torch.equal(a, w) and torch.equal(b, w)
        assert sum(a.shape[0] for a in dev) == len(ticks) * crops * length
        assert max(seen) == int(ticks[-1]) + new_length - 1 <= video.num_frames - 1
        tails += len(ticks) % 4 != 0
    assert tails >= 1 and device_chain.host_scaled == 0 and device_chain.decoder.fallbacks == 0


def test_device_chain_scales_oversized_frames_on_the_host(emu, tmp_path):
    """Frames more than 6x the scale size leave the device path: PIL decodes and scales them, the device crops; counted."""
    Image.fromarray(picture(30, 40, 1)).save(str(tmp_path / "a.jpg"), quality=90)
    blob = (tmp_path / "a.jpg").read_bytes()
    chain = TD.DeviceTestChain(3, 4, [104, 117, 128], [1], "RGB", 10, device="cpu")
    got = chain([blob, blob])
    want = T.Compose([T.GroupOverSample(3, 4), T.Stack(roll=True), T.ToTorchFormatTensor(div=False),
                      T.GroupNormalize([104, 117, 128], [1])])([Image.open(str(tmp_path / "a.jpg")).convert("RGB")] * 2)
    assert chain.host_scaled == 1 and torch.equal(got, want)
    # a file the device decoder does not take (progressive) AND beyond the cap goes the same way instead of failing in scale() ...
    Image.fromarray(picture(30, 40, 1)).save(str(tmp_path / "p.jpg"), quality=90, progressive=True)
    prog = (tmp_path / "p.jpg").read_bytes()
    want = T.Compose([T.GroupOverSample(3, 4), T.Stack(roll=True), T.ToTorchFormatTensor(div=False),
                      T.GroupNormalize([104, 117, 128], [1])])([Image.open(str(tmp_path / "p.jpg")).convert("RGB")] * 2)
    assert torch.equal(chain([prog, prog]), want) and chain.host_scaled == 2 and chain.host_decoded == 0
    # ... and within the cap it is decoded by PIL inside the decoder, scaled on the device, and counted
    small = TD.DeviceTestChain(20, 24, [104, 117, 128], [1], "RGB", 10, device="cpu")
    want = T.Compose([T.GroupOverSample(20, 24), T.Stack(roll=True), T.ToTorchFormatTensor(div=False),
                      T.GroupNormalize([104, 117, 128], [1])])([Image.open(str(tmp_path / "p.jpg")).convert("RGB")] * 2)
    assert torch.equal(small([prog, prog]), want) and small.host_scaled == 0 and small.host_decoded == 2


# ------------------------------------------------------------------------------------------------------------- worker plumbing
NUM_CLASS = 20


class StubTester(object):
    """Pure torch, deterministic in the video id: the tuple an SSNVideoTester returns."""

    def __init__(self, args, device, die_on_call=None):
        self.sampler = drv.load_videos(args)
        self.calls, self.die_on_call = 0, die_on_call

    def __call__(self, index):
        self.calls += 1
        if self.calls == self.die_on_call:
            os._exit(3)
        video = self.sampler.video_list[index]
        ticks, rel_props, _, _ = self.sampler.test_ticks(video)
        g = torch.Generator().manual_seed(zlib.crc32(video.id.encode()))
        p = len(rel_props)
        return (video.id, rel_props, torch.randn(p, NUM_CLASS + 1, generator=g).numpy(), torch.randn(p, NUM_CLASS, generator=g).numpy(),
                torch.randn(p, NUM_CLASS, 2, generator=g).numpy(), torch.randn(len(ticks), 7, generator=g).numpy())


def make_stub_tester(args, device):
    return StubTester(args, device)


def make_dying_tester(args, device):
    return StubTester(args, device, die_on_call=2)


class time_limit(object):
    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        def expired(signum, frame):
            raise AssertionError("the driver did not end within %d s" % self.seconds)
        self.old = signal.signal(signal.SIGALRM, expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.old)


def five_videos(tmp_path):
    records = []
    for v, n in enumerate((20, 31, 14, 25, 40)):
        props = [(1, 0.8, 0.9, 1, n - 3), (0, 0.0, 0.0, 0, 3), (2, 0.4, 0.5, n // 2, n - 1)][:2 + v % 2]
        records.append(proposal_io.format_window_list_record("videos/v%d" % v, n, n, [(0, (1, n - 2))], props))
    path = str(tmp_path / "proposal_list.txt")
    proposal_io.write_proposal_file(path, records)
    return path


def test_workers_equal_the_in_process_run(tmp_path):
    plist = five_videos(tmp_path)
    common = ["thumos14", "RGB", "no_weights.pth.tar"]
    with time_limit(60):
        solo = drv.main(common + [str(tmp_path / "solo.pc"), "--proposal-list", plist, "--save_raw_scores", str(tmp_path / "solo_raw.pc")],
                        make_tester=make_stub_tester)
        drv.main(common + [str(tmp_path / "pool.pc"), "--proposal-list", plist, "--save_raw_scores", str(tmp_path / "pool_raw.pc"),
                           "-j", "2"], make_tester=make_stub_tester)
    with open(str(tmp_path / "solo.pc"), "rb") as f:
        a = pickle.load(f)
    with open(str(tmp_path / "pool.pc"), "rb") as f:
        b = pickle.load(f)
    with open(str(tmp_path / "solo_raw.pc"), "rb") as f:
        ra = pickle.load(f)
    with open(str(tmp_path / "pool_raw.pc"), "rb") as f:
        rb = pickle.load(f)
    ids = {"videos/v%d" % v for v in range(5)}
    assert set(a) == set(b) == set(ra) == set(rb) == set(solo) == ids
    for vid in ids:
        assert isinstance(b[vid], tuple) and len(b[vid]) == 4
        rel, act, comp, reg = b[vid]
        p = rel.shape[0]
        assert rel.dtype == np.float64 and rel.shape == (p, 2) and p in (2, 3)
        assert act.dtype == np.float32 and act.shape == (p, NUM_CLASS + 1)
        assert comp.dtype == np.float32 and comp.shape == (p, NUM_CLASS)
        assert reg.dtype == np.float32 and reg.shape == (p, NUM_CLASS, 2)
        for x, y in zip(a[vid], b[vid]):
            assert np.array_equal(x, y)
        assert rb[vid].ndim == 2 and rb[vid].dtype == np.float32 and np.array_equal(ra[vid], rb[vid])


def test_worker_limit_and_rgbdiff(tmp_path):
    plist = five_videos(tmp_path)
    with pytest.raises(ValueError):
        drv.main(["thumos14", "RGB", "w", str(tmp_path / "s.pc"), "--proposal-list", plist, "-j", "17"], make_tester=make_stub_tester)
    with pytest.raises(NotImplementedError):
        drv.main(["thumos14", "RGBDiff", "w", str(tmp_path / "s.pc"), "--proposal-list", plist], make_tester=make_stub_tester)
    assert not os.path.exists(str(tmp_path / "s.pc"))


def test_a_dead_worker_ends_the_run(tmp_path):
    """A worker process that exits with status 3 on its second video: the driver reports the exit code instead of waiting for a result
    that never comes, and starts no replacement."""
    plist = five_videos(tmp_path)
    with time_limit(60):
        with pytest.raises(RuntimeError, match="exit code 3"):
            drv.main(["thumos14", "RGB", "w", str(tmp_path / "s.pc"), "--proposal-list", plist, "-j", "2"],
                     make_tester=make_dying_tester)
    assert not os.path.exists(str(tmp_path / "s.pc"))


# ------------------------------------------------------------------------------------------------------------- the driver on the GPU
def save_checkpoint(net, path, stats):
    torch.save({"epoch": 3, "best_loss": 1.25, "arch": "BNInception",
                "state_dict": {"module." + k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                "reg_stats": torch.from_numpy(stats)}, path)


def load_scores(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def compare_scores(a, b, tol=1e-4):
    assert set(a) == set(b) and len(a) > 0
    for vid in a:
        assert np.array_equal(a[vid][0], b[vid][0]) and a[vid][0].dtype == np.float64
        for k, (x, y) in enumerate(zip(a[vid][1:], b[vid][1:])):
            assert x.dtype == y.dtype == np.float32 and x.shape == y.shape
            err = rel_err(torch.from_numpy(x), torch.from_numpy(y))
            print("video %s, output %d: rel err %.3g" % (vid, k, err))
            assert err < tol, (vid, k, err)


@pytest.mark.gpu
def test_driver_host_chain_gpu_decode_and_oracle(hip_library, tmp_path):
    from action_detection_amd.ssn_models import SSN
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic
    num_class = 20
    torch.manual_seed(0)
    net = SSN(num_class, 2, 5, 2, "RGB", test_mode=True, stpp_cfg=(1, 1, 1))
    init_backbone_synthetic(net.base_model)
    init_heads_synthetic(net, std=0.05)
    stats = np.array([[0.1, -0.3], [1.5, 0.7]])
    weights = str(tmp_path / "ssn.pth.tar")
    save_checkpoint(net, weights, stats)
    plist = write_videos(tmp_path, (13, 13), 72, 96, "RGB")
    common = ["thumos14", "RGB", weights]
    tail = ["--proposal-list", plist, "--frame-root", str(tmp_path), "--frame_interval", "2", "--test_crops", "10", "--tick_batch", "4"]
    drv.main(common + [str(tmp_path / "host.pc"), "--save_raw_scores", str(tmp_path / "host_raw.pc")] + tail)
    drv.main(common + [str(tmp_path / "dev.pc"), "--gpu-decode"] + tail)
    host, dev = load_scores(str(tmp_path / "host.pc")), load_scores(str(tmp_path / "dev.pc"))
    assert set(host) == {"v0", "v1"}
    compare_scores(host, dev)
    # the spawned-worker path on a real device: a fresh child makes cuda:0 its current device, builds the tester and scores one video
    drv.main(common + [str(tmp_path / "pool.pc"), "--gpu-decode", "-j", "1", "--gpus", "0", "--max_num", "1"] + tail)
    pool = load_scores(str(tmp_path / "pool.pc"))
    assert set(pool) == {"v0"}
    compare_scores(pool, {"v0": dev["v0"]})

    # one video against the oracle's restatement of the reference loop, fed by the host chain
    oracle = O.OracleSSN(num_class, 2, 5, 2, "RGB", test_mode=True, stpp_cfg=(1, 1, 1))
    oracle.load_state_dict(net.state_dict())
    oracle.prepare_test_fc()
    oracle.eval()
    sampler = ProposalSampler(plist, new_length=1, test_interval=2, reg_stats=np.zeros((2, 2)))
    video = sampler.video_list[0]
    ticks, rel, pticks, scaling = sampler.test_ticks(video)
    chain = TD.host_test_chain(224, 256, [104, 117, 128], [1], 10)
    gen = TD.test_frame_batches(sampler, video, D.FrameDirReader(str(tmp_path), "RGB"), chain, 4)
    r_act, r_comp, r_reg, r_out = O.dense_test_video(oracle, gen, len(ticks), pticks, scaling, num_class, num_crop=10, stats=stats)
    got = host[video.id]
    assert np.array_equal(got[0], rel)
    for k, (x, y) in enumerate(zip(got[1:], (r_act, r_comp, r_reg))):
        err = rel_err(torch.from_numpy(x), torch.from_numpy(np.asarray(y)))
        print("against the oracle, output %d: rel err %.3g" % (k, err))
        assert err < 1e-4, (k, err)
    raw = load_scores(str(tmp_path / "host_raw.pc"))[video.id]
    assert raw.shape == r_out.shape and rel_err(torch.from_numpy(raw), torch.from_numpy(r_out)) < 1e-4


@pytest.mark.gpu
def test_driver_flow_one_crop(hip_library, tmp_path):
    from action_detection_amd.ssn_models import SSN
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic
    torch.manual_seed(1)
    net = SSN(20, 2, 5, 2, "Flow", test_mode=True, stpp_cfg=(1, 1, 1))
    init_backbone_synthetic(net.base_model)
    init_heads_synthetic(net, std=0.05)
    weights = str(tmp_path / "ssn_flow.pth.tar")
    save_checkpoint(net, weights, np.array([[0.0, 0.1], [1.0, 2.0]]))
    plist = write_videos(tmp_path, (11,), 72, 96, "Flow")
    common = ["thumos14", "Flow", weights]
    tail = ["--proposal-list", plist, "--frame-root", str(tmp_path), "--frame_interval", "2", "--test_crops", "1", "--tick_batch", "2"]
    drv.main(common + [str(tmp_path / "host.pc")] + tail)
    drv.main(common + [str(tmp_path / "dev.pc"), "--gpu-decode"] + tail)
    compare_scores(load_scores(str(tmp_path / "host.pc")), load_scores(str(tmp_path / "dev.pc")))


def test_extract_actionness_gpu_scale(emu, tmp_path):
    """tools/extract_actionness.py --gpu-decode --gpu-scale: frames of any size; without --gpu-scale they are still refused."""
    import importlib.util
    import io
    spec = importlib.util.spec_from_file_location("extract_actionness_tool", os.path.join(ROOT, "tools", "extract_actionness.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    class Net(object):
        input_size, scale_size, input_mean, input_std = 20, 24, [104, 117, 128], [1]
    files = []
    for seed in (1, 2):
        b = io.BytesIO()
        Image.fromarray(picture(18, 25, seed)).save(b, "JPEG", quality=90)
        files.append(b.getvalue())
    got = tool.device_transform(Net, "RGB", "cpu", scale=True)(files)
    host = T.Compose([T.GroupOverSample(20, 24), T.Stack(roll=True), T.ToTorchFormatTensor(div=False), T.GroupNormalize([104, 117, 128], [1])])
    assert torch.equal(got, host([Image.open(io.BytesIO(f)).convert("RGB") for f in files]))
    with pytest.raises(ValueError, match="short side"):
        tool.device_transform(Net, "RGB", "cpu")(files)
