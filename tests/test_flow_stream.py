"""``flow_stream.FlowStreamSource`` against the file chain it replaces, array for array: ``FlowExtractor.extract`` -> the writer of
``tools/extract_flow.py`` (PIL, quality 95) -> ``FrameDirReader(modality="Flow")``.  Every comparison is ``np.array_equal`` /
``torch.equal``.  The clips are seeded: 8 RGB frames of 20 x 36, a textured square moving two pixels a frame over a textured
background, saved as JPEG files with PIL; TV-L1 runs with 2 scales, 2 warps and 10 iterations so that the emulator finishes in seconds.
The file chain is made once per backend and shared.
"""
import importlib.util
import os
from collections import namedtuple

import numpy as np
import pytest
import torch
from PIL import Image

import action_detection_amd  # noqa: F401
from action_detection_amd import test_data as TD
from action_detection_amd.flow_stream import FlowStreamSource, chain_from_frames
from action_detection_amd.optical_flow import TVL1, FlowExtractor
from action_detection_amd.train_data import CompressedFrameDirReader, FrameDirReader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W = 8, 20, 36
VIDEOS = ("clip_a", "clip_b")
COUNTS = {v: T for v in VIDEOS}


def flow_tool():
    spec = importlib.util.spec_from_file_location("extract_flow_tool", os.path.join(ROOT, "tools", "extract_flow.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def clip(seed, t=T, h=H, w=W):
    """uint8 [t, h, w, 3]: a textured 8 x 8 square moving two pixels a frame (and one down every other frame)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    background = np.stack([110 + 50 * np.sin(xx / 4.0 + c) * np.cos(yy / 3.0 - c) for c in range(3)], 2) + rs.randint(-12, 12, (h, w, 3))
    square = rs.randint(30, 226, (8, 8, 3))
    frames = []
    for i in range(t):
        f = background.copy()
        y0, x0 = (4 + i // 2) % (h - 8), (3 + 2 * i) % (w - 8)      # (longer clips start over at the left edge)
        f[y0:y0 + 8, x0:x0 + 8] = square
        frames.append(np.clip(f, 0, 255).astype(np.uint8))
    return np.stack(frames)


def extractor():
    return FlowExtractor(TVL1(nscales=2, warps=2, iterations=10), bound=20, pair_batch=16)


def write_rgb(root, vid, frames):
    os.makedirs(os.path.join(root, vid))
    for i, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(root, vid, "img_%05d.jpg" % (i + 1)), quality=90)


_CHAINS = {}


@pytest.fixture
def chain(backend, tmp_path_factory):
    """(backend, frame root, FrameDirReader of the flow files the file chain wrote there) -- made once per backend."""
    if backend.name not in _CHAINS:
        root = str(tmp_path_factory.mktemp("flow_chain_" + backend.name))
        tool = flow_tool()
        for k, vid in enumerate(VIDEOS):
            write_rgb(root, vid, clip(3 + k))
            frames = torch.from_numpy(tool.load_frames(os.path.join(root, vid), T)).to(backend.device)
            flow = extractor().extract(frames)
            assert flow.shape == (T - 1, 2, H, W)
            tool.write_flow(os.path.join(root, vid), "flow_", flow.cpu().numpy(), 95)
        _CHAINS[backend.name] = root
    root = _CHAINS[backend.name]
    return backend, root, FrameDirReader(root, modality="Flow", flow_prefix="flow_")


def source_for(backend, root, **kw):
    kw.setdefault("extractor", extractor())
    reader = kw.pop("reader", FrameDirReader)
    return FlowStreamSource(reader(root, "RGB"), COUNTS, device=backend.device, **kw)


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


# ---------------------------------------------------------------------------------------------------------------- 1. equality
def test_the_clip_moves_and_the_files_are_lossy(chain):
    """On the file chain alone: the flow is not flat, and the JPEG file changed it (the round trip is not the identity)."""
    backend, root, files = chain
    got = files("clip_a", list(range(1, T)))
    assert got.shape == (2 * (T - 1), H, W, 1) and got.max() > 132
    frames = torch.from_numpy(flow_tool().load_frames(os.path.join(root, "clip_a"), T)).to(backend.device)
    raw = extractor().extract(frames).cpu().numpy().reshape(2 * (T - 1), H, W, 1)
    assert not np.array_equal(raw, got)


@pytest.mark.parametrize("numbers", [[1, 2, 3], [7, 7, 1]], ids=["first", "repeats-last-unordered"])
def test_source_returns_the_files_arrays(chain, numbers):
    backend, root, files = chain
    src = source_for(backend, root)
    got = src("clip_a", numbers)
    assert torch.is_tensor(got) and got.dtype == torch.uint8 and got.device.type == torch.device(backend.device).type
    assert np.array_equal(host(got), files("clip_a", numbers))
    assert (src.videos_computed, src.pairs_computed, src.cache_hits) == (1, T - 1, 0)
    assert np.array_equal(host(src("clip_a", numbers[::-1])), files("clip_a", numbers[::-1]))
    assert (src.videos_computed, src.pairs_computed, src.cache_hits) == (1, T - 1, 1)


_LONG = {}


@pytest.mark.parametrize("interval", [6, 5])
def test_source_serves_the_testers_tick_lists(chain, interval, tmp_path_factory):
    """The frame numbers ``test_frame_batches`` asks for at new_length 5, through that function itself, on a video of 20 RGB frames
    (19 flow frames: ticks 1, 7, 13 at interval 6 and 1, 6, 11 at interval 5; TV-L1 calls of 16 and 3 pairs)."""
    from action_detection_amd.detect import _TickRule
    backend = chain[0]
    t = 20
    if backend.name not in _LONG:
        root = str(tmp_path_factory.mktemp("flow_long_" + backend.name))
        tool = flow_tool()
        write_rgb(root, "clip_long", clip(9, t=t))
        frames = torch.from_numpy(tool.load_frames(os.path.join(root, "clip_long"), t)).to(backend.device)
        tool.write_flow(os.path.join(root, "clip_long"), "flow_", extractor().extract(frames).cpu().numpy(), 95)
        _LONG[backend.name] = root
    root = _LONG[backend.name]
    files = FrameDirReader(root, modality="Flow", flow_prefix="flow_")
    video = namedtuple("Video", "id num_frames")("clip_long", t - 1)
    asked = []

    def spy(reader):
        def read(vid, numbers):
            asked.append(list(numbers))
            return reader(vid, numbers)
        return read
    src = FlowStreamSource(FrameDirReader(root, "RGB"), {"clip_long": t}, extractor(), device=backend.device)
    want = list(TD.test_frame_batches(_TickRule(5, interval), video, spy(files), np.asarray, tick_batch=2))
    got = list(TD.test_frame_batches(_TickRule(5, interval), video, spy(src), host, tick_batch=2))
    first = {6: [1, 7, 13], 5: [1, 6, 11]}[interval]
    assert len(want) == len(got) == 2 and asked[:2] == asked[2:]
    assert asked[0] + asked[1] == [p + x for p in first for x in range(5)]
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert (src.videos_computed, src.pairs_computed, src.cache_hits) == (1, t - 1, 1)


def test_both_outputs_and_both_readers_give_the_same_arrays(chain):
    backend, root, files = chain
    numbers = [2, 5, 7, 1]
    want = files("clip_a", numbers)
    on_host = source_for(backend, root, output="host")("clip_a", numbers)
    assert isinstance(on_host, np.ndarray) and on_host.dtype == np.uint8 and np.array_equal(on_host, want)
    compressed = source_for(backend, root, reader=CompressedFrameDirReader)
    assert isinstance(compressed.reader("clip_a", [1])[0], bytes)
    assert np.array_equal(host(compressed("clip_a", numbers)), want)
    assert compressed._decoder is not None and compressed._decoder.fallbacks == 0


# ---------------------------------------------------------------------------------------------------------------- 2. prepare
def test_prepared_pairs_and_a_later_pair_equal_the_full_computation(chain):
    backend, root, files = chain
    full = files("clip_a", list(range(1, T)))
    src = source_for(backend, root)
    src.prepare("clip_a", pairs=[0, 1, 2, 3, 4])
    assert (src.videos_computed, src.pairs_computed) == (1, 5)
    entry = src._cache["clip_a"]
    assert entry.present.tolist() == [True] * 5 + [False] * 2
    assert np.array_equal(host(src("clip_a", [1, 2, 3, 4, 5])), full[:10])
    assert (src.pairs_computed, src.cache_hits) == (5, 1)
    assert np.array_equal(host(src("clip_a", [7, 3])), np.concatenate([full[12:14], full[4:6]]))      # pair 6: on demand
    assert (src.videos_computed, src.pairs_computed, src.cache_hits) == (1, 6, 1)
    assert entry.present.tolist() == [True] * 5 + [False, True]
    assert np.array_equal(host(src("clip_a", list(range(1, T)))), full)                                # row for row
    assert (src.videos_computed, src.pairs_computed) == (1, 7)
    with pytest.raises(IndexError, match="clip_a"):
        src.prepare("clip_a", pairs=[T - 1])


def test_chunks_and_batches_do_not_change_a_pixel(chain):
    """Three pairs a TV-L1 call, six pairs an RGB read: two reads, three calls -- against files written from one call of seven."""
    backend, root, files = chain
    reads = []

    class Spy(FrameDirReader):
        def __call__(self, vid, numbers):
            reads.append(list(numbers))
            return super(Spy, self).__call__(vid, numbers)
    src = FlowStreamSource(Spy(root, "RGB"), COUNTS, FlowExtractor(TVL1(nscales=2, warps=2, iterations=10), bound=20, pair_batch=3),
                           device=backend.device, chunk_batches=2)
    assert np.array_equal(host(src("clip_b", list(range(1, T)))), files("clip_b", list(range(1, T))))
    assert reads == [[1, 2, 3, 4, 5, 6, 7], [7, 8]] and src.pairs_computed == T - 1


# ---------------------------------------------------------------------------------------------------------------- 3. the cache
def test_a_budget_of_one_video_evicts_and_recomputes_the_same_bytes(chain):
    backend, root, files = chain
    one = 2 * H * W * (T - 1)
    src = source_for(backend, root, cache_bytes=one)
    numbers = [1, 4, 7]
    want = {v: files(v, numbers) for v in VIDEOS}
    for k, vid in enumerate(["clip_a", "clip_b", "clip_a", "clip_b"]):
        assert np.array_equal(host(src(vid, numbers)), want[vid])
        assert src.cached_videos() == [vid]
        assert (src.videos_computed, src.pairs_computed, src.cache_hits) == (k + 1, (k + 1) * (T - 1), 0)
    assert np.array_equal(host(src("clip_b", numbers)), want["clip_b"])
    assert (src.videos_computed, src.cache_hits) == (4, 1)
    # twice the budget keeps both: the least recently used one leaves first when a third arrives
    both = source_for(backend, root, cache_bytes=2 * one)
    for vid in ("clip_a", "clip_b", "clip_a", "clip_b"):
        assert np.array_equal(host(both(vid, numbers)), want[vid])
    assert (both.videos_computed, both.pairs_computed, both.cache_hits) == (2, 2 * (T - 1), 2)
    assert both.cached_videos() == ["clip_a", "clip_b"]
    # a budget below one video keeps that video alone
    tiny = source_for(backend, root, cache_bytes=1)
    assert np.array_equal(host(tiny("clip_a", numbers)), want["clip_a"]) and tiny.cached_videos() == ["clip_a"]
    assert np.array_equal(host(tiny("clip_a", numbers)), want["clip_a"]) and tiny.cache_hits == 1


# ---------------------------------------------------------------------------------------------------------------- 4. arguments
def test_numbers_outside_the_video_raise_index_error(chain):
    backend, root, files = chain
    src = source_for(backend, root)
    for bad in ([0], [1, T], [-1]):
        with pytest.raises(IndexError, match="clip_a"):
            src("clip_a", bad)
    assert src.videos_computed == 0                       # (refused before anything was computed)
    with pytest.raises(KeyError):
        src("unknown", [1])
    with pytest.raises(ValueError, match="output"):
        FlowStreamSource(FrameDirReader(root, "RGB"), COUNTS, output="pinned")
    with pytest.raises(ValueError, match="quality"):
        FlowStreamSource(FrameDirReader(root, "RGB"), COUNTS, quality=0)
    with pytest.raises(ValueError, match="RGB"):
        FlowStreamSource(FrameDirReader(root, "Flow"), COUNTS)


# ---------------------------------------------------------------------------------------------------------------- 5. the chain from frames
@pytest.mark.parametrize("modality,crops", [("RGB", 10), ("Flow", 10), ("Flow", 1)])
def test_device_chain_from_frames_equals_the_chain_from_blobs(chain, modality, crops):
    backend, root, files = chain
    numbers = [1, 2, 3, 4, 5]
    blobs = CompressedFrameDirReader(root, modality, "flow_")("clip_a", numbers)
    mean, std = ([104.0, 117.0, 128.0], [1.0, 1.0, 1.0]) if modality == "RGB" else ([128.0], [1.0])
    tc = TD.DeviceTestChain(16, 18, mean, std, modality, crops, backend.device)
    want = tc(blobs)
    decoded = tc.decoder.decode(blobs, tc.mode, stack=True)
    assert decoded.shape == (len(blobs), H, W, 3 if modality == "RGB" else 1)
    got = chain_from_frames(tc, decoded)
    assert got.shape == want.shape and torch.equal(got, want) and tc.host_scaled == 0
    if modality == "Flow":      # and from the source: the same input as the files give
        src = source_for(backend, root)
        assert torch.equal(chain_from_frames(tc, src("clip_a", numbers)), want)
    with pytest.raises(ValueError, match="chain_from_frames"):
        chain_from_frames(tc, decoded.float())


@pytest.mark.parametrize("modality,crops", [("RGB", 10), ("Flow", 1)])
def test_frames_past_the_scale_ratio_take_the_host_branch_of_both(backend, tmp_path, modality, crops):
    """120 x 130 frames under a scale size of 18 shrink by more than the scale kernel's ratio of 6: ``DeviceTestChain(blobs)`` and
    ``chain_from_frames`` both scale with PIL on the host, and give the same input."""
    big = clip(6, t=3, h=120, w=130)
    folder = str(tmp_path / "big")
    os.makedirs(folder)
    for i, f in enumerate(big):
        Image.fromarray(f).save(os.path.join(folder, "img_%05d.jpg" % (i + 1)), quality=90)
        for axis, c in (("x", 0), ("y", 1)):
            Image.fromarray(np.ascontiguousarray(f[:, :, c])).save(os.path.join(folder, "flow_%s_%05d.jpg" % (axis, i + 1)), quality=95)
    blobs = CompressedFrameDirReader(str(tmp_path), modality, "flow_")("big", [1, 2, 3])
    mean, std = ([104.0, 117.0, 128.0], [1.0, 1.0, 1.0]) if modality == "RGB" else ([128.0], [1.0])
    tc = TD.DeviceTestChain(16, 18, mean, std, modality, crops, backend.device)
    want = tc(blobs)
    assert tc.host_scaled == 1
    decoded = tc.decoder.decode(blobs, tc.mode, stack=True)
    assert decoded.shape[1:3] == (120, 130)
    got = chain_from_frames(tc, decoded)
    assert tc.host_scaled == 2 and got.shape == want.shape and torch.equal(got, want)


def test_flow_bytes_come_from_the_readers_first_frame(chain):
    backend, root, files = chain
    want = 2 * H * W * (T - 1)
    for reader in (FrameDirReader, CompressedFrameDirReader):
        src = source_for(backend, root, reader=reader)
        assert src.flow_bytes("clip_a") == want and src.videos_computed == 0
        src("clip_a", [1])
        assert src.flow_bytes("clip_a") == want == src._cache["clip_a"].nbytes
