"""A video's optical flow as a frame source: what ``FrameDirReader(modality="Flow")`` reads from the ``flow_x_%05d.jpg`` /
``flow_y_%05d.jpg`` files of ``tools/extract_flow.py``, computed from the RGB frames when it is asked for and kept on the device.

    source = FlowStreamSource(FrameDirReader(root, "RGB"), {"video": 120})
    source("video", [1, 2, 3])          # uint8 [6, H, W, 1]: x and y image of the pairs (1, 2), (2, 3), (3, 4)

The chain per pair is the file chain's: ``rgb_to_gray`` -> ``TVL1`` -> ``flow_to_uint8(bound)`` -> the pixels a JPEG file of
``quality`` gives back (``jpeg_encode.roundtrip_gray``: the networks were trained on those, not on the quantised flow itself).  The
result equals the file chain's bit for bit.  Nothing is read back to the host on the way, except what ``JpegDecoder``
reads for compressed RGB frames.
"""
from collections import OrderedDict

import numpy as np
import torch

from .jpeg_encode import roundtrip_gray
from .optical_flow import FlowExtractor, flow_to_uint8, rgb_to_gray


class _Entry(object):
    """The flow of one video: ``flow`` uint8 [T - 1, 2, H, W] on the device; ``present`` (host) marks the rows that are computed."""

    def __init__(self, flow, present):
        self.flow, self.present = flow, present

    @property
    def nbytes(self):
        return self.flow.numel()


class FlowStreamSource(object):
    """``source(video_id, frame_numbers)`` with the signature and the result of ``FrameDirReader(modality="Flow")``: for every flow
    frame number f (1-based: the pair of RGB frames f and f + 1) the x and then the y image, uint8 [2 n, H, W, 1] -- a device tensor
    (``output="device"``, for ``chain_from_frames``) or a numpy array (``output="host"``, for ``host_test_chain``).

    rgb_reader: a ``FrameDirReader`` (decoded arrays, uploaded) or ``CompressedFrameDirReader`` (bytes, decoded on the device) of
    modality RGB.  frame_counts: ``{video id: RGB frames T}``; the video has T - 1 flow frames, a number outside 1 .. T - 1 raises
    ``IndexError``.  extractor: a ``FlowExtractor`` (TV-L1 parameters, bound, pairs per launch set).

    The first request for a video computes its whole flow into a cache of ``cache_bytes`` that drops the least recently used video
    first (a video larger than the budget is kept alone).  The RGB frames are read ``chunk_batches * pair_batch + 1`` at a time, so
    a long video is never resident as RGB, and each chunk runs through TV-L1 ``pair_batch`` pairs at a time, as
    ``FlowExtractor.extract`` does it.  (A call of the device decoder costs nearly as much for 17 files as for 289: with one read
    per TV-L1 batch, ``chunk_batches=1``, the source is 2.6 x slower than the file chain; profiles/flow_stream_measured.txt.)  ``prepare(video_id, pairs)`` computes only the given
    pairs; others follow when they are asked for.
    ``videos_computed`` / ``pairs_computed`` / ``cache_hits`` count cache fills, TV-L1 pairs and requests served without computing."""

    def __init__(self, rgb_reader, frame_counts, extractor=None, quality=95, cache_bytes=16 << 30, output="device", device="cuda:0",
                 chunk_batches=64):
        if output not in ("device", "host"):
            raise ValueError("FlowStreamSource: output is 'device' or 'host', got %r" % (output,))
        if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
            raise ValueError("FlowStreamSource: quality is an integer 1 .. 100, got %r" % (quality,))
        if getattr(rgb_reader, "modality", "RGB") != "RGB":
            raise ValueError("FlowStreamSource: the reader must deliver RGB frames")
        self.reader, self.frame_counts = rgb_reader, dict(frame_counts)
        self.extractor = extractor if extractor is not None else FlowExtractor()
        self.quality, self.cache_bytes, self.output = quality, int(cache_bytes), output
        self.device = torch.device(device)
        if int(chunk_batches) < 1:
            raise ValueError("FlowStreamSource: chunk_batches is at least 1")
        self.chunk_pairs = int(chunk_batches) * self.extractor.pair_batch
        self._cache = OrderedDict()
        self._decoder = None
        self.videos_computed = self.pairs_computed = self.cache_hits = 0

    # ---- RGB side
    def _rgb(self, video_id, first, last):
        """RGB frames first .. last (1-based, inclusive) -> uint8 [n, H, W, 3] on the device."""
        got = self.reader(video_id, list(range(first, last + 1)))
        if isinstance(got, (list, tuple)):                      # the files' bytes
            if self._decoder is None:
                from .jpeg_decode import JpegDecoder
                self._decoder = JpegDecoder(self.device)
            return self._decoder.decode(list(got), "RGB", stack=True)
        return torch.from_numpy(np.ascontiguousarray(got)).to(self.device)

    # ---- the cache
    def _pairs_of(self, video_id):
        if video_id not in self.frame_counts:
            raise KeyError("FlowStreamSource: no frame count for video %r" % (video_id,))
        t = int(self.frame_counts[video_id])
        if t < 2:
            raise ValueError("FlowStreamSource: video %r has %d RGB frames, flow needs at least 2" % (video_id, t))
        return t - 1

    def flow_bytes(self, video_id):
        """Bytes the flow of a video takes in the cache, 2 H W (T - 1), with H and W of the first frame the RGB reader delivers (the
        header of its file where the reader hands out bytes)."""
        n_pairs = self._pairs_of(video_id)
        entry = self._cache.get(video_id)
        if entry is not None:
            return entry.nbytes
        first = self.reader(video_id, [1])
        if isinstance(first, (list, tuple)):
            import io
            from PIL import Image
            with Image.open(io.BytesIO(first[0])) as im:      # (reads the header only)
                w, h = im.size
        else:
            h, w = first.shape[1:3]
        return 2 * int(h) * int(w) * n_pairs

    def _evict(self, keep):
        total = sum(e.nbytes for e in self._cache.values())
        for vid in list(self._cache):
            if total <= self.cache_bytes:
                break
            if vid != keep:
                total -= self._cache.pop(vid).nbytes

    @torch.no_grad()
    def _compute(self, video_id, pairs):
        """Computes the rows ``pairs`` (0-based, sorted, all absent) of the video's entry, which is created on the first call."""
        n_pairs = self._pairs_of(video_id)
        entry = self._cache.get(video_id)
        batch, chunk = self.extractor.pair_batch, self.chunk_pairs
        runs, k = [], 0
        while k < len(pairs):                                    # runs of consecutive pairs, at most `chunk` long
            j = k + 1
            while j < len(pairs) and pairs[j] == pairs[j - 1] + 1 and j - k < chunk:
                j += 1
            runs.append((pairs[k], j - k))
            k = j
        for p0, n in runs:
            gray = rgb_to_gray(self._rgb(video_id, p0 + 1, p0 + n + 1))
            if entry is None:
                flow = torch.empty((n_pairs, 2, gray.shape[1], gray.shape[2]), device=self.device, dtype=torch.uint8)
                entry = self._cache[video_id] = _Entry(flow, np.zeros(n_pairs, dtype=bool))
                self.videos_computed += 1
                self._evict(video_id)
            h, w = entry.flow.shape[2:]
            if tuple(gray.shape[1:]) != (h, w):
                raise ValueError("FlowStreamSource: the frames of video %r differ in size" % (video_id,))
            for s in range(0, n, batch):                         # (a whole video: the launches of FlowExtractor.extract)
                e = min(s + batch, n)
                quantised = flow_to_uint8(self.extractor.tvl1(gray[s:e], gray[s + 1:e + 1]).flow, self.extractor.bound)
                roundtrip_gray(quantised.view(2 * (e - s), h, w), self.quality,
                               out=entry.flow[p0 + s:p0 + e].view(2 * (e - s), h, w))
            entry.present[p0:p0 + n] = True
            self.pairs_computed += n
        return entry

    def _ensure(self, video_id, pairs):
        """The video's entry with the rows ``pairs`` computed (None: all of them); -> (entry, whether anything was computed)."""
        n_pairs = self._pairs_of(video_id)
        entry = self._cache.get(video_id)
        wanted = np.arange(n_pairs) if pairs is None else np.unique(np.asarray(pairs, dtype=np.int64))
        missing = wanted if entry is None else wanted[~entry.present[wanted]]
        if len(missing):
            entry = self._compute(video_id, [int(p) for p in missing])
        self._cache.move_to_end(video_id)
        return entry, bool(len(missing))

    def prepare(self, video_id, pairs=None):
        """Compute the flow of ``pairs`` (0-based: pair p is flow frame p + 1; None: every pair) of a video ahead of its requests."""
        n_pairs = self._pairs_of(video_id)
        if pairs is not None:
            pairs = [int(p) for p in pairs]
            if any(p < 0 or p >= n_pairs for p in pairs):
                raise IndexError("FlowStreamSource: video %r has the pairs 0 .. %d" % (video_id, n_pairs - 1))
        self._ensure(video_id, pairs)

    def cached_videos(self):
        """Ids of the videos in the cache, least recently used first."""
        return list(self._cache)

    # ---- the reader's call
    @torch.no_grad()
    def __call__(self, video_id, frame_numbers):
        n_pairs = self._pairs_of(video_id)
        numbers = [int(f) for f in frame_numbers]
        for f in numbers:
            if f < 1 or f > n_pairs:
                raise IndexError("FlowStreamSource: video %r has the flow frames 1 .. %d, got %d" % (video_id, n_pairs, f))
        rows = [f - 1 for f in numbers]
        # a video that is not in the cache is computed whole; one that `prepare` filled in part gets the rows that are asked for
        entry, computed = self._ensure(video_id, None if video_id not in self._cache else rows)
        self.cache_hits += int(not computed)
        idx = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(self.device)
        h, w = entry.flow.shape[2:]
        out = entry.flow.index_select(0, idx).view(2 * len(rows), h, w, 1)
        return out if self.output == "device" else out.cpu().numpy()


def chain_from_frames(chain, frames):
    """The tail of ``test_data.DeviceTestChain.__call__`` for frames that are decoded and on the device already (this source's
    output): ``chain`` is a ``DeviceTestChain``, ``frames`` uint8 [n, H, W, C].  The scale-ratio check is made on the tensor's own
    size; frames past it are scaled with PIL on the host, as ``__call__`` does it, and counted in ``chain.host_scaled``.  Both
    branches are held against ``chain(blobs)`` in tests/test_flow_stream.py.  (A function beside the source and not a method: a
    change may not touch ``test_data.py``; ``functools.partial(chain_from_frames, chain)`` is the transform.)"""
    from PIL import Image
    from . import kernels as K
    from .input_pipeline import scaled_size
    from .transforms import GroupScale
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.dtype != torch.uint8:
        raise ValueError("chain_from_frames: a uint8 tensor [n, H, W, C] is expected")
    scale = chain.scale_size
    hh, w = int(frames.shape[1]), int(frames.shape[2])
    ow, oh = scaled_size(w, hh, scale)
    if not K.frames_scale_supported(hh, w, oh, ow):
        host = frames.cpu().numpy()
        ims = GroupScale(scale)([Image.fromarray(f if f.shape[2] == 3 else f[:, :, 0]) for f in host])
        a = np.stack([np.asarray(im) for im in ims])
        frames, scale = torch.from_numpy(a if a.ndim == 4 else a[:, :, :, None]).to(chain.tf.mean.device), None
        chain.host_scaled += 1
    if chain.test_crops == 10:
        return chain.tf.oversample(frames, scale_size=scale)
    return chain.tf.center_crop(frames, scale_size=scale)
