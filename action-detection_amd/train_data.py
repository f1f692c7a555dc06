"""Batch sources of the training drivers (tools/train_ssn.py, tools/train_binary.py): what the reference's ``SSNDataSet`` /
``BinaryDataSet`` + ``DataLoader`` deliver (/root/reference/ssn_dataset.py:347-391, load_binary_score.py:243-262), split the way
this library runs it -- the host only picks proposals and decodes, ``TrainingBatchPrefetcher`` uploads the uint8 frames and
``GpuTrainAugment`` crops, resizes, flips and normalises on the device.

Every source yields the prefetcher's item: ``(frames uint8 [videos, images, H, W, C], scaling, target, reg_target, prop_type)``.
The actionness sources leave the three fields the binary loop does not have as zeros; ``binary_view`` drops them again.
"""
import os

import numpy as np

from .input_pipeline import GpuTrainAugment


class FrameDirReader(object):
    """Decoded frames of ``<root>/<video id>/img_00001.jpg`` ... (RGB) or ``<flow_prefix>x_00001.jpg`` / ``y_`` (Flow) with PIL,
    as ``_load_image`` of the reference does (ssn_dataset.py:208-215).  -> uint8 [n, H, W, C], C = 3 (RGB) or 1 (Flow, x then y)."""

    def __init__(self, root, modality="RGB", flow_prefix=""):
        self.root, self.modality, self.flow_prefix = root, modality, flow_prefix

    def _open(self, path, mode):
        from PIL import Image
        with Image.open(path) as im:
            a = np.asarray(im.convert(mode))
        return a if a.ndim == 3 else a[:, :, None]

    def __call__(self, video_id, indices):
        d = video_id if os.path.isabs(video_id) else os.path.join(self.root, video_id)
        out = []
        for i in indices:
            if self.modality in ("RGB", "RGBDiff"):
                out.append(self._open(os.path.join(d, "img_{:05d}.jpg".format(int(i))), "RGB"))
            else:
                out.append(self._open(os.path.join(d, self.flow_prefix + "x_{:05d}.jpg".format(int(i))), "L"))
                out.append(self._open(os.path.join(d, self.flow_prefix + "y_{:05d}.jpg".format(int(i))), "L"))
        return np.stack(out)


class CompressedFrameDirReader(FrameDirReader):
    """The same files as ``FrameDirReader``, undecoded: -> list of ``bytes``, one per image (Flow: x then y), for
    ``jpeg_decode.CompressedBatchPrefetcher``, which decodes them on the device."""

    def _open(self, path, mode):
        with open(path, "rb") as f:
            return f.read()

    def __call__(self, video_id, indices):
        d = video_id if os.path.isabs(video_id) else os.path.join(self.root, video_id)
        out = []
        for i in indices:
            if self.modality in ("RGB", "RGBDiff"):
                out.append(self._open(os.path.join(d, "img_{:05d}.jpg".format(int(i))), "RGB"))
            else:
                out.append(self._open(os.path.join(d, self.flow_prefix + "x_{:05d}.jpg".format(int(i))), "L"))
                out.append(self._open(os.path.join(d, self.flow_prefix + "y_{:05d}.jpg".format(int(i))), "L"))
        return out


class SyntheticReader(object):
    """Seeded noise frames of the decoded size, a stand-in for a frame directory (``--synthetic``)."""

    def __init__(self, modality="RGB", hw=(256, 340)):
        self.modality, self.hw = modality, hw

    def __call__(self, video_id, indices):
        rs = np.random.RandomState((hash(str(video_id)) % 100003) * 31 + int(indices[0]))
        per, c = (1, 3) if self.modality in ("RGB", "RGBDiff") else (2, 1)
        return rs.randint(0, 256, (len(indices) * per,) + tuple(self.hw) + (c,)).astype(np.uint8)


def ssn_batches(sampler, reader, videos_per_batch, order=None, drop_last=True):
    """One pass over ``sampler`` (a ``ProposalSampler``): per video its 8 proposals x 9 snippets, decoded by ``reader``."""
    order = range(len(sampler)) if order is None else order
    group = []
    for index in order:
        props, arr = sampler.sample_video(index)
        frames = np.concatenate([reader(p.video_id, p.frame_indices) for p in props])
        group.append((frames, arr["scaling"], arr["labels"].astype(np.int64), arr["reg_targets"], arr["prop_type"].astype(np.int64)))
        if len(group) == videos_per_batch:
            yield tuple(np.stack(x) for x in zip(*group))
            group = []
    if group and not drop_last:
        yield tuple(np.stack(x) for x in zip(*group))


def binary_batches(sampler, reader, videos_per_batch=4, order=None, drop_last=True):
    """One pass over ``sampler`` (an ``ActionnessSampler``): per video its foreground and background proposals x body_seg snippets."""
    order = range(len(sampler)) if order is None else order
    group = []
    for index in order:
        props, arr = sampler.sample_video(index)
        frames = np.concatenate([reader(p.video_id, p.frame_indices) for p in props])
        n = len(props)
        group.append((frames, np.zeros((n, 2), np.float32), np.zeros(n, np.int64), np.zeros((n, 2), np.float32),
                      arr["prop_type"].astype(np.int64)))
        if len(group) == videos_per_batch:
            yield tuple(np.stack(x) for x in zip(*group))
            group = []
    if group and not drop_last:
        yield tuple(np.stack(x) for x in zip(*group))


def _file_batches(rows, videos_per_batch, drop_last):
    group = []
    for row in rows:
        group.append(row)
        if len(group) == videos_per_batch:
            yield (tuple(g[0] for g in group),) + tuple(np.stack(x) for x in list(zip(*group))[1:])
            group = []
    if group and not drop_last:
        yield (tuple(g[0] for g in group),) + tuple(np.stack(x) for x in list(zip(*group))[1:])


def compressed_ssn_batches(sampler, reader, videos_per_batch, order=None, drop_last=True):
    """``ssn_batches`` with a ``CompressedFrameDirReader``: the first field is, per video, the list of its files' bytes."""
    def rows():
        for index in (range(len(sampler)) if order is None else order):
            props, arr = sampler.sample_video(index)
            files = [b for p in props for b in reader(p.video_id, p.frame_indices)]
            yield files, arr["scaling"], arr["labels"].astype(np.int64), arr["reg_targets"], arr["prop_type"].astype(np.int64)
    return _file_batches(rows(), videos_per_batch, drop_last)


def compressed_binary_batches(sampler, reader, videos_per_batch=4, order=None, drop_last=True):
    """``binary_batches`` with a ``CompressedFrameDirReader``."""
    def rows():
        for index in (range(len(sampler)) if order is None else order):
            props, arr = sampler.sample_video(index)
            files = [b for p in props for b in reader(p.video_id, p.frame_indices)]
            n = len(props)
            yield (files, np.zeros((n, 2), np.float32), np.zeros(n, np.int64), np.zeros((n, 2), np.float32),
                   arr["prop_type"].astype(np.int64))
    return _file_batches(rows(), videos_per_batch, drop_last)


def synthetic_ssn_source(n_batches, videos_per_batch, num_class, modality="RGB", new_length=1, hw=(256, 340), seed=0,
                         prop_per_video=8, num_segments=9):
    """``n_batches`` seeded batches in the sampler's layout (foreground, 6 incomplete, background per video), no data set needed."""
    per, c = (1, 3) if modality in ("RGB", "RGBDiff") else (2, 1)
    v, p = videos_per_batch, prop_per_video
    for b in range(n_batches):
        rs = np.random.RandomState(seed * 7919 + b)
        frames = rs.randint(0, 256, (v, p * num_segments * new_length * per) + tuple(hw) + (c,)).astype(np.uint8)
        scaling = rs.uniform(0, 1, (v, p, 2)).astype(np.float32)
        target = rs.randint(1, num_class + 1, (v, p)).astype(np.int64)
        target[:, -1] = 0
        reg = np.zeros((v, p, 2), np.float32)
        reg[:, 0] = rs.standard_normal((v, 2)).astype(np.float32)
        prop_type = np.array([[0] + [1] * (p - 2) + [2]] * v, np.int64)
        yield frames, scaling, target, reg, prop_type


def synthetic_binary_source(n_batches, videos_per_batch, modality="RGB", new_length=1, hw=(256, 340), seed=0, fg=3, bg=9, body_seg=5):
    per, c = (1, 3) if modality in ("RGB", "RGBDiff") else (2, 1)
    v, p = videos_per_batch, fg + bg
    for b in range(n_batches):
        rs = np.random.RandomState(seed * 7919 + b)
        frames = rs.randint(0, 256, (v, p * body_seg * new_length * per) + tuple(hw) + (c,)).astype(np.uint8)
        prop_type = np.array([[1] * fg + [0] * bg] * v, np.int64)
        yield frames, np.zeros((v, p, 2), np.float32), np.zeros((v, p), np.int64), np.zeros((v, p, 2), np.float32), prop_type


def binary_view(batches):
    """Prefetcher output -> the ``(frames, prop_type)`` pairs of the binary loop."""
    for b in batches:
        yield b[0], b[4]


def closing(prefetcher):
    """Iterate a ``TrainingBatchPrefetcher`` and stop its thread afterwards."""
    try:
        for b in prefetcher:
            yield b
    finally:
        prefetcher.close()


class Counted(object):
    """An iterable with the length the loop prints (``len(train_loader)``)."""

    def __init__(self, iterable, n):
        self.iterable, self.n = iterable, int(n)

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(self.iterable)


class CenterCropAugment(GpuTrainAugment):
    """The validation transform: the centre box that ``GroupScale(scale_size)`` -> ``GroupCenterCrop(crop)`` keeps, resized to the
    crop size in the same launch.  Identical to the reference when the decoded short side equals ``scale_size`` (340 x 256
    frames, the size its extraction scripts write); otherwise the resize runs after the crop instead of before it."""

    def __init__(self, *a, scale_size=256, **kw):
        super().__init__(*a, **kw)
        self.scale_size = scale_size

    def sample(self, frame_wh, n_groups):
        w, h = frame_wh
        side = min(w, h) * self.crop_w // self.scale_size
        box = ((w - side) // 2, (h - side) // 2, side, side)
        return [box] * n_groups, [False] * n_groups


def make_transforms(model, device):
    """(training, validation) device transforms of a model: ``get_augmentation()`` + Stack / ToTorchFormatTensor / GroupNormalize
    (ssn_train.py:106-111), and GroupScale(scale_size) + GroupCenterCrop(crop_size) (ssn_train.py:123-129)."""
    flow = model.modality == "Flow"
    scales = [1, .875, .75] if flow else [1, .875, .75, .66]
    kw = dict(roll=True, is_flow=flow, device=device)
    train = GpuTrainAugment(model.input_size, model.input_mean, model.input_std, scales, **kw)
    val = CenterCropAugment(model.input_size, model.input_mean, model.input_std, [1], scale_size=model.scale_size, **kw)
    return train, val
