"""Baseline JPEG decoding on the device (csrc/jpeg.hip, jpeg_decode.py) against PIL, bit for bit.

The criterion everywhere is equality with ``np.asarray(Image.open(f).convert(mode))``.  tests/jpeg_referee.py, a plain numpy
decoder that shares no code with the product, is first held against PIL on every file (``test_referee_equals_pil``) and then
referees the stages: coefficients after the entropy stage, component planes after the inverse DCT.  Files are made at test time
with ``PIL.Image.save`` from seeded arrays.  The shapes are the smallest at which each mechanism can fail: 8 x 8 gray is one
block, 16 x 16 4:2:0 one MCU, 17 x 33 and 31 x 15 have ragged right and bottom MCUs and odd chroma extents, 37 x 53 and 64 x 80
more than one MCU row and column.

Coverage condition: over every well-formed input here ``decoder.fallbacks == 0`` and every status word is 0 -- the kernels decoded
them, PIL did not.
"""
import functools
import importlib.util
import io
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import action_detection_amd  # noqa: F401
import jpeg_referee as R
from action_detection_amd import kernels as K
from action_detection_amd.jpeg_decode import CompressedBatchPrefetcher, JpegDecoder, parse_jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 8), (16, 16), (17, 33), (31, 15), (37, 53), (64, 80)]
SAMPLINGS = [None, 0, 1, 2]          # gray, 4:4:4, 4:2:2, 4:2:0
QUALITIES = [50, 75, 95, 100]


def picture(h, w, sampling, kind="smooth", seed=0):
    rs = np.random.RandomState(seed * 7 + h * 131 + w)
    c = 1 if sampling is None else 3
    if kind == "noise":
        a = rs.randint(0, 256, (h, w, c))
    elif kind == "flat":
        a = np.full((h, w, c), 77) + np.arange(c) * 40
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([128 + 100 * np.sin(xx / 7.0 + k) * np.cos(yy / 5.0 - k) for k in range(c)], 2) + rs.randint(-20, 20, (h, w, c))
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a[:, :, 0] if c == 1 else a


@functools.lru_cache(maxsize=None)
def jpeg(h, w, sampling, quality, kind="smooth", **extra):
    b = io.BytesIO()
    kw = dict(quality=quality, **extra)
    if sampling is not None:
        kw["subsampling"] = sampling
    Image.fromarray(picture(h, w, sampling, kind, quality)).save(b, "JPEG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def pil(data, mode):
    """The yardstick, computed once per (file, mode) and shared."""
    a = np.asarray(Image.open(io.BytesIO(data)).convert(mode))
    a = a if a.ndim == 3 else a[:, :, None]
    a.setflags(write=False)
    return a


def grid(shape):
    return [jpeg(shape[0], shape[1], s, q) for s in SAMPLINGS for q in QUALITIES]


def special_cases():
    """Restart markers, optimised (non-standard) Huffman tables, uniform noise at quality 100, flat pictures."""
    out = []
    for (h, w) in [(17, 33), (37, 53), (64, 80)]:
        for s in SAMPLINGS:
            out.append(jpeg(h, w, s, 75, restart_marker_blocks=3))
            out.append(jpeg(h, w, s, 95, optimize=True))
            out.append(jpeg(h, w, s, 100, "noise"))
            out.append(jpeg(h, w, s, 75, "flat"))
    return out


def all_files():
    return [f for shape in SHAPES for f in grid(shape)] + special_cases()


def assert_equal_pil(decoder, files, mode, outputs):
    assert decoder.fallbacks == 0, "PIL decoded %d of these files, not the kernels" % decoder.fallbacks
    assert not decoder.status.cpu().any(), "status words %r" % decoder.status.cpu().tolist()
    assert len(outputs) == len(files)
    for i, (f, o) in enumerate(zip(files, outputs)):
        want = pil(f, mode)
        assert tuple(o.shape) == want.shape and o.dtype == torch.uint8
        assert np.array_equal(o.cpu().numpy(), want), "file %d (%d x %d), mode %s" % (i, want.shape[1], want.shape[0], mode)


# ------------------------------------------------------------------------------------------------------------------ the referee
def test_referee_equals_pil():
    files = all_files()
    assert len(files) == 6 * 16 + 3 * 16
    for f in files:
        for mode in ("RGB", "L"):
            got = R.decode(f, mode)
            assert np.array_equal(got if got.ndim == 3 else got[:, :, None], pil(f, mode))


def test_special_cases_are_what_they_claim():
    f = jpeg(37, 53, 2, 75, restart_marker_blocks=3)
    assert b"\xff\xdd\x00\x04\x00\x03" in f and b"\xff\xd0" in f and b"\xff\xd1" in f        # a DRI segment and restart markers
    h = parse_jpeg(f)
    assert h.supported and h.restart_interval == 3 and len(h.units) == -(-(3 * 4) // 3) and h.units[1][2] == 3
    std, opt = parse_jpeg(jpeg(37, 53, 2, 95)), parse_jpeg(jpeg(37, 53, 2, 95, optimize=True))
    assert std.huffman != opt.huffman                                                          # non-standard tables
    noise = parse_jpeg(jpeg(64, 80, 0, 100, "noise"))
    assert max(i + 1 for i, c in enumerate(noise.huffman[(1, 0)][0]) if c) == 16             # codes of 16 bits: the overflow path
    assert jpeg(64, 80, 0, 100, "noise").count(b"\xff\x00") > 20                               # dense stuffing
    flat = R.entropy(jpeg(37, 53, 2, 75, "flat"), R.parse(jpeg(37, 53, 2, 75, "flat")))
    assert all(not c[..., 1:].any() for c in flat)                                             # DC-only blocks


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_every_sampling_and_quality(backend, shape):
    files = grid(shape)
    for mode in ("RGB", "L"):
        dec = JpegDecoder(backend.device)
        assert_equal_pil(dec, files, mode, dec.decode(files, mode))


def test_restart_optimised_noise_flat(backend):
    files = special_cases()
    for mode in ("RGB", "L"):
        dec = JpegDecoder(backend.device)
        assert_equal_pil(dec, files, mode, dec.decode(files, mode))


def test_one_batch_mixing_everything(backend):
    """Different sizes, samplings and table sets in one launch: lanes of one wave own different files, the units fill more than
    one workgroup and the optimised files bring more table sets than a workgroup holds."""
    files = all_files()
    random.Random(5).shuffle(files)
    dec = JpegDecoder(backend.device)
    headers = [parse_jpeg(f) for f in files]
    assert sum(len(h.units) for h in headers) > 128
    assert len({tuple(sorted(h.huffman.items())) for h in headers}) > dec.lds_sets
    for mode in ("RGB", "L"):
        assert_equal_pil(dec, files, mode, dec.decode(files, mode))


def test_stack(backend):
    files = [jpeg(37, 53, s, 75) for s in SAMPLINGS] + [jpeg(37, 53, 2, 75, restart_marker_blocks=3)]
    dec = JpegDecoder(backend.device)
    for mode, c in (("RGB", 3), ("L", 1)):
        out = dec.decode(files, mode, stack=True)
        assert out.shape == (5, 37, 53, c) and out.is_contiguous()
        assert_equal_pil(dec, files, mode, list(out))
    with pytest.raises(ValueError, match="one size"):
        dec.decode(files + [jpeg(31, 15, 2, 75)], "RGB", stack=True)
    with pytest.raises(ValueError):
        dec.decode(files, "CMYK")


def test_stage_by_stage(backend):
    """Coefficients after the entropy stage equal the referee's; the pixel kernels fed the REFEREE's coefficients equal the
    referee's planes and pixels -- a wrong pixel can be placed in a stage."""
    files = [jpeg(17, 33, None, 95), jpeg(31, 15, 0, 50), jpeg(37, 53, 1, 100, "noise"), jpeg(37, 53, 2, 75, restart_marker_blocks=3),
             jpeg(64, 80, 2, 95, optimize=True), jpeg(16, 16, 2, 75)]
    dec = JpegDecoder(backend.device)
    dec.decode(files, "RGB")
    desc, coef, planes, quant, sz = dec._stages
    rows, ref_coef, ref_planes = desc.cpu().numpy(), [], []
    for f in files:
        h = R.parse(f)
        c = R.entropy(f, h)
        ref_coef.append(np.concatenate([x.reshape(-1, 64) for x in c]))
        ref_planes.append(np.concatenate([x.reshape(-1) for x in R.idct_planes(h, c)]))
    for i in range(len(files)):
        off, n, poff = rows[i, 7], rows[i, 8], rows[i, 9]
        assert n == len(ref_coef[i])
        assert np.array_equal(coef[off:off + n].cpu().numpy(), ref_coef[i]), "coefficients of file %d" % i
        assert np.array_equal(planes[poff:poff + 64 * n].cpu().numpy(), ref_planes[i]), "planes of file %d" % i
    fed = backend.put(torch.from_numpy(np.concatenate(ref_coef)))
    planes2 = backend.put(torch.zeros(planes.numel(), dtype=torch.uint8))
    K.jpeg_idct(fed, desc, sz["max_blocks"], quant, planes2)
    assert np.array_equal(planes2.cpu().numpy(), np.concatenate(ref_planes))
    for mode, c in (("RGB", 3), ("L", 1)):
        total = sum(pil(f, mode).size for f in files)
        out = backend.put(torch.zeros(total, dtype=torch.uint8))
        d2 = desc.clone()
        offs = np.cumsum([0] + [pil(f, mode).size for f in files])
        d2[:, 10] = backend.put(torch.from_numpy(offs[:-1].astype(np.int32)))
        K.jpeg_pixels(backend.put(torch.from_numpy(np.concatenate(ref_planes))), d2, sz["max_pixels"], c, out)
        got = out.cpu().numpy()
        for i, f in enumerate(files):
            assert np.array_equal(got[offs[i]:offs[i + 1]].reshape(pil(f, mode).shape), pil(f, mode))


def test_wrappers_validate_before_any_launch(backend):
    dec = JpegDecoder(backend.device)
    dec.decode([jpeg(16, 16, 2, 75)], "RGB")
    desc, coef, planes, quant, sz = dec._stages
    with pytest.raises(ValueError):
        K.jpeg_idct(coef.to(torch.int32), desc, 6, quant, planes)
    with pytest.raises(ValueError):
        K.jpeg_idct(coef, desc[:, :5].contiguous(), 6, quant, planes)
    with pytest.raises(ValueError):
        K.jpeg_pixels(planes, desc, 256, 2, torch.zeros(768, dtype=torch.uint8, device=planes.device))
    with pytest.raises(ValueError):
        K.jpeg_entropy(planes, desc, desc, quant, coef, dec.status)


# ------------------------------------------------------------------------------------------------- damaged files: emulator only
GUARD = 4096


def guarded(dec):
    """Make the decoder allocate its coefficient, plane and output buffers inside sentinel bands."""
    bands = []

    def alloc(shape, dtype):
        n = int(np.prod(shape))
        big = torch.full((n + 2 * GUARD,), 0x5A, dtype=dtype)
        bands.append((big, n))
        return big[GUARD:GUARD + n].view(shape)
    dec._alloc = alloc
    return bands


def test_damaged_files_stay_inside_their_buffers(emu):
    good = [jpeg(37, 53, 2, 75), jpeg(64, 80, 0, 95), jpeg(31, 15, None, 75), jpeg(37, 53, 1, 75, restart_marker_blocks=3)]
    victim = jpeg(64, 80, 2, 95)
    b, e = parse_jpeg(victim).scan
    cut = victim[:(b + e) // 2]                                                       # ends in the middle of its scan
    mid = (b + e) // 2
    bad_code = victim[:mid] + b"\xff\x00" * 16 + victim[mid + 32:]                     # 128 one-bits: no table assigns that code
    victim_r = jpeg(64, 80, 1, 75, restart_marker_blocks=3)
    b, e = parse_jpeg(victim_r).scan
    cut_r = victim_r[:(b + e) // 2]
    files = [good[0], cut, good[1], bad_code, good[2], cut_r, good[3]]
    assert all(parse_jpeg(f).supported for f in files)
    dec = JpegDecoder("cpu")
    bands = guarded(dec)
    out = dec.decode(files, "RGB")
    assert len(bands) == 3
    for big, n in bands:
        assert (big[:GUARD] == 0x5A).all() and (big[GUARD + n:] == 0x5A).all(), "a guard band was written"
    status = dec.status.tolist()
    assert status[1] & 1 and status[3] & 2 and status[5] & 1 and [status[i] for i in (0, 2, 4, 6)] == [0, 0, 0, 0]
    for i, g in zip((0, 2, 4, 6), good):
        assert np.array_equal(out[i].numpy(), pil(g, "RGB"))
    assert dec.fallbacks == 0
    # check(): the one host read; the damaged files go to PIL, which decodes the bad code with a warning and refuses the cut files
    dec2 = JpegDecoder("cpu")
    out = dec2.decode([good[0], bad_code, good[1]], "RGB")
    assert dec2.check() == [1] and dec2.fallbacks == 1
    assert np.array_equal(out[1].numpy(), pil(bad_code, "RGB")) and np.array_equal(out[2].numpy(), pil(good[1], "RGB"))
    dec3 = JpegDecoder("cpu")
    dec3.decode([good[0], cut], "RGB")
    with pytest.raises(OSError) as pil_says:
        pil(cut, "RGB")
    with pytest.raises(OSError, match=str(pil_says.value)[:20]):
        dec3.check()


def test_parse_never_reads_past_the_file(emu):
    """The marker walk is Python: its bounds are checked by running it over every prefix of a file and over seeded mutations of
    its header -- it answers, it does not raise -- and whatever it calls supported decodes inside guard bands."""
    f = jpeg(37, 53, 2, 75, restart_marker_blocks=3)
    for n in range(len(f)):
        h = parse_jpeg(f[:n])
        assert h.supported or h.reason
    rs = np.random.RandomState(9)
    scan = parse_jpeg(f).scan[0]
    accepted = []
    for _ in range(400):
        m = bytearray(f)
        for _ in range(rs.randint(1, 4)):
            m[rs.randint(2, scan)] = rs.randint(0, 256)
        h = parse_jpeg(bytes(m))
        assert h.supported or h.reason
        if h.supported and h.width * h.height <= 1 << 16:
            accepted.append(bytes(m))
    assert len(accepted) > 20
    dec = JpegDecoder("cpu")
    bands = guarded(dec)
    dec.decode(accepted[:64], "RGB")
    for big, n in bands:
        assert (big[:GUARD] == 0x5A).all() and (big[GUARD + n:] == 0x5A).all()


def test_unsupported_files_go_to_pil(emu):
    rgb = picture(37, 53, 0)
    files, reasons = [], []

    def add(img, reason, **kw):
        b = io.BytesIO()
        try:
            img.save(b, "JPEG", **kw)
        except Exception:
            return                      # (this PIL does not write such a file: the case is omitted)
        files.append(b.getvalue())
        reasons.append(reason)
    add(Image.fromarray(rgb), "progressive", quality=75, progressive=True)
    add(Image.fromarray(rgb).convert("CMYK"), "CMYK", quality=75)
    add(Image.fromarray(rgb), "sampling", quality=75, subsampling=(4, 1, 1, 1, 1, 1))
    assert reasons[:2] == ["progressive", "CMYK"]
    for f, r in zip(files, reasons):
        h = parse_jpeg(f)
        assert not h.supported and r in h.reason, (r, h.reason)
    assert not parse_jpeg(b"GIF89a" + bytes(40)).supported
    batch = files + [jpeg(37, 53, 2, 75)]
    for mode in ("RGB", "L"):
        dec = JpegDecoder("cpu")
        out = dec.decode(batch, mode)
        assert dec.fallbacks == len(files) and not dec.status.any()
        for f, o in zip(batch, out):
            assert np.array_equal(o.numpy(), pil(f, mode))
    dec = JpegDecoder("cpu")
    out = dec.decode(files[:1], "RGB", stack=True)                                     # a batch with nothing for the kernels
    assert dec.fallbacks == 1 and np.array_equal(out[0].numpy(), pil(files[0], "RGB"))
    with pytest.raises(Exception) as pil_says:
        Image.open(io.BytesIO(b"GIF89a" + bytes(40))).convert("RGB")
    with pytest.raises(type(pil_says.value)):
        dec.decode([b"GIF89a" + bytes(40)], "RGB")


# ------------------------------------------------------------------------------------------------------------------ the pipeline
class Proposal(object):
    def __init__(self, video_id, frame_indices):
        self.video_id, self.frame_indices = video_id, frame_indices


class Sampler(object):
    """Two proposals of three snippets per video, fixed."""

    def __init__(self, videos):
        self.videos = videos

    def __len__(self):
        return len(self.videos)

    def sample_video(self, index):
        rs = np.random.RandomState(index)
        props = [Proposal(self.videos[index], [1, 3, 4]), Proposal(self.videos[index], [2, 2, 5])]
        return props, dict(scaling=rs.rand(2, 2).astype(np.float32), labels=np.array([1, 0]), reg_targets=rs.randn(2, 2).astype(np.float32),
                           prop_type=np.array([0, 2]))


@pytest.mark.parametrize("modality", ["RGB", "Flow"])
def test_compressed_pipeline_equals_the_decoded_one(backend, modality, tmp_path):
    from action_detection_amd import train_data as D
    from action_detection_amd.input_pipeline import GpuTrainAugment, TrainingBatchPrefetcher
    videos = ["video_a", "video_b", "video_c", "video_d"]
    for v, name in enumerate(videos):
        os.makedirs(str(tmp_path / name))
        for i in range(1, 6):
            if modality == "RGB":
                Image.fromarray(picture(40, 52, 2, seed=10 * v + i)).save(str(tmp_path / name / ("img_%05d.jpg" % i)), quality=75)
            else:
                for k, axis in enumerate("xy"):
                    Image.fromarray(picture(40, 52, None, seed=100 * v + 2 * i + k)).save(
                        str(tmp_path / name / ("flow_%s_%05d.jpg" % (axis, i))), quality=95)
    flow = modality == "Flow"
    aug = GpuTrainAugment(32, [128] if flow else [104, 117, 128], [1], [1, .875, .75], roll=True, is_flow=flow, device=backend.device)
    group = 3 * (2 if flow else 1)
    sampler = Sampler(videos)
    random.seed(21)
    want = list(TrainingBatchPrefetcher(D.ssn_batches(sampler, D.FrameDirReader(str(tmp_path), modality, "flow_"), 2), aug,
                                        group_size=group))
    random.seed(21)
    pre = CompressedBatchPrefetcher(D.compressed_ssn_batches(sampler, D.CompressedFrameDirReader(str(tmp_path), modality, "flow_"), 2),
                                    aug, group_size=group)
    got = list(pre)
    assert len(got) == len(want) == 2 and pre.decoder.fallbacks == 0 and not pre.decoder.status.cpu().any()
    for g, w in zip(got, want):
        assert g[0].shape == (2, 2 * group * (1 if flow else 3), 32, 32)
        for a, b in zip(g, w):
            assert a.device == b.device and torch.equal(a.cpu(), b.cpu())
    binary = list(D.compressed_binary_batches(sampler, D.CompressedFrameDirReader(str(tmp_path), modality, "flow_"), 4))
    plain = list(D.binary_batches(sampler, D.FrameDirReader(str(tmp_path), modality, "flow_"), 4))
    assert len(binary) == len(plain) == 1 and len(binary[0][0]) == 4 and len(binary[0][0][0]) == plain[0][0].shape[1]
    assert all(np.array_equal(a, b) for a, b in zip(binary[0][1:], plain[0][1:]))


def test_extract_flow_with_gpu_decode_writes_the_same_files(backend, tmp_path):
    from action_detection_amd import _lib
    if backend.is_gpu:
        assert not _lib.emulator_active()
    src = tmp_path / "frames"
    os.makedirs(str(src / "video_a"))
    for t in range(3):
        Image.fromarray(np.roll(picture(32, 40, 2, seed=3), 2 * t, axis=1)).save(str(src / "video_a" / ("img_%05d.jpg" % (t + 1))), quality=90)
    spec = importlib.util.spec_from_file_location("extract_flow_tool", os.path.join(ROOT, "tools", "extract_flow.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    common = ["--bound", "20", "--flow-prefix", "flow_", "--iterations", "20", "--quiet"]
    assert tool.main([str(src), str(tmp_path / "host")] + common) == 0
    assert tool.main([str(src), str(tmp_path / "device"), "--gpu-decode"] + common) == 0
    names = sorted(os.listdir(str(tmp_path / "host" / "video_a")))
    assert len(names) == 4 and names == sorted(os.listdir(str(tmp_path / "device" / "video_a")))
    for name in names:
        with open(str(tmp_path / "host" / "video_a" / name), "rb") as a, open(str(tmp_path / "device" / "video_a" / name), "rb") as b:
            assert a.read() == b.read(), name


def test_extract_actionness_device_transform_equals_the_host_chain(backend):
    """tools/extract_actionness.py --gpu-decode: files -> the ten crops, equal to PIL + the host transform chain."""
    from action_detection_amd import transforms as T
    spec = importlib.util.spec_from_file_location("extract_actionness_tool", os.path.join(ROOT, "tools", "extract_actionness.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    class Net(object):
        input_size, scale_size, input_mean, input_std = 24, 32, [104, 117, 128], [1]
    files = [jpeg(32, 43, 2, 75), jpeg(32, 43, 0, 95)]
    got = tool.device_transform(Net, "RGB", backend.device)(files)
    host = T.Compose([T.GroupOverSample(24, 32), T.Stack(roll=True), T.ToTorchFormatTensor(div=False), T.GroupNormalize([104, 117, 128], [1])])
    want = host([Image.open(io.BytesIO(f)).convert("RGB") for f in files])
    assert torch.equal(got.cpu(), want)
    with pytest.raises(ValueError, match="short side"):
        tool.device_transform(Net, "RGB", backend.device)([jpeg(37, 53, 2, 75)])
