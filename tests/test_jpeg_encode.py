"""Baseline JPEG encoding on the device (csrc/jpeg_encode.hip, jpeg_encode.py) against PIL, byte for byte.

The criterion everywhere is ``bytes == PIL's bytes``: PIL's file is made at test time with ``Image.fromarray(a).save(buf, "JPEG",
quality=, subsampling=, restart_marker_blocks=)`` from seeded arrays.  tests/jpeg_encode_referee.py, a plain numpy encoder that shares
no code with the product, is first held against PIL on every file (``test_referee_equals_pil``) and then referees the stages:
coefficients after the first stage, scan bytes after pack + assemble.  Shapes (height x width) are the smallest at which each
mechanism can fail: 1 x 1; 8 x 8 one block (at 4:2:0 one real luma block and three dummies); 16 x 16 one 4:2:0 MCU; 17 x 33 and
31 x 15 ragged right and bottom with odd chroma extents; 40 x 9 an even height that is no multiple of 16 under an MCU wider than the
image; 37 x 53 and 64 x 80 several MCU rows and columns (64 x 80 4:4:4 has 240 blocks a component: the scans cross a 256-thread chunk).
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
import jpeg_encode_referee as R
from action_detection_amd import kernels as K
from action_detection_amd.jpeg_decode import JpegDecoder
from action_detection_amd.jpeg_encode import JpegEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 33), (31, 15), (40, 9), (37, 53), (64, 80)]
LARGE = [(37, 53), (64, 80)]
SAMPLINGS = [None, 0, 1, 2]          # gray, 4:4:4, 4:2:2, 4:2:0
QUALITIES = [10, 50, 75, 95, 100]
RESTARTS = [1, 3, 8]


@functools.lru_cache(maxsize=None)
def picture(h, w, sampling, kind="smooth", seed=0):
    rs = np.random.RandomState(seed * 7 + h * 131 + w)
    c = 1 if sampling is None else 3
    if kind == "noise":
        a = rs.randint(0, 256, (h, w, c))
    elif kind == "binary":
        a = rs.randint(0, 2, (h, w, c)) * 255
    elif kind == "flat":
        a = np.full((h, w, c), 77) + np.arange(c) * 40
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([128 + 100 * np.sin(xx / 7.0 + k) * np.cos(yy / 5.0 - k) for k in range(c)], 2) + rs.randint(-20, 20, (h, w, c))
    a = np.clip(a, 0, 255).astype(np.uint8)
    a = a[:, :, 0] if c == 1 else a
    a.setflags(write=False)
    return a


def case_picture(case):
    h, w, sampling, quality, kind = case
    return picture(h, w, sampling, kind, quality)


@functools.lru_cache(maxsize=None)
def pil_bytes(case, restart=0, default_sampling=False):
    """The yardstick, made once per case and shared."""
    h, w, sampling, quality, kind = case
    kw = dict(quality=quality)
    if sampling is not None and not default_sampling:
        kw["subsampling"] = sampling
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    Image.fromarray(case_picture(case)).save(b, "JPEG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def grid():
    cases = [(h, w, s, q, "smooth") for (h, w) in SHAPES for s in SAMPLINGS for q in QUALITIES]
    cases += [(h, w, s, q, kind) for (h, w) in LARGE for kind in ("noise", "flat", "binary") for s in SAMPLINGS for q in QUALITIES]
    return tuple(cases)


def restart_cases():
    return [((h, w, s, 75, "smooth"), r) for (h, w) in LARGE for s in SAMPLINGS for r in RESTARTS]


def encode_cases(backend, cases, restart=0, encoder=None):
    """One ``encode`` call (a list of images of different sizes) per sampling and quality -> {case: bytes}."""
    enc = encoder or JpegEncoder(backend.device)
    out = {}
    for key in sorted({(c[2], c[3]) for c in cases}, key=str):
        group = [c for c in cases if (c[2], c[3]) == key]
        files = enc.encode([backend.put(torch.from_numpy(case_picture(c).copy())) for c in group], quality=key[1], subsampling=key[0],
                           restart_blocks=restart)
        out.update(zip(group, files))
    return out


def first_difference(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


# ---------------------------------------------------------------------------------------------------------------- 1. the referee
def test_referee_equals_pil():
    for case in grid():
        h, w, s, q, _ = case
        assert R.encode(case_picture(case), q, s) == pil_bytes(case), case
    for case, r in restart_cases():
        assert R.encode(case_picture(case), case[3], case[2], restart=r) == pil_bytes(case, r), (case, r)


# ---------------------------------------------------------------------------------------------------------------- 2. the grid
def test_grid_equals_pil(backend):
    got = encode_cases(backend, grid())
    assert len(got) == len(grid()) == 280
    for case in grid():
        want = pil_bytes(case)
        assert got[case] == want, (case, len(got[case]), len(want), first_difference(got[case], want))


def test_default_subsampling_of_rgb_is_pils(backend):
    case = (37, 53, 2, 75, "smooth")
    want = pil_bytes(case, default_sampling=True)
    assert want == pil_bytes(case)          # (PIL's default for RGB is 4:2:0)
    got = JpegEncoder(backend.device).encode([backend.put(torch.from_numpy(case_picture(case).copy()))], quality=75)
    assert got == [want]


# ---------------------------------------------------------------------------------------------------------------- 3. the cases
def scan_of(data):
    begin = data.index(b"\xff\xda")
    begin += 2 + ((data[begin + 2] << 8) | data[begin + 3])
    return data[begin:-2]


def test_the_cases_are_what_they_claim():
    """On PIL's bytes and the referee's symbols, never on the product."""
    noisy = (64, 80, None, 100, "binary")
    assert scan_of(pil_bytes(noisy)).count(b"\xff\x00") >= 10
    sym = R.symbols_of(case_picture((64, 80, 0, 10, "noise")), 10, 0)
    assert any(cls == 1 and symbol == 0xF0 for (cls, symbol, _) in sym), "no ZRL symbol"
    assert any(length == 16 for s in (R.symbols_of(case_picture(c), c[3], c[2]) for c in [(64, 80, None, 100, "noise"), noisy])
               for (_, _, length) in s), "no 16-bit code"
    flat = (64, 80, None, 75, "flat")
    coef = R.coefficients(case_picture(flat), 75, None)[0]
    assert not coef[:, 1:].any() and coef[:, 0].any(), "flat picture: DC-only blocks"
    for (h, w) in [(8, 8), (40, 9)]:
        a = case_picture((h, w, 2, 75, "smooth"))
        coef, mcux, mcuy, ncomp, hs, vs = R.coefficients(a, 75, 2)
        real = (-(-w // 8)) * (-(-h // 8)) + 2 * mcux * mcuy
        assert len(coef) == 6 * mcux * mcuy > real, "no dummy blocks at %d x %d" % (h, w)
    many = pil_bytes((64, 80, 0, 75, "smooth"), 1)
    markers = [many[i + 1] for i in range(len(many) - 1) if many[i] == 0xFF and 0xD0 <= many[i + 1] <= 0xD7]
    assert len(markers) > 8 and markers[8] == 0xD0 and markers[7] == 0xD7, "RSTn does not wrap"


# ---------------------------------------------------------------------------------------------------------------- 4. restarts
def test_restart_intervals_equal_pil(backend):
    for r in RESTARTS:
        cases = [c for c, rr in restart_cases() if rr == r]
        got = encode_cases(backend, cases, restart=r)
        for case in cases:
            want = pil_bytes(case, r)
            assert got[case] == want, (case, r, len(got[case]), len(want), first_difference(got[case], want))


# ---------------------------------------------------------------------------------------------------------------- 5. mixed batch
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_mixed_batch_equals_single_images(backend, sampling):
    enc = JpegEncoder(backend.device)
    cases = [(h, w, sampling, 75, "smooth") for (h, w) in SHAPES]
    random.Random(5).shuffle(cases)
    images = [backend.put(torch.from_numpy(case_picture(c).copy())) for c in cases]
    together = enc.encode(images, quality=75, subsampling=sampling)
    for case, image, got in zip(cases, images, together):
        assert got == pil_bytes(case), case
        assert enc.encode([image], quality=75, subsampling=sampling) == [got], case
    same = [images[cases.index((64, 80, sampling, 75, "smooth"))]] * 3
    assert enc.encode(torch.stack(same), quality=75, subsampling=sampling) == enc.encode(same, quality=75, subsampling=sampling)
    if sampling is None:
        assert enc.encode(torch.stack(same).unsqueeze(-1), quality=75) == enc.encode(same, quality=75)


# ---------------------------------------------------------------------------------------------------------------- 6. stages
STAGE_CASES = [(8, 8, 2, 75, "smooth"), (40, 9, 2, 95, "smooth"), (31, 15, 1, 50, "smooth"), (37, 53, 2, 100, "noise"),
               (64, 80, 0, 95, "smooth"), (17, 33, None, 10, "smooth"), (64, 80, None, 100, "binary")]


def test_first_stage_coefficients_equal_the_referees(backend):
    for case in STAGE_CASES:
        enc = JpegEncoder(backend.device)
        enc.encode([backend.put(torch.from_numpy(case_picture(case).copy()))], quality=case[3], subsampling=case[2])
        want = R.coefficients(case_picture(case), case[3], case[2])[0]
        got = enc._stages["coef"].cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (case, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("restart", [0, 3])
def test_pack_and_assemble_code_the_referees_coefficients(backend, restart):
    """The stages behind the first, fed the REFEREE's coefficients, give the referee's scan: a wrong byte is then in one of them."""
    for case in STAGE_CASES:
        a = case_picture(case)
        want_coef, mcux, mcuy, ncomp, hs, vs = R.coefficients(a, case[3], case[2])
        want_scan, _ = R.scan(want_coef, ncomp, hs, vs, restart)
        enc = JpegEncoder(backend.device)
        staging, offs, sz = enc._plan([a.shape[:2]], ncomp, hs, vs, case[3], restart, None)
        flat = backend.put(torch.zeros(a.size, dtype=torch.uint8))      # (the pixels are not looked at)
        files = enc._run(flat, staging, offs, sz, 1, True, coef=backend.put(torch.from_numpy(want_coef.copy())))
        assert scan_of(files[0]) == want_scan, (case, restart)
        assert files[0] == pil_bytes(case, restart), (case, restart)


# ---------------------------------------------------------------------------------------------------------------- 7. round trip
def test_round_trip_through_the_device_decoder(backend):
    for sampling in SAMPLINGS:
        cases = [(h, w, sampling, 75, "smooth") for (h, w) in LARGE + [(17, 33)]]
        files = [encode_cases(backend, [c], restart=3)[c] for c in cases]
        dec = JpegDecoder(backend.device)
        mode = "L" if sampling is None else "RGB"
        out = dec.decode(files, mode)
        assert dec.fallbacks == 0 and not dec.status.cpu().any()
        for case, got in zip(cases, out):
            want = np.asarray(Image.open(io.BytesIO(pil_bytes(case, 3))))
            assert np.array_equal(got.cpu().numpy().reshape(want.shape), want), case


# ---------------------------------------------------------------------------------------------------------------- 8. bounds
GUARD = 64


class GuardedEncoder(JpegEncoder):
    """Every buffer the encoder allocates lies between GUARD bytes of 0xA5 on either side."""

    def __init__(self, device):
        super().__init__(device)
        self.guarded = []

    def _alloc(self, shape, dtype):
        size = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape)) * size
        padded = -(-n // 8) * 8
        base = torch.full((padded + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=self.device)
        self.guarded.append((base, n))
        return base[GUARD:GUARD + n].view(dtype).view(shape)

    def guards_intact(self):
        return all(bool((b[:GUARD] == 0xA5).all()) and bool((b[GUARD + n:] == 0xA5).all()) for b, n in self.guarded)


def worst_cases():
    return [(h, w, s, 100, kind) for (h, w) in LARGE for s in SAMPLINGS for kind in ("noise", "binary")]


def test_worst_pictures_stay_inside_guarded_buffers(backend):
    enc = GuardedEncoder(backend.device)
    got = encode_cases(backend, worst_cases(), encoder=enc)
    assert len(enc.guarded) == 4 * 10 and enc.guards_intact()
    for case in worst_cases():
        assert got[case] == pil_bytes(case), case
    # two runs: every intermediate and output buffer bit for bit the same (what is never written keeps the guard pattern in both)
    enc2 = GuardedEncoder(backend.device)
    encode_cases(backend, worst_cases(), encoder=enc2)
    assert len(enc.guarded) == len(enc2.guarded)
    for k, ((b1, n1), (b2, n2)) in enumerate(zip(enc.guarded, enc2.guarded)):
        assert n1 == n2 and torch.equal(b1, b2), "allocation %d differs between two runs" % k


@pytest.mark.parametrize("shortfall", ["by one byte", "by half"])
def test_an_image_past_its_capacity_sets_its_status_only(emu, shortfall):
    big = (64, 80, None, 100, "noise")
    cases = [(37, 53, None, 100, "smooth"), big, (17, 33, None, 100, "smooth")]
    capacity = len(pil_bytes(big)) - 1 if shortfall == "by one byte" else len(pil_bytes(big)) // 2
    assert all(len(pil_bytes(c)) <= capacity for c in cases if c != big)
    enc = GuardedEncoder("cpu")
    batch = enc.encode([torch.from_numpy(case_picture(c).copy()) for c in cases], quality=100, capacity=capacity, as_bytes=False)
    assert enc.guards_intact()
    assert batch.status.tolist() == [0, 1, 0] and batch.lengths[1] == 0
    with pytest.raises(RuntimeError, match="not written"):
        batch.check()
    for i in (0, 2):
        o, n = int(batch.offsets[i]), int(batch.lengths[i])
        assert batch.data[o:o + n].numpy().tobytes() == pil_bytes(cases[i]), cases[i]


# ---------------------------------------------------------------------------------------------------------------- 9. arguments
@pytest.fixture
def no_launch(emu, monkeypatch):
    """Fails the test if anything of the encoder reaches the library."""
    call = emu.call

    def refuse(name, *args):
        if name == "ssn_jpeg_enc_layout":      # (two constants; launches nothing)
            return call(name, *args)
        raise AssertionError("%s was called" % name)
    enc = JpegEncoder("cpu")
    monkeypatch.setattr(emu, "call", refuse)
    return enc


def test_interface_refuses_bad_requests_before_any_launch(no_launch):
    enc = no_launch
    gray, rgb = torch.zeros(2, 16, 16, dtype=torch.uint8), torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        enc.encode(gray.float())
    with pytest.raises(ValueError, match="uint8"):
        enc.encode([gray[0], gray[1].to(torch.int16)])
    for bad in (torch.zeros(16, dtype=torch.uint8), torch.zeros(16, 16, dtype=torch.uint8), torch.zeros(1, 2, 16, 16, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[N, H, W\]"):
            enc.encode(bad)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        enc.encode([rgb])
    with pytest.raises(ValueError, match="channels"):
        enc.encode(torch.zeros(2, 16, 16, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mixed modes"):
        enc.encode([gray[0], rgb[0]])
    with pytest.raises(ValueError, match="non-empty"):
        enc.encode([])
    for q in (0, 101, -5, 95.0, "keep", None, True):
        with pytest.raises(ValueError, match="quality"):
            enc.encode(gray, quality=q)
    with pytest.raises(ValueError, match="RGB images only"):
        enc.encode(gray, subsampling=2)
    for s in (3, -1, "4:2:0"):
        with pytest.raises(ValueError, match="subsampling"):
            enc.encode(rgb, subsampling=s)
    for r in (-1, 65536, 2.5):
        with pytest.raises(ValueError, match="restart_blocks"):
            enc.encode(gray, restart_blocks=r)
    with pytest.raises(ValueError, match="capacity"):
        enc.encode(gray, capacity=0)
    for option in (dict(progressive=True), dict(optimize=True), dict(qtables="web_low"), dict(exif=b"Exif\0\0II"), dict(icc_profile=b"x"),
                   dict(restart_marker_rows=1)):
        with pytest.raises(ValueError, match="not supported"):
            enc.encode(gray, **option)
    with pytest.raises(ValueError, match="unknown option"):
        enc.encode(gray, qualty=3)


def test_wrappers_refuse_bad_tensors_before_any_launch(no_launch):
    enc = no_launch
    n, blocks = 2, 8
    i32 = torch.int32
    desc = torch.zeros(n, enc.desc_ints, dtype=i32)
    coef, quant, tables = torch.zeros(blocks, 64, dtype=torch.int16), torch.ones(2, 64, dtype=torch.int16), torch.zeros(4, 256, dtype=i32)
    blkbits, ivals = torch.zeros(blocks, dtype=i32), torch.zeros(n, dtype=i32)
    rawlen, status, ffcount, lengths = (torch.zeros(n, dtype=i32) for _ in range(4))
    offsets = torch.zeros(n, dtype=torch.int64)
    pix, raw, data, headers = (torch.zeros(64, dtype=torch.uint8) for _ in range(4))

    def raises(fn, *args):
        with pytest.raises(ValueError, match="jpeg_enc"):
            fn(*args)
    raises(K.jpeg_enc_blocks, pix.float(), desc, 4, quant, coef)
    raises(K.jpeg_enc_blocks, pix, desc[:, :-1].contiguous(), 4, quant, coef)
    raises(K.jpeg_enc_blocks, pix, desc.long(), 4, quant, coef)
    raises(K.jpeg_enc_blocks, pix, desc, 4, quant[:1], coef)
    raises(K.jpeg_enc_blocks, pix, desc, 4, quant, coef.int())
    raises(K.jpeg_enc_blocks, pix, desc, 4, quant, coef[:, :32].contiguous())
    raises(K.jpeg_enc_blocks, pix, desc, 0, quant, coef)
    raises(K.jpeg_enc_count, coef, desc, 4, tables[:3], blkbits, status)
    raises(K.jpeg_enc_count, coef, desc, 4, tables, blkbits[:4], status)
    raises(K.jpeg_enc_count, coef, desc, 4, tables, blkbits, status[:1])
    raises(K.jpeg_enc_count, coef, desc, 4, tables, blkbits.long(), status)
    raises(K.jpeg_enc_scan, desc, blkbits, torch.zeros(blocks + 1, dtype=i32), rawlen, status)
    raises(K.jpeg_enc_scan, desc, blkbits, ivals.long(), rawlen, status)
    raises(K.jpeg_enc_scan, desc, blkbits, ivals, rawlen[:1], status)
    raises(K.jpeg_enc_pack, coef, desc, 4, tables, blkbits, ivals, rawlen, raw[:62], status)
    raises(K.jpeg_enc_pack, coef, desc, 4, tables, blkbits, ivals, rawlen, raw.short(), status)
    raises(K.jpeg_enc_pack, coef, desc, 4, tables, blkbits, ivals, rawlen, raw[1:61], status)
    raises(K.jpeg_enc_assemble, raw, desc, ivals, rawlen, headers, ffcount, data, offsets.int(), lengths, status)
    raises(K.jpeg_enc_assemble, raw, desc, ivals, rawlen, headers, ffcount, data, offsets, lengths.long(), status)
    raises(K.jpeg_enc_assemble, raw, desc, ivals, rawlen, headers[:0], ffcount, data, offsets, lengths, status)
    raises(K.jpeg_enc_assemble, raw, desc, ivals, rawlen, headers, ffcount, data.int(), offsets, lengths, status)
    with pytest.raises(ValueError, match="contiguous"):
        K.jpeg_enc_blocks(pix, desc, 4, quant, coef.t())


# ---------------------------------------------------------------------------------------------------------------- 10. the tool
def _flow_tool():
    spec = importlib.util.spec_from_file_location("extract_flow_tool", os.path.join(ROOT, "tools", "extract_flow.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _read_dir(path):
    out = {}
    for name in sorted(os.listdir(path)):
        with open(os.path.join(path, name), "rb") as f:
            out[name] = f.read()
    return out


def test_extract_flow_with_gpu_encode_writes_the_same_files(backend, tmp_path):
    from action_detection_amd import _lib
    from action_detection_amd.train_data import FrameDirReader
    if backend.is_gpu:
        assert not _lib.emulator_active()
    src = tmp_path / "frames"
    os.makedirs(str(src / "video_a"))
    for t in range(3):
        Image.fromarray(np.roll(picture(32, 40, 2, seed=3), 2 * t, axis=1)).save(str(src / "video_a" / ("img_%05d.jpg" % (t + 1))), quality=90)
    tool = _flow_tool()
    common = ["--bound", "20", "--flow-prefix", "flow_", "--iterations", "20", "--quiet"]
    assert tool.main([str(src), str(tmp_path / "host")] + common) == 0
    assert tool.main([str(src), str(tmp_path / "device"), "--gpu-encode"] + common) == 0
    assert tool.main([str(src), str(tmp_path / "restart"), "--gpu-encode", "--restart-blocks", "4"] + common) == 0
    host, device, restart = (_read_dir(str(tmp_path / d / "video_a")) for d in ("host", "device", "restart"))
    assert sorted(host) == ["flow_x_00001.jpg", "flow_x_00002.jpg", "flow_y_00001.jpg", "flow_y_00002.jpg"]
    assert device == host
    assert sorted(restart) == sorted(host)
    for name, blob in host.items():
        assert restart[name] != blob and b"\xff\xdd\x00\x04\x00\x04" in restart[name], name
    # the flow both runs compressed, recovered from the tool's own pieces, compressed by PIL with restart markers
    from action_detection_amd.optical_flow import TVL1, FlowExtractor
    frames = torch.from_numpy(tool.load_frames(str(src / "video_a"), 3)).to(backend.device)
    flow = FlowExtractor(TVL1(iterations=20), bound=20.0, pair_batch=16).extract(frames).cpu().numpy()
    for i in range(2):
        for c, axis in enumerate("xy"):
            want = io.BytesIO()
            Image.fromarray(flow[i, c]).save(want, "JPEG", quality=95, restart_marker_blocks=4)
            assert restart["flow_%s_%05d.jpg" % (axis, i + 1)] == want.getvalue()
    for d in ("device", "restart"):
        got = FrameDirReader(str(tmp_path / d), modality="Flow", flow_prefix="flow_")("video_a", [1, 2])
        want = np.stack([np.asarray(Image.open(io.BytesIO(blobs["flow_%s_%05d.jpg" % (axis, i)])))
                         for blobs in [device if d == "device" else restart] for i in (1, 2) for axis in "xy"])
        assert np.array_equal(np.asarray(got).reshape(want.shape), want)


def test_restart_blocks_without_gpu_encode_is_refused(tmp_path):
    with pytest.raises(SystemExit):
        _flow_tool().main([str(tmp_path), str(tmp_path / "out"), "--restart-blocks", "4"])
