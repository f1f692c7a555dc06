"""The gray JPEG round trip without the file (csrc/jpeg_roundtrip.hip, jpeg_encode.roundtrip_gray) against PIL, bit for bit.

The truth everywhere is PIL itself: ``Image.fromarray(a).save(buf, "JPEG", quality=q)`` and ``Image.open(buf).convert("L")``, made at
test time from seeded arrays and shared between the tests.  Every comparison is ``torch.equal`` / ``np.array_equal``.  Shapes (height x
width) are the smallest at which each mechanism can fail: 1 x 1; 8 x 8 one full block; 7 x 9 and 9 x 7 ragged both ways with one and
two blocks; 16 x 24 no ragged edge; 20 x 36 and 37 x 52 rows that start at odd addresses (byte, 4-byte and 8-byte loads all taken);
64 x 340 with three images: the production row length (42.5 blocks), 1032 blocks in more than one workgroup.
"""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import action_detection_amd  # noqa: F401
from action_detection_amd import jpeg_encode as JE
from action_detection_amd import kernels as K
from action_detection_amd.jpeg_decode import JpegDecoder
from action_detection_amd.jpeg_encode import JpegEncoder, roundtrip_gray

SHAPES = [(1, 1), (8, 8), (7, 9), (9, 7), (16, 24), (20, 36), (37, 52), (64, 340)]
QUALITIES = [95, 75, 30, 100]
KINDS = ["noise", "zeros", "full", "ramp", "checker", "flow"]


def batches_of(h, w):
    return (3,) if (h, w) == (64, 340) else (1, 5)


@functools.lru_cache(maxsize=None)
def flow_field():
    """A quantised flow field as the extractor writes it (``flow_to_uint8``'s rule at bound 20, in numpy: rint is half to even as
    rintf): a blob moving by two pixels on a still background with sub-pixel jitter -> mostly 127 / 128."""
    rs = np.random.RandomState(11)
    yy, xx = np.mgrid[0:64, 0:340].astype(np.float32)
    v = 2.0 * np.exp(-(((yy - 30) / 9.0) ** 2 + ((xx - 150) / 25.0) ** 2)) + rs.normal(0, 0.04, yy.shape)
    q = np.rint(np.float32(255.0) * (v.astype(np.float32) + np.float32(20.0)) / np.float32(40.0))
    a = np.clip(q, 0, 255).astype(np.uint8)
    assert ((a == 127) | (a == 128)).mean() > 0.5 and a.max() > 135
    return a


@functools.lru_cache(maxsize=None)
def images(kind, n, h, w):
    """uint8 [n, h, w], read-only; the images of a batch differ where the kind allows it."""
    rs = np.random.RandomState(h * 1009 + w * 13 + n)
    if kind == "noise":
        a = rs.randint(0, 256, (n, h, w))
    elif kind == "zeros":
        a = np.zeros((n, h, w))
    elif kind == "full":
        a = np.full((n, h, w), 255)
    elif kind == "ramp":
        a = np.stack([np.broadcast_to((np.arange(w) * (3 + i) + 17 * i) % 256, (h, w)) for i in range(n)])
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([((yy + xx + i) & 1) * 255 for i in range(n)])
    else:
        f = flow_field()
        a = np.stack([np.roll(f, (5 * i, 31 * i), axis=(0, 1))[64 - h:, 150 - min(w, 150):][:, :w] for i in range(n)])
    a = np.ascontiguousarray(a.astype(np.uint8))
    assert a.shape == (n, h, w)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pil_roundtrip(kind, n, h, w, quality):
    """The yardstick, made once per case and shared."""
    out = []
    for a in images(kind, n, h, w):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=quality)
        out.append(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("L")))
    out = np.stack(out)
    out.setflags(write=False)
    return out


def put(backend, a):
    return backend.put(torch.from_numpy(np.array(a)))


# ---------------------------------------------------------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_equals_pil(backend, shape, quality):
    h, w = shape
    for n in batches_of(h, w):
        for kind in KINDS:
            got = roundtrip_gray(put(backend, images(kind, n, h, w)), quality).cpu().numpy()
            want = pil_roundtrip(kind, n, h, w, quality)
            assert got.dtype == np.uint8 and got.shape == want.shape
            assert np.array_equal(got, want), (kind, n, shape, quality, np.argwhere(got != want)[:4])


def test_the_cases_are_what_they_claim():
    """On PIL's pixels, never on the product: the contents reach the range limit on both sides and change under every quality but
    the flat ones."""
    checker = pil_roundtrip("checker", 1, 37, 52, 30)
    assert checker.min() == 0 and checker.max() == 255 and not np.array_equal(checker, images("checker", 1, 37, 52))
    assert not np.array_equal(pil_roundtrip("noise", 1, 37, 52, 95), images("noise", 1, 37, 52))
    assert not np.array_equal(pil_roundtrip("flow", 3, 64, 340, 95), images("flow", 3, 64, 340))
    for kind in ("zeros", "full"):
        assert np.array_equal(pil_roundtrip(kind, 1, 20, 36, 30), images(kind, 1, 20, 36))
    assert JE.quant_tables(100)[0].tolist() == [1] * 64


# ---------------------------------------------------------------------------------------------------------------- 2. in place, views, repeats
@pytest.mark.parametrize("shape", [(7, 9), (37, 52), (64, 340)], ids=lambda s: "%dx%d" % s)
def test_in_place_equals_out_of_place(backend, shape):
    h, w = shape
    for kind in ("noise", "flow"):
        x = put(backend, images(kind, 3, h, w))
        keep = x.clone()
        want = roundtrip_gray(x, 95)
        assert torch.equal(x, keep)                       # (out of place leaves the input alone)
        got = roundtrip_gray(x, 95, out=x)
        assert got.data_ptr() == x.data_ptr() and torch.equal(x, want)
        assert np.array_equal(want.cpu().numpy(), pil_roundtrip(kind, 3, h, w, 95))


def test_a_non_contiguous_view_equals_its_copy(backend):
    big = put(backend, images("noise", 3, 64, 340))
    for view in (big[:, 3:40, 7:59], big[:, ::2, ::3], big.transpose(1, 2), big[:, :, :, None][:, 1:, :-1]):
        assert not view.is_contiguous()
        got = roundtrip_gray(view, 75)
        assert got.shape == view.shape and torch.equal(got, roundtrip_gray(view.contiguous(), 75))
    sub = np.ascontiguousarray(images("noise", 3, 64, 340)[:, 3:40, 7:59])
    want = []
    for a in sub:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=75)
        want.append(np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("L")))
    assert np.array_equal(roundtrip_gray(big[:, 3:40, 7:59], 75).cpu().numpy(), np.stack(want))


def test_trailing_channel_axis_is_accepted(backend):
    x = put(backend, images("flow", 5, 20, 36))
    got = roundtrip_gray(x[:, :, :, None], 95)
    assert got.shape == (5, 20, 36, 1) and torch.equal(got[:, :, :, 0], roundtrip_gray(x, 95))


def test_a_repeat_is_bit_identical(backend):
    x = put(backend, images("noise", 3, 64, 340))
    first = roundtrip_gray(x, 95)
    for _ in range(2):
        assert torch.equal(roundtrip_gray(x, 95), first)


# ---------------------------------------------------------------------------------------------------------------- 3. bounds
@pytest.mark.parametrize("shape", [(1, 1), (7, 9), (9, 7), (37, 52), (64, 340)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("shift", [0, 1, 4])
def test_output_stays_between_its_guards(backend, shape, shift):
    """The output is an inner view of a flat buffer whose other bytes hold a pattern; `shift` moves its first byte off the 8- and
    4-byte alignment, so that every store width is taken next to a guard."""
    h, w = shape
    n = 3
    guard = 64 + shift
    size = n * h * w
    src = put(backend, images("noise", n, h, w))
    flat = torch.full((size + 2 * guard + 8,), 0xA5, dtype=torch.uint8, device=backend.device)
    out = flat[guard:guard + size].view(n, h, w)
    got = roundtrip_gray(src, 95, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((flat[:guard] == 0xA5).all()) and bool((flat[guard + size:] == 0xA5).all())
    assert np.array_equal(out.cpu().numpy(), pil_roundtrip("noise", n, h, w, 95))
    # the same from a source that sits at the shifted address (the load widths), in place
    flat2 = torch.full_like(flat, 0x5A)
    inner = flat2[guard:guard + size].view(n, h, w)
    inner.copy_(src)
    roundtrip_gray(inner, 95, out=inner)
    assert bool((flat2[:guard] == 0x5A).all()) and bool((flat2[guard + size:] == 0x5A).all())
    assert torch.equal(inner, out)


# ---------------------------------------------------------------------------------------------------------------- 4. the three code paths
def test_equals_encoder_then_decoder(backend):
    for kind, n, h, w in (("noise", 3, 64, 340), ("flow", 3, 64, 340), ("checker", 5, 37, 52), ("noise", 5, 7, 9)):
        x = put(backend, images(kind, n, h, w))
        files = JpegEncoder(backend.device).encode(x, quality=95)
        dec = JpegDecoder(backend.device)
        decoded = dec.decode(files, mode="L", stack=True)
        assert dec.fallbacks == 0
        assert torch.equal(roundtrip_gray(x, 95), decoded.reshape(n, h, w)), (kind, n, h, w)


# ---------------------------------------------------------------------------------------------------------------- 5. arguments
@pytest.fixture
def no_launch(emu, monkeypatch):
    """Fails the test if anything reaches the library."""
    def refuse(name, *args):
        raise AssertionError("%s was called" % name)
    monkeypatch.setattr(emu, "call", refuse)


def test_interface_refuses_bad_requests_before_any_launch(no_launch):
    gray = torch.zeros(2, 16, 16, dtype=torch.uint8)
    for bad in (gray.float(), gray.to(torch.int16), gray.numpy()):
        with pytest.raises(ValueError, match="uint8"):
            roundtrip_gray(bad)
    for bad in (gray[0], gray[0, 0], gray[None, :, :, :, None], torch.zeros(2, 16, 16, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\[N, H, W\]"):
            roundtrip_gray(bad)
    with pytest.raises(ValueError, match="N >= 1"):
        roundtrip_gray(gray[:0])
    for q in (0, 101, -5, 95.0, "keep", None, True):
        with pytest.raises(ValueError, match="quality"):
            roundtrip_gray(gray, quality=q)
    for out in (gray[:1], gray.float(), torch.zeros(2, 16, 32, dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(ValueError, match="out must be"):
            roundtrip_gray(gray, out=out)
    table = torch.ones(64, dtype=torch.int32)
    for args in ((gray.float(), table), (gray, table.long()), (gray, table[:63]), (gray[0], table)):
        with pytest.raises(ValueError, match="jpeg_roundtrip_gray"):
            K.jpeg_roundtrip_gray(*args)
    with pytest.raises(ValueError, match="jpeg_roundtrip_gray"):
        K.jpeg_roundtrip_gray(gray, table, out=gray[:1])
    with pytest.raises(ValueError, match="contiguous"):
        K.jpeg_roundtrip_gray(gray.transpose(1, 2), table)


def test_a_host_tensor_is_refused_outside_the_emulator():
    from action_detection_amd import _lib
    assert not _lib.emulator_active()
    with pytest.raises(ValueError, match="on the device"):
        roundtrip_gray(torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_the_library_refuses_bad_sizes_and_null_pointers(emu):
    buf = torch.zeros(64, dtype=torch.uint8)
    table = torch.ones(64, dtype=torch.int32)
    for args in ((buf.data_ptr(), buf.data_ptr(), 0, 8, 8, table.data_ptr()), (buf.data_ptr(), buf.data_ptr(), 1, 0, 8, table.data_ptr()),
                 (buf.data_ptr(), buf.data_ptr(), 1, 8, 65536, table.data_ptr()), (None, buf.data_ptr(), 1, 8, 8, table.data_ptr()),
                 (buf.data_ptr(), None, 1, 8, 8, table.data_ptr()), (buf.data_ptr(), buf.data_ptr(), 1, 8, 8, None)):
        with pytest.raises(RuntimeError, match="jpeg_roundtrip_gray"):
            emu.call("ssn_jpeg_roundtrip_gray", *args, None)
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------- 6. past 2^31 bytes
@pytest.mark.gpu
def test_a_batch_past_two_gib_addresses_its_last_image(hip_library):
    """24 700 images of 256 x 340 are 2.15e9 bytes: the offset of the last image does not fit 32 bits.  In place, noise in the first
    and the last image, zeros between (a flat image comes back as it went in)."""
    h, w, n = 256, 340, 24700
    assert n * h * w > 2 ** 31
    x = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
    noise = np.random.RandomState(5).randint(0, 256, (2, h, w)).astype(np.uint8)
    x[0].copy_(torch.from_numpy(noise[0]))
    x[n - 1].copy_(torch.from_numpy(noise[1]))
    roundtrip_gray(x, 95, out=x)
    for i, a in ((0, noise[0]), (n - 1, noise[1])):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=95)
        assert np.array_equal(x[i].cpu().numpy(), np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("L"))), i
    assert not bool(x[1:n - 1].any())
