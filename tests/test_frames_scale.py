"""GroupScale on the device (csrc/frames.hip: ssn_frames_scale) against Pillow itself -- ``img.resize((w, h), Image.BILINEAR)`` /
``transforms.GroupScale`` -- bit for bit, and the test-time chains built on it (``GpuFrameTransform.oversample(scale_size=)``,
``center_crop``) against the host chain of ``action_detection_amd.transforms``.

The kernel works on tiles of 16 x 64 output pixels (SC_TH x SC_TW) and holds 13 taps per axis; the shapes below are the smallest
at which each of its paths can go wrong."""
import numpy as np
import pytest
import torch
from PIL import Image

import action_detection_amd  # noqa: F401
import ssn_oracle as O
from action_detection_amd import _lib
from action_detection_amd import kernels as K
from action_detection_amd import transforms as T
from action_detection_amd.input_pipeline import GpuFrameTransform, scaled_size

TH, TW = 16, 64      # the kernel's tile


def _pil(frame):
    return Image.fromarray(frame if frame.shape[2] == 3 else frame[:, :, 0])


def _pil_resize(frames, out_hw):
    oh, ow = out_hw
    return np.stack([np.asarray(_pil(f).resize((ow, oh), Image.BILINEAR)).reshape(oh, ow, frames.shape[3]) for f in frames])


def _frames(rs, n, h, w, c):
    """n random images, then an all-255 and an all-0 one."""
    a = rs.randint(0, 256, size=(n + 2, h, w, c)).astype(np.uint8)
    a[n], a[n + 1] = 255, 0
    return a


# (H, W, size, C, n): GroupScale(size) of n random + 2 constant images
GROUP_SCALE_CASES = [
    (12, 17, 16, 3, 3),      # upscale, landscape: 2-3 taps, windows clipped at both borders, rows of 51 bytes -> 22 x 16
    (20, 15, 24, 1, 2),      # upscale, portrait: which side is short, int(size * h / w) -> 24 x 32
    (40, 52, 24, 3, 1),      # downscale by 1.67: 4 taps, odd output width (ragged packed stores) -> 31 x 24
    (72, 96, 24, 3, 1),      # downscale by exactly 3: the tap count of the training kernel's cap
    (78, 104, 13, 3, 1),     # downscale by exactly 6 on the side GroupScale sets: the tap count of this kernel's cap
    (20, 20, 28, 3, 1),      # square: the `w <= h and w == size` branch ordering
]


@pytest.mark.parametrize("h,w,size,c,n", GROUP_SCALE_CASES)
def test_scale_matches_group_scale(backend, h, w, size, c, n):
    rs = np.random.RandomState(h * 131 + w)
    frames = _frames(rs, n, h, w, c)
    tf = GpuFrameTransform(8, [128], [1], device=backend.device)
    got = tf.scale(backend.put(torch.from_numpy(frames)), size)
    ref = np.stack([np.asarray(im).reshape(im.size[1], im.size[0], c) for im in T.GroupScale(size)([_pil(f) for f in frames])])
    ow, oh = scaled_size(w, h, size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == ref.shape == (n + 2, oh, ow, c)
    assert min(oh, ow) == size
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
    again = tf.scale(backend.put(torch.from_numpy(frames)), size)       # two runs: identical bytes
    assert torch.equal(again.cpu(), got.cpu())


def test_scale_noop_returns_its_input(backend):
    tf = GpuFrameTransform(8, [128], [1], device=backend.device)
    for h, w in ((24, 31), (31, 24), (24, 24)):
        frames = backend.put(torch.zeros((2, h, w, 3), dtype=torch.uint8))
        assert tf.scale(frames, 24) is frames
        assert scaled_size(w, h, 24) == (w, h)


def test_scale_refuses_more_than_the_tap_cap(backend):
    """79 x 105 -> GroupScale(13): 6.08 on the short side.  ValueError before anything is launched; dst stays as it was."""
    src = backend.put(torch.from_numpy(np.random.RandomState(0).randint(0, 256, (1, 79, 105, 3)).astype(np.uint8)))
    ow, oh = scaled_size(105, 79, 13)
    dst = backend.put(torch.full((1, oh, ow, 3), 0xA5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        K.frames_scale(src, (oh, ow), dst=dst)
    assert bool((dst.cpu() == 0xA5).all())
    with pytest.raises(ValueError):
        GpuFrameTransform(8, [128], [1], device=backend.device).scale(src, 13)
    with pytest.raises(ValueError):
        K.frames_scale(src, (4, 100))                                   # one axis far beyond the taps, the other upscaled


@pytest.mark.parametrize("c", [1, 3])
def test_scale_tile_edges(backend, c):
    """Outputs smaller than one tile, and one pixel / one row past a whole number of tiles in both axes."""
    rs = np.random.RandomState(7 + c)
    for (h, w), (oh, ow) in (((9, 30), (TH - 5, 23)),                   # out_h < TH, out_w < TW
                             ((50, 90), (2 * TH + 1, TW + 1)),          # three tile rows, two tile columns, ragged in both
                             ((TH, TW), (TH, TW)),                      # exactly one tile, identity coefficients
                             ((40, 2 * TW + 6), (3 * TH, 2 * TW + 2))):  # row bytes not a multiple of 4 for C = 1 and 3
        frames = _frames(rs, 1, h, w, c)
        got = K.frames_scale(backend.put(torch.from_numpy(frames)), (oh, ow))
        assert torch.equal(got.cpu(), torch.from_numpy(_pil_resize(frames, (oh, ow)))), (h, w, oh, ow)


def test_scale_image_stride_and_non_contiguous_input(backend):
    rs = np.random.RandomState(21)
    big = rs.randint(0, 256, size=(10, 40, 60, 3)).astype(np.uint8)
    dev = backend.put(torch.from_numpy(big))
    one = K.frames_scale(dev[3:4], (24, 31))
    assert torch.equal(one.cpu(), torch.from_numpy(_pil_resize(big[3:4], (24, 31))))
    view = dev[::2, :, 4:56]                                            # 5 images, strided in the image and the row
    assert not view.is_contiguous()
    five = K.frames_scale(view, (24, 31))
    assert torch.equal(five.cpu(), torch.from_numpy(_pil_resize(np.ascontiguousarray(big[::2, :, 4:56]), (24, 31))))


@pytest.mark.parametrize("offset", [64, 7])
def test_scale_writes_only_its_output(backend, offset):
    """dst carved out of a flat buffer of 0xA5 (once dword-aligned, once not: the byte-store path): the bytes on both sides stay."""
    rs = np.random.RandomState(5)
    frames = _frames(rs, 1, 40, 52, 3)
    n, oh, ow = frames.shape[0], 24, 31
    size = n * oh * ow * 3
    flat = backend.put(torch.full((offset + size + 64,), 0xA5, dtype=torch.uint8))
    dst = flat[offset:offset + size].view(n, oh, ow, 3)
    out = K.frames_scale(backend.put(torch.from_numpy(frames)), (oh, ow), dst=dst)
    assert out.data_ptr() == dst.data_ptr()
    host = flat.cpu()
    assert bool((host[:offset] == 0xA5).all()) and bool((host[offset + size:] == 0xA5).all())
    assert torch.equal(host[offset:offset + size].view(n, oh, ow, 3), torch.from_numpy(_pil_resize(frames, (oh, ow))))


def test_scale_argument_errors(backend):
    lib = _lib.get_lib()
    src = backend.put(torch.zeros((1, 12, 16, 3), dtype=torch.uint8))
    dst = backend.put(torch.full((1, 6, 8, 3), 0xA5, dtype=torch.uint8))
    need = int(lib.cdll.ssn_frames_scale_workspace_bytes(6, 8))
    assert need > 0
    wsp = backend.put(torch.zeros(need // 4 + 1, dtype=torch.int32))
    fn, stream = lib._fn["ssn_frames_scale"], K._stream(lib, src)
    assert fn(K._p(src), K._p(dst), 1, 12, 16, 3, 6, 8, K._p(wsp), need - 1, stream) == -3          # SSN_ERR_WORKSPACE
    assert b"workspace" in lib.cdll.ssn_last_error()
    src2 = backend.put(torch.zeros((1, 12, 16, 2), dtype=torch.uint8))
    assert fn(K._p(src2), K._p(dst), 1, 12, 16, 2, 6, 8, K._p(wsp), need, stream) == -1             # SSN_ERR_ARG: C = 2
    assert fn(K._p(src), K._p(dst), 1, 79, 105, 3, 13, 17, K._p(wsp), 1 << 20, stream) == -1        # beyond the ratio of 6
    assert fn(K._p(src), K._p(dst), 1, 12, 16, 3, 0, 8, K._p(wsp), need, stream) == -1
    assert bool((dst.cpu() == 0xA5).all())
    assert fn(K._p(src), K._p(dst), 1, 12, 16, 3, 6, 8, K._p(wsp), need, stream) == 0


# ------------------------------------------------------------------------------------------------------------- the test-time chains
def _host_chain(cropping, roll, mean, std):
    return T.Compose(cropping + [T.Stack(roll=roll), T.ToTorchFormatTensor(div=False), T.GroupNormalize(mean, std)])


def test_oversample_with_scale_rgb(backend):
    rs = np.random.RandomState(31)
    frames = rs.randint(0, 256, size=(3, 18, 25, 3)).astype(np.uint8)
    tf = GpuFrameTransform(20, [104, 117, 128], [1], roll=True, device=backend.device)
    got = tf.oversample(backend.put(torch.from_numpy(frames)), scale_size=24)
    want = _host_chain([T.GroupOverSample(20, 24)], True, [104, 117, 128], [1])([_pil(f) for f in frames])
    assert got.shape == want.shape == (10 * 3 * 3, 20, 20)
    assert torch.equal(got.cpu(), want)


def test_oversample_with_scale_flow(backend):
    """4 'L' images = x, y, x, y: the flipped crops invert the x component AFTER scaling."""
    rs = np.random.RandomState(32)
    flow = rs.randint(0, 256, size=(4, 18, 25, 1)).astype(np.uint8)
    tf = GpuFrameTransform(20, [128], [1], roll=True, is_flow=True, device=backend.device)
    got = tf.oversample(backend.put(torch.from_numpy(flow)), scale_size=24)
    want = _host_chain([T.GroupOverSample(20, 24)], True, [128], [1])([_pil(f) for f in flow])
    assert got.shape == want.shape == (10 * 4, 20, 20)
    assert torch.equal(got.cpu(), want)
    scaled = torch.from_numpy(_pil_resize(flow, (24, 33))).float()
    flipped_x = got.cpu().reshape(10, 4, 20, 20)[1, 0]                  # crop 0 mirrored, first x image
    assert torch.equal(flipped_x, (255.0 - scaled[0, :20, :20, 0].flip(1)) - 128.0)


@pytest.mark.parametrize("h,w", [(18, 25), (25, 18)])
def test_center_crop_with_scale(backend, h, w):
    """GroupScale(24) -> GroupCenterCrop(20): 33 - 20 = 13 is odd on the long side, so round() (to even) decides the offset."""
    rs = np.random.RandomState(33)
    frames = rs.randint(0, 256, size=(3, h, w, 3)).astype(np.uint8)
    tf = GpuFrameTransform(20, [104, 117, 128], [1], roll=True, device=backend.device)
    got = tf.center_crop(backend.put(torch.from_numpy(frames)), scale_size=24)
    want = _host_chain([T.GroupScale(24), T.GroupCenterCrop(20)], True, [104, 117, 128], [1])([_pil(f) for f in frames])
    assert got.shape == want.shape == (3 * 3, 20, 20)
    assert torch.equal(got.cpu(), want)


def test_oversample_without_scale_is_unchanged(backend):
    rs = np.random.RandomState(34)
    frames = rs.randint(0, 256, size=(3, 32, 43, 3)).astype(np.uint8)
    tf = GpuFrameTransform(24, [104, 117, 128], [1], roll=True, device=backend.device)
    dev = backend.put(torch.from_numpy(frames))
    ref = O.oversample_transform([f for f in frames], 24, 24, [104, 117, 128], [1], True, False)
    assert torch.equal(tf.oversample(dev).cpu(), ref)
    assert torch.equal(tf.oversample(dev, scale_size=None).cpu(), ref)
    assert torch.equal(tf.oversample(dev, scale_size=32).cpu(), ref)     # the short side is 32 already: no-op
