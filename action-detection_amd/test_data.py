"""Frame source of the SSN tester (tools/test_ssn.py): what ``SSNDataSet.get_test_data`` hands its caller besides the proposal
arrays (/root/reference/ssn_dataset.py:430-450), split the way this library runs it -- a reader delivers the frames of a few ticks
(decoded with PIL, or as the files' bytes), a transform turns them into the crop-major network input ``DenseTester.frame_scores``
consumes: the host chain of ``transforms`` as in the reference, or ``DeviceTestChain`` (decode, GroupScale, crops and normalisation
on the device).
"""
import numpy as np
import torch

from .input_pipeline import GpuFrameTransform, scaled_size
from . import kernels as K


def test_frame_batches(sampler, video, reader, transform, tick_batch=32):
    """The generator of ``get_test_data`` (ssn_dataset.py:434-450) without its batch size of 4: for every tick ``p`` of
    ``sampler.test_ticks(video)[0]`` the frames ``min(frame_cnt, p + x)``, ``x < new_length`` (Flow: x then y image per frame), read
    through ``reader(video id, frame numbers)`` (``train_data.FrameDirReader`` / ``CompressedFrameDirReader``) and handed to
    ``transform`` every ``tick_batch`` ticks; the shorter tail batch is included.  Yields what ``transform`` returns."""
    frame_cnt = video.num_frames
    pending, ticks = [], 0
    for p in sampler.test_ticks(video)[0]:
        pending.extend(min(frame_cnt, int(p) + x) for x in range(sampler.new_length))
        ticks += 1
        if ticks % tick_batch == 0:
            yield transform(reader(video.id, pending))
            pending = []
    if pending:
        yield transform(reader(video.id, pending))


test_frame_batches.__test__ = False      # (a library function whose name starts with "test": not a test case)


def host_test_chain(net_input_size, scale_size, mean, std, test_crops=10, roll=True):
    """The reference's chain (ssn_test.py:107-143) on decoded uint8 frames [n, H, W, C]: PIL images -> GroupOverSample(input, scale) or
    GroupScale + GroupCenterCrop -> Stack(roll) -> ToTorchFormatTensor(div=False) -> GroupNormalize."""
    from PIL import Image
    from . import transforms as T
    if test_crops == 1:
        cropping = [T.GroupScale(scale_size), T.GroupCenterCrop(net_input_size)]
    elif test_crops == 10:
        cropping = [T.GroupOverSample(net_input_size, scale_size)]
    else:
        raise ValueError("Only 1 and 10 crops are supported while we got {}".format(test_crops))
    chain = T.Compose(cropping + [T.Stack(roll=roll), T.ToTorchFormatTensor(div=False), T.GroupNormalize(mean, std)])

    def transform(frames):
        frames = np.asarray(frames)
        return chain([Image.fromarray(f if f.shape[2] == 3 else f[:, :, 0]) for f in frames])
    return transform


class DeviceTestChain(object):
    """``--gpu-decode``: the files' bytes -> the network input of ``test_crops`` crops, on the device: ``JpegDecoder`` ->
    ``GpuFrameTransform.oversample(scale_size=)`` / ``center_crop(scale_size=)``.  Frames that GroupScale would shrink by more than
    the scale kernel's ratio of 6 are decoded and scaled with PIL on the host and uploaded at ``scale_size``; ``host_scaled`` counts the
    batches that went that way, ``host_decoded`` the files the device decoder could not take."""

    def __init__(self, net_input_size, scale_size, mean, std, modality, test_crops=10, device="cuda:0"):
        from .jpeg_decode import JpegDecoder, parse_jpeg
        if test_crops not in (1, 10):
            raise ValueError("Only 1 and 10 crops are supported while we got {}".format(test_crops))
        self._parse = parse_jpeg
        self.decoder = JpegDecoder(device)
        self.tf = GpuFrameTransform(net_input_size, mean, std, roll=True, is_flow=modality == "Flow", device=device)
        self.mode = "RGB" if modality in ("RGB", "RGBDiff") else "L"
        self.scale_size, self.test_crops = scale_size, test_crops
        self.host_scaled = 0

    @property
    def host_decoded(self):
        """Files the device decoder handed to PIL (``JpegDecoder.fallbacks``: progressive files, unsupported tables, ...)."""
        return self.decoder.fallbacks

    def _too_large(self, blob):
        h = self._parse(blob)
        if h.supported:
            w, hh = h.width, h.height
        else:                               # (a file the decoder hands to PIL: PIL reads its size from the header)
            import io
            from PIL import Image
            with Image.open(io.BytesIO(blob)) as im:
                w, hh = im.size
        ow, oh = scaled_size(w, hh, self.scale_size)
        return not K.frames_scale_supported(hh, w, oh, ow)

    def _host_scaled_frames(self, blobs):
        import io
        from PIL import Image
        from .transforms import GroupScale
        ims = GroupScale(self.scale_size)([Image.open(io.BytesIO(b)).convert(self.mode) for b in blobs])
        a = np.stack([np.asarray(im) for im in ims])
        return torch.from_numpy(a if a.ndim == 4 else a[:, :, :, None]).to(self.tf.mean.device)

    def __call__(self, blobs):
        scale = self.scale_size
        if self._too_large(blobs[0]):
            frames, scale = self._host_scaled_frames(blobs), None
            self.host_scaled += 1
        else:
            frames = self.decoder.decode(blobs, self.mode, stack=True)
        if self.test_crops == 10:
            return self.tf.oversample(frames, scale_size=scale)
        return self.tf.center_crop(frames, scale_size=scale)
