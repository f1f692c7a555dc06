#!/usr/bin/env python
"""Extract optical flow images: the "Extract Frames and Optical Flow Images" stage of the reference's workflow on the kernels of
this project (the reference hands it to dense_flow, i.e. OpenCV's CUDA TV-L1).

Every directory under SRC_ROOT that holds ``img_00001.jpg, img_00002.jpg, ...`` is one video; for each of them
``OUT_ROOT/<video>/<flow-prefix>x_%05d.jpg`` and ``<flow-prefix>y_%05d.jpg`` are written, number i holding the flow from frame i to
frame i + 1 quantised as dense_flow does (``--bound``) -- the files ``FrameDirReader(modality="Flow")`` and the reference's data
sets read.  The frames of a video go to the GPU once; the flow comes back as uint8, or with ``--gpu-encode`` as the finished files
(the same bytes; ``--restart-blocks K`` adds restart markers the device decoder splits at).

    python tools/extract_flow.py /data/frames /data/flow --bound 20 --flow-prefix flow_

The algorithm and the standing of its parity (a float64 restatement, not dense_flow's own files) are in DESIGN.md section 3.9.
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_FRAME = re.compile(r"^img_(\d{5})\.jpg$")


def video_dirs(src_root):
    """[(relative directory, number of consecutive frames from img_00001.jpg)] of every directory that holds frames."""
    out = []
    for d, _, files in sorted(os.walk(src_root)):
        numbers = {int(m.group(1)) for m in map(_FRAME.match, files) if m}
        n = 0
        while n + 1 in numbers:
            n += 1
        if n >= 2:
            out.append((os.path.relpath(d, src_root), n))
    return out


def load_frames(folder, n):
    import numpy as np
    from PIL import Image
    frames = []
    for i in range(1, n + 1):
        with Image.open(os.path.join(folder, "img_{:05d}.jpg".format(i))) as im:
            frames.append(np.asarray(im.convert("RGB")))
    return np.stack(frames)


def load_frames_on_device(folder, n, decoder):
    """The same frames, decoded on the device (--gpu-decode): only the files' bytes are uploaded."""
    blobs = []
    for i in range(1, n + 1):
        with open(os.path.join(folder, "img_{:05d}.jpg".format(i)), "rb") as f:
            blobs.append(f.read())
    return decoder.decode(blobs, "RGB", stack=True)


def write_flow(folder, prefix, flow_u8, quality):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i in range(flow_u8.shape[0]):
        for c, axis in enumerate("xy"):
            Image.fromarray(flow_u8[i, c]).save(os.path.join(folder, "{}{}_{:05d}.jpg".format(prefix, axis, i + 1)), quality=quality)


def write_flow_on_device(folder, prefix, flow_u8, quality, encoder, restart_blocks=0):
    """The same files from a flow that stays on the device (--gpu-encode): uint8 [T-1, 2, H, W] is compressed there
    (jpeg_encode.JpegEncoder) and only the files' bytes come down."""
    os.makedirs(folder, exist_ok=True)
    pairs, _, h, w = flow_u8.shape
    files = encoder.encode(flow_u8.reshape(pairs * 2, h, w), quality=quality, restart_blocks=restart_blocks)
    for i in range(pairs):
        for c, axis in enumerate("xy"):
            with open(os.path.join(folder, "{}{}_{:05d}.jpg".format(prefix, axis, i + 1)), "wb") as f:
                f.write(files[2 * i + c])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src_root")
    ap.add_argument("out_root")
    ap.add_argument("--bound", type=float, default=20)
    ap.add_argument("--flow-prefix", default="flow_")
    ap.add_argument("--pair-batch", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--jpeg-quality", type=int, default=95)
    ap.add_argument("--gpu-decode", action="store_true", help="decode the input frames on the device (jpeg_decode.JpegDecoder)"
                    "; files rewritten with tools/transcode_frames.py (restart markers, same pixels) decode on one lane per interval instead of one per file")
    ap.add_argument("--device-index", action="store_true", help="with --gpu-decode: find the restart intervals on the device too (JpegDecoder(index=\"device\")): no host work per interval or per byte")
    ap.add_argument("--gpu-encode", action="store_true",
                    help="compress the flow images on the device (jpeg_encode.JpegEncoder): the same bytes, without PIL")
    ap.add_argument("--restart-blocks", type=int, default=0,
                    help="with --gpu-encode: restart markers every K MCUs (PIL's restart_marker_blocks=K); the decoder splits at them")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)

    import torch
    from action_detection_amd import _lib
    from action_detection_amd.optical_flow import TVL1, FlowExtractor
    dev = torch.device("cpu") if _lib.emulator_active() else torch.device("cuda")
    extractor = FlowExtractor(TVL1(iterations=args.iterations), bound=args.bound, pair_batch=args.pair_batch)
    decoder = None
    if args.gpu_decode:
        from action_detection_amd.jpeg_decode import JpegDecoder
        decoder = JpegDecoder(dev, index="device" if args.device_index else "host")
    if args.restart_blocks and not args.gpu_encode:
        ap.error("--restart-blocks needs --gpu-encode")
    encoder = None
    if args.gpu_encode:
        from action_detection_amd.jpeg_encode import JpegEncoder
        encoder = JpegEncoder(dev)
    videos = video_dirs(args.src_root)
    if not videos:
        print("no directory with img_00001.jpg, img_00002.jpg, ... under %s" % args.src_root, file=sys.stderr)
        return 1
    for rel, n in videos:
        if decoder is not None:
            frames = load_frames_on_device(os.path.join(args.src_root, rel), n, decoder)
        else:
            frames = torch.from_numpy(load_frames(os.path.join(args.src_root, rel), n)).to(dev)
        flow = extractor.extract(frames)
        if encoder is not None:
            write_flow_on_device(os.path.join(args.out_root, rel), args.flow_prefix, flow, args.jpeg_quality, encoder, args.restart_blocks)
        else:
            write_flow(os.path.join(args.out_root, rel), args.flow_prefix, flow.cpu().numpy(), args.jpeg_quality)
        if not args.quiet:
            print("%s: %d frames -> %d flow pairs" % (rel, n, flow.shape[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
