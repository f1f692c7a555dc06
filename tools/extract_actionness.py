#!/usr/bin/env python
"""Extract actionness scores: the counterpart of the reference's binary_test.py on the kernels of this project.

A trained ``BinaryClassifier`` runs over every ``--frame_interval``-th frame of every video of a proposal list and the
``{video id: float32 [T, crops, 2]}`` score file ``gen_bottom_up_proposals.py`` (here: ``tag_proposals``) reads is written.
Flags are named as the reference's; ``--proposal-list`` stands in for its YAML lookup of (dataset, subset), ``--frame-root`` for
the frame folders the list names.  ``--grouping reference`` (default) writes exactly the rows binary_test.py writes, ``tick``
the honest ones (actionness_test.py says what the difference is).

    python tools/extract_actionness.py RGB weights.pth.tar scores_rgb.pc --proposal-list data/thumos14_tag_val_proposal_list.txt \\
        --frame-root /data/frames --frame_interval 5 --test_crops 10

The frame source is a callable ``load(video id, frame number) -> [PIL images]`` (one RGB image, or the x and y flow images);
``pil_loader`` below reads the reference's file layout.  ``extract(...)`` takes any other.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pil_loader(frame_root, modality, flow_pref=""):
    """load_binary_score.py:198-205: img_{:05d}.jpg, or {flow_pref}x_{:05d}.jpg + {flow_pref}y_{:05d}.jpg as 'L' images."""
    from PIL import Image

    def load(vid, idx):
        folder = os.path.join(frame_root, vid)
        if modality == "RGB":
            return [Image.open(os.path.join(folder, "img_{:05d}.jpg".format(idx))).convert("RGB")]
        return [Image.open(os.path.join(folder, "{}{}_{:05d}.jpg".format(flow_pref, p, idx))).convert("L") for p in "xy"]
    return load


def frame_batches(load, video, sampler, transform, gen_batch=4):
    """The generator of load_binary_score.get_test_data (:288-304): gen_batch ticks per batch, crop-major after the transform."""
    frames = []
    for n, row in enumerate(sampler.test_frames(video)):
        for idx in row:
            frames.extend(load(video.id, int(idx)))
        if (n + 1) % gen_batch == 0:
            yield transform(frames)
            frames = []
    if frames:
        yield transform(frames)


def file_reader(frame_root, modality, flow_pref=""):
    """The same files as ``pil_loader``, undecoded: read(video id, frame number) -> [bytes]."""
    def read(vid, idx):
        folder = os.path.join(frame_root, vid)
        names = ["img_{:05d}.jpg".format(idx)] if modality == "RGB" else ["{}{}_{:05d}.jpg".format(flow_pref, p, idx) for p in "xy"]
        out = []
        for name in names:
            with open(os.path.join(folder, name), "rb") as f:
                out.append(f.read())
        return out
    return read


def device_transform(net, modality, device, input_size=None, scale=False, index="host"):
    """--gpu-decode: [bytes] -> what ``transform(frames)`` of ``extract`` yields for 10 crops, with the files decoded on the device
    (jpeg_decode.JpegDecoder) and GroupOverSample -> Stack -> ToTorchFormatTensor -> GroupNormalize as one launch
    (input_pipeline.GpuFrameTransform).  GroupOverSample's GroupScale(scale_size) is the identity on frames whose short side is
    scale_size already -- the 340 x 256 frames the extraction scripts write; other sizes are refused unless ``scale`` (--gpu-scale)
    is set: then GroupScale runs on the device too (``GpuFrameTransform.scale``; Inception-v3's scale_size is 341, so its frames
    always need it)."""
    from action_detection_amd.input_pipeline import GpuFrameTransform
    from action_detection_amd.jpeg_decode import JpegDecoder
    decoder = JpegDecoder(device, index=index)
    tf = GpuFrameTransform(net.input_size if input_size is None else input_size, net.input_mean, net.input_std, roll=True,
                           is_flow=modality == "Flow", device=device)

    def transform(blobs):
        frames = decoder.decode(blobs, "RGB" if modality == "RGB" else "L", stack=True)
        if scale:
            return tf.oversample(frames, scale_size=net.scale_size)
        if min(frames.shape[1], frames.shape[2]) != net.scale_size:
            raise ValueError("--gpu-decode needs frames whose short side is %d, got %d x %d" % (net.scale_size, frames.shape[2], frames.shape[1]))
        return tf.oversample(frames)
    return transform


def build_net(modality, weights, arch="BNInception", device="cuda:0"):
    """The trained ``BinaryClassifier`` of a checkpoint, ready for ``ActionnessTester`` on ``device``."""
    import torch
    from action_detection_amd.binary_model import BinaryClassifier
    data_length = 1 if modality == "RGB" else 5
    net = BinaryClassifier(2, 5, modality, test_mode=True, new_length=data_length, base_model=arch)
    checkpoint = torch.load(weights, map_location="cpu")
    print("model epoch {} loss: {}".format(checkpoint.get('epoch'), checkpoint.get('best_loss')))
    net.load_state_dict({'.'.join(k.split('.')[1:]): v for k, v in checkpoint['state_dict'].items()})
    net.prepare_test_fc()
    return net.to(device).eval()


def extract(net, sampler, load, test_crops=10, input_size=None, tick_batch=32, grouping="reference", max_num=-1, verbose=True,
            transform=None):
    """-> ActionnessScores of the first max_num (all) videos of the sampler's list; ``net`` as ActionnessTester takes it.
    ``transform``: replaces the host chain (``device_transform`` with a ``file_reader`` as ``load``)."""
    import time
    from action_detection_amd import transforms as T
    from action_detection_amd.actionness_test import ActionnessTester
    input_size = net.input_size if input_size is None else input_size
    if transform is not None:
        if test_crops != 10:
            raise ValueError("a device transform yields the 10 crops of GroupOverSample, got test_crops = {}".format(test_crops))
        cropping = None
    elif test_crops == 1:
        cropping = [T.GroupScale(net.scale_size), T.GroupScale(input_size)]
    elif test_crops == 10:
        cropping = [T.GroupOverSample(input_size, net.scale_size)]
    else:
        raise ValueError("only 1 and 10 crops are supported while we got {}".format(test_crops))
    if transform is None:
        transform = T.Compose(cropping + [T.Stack(roll=True), T.ToTorchFormatTensor(div=False),
                                          T.GroupNormalize(net.input_mean, net.input_std)])
    tester = ActionnessTester(net, tick_batch=tick_batch, grouping=grouping)
    videos = sampler.video_list if max_num <= 0 else sampler.video_list[:max_num]
    start = time.time()

    def items():
        for i, video in enumerate(videos):
            yield video.id.split('/')[-1], frame_batches(load, video, sampler, transform), len(sampler.test_ticks(video)), test_crops
            if verbose and i:
                print('video {} done, total {}/{}, average {:.04f} sec/video'.format(i - 1, i, len(videos),
                                                                                     (time.time() - start) / i))
    return tester.score_videos(items())


def main(argv=None):
    ap = argparse.ArgumentParser(description="extract actionness scores")
    ap.add_argument("modality", type=str, choices=["RGB", "Flow"])
    ap.add_argument("weights", type=str)
    ap.add_argument("save_scores", type=str)
    ap.add_argument("--proposal-list", required=True, help="the processed proposal list of the subset to score")
    ap.add_argument("--frame-root", type=str, default="")
    ap.add_argument("--arch", type=str, default="BNInception", choices=["BNInception", "InceptionV3"])
    ap.add_argument("--frame_interval", type=int, default=5)
    ap.add_argument("--max_num", type=int, default=-1)
    ap.add_argument("--test_crops", type=int, default=10)
    ap.add_argument("--input_size", type=int, default=None)
    ap.add_argument("--flow_pref", type=str, default="")
    ap.add_argument("--tick_batch", type=int, default=32)
    ap.add_argument("--grouping", type=str, default="reference", choices=["reference", "tick"])
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--gpu-decode", action="store_true", help="decode the frames on the device (10 crops, frames at scale_size)"
                    "; files rewritten with tools/transcode_frames.py (restart markers, same pixels) decode on one lane per interval instead of one per file")
    ap.add_argument("--device-index", action="store_true", help="with --gpu-decode: find the restart intervals on the device too (JpegDecoder(index=\"device\")): no host work per interval or per byte")
    ap.add_argument("--gpu-scale", action="store_true", help="with --gpu-decode: frames of any size, GroupScale on the device")
    args = ap.parse_args(argv)

    import action_detection_amd as pkg
    from action_detection_amd.actionness_sampling import ActionnessSampler
    pkg.build()
    data_length = 1 if args.modality == "RGB" else 5
    net = build_net(args.modality, args.weights, args.arch, args.device)
    sampler = ActionnessSampler(args.proposal_list, new_length=data_length, test_interval=args.frame_interval)
    if args.gpu_decode:
        scores = extract(net, sampler, file_reader(args.frame_root, args.modality, args.flow_pref), args.test_crops, args.input_size,
                         args.tick_batch, args.grouping, args.max_num,
                         transform=device_transform(net, args.modality, args.device, args.input_size, scale=args.gpu_scale,
                                                    index="device" if args.device_index else "host"))
    else:
        scores = extract(net, sampler, pil_loader(args.frame_root, args.modality, args.flow_pref), args.test_crops, args.input_size,
                         args.tick_batch, args.grouping, args.max_num)
    scores.save(args.save_scores)
    print("wrote {} videos to {}".format(len(scores), args.save_scores))
    return scores


if __name__ == "__main__":
    main()
