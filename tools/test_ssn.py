#!/usr/bin/env python
"""Test an SSN: the counterpart of the reference's ssn_test.py on the kernels of this project.

A trained ``SSN`` scores every ``--frame_interval``-th frame of every video of a proposal list (``dense_test.DenseTester``) and the
score pickle ``tools/eval_detections.py`` reads is written: ``{video id: (rel_props float64 [P, 2], act float32 [P, C + 1], comp
float32 [P, C], reg float32 [P, C, 2] or None)}``; ``--save_raw_scores`` also writes ``{video id: output [T, D]}``.  Positionals
and flags are named as the reference's; ``--proposal-list`` stands in for its YAML lookup of the test list, ``--frame-root`` for the
frame folders the list names.

    python tools/test_ssn.py thumos14 RGB weights.pth.tar scores_rgb.pc --proposal-list data/thumos14_tag_test_proposal_list.txt \\
        --frame-root /data/frames --gpu-decode

``--gpu-decode`` uploads the frames' JPEG files and decodes, scales (GroupScale), crops and normalises them on the device; without
it the reference's PIL chain runs on the host.  Without ``--gpus`` and with ``-j`` at most 1 everything runs in this process on
``--device``; otherwise ``-j`` fresh worker processes are spawned, worker i on ``gpus[i % len(gpus)]``, and this process never
touches a GPU.  A worker that dies ends the run with its exit code in the message.
"""
import argparse
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NUM_CLASS = {"thumos14": 20, "activitynet1.2": 100}
STPP = {"thumos14": (1, 1, 1), "activitynet1.2": (1, 1, 1)}
MAX_WORKERS = 16


def parse(argv=None):
    p = argparse.ArgumentParser(description="SSN Testing Tool")
    p.add_argument("dataset", type=str, choices=sorted(NUM_CLASS))
    p.add_argument("modality", type=str, choices=["RGB", "Flow", "RGBDiff"])
    p.add_argument("weights", type=str)
    p.add_argument("save_scores", type=str)
    p.add_argument("--arch", type=str, default="BNInception")
    p.add_argument("--save_raw_scores", type=str, default=None)
    p.add_argument("--frame_interval", type=int, default=6)
    p.add_argument("--no_regression", action="store_true", default=False)
    p.add_argument("--max_num", type=int, default=-1)
    p.add_argument("--test_crops", type=int, default=10, choices=[1, 10])
    p.add_argument("--input_size", type=int, default=None)
    p.add_argument("-j", "--workers", default=1, type=int, metavar="N", help="worker processes (default: 1, in this process)")
    p.add_argument("--gpus", nargs="+", type=int, default=None)
    p.add_argument("--flow_pref", type=str, default="")
    p.add_argument("--proposal-list", required=True, help="the processed proposal list of the videos to test")
    p.add_argument("--frame-root", type=str, default="")
    p.add_argument("--tick_batch", type=int, default=32,
                   help="ticks per decoder / backbone call; with --gpu-decode the Huffman launch costs the same for any batch: use 256")
    p.add_argument("--gpu-decode", action="store_true", help="decode, scale and crop the frames on the device")
    p.add_argument("--device", type=str, default="cuda:0")
    args = p.parse_args(argv)
    if args.modality == "RGBDiff":
        raise NotImplementedError("RGBDiff testing: DenseTester has no RGBDiff input length")
    if args.workers > MAX_WORKERS:
        raise ValueError("at most {} workers, got {}".format(MAX_WORKERS, args.workers))
    return args


def load_videos(args):
    """The videos of the list in the reference's order (SSNDataSet in test mode) and the sampler that knows their ticks."""
    from action_detection_amd.proposal_sampling import ProposalSampler
    import numpy as np
    data_length = 1 if args.modality == "RGB" else 5
    return ProposalSampler(args.proposal_list, new_length=data_length, test_interval=args.frame_interval,
                           reg_stats=np.zeros((2, 2)))


class SSNVideoTester(object):
    """``tester(index) -> (video id, rel_props, act, comp, reg or None, output)`` as numpy arrays: the body of the reference's
    runner_func (ssn_test.py:55-96) for one video, on ``device``."""

    def __init__(self, args, device):
        import numpy as np
        import torch
        import action_detection_amd as pkg
        from action_detection_amd import test_data as TD
        from action_detection_amd import train_data as D
        from action_detection_amd.dense_test import DenseTester
        from action_detection_amd.ssn_models import SSN
        pkg.build()
        if torch.device(device).type == "cuda":
            # the library launches on torch's current stream of the tensors' device, and the default stream's handle (0) means "the
            # CURRENT device's null stream": the tester's device has to be the current one (ssn_test.py:56 does the same)
            torch.cuda.set_device(torch.device(device))
        num_class, stpp = NUM_CLASS[args.dataset], STPP[args.dataset]
        net = SSN(num_class, 2, 5, 2, args.modality, test_mode=True, base_model=args.arch, no_regression=args.no_regression,
                  stpp_cfg=stpp)
        checkpoint = torch.load(args.weights, map_location="cpu", weights_only=False)
        print("model epoch {} loss: {}".format(checkpoint.get("epoch"), checkpoint.get("best_loss")))
        net.load_state_dict({".".join(k.split(".")[1:]): v for k, v in checkpoint["state_dict"].items()})
        stats = checkpoint.get("reg_stats")
        stats = None if stats is None else np.asarray(stats.numpy() if torch.is_tensor(stats) else stats, dtype=np.float64)
        net.prepare_test_fc()
        net.to(device).eval()
        self.tester = DenseTester(net, num_class, stpp_cfg=stpp, stats=stats, tick_batch=args.tick_batch)
        self.sampler = load_videos(args)
        self.test_crops, self.tick_batch = args.test_crops, args.tick_batch
        input_size = net.input_size if args.input_size is None else args.input_size
        self.host_scaled_videos = 0
        self.host_decoded_files = 0             # files the device decoder handed to PIL (progressive, unsupported tables, ...)
        if args.gpu_decode:
            self.reader = D.CompressedFrameDirReader(args.frame_root, args.modality, args.flow_pref)
            self.transform = TD.DeviceTestChain(input_size, net.scale_size, net.input_mean, net.input_std, args.modality,
                                                args.test_crops, device)
        else:
            self.reader = D.FrameDirReader(args.frame_root, args.modality, args.flow_pref)
            self.transform = TD.host_test_chain(input_size, net.scale_size, net.input_mean, net.input_std, args.test_crops,
                                                roll=args.arch in ("BNInception", "InceptionV3"))
        self._batches = TD.test_frame_batches

    def __call__(self, index):
        import torch
        video = self.sampler.video_list[index]
        ticks, rel_props, prop_ticks, prop_scaling = self.sampler.test_ticks(video)
        before = getattr(self.transform, "host_scaled", 0)
        gen = self._batches(self.sampler, video, self.reader, self.transform, self.tick_batch)
        act, comp, reg, output = self.tester.score_video(gen, len(ticks), torch.from_numpy(prop_ticks),
                                                         torch.from_numpy(prop_scaling), num_crop=self.test_crops)
        self.host_scaled_videos += int(getattr(self.transform, "host_scaled", 0) > before)
        self.host_decoded_files = getattr(self.transform, "host_decoded", 0)
        return (video.id, rel_props, act.cpu().numpy(), comp.cpu().numpy(), None if reg is None else reg.cpu().numpy(),
                output.cpu().numpy())


def make_ssn_tester(args, device):
    return SSNVideoTester(args, device)


def worker_loop(make_tester, args, device, index_queue, result_queue):
    """One worker process: build the tester on ``device``, score the indices that arrive until the ``None`` that ends the run.
    Results are ``((video id, numpy arrays ...), host-scaled videos, host-decoded files)``, the counts those of this one video."""
    tester = make_tester(args, device)
    while True:
        index = index_queue.get()
        if index is None:
            return
        before = _host_counts(tester)
        rst = tester(index)
        after = _host_counts(tester)
        result_queue.put((rst, after[0] - before[0], after[1] - before[1]))


def _host_counts(tester):
    return getattr(tester, "host_scaled_videos", 0), getattr(tester, "host_decoded_files", 0)


def _progress(i, total, start):
    print('video {} done, total {}/{}, average {:.04f} sec/video'.format(i, i + 1, total, float(time.time() - start) / (i + 1)))


def run(args, n_videos, make_tester=make_ssn_tester, poll=0.5):
    """-> ({video id: (rel_props, act, comp, reg, output)}, (host-scaled videos, host-decoded files)) of the first ``n_videos``
    videos."""
    import queue
    out, host_scaled, host_decoded = {}, 0, 0
    start = time.time()
    if args.gpus is None and args.workers <= 1:
        tester = make_tester(args, args.device)
        for i in range(n_videos):
            rst = tester(i)
            out[rst[0]] = rst[1:]
            _progress(i, n_videos, start)
        return out, _host_counts(tester)

    import multiprocessing
    ctx = multiprocessing.get_context("spawn")      # fresh processes: each initialises its own GPU, this one none
    n_workers = max(1, args.workers)
    if n_workers > MAX_WORKERS:
        raise ValueError("at most {} workers, got {}".format(MAX_WORKERS, n_workers))
    devices = ["cuda:{}".format(g) for g in args.gpus] if args.gpus is not None else [args.device]
    index_queue, result_queue = ctx.Queue(), ctx.Queue()
    workers = [ctx.Process(target=worker_loop, args=(make_tester, args, devices[i % len(devices)], index_queue, result_queue),
                           daemon=True) for i in range(n_workers)]
    for w in workers:
        w.start()
    for i in range(n_videos):
        index_queue.put(i)
    for _ in workers:
        index_queue.put(None)

    def check_workers(done):
        dead = [(i, w.exitcode) for i, w in enumerate(workers) if not w.is_alive() and w.exitcode != 0]
        if dead:
            raise RuntimeError("worker {} died with exit code {}; {} of {} videos done".format(dead[0][0], dead[0][1], done, n_videos))

    try:
        done = 0
        while done < n_videos:
            # a dead worker took the index it held with it: the run cannot complete, so it ends now, not after the others have scored
            # everything that is left
            check_workers(done)
            try:
                rst, scaled, decoded = result_queue.get(timeout=poll)
            except queue.Empty:
                check_workers(done)
                if not any(w.is_alive() for w in workers) and result_queue.empty():
                    raise RuntimeError("the workers ended after {} of {} videos".format(done, n_videos))
                continue
            out[rst[0]] = rst[1:]
            host_scaled += scaled
            host_decoded += decoded
            _progress(done, n_videos, start)
            done += 1
        for w in workers:
            w.join(timeout=30)
    finally:
        for w in workers:
            if w.is_alive():
                w.terminate()
        for w in workers:
            w.join(timeout=10)
    return out, (host_scaled, host_decoded)


def main(argv=None, make_tester=make_ssn_tester):
    args = parse(argv)
    if make_tester is make_ssn_tester:
        import action_detection_amd as pkg
        pkg.build()                                  # once, before any worker starts (compiles; does not touch a GPU)
    n_videos = len(load_videos(args))
    if args.max_num > 0:
        n_videos = min(n_videos, args.max_num)
    out, (host_scaled, host_decoded) = run(args, n_videos, make_tester)
    if args.save_scores is not None:
        with open(args.save_scores, "wb") as f:
            pickle.dump({k: v[:-1] for k, v in out.items()}, f, pickle.HIGHEST_PROTOCOL)
    if args.save_raw_scores is not None:
        with open(args.save_raw_scores, "wb") as f:
            pickle.dump({k: v[-1] for k, v in out.items()}, f, pickle.HIGHEST_PROTOCOL)
    if args.gpu_decode:
        print("{} of {} videos were scaled with PIL on the host (frames more than 6x the scale size); {} files were decoded with PIL "
              "on the host (not baseline JPEG)".format(host_scaled, n_videos, host_decoded))
    return out


if __name__ == "__main__":
    main()
