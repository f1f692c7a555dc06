#!/usr/bin/env python
"""Measure the test-time input chains of tools/test_ssn.py against what the tester consumes.

    python tools/bench_test_input.py --out profiles/test_input_measured.txt

One tick = one RGB frame file of 340 x 256 -> its 10 crops as normalised fp32.  Shape (a), BNInception: no resize (the short side is
scale_size = 256), 10 x 224^2.  Shape (b), Inception-v3: GroupScale(341) -> 452 x 341, 10 x 299^2.  Per shape:

* host chain: PIL decode + GroupOverSample + Stack + ToTorchFormatTensor + GroupNormalize on ``--threads`` threads (the reference's
  batches of 4 ticks), into pinned memory, one upload per ``--tick-batch`` ticks, synchronise;
* device chain (``--gpu-decode``): upload of the files' scans, JpegDecoder, ``ssn_frames_scale``, the ten-crop launch, synchronise;
* the tester's own consumption rate: tools/bench_dense_test.py for that backbone, run as a child process in the same session;
* kernel cost at shape (b): device events around ``ssn_frames_scale`` alone and around the ten-crop launch on pre-scaled frames,
  with the bytes each needs computed from the shapes.

Rates are ticks/s from a host clock around work that ends in a device synchronise, after warm-up; each is the median of
``--repeats`` windows with the extremes next to it.
"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = (("a", "BNInception", 224, 256), ("b", "InceptionV3", 299, 341))
MEAN, STD = [104, 117, 128], [1]
DRIVER_TICK_BATCH = 32      # the default of tools/test_ssn.py --tick_batch


def make_files(n, quality=75, hw=(256, 340), seed=0):
    """Seeded smooth-plus-noise pictures as 4:2:0 JPEG files (the files tools/bench_jpeg.py measures)."""
    import numpy as np
    from PIL import Image
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    files = []
    for i in range(n):
        rs = np.random.RandomState(seed * 100003 + i)
        ph = rs.uniform(0, 6.28, (3, 4))
        a = np.stack([128 + 60 * np.sin(xx / 23.0 + ph[k, 0]) * np.cos(yy / 17.0 + ph[k, 1]) + 30 * np.sin(xx / 5.0 + yy / 7.0 + ph[k, 2])
                      for k in range(3)], 2) + rs.normal(0, 6, (h, w, 3))
        b = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(b, "JPEG", quality=quality, subsampling=2)
        files.append(b.getvalue())
    return files


def stats(values):
    v = sorted(values)
    return dict(median=v[len(v) // 2], lo=v[0], hi=v[-1], n=len(v))


def host_chain_rate(files, crop, scale, device, threads, tick_batch, repeats):
    """-> ticks/s statistics, and the last batch on the device (for the equality check)."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from action_detection_amd import transforms as T
    chain = T.Compose([T.GroupOverSample(crop, scale), T.Stack(roll=True), T.ToTorchFormatTensor(div=False), T.GroupNormalize(MEAN, STD)])
    n = len(files)
    pinned = torch.empty((10, tick_batch, 3, crop, crop), dtype=torch.float32, pin_memory=True)
    dev = torch.empty((10, tick_batch, 3, crop, crop), dtype=torch.float32, device=device)

    def four_ticks(t0):
        ims = [Image.open(io.BytesIO(files[t])).convert("RGB") for t in range(t0, t0 + 4)]
        out = chain(ims).view(10, 4, 3, crop, crop)                 # crop-major, as the reference's generator yields it
        k = t0 % tick_batch
        pinned[:, k:k + 4].copy_(out)
    rates = []
    with ThreadPoolExecutor(threads) as pool:
        for r in range(repeats + 1):
            t0 = time.perf_counter()
            for b in range(0, n, tick_batch):
                list(pool.map(four_ticks, range(b, b + tick_batch, 4)))
                dev.copy_(pinned, non_blocking=True)
                torch.cuda.synchronize(device)                      # (the one staging buffer is reused by the next batch)
            if r:
                rates.append(n / (time.perf_counter() - t0))
    return stats(rates), dev.reshape(-1, crop, crop)


def device_chain_rate(files, crop, scale, device, tick_batch, repeats):
    import torch
    from action_detection_amd.test_data import DeviceTestChain
    chain = DeviceTestChain(crop, scale, MEAN, STD, "RGB", 10, device)
    n = len(files)
    out = None
    rates = []
    for r in range(repeats + 2):
        t0 = time.perf_counter()
        for b in range(0, n, tick_batch):
            out = chain(files[b:b + tick_batch])
        torch.cuda.synchronize(device)
        if r > 1:
            rates.append(n / (time.perf_counter() - t0))
    assert chain.host_scaled == 0 and chain.decoder.fallbacks == 0
    return stats(rates), out


def decoder_stages(files, crop, scale, device, tick_batch, repeats):
    """Device events around the decoder's upload and three launches inside the chain -> {stage: ms per batch of ``tick_batch``}."""
    import torch
    from action_detection_amd.test_data import DeviceTestChain
    chain = DeviceTestChain(crop, scale, MEAN, STD, "RGB", 10, device)
    chain(files[:tick_batch])
    torch.cuda.synchronize(device)
    chain.decoder.profile = []
    for _ in range(repeats):
        chain(files[:tick_batch])
    torch.cuda.synchronize(device)
    stages = {}
    for name, a, b in chain.decoder.profile:
        stages.setdefault(name, []).append(a.elapsed_time(b))
    chain.decoder.profile = None
    return {k: sorted(v)[len(v) // 2] for k, v in stages.items()}


def event_ms(fn, device, launches, windows):
    """ms per call: ``windows`` event spans of ``launches`` back-to-back calls each, after a warm-up window."""
    import torch
    out = []
    for w in range(windows + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize(device)
        if w:
            out.append(a.elapsed_time(b) / launches)
    return stats(out)


def kernel_cost(files, device, tick_batch, windows):
    """Shape (b): ssn_frames_scale alone and the ten-crop launch on pre-scaled frames, per batch of ``tick_batch`` frames."""
    import torch
    from action_detection_amd import kernels as K
    from action_detection_amd.input_pipeline import GpuFrameTransform, scaled_size
    from action_detection_amd.jpeg_decode import JpegDecoder
    frames = JpegDecoder(device).decode(files[:tick_batch], "RGB", stack=True)
    n, h, w, c = frames.shape
    ow, oh = scaled_size(w, h, 341)
    dst = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=device)
    tf = GpuFrameTransform(299, MEAN, STD, roll=True, device=device)
    scaled = K.frames_scale(frames, (oh, ow), dst=dst)
    scale_ms = event_ms(lambda: K.frames_scale(frames, (oh, ow), dst=dst), device, 50, windows)
    crop_ms = event_ms(lambda: tf.oversample(scaled), device, 20, windows)
    scale_bytes = n * (h * w * c + oh * ow * c)
    crop_bytes = n * (oh * ow * c + 10 * c * 299 * 299 * 4)
    return dict(frames=n, src="%d x %d" % (w, h), scaled="%d x %d" % (ow, oh), scale_ms=scale_ms, crop_ms=crop_ms,
                scale_bytes=scale_bytes, crop_bytes=crop_bytes,
                scale_gbps=scale_bytes / scale_ms["median"] / 1e6, crop_gbps=crop_bytes / crop_ms["median"] / 1e6,
                written_ratio=(10 * c * 299 * 299 * 4) / float(oh * ow * c))


def tester_rate(arch, timeout):
    """tools/bench_dense_test.py in a child process -> frames/s (crops counted) on synthetic device tensors."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_dense_test.py"), "--arch", arch, "--cpu-ticks", "0", "--videos", "2"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    if p.returncode != 0:
        raise RuntimeError("bench_dense_test.py --arch %s ended with %d:\n%s" % (arch, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])["value"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--tick-batch", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--no-tester", action="store_true", help="skip the dense-test child processes")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if args.ticks % args.tick_batch or args.tick_batch % 4:
        raise SystemExit("--ticks must be a multiple of --tick-batch, --tick-batch of 4")

    import torch
    import action_detection_amd as pkg
    pkg.build()
    if not torch.cuda.is_available():
        raise SystemExit("bench_test_input needs a HIP device: a CPU run says nothing about either chain")
    torch.set_num_threads(1)            # the host chain's parallelism is its thread pool
    files = make_files(args.ticks, args.quality)
    lines = ["Test-time input chains of tools/test_ssn.py, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "%d ticks = RGB files of 340 x 256, 4:2:0, quality %d, %.1f KB per file; one tick -> 10 crops; batches of %d ticks" %
             (args.ticks, args.quality, sum(map(len, files)) / len(files) / 1e3, args.tick_batch),
             "rates: host clock ending in a device synchronise, median [lowest .. highest] of %d windows after warm-up" % args.repeats,
             "host chain: PIL decode + GroupOverSample + Stack + ToTorchFormatTensor + GroupNormalize on %d threads, pinned upload" %
             args.threads,
             "device chain: upload of the scans + csrc/jpeg.hip + ssn_frames_scale + ssn_frames_crop_normalize, one host thread"]
    results = {}
    for key, arch, crop, scale in SHAPES:
        host, ref = host_chain_rate(files, crop, scale, args.device, args.threads, args.tick_batch, args.repeats)
        dev, out = device_chain_rate(files, crop, scale, args.device, args.tick_batch, args.repeats)
        equal = bool(torch.equal(ref, out))
        dev_all, _ = device_chain_rate(files, crop, scale, args.device, len(files), args.repeats)
        dev_dflt, _ = device_chain_rate(files, crop, scale, args.device, DRIVER_TICK_BATCH, args.repeats)
        stages = decoder_stages(files, crop, scale, args.device, args.tick_batch, args.repeats)
        need = None if args.no_tester else tester_rate(arch, 600) / 10.0
        results[key] = dict(arch=arch, crop=crop, scale_size=scale, host=host, device=dev, device_one_batch=dev_all, device_driver_default=dev_dflt,
                            decoder_stages_ms=stages,
                            equal=equal, tester_ticks_per_s=need)
        fmt = lambda s: "%8.0f ticks/s [%.0f .. %.0f]" % (s["median"], s["lo"], s["hi"])      # noqa: E731
        lines += ["", "shape (%s) %s: 340 x 256 -> GroupScale(%d) -> 10 x %d^2; last batches of the two chains equal: %s" %
                  (key, arch, scale, crop, equal),
                  "  host chain    " + fmt(host),
                  "  device chain  " + fmt(dev) + "   (%.1f x the host chain)" % (dev["median"] / host["median"]),
                  "    per batch of %d: %.2f ms, of which the decoder's events: %s ms" %
                  (args.tick_batch, 1e3 * args.tick_batch / dev["median"],
                   " + ".join("%s %.2f" % (k, stages[k]) for k in ("upload", "entropy", "idct", "pixels") if k in stages)),
                  "  device chain, all %d ticks in one batch  " % len(files) + fmt(dev_all),
                  "  device chain, %d ticks per batch (the driver's default --tick_batch)  " % DRIVER_TICK_BATCH + fmt(dev_dflt)]
        if need is not None:
            lines.append("  the tester consumes %8.0f ticks/s (tools/bench_dense_test.py --arch %s: %.0f frames/s on synthetic device tensors)" %
                         (need, arch, need * 10))
            for name, s in (("host chain", host), ("device chain", dev), ("device chain, one batch of %d" % len(files), dev_all),
                            ("device chain, %d per batch" % DRIVER_TICK_BATCH, dev_dflt)):
                lines.append("  %-13s %s the tester fed (%.2f x its rate)" %
                             (name, "KEEPS" if s["median"] >= need else "does NOT keep", s["median"] / need))
    lines += ["", "these are stand-alone RATES of a producer and a consumer, not an overlapped pipeline: tools/test_ssn.py runs the chain and the",
              "tester one after the other on one stream, so the time of a video there is the SUM of the two"]
    kc = kernel_cost(files, args.device, args.tick_batch, args.repeats)
    results["kernel_cost"] = kc
    lines += ["", "kernel cost at shape (b), %d frames per launch, device events (median [lowest .. highest] ms per launch):" % kc["frames"],
              "  ssn_frames_scale %s -> %s   %.4f ms [%.4f .. %.4f], %.1f KB read + written per frame -> %.0f GB/s" %
              (kc["src"], kc["scaled"], kc["scale_ms"]["median"], kc["scale_ms"]["lo"], kc["scale_ms"]["hi"],
               kc["scale_bytes"] / kc["frames"] / 1e3, kc["scale_gbps"]),
              "  ten-crop launch on %s frames        %.4f ms [%.4f .. %.4f], %.1f KB read + written per frame -> %.0f GB/s" %
              (kc["scaled"], kc["crop_ms"]["median"], kc["crop_ms"]["lo"], kc["crop_ms"]["hi"], kc["crop_bytes"] / kc["frames"] / 1e3,
               kc["crop_gbps"]),
              "  the crop launch writes %.1f x what the scale launch writes; scale / crop time = %.3f" %
              (kc["written_ratio"], kc["scale_ms"]["median"] / kc["crop_ms"]["median"])]
    text = "\n".join(lines)
    print(text)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return results


if __name__ == "__main__":
    main()
