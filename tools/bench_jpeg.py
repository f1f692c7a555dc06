#!/usr/bin/env python
"""Measure JPEG decoding for the input pipeline: the host path (PIL on 16 threads, then a pinned upload of the decoded frames)
against the device path (upload of the files' scans, then csrc/jpeg.hip), on one training step's worth of frames.

    python tools/bench_jpeg.py --out profiles/jpeg_decode_measured.txt

Workloads: 288 RGB frames of 340 x 256, 4:2:0, quality 75 (one SSN step: 4 videos x 8 proposals x 9 snippets), and 2880 gray frames
of the same size (the Flow batch), all made with PIL from a seeded smooth-plus-noise picture.  Device times are HIP events around
warmed-up, repeated batches; host times are a host clock around work that ends in a device synchronise.
"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_MS = 13.9      # one training step of 288 frames (README)


def make_files(n, gray, quality=75, hw=(256, 340), seed=0):
    import numpy as np
    from PIL import Image
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    files = []
    for i in range(n):
        rs = np.random.RandomState(seed * 100003 + i)
        c = 1 if gray else 3
        ph = rs.uniform(0, 6.28, (c, 4))
        a = np.stack([128 + 60 * np.sin(xx / 23.0 + ph[k, 0]) * np.cos(yy / 17.0 + ph[k, 1]) + 30 * np.sin(xx / 5.0 + yy / 7.0 + ph[k, 2])
                      for k in range(c)], 2) + rs.normal(0, 6, (h, w, c))
        a = np.clip(a, 0, 255).astype(np.uint8)
        b = io.BytesIO()
        if gray:
            Image.fromarray(a[:, :, 0]).save(b, "JPEG", quality=quality)
        else:
            Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=2)
        files.append(b.getvalue())
    return files


def host_path(files, mode, device, threads, repeats):
    """PIL on `threads` threads into a pinned buffer, one upload, synchronise.  -> (ms per batch, bytes uploaded)"""
    import numpy as np
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    c = 3 if mode == "RGB" else 1
    with Image.open(io.BytesIO(files[0])) as im:
        w, h = im.size
    pinned = torch.empty((len(files), h, w, c), dtype=torch.uint8, pin_memory=True)
    view = pinned.numpy()
    dev = torch.empty_like(pinned, device=device)

    def one(i):
        with Image.open(io.BytesIO(files[i])) as im:
            view[i] = np.asarray(im.convert(mode)).reshape(h, w, c)
    with ThreadPoolExecutor(threads) as pool:
        times = []
        for r in range(repeats + 1):
            t0 = time.perf_counter()
            list(pool.map(one, range(len(files)), chunksize=max(1, len(files) // (4 * threads))))
            t1 = time.perf_counter()
            dev.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize(device)
            t2 = time.perf_counter()
            if r:
                times.append((t2 - t0, t1 - t0, t2 - t1))
    tot, dec, up = (1e3 * sum(t[k] for t in times) / len(times) for k in range(3))
    return dict(ms=tot, decode_ms=dec, upload_ms=up, bytes_h2d=pinned.numel(), bytes_d2h=0), dev


def device_path(files, mode, device, repeats):
    import torch
    from action_detection_amd.jpeg_decode import JpegDecoder
    dec = JpegDecoder(device)
    out = None
    for _ in range(2):
        out = dec.decode(files, mode, stack=True)
    torch.cuda.synchronize(device)
    # (a) everything, host clock: marker walk + tables + upload + the three launches, ending in a synchronise
    t0 = time.perf_counter()
    for _ in range(repeats):
        out = dec.decode(files, mode, stack=True)
    torch.cuda.synchronize(device)
    wall = 1e3 * (time.perf_counter() - t0) / repeats
    # (b) the host part alone: what a loader thread spends per batch before anything is enqueued
    t0 = time.perf_counter()
    for _ in range(repeats):
        from action_detection_amd.jpeg_decode import parse_jpeg
        headers = [parse_jpeg(f) for f in files]
        dec._out_off = [0]
        for h in headers:
            dec._out_off.append(dec._out_off[-1] + h.height * h.width * (3 if mode == "RGB" else 1))
        dec._plan(files, headers, 3 if mode == "RGB" else 1)
    host = 1e3 * (time.perf_counter() - t0) / repeats
    # (c) the device part: events around the upload and each launch
    dec.profile = []
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spans = []
    for _ in range(repeats):
        start.record()
        out = dec.decode(files, mode, stack=True)
        end.record()
        torch.cuda.synchronize(device)
        spans.append(start.elapsed_time(end))
    stages = {}
    for name, a, b in dec.profile:
        stages.setdefault(name, []).append(a.elapsed_time(b))
    dec.profile = None
    status = int(dec.status.abs().sum().item())
    res = dict(ms=wall, host_ms=host, stream_span_ms=sum(spans) / len(spans), bytes_h2d=dec.uploaded_bytes, bytes_d2h=0,
               fallbacks=dec.fallbacks, status_sum=status, launches=3)
    for name, v in stages.items():
        res[name + "_ms"] = sum(v) / len(v)
    res["device_ms"] = sum(res[k + "_ms"] for k in ("upload", "entropy", "idct", "pixels"))
    return res, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=288)
    ap.add_argument("--flow-frames", type=int, default=2880)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    import torch
    import action_detection_amd as pkg
    pkg.build()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg needs a HIP device: a CPU run says nothing about either path")
    lines = ["JPEG decoding for the input pipeline, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "340 x 256 frames, quality %d, made with PIL from a seeded smooth-plus-noise picture; %d repeats after warm-up" %
             (args.quality, args.repeats),
             "host path: PIL on %d threads into pinned memory + one upload; device path: upload of the scans + csrc/jpeg.hip" % args.threads]
    results = {}
    for label, n, gray, mode in (("RGB 4:2:0", args.frames, False, "RGB"), ("Flow gray", args.flow_frames, True, "L")):
        files = make_files(n, gray, args.quality)
        host, ref = host_path(files, mode, args.device, args.threads, max(2, args.repeats // 2))
        dev, out = device_path(files, mode, args.device, args.repeats)
        equal = bool(torch.equal(ref, out))
        results[label] = dict(frames=n, file_bytes=sum(map(len, files)), host=host, device=dev, equal=equal)
        fps = lambda ms: n / ms * 1e3
        lines += ["",
                  "%s: %d frames, %.1f KB per file, outputs of the two paths equal: %s (fallbacks %d, status %d)" %
                  (label, n, sum(map(len, files)) / n / 1e3, equal, dev["fallbacks"], dev["status_sum"]),
                  "  host path    %8.2f ms per batch = %7.0f frames/s   (PIL %.2f ms, upload %.2f ms; %d bytes to the device, 0 back)" %
                  (host["ms"], fps(host["ms"]), host["decode_ms"], host["upload_ms"], host["bytes_h2d"]),
                  "  device path  %8.2f ms per batch = %7.0f frames/s   host clock, marker walk + tables + upload + 3 launches, one thread" %
                  (dev["ms"], fps(dev["ms"])),
                  "    host part  %8.2f ms   (marker walk and table building, Python, one thread)" % dev["host_ms"],
                  "    device     %8.2f ms = %7.0f frames/s   upload %.3f + entropy %.3f + idct %.3f + pixels %.3f ms (events per stage)" %
                  (dev["device_ms"], fps(dev["device_ms"]), dev["upload_ms"], dev["entropy_ms"], dev["idct_ms"], dev["pixels_ms"]),
                  "    %d bytes to the device (%.1f x fewer), 0 back" % (dev["bytes_h2d"], host["bytes_h2d"] / max(dev["bytes_h2d"], 1))]
        if not gray:
            per_step = dev["device_ms"] * 288.0 / n
            lines.append("  one step's 288 frames per %.1f ms: device part %.2f ms -> %s; host part %.2f ms on one thread -> %s" %
                         (STEP_MS, per_step, "keeps up" if per_step < STEP_MS else "does NOT keep up",
                          dev["host_ms"] * 288.0 / n, "keeps up" if dev["host_ms"] * 288.0 / n < STEP_MS else "does NOT keep up"))
            lines.append("  host path for the same 288 frames: %.2f ms -> %s" %
                         (host["ms"] * 288.0 / n, "keeps up" if host["ms"] * 288.0 / n < STEP_MS else "does NOT keep up"))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return results


if __name__ == "__main__":
    main()
