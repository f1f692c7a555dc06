#!/usr/bin/env python
"""Measure JPEG encoding of the flow images: the parent's write path of tools/extract_flow.py (device-to-host copy of the raw
uint8 flow, then ``PIL.Image.save(quality=95)`` per image, on 1 and on 16 host threads) against ``--gpu-encode`` (csrc/jpeg_encode.hip,
then only the files' bytes come down), on the same images.

    python tools/bench_jpeg_encode.py --out profiles/jpeg_encode_measured.txt

Workloads: 32 gray 340 x 256 flow images (one pair_batch of 16) and 2000 of them, quality 95, taken from ``FlowExtractor`` on the seeded
synthetic clip of tools/bench_flow.py (the 2000 cycle through the images of ``--clip-pairs`` consecutive pairs), without and with
restart markers.  Device times are HIP events around each stage of warmed-up, repeated batches; end-to-end times are a host clock
around the whole write path, files included, alternating the versions, medians.  Nothing here is a pass/fail condition.
"""
import argparse
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_write(folder, flow_dev, quality, threads):
    """The parent's path: raw pixels over PCIe, PIL per image (``threads`` > 1: the same saves on a thread pool)."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    flow = flow_dev.cpu().numpy()
    os.makedirs(folder, exist_ok=True)

    def one(k):
        i, c = divmod(k, 2)
        Image.fromarray(flow[i, c]).save(os.path.join(folder, "flow_{}_{:05d}.jpg".format("xy"[c], i + 1)), quality=quality)
    if threads == 1:
        for k in range(2 * flow.shape[0]):
            one(k)
    else:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(one, range(2 * flow.shape[0]), chunksize=max(1, flow.shape[0] // (2 * threads))))
    return flow.size


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(flow, quality, restart, repeats, threads, tool, encoder):
    import torch
    n = 2 * flow.shape[0]
    tmp = tempfile.mkdtemp(prefix="bench_jpeg_encode_")
    res = dict(images=n, restart_blocks=restart)
    try:
        paths = {"pil_1": lambda d: host_write(d, flow, quality, 1), "pil_%d" % threads: lambda d: host_write(d, flow, quality, threads),
                 "device": lambda d: tool.write_flow_on_device(d, "flow_", flow, quality, encoder, restart)}
        times = {k: [] for k in paths}
        for r in range(repeats + 1):
            for name, fn in paths.items():
                d = os.path.join(tmp, name)
                shutil.rmtree(d, ignore_errors=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(d)
                torch.cuda.synchronize()
                if r:
                    times[name].append(1e3 * (time.perf_counter() - t0))
        for name in paths:
            res[name + "_ms"] = median(times[name])
            res[name + "_all_ms"] = [round(t, 2) for t in times[name]]
        if restart == 0:
            names = sorted(os.listdir(os.path.join(tmp, "device")))
            res["equal"] = names == sorted(os.listdir(os.path.join(tmp, "pil_1"))) and all(
                open(os.path.join(tmp, "device", f), "rb").read() == open(os.path.join(tmp, "pil_1", f), "rb").read() for f in names)
        res["file_bytes"] = sum(os.path.getsize(os.path.join(tmp, "device", f)) for f in os.listdir(os.path.join(tmp, "device")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res["raw_bytes_d2h"] = flow.numel()
    res["device_bytes_d2h"] = encoder.downloaded_bytes
    # the device part alone: events around each stage, then the two host reads
    images = flow.reshape(n, flow.shape[2], flow.shape[3])
    encoder.profile = []
    spans, reads = [], []
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(repeats + 1):
        start.record()
        batch = encoder.encode(images, quality=quality, restart_blocks=restart, as_bytes=False)
        end.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch.to_bytes()
        if r:
            spans.append(start.elapsed_time(end))
            reads.append(1e3 * (time.perf_counter() - t0))
        else:
            encoder.profile = []
    stages = {}
    for name, a, b in encoder.profile:
        stages.setdefault(name, []).append(a.elapsed_time(b))
    encoder.profile = None
    res["stages_ms"] = {k: median(v) for k, v in stages.items()}
    res["stream_span_ms"] = median(spans)
    res["read_back_ms"] = median(reads)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, nargs="+", default=[32, 2000])
    ap.add_argument("--clip-pairs", type=int, default=64)
    ap.add_argument("--restart-blocks", type=int, default=43, help="the second run's interval (43 MCUs: one block row of 340 x 256)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    import torch
    import action_detection_amd as pkg
    pkg.build()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode needs a HIP device: a CPU run says nothing about either path")
    from action_detection_amd.jpeg_encode import JpegEncoder
    from action_detection_amd.optical_flow import TVL1, FlowExtractor
    dev = torch.device("cuda:0")
    tool = _tool("extract_flow")
    frames = torch.from_numpy(_tool("bench_flow").synthetic_clip(args.clip_pairs + 1, 256, 340, seed=0)).to(dev)
    clip = FlowExtractor(TVL1(), pair_batch=16).extract(frames)          # uint8 [pairs, 2, 256, 340]
    encoder = JpegEncoder(dev)
    lines = ["JPEG encoding of flow images, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "gray 340 x 256, quality %d, from FlowExtractor on the seeded synthetic clip of tools/bench_flow.py (%d distinct pairs, cycled);"
             % (args.quality, args.clip_pairs),
             "%d timed repeats after a warm-up, the versions alternating, medians; end-to-end = the tool's write path, files included" % args.repeats,
             "parent path: raw uint8 flow to the host + PIL.Image.save per image; device path: csrc/jpeg_encode.hip, then lengths + bytes"]
    results = []
    for n in args.images:
        pairs = n // 2
        flow = clip[torch.arange(pairs, device=dev) % clip.shape[0]].contiguous()
        for restart in (0, args.restart_blocks):
            r = measure(flow, args.quality, restart, args.repeats if n <= 256 else max(2, args.repeats // 2), args.threads, tool, encoder)
            results.append(r)
            st = r["stages_ms"]
            dev_ms = sum(st.values())
            best_host = r["pil_%d_ms" % args.threads]
            bind = max(st, key=st.get)
            lines += ["",
                      "%d images, restart_blocks %d: %.1f KB per file%s" %
                      (n, restart, r["file_bytes"] / n / 1e3, ", files of the two paths byte-equal: %s" % r["equal"] if "equal" in r else ""),
                      "  parent, 1 thread    %9.2f ms = %7.0f images/s   (all: %s)" % (r["pil_1_ms"], n / r["pil_1_ms"] * 1e3, r["pil_1_all_ms"]),
                      "  parent, %2d threads  %9.2f ms = %7.0f images/s   (all: %s)" %
                      (args.threads, best_host, n / best_host * 1e3, r["pil_%d_all_ms" % args.threads]),
                      "  --gpu-encode        %9.2f ms = %7.0f images/s   (all: %s)" % (r["device_ms"], n / r["device_ms"] * 1e3, r["device_all_ms"]),
                      "    ratio to 1 thread %.2f x, to %d threads %.2f x -> the device path %s %d host threads" %
                      (r["pil_1_ms"] / r["device_ms"], args.threads, best_host / r["device_ms"],
                       "beats" if r["device_ms"] < best_host else "does NOT beat", args.threads),
                      "    device stages (events): " + " + ".join("%s %.3f" % (k, v) for k, v in st.items()) +
                      " = %.3f ms; stream span of encode() %.3f ms; the two host reads %.3f ms" % (dev_ms, r["stream_span_ms"], r["read_back_ms"]),
                      "    the stage that binds on the device: %s; of the end-to-end time the device stages are %.0f %%" %
                      (bind, 100 * dev_ms / r["device_ms"]),
                      "    PCIe, device to host: %d bytes raw (parent) against %d bytes (files + lengths): %.1f x fewer" %
                      (r["raw_bytes_d2h"], r["device_bytes_d2h"], r["raw_bytes_d2h"] / max(r["device_bytes_d2h"], 1))]
    lines += ["", "To repeat: timeout -k 10 900 python tools/bench_jpeg_encode.py --out profiles/jpeg_encode_measured.txt"]
    text = "\n".join(lines)
    print(text)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return results


if __name__ == "__main__":
    main()
