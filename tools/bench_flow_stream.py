#!/usr/bin/env python
"""Measure the on-the-fly Flow input on one MI355X: one JSON line, and with --out the text of profiles/flow_stream_measured.txt.

    python tools/bench_flow_stream.py [--pairs 288] [--repeats 7] [--chunk-batches 64,16,1] [--out profiles/flow_stream_measured.txt]

One seeded synthetic clip at 340 x 256 (tools/bench_flow.py's).  Two steps, each a fresh process under its own ``timeout``; a step
that fails ends the run:

  a  ``jpeg_encode.roundtrip_gray`` alone on 2 x PAIRS and 20 x PAIRS quantised flow images against
     ``JpegEncoder.encode(as_bytes=True)`` + ``JpegDecoder.decode(mode="L")`` on the same images (outputs compared)
  b  the flow frames of one video delivered through ``flow_stream.FlowStreamSource`` (RGB files -> device decode -> TV-L1 ->
     quantise -> round trip -> device tensors, a cold cache every repeat) against the file chain: ``tools/extract_flow.py``'s
     --gpu-decode --gpu-encode path into a temporary directory, then ``CompressedFrameDirReader`` + ``JpegDecoder`` (outputs compared);
     what of (b) is TV-L1 itself, from frames that are resident; and the source again at every RGB read size of --chunk-batches

Medians of REPEATS alternating repeats with min and max; host clock around work that ends in a device synchronise; one warm-up of
each version first.  Nothing is gated on these times.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STEP_SECONDS = {"a": 300, "b": 420}
REQUEST = 160      # flow frames per request of step b: a tick batch of 32 ticks of 5 frames


def stats(ts):
    import numpy as np
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def alternate(versions, repeats):
    """versions: {name: fn() -> result}; a warm-up of each, then `repeats` rounds alternating them -> ({name: stats}, {name: result})"""
    import torch

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    results = {name: timed(fn)[1] for name, fn in versions.items()}
    times = {name: [] for name in versions}
    for _ in range(repeats):
        for name, fn in versions.items():
            times[name].append(timed(fn)[0])
    return {name: stats(ts) for name, ts in times.items()}, results


def setup(a):
    import torch
    import action_detection_amd as pkg
    import bench_flow
    from action_detection_amd.optical_flow import FlowExtractor
    assert torch.cuda.is_available(), "bench_flow_stream.py measures on the GPU; there is nothing to measure without one"
    pkg.build()
    clip = bench_flow.synthetic_clip(a.pairs + 1, a.height, a.width, seed=0)
    return torch.device("cuda:0"), clip, FlowExtractor(pair_batch=a.pair_batch)


def step_a(a):
    import torch
    from action_detection_amd.jpeg_decode import JpegDecoder
    from action_detection_amd.jpeg_encode import JpegEncoder, roundtrip_gray
    dev, clip, extractor = setup(a)
    flow = extractor.extract(torch.from_numpy(clip).to(dev))                      # uint8 [pairs, 2, H, W]
    small = flow.reshape(-1, a.height, a.width).contiguous()
    out = {}
    for name, images in (("small", small), ("large", small.repeat(10, 1, 1))):
        enc, dec = JpegEncoder(dev), JpegDecoder(dev)
        t, res = alternate({"roundtrip": lambda: roundtrip_gray(images, a.quality),
                            "codec": lambda: dec.decode(enc.encode(images, quality=a.quality, as_bytes=True), mode="L", stack=True)}, a.repeats)
        equal = bool(torch.equal(res["roundtrip"], res["codec"].reshape(res["roundtrip"].shape)))
        out[name] = {"images": int(images.shape[0]), "roundtrip": t["roundtrip"], "codec": t["codec"], "equal": equal}
        del res
    return out


def step_b(a):
    import torch
    from PIL import Image
    import extract_flow
    from action_detection_amd.flow_stream import FlowStreamSource
    from action_detection_amd.jpeg_decode import JpegDecoder
    from action_detection_amd.jpeg_encode import JpegEncoder, roundtrip_gray
    from action_detection_amd.train_data import CompressedFrameDirReader
    dev, clip, extractor = setup(a)
    t_frames = a.pairs + 1
    numbers = list(range(1, a.pairs + 1))
    with tempfile.TemporaryDirectory() as tmp:
        rgb_root, flow_root = os.path.join(tmp, "rgb"), os.path.join(tmp, "flow")
        os.makedirs(os.path.join(rgb_root, "video"))
        for i, f in enumerate(clip):
            Image.fromarray(f).save(os.path.join(rgb_root, "video", "img_%05d.jpg" % (i + 1)), quality=90)
        rgb_decoder, flow_decoder, encoder = JpegDecoder(dev), JpegDecoder(dev), JpegEncoder(dev)

        chunks = [int(c) for c in a.chunk_batches.split(",")]

        def on_the_fly(chunk_batches=chunks[0]):
            src = FlowStreamSource(CompressedFrameDirReader(rgb_root, "RGB"), {"video": t_frames}, extractor, quality=a.quality, device=dev,
                                   chunk_batches=chunk_batches)
            return torch.cat([src("video", numbers[k:k + REQUEST]) for k in range(0, a.pairs, REQUEST)])

        def file_chain():
            frames = extract_flow.load_frames_on_device(os.path.join(rgb_root, "video"), t_frames, rgb_decoder)
            extract_flow.write_flow_on_device(os.path.join(flow_root, "video"), "flow_", extractor.extract(frames), a.quality, encoder)
            reader = CompressedFrameDirReader(flow_root, "Flow", "flow_")
            return torch.cat([flow_decoder.decode(reader("video", numbers[k:k + REQUEST]), "L", stack=True) for k in range(0, a.pairs, REQUEST)])
        t, res = alternate({"on_the_fly": on_the_fly, "file_chain": file_chain}, a.repeats)
        equal = bool(torch.equal(res["on_the_fly"], res["file_chain"].reshape(res["on_the_fly"].shape)))
        # the same source with other RGB read sizes (chunk_batches x pair_batch + 1 files a decoder call)
        sweep, _ = alternate({str(c): (lambda c=c: on_the_fly(c)) for c in chunks}, a.repeats)
        few = a.pair_batch + 1
        # the parts of on_the_fly, each alone: RGB files -> device frames; TV-L1 + quantiser from resident frames; the round trip
        frames = extract_flow.load_frames_on_device(os.path.join(rgb_root, "video"), t_frames, rgb_decoder)
        quantised = extractor.extract(frames)
        parts, _ = alternate({"rgb_decode": lambda: extract_flow.load_frames_on_device(os.path.join(rgb_root, "video"), t_frames, rgb_decoder),
                              "rgb_decode_few": lambda: extract_flow.load_frames_on_device(os.path.join(rgb_root, "video"), few, rgb_decoder),
                              "tvl1": lambda: extractor.extract(frames),
                              "roundtrip": lambda: roundtrip_gray(quantised.view(-1, a.height, a.width), a.quality),
                              "encode_write": lambda: extract_flow.write_flow_on_device(os.path.join(flow_root, "video"), "flow_", quantised,
                                                                                       a.quality, encoder),
                              "read_decode": lambda: [flow_decoder.decode(CompressedFrameDirReader(flow_root, "Flow", "flow_")(
                                  "video", numbers[k:k + REQUEST]), "L", stack=True) for k in range(0, a.pairs, REQUEST)]}, a.repeats)
        flow_bytes = sum(os.path.getsize(os.path.join(flow_root, "video", n)) for n in os.listdir(os.path.join(flow_root, "video")))
    return {"pairs": a.pairs, "on_the_fly": t["on_the_fly"], "file_chain": t["file_chain"], "equal": equal, "parts": parts,
            "sweep": sweep, "chunk_batches": chunks, "few": few, "flow_files": 2 * a.pairs, "flow_file_bytes": int(flow_bytes)}


def commit_name():
    import bench_flow
    return bench_flow.commit_name()


def fmt(s, scale=1e3, unit="ms"):
    return "median %.3f %s (min %.3f, max %.3f)" % (s["median"] * scale, unit, s["min"] * scale, s["max"] * scale)


def report(r):
    a, b = r["a"], r["b"]
    lines = ["On-the-fly Flow input: tools/bench_flow_stream.py on one {device} (host {host}), commit measured: {commit}.".format(**r),
             "Method: every step a fresh process; a warm-up of each version, then {repeats} rounds alternating the versions; medians with".format(**r),
             "min and max; host clock around work that ends in a device synchronise.  No profiler attached.  Input: the seeded synthetic",
             "clip of tools/bench_flow.py, {pairs} consecutive pairs at {w} x {h}, TV-L1 defaults, pair_batch {pair_batch}, JPEG quality {quality}.".format(**r),
             "", "a. The round trip alone: roundtrip_gray (one launch) against JpegEncoder.encode(as_bytes=True) + JpegDecoder.decode(mode=\"L\")",
             "   on the same quantised flow images (the files go to the host and come back, as the decoder takes host bytes):"]
    for name in ("small", "large"):
        x = a[name]
        lines += ["   {} images: roundtrip_gray {}".format(x["images"], fmt(x["roundtrip"])),
                  "   {}         encode + decode {}".format(" " * len(str(x["images"])), fmt(x["codec"])),
                  "   {}         ratio of medians {:.1f} x; outputs bit-equal: {}".format(" " * len(str(x["images"])),
                                                                                    x["codec"]["median"] / x["roundtrip"]["median"], x["equal"])]
    p = b["parts"]
    fly, chain = b["on_the_fly"]["median"], b["file_chain"]["median"]
    lines += ["", "b. The {} flow frames of one video ({} RGB files on disk -> uint8 flow images on the device):".format(2 * b["pairs"], b["pairs"] + 1),
              "   FlowStreamSource (cold cache)                 {}  = {:.0f} pairs/s".format(fmt(b["on_the_fly"]), b["pairs"] / fly),
              "   file chain (extract + encode + write + read + decode)  {}  = {:.0f} pairs/s".format(fmt(b["file_chain"]), b["pairs"] / chain),
              "   ratio of medians {:.2f} x; outputs bit-equal: {}".format(chain / fly, b["equal"]),
              "   the parts, each alone on the same data:",
              "     RGB files -> frames on the device          {}".format(fmt(p["rgb_decode"])),
              "       the first {} of them alone, one decoder call   {}".format(b["few"], fmt(p["rgb_decode_few"])),
              "     TV-L1 + quantiser from resident frames     {}  ({:.0f} % of the on-the-fly median)".format(fmt(p["tvl1"]), 100 * p["tvl1"]["median"] / fly),
              "     roundtrip_gray of the {} images            {}  ({:.1f} %)".format(2 * b["pairs"], fmt(p["roundtrip"]), 100 * p["roundtrip"]["median"] / fly),
              "     file chain only: encode + write {} files ({} bytes)   {}".format(b["flow_files"], b["flow_file_bytes"], fmt(p["encode_write"])),
              "     file chain only: read + decode them        {}".format(fmt(p["read_decode"])),
              "   The file chain's median minus the on-the-fly median is {:.1f} ms: what the skipped encode, file traffic and decode cost, less".format((chain - fly) * 1e3),
              "   the round trip that replaces them.",
              "   The source at other RGB read sizes (--chunk-batches; chunk_batches x pair_batch + 1 files a decoder call; the first is the one above,",
              "   measured again in alternation with the others):"] + [
              "     chunk_batches {:>3} ({:>4} files a call, {:>2} calls)   {}".format(
                  c, c * r["pair_batch"] + 1, -(-b["pairs"] // (c * r["pair_batch"])), fmt(b["sweep"][str(c)])) for c in b["chunk_batches"]] + [
              "", "Nothing here is a pass/fail condition.",
              "To repeat: python tools/bench_flow_stream.py --out profiles/flow_stream_measured.txt", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=288)
    ap.add_argument("--pair-batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=340)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-batches", type=str, default="64,16,1",
                    help="FlowStreamSource(chunk_batches=) values of step b, comma-separated; the first is compared with the file chain")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--step", type=str, default=None, choices=sorted(STEP_SECONDS), help="(internal) run one step and print its JSON")
    a = ap.parse_args()
    if a.step:
        import torch
        out = {"a": step_a, "b": step_b}[a.step](a)
        out["device"] = torch.cuda.get_device_name(0)
        print("STEP " + json.dumps(out))
        return 0
    # the parent never touches the GPU: every step is a child of its own, under its own time limit
    r = {"what": "on-the-fly Flow input on one MI355X", "host": socket.gethostname(), "commit": commit_name(), "repeats": a.repeats,
         "pairs": a.pairs, "pair_batch": a.pair_batch, "h": a.height, "w": a.width, "quality": a.quality}
    for step in sorted(STEP_SECONDS):
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--pairs", str(a.pairs),
               "--pair-batch", str(a.pair_batch), "--height", str(a.height), "--width", str(a.width), "--quality", str(a.quality), "--repeats",
               str(a.repeats), "--chunk-batches", a.chunk_batches]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        line = [ln for ln in done.stdout.splitlines() if ln.startswith("STEP ")]
        if done.returncode != 0 or not line:
            print("step %s failed (exit status %d); nothing further is run" % (step, done.returncode), file=sys.stderr)
            return done.returncode or 1
        r[step] = json.loads(line[-1][5:])
    r["device"] = r["a"].pop("device")
    r["b"].pop("device")
    print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
