#!/usr/bin/env python
"""Measure lossless JPEG transcoding (jpeg_transcode.JpegTranscoder) and what it is for: ``JpegDecoder.decode`` on the files it
writes against the files it read.

    python tools/bench_jpeg_transcode.py --out profiles/jpeg_transcode_measured.txt

Workloads (the synthetic frames of tools/bench_jpeg.py): 288 RGB frames of 340 x 256, 4:2:0, quality 75 (one SSN step) and 2880 gray
flow frames of the same size, quality 95, all written by PIL without restart markers.  Reported per workload:
  (a) the transcoding of one batch at ``restart_rows=1``: host clock around the whole call (files in, files out), and HIP events around
      every stage it enqueues;
  (b) ``JpegDecoder.decode`` on the ORIGINAL files and on the files transcoded at ``restart_rows`` 1, 2 and 4: the same decoder, the
      same pixels (checked with ``torch.equal``), only the input files differ.  The four variants alternate inside every repeat;
      medians of the entropy stage (events) and of the whole call's span on the stream;
  (c) the growth of the files in percent.
Nothing here is a pass/fail condition.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = (1, 2, 4)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def stage_medians(profile, calls):
    """{stage: median ms} of a profile list that holds `calls` calls"""
    stages = {}
    for name, a, b in profile:
        stages.setdefault(name, []).append(a.elapsed_time(b))
    return {name: median(v) for name, v in stages.items() if len(v) == calls}


def measure_transcode(files, rows, device, repeats):
    import torch
    from action_detection_amd.jpeg_transcode import JpegTranscoder
    t = JpegTranscoder(device)
    for _ in range(2):
        out = t.transcode(files, restart_rows=rows)
    assert t.skipped == [], t.skipped[:3]
    torch.cuda.synchronize(device)
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        t.transcode(files, restart_rows=rows)
        wall.append(1e3 * (time.perf_counter() - t0))      # (the call ends in the host reads of the files)
    t.profile = []
    spans = []
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        start.record()
        t.transcode(files, restart_rows=rows, as_bytes=False)
        end.record()
        torch.cuda.synchronize(device)
        spans.append(start.elapsed_time(end))
    stages = stage_medians(t.profile, repeats)
    t.profile = None
    return out, dict(wall_ms=median(wall), stream_span_ms=median(spans), stages_ms=stages)


def measure_decode(variants, mode, device, repeats):
    """variants: {label: files}.  -> {label: dict}, and whether every variant decoded to the pixels of the first"""
    import torch
    from action_detection_amd.jpeg_decode import JpegDecoder, parse_jpeg
    decs = {label: JpegDecoder(device) for label in variants}
    ref, equal = None, True
    for label, files in variants.items():
        for _ in range(2):
            out = decs[label].decode(files, mode, stack=True)
        torch.cuda.synchronize(device)
        assert decs[label].fallbacks == 0 and int(decs[label].status.abs().sum().item()) == 0, label
        if ref is None:
            ref = out.clone()
        else:
            equal = equal and bool(torch.equal(ref, out))
    spans = {label: [] for label in variants}
    walls = {label: [] for label in variants}
    for d in decs.values():
        d.profile = []
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        for label, files in variants.items():      # (alternating: a drift of the machine hits every variant alike)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            start.record()
            decs[label].decode(files, mode, stack=True)
            end.record()
            torch.cuda.synchronize(device)
            walls[label].append(1e3 * (time.perf_counter() - t0))
            spans[label].append(start.elapsed_time(end))
    res = {}
    for label, files in variants.items():
        stages = stage_medians(decs[label].profile, repeats)
        res[label] = dict(entropy_ms=stages["entropy"], device_ms=sum(stages.values()), stages_ms=stages, stream_span_ms=median(spans[label]),
                          wall_ms=median(walls[label]), units=sum(len(parse_jpeg(f).units) for f in files), file_bytes=sum(map(len, files)))
    return res, equal


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=288)
    ap.add_argument("--flow-frames", type=int, default=2880)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)

    import torch
    import action_detection_amd as pkg
    pkg.build()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_transcode needs a HIP device: a CPU run says nothing about either path")
    make_files = _tool("bench_jpeg").make_files
    lines = ["Lossless JPEG transcoding and decoding of its output, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "340 x 256 frames made with PIL (no restart markers) from a seeded smooth-plus-noise picture; medians of %d repeats after "
             "warm-up" % args.repeats,
             "decode: the same JpegDecoder build on every variant, variants alternating inside every repeat; only the files differ"]
    results = {}
    for label, n, gray, mode, quality in (("RGB 4:2:0 q75", args.frames, False, "RGB", 75), ("Flow gray q95", args.flow_frames, True, "L", 95)):
        files = make_files(n, gray, quality)
        variants = {"original": files}
        transcode = None
        for rows in ROWS:
            out, tr = measure_transcode(files, rows, args.device, args.repeats if rows == 1 else 1)
            variants["restart_rows=%d" % rows] = out
            if rows == 1:
                transcode = tr
        dec, equal = measure_decode(variants, mode, args.device, args.repeats)
        results[label] = dict(frames=n, transcode=transcode, decode=dec, pixels_equal=equal)
        base = dec["original"]
        st = transcode["stages_ms"]
        lines += ["",
                  "%s: %d frames, %.1f KB per file; every variant decodes to the pixels of the original: %s" %
                  (label, n, base["file_bytes"] / n / 1e3, equal),
                  "  (a) transcode at restart_rows=1: %8.2f ms per batch, host clock, files in -> files out (%.0f frames/s)" %
                  (transcode["wall_ms"], n / transcode["wall_ms"] * 1e3),
                  "      on the stream %8.2f ms: %s" %
                  (transcode["stream_span_ms"], " + ".join("%s %.3f" % (k, st[k]) for k in
                                                            ("upload", "entropy", "layout", "count", "scan", "pack", "assemble") if k in st)),
                  "  (b) JpegDecoder.decode                units   entropy ms   all stages ms   span on the stream ms   host clock ms"]
        for name, d in dec.items():
            lines.append("      %-22s %14d %12.3f %15.3f %23.3f %15.2f   entropy x %.2f" %
                         (name, d["units"], d["entropy_ms"], d["device_ms"], d["stream_span_ms"], d["wall_ms"],
                          base["entropy_ms"] / d["entropy_ms"]))
        lines.append("  (c) file size: " + ", ".join("%s %+.2f %%" % (name, 100.0 * (d["file_bytes"] - base["file_bytes"]) / base["file_bytes"])
                                                     for name, d in dec.items() if name != "original"))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return results


if __name__ == "__main__":
    main()
