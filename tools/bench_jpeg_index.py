#!/usr/bin/env python
"""Measure who should find the restart intervals of a batch of JPEG files: the host walk (``JpegDecoder(index="host")``, the default)
or ``ssn_jpeg_index`` on the device (``index="device"``).

    python tools/bench_jpeg_index.py --out profiles/jpeg_index_measured.txt

The workloads and variants of tools/bench_jpeg_transcode.py part (b): 288 RGB frames of 340 x 256, 4:2:0, quality 75 (one SSN step)
and 2880 gray flow frames of the same size, quality 95, as PIL writes them (no restart markers) and transcoded in this run at
``restart_rows`` 1, 2 and 4.  Every (variant, index mode) pair has a decoder of its own; all of them alternate inside every repeat,
so a drift of the machine hits both modes alike.  Per pair: medians of the repeats after warm-up, with minimum and maximum of the
span, of
  enqueue   host clock from the call to its return (the last launch is enqueued; nothing is waited for),
  index     the ``ssn_jpeg_index`` launch plus the launch that ORs its verdicts into ``status`` (HIP events),
  entropy   the Huffman launch,
  stages    everything the call enqueues: upload, index, entropy, inverse DCT, pixels,
  span      one event in front of the call to one behind it, on the stream,
  clock     host clock from the call to the end of a synchronisation behind it,
and the bytes that went over PCIe.  The outputs of the two modes are compared with ``torch.equal``.  Nothing here is a pass/fail
condition.
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
MODES = ("host", "device")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(variants, mode, device, repeats):
    """variants: {label: files} -> {label: {index mode: dict}}, {label: outputs of the two modes equal}"""
    import torch
    from action_detection_amd.jpeg_decode import JpegDecoder, parse_jpeg
    decs = {(label, m): JpegDecoder(device, index=m) for label in variants for m in MODES}
    equal = {}
    for label, files in variants.items():
        outs = []
        for m in MODES:
            d = decs[(label, m)]
            for _ in range(2):
                out = d.decode(files, mode, stack=True)
            torch.cuda.synchronize(device)
            assert d.fallbacks == 0 and int(d.status.abs().sum().item()) == 0, (label, m)
            outs.append(out.clone())
        equal[label] = bool(torch.equal(outs[0], outs[1]))
        del outs
    series = {key: dict(enqueue=[], span=[], clock=[]) for key in decs}
    for d in decs.values():
        d.profile = []
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        for key, d in decs.items():
            files = variants[key[0]]
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            start.record()
            d.decode(files, mode, stack=True)
            t1 = time.perf_counter()
            end.record()
            torch.cuda.synchronize(device)
            t2 = time.perf_counter()
            s = series[key]
            s["enqueue"].append(1e3 * (t1 - t0))
            s["clock"].append(1e3 * (t2 - t0))
            s["span"].append(start.elapsed_time(end))
    res = {}
    for (label, m), d in decs.items():
        stages = {}
        for name, a, b in d.profile:
            stages.setdefault(name, []).append(a.elapsed_time(b))
        stages = {name: median(v) for name, v in stages.items()}
        s = series[(label, m)]
        res.setdefault(label, {})[m] = dict(
            units=sum(len(parse_jpeg(f).units) for f in variants[label]), enqueue_ms=median(s["enqueue"]),
            index_ms=stages.get("index", 0.0) + stages.get("verdicts", 0.0), entropy_ms=stages["entropy"], device_ms=sum(stages.values()),
            stages_ms=stages, span_ms=median(s["span"]), span_min_ms=min(s["span"]), span_max_ms=max(s["span"]), clock_ms=median(s["clock"]),
            uploaded_bytes=d.uploaded_bytes)
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
        raise SystemExit("bench_jpeg_index needs a HIP device: a CPU run says nothing about either path")
    from action_detection_amd.jpeg_transcode import JpegTranscoder
    make_files = _tool("bench_jpeg").make_files
    lines = ["Restart-interval index on the host and on the device, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "340 x 256 frames made with PIL (no restart markers) from a seeded smooth-plus-noise picture, transcoded in this run; medians "
             "of %d repeats after warm-up, span with [min .. max]" % args.repeats,
             "JpegDecoder.decode(files, mode, stack=True); the eight (variant, index) decoders alternate inside every repeat; times in ms"]
    results = {}
    for label, n, gray, mode, quality in (("RGB 4:2:0 q75", args.frames, False, "RGB", 75), ("Flow gray q95", args.flow_frames, True, "L", 95)):
        files = make_files(n, gray, quality)
        variants = {"original": files}
        transcoder = JpegTranscoder(args.device)
        for rows in ROWS:
            variants["restart_rows=%d" % rows] = transcoder.transcode(files, restart_rows=rows)
            assert transcoder.skipped == [], transcoder.skipped[:3]
        del transcoder
        res, equal = measure(variants, mode, args.device, args.repeats)
        results[label] = dict(frames=n, decode=res, outputs_equal=equal)
        lines += ["", "%s: %d frames" % (label, n),
                  "  %-16s %-7s %8s %9s %8s %9s %9s %28s %9s %12s  %s" %
                  ("files", "index", "units", "enqueue", "index", "entropy", "stages", "span [min .. max]", "clock", "uploaded MB", "equal")]
        for name, modes in res.items():
            for m in MODES:
                d = modes[m]
                lines.append("  %-16s %-7s %8d %9.2f %8.3f %9.3f %9.3f %9.2f [%7.2f .. %7.2f] %9.2f %12.2f  %s" %
                             (name, m, d["units"], d["enqueue_ms"], d["index_ms"], d["entropy_ms"], d["device_ms"], d["span_ms"],
                              d["span_min_ms"], d["span_max_ms"], d["clock_ms"], d["uploaded_bytes"] / 1e6, equal[name]))
            h, dv = modes["host"], modes["device"]
            spread = max(h["span_max_ms"] - h["span_min_ms"], dv["span_max_ms"] - dv["span_min_ms"])
            lines.append("  %-16s span host - device = %+.2f ms (larger min-max spread of the two: %.2f ms)" %
                         ("", h["span_ms"] - dv["span_ms"], spread))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return results


if __name__ == "__main__":
    main()
