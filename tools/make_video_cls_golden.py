#!/usr/bin/env python
"""Generate tests/golden/ref_video_cls.npz: what the REFERENCE's own ops.video_funcs and ops.metrics make of the seeded
inputs of tests/video_cls_referee.py (test infrastructure; runs only where the reference tree, sklearn, scipy and pandas
exist, the fixture it writes is committed).

Two facts about the reference under Python 3: it uses ``xrange`` (this script sets ``builtins.xrange = range`` before the
import), and ``sliding_window_aggregation_func`` computes ``k = max(15, len(local_agg) / 4)``, a float as soon as a span
has more than 60 windows -- the slice then raises TypeError.  Such (video, fps) pairs are masked out (``*_ok``) and the
tests compare them with the ``n // 4`` restatement instead.  The per-span rows are the reference function's output for
``spans=[t_span]`` (the mean over one span is that span's row).

Also recorded: e_ref per mode = max |reference float32 result - float64 restatement| over the tolerance inputs; the
tests allow the device 4 x e_ref (floor: one float32 ulp of the largest restatement value).
"""
import builtins
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_video_cls.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
builtins.xrange = range

import video_cls_referee as R      # noqa: E402
from ops import metrics as M      # noqa: E402
from ops import video_funcs as VF      # noqa: E402


def as3(v):
    return v if v.ndim == 3 else v[:, None, :]


def sliding(v, fps, norm, spans=R.SPANS):
    try:
        return VF.sliding_window_aggregation_func(as3(v), spans=list(spans), norm=norm, fps=fps)
    except TypeError:
        return None


def main():
    g = {}
    # ---- exact cases: dyadic inputs, no softmax
    for i, (c, crops) in enumerate(R.EXACT_CASES):
        vids = R.dyadic_batch(100 + i, c, crops)
        tag = "%d_%d" % (c, crops)
        g["xd_" + tag] = np.stack([VF.default_aggregation_func(as3(v), normalization=False) for v in vids]).astype(np.float32)
        g["xk1_" + tag] = np.stack([VF.top_k_aggregation_func(as3(v), 1, normalization=False) for v in vids]).astype(np.float32)
        g["xk_" + tag] = np.stack([VF.top_k_aggregation_func(as3(v), R.TOP_K, normalization=False) for v in vids]).astype(np.float32)
        if crops:
            g["xdmax_" + tag] = np.stack([VF.default_aggregation_func(v, normalization=False, crop_agg=np.max)
                                          for v in vids]).astype(np.float32)
        for fps in (1, 3):
            rows = np.full((len(vids), len(R.SPANS), c), np.nan, dtype=np.float32)
            outs = np.full((len(vids), c), np.nan, dtype=np.float32)
            ok = np.zeros(len(vids), dtype=bool)
            for j, v in enumerate(vids):
                o = sliding(v, fps, False)
                if o is None:
                    continue
                ok[j] = True
                outs[j] = o
                for s, t_span in enumerate(R.SPANS):
                    rows[j, s] = sliding(v, fps, False, spans=[t_span])
            g["xs%d_%s" % (fps, tag)], g["xo%d_%s" % (fps, tag)], g["xok%d_%s" % (fps, tag)] = rows, outs, ok
    # ---- tolerance cases: general floats, softmax on; e_ref against the float64 restatement
    e = dict(default=0.0, top_k=0.0, sliding_window=0.0, fusion=0.0)
    for i, (c, crops) in enumerate(R.TOL_CASES):
        vids = R.float_batch(200 + i, c, crops)
        for v in vids:
            e["default"] = max(e["default"], np.abs(VF.default_aggregation_func(v) - R.agg_default(v, True)).max())
            e["top_k"] = max(e["top_k"], np.abs(VF.top_k_aggregation_func(v, R.TOP_K) - R.agg_top_k(v, R.TOP_K, True)).max())
            for fps in (1, 3):
                o = sliding(v, fps, True)
                if o is not None:
                    assert o.dtype == np.float32
                    e["sliding_window"] = max(e["sliding_window"], np.abs(o - R.agg_sliding(v, fps, True)).max())
    # ---- fusion
    rs = np.random.RandomState(300)
    streams = [(2 * rs.randn(len(R.TS), 65)).astype(np.float32) for _ in range(3)]
    dyadic = [rs.randint(-512, 513, size=(len(R.TS), 65)).astype(np.float32) / 64 for _ in range(3)]
    g["fuse_streams"], g["fuse_dyadic"] = np.stack(streams), np.stack(dyadic)
    g["fuse_w"], g["fuse_w_dyadic"] = np.float32([1.5, 0.4]), np.float32([0.5, 2.0])
    for n_other in (1, 2):
        for norm in (False, True):
            ref = np.stack([VF.default_fusion_func(streams[0][j].copy(), [s[j] for s in streams[1:1 + n_other]],
                                                   [float(w) for w in g["fuse_w"][:n_other]], norm=norm)
                            for j in range(len(R.TS))])
            assert ref.dtype == np.float32
            if norm:
                rest = np.stack([R.fuse(streams[0][j], [s[j] for s in streams[1:1 + n_other]], g["fuse_w"][:n_other], True)
                                 for j in range(len(R.TS))])
                e["fusion"] = max(e["fusion"], np.abs(ref - rest).max())
        g["fuse_exact_%d" % n_other] = np.stack([
            VF.default_fusion_func(dyadic[0][j].copy(), [s[j] for s in dyadic[1:1 + n_other]],
                                   [float(w) for w in g["fuse_w_dyadic"][:n_other]], norm=False) for j in range(len(R.TS))])
    for k, val in e.items():
        g["e_" + k] = np.float64(val)
        print("e_ref %-15s %.3e" % (k, val))
    # ---- TPP stage indices through one-hot probes
    for t, stages in R.TPP_PROBES:
        x = R.tpp_probe(t, stages)
        ref = VF.tpp_aggregation_func(x, t)
        assert np.array_equal(ref, np.round(ref)) and np.array_equal(ref, R.agg_tpp(x, t))
        g["tpp_%d_%d" % (t, stages)] = ref.astype(np.float32)
    # ---- metrics
    from sklearn.metrics import average_precision_score
    cases = dict(m1=dict(seed=1, v=40, c=11), m2=dict(seed=2, v=30, c=6, ties=True), m4=dict(seed=4, v=45, c=9, multi=True),
                 m5=dict(seed=5, v=300, c=140))
    for name, kw in cases.items():
        s, sets = R.metric_case(**kw)
        score_dict = {"v%d" % j: s[j] for j in range(len(s))}
        vlist = [SimpleNamespace(id="v%d" % j, instances=[SimpleNamespace(num_label=x) for x in sets[j]]) for j in range(len(s))]
        if not kw.get("ties"):
            g[name + "_topk"] = np.float64([M.top_k_accuracy(score_dict, vlist, k) for k in (1, 3, 5)])
        gt = np.zeros(s.shape)
        for j, lb in enumerate(sets):
            gt[j, lb] = 1
        g[name + "_map"] = np.float64(M.video_mean_ap(score_dict, vlist))
        g[name + "_ap"] = np.float64(average_precision_score(gt, s, average=None))
        if not kw.get("multi"):
            g[name + "_mca"] = np.float64(M.mean_class_accuracy(s, np.array([lb[0] for lb in sets])))
    # a class that is only predicted: labels avoid class 8, video 0 is predicted as class 8
    s, sets = R.predicted_only_case()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g["m3_mca"] = np.float64(M.mean_class_accuracy(s, np.array([lb[0] for lb in sets])))
    assert np.isnan(g["m3_mca"])
    np.savez_compressed(OUT, **g)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(g), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
