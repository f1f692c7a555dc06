"""TEST INFRASTRUCTURE: numpy restatement of the video-level aggregation rules and the seeded inputs the fixture
generator (tools/make_video_cls_golden.py) and tests/test_video_cls.py share.

The restatement is written from the rules in DESIGN.md section 3.14, in float64.  It differs from the reference's
``sliding_window_aggregation_func`` in ONE place: the number of windows averaged per span is ``max(15, n // 4)``, the
Python 2 integer division the reference was written for (its ``n / 4`` is a float under Python 3 and the function
fails for n > 60)."""
import math

import numpy as np

TS = (1, 3, 14, 15, 16, 59, 60, 61, 64, 65, 257, 1000)      # ragged batch: n < 15, n // 4 passing 15, > 1 LDS tile of rows
CS = (1, 7, 64, 65, 101)
EXACT_CASES = [(c, 0) for c in CS] + [(7, 1), (7, 2), (65, 2), (65, 4), (101, 1)]      # (C, crops); crops 0: [T, C] input
TOL_CASES = [(7, 1), (65, 10), (101, 10)]
SPANS = (1, 2, 4, 8, 16)
TOP_K = 5


def plan(fps, spans=SPANS, overlap=0.2):
    out = []
    for t_span in spans:
        span = t_span * fps
        out.append((span, int(math.ceil(span * (1 - overlap)))))
    return out


def dyadic_batch(seed, c, crops, ts=TS):
    """float32 videos whose entries are multiples of 2^-6 with |x| <= 8 (every sum of <= 4096 of them is exact in
    float32 in any order).  Columns cycle through: random, constant, three values (ties at every cut), +-0.0 mixed
    with a few other values, all negative."""
    rs = np.random.RandomState(seed)
    out = []
    for t in ts:
        shape = (t, crops, c) if crops else (t, c)
        x = rs.randint(-512, 513, size=shape).astype(np.float32) / 64
        for col in range(c):
            kind = col % 5
            if kind == 1:
                x[..., col] = -2.75
            elif kind == 2:
                x[..., col] = rs.choice(np.float32([-1.5, 0.25, 3.0]), size=shape[:-1])
            elif kind == 3:
                x[..., col] = rs.choice(np.float32([0.0, -0.0, -0.0, 0.0, 1.0, -1.0]), size=shape[:-1])
            elif kind == 4:
                x[..., col] = -np.abs(x[..., col]) - np.float32(0.5)
        out.append(x)
    return out


def float_batch(seed, c, crops, ts=TS):
    rs = np.random.RandomState(seed)
    return [(3 * rs.randn(t, crops, c)).astype(np.float32) for t in ts]


def softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def frames(v, crop_agg="mean"):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 2:
        return v
    return v.max(axis=1) if crop_agg == "max" else v.sum(axis=1) / v.shape[1]


def mean_of_largest(rows, k):
    k = min(k, rows.shape[0])
    return np.sort(rows, axis=0)[rows.shape[0] - k:].sum(axis=0) / k


def agg_default(v, norm, crop_agg="mean"):
    f = frames(v, crop_agg)
    out = f.sum(axis=0) / f.shape[0]
    return softmax(out) if norm else out


def agg_top_k(v, k, norm, crop_agg="mean"):
    out = mean_of_largest(frames(v, crop_agg), k)
    return softmax(out) if norm else out


def span_rows(v, fps, crop_agg="mean"):
    """[S, C]: per span the mean of the max(15, n // 4) largest of its n window maxima"""
    f = frames(v, crop_agg)
    rows = []
    for span, step in plan(fps):
        wins = np.stack([f[i:i + span].max(axis=0) for i in range(0, f.shape[0], step)])
        rows.append(mean_of_largest(wins, max(15, wins.shape[0] // 4)))
    return np.stack(rows)


def agg_sliding(v, fps, norm, crop_agg="mean"):
    r = span_rows(v, fps, crop_agg)
    out = r.sum(axis=0) / r.shape[0]
    return softmax(out) if norm else out


def agg_tpp(v, num_class):
    f = frames(v)
    t, stages = f.shape[0], f.shape[1] // num_class
    out = np.zeros(num_class)
    for i in range(t):
        k = int(i * (float(stages) / t))
        out += f[i, k * num_class:(k + 1) * num_class]
    return out / t


def fuse(major, others, weights, norm):
    out = np.asarray(major, dtype=np.float64).copy()
    for s, w in zip(others, weights):
        out = out + np.asarray(s, dtype=np.float64) * float(np.float32(w))
    return softmax(out) if norm else out


def tpp_probe(t, stages):
    """[t, 1, stages * t] with num_class = t: frame i holds (k + 1) * t in column k * t + i, so that the aggregate's
    entry i is exactly k_i + 1 -- the stage index the function used for frame i."""
    x = np.zeros((t, 1, stages * t), dtype=np.float32)
    for i in range(t):
        for k in range(stages):
            x[i, 0, k * t + i] = (k + 1) * t
    return x


TPP_PROBES = [(1, 1), (1, 4), (3, 2), (7, 3), (10, 3), (49, 7), (64, 5), (100, 3), (257, 7)]      # (T, stages)


def metric_case(seed, v, c, ties=False, every_class_positive=True, multi=False):
    """(scores float32 [v, c], label sets).  ties: scores drawn from a few values.  every_class_positive: labels cover
    all classes (v >= c)."""
    rs = np.random.RandomState(seed)
    if ties:
        s = rs.choice(np.float32([-1.0, 0.0, 0.5, 2.0]), size=(v, c))
    else:
        s = rs.permutation(v * c).reshape(v, c).astype(np.float32) / 16 - v * c / 32      # all distinct
    lab = rs.randint(0, c, v)
    if every_class_positive:
        lab[:c] = np.arange(c)
    sets = [[int(x)] for x in lab]
    if multi:
        for i in range(0, v, 3):
            sets[i] = sorted(set(sets[i] + [int(rs.randint(0, c))]))
    return s, sets


def predicted_only_case():
    """24 videos, 9 classes: no video is labelled 8, video 0 is predicted as class 8"""
    s, sets = metric_case(seed=3, v=24, c=9, every_class_positive=False)
    sets = [[x[0] % 8] for x in sets]
    s[0, 8] = s.max() + 1
    return s, sets


def stable_top_k_hit_rate(scores, sets, k):
    hits = 0
    for s, lb in zip(scores, sets):
        top = np.argsort(s, kind="stable")[-k:]
        hits += bool(set(lb) & set(int(x) for x in top))
    return hits / float(len(sets))
