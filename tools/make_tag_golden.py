#!/usr/bin/env python
"""Generate tests/golden/ref_tag.npz: seeded actionness scores and what the REFERENCE's own functions make of them
(test infrastructure; runs only where the reference tree exists, the fixture it writes is committed).

Per video: label rows (ops/sequence_funcs.py label_frame_by_threshold), every candidate before the NMS
(build_box_by_search), the kept boxes / scores and the spans in seconds (gen_prop of gen_bottom_up_proposals.py,
compiled from the script at run time), named proposals (ops/detection_metrics.py name_proposal) and the dumped record
(ops/io.py dump_window_list).  Plus merged scores (the merging loop of the script) and sliding windows.

Two conditions on the inputs make exact comparison legitimate, both asserted here (another seed is drawn otherwise):
  * no smoothed probability lies within MARGIN = 1e-5 of a threshold (the product's expf / softmax differ from numpy's
    by a few float32 ulp, <= 3e-7 on a probability);
  * the reference's kept list does not depend on how EQUAL scores are ordered (numpy's default argsort is unstable):
    greedy NMS on the reference's candidates with ties lowest-index-first and highest-index-first both give the
    multiset the reference's temporal_nms returned, and no tie group of different spans is larger than two.
"""
import argparse
import ast
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ref_tag.npz")
THRESH = [0.01, 0.05, 0.1, .15, 0.25, .4, .5, .6, .7, .8, .9, .95]
TOL = [0.05, .1, .2, .3, .4, .5, .6, 0.8, 1.0]
MARGIN = 1e-5
MINIMUM_LEN = 1.5


def script_nodes(path, pick):
    """Top-level statements of a reference SCRIPT (it parses argv and loads files at import time, so it cannot be
    imported) selected by `pick`, compiled from the file where it lies; nothing is copied."""
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if pick(n)]
    assert body
    return compile(ast.Module(body=body, type_ignores=[]), path, "exec")


def noisy_video(T, n_seg, seed, amp=1.5, sigma=2.0):
    rs = np.random.RandomState(seed)
    base = -np.ones(T)
    segs = []
    for _ in range(n_seg):
        ln = int(rs.randint(max(2, T // (6 * n_seg)), max(3, T // (2 * n_seg)) + 1))
        s = int(rs.randint(0, max(1, T - ln)))
        base[s:s + ln] = 1.0
        segs.append((s, s + ln))
    logit = base * amp + rs.standard_normal(T) * sigma
    common = rs.standard_normal(T) * 0.5
    return np.stack([common - logit / 2, common + logit / 2], axis=1).astype(np.float32), segs


def const_video(pattern, seed):
    """clean foreground / background frames; a little jitter so that spans of equal length do not tie on their score"""
    fg = np.asarray(pattern, dtype=bool)
    jit = np.random.RandomState(seed).uniform(-0.2, 0.2, (len(fg), 2))
    return (np.stack([np.where(fg, -3.0, 3.0), np.where(fg, 3.0, -3.0)], axis=1) + jit).astype(np.float32)


def both_ends_video(seed):
    """foreground touching both ends.  Every label row's first run starts at frame 0 here, and the backward search's
    fall-through branch scores the span (0, down + 1) with the sum up to down + 2 -- the score of the span (0, down + 2)
    of a row whose first run is one frame longer: an exact tie of two spans that suppress each other.  The first run
    therefore fades out over 80 frames, so that no two thresholds are crossed on neighbouring frames."""
    p = np.concatenate([np.full(30, 0.998), np.linspace(0.998, 0.002, 80), np.full(40, 0.002), np.linspace(0.002, 0.998, 30),
                        np.full(20, 0.998)])
    logit = np.log(p / (1 - p)) + np.random.RandomState(seed).uniform(-0.02, 0.02, len(p))
    return np.stack([-logit / 2, logit / 2], axis=1).astype(np.float32)


def greedy_nms(boxes, thresh, lowest_first):
    t1 = np.array([b[0] for b in boxes], dtype=np.int64)
    t2 = np.array([b[1] for b in boxes], dtype=np.int64)
    sc = np.array([b[3] for b in boxes])
    idx = np.arange(len(boxes))
    order = np.lexsort((idx if lowest_first else -idx, -sc.astype(np.float64)))
    keep = []
    while order.size:
        i = order[0]
        keep.append(i)
        rest = order[1:]
        inter = np.minimum(t2[i], t2[rest]) - np.maximum(t1[i], t1[rest]) + 1
        iou = inter / ((t2[i] - t1[i] + 1) + (t2[rest] - t1[rest] + 1) - inter).astype(float)
        order = rest[iou <= thresh]
    return sorted((int(t1[i]), int(t2[i]), np.float32(sc[i]).view(np.uint32).item()) for i in keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    assert os.path.isdir(REF), "this script needs the reference tree at %s" % REF
    sys.path.insert(0, REF)
    from ops import sequence_funcs as SF
    from ops.detection_metrics import name_proposal
    from ops.io import dump_window_list

    script = os.path.join(REF, "gen_bottom_up_proposals.py")
    ns = {"np": np, "label_frame_by_threshold": SF.label_frame_by_threshold, "build_box_by_search": SF.build_box_by_search,
          "temporal_nms": SF.temporal_nms, "reg_score_dict": None, "score_dict": {},
          "args": SimpleNamespace(dataset="thumos14", minimum_len=MINIMUM_LEN)}
    exec(script_nodes(script, lambda n: isinstance(n, ast.FunctionDef) and n.name == "gen_prop"), ns)
    gen_prop = ns["gen_prop"]

    def reference(scores, duration, vid):
        """-> dict of the reference's results for one video, or a string saying which input condition failed"""
        T = len(scores)
        rows = SF.label_frame_by_threshold(scores, [0], bw=3, thresh=THRESH, multicrop=False)
        from ops.metrics import softmax
        from scipy.ndimage import gaussian_filter
        sm = gaussian_filter(softmax(scores)[:, 1], 3)
        assert sm.dtype == np.float32
        margin = float(np.abs(sm[None, :].astype(np.float64) - np.asarray(THRESH, dtype=np.float32)[:, None]).min())
        if margin < MARGIN:
            return "margin %.2g" % margin
        for (_, lab, _), th in zip(rows, THRESH):
            assert np.array_equal(lab, sm > th)
        cands = SF.build_box_by_search(rows, np.array(TOL))
        ns["score_dict"][vid] = scores
        _, pr_box, kept_scores = gen_prop(SimpleNamespace(id=vid, duration=duration))
        kept = SF.temporal_nms(cands, 0.9) if cands else []
        assert [np.float32(k[3]) for k in kept] == [np.float32(s) for s in kept_scores] or not kept
        ref_set = sorted((int(k[0]), int(k[1]), np.float32(k[3]).view(np.uint32).item()) for k in kept)
        if cands:
            groups = {}
            for c in cands:
                groups.setdefault(np.float32(c[3]).view(np.uint32).item(), set()).add((int(c[0]), int(c[1])))
            if max(len(g) for g in groups.values()) > 2:
                return "tie group larger than two"
            if greedy_nms(cands, 0.9, True) != ref_set or greedy_nms(cands, 0.9, False) != ref_set:
                return "kept list depends on the order of equal scores"
        all_sec = [(k[0] / float(T) * duration, k[1] / float(T) * duration) for k in kept]
        assert [s for s in all_sec if s[1] - s[0] > MINIMUM_LEN] == list(pr_box)
        return {"labels": np.stack([r[1] for r in rows]), "cands": cands, "kept": kept, "seconds": pr_box,
                "margin": margin, "runs": max(int(np.sum(np.diff(np.concatenate([[0], r[1].astype(int)])) == 1)) for r in rows)}

    # (name, gpu_only, maker(seed) -> scores, searched over seeds?)
    cases = [("all_bg", False, lambda s: const_video(np.zeros(50), s), True),
             ("all_fg", False, lambda s: const_video(np.ones(50), s), True),
             ("t1_fg", False, lambda s: const_video([1], s), True),
             ("t1_bg", False, lambda s: const_video([0], s), True),
             ("t5", False, lambda s: const_video([1, 1, 0, 1, 1], s), True),
             ("both_ends", False, lambda s: both_ends_video(s), True),
             ("noisy60", False, lambda s: noisy_video(60, 3, s)[0], True),
             ("noisy300", False, lambda s: noisy_video(300, 6, s)[0], True),
             ("noisy1200", True, lambda s: noisy_video(1200, 8, s)[0], True),
             ("noisy4000", True, lambda s: noisy_video(4000, 10, s)[0], True),
             ("runs3000", True, lambda s: noisy_video(3000, 50, s, amp=2.0, sigma=1.5)[0], True)]
    out = {"thresholds": np.asarray(THRESH), "tolerances": np.asarray(TOL), "minimum_len": np.asarray([MINIMUM_LEN]),
           "margin_required": np.asarray([MARGIN]), "names": np.asarray([c[0] for c in cases])}
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(tmp)
    for i, (name, gpu_only, make, search) in enumerate(cases):
        for seed in range(1000 * i, 1000 * i + (400 if search else 1)):
            scores = make(seed)
            T = len(scores)
            duration = round(T * 0.21 + 0.37, 2)
            r = reference(scores, duration, name)
            if not isinstance(r, str):
                break
            print("  %s seed %d rejected: %s" % (name, seed, r))
        assert not isinstance(r, str), (name, r)
        if name == "runs3000":
            assert len(r["cands"]) > 2048, "the global-memory case needs more than 2048 candidates"
        # ground truth: none / one / several instances (seconds); labels arbitrary class numbers
        rs = np.random.RandomState(77 + i)
        n_gt = [0, 1, 0, 1, 1, 3, 1, 3, 4, 0, 6][i]
        starts = np.sort(rs.uniform(0, duration * 0.8, n_gt))
        gt = [(int(rs.randint(0, 20)), (float(s), float(min(duration, s + rs.uniform(0.5, duration * 0.3))))) for s in starts]
        named = name_proposal(gt, r["seconds"])
        frame_cnt = 2 * T + 3
        os.makedirs(os.path.join("frames", name))
        for f in range(frame_cnt):
            open(os.path.join("frames", name, "img_%05d.jpg" % (f + 1)), "w").close()
        info = SimpleNamespace(path="videos/%s.mp4" % name, id=name, duration=duration,
                               instance=[SimpleNamespace(num_label=g[0], time_span=g[1]) for g in gt])
        text = dump_window_list(info, named, "frames", "img_*.jpg")
        p = "v%d_" % i
        out[p + "scores"] = scores
        out[p + "duration"] = np.asarray([duration])
        out[p + "gpu_only"] = np.asarray([int(gpu_only)])
        out[p + "seed"] = np.asarray([seed])
        out[p + "margin"] = np.asarray([r["margin"]])
        out[p + "labels"] = np.packbits(r["labels"], axis=1)
        out[p + "cand_box"] = np.asarray([[c[0], c[1]] for c in r["cands"]], dtype=np.int32).reshape(-1, 2)
        out[p + "cand_score"] = np.asarray([c[3] for c in r["cands"]], dtype=np.float32)
        out[p + "kept_box"] = np.asarray([[k[0], k[1]] for k in r["kept"]], dtype=np.int32).reshape(-1, 2)
        out[p + "kept_score"] = np.asarray([k[3] for k in r["kept"]], dtype=np.float32)
        out[p + "seconds"] = np.asarray(r["seconds"], dtype=np.float64).reshape(-1, 2)
        out[p + "gt_label"] = np.asarray([g[0] for g in gt], dtype=np.int32)
        out[p + "gt_span"] = np.asarray([g[1] for g in gt], dtype=np.float64).reshape(-1, 2)
        out[p + "named"] = np.asarray(named, dtype=np.float64).reshape(-1, 5)
        out[p + "frame_cnt"] = np.asarray([frame_cnt])
        out[p + "dump"] = np.asarray(text)
        print("%-10s T %5d seed %5d margin %.2g runs<=%d candidates %5d kept %4d spans>%.1fs %4d gt %d"
              % (name, T, seed, r["margin"], r["runs"], len(r["cands"]), len(r["kept"]), MINIMUM_LEN, len(r["seconds"]), n_gt))
    os.chdir(cwd)

    # merged scores: 2 files, the second one shorter for video "a" and longer for "b", with weights
    rs = np.random.RandomState(5)
    files = [{"a": rs.standard_normal((40, 10, 2)).astype(np.float32), "b": rs.standard_normal((33, 10, 2)).astype(np.float32)},
             {"a": rs.standard_normal((31, 10, 2)).astype(np.float32), "b": rs.standard_normal((57, 10, 2)).astype(np.float32)}]
    for tag, weights in (("w", [0.7, 1.3]), ("n", None)):
        mns = {"score_list": files, "args": SimpleNamespace(score_weights=weights), "score_dict": {}}
        exec(script_nodes(script, lambda n: isinstance(n, ast.For) and getattr(n.target, "id", "") == "key"
                          and "score_list" in ast.dump(n.iter)), mns)
        for k in "ab":
            out["merge_%s_%s" % (tag, k)] = mns["score_dict"][k]
            assert mns["score_dict"][k].dtype == np.float32
    for f in range(2):
        for k in "ab":
            out["merge_in%d_%s" % (f, k)] = files[f][k]
    out["merge_weights"] = np.asarray([0.7, 1.3])

    for j, d in enumerate((7, 33.5, 200)):
        sw = SF.gen_exponential_sw_proposal(SimpleNamespace(duration=d))
        out["sw%d_duration" % j] = np.asarray([d], dtype=np.float64)
        out["sw%d" % j] = np.asarray(sw, dtype=np.float64).reshape(-1, 2)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
