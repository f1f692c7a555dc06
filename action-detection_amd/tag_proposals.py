"""Temporal actionness grouping (TAG): from per-frame actionness scores to temporal proposals -- stage 2 of the
reference's workflow (/root/reference/gen_bottom_up_proposals.py with ops/sequence_funcs.py, ops/detection_metrics.py),
between ``binary_model.BinaryClassifier`` (stage 1) and the proposal list ``SSN`` trains and tests on (stage 3).

The reference runs ``gen_prop`` per video in a pool of 32 processes.  ``TagProposalGenerator.generate`` takes a LIST of
videos and runs them as one batch through csrc/tag.hip: a counting phase, one host read (to size the candidate
workspace), a generating phase -- the number of launches and host synchronisations does not depend on the number of
videos.  Results are the reference's, quirks included: a box ends at ``down + 1`` (up to ``T + 1``), the returned
scores are not filtered by ``minimum_len``.  The one free choice -- how EQUAL scores are ordered in front of the NMS,
which numpy's unstable argsort leaves open -- is fixed here: smaller start, then smaller end, first.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import kernels as K

# the lists gen_prop hard-codes (gen_bottom_up_proposals.py:124,127)
DEFAULT_THRESHOLDS = (0.01, 0.05, 0.1, .15, 0.25, .4, .5, .6, .7, .8, .9, .95)
DEFAULT_TOLERANCES = (0.05, .1, .2, .3, .4, .5, .6, 0.8, 1.0)

TagResult = namedtuple("TagResult", "boxes scores seconds candidates labels")
TagResult.__doc__ = """One video: boxes int32 [K, 2] (frames) and scores float32 [K] of the proposals the NMS kept, in NMS
order; seconds float64 [K', 2], the spans longer than minimum_len; with return_candidates the (boxes [N, 2], scores
[N]) of every candidate before the NMS in the reference's order, with return_labels the bool label rows [n_thr, T]."""


def _default_device():
    return torch.device("cpu") if _lib.emulator_active() else torch.device("cuda")


def merge_scores(score_dicts, weights=None):
    """Merge the score files of several models (gen_bottom_up_proposals.py:76-91): per video the mean over the crop axis
    of every file's [T, crops, 2] scores, times the file's weight, summed; a shorter file truncates the sum, a longer one
    is resampled at ``int(x * tick)``.  float32 throughout; the crop mean is sequential adds in crop order, then one
    division, which is what numpy's mean does on this layout.  Host arithmetic."""
    def crop_mean(a):
        a = np.asarray(a, dtype=np.float32)
        acc = a[:, 0].copy()
        for c in range(1, a.shape[1]):
            acc += a[:, c]
        return acc / np.float32(a.shape[1])

    def weight(i):
        return np.float32(1.0 if weights is None else weights[i])

    out = {}
    for key in score_dicts[0]:
        merged = crop_mean(score_dicts[0][key]) * weight(0)
        for i in range(1, len(score_dicts)):
            add = crop_mean(score_dicts[i][key])
            if add.shape[0] < merged.shape[0]:
                merged = merged[:add.shape[0]]
            elif add.shape[0] > merged.shape[0]:
                tick = add.shape[0] / float(merged.shape[0])
                add = add[[int(x * tick) for x in range(merged.shape[0])]]
            merged += add * weight(i)
        out[key] = merged
    return out


@torch.no_grad()
def merge_scores_device(streams, weights=None):
    """``merge_scores`` without leaving the GPU: ``streams`` is a list of ``{video id: float32 [T_s, C] device tensor}``,
    already crop-averaged (``ActionnessScores.mean``); -> ``{video id: [T, C] device tensor}`` from ONE
    ``ssn_actionness_merge`` launch for all videos.  Same arithmetic, bit for bit: weights rounded to float32, multiply then
    add, a shorter stream truncates the sum, a longer one is read at ``int(x * (T_s / float(T)))``.  The output lengths
    follow from the input lengths, so nothing is read back."""
    if len(streams) < 1:
        raise ValueError("merge_scores_device: at least one stream")
    if weights is not None and len(weights) != len(streams):
        raise ValueError("merge_scores_device: one weight per stream")
    keys = list(streams[0])
    if not keys:
        return {}
    parts, lens = [], []
    for st in streams:
        for k in keys:
            t = st[k]
            if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1 \
                    or t.shape[1] != streams[0][keys[0]].shape[1]:
                raise ValueError("merge_scores_device: every stream must hold float32 [T >= 1, C] tensors, got %r for %r"
                                 % (getattr(t, "shape", t), k))
            parts.append(t)
            lens.append(t.shape[0])
    dev = parts[0].device
    v = len(keys)
    lens = np.asarray(lens, dtype=np.int64).reshape(len(streams), v)
    out_len = lens[0].copy()
    for s in range(1, len(streams)):            # (a longer stream is resampled: the merged length only ever shrinks)
        out_len = np.minimum(out_len, lens[s])
    off = np.concatenate([[0], np.cumsum(lens.ravel())])
    out_off = np.concatenate([[0], np.cumsum(out_len)])
    if off[-1] >= 2 ** 30:
        raise ValueError("merge_scores_device: more than 2^30 rows in one batch")
    w = np.asarray([1.0 if weights is None else weights[i] for i in range(len(streams))], dtype=np.float32)
    rows = torch.cat([p.to(dev) for p in parts]).contiguous()
    out = K.actionness_merge(rows, torch.from_numpy(off.astype(np.int32)).to(dev), torch.from_numpy(w).to(dev),
                             torch.from_numpy(out_off.astype(np.int32)).to(dev), int(out_off[-1]))
    return {k: out[int(out_off[i]):int(out_off[i + 1])] for i, k in enumerate(keys)}


def sliding_window_proposals(duration, time_step=1, max_level=8, overlap=0.4):
    """Exponential sliding windows over a video of ``duration`` seconds (ops/sequence_funcs.py:37-54): spans of
    2**level seconds every ceil(span * (1 - overlap)), kept when at least one second lies inside the video."""
    out = []
    for t_span in (2 ** x for x in range(max_level)):
        step = int(np.ceil(t_span * time_step * (1 - overlap)))
        out.extend((i, i + t_span) for i in np.arange(0, duration, step))
    return [s for s in out if min(duration, s[1]) - s[0] >= 1]


class TagProposalGenerator(object):
    def __init__(self, thresholds=DEFAULT_THRESHOLDS, tolerances=DEFAULT_TOLERANCES, bw=3, nms_threshold=0.9,
                 minimum_len=0, device=None):
        self.thresholds = np.asarray(thresholds, dtype=np.float32)      # numpy compares float32 scores with (float)th
        self.tolerances = np.asarray(tolerances, dtype=np.float64)
        if self.thresholds.ndim != 1 or self.thresholds.size < 1 or self.tolerances.ndim != 1 or self.tolerances.size < 1:
            raise ValueError("thresholds and tolerances must be non-empty lists")
        self.bw = float(bw)
        self.nms_threshold = float(nms_threshold)
        self.minimum_len = float(minimum_len)
        self.device = device

    @torch.no_grad()
    def generate(self, scores, durations, return_candidates=False, return_labels=False):
        """scores: one float32 [T, 2] array / tensor of (background, foreground) actionness scores per video; durations:
        their lengths in seconds.  -> [TagResult] in the order of the input."""
        dev = torch.device(self.device) if self.device is not None else _default_device()
        vids = [s if torch.is_tensor(s) else torch.from_numpy(np.ascontiguousarray(s)) for s in scores]
        if len(vids) < 1 or len(vids) != len(durations):
            raise ValueError("generate: one duration per video, at least one video")
        for s in vids:
            if s.dim() != 2 or s.shape[1] != 2 or s.shape[0] < 1 or s.dtype != torch.float32:
                raise ValueError("generate: every video's scores must be float32 [T >= 1, 2], got %s %s"
                                 % (s.dtype, tuple(s.shape)))
        lens = np.array([s.shape[0] for s in vids], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(lens)])
        if offsets[-1] >= 2 ** 30:
            raise ValueError("generate: more than 2^30 frames in one batch")
        v, n_thr, n_tol = len(vids), self.thresholds.size, self.tolerances.size
        h_off = torch.from_numpy(offsets.astype(np.int32))
        d_off = h_off.to(dev)
        # ONE host-to-device copy for the batch: videos given on the host are concatenated there (a copy per video
        # would make the number of blocking transfers grow with V); only inputs already on a device are joined there
        if not any(s.is_cuda for s in vids):
            cat = torch.cat(vids).contiguous().to(dev)
        else:
            cat = torch.cat([s.to(dev) for s in vids]).contiguous()
        thr = torch.from_numpy(self.thresholds).to(dev)
        tol = torch.from_numpy(self.tolerances).to(dev)
        dur = torch.tensor([float(d) for d in durations], dtype=torch.float64).to(dev)

        smoothed, labels, runs = K.tag_count(cat, h_off, d_off, thr, self.bw, want_labels=return_labels)
        runs = runs.cpu().numpy().astype(np.int64).ravel()              # the one host read between the two phases
        run_off = np.concatenate([[0], np.cumsum(runs)])
        total_runs = int(run_off[-1])
        if 2 * n_tol * total_runs >= 2 ** 30:
            raise ValueError("generate: %d candidates in one batch, split it" % (2 * n_tol * total_runs))
        cand_base = 2 * n_tol * run_off[::n_thr]                         # [V + 1] first candidate of every video
        n_cand = np.diff(cand_base)
        # sort workspace of the videos whose candidates do not fit in LDS: pow2(candidates) entries each
        pow2 = np.left_shift(np.int64(1), np.frexp(np.maximum(n_cand - 1, 0).astype(np.float64))[1].astype(np.int64))
        sort_off = np.concatenate([[0], np.cumsum(np.where(n_cand > K.tag_lds_candidates(), pow2, 0))])
        out = K.tag_generate(cat, smoothed, d_off, dur, thr, tol, torch.from_numpy(run_off.astype(np.int32)).to(dev),
                             torch.from_numpy(sort_off.astype(np.int64)).to(dev), total_runs, int(sort_off[-1]),
                             self.nms_threshold, self.minimum_len)
        # device -> host: the kept rows of every video in one gather per output (a constant number of copies), the
        # candidates only when asked for
        kept_count = out["kept_count"].cpu().numpy().astype(np.int64)
        kept_off = np.concatenate([[0], np.cumsum(kept_count)])
        rows = np.repeat(cand_base[:-1] - kept_off[:-1], kept_count) + np.arange(kept_off[-1])
        rows = torch.from_numpy(rows.astype(np.int64)).to(dev)
        host = {k: out[k].index_select(0, rows).cpu().numpy() for k in ("kept_box", "kept_score", "seconds", "longer")}
        if return_candidates:
            host["cand_box"], host["cand_score"] = out["cand_box"].cpu().numpy(), out["cand_score"].cpu().numpy()
        labels = labels.cpu().numpy().astype(bool) if return_labels else None
        results = []
        for i in range(v):
            b, k = int(cand_base[i]), slice(int(kept_off[i]), int(kept_off[i + 1]))
            longer = host["longer"][k].astype(bool)
            cands = (host["cand_box"][b:b + n_cand[i]].copy(), host["cand_score"][b:b + n_cand[i]].copy()) \
                if return_candidates else None
            results.append(TagResult(host["kept_box"][k].copy(), host["kept_score"][k].copy(),
                                     host["seconds"][k][longer].copy(), cands,
                                     labels[:, offsets[i]:offsets[i + 1]] if return_labels else None))
        return results


@torch.no_grad()
def name_proposals(gt, proposals, thresh=0.0, device=None):
    """``name_proposal`` (ops/detection_metrics.py:54-76) for a list of videos in one launch.  gt: per video
    ``[(label, (start, end)), ...]``; proposals: per video the spans [K, 2] (seconds, or whatever unit gt uses).
    -> per video ``[(label + 1 or 0, best IoU, overlap over the proposal's own length, start, end), ...]``."""
    if len(gt) != len(proposals) or len(gt) < 1:
        raise ValueError("name_proposals: one ground-truth list per video, at least one video")
    dev = torch.device(device) if device is not None else _default_device()
    props = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in proposals]
    spans = [np.asarray([g[1] for g in video], dtype=np.float64).reshape(-1, 2) for video in gt]
    glabel = np.asarray([g[0] for video in gt for g in video], dtype=np.int32)
    p_off = np.concatenate([[0], np.cumsum([len(p) for p in props])]).astype(np.int32)
    g_off = np.concatenate([[0], np.cumsum([len(s) for s in spans])]).astype(np.int32)

    def put(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    label, iou, own = K.tag_name_proposals(put(np.concatenate(spans)), put(glabel), put(g_off), put(np.concatenate(props)),
                                           put(p_off), thresh)
    label, iou, own = label.cpu().numpy(), iou.cpu().numpy(), own.cpu().numpy()
    out = []
    for i, p in enumerate(props):
        sl = slice(p_off[i], p_off[i + 1])
        out.append([(int(l), float(o), float(s), float(a), float(b))
                    for l, o, s, (a, b) in zip(label[sl], iou[sl], own[sl], p)])
    return out
