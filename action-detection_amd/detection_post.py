"""Detections of one video from the tester's outputs: the per-video part of the reference's evaluation script
(/root/reference/eval_detection_results.py:91-178 with ops/utils.py:56-82) in one GPU call.

Input = what ``ssn_test.py:92`` puts on the result queue (``DenseTester.score_video``): relative proposal spans,
activity / completeness / regression scores.  Output = ``{class: array [n, 5]}`` of (start, end, score, loc, dur)
after score fusion, the optional top-k over all (proposal, class) pairs, per-class temporal NMS and location
regression, in the reference's order (descending score) -- the rows ``dataset_detections[cls][video_id]`` holds
before they are handed to the ActivityNet toolkit.  ``video_cls_score`` selects the ``--cls_scores`` branch (:130-144):
detections only for the ``cls_top_k`` classes an external video-level classifier ranks highest, every proposal kept,
fused score from the raw class scores (or their softmax with ``softmax_before_filter``).
"""
import numpy as np
import torch

from . import kernels as K


class DetectionPostProcessor(object):
    def __init__(self, num_class, nms_threshold, top_k=0, no_regression=False, cls_top_k=1, softmax_before_filter=False):
        self.num_class = num_class
        self.nms_threshold = float(nms_threshold)
        self.top_k = int(top_k) if top_k else 0
        self.no_regression = bool(no_regression)
        self.cls_top_k = int(cls_top_k)                              # --cls_top_k (default 1, :32)
        self.softmax_before_filter = bool(softmax_before_filter)     # --softmax_before_filter (:28)

    def _run(self, rel_prop, act_scores, comp_scores, reg_scores, device, video_cls_score):
        """-> (combined, dets [C, n_max, 5], counts [C]) on the device and the classes that are reported."""
        dev = torch.device(device) if device is not None else act_scores.device

        def f32(t):
            return (t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))).to(dev, torch.float32).contiguous()
        rp = (rel_prop if torch.is_tensor(rel_prop) else torch.as_tensor(np.asarray(rel_prop)))
        rp = rp.reshape(-1, 2).to(dev, torch.float64).contiguous()        # (1, P, 2) in the pickles: squeezed, :93-96
        act, comp = f32(act_scores), f32(comp_scores)
        reg = None if reg_scores is None else f32(reg_scores).reshape(-1, self.num_class, 2)
        # top_k <= 0: softmax over all C+1 activity scores (:98); top_k > 0: over the C class scores (:113)
        if video_cls_score is not None:
            # every (proposal, class) pair is a candidate (top_k plays no role in this branch, :130-144); the classes the
            # external classifier does not rank among its cls_top_k best are dropped from the result
            mode = 1 if self.softmax_before_filter else 2
            combined, dets, counts = K.detections(act, comp, reg, rp, 0, mode, self.nms_threshold, not self.no_regression)
            vs = np.asarray(video_cls_score.detach().cpu() if torch.is_tensor(video_cls_score) else video_cls_score).reshape(-1)
            assert vs.shape[0] == self.num_class
            # the reference's own expression (eval_detection_results.py:137: default-kind np.argsort): with exact ties in the
            # classifier's scores the same numpy picks the same classes
            classes = sorted(int(c) for c in np.argsort(vs,)[-self.cls_top_k:])
        else:
            combined, dets, counts = K.detections(act, comp, reg, rp, self.top_k, self.top_k <= 0, self.nms_threshold,
                                                  not self.no_regression)
            classes = range(self.num_class)
        return combined, dets, counts, classes

    @torch.no_grad()
    def process_video(self, rel_prop, act_scores, comp_scores, reg_scores=None, device=None, video_cls_score=None):
        """video_cls_score: the [C] scores of this video from the external classifier's pickle (``--cls_scores``), or None."""
        combined, dets, counts, classes = self._run(rel_prop, act_scores, comp_scores, reg_scores, device, video_cls_score)
        counts = counts.cpu().numpy()
        dets = dets.cpu().numpy()
        return {c: dets[c, :counts[c]].copy() for c in classes if counts[c] > 0}, combined

    @torch.no_grad()
    def process_video_device(self, rel_prop, act_scores, comp_scores, reg_scores=None, device=None, video_cls_score=None):
        """The same detections WITHOUT the copy to the host: -> ((dets [C, n_max, 5] float64, counts [C] int32), combined),
        all on the device; class c's rows are ``dets[c, :counts[c]]``.  In the ``--cls_scores`` branch the counts of the
        classes that are not reported are zero.  ``detection_eval.DetectionEvaluator.add_video`` takes the pair as it is."""
        combined, dets, counts, classes = self._run(rel_prop, act_scores, comp_scores, reg_scores, device, video_cls_score)
        if video_cls_score is not None:
            mask = torch.zeros(self.num_class, dtype=counts.dtype)
            mask[list(classes)] = 1
            counts = counts * mask.to(counts.device)
        return (dets, counts), combined

    @torch.no_grad()
    def process_videos(self, videos, device=None, video_cls_scores=None):
        """All videos in one pass (csrc/detect_batch.hip): the detections ``process_video`` gives video by video, bit for bit,
        as flat compact rows on the device; launches, allocations and transfers do not depend on the number of videos.

        videos: a dict ``{video id: (rel_prop, act, comp, reg)}`` (a score pickle) or a list of such pairs; the parts are
        numpy arrays as in the pickles (rel_prop may be ``(1, P, 2)``) or tensors; P = 0 is allowed; reg is None for all
        videos or for none.  Host parts are concatenated once and go up as one copy per part.  video_cls_scores: ``{video
        id: [C] scores}`` of the external classifier (the ``--cls_scores`` branch), or None.  -> BatchedDetections."""
        items = list(videos.items()) if isinstance(videos, dict) else [(v, parts) for v, parts in videos]
        if not items:
            raise ValueError("process_videos: no video")
        c = self.num_class
        ids, sizes, parts = [], [], ([], [], [], [])
        for vid, (rel_prop, act, comp, reg) in items:
            shapes = [tuple(x.shape) if x is not None else None for x in (rel_prop, act, comp, reg)]
            p = shapes[2][0] if len(shapes[2]) == 2 else -1
            if len(shapes[2]) != 2 or shapes[2][1] != c:
                raise ValueError("video %r: completeness scores must be [P, %d], got %r" % (vid, c, shapes[2]))
            if shapes[1] != (p, c + 1):
                raise ValueError("video %r: activity scores must be [%d, %d], got %r" % (vid, p, c + 1, shapes[1]))
            if int(np.prod(shapes[0])) != 2 * p or (p and shapes[0][-1] != 2):
                raise ValueError("video %r: %d proposals need spans [%d, 2], got %r" % (vid, p, p, shapes[0]))
            if reg is not None and int(np.prod(shapes[3])) != 2 * p * c:
                raise ValueError("video %r: regression scores must be [%d, %d, 2], got %r" % (vid, p, c, shapes[3]))
            if (reg is None) != (items[0][1][3] is None):
                raise ValueError("regression scores must be given for all videos or for none (video %r)" % (vid,))
            ids.append(vid)
            sizes.append(p)
            for dst, x in zip(parts, (rel_prop, act, comp, reg)):
                dst.append(x)
        K.detections_batch_check_sizes(sum(sizes), len(sizes), c)          # on shapes alone: nothing was copied yet
        tensors = [x for part in parts for x in part if torch.is_tensor(x)]
        dev = torch.device(device) if device is not None else (tensors[0].device if tensors else None)
        if dev is None:
            raise ValueError("process_videos: no device given and no part is a tensor")

        def gather(part, dtype, shape):
            """The videos' arrays one after the other on the device: host parts in one concatenation and one copy."""
            if all(not torch.is_tensor(x) or x.device.type == "cpu" for x in part):
                # concatenated and rounded to the kernels' type in one pass over the host arrays (the merged pickles are
                # float64; the rounding is the one `.to(float32)` does), so that the copy moves no more than is used
                arrs = [(x.numpy() if torch.is_tensor(x) else np.asarray(x)).reshape(shape) for x in part]
                buf = torch.empty((sum(len(x) for x in arrs),) + arrs[0].shape[1:], dtype=dtype)
                if len(buf):
                    np.concatenate(arrs, out=buf.numpy(), casting="unsafe")
                return buf.to(dev)
            return torch.cat([(x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(dev).reshape(shape)
                              for x in part]).to(dev, dtype).contiguous()
        rel = gather(parts[0], torch.float64, (-1, 2))
        act = gather(parts[1], torch.float32, (-1, c + 1))
        comp = gather(parts[2], torch.float32, (-1, c))
        reg = None if parts[3][0] is None else gather(parts[3], torch.float32, (-1, c, 2))
        h_p_off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
        d_p_off = h_p_off.to(dev)
        report = None
        if video_cls_scores is not None:
            # the classes each video reports, by the reference's own expression as in _run; every pair of a reported class is
            # a candidate (top_k plays no role in this branch)
            mask = np.zeros((len(ids), c), dtype=np.uint8)
            for i, vid in enumerate(ids):
                vs = video_cls_scores[vid]
                vs = np.asarray(vs.detach().cpu() if torch.is_tensor(vs) else vs).reshape(-1)
                if vs.shape[0] != c:
                    raise ValueError("video %r: %d classifier scores for %d classes" % (vid, vs.shape[0], c))
                mask[i, np.argsort(vs,)[-self.cls_top_k:]] = 1
            report = torch.from_numpy(mask).to(dev)
            top_k, mode = 0, (1 if self.softmax_before_filter else 2)
        else:
            top_k, mode = self.top_k, int(self.top_k <= 0)
        combined, kept, row_off = K.detections_batch(act, comp, rel, h_p_off, d_p_off, report, top_k, mode, self.nms_threshold)
        n = int(row_off[-1])                                              # the one sizing read
        rows, cls, vid, prop = K.detections_batch_fill(rel, combined, reg, d_p_off, kept, row_off, n, not self.no_regression)
        return BatchedDetections(rows, cls, vid, prop, row_off, combined, d_p_off, ids, c)


class BatchedDetections(object):
    """The detections of a batch of videos as flat rows on the device, in the order video (as given), class ascending,
    descending score (equal scores: higher proposal index first): rows [N, 5] float64 = (start, end, score, loc, dur), cls /
    vid / prop [N] int32 (vid: index into video_ids; prop: the proposal's index inside its video), row_off [V * C + 1] int32
    (the rows of class c of video v are row_off[v * C + c] : row_off[v * C + c + 1]), combined [sum P, C] float32 (the
    fused scores of all videos one after the other), p_off [V + 1] int32.  ``DetectionEvaluator.add_batch`` takes it as it is."""

    def __init__(self, rows, cls, vid, prop, row_off, combined, p_off, video_ids, num_class):
        self.rows, self.cls, self.vid, self.prop = rows, cls, vid, prop
        self.row_off, self.combined, self.p_off = row_off, combined, p_off
        self.video_ids = list(video_ids)
        self.num_class = int(num_class)

    def __len__(self):
        return len(self.video_ids)

    def to_host(self):
        """-> ``{video id: {class: rows [n, 5]}}``: per video what ``process_video`` returns first."""
        rows, off, c = self.rows.cpu().numpy(), self.row_off.cpu().numpy(), self.num_class
        out = {}
        for i, vid in enumerate(self.video_ids):
            o = off[i * c:(i + 1) * c + 1]
            out[vid] = {k: rows[o[k]:o[k + 1]].copy() for k in range(c) if o[k + 1] > o[k]}
        return out

    def video(self, i):
        """-> (dets [C, n_max, 5], counts [C]) of the i-th video, in the padded form of ``process_video_device``."""
        c = self.num_class
        off = self.row_off[i * c:(i + 1) * c + 1].to(torch.int64)
        p = self.p_off[i:i + 2].cpu()
        dets = torch.zeros((c, max(1, int(p[1] - p[0])), 5), device=self.rows.device, dtype=torch.float64)
        lo, hi = int(off[0]), int(off[-1])
        cls = self.cls[lo:hi].to(torch.int64)
        dets[cls, torch.arange(lo, hi, device=self.rows.device) - off[cls]] = self.rows[lo:hi]
        return dets, (off[1:] - off[:-1]).to(torch.int32)
