"""Actionness scoring of whole videos: stage 2 of the reference's workflow (/root/reference/binary_test.py:63-94, 160-172),
between training the classifier (``binary_model.BinaryClassifier``) and TAG (``tag_proposals``).

The reference runs the classifier's test path over every ``frame_interval``-th frame ("tick") of a video, ``num_crop`` crops
each, and writes ``{video id: float32 [T, num_crop, 2]}`` -- the score file ``gen_bottom_up_proposals.py`` reads.  Here the
backbone runs on ``tick_batch`` ticks per call whatever batching the frame source uses (``run_tick_batches``, the loop of
``DenseTester`` with the scoring step as a callback), and the scoring tail is one ``ssn_actionness_fc`` launch per backbone
call plus one ``ssn_actionness_group`` launch per video (csrc/actionness.hip).

What the reference's rows are
-----------------------------
``binary_test.py:87-91`` gets its frames from ``GroupOverSample`` + ``Stack`` in CROP-MAJOR order -- ``[crop][tick]``, 4 ticks
per generator batch (``load_binary_score.py:265``) -- but views the logits as ``view(-1, num_crop, D)``, i.e. as if they
were tick-major (``ssn_test.py:84`` does it right with ``view(num_crop, -1, D)``).  Row ``i`` of its file is therefore NOT the
ten crops of tick ``i``: it is ten consecutive entries of the crop-major list of its batch of four, and after TAG's
``.mean(axis=1)`` every "tick" is a near-uniform blend of the four ticks of its batch.  The published TAG thresholds were
tuned on such files, so both groupings exist:

* ``grouping="reference"`` (default): the file equals what ``binary_test.py`` writes, row for row.  With ``g = ref_batch``
  (``gen_batchsize``, 4), ``q = i // g``, ``b = min(g, T - g*q)`` and ``r = (i - g*q) * num_crop + j``, row ``i`` slot ``j``
  holds the logits of crop ``r // b`` of tick ``g*q + r % b``.
* ``grouping="tick"``: row ``i`` really is the crops of tick ``i``.

Scope: RGB and Flow on BNInception / InceptionV3, as everywhere else; RGBDiff stays NotImplementedError (the reference's own
``BinaryClassifier`` cannot be constructed for it, binary_model.py:49 calls a method that does not exist).
"""
import pickle

import torch

from . import kernels as K


@torch.no_grad()
def run_tick_batches(net, frames_gen, frame_cnt, num_crop, length, tick_batch, max_keep_bytes, score):
    """The per-video loop of ``DenseTester.frame_scores`` (dense_test.py) with the scoring step as a callback: crop-major frame
    batches of any tick count are re-packed to ``tick_batch`` ticks per backbone call and handed to
    ``score(x, first tick, ticks)``.  The range guard of the backbone's delayed scales is polled once per video, as DenseTester
    does: every call leaves its fault word in a per-call slot, its input stays referenced, and after the last call one host read
    says which calls have to be scored again.  -> the number of repeated calls.  Raises ValueError on a batch that is not a
    multiple of ``num_crop`` images and when the ticks delivered differ from ``frame_cnt``."""
    dev = net.test_fc.weight.device
    cnt = 0
    repeated = 0
    pending, pending_ticks = [], 0
    bm = net.base_model
    lag = {"on": (getattr(bm, "scale_guard", "") == "sync" and dev.type == "cuda" and getattr(bm, "layout", "") == "planes"),
           "kept": [], "marks": [], "bytes": 0}
    word = bm.planes_flag(dev)[0:1] if lag["on"] else None
    # the fault word is shared by every user of the backbone on this device (a graph owner polls it): what it held before this video
    # is put back at the end -- the tester only ever clears what its own calls set
    prior = word.clone() if lag["on"] else None
    keep_cap = max_keep_bytes
    if keep_cap is None:
        keep_cap = min(24 << 30, torch.cuda.mem_get_info(dev)[0] // 2) if dev.type == "cuda" else 0

    def flush():
        nonlocal cnt, pending, pending_ticks
        if not pending:
            return
        # re-pack crop-major sub-batches [crop][tick] into one crop-major batch
        if len(pending) == 1:
            x = pending[0]
        else:
            x = torch.cat([p.reshape((num_crop, -1) + tuple(p.shape[1:])) for p in pending], dim=1)
            x = x.reshape((-1,) + tuple(pending[0].shape[1:]))
        x = x.contiguous()
        if lag["on"] and lag["bytes"] + x.numel() * x.element_size() > keep_cap:
            lag["on"] = False                                           # (a very long video: poll call by call from here on)
        if lag["on"]:
            bm.scale_guard = "deferred"                                 # the call launches its range check, polls nothing
            try:
                score(x, cnt, pending_ticks)
            finally:
                bm.scale_guard = "sync"
            lag["marks"].append(word.clone())                           # this call's fault word (device-side copy, no sync)
            word.zero_()
            lag["kept"].append((x, cnt, pending_ticks))
            lag["bytes"] += x.numel() * x.element_size()
        else:
            score(x, cnt, pending_ticks)
        cnt += pending_ticks
        pending, pending_ticks = [], 0

    for frames in frames_gen:
        x = frames.to(dev, non_blocking=True).reshape((-1, length) + tuple(frames.shape[-2:]))
        if x.shape[0] % num_crop:
            raise ValueError("a frame batch of %d images is not a multiple of %d crops" % (x.shape[0], num_crop))
        pending.append(x)
        pending_ticks += x.shape[0] // num_crop
        if pending_ticks >= tick_batch:
            flush()
    flush()
    if lag["marks"]:
        bad = [i for i, v in enumerate(torch.cat(lag["marks"]).tolist()) if v]      # the one host read of the video
        for i in bad:                                                   # repeat exactly the calls that left their range
            repeated += 1
            score(*lag["kept"][i])                                      # (sync guard: repairs itself)
    if prior is not None:
        torch.maximum(word, prior, out=word)
    if cnt != frame_cnt:
        raise ValueError("the frame source gave %d ticks, expected %d" % (cnt, frame_cnt))
    return repeated


class ActionnessScores(object):
    """The scores of a set of videos, on the device: ``raw[vid]`` float32 [T, crops, C] (the rows of the score file) and
    ``mean[vid]`` float32 [T, C] (their crop mean, what ``tag_proposals.merge_scores_device`` and
    ``TagProposalGenerator.generate`` take)."""

    def __init__(self):
        self.raw = {}
        self.mean = {}

    def __len__(self):
        return len(self.raw)

    def to_host(self):
        """-> {video id: float32 numpy [T, crops, C]}, the dictionary binary_test.py collects (:160-163)."""
        return {k: v.cpu().numpy() for k, v in self.raw.items()}

    def save(self, path):
        """The reference's score file: the dictionary of ``to_host`` pickled with protocol 2 (binary_test.py:168-172)."""
        with open(path, "wb") as f:
            pickle.dump(self.to_host(), f, 2)


class ActionnessTester(object):
    """``net``: a ``BinaryClassifier(..., test_mode=True)`` with ``prepare_test_fc()`` done, in eval mode, on a HIP device.
    ``grouping``: ``"reference"`` (the rows binary_test.py writes, see the module docstring) or ``"tick"``; ``ref_batch``:
    the ticks per generator batch the reference's rows are formed over (``gen_batchsize`` of load_binary_score.py:265)."""

    def __init__(self, net, tick_batch=32, grouping="reference", ref_batch=4, max_keep_bytes=None):
        if net.test_fc is None:
            raise RuntimeError("call net.prepare_test_fc() first (binary_test.py:70)")
        if grouping not in ("reference", "tick"):
            raise ValueError("grouping must be 'reference' or 'tick', got %r" % (grouping,))
        if grouping == "reference" and int(ref_batch) < 1:
            raise ValueError("the reference grouping needs ref_batch >= 1")
        if net.modality not in ("RGB", "Flow"):
            raise NotImplementedError("only RGB and Flow are scored")
        self.net = net
        self.tick_batch = int(tick_batch)
        self.grouping = grouping
        self.ref_batch = int(ref_batch) if grouping == "reference" else 0
        self.output_dim = net.test_fc.out_features
        self.length = (3 if net.modality == "RGB" else 2) * net.new_length      # binary_test.py:78-82
        self.max_keep_bytes = max_keep_bytes
        self.repeated_calls = 0             # backbone calls the once-per-video poll had to repeat

    @torch.no_grad()
    def score_video(self, frames_gen, frame_cnt, num_crop=10):
        """-> (raw [frame_cnt, num_crop, C], mean [frame_cnt, C]) on the device.  ``frames_gen`` yields crop-major frame
        batches of any tick count (``[num_crop * b, length, H, W]`` or anything that views to it), as
        load_binary_score.get_test_data does."""
        fc = self.net.test_fc
        dev = fc.weight.device
        raw_true = torch.empty((frame_cnt, num_crop, self.output_dim), device=dev, dtype=torch.float32)
        w, b = fc.weight.detach().contiguous(), fc.bias.detach().contiguous()

        def score(x, tick0, ticks):
            if tick0 + ticks > frame_cnt:                                   # (before anything is written behind the staging tensor)
                raise ValueError("the frame source gave more than the %d ticks expected" % frame_cnt)
            base = self.net._backbone(x)                                    # [num_crop * ticks, feat], crop-major
            K.actionness_fc(base.contiguous(), w, b, raw_true, tick0, num_crop)

        self.repeated_calls += run_tick_batches(self.net, frames_gen, frame_cnt, num_crop, self.length, self.tick_batch,
                                                self.max_keep_bytes, score)
        return K.actionness_group(raw_true, self.ref_batch)

    def score_videos(self, items):
        """``items`` yields ``(video id, frames_gen, frame_cnt)`` or ``(video id, frames_gen, frame_cnt, num_crop)``
        -> ActionnessScores."""
        out = ActionnessScores()
        for item in items:
            vid, gen, cnt = item[0], item[1], item[2]
            raw, mean = self.score_video(gen, cnt, *item[3:4])
            out.raw[vid], out.mean[vid] = raw, mean
        return out
