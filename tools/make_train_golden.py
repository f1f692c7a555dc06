#!/usr/bin/env python
"""Generate tests/golden/ref_train_meters.npz: what the REFERENCE's own ``accuracy`` and ``AverageMeter`` make of seeded logits,
targets and losses when they are driven as the loop of ssn_train.py:216-233 drives them (test infrastructure; runs only where the
reference tree exists, the fixture it writes is committed).

The two definitions are taken from binary_train.py by ``ast`` -- only those two, compiled from the file where it lies and run
here, nothing copied.  (ssn_train.py does not parse on a current Python -- ``async=True`` at :297 -- and its two definitions
differ from binary_train.py's in comments only.)

Per shape (rows, cols) the fixture holds STEPS steps of logits / targets / the four losses (total, act, comp, reg) and, after
every step, ``val`` / ``sum`` / ``count`` / ``avg`` of the seven meters in the order loss, act_loss, comp_loss, reg_loss, act_acc,
fg_acc, bg_acc.  No row has a tie for its maximum or a NaN (asserted): torch leaves the winner of a tie unspecified.
"""
import ast
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = ((2, 2), (8, 21), (10, 64), (6, 65), (130, 101), (64, 201))
STEPS = 6
LOSS_WEIGHT = 4          # out_frames.size(0) of the loop


def reference_definitions():
    path = os.path.join(REF, "binary_train.py")
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in ("accuracy", "AverageMeter")]
    assert sorted(n.name for n in body) == ["AverageMeter", "accuracy"]
    ns = {}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["accuracy"], ns["AverageMeter"]


def main():
    accuracy, AverageMeter = reference_definitions()
    out = {"shapes": np.array(SHAPES, np.int64), "loss_weight": np.array(LOSS_WEIGHT, np.int64)}
    for rows, cols in SHAPES:
        rs = np.random.RandomState(rows * 1000 + cols)
        logits = rs.standard_normal((STEPS, rows, cols)).astype(np.float32)
        targets = rs.randint(0, cols, (STEPS, rows)).astype(np.int64)
        hit = rs.uniform(size=(STEPS, rows)) < 0.6          # 60 % of the rows are classified correctly
        targets = np.where(hit, logits.argmax(-1), targets)
        losses = rs.uniform(0.05, 3.0, (STEPS, 4)).astype(np.float32)
        top2 = np.sort(logits, -1)[..., -2:] if cols > 1 else None
        assert not np.isnan(logits).any() and (top2 is None or (top2[..., 0] < top2[..., 1]).all()), "tie / NaN in a row"
        meters = [AverageMeter() for _ in range(7)]
        expected = np.zeros((STEPS, 7, 4), np.float64)
        for s in range(STEPS):
            act = torch.from_numpy(logits[s])
            tgt = torch.from_numpy(targets[s])
            loss_t = torch.from_numpy(losses[s])
            # ssn_train.py:216-233 (``.data[0]`` of a 0-dim tensor is ``.item()`` on a current torch)
            for k in range(4):
                meters[k].update(loss_t[k].item(), LOSS_WEIGHT)
            act_acc = accuracy(act, tgt)
            meters[4].update(act_acc[0].item(), act.size(0))
            fg_acc = accuracy(act.view(-1, 2, act.size(1))[:, 0, :].contiguous(), tgt.view(-1, 2)[:, 0].contiguous())
            bg_acc = accuracy(act.view(-1, 2, act.size(1))[:, 1, :].contiguous(), tgt.view(-1, 2)[:, 1].contiguous())
            meters[5].update(fg_acc[0].item(), act.size(0) // 2)
            meters[6].update(bg_acc[0].item(), act.size(0) // 2)
            for k, m in enumerate(meters):
                expected[s, k] = (m.val, m.sum, m.count, m.avg)
        tag = "r%d_c%d_" % (rows, cols)
        out[tag + "logits"], out[tag + "targets"], out[tag + "losses"], out[tag + "expected"] = logits, targets, losses, expected
    path = os.path.join(GOLDEN, "ref_train_meters.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
