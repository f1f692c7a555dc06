"""The training loops of the reference (/root/reference/ssn_train.py:150-370, binary_train.py:127-270) on the library's pieces:
epoch schedule, ``train`` / ``validate``, meters and checkpoints.

What differs from the reference is where the per-step bookkeeping runs.  Its loop reads seven scalars per step (``.data[0]``),
calls ``accuracy()`` three times and clips with a host read of the norm.  Here

* ``StepMeters.update`` is one launch (``ssn_step_meters``) that keeps every ``AverageMeter`` in a float64 state on the device --
  bit for bit the values ``accuracy()`` + ``AverageMeter.update(x.item(), n)`` compute;
* ``optim.clip_grad_norm_device`` leaves the norm and the gradient scale on the device (``ssn_sumsq_multi``);
* ``SSNSGD.step(grad_scale_dev=)`` applies that scale inside the update.

The host reads the meters only when it prints (``print_freq``) -- ``StepMeters.read()`` is the only synchronisation of a step.
"""
import math
import os
import shutil
import time
from collections import OrderedDict, namedtuple

import torch

from . import kernels as K
from . import optim as O
from .ops.ssn_ops import ActivityLoss, SSNObjective

Meter = namedtuple("Meter", "val avg sum count")
ACC_NAMES = ("act_acc", "fg_acc", "bg_acc")


class StepMeters(object):
    """The ``AverageMeter`` s of one loop, on the device.  ``names``: the loss meters (at most 4), in the order of the ``losses``
    tensor ``update`` receives; three accuracy meters follow: ``act_acc`` (top-1 over all rows), ``fg_acc`` (even rows -- the
    reference's ``view(-1, 2, C)[:, 0]``), ``bg_acc`` (odd rows).

    State (float64, ``4 * (len(names) + 3) + 1`` words): per meter ``sum`` (sum of val * n), ``count`` (sum of n), ``last_num``
    (val * n of the last update) and ``last_den`` (its n), then the number of skipped updates.  ``val = last_num / last_den``
    returns the fp32 value of the last update exactly; every word is additive over ranks (``reduce_``)."""

    def __init__(self, names, device):
        self.names = tuple(names)
        if len(self.names) > 4:
            raise ValueError("at most 4 loss meters")
        self.device = torch.device(device)
        self.state = torch.zeros(4 * (len(self.names) + 3) + 1, dtype=torch.float64, device=self.device)

    def update(self, logits, target, losses, loss_weight, skip_flag=None):
        """One launch, no host read.  logits fp32 [rows, cols] (rows even: FG / BG pairs), target int64 [rows], losses fp32
        [len(names)] on the device, loss_weight the ``n`` of the loss meters (the loops pass ``out_frames.size(0)``).  While
        skip_flag (device int32) reads non-zero only the ``skipped`` counter moves: a step flagged by the range guard is redone."""
        K.step_meters(logits, target, losses if self.names else None, loss_weight, self.state, skip_flag)

    def reset(self):
        self.state.zero_()

    def reduce_(self, group=None):
        """One SUM all-reduce of the state over the ranks: a global ``val`` / ``avg`` is then the n-weighted mean over the ranks."""
        import torch.distributed as dist
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        return self

    def read(self):
        """The only host read: ``{name: Meter(val, avg, sum, count)}`` plus ``skipped``."""
        s = self.state.cpu().tolist()
        out = OrderedDict()
        for i, name in enumerate(self.names + ACC_NAMES):
            total, count, num, den = s[4 * i:4 * i + 4]
            out[name] = Meter(num / den if den else 0.0, total / count if count else 0.0, total, count)
        out["skipped"] = int(s[-1])
        return out


class _Clock(object):
    """The reference's batch_time / data_time meters (host clocks; nothing to do with the device)."""

    def __init__(self):
        self.val = self.avg = self.sum = 0.0
        self.count = 0

    def update(self, val):
        self.val = val
        self.sum += val
        self.count += 1
        self.avg = self.sum / self.count


class _TrainerBase(object):
    loss_names = ()

    def __init__(self, model, optimizer, lr_steps=(), iter_size=1, clip_gradient=None, print_freq=20, reducer=None, log=print):
        self.model, self.optimizer = model, optimizer
        self.lr_steps, self.iter_size, self.clip_gradient = list(lr_steps), int(iter_size), clip_gradient
        self.print_freq, self.reducer, self.log = int(print_freq), reducer, log
        self.device = next(model.parameters()).device
        self.meters = StepMeters(self.loss_names, self.device)
        self.val_meters = StepMeters(self.loss_names, self.device)
        self._params = [p for g in optimizer.param_groups for p in g["params"]]
        # out[0] = norm, out[1] = gradient scale; without clipping and with iter_size 1 the update takes the host scale 1.0
        self._clip_out = torch.empty(2, dtype=torch.float32, device=self.device)
        self._clip_ws = torch.empty(O.clip_workspace_floats(self._params), dtype=torch.float32, device=self.device)
        self._loss_buf = torch.empty(len(self.loss_names), dtype=torch.float32, device=self.device)

    # -- what a subclass states: forward of one batch -> (logits, target, loss, losses tensor, loss_weight)
    def _forward(self, batch):
        raise NotImplementedError

    def _fault_flag(self):
        fn = getattr(self.model, "scale_fault_flag", None)
        return fn() if fn is not None else None

    def _optimizer_step(self):
        """ssn_train.py:238-253: gradients times 1 / iter_size, clipping, step, zero_grad -- the scale is applied inside the update."""
        flag = self._fault_flag()
        if self.reducer is not None:
            self.reducer.reduce_heads()
            if flag is not None:
                self.reducer.agree_flag_(flag)      # all ranks skip a flagged step together
        pre = 1.0 / self.iter_size
        if self.clip_gradient is not None:
            out = O.clip_grad_norm_device(self._params, self.clip_gradient, pre, self._clip_out, self._clip_ws)
            self.optimizer.step(grad_scale_dev=out[1:], skip_flag=flag)
        else:
            self.optimizer.step(grad_scale=pre, skip_flag=flag)
        self.optimizer.zero_grad(set_to_none=True)

    def train_epoch(self, batches, epoch, num_batches=None):
        batch_time, data_time = _Clock(), _Clock()
        self.meters.reset()
        self.model.train()
        self.optimizer.adjust_learning_rate(epoch, self.lr_steps)
        if num_batches is None:
            num_batches = len(batches) if hasattr(batches, "__len__") else 0
        end = time.time()
        self.optimizer.zero_grad(set_to_none=True)
        for i, batch in enumerate(batches):
            data_time.update(time.time() - end)
            logits, target, loss, losses, weight = self._forward(batch)
            self.meters.update(logits, target, losses, weight, self._fault_flag())
            loss.backward()
            if i % self.iter_size == 0:
                self._optimizer_step()
            batch_time.update(time.time() - end)
            end = time.time()
            if self.print_freq > 0 and i % self.print_freq == 0:
                self.log(self.train_line(epoch, i, num_batches, batch_time, data_time, self.meters.read()))
        return self.meters

    def validate(self, batches, num_batches=None):
        batch_time = _Clock()
        self.val_meters.reset()
        self.model.eval()
        if num_batches is None:
            num_batches = len(batches) if hasattr(batches, "__len__") else 0
        end = time.time()
        with torch.no_grad():
            for i, batch in enumerate(batches):
                logits, target, _, losses, weight = self._forward(batch)
                self.val_meters.update(logits, target, losses, weight)
                batch_time.update(time.time() - end)
                end = time.time()
                if self.print_freq > 0 and i % self.print_freq == 0:
                    self.log(self.test_line(i, num_batches, batch_time, self.val_meters.read()))
        if self.reducer is not None and self.reducer.world > 1:
            self.val_meters.reduce_(self.reducer.group)
        m = self.val_meters.read()
        self.log(self.summary_line(m))
        return m["loss"].avg


class SSNTrainer(_TrainerBase):
    """``train`` / ``validate`` of /root/reference/ssn_train.py:172-362 for an ``SSN`` (any module returning its 7-tuple).

    ``batches`` yield the five arguments of ``SSN.forward`` -- (input, aug_scaling, target, reg_target, prop_type), what
    ``TrainingBatchPrefetcher`` emits -- or the seven fields of the reference's loader.  ``sample_split`` / ``sample_group_size`` are
    the loop's ``ohem_num`` / ``comp_group_size`` (fg_per_video, fg_per_video + incomplete_per_video).  With a ``reducer``
    (``GradReducer``) the head gradients are averaged, the completeness loss takes the global denominator and the fault word of the
    range guard is agreed on before the optimizer runs."""
    loss_names = ("loss", "act_loss", "comp_loss", "reg_loss")

    def __init__(self, model, optimizer, objective=None, sample_split=1, sample_group_size=7, **kw):
        super(SSNTrainer, self).__init__(model, optimizer, **kw)
        self.objective = objective if objective is not None else SSNObjective()
        self.sample_split, self.sample_group_size = sample_split, sample_group_size

    def _forward(self, batch):
        if len(batch) == 7:      # the reference loader's order (ssn_train.py:191-192)
            frames, _, scaling, prop_type, labels, reg_targets, _ = batch
            batch = (frames, scaling, labels, reg_targets, prop_type)
        batch = tuple(t.to(self.device) for t in batch)
        out = self.model(*batch)
        global_rows = None
        if self.reducer is not None and self.reducer.world > 1:
            global_rows = out[2].reshape(-1, out[2].size(-1)).size(0) * self.reducer.world
        loss = self.objective(*out, sample_split=self.sample_split, sample_group_size=self.sample_group_size,
                              global_rows=global_rows)
        # total / act / comp / reg, the order of the meters (parts = act, comp, reg)
        torch.cat([loss.detach().reshape(1), self.objective.parts], out=self._loss_buf)
        return out[0], out[1], loss, self._loss_buf, batch[0].size(0)

    def train_line(self, epoch, i, n, batch_time, data_time, m):
        # (ssn_train.py:272 prints bg_acc.avg twice; val (avg) here)
        return ('Epoch: [{0}][{1}/{2}], lr: {lr:.5f}\t'
                'Time {bt.val:.3f} ({bt.avg:.3f})\t'
                'Data {dt.val:.3f} ({dt.avg:.3f})\t'
                'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                'Act. Loss {act.val:.3f} ({act.avg: .3f}) \t'
                'Comp. Loss {comp.val:.3f} ({comp.avg: .3f}) '
                '\tReg. Loss {reg.val:.3f} ({reg.avg:.3f})'
                '\n Act. FG {fg.val:.02f} ({fg.avg:.02f}) Act. BG {bg.val:.02f} ({bg.avg:.02f})').format(
                    epoch, i, n, lr=self.optimizer.param_groups[0]['lr'], bt=batch_time, dt=data_time, loss=m["loss"],
                    act=m["act_loss"], comp=m["comp_loss"], reg=m["reg_loss"], fg=m["fg_acc"], bg=m["bg_acc"])

    def test_line(self, i, n, batch_time, m):
        return ('Test: [{0}/{1}]\t'
                'Time {bt.val:.3f} ({bt.avg:.3f})\t'
                'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                'Act. Loss {act.val:.3f} ({act.avg:.3f})\t'
                'Comp. Loss {comp.val:.3f} ({comp.avg:.3f})\t'
                'Act. Accuracy {acc.val:.02f} ({acc.avg:.2f}) FG {fg.val:.02f} BG {bg.val:.02f}'
                '\tReg. Loss {reg.val:.3f} ({reg.avg:.3f})').format(
                    i, n, bt=batch_time, loss=m["loss"], act=m["act_loss"], comp=m["comp_loss"], acc=m["act_acc"],
                    fg=m["fg_acc"], bg=m["bg_acc"], reg=m["reg_loss"])

    def summary_line(self, m):
        return ('Testing Results: Loss {loss.avg:.5f} \t '
                'Activity Loss {act.avg:.3f} \t '
                'Completeness Loss {comp.avg:.3f}\n'
                'Act Accuracy {acc.avg:.02f} FG Acc. {fg.avg:.02f} BG Acc. {bg.avg:.02f}'
                '\t Regression Loss {reg.avg:.3f}').format(
                    loss=m["loss"], act=m["act_loss"], comp=m["comp_loss"], acc=m["act_acc"], fg=m["fg_acc"], bg=m["bg_acc"],
                    reg=m["reg_loss"])


class BinaryTrainer(_TrainerBase):
    """``train`` / ``validate`` of /root/reference/binary_train.py:147-261 for a ``BinaryClassifier``: batches are
    ``(frames, prop_type)``, the loss is the cross entropy of the binary scores."""
    loss_names = ("loss",)

    def __init__(self, model, optimizer, criterion=None, **kw):
        super(BinaryTrainer, self).__init__(model, optimizer, **kw)
        self.criterion = criterion if criterion is not None else ActivityLoss()

    def _forward(self, batch):
        frames, prop_type = (t.to(self.device) for t in batch)
        score, target = self.model(frames, prop_type)
        loss = self.criterion(score, target)
        self._loss_buf.copy_(loss.detach().reshape(1))
        return score, target.contiguous().long(), loss, self._loss_buf, frames.size(0)

    def train_line(self, epoch, i, n, batch_time, data_time, m):
        return ('Epoch: [{0}][{1}/{2}], lr: {lr:.5f}\t'
                'Time {bt.val:.3f} ({bt.avg:.3f})\t'
                'Data {dt.val:.3f} ({dt.avg:.3f})\t'
                'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                '\n FG{fg.val:.02f}({fg.avg:.02f}) BG {bg.val:.02f} ({bg.avg:.02f})').format(
                    epoch, i, n, lr=self.optimizer.param_groups[0]['lr'], bt=batch_time, dt=data_time, loss=m["loss"],
                    fg=m["fg_acc"], bg=m["bg_acc"])

    def test_line(self, i, n, batch_time, m):
        return ('Test: [{0}/{1}]\t'
                'Time {bt.val:.4f} ({bt.avg:.4f})\t'
                'Loss {loss.val:.4f} ({loss.avg:.4f})\t'
                'FG {fg.val:.02f} BG {bg.val:.02f}').format(i, n, bt=batch_time, loss=m["loss"], fg=m["fg_acc"], bg=m["bg_acc"])

    def summary_line(self, m):
        return ('Testing Results: Loss {loss.avg:.5f} \t'
                'FG Acc. {fg.avg:.02f} BG Acc. {bg.avg:.02f}').format(loss=m["loss"], fg=m["fg_acc"], bg=m["bg_acc"])


# ------------------------------------------------------------------------------------------------------------ checkpoints
def checkpoint_names(kind, snapshot_pref, dataset, arch, modality, filename="checkpoint.pth.tar"):
    """File names of ``save_checkpoint`` (ssn_train.py:365-370, binary_train.py:265-270): kind 'ssn' / 'binaryclassifier'.
    -> (checkpoint, best copy).  The reference prepends the kind to the whole string; a ``snapshot_pref`` with a directory part
    keeps that directory here and the kind goes in front of the file name."""
    d, base = os.path.split(snapshot_pref)
    name = os.path.join(d, kind + "_".join((base, dataset, arch, modality.lower(), filename)))
    best = "_".join((snapshot_pref, modality.lower(), "model_best.pth.tar"))
    return name, best


def save_checkpoint(model, epoch, arch, best_loss, is_best, filename, best_filename, reg_stats=None):
    """The reference's dict -- {'epoch', 'arch', 'state_dict', 'best_loss'[, 'reg_stats']} -- with the ``module.`` prefix
    DataParallel gave its keys, so the reference's tester and ``--resume`` read the file (ssn_test.py:128).  Like the reference,
    optimizer state is not saved.  ``is_best`` is the loop's ``loss < best_loss``: the file is then copied to ``best_filename``."""
    state = OrderedDict(("module." + k, v.detach().cpu()) for k, v in model.state_dict().items())
    ckpt = {"epoch": epoch, "arch": arch, "state_dict": state, "best_loss": best_loss}
    if reg_stats is not None:
        ckpt["reg_stats"] = torch.as_tensor(reg_stats)
    torch.save(ckpt, filename)
    if is_best:
        shutil.copyfile(filename, best_filename)
    return filename


def load_checkpoint(filename, model=None, strict=True):
    """-> the checkpoint dict with ``state_dict`` keys stripped of ``module.`` (both forms are accepted); loads it into ``model``
    when given."""
    ckpt = torch.load(filename, map_location="cpu", weights_only=False)
    sd = ckpt["state_dict"]
    ckpt["state_dict"] = OrderedDict((k[len("module."):] if k.startswith("module.") else k, v) for k, v in sd.items())
    if model is not None:
        model.load_state_dict(ckpt["state_dict"], strict=strict)
    return ckpt


def fit(trainer, train_batches, val_batches, epochs, arch, names, start_epoch=0, best_loss=math.inf, eval_freq=5, reg_stats=None):
    """The epoch schedule of ssn_train.py:150-169 / binary_train.py:127-144.  ``train_batches`` / ``val_batches``: callables
    ``epoch -> iterable`` (a fresh pass per epoch).  ``names``: (checkpoint, best copy) from ``checkpoint_names``.  -> best_loss."""
    for epoch in range(start_epoch, epochs):
        trainer.train_epoch(train_batches(epoch), epoch)
        if (epoch + 1) % eval_freq == 0 or epoch == epochs - 1:
            loss = trainer.validate(val_batches(epoch))
            is_best = loss < best_loss
            best_loss = min(loss, best_loss)
            rank0 = True
            if trainer.reducer is not None:
                import torch.distributed as dist
                rank0 = dist.get_rank(trainer.reducer.group) == 0
            if rank0:
                d = os.path.dirname(names[0])
                if d:
                    os.makedirs(d, exist_ok=True)
                save_checkpoint(trainer.model, epoch + 1, arch, best_loss, is_best, names[0], names[1], reg_stats)
    return best_loss
