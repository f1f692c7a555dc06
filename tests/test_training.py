"""The training loop's bookkeeping kernels (csrc/train_step.hip) and the loops built on them (training.py).

Kernel tests run through the ``backend`` fixture: the host emulator on the CPU tier, the real library with ``-m gpu``.
tests/golden/ref_train_meters.npz holds what the reference's own ``accuracy`` / ``AverageMeter`` compute
(tools/make_train_golden.py)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import action_detection_amd  # noqa: F401
from action_detection_amd import _lib
from action_detection_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -24          # unit roundoff of fp32
LOSS_NAMES = ("loss", "act_loss", "comp_loss", "reg_loss")
ALL_NAMES = LOSS_NAMES + ("act_acc", "fg_acc", "bg_acc")

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(GOLD, "ref_train_meters.npz")) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def bits(t):
    """float64 tensor -> its bit patterns (so that comparisons are exact, NaN and -0.0 included)"""
    return t.detach().cpu().contiguous().view(torch.int64).tolist()


# ------------------------------------------------------------------------------------------------------------------ meters
@pytest.mark.parametrize("rows,cols,pad", [(2, 2, 0), (8, 21, 0), (10, 64, 0), (6, 65, 0), (130, 101, 0), (64, 201, 0), (8, 21, 3)])
def test_step_meters_match_reference(backend, rows, cols, pad):
    """Every double of every meter after every step is bit-equal to the reference's accuracy() + AverageMeter.update(x.item(), n);
    one case reads rows that are cols + 3 elements apart."""
    from action_detection_amd.training import StepMeters
    g = golden()
    tag = "r%d_c%d_" % (rows, cols)
    logits, targets, losses, expected = (g[tag + k] for k in ("logits", "targets", "losses", "expected"))
    weight = int(g["loss_weight"])
    meters = StepMeters(LOSS_NAMES, backend.device)
    for s in range(logits.shape[0]):
        lg = torch.from_numpy(logits[s])
        if pad:
            wide = torch.full((rows, cols + pad), float("inf"))     # a kernel that read the padding would pick it
            wide[:, :cols] = lg
            lg = backend.put(wide)[:, :cols]
            assert lg.stride(0) == cols + pad
        else:
            lg = backend.put(lg)
        meters.update(lg, backend.put(torch.from_numpy(targets[s])), backend.put(torch.from_numpy(losses[s])), weight)
        m = meters.read()
        for k, name in enumerate(ALL_NAMES):
            val, total, count, avg = expected[s, k]
            got = m[name]
            assert (got.val, got.sum, got.count, got.avg) == (val, total, count, avg), (s, name, got, expected[s, k])
        assert m["skipped"] == 0
    meters.reset()
    assert meters.state.abs().sum().item() == 0


def test_step_meters_tie_and_nan_rule(backend):
    """The largest value wins, the lowest column among equals, NaN above every number, the first NaN taken; a target outside
    [0, cols) is a miss."""
    from action_detection_amd.training import StepMeters
    nan, inf = float("nan"), float("inf")
    rows = [
        ([1.0, 3.0, 3.0, 2.0], 1, True),        # tie: the lowest column
        ([1.0, 3.0, 3.0, 2.0], 2, False),
        ([0.0, nan, 5.0, nan], 1, True),        # NaN beats numbers, the first NaN
        ([0.0, nan, 5.0, nan], 3, False),
        ([nan, inf, 1.0, 0.0], 0, True),        # NaN in column 0 stays
        ([-inf, -inf, -inf, -inf], 0, True),    # all equal: column 0
        ([-0.0, 0.0, -1.0, -2.0], 0, True),     # -0.0 == 0.0: the lowest column
        ([1.0, 2.0, 3.0, inf], 3, True),
        ([1.0, 2.0, 3.0, 4.0], 4, False),       # target == cols: a miss, nothing read out of range
        ([4.0, 2.0, 3.0, 1.0], -1, False),      # negative target: a miss
    ]
    logits = backend.put(torch.tensor([r[0] for r in rows], dtype=torch.float32))
    target = backend.put(torch.tensor([r[1] for r in rows], dtype=torch.int64))
    hits = [r[2] for r in rows]
    meters = StepMeters((), backend.device)
    meters.update(logits, target, None, 1)
    m = meters.read()
    n = len(rows)
    f32 = np.float32
    assert m["act_acc"].val == float(f32(sum(hits)) * f32(100.0 / n))
    assert m["fg_acc"].val == float(f32(sum(hits[0::2])) * f32(100.0 / (n // 2)))
    assert m["bg_acc"].val == float(f32(sum(hits[1::2])) * f32(100.0 / (n // 2)))
    assert (m["act_acc"].count, m["fg_acc"].count, m["bg_acc"].count) == (n, n // 2, n // 2)


def test_step_meters_skip_flag(backend):
    """A raised skip_flag leaves the state bit-identical except the skipped counter; a cleared one counts the step."""
    from action_detection_amd.training import StepMeters
    g = golden()
    lg, tg, ls = (backend.put(torch.from_numpy(g["r8_c21_" + k][0])) for k in ("logits", "targets", "losses"))
    meters = StepMeters(LOSS_NAMES, backend.device)
    flag = backend.put(torch.zeros(1, dtype=torch.int32))
    meters.update(lg, tg, ls, 4, flag)
    before = bits(meters.state)
    flag.fill_(2)
    meters.update(lg, tg, ls, 4, flag)
    meters.update(lg, tg, ls, 4, flag)
    after = bits(meters.state)
    assert after[:-1] == before[:-1]
    assert meters.read()["skipped"] == 2 and meters.read()["loss"].count == 4
    flag.zero_()
    meters.update(lg, tg, ls, 4, flag)
    m = meters.read()
    assert m["skipped"] == 2 and m["loss"].count == 8 and m["act_acc"].count == 16


def test_step_meters_argument_errors(backend):
    """Odd or zero rows, cols < 1, null pointers and n_losses out of range fail before any launch."""
    lib = _lib.get_lib()
    dev = backend.device
    lg = torch.zeros((4, 3), dtype=torch.float32, device=dev)
    tg = torch.zeros(4, dtype=torch.int64, device=dev)
    ls = torch.zeros(4, dtype=torch.float32, device=dev)
    st = torch.zeros(29, dtype=torch.float64, device=dev)
    K.train_step_launches(reset=True)
    good = [lg.data_ptr(), 3, tg.data_ptr(), 4, 3, ls.data_ptr(), 4, 1.0, st.data_ptr(), None, None]

    def bad(**kw):
        args = list(good)
        for i, v in kw.items():
            args[int(i[1:])] = v
        with pytest.raises(RuntimeError, match="step_meters"):
            lib.call("ssn_step_meters", *args)
    bad(a3=3)               # odd rows
    bad(a3=0)               # no rows
    bad(a4=0)               # cols < 1
    bad(a0=None)            # null logits
    bad(a2=None)            # null target
    bad(a8=None)            # null state
    bad(a5=None)            # losses missing while n_losses > 0
    bad(a6=5)               # n_losses out of range
    bad(a6=-1)
    bad(a1=2)               # row_stride < cols
    with pytest.raises(RuntimeError, match="sumsq_multi"):
        lib.call("ssn_sumsq_multi", 1, None, None, None, 0, 1.0, 0.0, None, None)
    with pytest.raises(RuntimeError, match="sgd_step_multi_dev"):
        lib.call("ssn_sgd_step_multi_dev", 1, None, None, None, None, None, None, 0.9, None, 0, None, None)
    assert K.train_step_launches() == 0
    assert st.abs().sum().item() == 0


# ------------------------------------------------------------------------------------------------------------- sumsq_multi
LENGTHS = (1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5, 0)


def flat_views(count, device, seed=0):
    """`count` tensors of the LENGTHS (cycled) as views at ODD element offsets of one flat fp32 buffer (4-byte alignment only)."""
    rs = np.random.RandomState(seed)
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(count)]
    offs, o = [], 1
    for n in lens:
        offs.append(o)
        o += n + (2 if n % 2 == 0 else 1)        # keeps every offset odd
    flat = torch.from_numpy((rs.standard_normal(o + 1) * rs.uniform(0.1, 3.0)).astype(np.float32)).to(device)
    views = [flat[a:a + n] for a, n in zip(offs, lens)]
    assert all(a % 2 == 1 for a in offs)
    return flat, views


@pytest.mark.parametrize("count", [1, 48, 49, 100])
def test_sumsq_multi_norm(backend, count):
    """|norm - float64 norm| <= 32 * 2^-24 * norm.  A priori: with 4096-element blocks and 256 threads a term passes 16 + 6 + 2 fp32
    roundings (thread chain, wave butterfly, the four waves), the tail runs in double, then one rounding each for the square root's
    conversion and the pre_scale product -- 26, and the square root halves the relative error of the sum.  Two calls give the same
    bits; the launch count is ceil(count / 48) + 1 (groups that hold only empty tensors launch nothing)."""
    flat, views = flat_views(count, backend.device, seed=count)
    ref = math.sqrt(sum(float((v.double() ** 2).sum()) for v in views))
    K.train_step_launches(reset=True)
    out = K.sumsq_multi(views)
    groups = sum(1 for b in range(0, count, 48) if any(v.numel() for v in views[b:b + 48]))
    assert K.train_step_launches() == groups + 1 <= math.ceil(count / 48) + 1
    got = out.cpu()
    print("count %d: norm %.9g ref %.9g rel err %.3g (bound %.3g)" % (count, got[0], ref, abs(got[0].item() - ref) / ref, 32 * U))
    assert abs(got[0].item() - ref) <= 32 * U * ref
    assert got[1].item() == 1.0
    ws = torch.full((K.sumsq_multi_workspace_floats([v.numel() for v in views]),), float("nan"), device=backend.device)
    out2 = torch.empty(2, device=backend.device)
    assert K.sumsq_multi(views, out=out2, workspace=ws) is out2
    assert out2.cpu().view(torch.int32).tolist() == got.view(torch.int32).tolist()
    # pre_scale multiplies the norm (one more rounding is already in the bound)
    third = K.sumsq_multi(views, pre_scale=1.0 / 3).cpu()
    assert abs(third[0].item() - ref / 3) <= 32 * U * ref / 3
    assert third[1].item() == float(np.float32(1.0 / 3))


def test_sumsq_multi_scale(backend):
    """out[1] = pre_scale * c when c = max_norm / (out[0] + 1e-6) < 1, else pre_scale; max_norm = 0: no clipping; a NaN norm leaves
    the gradients unscaled.  Tolerance 4 * 2^-24 relative: the quotient, the sum and the product each round at most once in fp32."""
    flat, views = flat_views(10, backend.device, seed=5)
    f32 = np.float32

    def check(max_norm, pre):
        out = K.sumsq_multi(views, pre_scale=pre, max_norm=max_norm).cpu()
        norm = float(out[0])
        c = float(f32(max_norm)) / (norm + 1e-6)
        want = float(f32(pre)) * c if (max_norm > 0 and c < 1) else float(f32(pre))
        assert abs(float(out[1]) - want) <= 4 * U * want, (max_norm, pre, out, want)
        return norm, float(out[1])
    norm, s = check(0.0, 1.0)
    assert s == 1.0
    _, s = check(norm * 4, 1.0)          # above the norm: untouched
    assert s == 1.0
    _, s = check(norm / 4, 1.0)          # below: clipped
    assert 0.24 < s < 0.26
    n3, s = check(norm / 4, 1.0 / 3)     # iter_size 3: the norm of the averaged gradient decides
    assert abs(n3 - norm / 3) <= 2 * U * norm and 0.24 < s < 0.26
    _, s = check(norm / 2, 1.0 / 3)      # ... which max_norm = norm / 2 does not clip
    assert s == float(f32(1.0 / 3))
    flat[views[7].storage_offset() + 100] = float("nan")
    out = K.sumsq_multi(views, pre_scale=0.5, max_norm=1e-3).cpu()
    assert math.isnan(float(out[0])) and float(out[1]) == 0.5


# -------------------------------------------------------------------------------------------- SGD with the scale on the device
def test_sgd_step_device_scale_bit_identical(backend):
    """step(grad_scale_dev=tensor([s])) == step(grad_scale=s) in weights and momentum, bit for bit, over several steps and 50
    tensors (two launches), with the skip flag down and up."""
    from action_detection_amd.optim import SSNSGD
    dev = backend.device
    rs = np.random.RandomState(1)
    sizes = [LENGTHS[i % 8] for i in range(50)]

    def make():
        ps = [torch.nn.Parameter(torch.from_numpy(np.random.RandomState(i).standard_normal(n).astype(np.float32)).to(dev))
              for i, n in enumerate(sizes)]
        opt = SSNSGD([dict(params=ps[:20], lr_mult=1, decay_mult=1), dict(params=ps[20:], lr_mult=2, decay_mult=0)], lr=0.01)
        return ps, opt
    pa, oa = make()
    pb, ob = make()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for step, s in enumerate((1.0, 1.0 / 3, 0.37109375, 0.5)):
        grads = [torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev) for n in sizes]
        for p, q, g in zip(pa, pb, grads):
            p.grad, q.grad = g.clone(), g.clone()
        flag.fill_(1 if step == 2 else 0)
        before = [p.detach().clone() for p in pb]
        oa.step(grad_scale=float(np.float32(s)), skip_flag=flag)
        ob.step(grad_scale_dev=torch.tensor([s], dtype=torch.float32, device=dev), skip_flag=flag)
        for p, q, w0 in zip(pa, pb, before):
            assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
            assert torch.equal(oa.state[p]["momentum_buffer"].view(torch.int32), ob.state[q]["momentum_buffer"].view(torch.int32))
            if step == 2:
                assert torch.equal(q.detach(), w0)        # flagged: untouched
            elif q.numel():
                assert not torch.equal(q.detach(), w0)


# ---------------------------------------------------------------------------------------------------------------- trainer
NUM_CLASS, FEAT = 5, 12


class StubSSN(torch.nn.Module):
    """Head-only stand-in for SSN: per-proposal features in, the 7-tuple of SSN.forward out (rows as ssn_models.py:275-289 picks
    them: activity = fg + bg, completeness = fg + incomplete, regression = fg).  56 parameter tensors: two optimizer launches."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.activity_fc = torch.nn.Linear(FEAT, NUM_CLASS + 1)
        self.completeness_fc = torch.nn.Linear(FEAT, NUM_CLASS)
        self.regressor_fc = torch.nn.Linear(FEAT, 2 * NUM_CLASS)
        self.extras = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(3)) for _ in range(50)])
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        self.seen = []

    def forward(self, feat, scaling, target, reg_target, prop_type):
        v = feat.shape[0]
        shift = 0.01 * torch.stack(list(self.extras)).sum()
        act = self.activity_fc(feat[:, [0, 7]].reshape(2 * v, FEAT)) + shift
        comp = self.completeness_fc(feat[:, :7].reshape(7 * v, FEAT))
        reg = self.regressor_fc(feat[:, 0]).reshape(v, NUM_CLASS, 2)
        out = (act, target[:, [0, 7]].reshape(-1).contiguous(), comp, target[:, :7].reshape(-1).contiguous(), reg,
               target[:, 0].contiguous(), reg_target[:, 0].contiguous())
        self.seen.append((act.detach().clone(), out[1].clone()))
        return out

    def get_optim_policies(self):
        heads = [self.activity_fc, self.completeness_fc, self.regressor_fc]
        return [dict(params=[m.weight for m in heads] + list(self.extras), lr_mult=1, decay_mult=1, name="w"),
                dict(params=[m.bias for m in heads], lr_mult=2, decay_mult=0, name="b")]


def stub_batches(n, videos, device, seed=0):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        feat = torch.from_numpy(rs.standard_normal((videos, 8, FEAT)).astype(np.float32) * 2)
        target = torch.from_numpy(rs.randint(1, NUM_CLASS + 1, (videos, 8)).astype(np.int64))
        target[:, 7] = 0
        reg = torch.from_numpy(rs.standard_normal((videos, 8, 2)).astype(np.float32))
        ptype = torch.tensor([[0] + [1] * 6 + [2]] * videos)
        scaling = torch.ones((videos, 8, 2))
        out.append(tuple(t.to(device) for t in (feat, scaling, target, reg, ptype)))
    return out


class RefMeter(object):
    """AverageMeter of the reference, restated (ssn_train.py:373-388)."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def ref_accuracy(output, target):
    """accuracy() of the reference for topk = (1,), restated (ssn_train.py:401-414)."""
    _, pred = output.topk(1, 1, True, True)
    correct = pred.t().eq(target.view(1, -1))
    return correct[:1].reshape(-1).float().sum(0).mul_(100.0 / target.size(0))


def ref_meter_update(meters, act, tgt, losses4, weight):
    """ssn_train.py:216-233; losses4 = total, act, comp, reg"""
    for k in range(4):
        meters[k].update(losses4[k].item(), weight)
    c = act.size(1)
    meters[4].update(ref_accuracy(act, tgt).item(), act.size(0))
    meters[5].update(ref_accuracy(act.view(-1, 2, c)[:, 0, :].contiguous(), tgt.view(-1, 2)[:, 0].contiguous()).item(), act.size(0) // 2)
    meters[6].update(ref_accuracy(act.view(-1, 2, c)[:, 1, :].contiguous(), tgt.view(-1, 2)[:, 1].contiguous()).item(), act.size(0) // 2)


def reference_loop(model, opt, batches, iter_size, clip):
    """The reference's train() (ssn_train.py:191-253), literally, from pieces the library already had."""
    from action_detection_amd.ops.ssn_ops import SSNObjective
    from action_detection_amd.optim import clip_grad_norm
    objective = SSNObjective(0.1, 0.1)
    meters = [RefMeter() for _ in range(7)]
    gmax = 0.0
    model.train()
    opt.adjust_learning_rate(0, [])
    opt.zero_grad(set_to_none=True)
    for i, batch in enumerate(batches):
        out = model(*batch)
        loss = objective(*out, sample_split=1, sample_group_size=7)      # ssn_train.py:210-214 in the library's one launch
        act_loss, comp_loss, reg_loss = objective.parts.unbind(0)
        ref_meter_update(meters, out[0].detach(), out[1], [loss.detach(), act_loss, comp_loss, reg_loss], batch[0].size(0))
        loss.backward()
        if i % iter_size == 0:
            if iter_size != 1:
                for g in opt.param_groups:
                    for p in g["params"]:
                        p.grad /= iter_size
            if clip is not None:
                clip_grad_norm(model.parameters(), clip)
            gmax = max(gmax, max(float(p.grad.abs().max()) for p in model.parameters()))
            opt.step()
            opt.zero_grad(set_to_none=True)
    return meters, gmax


@pytest.mark.parametrize("iter_size,clip", [(1, None), (2, None), (1, 0.5), (2, 0.5)])
def test_trainer_matches_reference_loop(backend, iter_size, clip):
    """SSNTrainer.train_epoch over 5 batches against the reference's loop restated from pieces the library already had: SSNObjective
    (the fused total is not bit-equal to ``act + 0.1 * comp + 0.1 * reg`` in torch arithmetic, so both loops take the objective),
    clip_grad_norm, SSNSGD.step and torch accuracy.

    Meters: bit-equal to accuracy() / AverageMeter on the outputs the trainer's own forwards produced, in every configuration;
    without clipping the two loops apply the same bits (p.grad / 2 == p.grad * 0.5), so there the meters of the independent loop are
    bit-equal too and so are the weights.

    Weights with clipping, a priori: the two paths give the update a gradient that differs by the two norms (each within
    32 * 2^-24, the sumsq_multi bound; the per-tensor kernels of clip_grad_norm have chains no longer at these sizes), and by where
    the scale is applied: ``(g / iter) * coef`` rounds twice, ``g * (coef / iter)`` rounds the product of the scales once and the
    product once -- 4 * 2^-24 together.  So |d g_eff| <= 68 * 2^-24 * gmax per element, gmax = the largest clipped gradient element
    of the restated loop.  The update (same kernel body both ways, one rounding per operation) turns that into
    lr_max / (1 - momentum) * |d g_eff| per step at most (momentum sums a geometric series), plus 4 roundings of the result
    (4 * 2^-24 * |w|) where the inputs differed.  Later gradients are computed at weights that differ by that much; at lr 0.01 on
    this convex-ish stub the feedback is far below the first-order term, a factor 2 covers it.  Over 5 steps:
    tol = 5 * 2 * (lr_max / (1 - m) * 68 * 2^-24 * gmax + 4 * 2^-24 * max|w|)."""
    from action_detection_amd.ops.ssn_ops import SSNObjective
    from action_detection_amd.optim import SSNSGD
    from action_detection_amd.training import SSNTrainer
    dev = backend.device
    batches = stub_batches(5, 4, dev)
    model, ref_model = StubSSN().to(dev), StubSSN().to(dev)
    opt = SSNSGD(model.get_optim_policies(), lr=0.01)
    ref_opt = SSNSGD(ref_model.get_optim_policies(), lr=0.01)
    ref_meters, gmax = reference_loop(ref_model, ref_opt, batches, iter_size, clip)

    objective = SSNObjective(0.1, 0.1)
    parts_seen = []
    fwd = objective.forward

    def recording_forward(*a, **k):
        total = fwd(*a, **k)
        parts_seen.append(torch.cat([total.detach().reshape(1), objective.parts]).clone())
        return total
    objective.forward = recording_forward
    lib = _lib.get_lib()
    calls = []
    orig_call = lib.call

    def recording_call(name, *a):
        calls.append(name)
        return orig_call(name, *a)
    lines = []
    trainer = SSNTrainer(model, opt, objective, iter_size=iter_size, clip_gradient=clip, print_freq=2, log=lines.append)
    lib.call = recording_call
    K.train_step_launches(reset=True)
    try:
        trainer.train_epoch(batches, 0)
    finally:
        del lib.call
    launches = K.train_step_launches()
    got = trainer.meters.read()

    # meters against the reference's functions on the trainer's own outputs
    own = [RefMeter() for _ in range(7)]
    assert len(model.seen) == len(parts_seen) == 5
    for (act, tgt), losses4 in zip(model.seen, parts_seen):
        ref_meter_update(own, act, tgt, losses4, 4)
    for k, name in enumerate(ALL_NAMES):
        assert (got[name].val, got[name].sum, got[name].count, got[name].avg) == (own[k].val, own[k].sum, own[k].count, own[k].avg), name
    if clip is None:
        for k, name in enumerate(ALL_NAMES):
            assert (got[name].val, got[name].avg) == (ref_meters[k].val, ref_meters[k].avg), name

    # weights
    wmax = max(float(p.detach().abs().max()) for p in ref_model.parameters())
    tol = 5 * 2 * (0.02 / (1 - 0.9) * 68 * U * gmax + 4 * U * wmax)
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(model.parameters(), ref_model.parameters()))
    print("iter_size %d clip %r: worst weight difference %.3g (bound %.3g), gmax %.3g" % (iter_size, clip, worst, tol, gmax))
    assert worst <= (tol if clip is not None else 0.0)
    moved = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(model.parameters(), StubSSN().to(dev).parameters()))
    assert moved > 1e-3

    # launches: one ssn_step_meters per batch; per optimizer step one ssn_sumsq_multi call = ceil(T / 48) + 1 launches and
    # ceil(T / 48) update launches; never the per-parameter kernels
    t = sum(1 for _ in model.parameters())
    steps = sum(1 for i in range(5) if i % iter_size == 0)
    assert t == 56 and calls.count("ssn_step_meters") == 5
    assert "ssn_sumsq" not in calls and "ssn_scale" not in calls
    if clip is not None:
        assert calls.count("ssn_sumsq_multi") == steps and calls.count("ssn_sgd_step_multi_dev") == steps
        assert "ssn_sgd_step_multi" not in calls
        assert launches == 5 + steps * (math.ceil(t / 48) + 1 + math.ceil(t / 48))
    else:
        assert calls.count("ssn_sgd_step_multi") == steps and "ssn_sumsq_multi" not in calls
        assert launches == 5
    # a line for i = 0, 2, 4 with the reference's fields
    assert len(lines) == 3 and lines[0].startswith("Epoch: [0][0/5], lr: 0.01000\t") and "Act. FG " in lines[0]
    assert "Loss %.4f (%.4f)" % (got["loss"].val, got["loss"].avg) in lines[2]


def test_validate_and_checkpoint(backend, tmp_path):
    """validate() leaves parameters and .grad untouched and returns losses.avg; the checkpoint carries the reference's keys with the
    ``module.`` prefix, both key forms load, and a resumed run continues with the same epoch / best_loss."""
    from action_detection_amd.optim import SSNSGD
    from action_detection_amd.training import SSNTrainer, checkpoint_names, fit, load_checkpoint, save_checkpoint
    dev = backend.device
    model = StubSSN().to(dev)
    opt = SSNSGD(model.get_optim_policies(), lr=0.01)
    lines = []
    trainer = SSNTrainer(model, opt, print_freq=1, log=lines.append)
    batches = stub_batches(3, 2, dev, seed=3)
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
    before = [(p.detach().clone(), p.grad.clone()) for p in model.parameters()]
    loss = trainer.validate(batches)
    for p, (w, g) in zip(model.parameters(), before):
        assert torch.equal(p.detach(), w) and torch.equal(p.grad, g)
    m = trainer.val_meters.read()
    assert loss == m["loss"].avg and m["loss"].count == 6 and m["act_acc"].count == 12 and math.isfinite(loss)
    assert lines[0].startswith("Test: [0/3]\t") and lines[-1].startswith("Testing Results: Loss %.5f" % loss)
    assert not model.training

    names = checkpoint_names("ssn", str(tmp_path / "run"), "thumos14", "BNInception", "RGB")
    assert os.path.basename(names[0]) == "ssnrun_thumos14_BNInception_rgb_checkpoint.pth.tar"
    assert os.path.basename(names[1]) == "run_rgb_model_best.pth.tar"
    stats = np.array([[0.1, 0.2], [0.3, 0.4]])
    opt.zero_grad(set_to_none=True)
    best = fit(trainer, lambda e: batches, lambda e: batches, 2, "BNInception", names, eval_freq=1, reg_stats=stats)
    raw = torch.load(names[0], map_location="cpu", weights_only=False)
    assert sorted(raw) == ["arch", "best_loss", "epoch", "reg_stats", "state_dict"]
    assert raw["epoch"] == 2 and raw["arch"] == "BNInception" and raw["best_loss"] == best
    assert all(k.startswith("module.") for k in raw["state_dict"]) and len(raw["state_dict"]) == len(model.state_dict())
    assert os.path.exists(names[1])                                          # the loss fell: the best copy was written
    assert torch.equal(raw["reg_stats"], torch.from_numpy(stats))
    fresh = StubSSN().to(dev)
    with torch.no_grad():
        for p in fresh.parameters():
            p.zero_()
    ck = load_checkpoint(names[0], fresh)
    assert ck["epoch"] == 2 and ck["best_loss"] == best
    for p, q in zip(fresh.parameters(), model.parameters()):
        assert torch.equal(p.detach().cpu(), q.detach().cpu())
    # the other key form (no prefix), and is_best False writes no best copy
    plain = str(tmp_path / "plain.pth.tar")
    torch.save({"epoch": 7, "arch": "x", "best_loss": 1.5, "state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, plain)
    assert load_checkpoint(plain, StubSSN())["epoch"] == 7
    other = str(tmp_path / "other.pth.tar")
    save_checkpoint(model, 3, "x", 0.5, False, other, str(tmp_path / "other_best.pth.tar"))
    assert os.path.exists(other) and not os.path.exists(str(tmp_path / "other_best.pth.tar"))
    # resume: the schedule continues at the stored epoch with the stored best_loss (an unreachable one: no new best copy)
    os.remove(names[1])
    resumed = fit(trainer, lambda e: batches, lambda e: batches, 3, "BNInception", names, start_epoch=ck["epoch"], best_loss=-1.0,
                  eval_freq=1)
    assert resumed == -1.0 and not os.path.exists(names[1])
    assert torch.load(names[0], map_location="cpu", weights_only=False)["epoch"] == 3


def test_binary_trainer(backend):
    """BinaryTrainer on a stub returning (scores, target): loss meter = the cross entropy, FG / BG accuracies as torch computes them."""
    from action_detection_amd.optim import SSNSGD
    from action_detection_amd.training import BinaryTrainer

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.classifier_fc = torch.nn.Linear(FEAT, 2)
            self.seen = []

        def forward(self, x, target):
            s = self.classifier_fc(x.reshape(-1, FEAT))
            self.seen.append((s.detach().clone(), target.reshape(-1).clone()))
            return s, target.reshape(-1)
    dev = backend.device
    model = Stub().to(dev)
    opt = SSNSGD([dict(params=list(model.parameters()))], lr=0.05)
    rs = np.random.RandomState(0)
    batches = [(torch.from_numpy(rs.standard_normal((4, 8, FEAT)).astype(np.float32)).to(dev),
                torch.tensor([[1, 0] * 4] * 4).to(dev)) for _ in range(4)]
    lines = []
    trainer = BinaryTrainer(model, opt, clip_gradient=0.1, print_freq=1, log=lines.append)
    w0 = model.classifier_fc.weight.detach().clone()
    trainer.train_epoch(batches, 0)
    got = trainer.meters.read()
    fg, bg, ls = RefMeter(), RefMeter(), RefMeter()
    for s, t in model.seen:
        ls.update(torch.nn.functional.cross_entropy(s, t).item(), 4)
        fg.update(ref_accuracy(s.view(-1, 2, 2)[:, 0, :].contiguous(), t.view(-1, 2)[:, 0].contiguous()).item(), s.size(0) // 2)
        bg.update(ref_accuracy(s.view(-1, 2, 2)[:, 1, :].contiguous(), t.view(-1, 2)[:, 1].contiguous()).item(), s.size(0) // 2)
    assert (got["fg_acc"].val, got["fg_acc"].avg, got["bg_acc"].val, got["bg_acc"].avg) == (fg.val, fg.avg, bg.val, bg.avg)
    assert got["loss"].count == 16 and abs(got["loss"].avg - ls.avg) <= 8 * U * ls.avg     # (the CE kernel's own sum order)
    assert not torch.equal(w0, model.classifier_fc.weight.detach())
    assert lines[0].startswith("Epoch: [0][0/4], lr: 0.05000\t") and "\n FG" in lines[0]


# ----------------------------------------------------------------------------------------------------- StepMeters.reduce_
def _reduce_worker(rank, world, port, emu_path, ret):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from action_detection_amd import _lib as L
    from action_detection_amd.training import StepMeters
    L.use_library_for_testing(L.SsnLibrary(emu_path, is_emulator=True))
    g = golden()
    meters = StepMeters(LOSS_NAMES, "cpu")
    for s in range(2):       # rank r owns rows [65 r, 65 r + 64) of the (130, 101) case: 64 rows each (FG / BG pairs kept)
        lo = 65 * rank + (rank % 2)
        sl = slice(lo, lo + 64)
        meters.update(torch.from_numpy(g["r130_c101_logits"][s, sl]), torch.from_numpy(g["r130_c101_targets"][s, sl]),
                      torch.from_numpy(g["r130_c101_losses"][s] * (rank + 1)), 4 + rank)
    meters.reduce_()
    m = meters.read()
    ret[rank] = {k: tuple(v) for k, v in m.items() if k != "skipped"}
    dist.destroy_process_group()


def test_step_meters_reduce_two_processes(emu_library):
    """Two gloo processes: after reduce_ the global val / avg are those of the concatenated batch -- the n-weighted mean over the
    ranks.  Accuracies: each rank's fp32 percentage carries two roundings (100 / n, the product), so the weighted mean lies within
    4 * 2^-24 * 100 of the concatenated batch's own; losses: within double rounding of the weighted mean."""
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_reduce_worker, args=(world, port, emu_library.path, ret), nprocs=world, join=True)
    g = golden()
    assert ret[0] == ret[1]
    rows = [slice(0, 64), slice(66, 130)]
    hits_sum = np.zeros(3)
    for s in range(2):
        lg = np.concatenate([g["r130_c101_logits"][s, r] for r in rows])
        tg = np.concatenate([g["r130_c101_targets"][s, r] for r in rows])
        hit = lg.argmax(-1) == tg
        hits = np.array([hit.sum(), hit[0::2].sum(), hit[1::2].sum()])
        hits_sum += hits
        if s == 1:
            last = hits
    for k, name in enumerate(("act_acc", "fg_acc", "bg_acc")):
        n = 128 if k == 0 else 64
        val, avg, _, count = ret[0][name]
        assert count == 2 * n
        assert abs(val - 100.0 * last[k] / n) <= 4 * U * 100 and abs(avg - 100.0 * hits_sum[k] / (2 * n)) <= 4 * U * 100
    for k, name in enumerate(LOSS_NAMES):
        l = g["r130_c101_losses"][:2, k].astype(np.float64)
        val, avg, _, count = ret[0][name]
        assert count == 2 * (4 + 5)
        want_val = (l[1] * 4 + float(np.float32(l[1] * 2)) * 5) / 9
        want_avg = sum(l[s] * 4 + float(np.float32(l[s] * 2)) * 5 for s in range(2)) / 18
        assert abs(val - want_val) <= 1e-14 * want_val and abs(avg - want_avg) <= 1e-14 * want_avg


# ---------------------------------------------------------------------------------------------------------------- GPU only
def _gpu_step_pieces(dev, seed=0):
    from action_detection_amd.optim import SSNSGD
    from action_detection_amd.training import StepMeters
    g = golden()
    rs = np.random.RandomState(seed)
    sizes = [LENGTHS[i % 8] for i in range(50)]
    ps = [torch.nn.Parameter(torch.from_numpy(np.random.RandomState(i).standard_normal(n).astype(np.float32)).to(dev))
          for i, n in enumerate(sizes)]
    for p in ps:
        p.grad = torch.from_numpy(rs.standard_normal(p.numel()).astype(np.float32)).to(dev)
    opt = SSNSGD([dict(params=ps)], lr=0.01)
    opt.step(grad_scale=0.0)          # creates the momentum buffers (allocations are not part of the step)
    meters = StepMeters(LOSS_NAMES, dev)
    static = dict(logits=torch.from_numpy(g["r8_c21_logits"][0]).to(dev), target=torch.from_numpy(g["r8_c21_targets"][0]).to(dev),
                  losses=torch.from_numpy(g["r8_c21_losses"][0]).to(dev), flag=torch.zeros(1, dtype=torch.int32, device=dev))
    return ps, opt, meters, static


@pytest.mark.gpu
def test_step_is_sync_free(hip_library):
    """StepMeters.update, clip_grad_norm_device and opt.step(grad_scale_dev=) raise nothing under sync debug mode 'error'."""
    from action_detection_amd.optim import clip_grad_norm_device, clip_workspace_floats
    dev = torch.device("cuda:0")
    ps, opt, meters, st = _gpu_step_pieces(dev)
    out = torch.empty(2, device=dev)
    ws = torch.empty(clip_workspace_floats(ps), device=dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        meters.update(st["logits"], st["target"], st["losses"], 4, st["flag"])
        clip_grad_norm_device(ps, 0.5, 0.5, out, ws)
        opt.step(grad_scale_dev=out[1:], skip_flag=st["flag"])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert meters.read()["loss"].count == 4 and 0 < float(out[1]) < 0.5


@pytest.mark.gpu
def test_step_graph_capture_matches_eager(hip_library):
    """The three calls captured on one stream in a CUDAGraph and replayed three times over changed static inputs: meter state,
    norm / scale, weights and momentum bit-equal to the same three steps run eagerly."""
    from action_detection_amd.optim import clip_grad_norm_device, clip_workspace_floats
    dev = torch.device("cuda:0")
    g = golden()

    def step(ps, opt, meters, st, out, ws):
        meters.update(st["logits"], st["target"], st["losses"], 4, st["flag"])
        clip_grad_norm_device(ps, 2.0, 0.5, out, ws)
        opt.step(grad_scale_dev=out[1:], skip_flag=st["flag"])

    def inputs(k):
        rs = np.random.RandomState(100 + k)
        return (torch.from_numpy(g["r8_c21_logits"][k]).to(dev), torch.from_numpy(g["r8_c21_targets"][k]).to(dev),
                torch.from_numpy(g["r8_c21_losses"][k]).to(dev), rs)
    results = []
    for graphed in (False, True):
        ps, opt, meters, st = _gpu_step_pieces(dev)
        out = torch.zeros(2, device=dev)
        ws = torch.empty(clip_workspace_floats(ps), device=dev)
        graph = None
        if graphed:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            snap = [p.detach().clone() for p in ps], [opt.state[p]["momentum_buffer"].clone() for p in ps], meters.state.clone()
            with torch.cuda.graph(graph):
                step(ps, opt, meters, st, out, ws)
            torch.cuda.synchronize()
            with torch.no_grad():       # capture ran nothing, but restore anyway so that both runs start from the same state
                for p, w, b in zip(ps, snap[0], snap[1]):
                    p.copy_(w)
                    opt.state[p]["momentum_buffer"].copy_(b)
                meters.state.copy_(snap[2])
        for k in range(3):
            lg, tg, ls, rs = inputs(k)
            st["logits"].copy_(lg); st["target"].copy_(tg); st["losses"].copy_(ls)
            st["flag"].fill_(1 if k == 1 else 0)          # the middle step is flagged: skipped, counted
            for p in ps:
                p.grad.copy_(torch.from_numpy(rs.standard_normal(p.numel()).astype(np.float32)).to(dev))
            if graphed:
                graph.replay()
            else:
                step(ps, opt, meters, st, out, ws)
        torch.cuda.synchronize()
        results.append((bits(meters.state), out.cpu().view(torch.int32).tolist(),
                        [p.detach().cpu().view(torch.int32) for p in ps],
                        [opt.state[p]["momentum_buffer"].cpu().view(torch.int32) for p in ps], meters.read()))
    eager, replay = results
    assert eager[0] == replay[0] and eager[1] == replay[1]
    assert all(torch.equal(a, b) for a, b in zip(eager[2], replay[2])) and all(torch.equal(a, b) for a, b in zip(eager[3], replay[3]))
    assert eager[4]["skipped"] == 1 and eager[4]["loss"].count == 8


@pytest.mark.gpu
def test_ssn_trainer_real_model(hip_library):
    """One real SSN (BN-Inception, V = 2, 224^2, the setting of test_trainer_chain): two SSNTrainer steps with clipping and a
    validate.  Meters equal torch's accuracy / the objective's parts on the same outputs; losses are finite."""
    from action_detection_amd.ops.ssn_ops import SSNObjective
    from action_detection_amd.optim import SSNSGD
    from action_detection_amd.ssn_models import SSN
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic, make_batch
    from action_detection_amd.training import SSNTrainer
    dev = torch.device("cuda:0")
    num_class = 20
    torch.manual_seed(0)
    model = SSN(num_class, 2, 5, 2, "RGB", dropout=0.8, stpp_cfg=(1, 1, 1))
    init_backbone_synthetic(model.base_model)
    init_heads_synthetic(model, std=0.01)
    model.to(dev)
    opt = SSNSGD(model.get_optim_policies(), lr=0.001)
    batch = tuple(t.to(dev) for t in make_batch(2, "RGB", num_class, seed=0))
    seen = []
    hook = model.register_forward_hook(lambda m, i, o: seen.append((o[0].detach().clone(), o[1].clone())))
    objective = SSNObjective(0.1, 0.1)
    parts_seen = []
    fwd = objective.forward

    def recording_forward(*a, **k):
        total = fwd(*a, **k)
        parts_seen.append(torch.cat([total.detach().reshape(1), objective.parts]).clone())
        return total
    objective.forward = recording_forward
    lines = []
    trainer = SSNTrainer(model, opt, objective, clip_gradient=10.0, print_freq=1, log=lines.append)
    w0 = model.activity_fc.weight.detach().clone()
    trainer.train_epoch([batch, batch], 0)
    got = trainer.meters.read()
    hook_train = list(zip(seen, parts_seen))
    own = [RefMeter() for _ in range(7)]
    for (act, tgt), losses4 in hook_train:
        ref_meter_update(own, act, tgt, losses4, 2)
    assert got["skipped"] == 0 and len(hook_train) == 2
    for k, name in enumerate(ALL_NAMES):
        assert (got[name].val, got[name].sum, got[name].count, got[name].avg) == (own[k].val, own[k].sum, own[k].count, own[k].avg), name
        assert math.isfinite(got[name].avg)
    assert got["loss"].val > 0 and not torch.equal(w0, model.activity_fc.weight.detach())
    del seen[:], parts_seen[:]
    loss = trainer.validate([batch])
    hook.remove()
    act, tgt = seen[0]
    val = [RefMeter() for _ in range(7)]
    ref_meter_update(val, act, tgt, parts_seen[0], 2)
    assert loss == val[0].avg and math.isfinite(loss)
    assert trainer.val_meters.read()["act_acc"].val == val[4].val
    assert len(lines) == 4 and lines[-1].startswith("Testing Results: Loss")


# ------------------------------------------------------------------------------------------------------------ batch sources
def test_driver_batch_sources(tmp_path):
    """What the drivers feed the prefetcher: sampler + reader batches in the prefetcher's layout, the synthetic sources, the PIL
    reader on a frame directory."""
    from PIL import Image
    from action_detection_amd import train_data as D
    from action_detection_amd.actionness_sampling import ActionnessSampler
    from action_detection_amd.proposal_sampling import ProposalSampler
    plist = os.path.join(GOLD, "proposal_list_processed.txt")
    np.random.seed(0)
    sampler = ProposalSampler(plist)
    reader = D.SyntheticReader("RGB", hw=(6, 8))
    got = list(D.ssn_batches(sampler, reader, 2, order=[0, 1, 0]))
    assert len(got) == 1                                        # the incomplete last batch is dropped, as the reference's loader does not
    frames, scaling, target, reg, ptype = got[0]
    assert frames.shape == (2, 8 * 9, 6, 8, 3) and frames.dtype == np.uint8
    assert scaling.shape == (2, 8, 2) and target.shape == (2, 8) and target.dtype == np.int64 and reg.shape == (2, 8, 2)
    assert ptype.tolist() == [[0, 1, 1, 1, 1, 1, 1, 2]] * 2 and (target[:, 7] == 0).all() and (target[:, 0] > 0).all()
    assert len(list(D.ssn_batches(sampler, reader, 2, order=[0, 1, 0], drop_last=False))) == 2
    bsampler = ActionnessSampler(plist)
    frames, _, _, _, ptype = next(D.binary_batches(bsampler, reader, 2))
    assert frames.shape == (2, 12 * 5, 6, 8, 3) and ptype.tolist() == [[1] * 3 + [0] * 9] * 2
    a = list(D.synthetic_ssn_source(2, 2, 20, hw=(6, 8), seed=3))
    b = list(D.synthetic_ssn_source(2, 2, 20, hw=(6, 8), seed=3))
    assert len(a) == 2 and all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))
    assert a[0][0].shape == (2, 72, 6, 8, 3) and not np.array_equal(a[0][0], a[1][0])
    f = next(D.synthetic_binary_source(1, 2, "Flow", 5, hw=(6, 8)))
    assert f[0].shape == (2, 12 * 5 * 5 * 2, 6, 8, 1) and f[4].shape == (2, 12)
    assert list(D.binary_view([(1, 2, 3, 4, 5)])) == [(1, 5)]
    c = D.Counted(iter([1, 2]), 7)
    assert len(c) == 7 and list(c) == [1, 2]
    # frame directory
    vid = tmp_path / "v1"
    vid.mkdir()
    for i in (1, 2):
        Image.fromarray(np.full((6, 8, 3), 40 * i, np.uint8)).save(str(vid / "img_{:05d}.jpg".format(i)))
        Image.fromarray(np.full((6, 8), 50 * i, np.uint8)).save(str(vid / "flow_x_{:05d}.jpg".format(i)))
        Image.fromarray(np.full((6, 8), 60 * i, np.uint8)).save(str(vid / "flow_y_{:05d}.jpg".format(i)))
    rgb = D.FrameDirReader(str(tmp_path), "RGB")("v1", [1, 2, 2])
    assert rgb.shape == (3, 6, 8, 3) and rgb.dtype == np.uint8 and abs(int(rgb[1, 0, 0, 0]) - 80) <= 2
    flow = D.FrameDirReader(str(tmp_path), "Flow", "flow_")("v1", [2])
    assert flow.shape == (2, 6, 8, 1) and abs(int(flow[0, 0, 0, 0]) - 100) <= 2 and abs(int(flow[1, 0, 0, 0]) - 120) <= 2
