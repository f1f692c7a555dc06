#!/usr/bin/env python
"""The per-step bookkeeping of the training loop on one MI355X: one JSON line, and with --out the text of
profiles/train_loop_measured.txt.

    timeout -k 10 540 python tools/bench_train_loop.py [--iters 20] [--out profiles/train_loop_measured.txt]

Parameter set: the RGB BN-Inception SSN with 20 classes, gradients resident on the device (seeded noise).  Two versions of the
bookkeeping of one step -- meters, clipping, optimizer -- alternate inside one process:

  (A) what the library had: three torch ``accuracy`` calls + seven ``.item()`` (ssn_train.py:216-233), ``optim.clip_grad_norm``
      (per-tensor ssn_sumsq, a host read of the norm, per-tensor ssn_scale), ``SSNSGD.step``;
  (B) ``StepMeters.update`` + ``clip_grad_norm_device`` + ``SSNSGD.step(grad_scale_dev=)``: no host read.

Host clock around a window that ends in a device synchronise; the gradients are restored before every window (A scales them in
place).  Then the whole eager step (4 videos: forward, objective, backward, bookkeeping) both ways.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def accuracy(output, target):
    """accuracy() of ssn_train.py:401-414 for topk = (1,)"""
    _, pred = output.topk(1, 1, True, True)
    correct = pred.t().eq(target.view(1, -1))
    return correct[:1].reshape(-1).float().sum(0).mul_(100.0 / target.size(0))


class HostMeter(object):
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def spread(samples):
    a = np.asarray(samples)
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
            "p25_ms": round(float(np.percentile(a, 25)), 4), "p75_ms": round(float(np.percentile(a, 75)), 4)}


def commit_name():
    if os.environ.get("BENCH_COMMIT"):
        return os.environ["BENCH_COMMIT"]
    try:
        head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain"], stderr=subprocess.DEVNULL).decode().strip()
        return head + (" + the working tree of this change" if dirty else "")
    except Exception:
        return "unknown (no git metadata where this ran; set BENCH_COMMIT)"


def device_kernels(torch, fn):
    """Number of device kernels one call of fn launches (torch profiler, outside every timed window); None when unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "emcpy" not in e.name
                   and "emset" not in e.name)
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=8)
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    import action_detection_amd as pkg
    from action_detection_amd import _lib
    from action_detection_amd import kernels as K
    from action_detection_amd.ops.ssn_ops import SSNObjective
    from action_detection_amd.optim import SSNSGD, clip_grad_norm, clip_grad_norm_device, clip_workspace_floats
    from action_detection_amd.ssn_models import SSN
    from action_detection_amd.synthetic import init_backbone_synthetic, init_heads_synthetic, make_batch
    from action_detection_amd.training import StepMeters
    pkg.build()
    assert torch.cuda.is_available(), "bench_train_loop.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda:0")
    num_class, v = 20, a.videos
    torch.manual_seed(0)
    model = SSN(num_class, 2, 5, 2, "RGB", dropout=0.8, stpp_cfg=(1, 1, 1))
    init_backbone_synthetic(model.base_model)
    init_heads_synthetic(model, std=0.01)
    model.to(dev).train()
    opt = SSNSGD(model.get_optim_policies(), lr=1e-6)
    params = [p for g in opt.param_groups for p in g["params"]]
    n_values = sum(p.numel() for p in params)
    gen = torch.Generator(device="cpu").manual_seed(1)
    master = [(torch.randn(p.shape, generator=gen) * 0.01).to(dev) for p in params]
    for p, m in zip(params, master):
        p.grad = m.clone()

    def restore():
        torch._foreach_copy_([p.grad for p in params], master)
        torch.cuda.synchronize()
    ref_norm = float(np.sqrt(sum(float((m.double() ** 2).sum()) for m in master)))
    max_norm = ref_norm / 2          # clipping is active: (A) runs its scale pass, as a clipped step does
    rows, cols = 2 * v, num_class + 1
    logits = torch.randn((rows, cols), generator=gen).to(dev)
    target = torch.randint(0, cols, (rows,), generator=gen).to(dev)
    losses4 = torch.rand(4, generator=gen).to(dev)      # total, act, comp, reg
    flag = model.scale_fault_flag()

    host = [HostMeter() for _ in range(7)]
    norms = {}

    def path_a():
        for k in range(4):
            host[k].update(losses4[k].item(), v)
        host[4].update(accuracy(logits, target).item(), rows)
        host[5].update(accuracy(logits.view(-1, 2, cols)[:, 0, :].contiguous(), target.view(-1, 2)[:, 0].contiguous()).item(), rows // 2)
        host[6].update(accuracy(logits.view(-1, 2, cols)[:, 1, :].contiguous(), target.view(-1, 2)[:, 1].contiguous()).item(), rows // 2)
        norms["a"] = clip_grad_norm(params, max_norm)
        opt.step(skip_flag=flag)

    meters = StepMeters(("loss", "act_loss", "comp_loss", "reg_loss"), dev)
    clip_out = torch.empty(2, device=dev)
    clip_ws = torch.empty(clip_workspace_floats(params), device=dev)

    def path_b():
        meters.update(logits, target, losses4, v, flag)
        clip_grad_norm_device(params, max_norm, 1.0, clip_out, clip_ws)
        opt.step(grad_scale_dev=clip_out[1:], skip_flag=flag)

    lib = _lib.get_lib()

    def library_calls(fn):
        calls = []
        orig = lib.call
        lib.call = lambda name, *args: (calls.append(name), orig(name, *args))[1]
        try:
            fn()
        finally:
            del lib.call
        return calls
    restore(); path_a(); restore(); path_b(); torch.cuda.synchronize()       # warm-up of both
    restore(); calls_a = library_calls(path_a)
    restore(); calls_b = library_calls(path_b)
    restore(); K.train_step_launches(reset=True); path_b(); launches_b = K.train_step_launches()
    restore(); kern_a = device_kernels(torch, path_a)
    restore(); kern_b = device_kernels(torch, path_b)
    norm_b = float(clip_out[0])
    t_a, t_b = [], []
    for _ in range(a.iters):
        for fn, acc in ((path_a, t_a), (path_b, t_b)):
            restore()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)

    # the whole eager step both ways
    batch = tuple(t.to(dev) for t in make_batch(v, "RGB", num_class, seed=0))
    objective = SSNObjective(0.1, 0.1)
    loss_buf = torch.empty(4, device=dev)

    def step(bookkeeping):
        out = model(*batch)
        loss = objective(*out)
        if bookkeeping == "a":
            parts = objective.parts
            host[0].update(loss.item(), v)
            for k in range(3):
                host[1 + k].update(parts[k].item(), v)
            act, tgt = out[0].detach(), out[1]
            c = act.size(1)
            host[4].update(accuracy(act, tgt).item(), act.size(0))
            host[5].update(accuracy(act.view(-1, 2, c)[:, 0, :].contiguous(), tgt.view(-1, 2)[:, 0].contiguous()).item(), act.size(0) // 2)
            host[6].update(accuracy(act.view(-1, 2, c)[:, 1, :].contiguous(), tgt.view(-1, 2)[:, 1].contiguous()).item(), act.size(0) // 2)
            loss.backward()
            clip_grad_norm(params, 1e9)
            opt.step(skip_flag=flag)
        else:
            torch.cat([loss.detach().reshape(1), objective.parts], out=loss_buf)
            meters.update(out[0], out[1], loss_buf, v, flag)
            loss.backward()
            clip_grad_norm_device(params, 1e9, 1.0, clip_out, clip_ws)
            opt.step(grad_scale_dev=clip_out[1:], skip_flag=flag)
        opt.zero_grad(set_to_none=True)
    s_a, s_b = [], []
    for i in range(a.step_iters + 2):
        for kind, acc in (("a", s_a), ("b", s_b)):
            t0 = time.perf_counter()
            step(kind)
            torch.cuda.synchronize()
            if i >= 2:                                   # two warm-up rounds
                acc.append((time.perf_counter() - t0) * 1e3)

    t = len(params)
    res = {"what": "training-step bookkeeping on one MI355X", "commit": commit_name(), "iters": a.iters, "tensors": t,
           "values": n_values, "videos": v, "bookkeeping_a": spread(t_a), "bookkeeping_b": spread(t_b),
           "library_calls_a": len(calls_a), "library_calls_b": len(calls_b),
           "library_launches_a": 2 * calls_a.count("ssn_sumsq") + calls_a.count("ssn_scale") + -(-t // 48),
           "library_launches_b": launches_b, "device_kernels_a": kern_a, "device_kernels_b": kern_b,
           "norm_float64": ref_norm, "norm_a": norms["a"], "norm_b": norm_b,
           "norm_rel_err_a": abs(norms["a"] - ref_norm) / ref_norm, "norm_rel_err_b": abs(norm_b - ref_norm) / ref_norm,
           "step_a": spread(s_a), "step_b": spread(s_b), "step_iters": a.step_iters}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(report(res))
    print(json.dumps(res))


def report(r):
    def line(s):
        return "median {median_ms} ms   (min {min_ms}, quartiles {p25_ms} .. {p75_ms}, max {max_ms})".format(**s)
    verdict = "B is not slower than A" if r["bookkeeping_b"]["median_ms"] <= r["bookkeeping_a"]["median_ms"] else "B IS SLOWER THAN A"
    return """Training-step bookkeeping: tools/bench_train_loop.py on one MI355X, commit measured: {commit}.
Method: both versions warmed up, then {iters} timed repetitions each, alternating inside one process; host clock around a window
that ends in a device synchronise; gradients restored (and the device idle) before every window; medians and spread.  Seeded
synthetic gradients on the parameter set of the RGB BN-Inception SSN, 20 classes: {tensors} tensors, {values} values.  Clipping
active (max_norm = half the norm).  No profiler attached to the timed windows.

1. Bookkeeping of one step (meters for {videos} videos, clipping, optimizer), gradients resident:
     (A) 3 torch accuracy + 7 .item() + optim.clip_grad_norm + SSNSGD.step        {a}
     (B) StepMeters.update + clip_grad_norm_device + step(grad_scale_dev=)        {b}
   {verdict}.
   library calls per step: A {ca}, B {cb}; kernel launches issued by the library: A {la} (2 per ssn_sumsq, 1 per ssn_scale,
   {sgd} optimizer launches), B {lb} (1 meters, {sq} norm, {sgd} optimizer); device kernels per step counted by the torch
   profiler, torch's own included: A {ka}, B {kb}.  A reads the host 8 times per step (7 meters, the norm), B never.

2. The norm of the same gradients: float64 {n64:.9g}; A {na:.9g} (relative error {ea:.3g}); B {nb:.9g} (relative error {eb:.3g};
   a-priori bound 32 * 2^-24 = 1.9e-06).

3. The whole eager step, {videos} videos (forward, objective, backward, bookkeeping, max_norm 1e9), {si} repetitions each after two
   warm-up rounds, alternating:
     with (A)   {sa}
     with (B)   {sb}

To repeat: timeout -k 10 540 python tools/bench_train_loop.py --out profiles/train_loop_measured.txt
""".format(commit=r["commit"], iters=r["iters"], tensors=r["tensors"], values=r["values"], videos=r["videos"],
           a=line(r["bookkeeping_a"]), b=line(r["bookkeeping_b"]), verdict=verdict, ca=r["library_calls_a"], cb=r["library_calls_b"],
           la=r["library_launches_a"], lb=r["library_launches_b"], sgd=-(-r["tensors"] // 48), sq=-(-r["tensors"] // 48) + 1,
           ka=r["device_kernels_a"], kb=r["device_kernels_b"], n64=r["norm_float64"], na=r["norm_a"], ea=r["norm_rel_err_a"],
           nb=r["norm_b"], eb=r["norm_rel_err_b"], si=r["step_iters"], sa=line(r["step_a"]), sb=line(r["step_b"]))


if __name__ == "__main__":
    main()
