"""The grouped weight gradients with per-family reductions and a fan-out over side streams (ssn_conv_wgrad_pl_group_lanes,
csrc/wgrad_pl.hip) and the executor's switch for it (planes_exec.run_backward, net.wgrad_lanes).

Everything here is an EQUALITY check: where a family runs, when its slabs are summed and whether a pass's problems travel in one call or
two must not change one bit of any gradient, so the referee is the existing entry point (ssn_conv_wgrad_pl_group, pinned against float64
autograd by tests/test_wgrad_pl_edges.py) on the same operands, compared with torch.equal.

The problem set (N = 2 images) holds one problem per kernel family of the planner, at the smallest shapes that still reach every body and
a ragged edge; test_set_reaches_every_family asserts that from the planner's own answer.  The host-emulator tier runs the same cases with
no streams (the per-family reduction, the two-call order, the pinned shares); the GPU tier adds 1, 2 and 3 streams, a first part left
unjoined, and the capture of a three-stream call into a graph (a test of its own).
"""
import pytest
import torch

import action_detection_amd  # noqa: F401
from action_detection_amd import planes as P

from test_conv_pl_edges import tiers
from test_wgrad_pl_edges import Problem, _guarded, _intact
from tiny_backbone import TinyBackbone, init_tiny

GPU = pytest.mark.gpu

# (case = (N, Cin, H, W, Cout, kh, kw, stride, ph, pw), row split, row gap, cropped, family, variants it may take or None)
SET = [
    ((2, 24, 7, 7, 40, 3, 3, 1, 1, 1), 0, 0, False, 0, None),       # nine taps, rows <= 14: channel counts off every tile, a last group of 8
    ((2, 16, 14, 14, 16, 3, 3, 1, 1, 1), 0, 0, False, 0, None),     # nine taps at the family's widest row
    ((2, 8, 30, 30, 16, 3, 3, 1, 1, 1), 0, 0, False, 1, None),      # nine taps, rows <= 30
    ((2, 8, 3, 56, 16, 3, 3, 1, 1, 1), 0, 0, False, 2, None),       # nine taps, rows <= 56
    ((2, 72, 7, 7, 136, 1, 1, 1, 0, 0), 64, 8, False, 3, (0, 1, 2)),  # one tap, rows behind 64 sit 8 channels up (fused block-input launch)
    ((2, 8, 56, 56, 8, 1, 1, 1, 0, 0), 0, 0, False, 3, (3,)),          # chunked 1x1
    ((2, 16, 28, 28, 24, 3, 3, 2, 1, 1), 0, 0, False, 3, None),     # stride 2: one tap
    ((2, 12, 8, 8, 16, 4, 4, 1, 2, 2), 0, 0, True, 4, None),        # the space-to-depth stem of 16 x 16 frames
    ((2, 8, 3, 10, 16, 1, 7, 1, 0, 3), 0, 0, False, 5, None),       # 1 x 7
    ((2, 8, 10, 5, 16, 7, 1, 1, 3, 0), 0, 0, False, 6, None),       # 7 x 1
]
CHUNKED = 5
ALL = list(range(len(SET)))

_cache = {}


def _problems(backend, key="a"):
    """the set's problems on this tier + the existing entry point's gradients for them, built once and left unchanged"""
    k = (backend.name, key)
    if k not in _cache:
        probs = [Problem(backend, case, ("lanes", key, i), split=split, gap=gap, crop=crop)
                 for i, (case, split, gap, crop, _, _) in enumerate(SET)]
        ref, plan = _call(backend, probs, ALL, None)
        for p, (dw, db) in zip(probs, ref):
            p.check(dw, db, "lanes", "reference call")           # (the referee itself against float64 autograd)
        _cache[k] = (probs, ref, plan)
    return _cache[k]


def _call(backend, probs, idx, streams, units=None, join=True):
    """one grouped call on probs[idx] -> ([(dw, db)] on the host -- or the jobs, when the streams are left unjoined --, plan)"""
    jobs = [probs[i].job(backend) for i in idx]
    for j, u in zip(jobs, units or []):
        j.units = u
    ws_bytes, tb_bytes, plan = P.wgrad_group_plan(jobs)
    ws, guard = _guarded(backend, ws_bytes)
    tb = backend.put(torch.zeros(tb_bytes, dtype=torch.uint8))
    P.conv_wgrad_group(jobs, ws, tb, streams=streams, join=join)
    if not join:
        return (jobs, ws, tb, guard), plan
    assert _intact(guard), ("wrote behind its workspace", plan)
    return [(j.dw.cpu(), j.db.cpu()) for j in jobs], plan


def _streams(backend, n):
    return [torch.cuda.Stream(device=backend.device) for _ in range(n)] if backend.is_gpu else []


def _same(got, ref, idx, what):
    for (dw, db), i in zip(got, idx):
        assert torch.equal(dw, ref[i][0]), ("dW differs", what, i, SET[i][0])
        assert torch.equal(db, ref[i][1]), ("db differs", what, i, SET[i][0])


@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_set_reaches_every_family(backend):
    """the planner's answer for the set: all seven families, the one-tap family with a one-tap, a chunked and a stride-2 problem, the
    gap problem and a problem in more than one share"""
    _, _, plan = _problems(backend)
    for (case, _, _, _, family, variant), p in zip(SET, plan):
        assert p[0] == family and (variant is None or p[1] in variant), (case, p)
    assert {p[0] for p in plan} == set(range(7)), plan
    assert {min(p[1], 3) == 3 for p in plan if p[0] == 3} == {False, True}, plan
    assert any(p[2] > 1 for p in plan), plan


@pytest.mark.parametrize("backend,n", tiers([(0,), (1,), (2,), (3,)], [(0,)]), indirect=["backend"])
def test_lanes_equal_group(backend, n):
    """the new entry point on 0, 1, 2 and 3 streams == the existing one, weight and bias gradients, bit for bit; on the GPU twice (the
    second call reuses the cached events)"""
    probs, ref, _ = _problems(backend)
    streams = _streams(backend, n)
    for rep in range(2 if backend.is_gpu else 1):
        got, _ = _call(backend, probs, ALL, streams)
        _same(got, ref, ALL, (n, "streams", rep))


PARTS = [([i for i in ALL if i != CHUNKED], [CHUNKED]),      # a part that is the chunked 56 x 56 problem alone
         (ALL[:4], ALL[4:]),
         (ALL[1::2], ALL[0::2])]


@pytest.mark.parametrize("backend,split,order,n", tiers([(s, o, n) for s in range(3) for o in (0, 1) for n in (0, 2)],
                                                        [(s, o, 0) for s in range(3) for o in (0, 1)]), indirect=["backend"])
def test_two_calls_equal_one(backend, split, order, n):
    """the set as two calls, in both orders, every problem with the share the plan of the whole set gave it (WgradJob.units): the same
    splits as in one call, so the same bits.  With streams the first call is left unjoined and the second joins both."""
    probs, ref, plan = _problems(backend)
    parts = PARTS[split][::-1] if order else PARTS[split]
    streams = _streams(backend, n)
    first = None
    for k, idx in enumerate(parts):
        units = [plan[i][3] for i in idx]
        out, part_plan = _call(backend, probs, idx, streams, units, join=not (streams and k == 0))
        assert [p[2:] for p in part_plan] == [plan[i][2:] for i in idx], ("the part is split differently", idx, part_plan)
        if streams and k == 0:
            first = out
        else:
            _same(out, ref, idx, ("part", k, parts))
    if first is not None:       # (joined by the second call: its streams are the same)
        jobs, _, _, guard = first
        assert _intact(guard)
        _same([(j.dw.cpu(), j.db.cpu()) for j in jobs], ref, parts[0], ("unjoined part", parts))


@GPU
def test_three_streams_captured(hip_library):
    """a three-stream call captured into a graph after one eager call (which creates the events: never inside a capture), replayed
    twice with the operands refilled in between: each replay == the existing entry point on those operands"""
    from test_conv_pl_edges import _Gpu
    probs, ref_a, _ = _problems(_Gpu, "a")
    other, ref_b, _ = _problems(_Gpu, "b")
    tensors = [t for p in probs for t in (p.gt, p.xt)]
    keep = [(t.data.clone(), t.scale.clone()) for t in tensors]
    fill_b = [(t.data, t.scale) for p in other for t in (p.gt, p.xt)]
    lanes = _streams(_Gpu, 3)
    jobs = [p.job(_Gpu) for p in probs]
    ws_bytes, tb_bytes, _ = P.wgrad_group_plan(jobs)
    ws, guard = _guarded(_Gpu, ws_bytes)
    tb = torch.zeros(tb_bytes, dtype=torch.uint8, device=_Gpu.device)
    s = torch.cuda.Stream(device=_Gpu.device)
    try:
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            P.conv_wgrad_group(jobs, ws, tb, streams=lanes)
        torch.cuda.current_stream().wait_stream(s)
        _same([(j.dw.cpu(), j.db.cpu()) for j in jobs], ref_a, ALL, "eager")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            P.conv_wgrad_group(jobs, ws, tb, streams=lanes)
        for name, fill, ref in (("replay b", fill_b, ref_b), ("replay a", keep, ref_a)):
            for t, (data, scale) in zip(tensors, fill):
                t.data.copy_(data)
                t.scale.copy_(scale)
            for j in jobs:
                j.dw.fill_(9.0)
                j.db.fill_(9.0)
            graph.replay()
            torch.cuda.synchronize()
            _same([(j.dw.cpu(), j.db.cpu()) for j in jobs], ref, ALL, name)
        assert _intact(guard)
    finally:
        for t, (data, scale) in zip(tensors, keep):      # (the cached problems stay what they were)
            t.data.copy_(data)
            t.scale.copy_(scale)


def _tiny_grads(dev, mode, monkeypatch):
    monkeypatch.setenv("SSN_WGRAD_LANES", mode)
    net = init_tiny(TinyBackbone()).to(dev).train()
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(3, 3, 16, 16, generator=g) * 40.0).to(dev)
    w = torch.randn(3, 32, generator=g).to(dev)
    out = []
    for _ in range(2):          # (the first backward of a state calibrates; the second runs the steady schedule)
        net.zero_grad(set_to_none=True)
        (net.features(x) * w).sum().backward()
        out.append({k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None})
    assert net.wgrad_lanes == (mode != "0")
    return out


@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_executor_lanes_equal_one_flush(backend, monkeypatch):
    """the five-layer backbone of the executor tests, forward + backward twice: SSN_WGRAD_LANES=1 (on the GPU: the families of the grouped
    call on three side streams, each with its own slab sum; the emulator has no streams: the per-family sums on one) ==
    SSN_WGRAD_LANES=0 (one stream, one reduction at the end) in every parameter gradient of both passes."""
    off = _tiny_grads(backend.device, "0", monkeypatch)
    on = _tiny_grads(backend.device, "1", monkeypatch)
    for a, b in zip(off, on):
        assert a.keys() == b.keys() and len(a) >= 6, a.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k
