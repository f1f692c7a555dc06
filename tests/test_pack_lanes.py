"""A packing pass in two parts (ssn_conv_x6_pack_batch_end_lanes / _join, csrc/conv_x6.hip) and the executor's switch for it
(planes_exec.run_forward, net.pack_lanes).

Everything here is an EQUALITY check: which stream an entry is packed on must not change one byte of its image, so the referee is the
per-table path (the same calls outside a batch) and, for the executor, the one-stream run.  The host-emulator tier has no streams: it
runs the two parts one after the other (the sub-ranges of the plan, their block bases); the GPU tier adds the side stream, the join and
the capture of the whole sequence into a graph.
"""
import pytest
import torch

import action_detection_amd  # noqa: F401
from action_detection_amd import kernels as K
from action_detection_amd import planes as P

from test_conv_pl_edges import tiers
from tiny_backbone import TinyBackbone, init_tiny

GPU = pytest.mark.gpu


def _weights(backend, seed):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return backend.put(torch.randn(*shape, generator=g) * 0.1)
    return {"sq": [([rnd(24, 40, 3, 3)], 0), ([rnd(8, 24, 1, 1), rnd(16, 24, 1, 1)], 0), ([rnd(40, 24, 3, 3)], 1)],
            "s2": rnd(16, 24, 3, 3), "rect": [rnd(16, 16, 1, 7), rnd(16, 16, 7, 1)]}


COUNT = 3 + 4 + 2      # entries _run_all records (a stride-2 data gradient is four)


def _run_all(w):
    return list(K.pack_weights_multi(w["sq"], x6=True)) + [K.pack_dgrad_s2(w["s2"])] + list(K.pack_rect_multi(w["rect"], dgrad=True))


def _side(backend):
    return torch.cuda.Stream(device=backend.device) if backend.is_gpu else object()


@pytest.mark.parametrize("backend,n_first", tiers([(0,), (1,), (COUNT - 1,), (COUNT,)], [(0,), (1,), (COUNT - 1,), (COUNT,)]),
                         indirect=["backend"])
def test_split_equals_unsplit(backend, n_first):
    """n_first leading entries on the calling stream, the others on the side stream == the per-table images, tails included; twice
    (the second pass reuses the plan and the events) with the buffers overwritten in between"""
    w = _weights(backend, 5)
    ref = [t.clone() for t in _run_all(w)]
    state, side = {}, _side(backend)
    for rep in range(2):
        with K.PackBatch(state, backend.device, n_first=n_first, side=side) as batch:
            got = _run_all(w)
            assert int(batch.lib.cdll.ssn_conv_x6_pack_batch_entries()) == COUNT
        K.pack_batch_join(backend.device)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ("entry", i, "n_first", n_first, "repeat", rep)
        for t in got:
            t.fill_(7.0)      # (on the calling stream: the next pass's side part starts behind its fork event, so behind this)


@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_join_without_pending_and_bad_split(backend):
    """a join with nothing pending returns at once, also right after another join; more leading entries than recorded is an argument
    error that closes the batch"""
    if backend.is_gpu:
        torch.cuda.synchronize()
    for _ in range(2):
        K.pack_batch_join(backend.device)
    if backend.is_gpu:
        assert torch.cuda.current_stream().query(), "the join left work on the stream"
    w = _weights(backend, 6)
    with pytest.raises(RuntimeError, match="leading entries"):
        with K.PackBatch({}, backend.device, n_first=COUNT + 1, side=_side(backend)):
            _run_all(w)
    with K.PackBatch({}, backend.device):
        one = K.pack_dgrad_s2(w["s2"])
    assert torch.equal(one.view(torch.int32), K.pack_dgrad_s2(w["s2"]).view(torch.int32))


@GPU
def test_split_packing_captured(hip_library):
    """split packing, the join and a 1x1 convolution whose weights are packed on the side stream, captured into a graph after one
    eager run (which creates the events: never inside a capture) and replayed twice with the weights changed in between: every
    replay == the uncaptured one-stream run on those weights"""
    dev = "cuda:0"
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(2, 16, 8, 8, generator=g) * 2.0).to(dev)
    wa = (torch.randn(32, 16, 1, 1, generator=g) * 0.3).to(dev)
    wb = (torch.randn(32, 16, 1, 1, generator=g) * 0.2 + 0.05).to(dev)
    stem = (torch.randn(8, 8, 1, 1, generator=g) * 0.1).to(dev)
    scale = (torch.rand(32, generator=g) + 0.5).to(dev)
    shift = (torch.randn(32, generator=g) * 0.1).to(dev)
    w = wa.clone()
    xp = P.from_f32(x)
    y = P.PlaneTensor(2, 32, 8, 8, dev)

    def conv(wp):
        P.conv_fwd(P.pfull(xp), wp, scale, shift, P.pfull(y), 1, 1, 1, 0, 0, True)

    def one_stream():
        y.data.fill_(9.0)
        conv(K.pack_weights_multi([([w], 0)], x6=True)[0])
        return y.data.clone()

    for src in (wb, wa):                # the delayed scale of y: settled once over both weights, then left alone
        w.copy_(src)
        one_stream()
    y.pool.update()
    ref = {}
    for name, src in (("a", wa), ("b", wb)):
        w.copy_(src)
        ref[name] = one_stream()
    assert not torch.equal(ref["a"], ref["b"])

    state, side = {}, torch.cuda.Stream(device=dev)

    def step():
        with K.PackBatch(state, dev, side=side) as batch:
            K.pack_weights_multi([([stem], 0)], x6=True)
            batch.stem_done()
            wp = K.pack_weights_multi([([w], 0)], x6=True)[0]
        K.pack_batch_join(dev)
        conv(wp)

    s = torch.cuda.Stream(device=dev)
    w.copy_(wa)
    y.data.fill_(9.0)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(y.data, ref["a"]), "eager split run"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        step()
    for name, src in (("b", wb), ("a", wa)):
        w.copy_(src)
        y.data.fill_(9.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.data, ref[name]), ("replay", name)


def _tiny_run(dev, mode, monkeypatch):
    monkeypatch.setenv("SSN_PACK_LANES", mode)
    net = init_tiny(TinyBackbone()).to(dev).train()
    assert net.pack_lanes == (mode != "0")
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(3, 3, 16, 16, generator=g) * 40.0).to(dev)
    w = torch.randn(3, 32, generator=g).to(dev)
    out = []
    for _ in range(2):          # (the first pass of a state calibrates; the second runs the steady schedule)
        net.zero_grad(set_to_none=True)
        feat = net.features(x)
        (feat * w).sum().backward()
        flat = torch.cat([p.grad.detach().reshape(-1) for _, p in sorted(net.named_parameters()) if p.grad is not None])
        out.append((feat.detach().cpu().clone(), flat.cpu().clone()))
    return out


@pytest.mark.parametrize("backend", tiers([()], []), indirect=["backend"])      # (the emulator has no streams: both runs would be one)
def test_executor_pack_lanes_equal_one_stream(backend, monkeypatch):
    """the five-layer backbone of the executor tests, forward + backward twice: SSN_PACK_LANES=1 (on the GPU: the first convolution's
    operand on the pass's stream, all others on the side stream, joined behind the pool) == SSN_PACK_LANES=0 in the features and in
    the flat gradient of both passes"""
    off = _tiny_run(backend.device, "0", monkeypatch)
    on = _tiny_run(backend.device, "1", monkeypatch)
    for (fa, ga), (fb, gb) in zip(off, on):
        assert ga.numel() > 1000
        assert torch.equal(fa, fb), "features differ"
        assert torch.equal(ga, gb), "flat gradient differs"
