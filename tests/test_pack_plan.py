"""The coalesced bodies of the device-resident packing plan (csrc/conv_x6.hip: pack_entry_amax_wide, pack_entry_rows_staged).

Everything here is an EQUALITY check: the plan's bodies only move the data differently, so the referee is the per-table path (the same
``ssn_conv_x6_pack_*`` call outside a batch, which keeps the element-wise bodies) on the same weights, and the packed image INCLUDING
its tail (the amax the scale is derived from) is compared bit for bit.  Shapes are the smallest that reach a half slab, a full + a half
slab, row counts that are no multiple of a staging run, a split boundary off every multiple of 16, tap subsets, rectangular taps, the
zero-filled space-to-depth stem and more entries than three kernel-argument tables hold; both tiers run every case.
"""
import pytest
import torch

import action_detection_amd  # noqa: F401
from action_detection_amd import kernels as K

XP_MAX = 40      # entries per kernel-argument table (csrc/conv_x6.hip)


def _mk(backend, g, shape, kind="normal", off=0):
    """a weight of `shape`; off: its first element sits `off` floats behind a 16-byte boundary"""
    n = 1
    for d in shape:
        n *= d
    w = torch.randn(n, generator=g) * 0.1
    if kind == "zero":
        w.zero_()
    elif kind in ("first", "last", "middle"):
        w[{"first": 0, "last": n - 1, "middle": n // 2}[kind]] = -7.5       # the maximum magnitude, at a chosen element
    elif kind == "tiny":
        # exact +0 / -0 and values that underflow f16 after scaling (amax 4 -> scale 2^12: below 2^-37 nothing is left of them)
        w[0] = 4.0
        w[1::5] = 0.0
        w[2::5] = -0.0
        w[3::5] = 1e-13
        w[4::7] = -3e-30
    flat = torch.zeros(n + 4)
    flat[off:off + n] = w
    return backend.put(flat)[off:off + n].view(*shape)


CASES = {
    # 1: 1x1, mode 0 -- a half slab only; one full + one half slab with rows off every staging run
    "1x1-half": lambda b, g: [("sq", [([_mk(b, g, (8, 8, 1, 1), "first")], 0)])],
    "1x1-full+half": lambda b, g: [("sq", [([_mk(b, g, (40, 24, 1, 1), "last")], 0)])],
    # 2: 3x3, mode 0
    "3x3-fwd": lambda b, g: [("sq", [([_mk(b, g, (24, 40, 3, 3), "middle")], 0)])],
    # 3: 3x3, modes 1 and 2
    "3x3-dgrad": lambda b, g: [("sq", [([_mk(b, g, (40, 24, 3, 3))], 1)]), ("rect_dg", [_mk(b, g, (40, 24, 3, 3), "tiny")])],
    # 4: one fused 1x1 entry of four sources, no split boundary on a multiple of 16 (and its transposed form)
    "fused4": lambda b, g: [("sq", [([_mk(b, g, (8, 24, 1, 1)), _mk(b, g, (16, 24, 1, 1), "last"), _mk(b, g, (8, 24, 1, 1), "zero"),
                                      _mk(b, g, (24, 24, 1, 1))], 0)]),
                            ("sq", [([_mk(b, g, (8, 24, 1, 1)), _mk(b, g, (16, 24, 1, 1)), _mk(b, g, (8, 24, 1, 1)),
                                      _mk(b, g, (24, 24, 1, 1), "first")], 1)])],
    # 5: tap subsets -- the four parity sections of a stride-2 data gradient: 1, 2, 2 and 4 of the nine source taps
    "taps-s2": lambda b, g: [("s2", _mk(b, g, (16, 24, 3, 3), "middle"))],
    # 6: 1x7 and 7x1, forward and transposed + tap-reversed
    "rect": lambda b, g: [("rect", [_mk(b, g, (16, 16, 1, 7)), _mk(b, g, (16, 16, 7, 1), "last")]),
                          ("rect_dg", [_mk(b, g, (16, 16, 1, 7), "first"), _mk(b, g, (16, 16, 7, 1))])],
    # 7: the stem weight in its space-to-depth form (C = 12: four zero-filled rows per slab)
    "stem": lambda b, g: [("rect1", _mk(b, g, (64, 12, 4, 4)))],
    # 8: 3 * XP_MAX + 1 entries: table boundaries and the block -> entry search
    "many": lambda b, g: [("sq", [([_mk(b, g, (8, 8, 1, 1), ("normal", "zero", "last")[i % 3])], i % 2) for i in range(3 * XP_MAX + 1)])],
    # an all-zero tensor (scale 1, every byte zero) beside a normal one
    "zero": lambda b, g: [("sq", [([_mk(b, g, (24, 40, 3, 3), "zero")], 0), ([_mk(b, g, (8, 8, 1, 1))], 1)])],
    # sources that start 1, 2 and 3 floats behind a 16-byte boundary (slices of a flat parameter buffer): head / tail elements of the
    # 16-byte loads in both bodies
    "unaligned": lambda b, g: [("sq", [([_mk(b, g, (40, 24, 1, 1), "last", 1)], 0), ([_mk(b, g, (24, 40, 3, 3), "first", 2)], 0),
                                       ([_mk(b, g, (40, 24, 3, 3), "middle", 3)], 1),
                                       ([_mk(b, g, (8, 24, 1, 1), "normal", 1), _mk(b, g, (16, 24, 1, 1), "last", 3)], 0)]),
                               ("s2", _mk(b, g, (16, 24, 3, 3), "normal", 3)), ("rect_dg", [_mk(b, g, (16, 16, 7, 1), "last", 2)])],
}


def _run(calls):
    out = []
    for kind, arg in calls:
        if kind == "sq":
            out += list(K.pack_weights_multi(arg, x6=True))
        elif kind == "rect":
            out += list(K.pack_rect_multi(arg))
        elif kind == "rect_dg":
            out += list(K.pack_rect_multi(arg, dgrad=True))
        elif kind == "s2":
            out.append(K.pack_dgrad_s2(arg))
        else:
            out.append(K.pack_weights_rect(arg))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_plan_bodies_equal_table_bodies(backend, case):
    """a plan launch == the per-table path on the same weights, packed rows and tail, byte for byte; a second plan launch on buffers
    filled with other bytes rewrites all of them"""
    g = torch.Generator().manual_seed(1000 + list(CASES).index(case))
    calls = CASES[case](backend, g)
    ref = [t.clone() for t in _run(calls)]
    state = {}
    for rep in range(2):
        with K.PackBatch(state, backend.device):
            got = _run(calls)
        assert len(got) == len(ref)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert a.numel() == b.numel(), (case, i)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (case, "entry", i, "repeat", rep)
        for t in got:
            t.fill_(7.0)
    if case == "zero":
        assert int(ref[0].view(torch.int32).abs().max()) == 0
