"""Everything that reads or writes the planes layout outside the convolutions (csrc/planes_ops.hip: from_f32 / to_f32 / im2col, the max and
average pools, relu_bn_bwd, the global pool, the channel sums; csrc/planes_bn.hip: training-mode BatchNorm) at every kernel variant and
edge, against plain float64 torch on the CPU (F.max_pool2d(ceil_mode=True, return_indices=True) + autograd, F.avg_pool2d(
count_include_pad=True), F.batch_norm(training=True) + autograd -- the formula written out where torch refuses one value per channel --,
plain sums and means).  The reference is computed from the values STORED in the planes (P.to_f32 of the source).

  A  max pool: 8 image shapes (1 x 1 ... 15 x 16, H != W, last 2 x 2 block row / column half outside) x 7 (k, s, pad); signed and post-ReLU
     inputs; the argmax against torch's indices; backward as planes (fast kernel where eligible), accumulating onto a base under a mask
     with NaN channels, as fp32 NCHW, with the pooled mask (planes, fp32, and a mask scale one float into its buffer: the general kernel,
     bit-identical to the fast one);
  B  average pool: k = 3 (fast) / 5 / 7, five shapes, with / without affine and ReLU, source and destination at different group offsets;
  C  relu_bn_bwd, gap_bwd, gap_fwd at HW = 1 ... 289 (64 | 65: the LDS limit of the global pool) x 1 / 17 / 21 groups; gap_fwd gives the
     bits of the host's pixel-order fp32 sum on both kernels;
  D  channel_sum, channel_sum_multi (27 entries: a second table; the empty list), BatchNorm statistics / apply / backward at N HW = 1, 31,
     33, 32, 245, 700, 900; a constant channel, |mean| / sigma = 50, negative gamma, no bias, no running statistics, no ReLU with y never
     written, 264 channels, dz as planes and as fp32;
  E  from_f32 / to_f32 at channel tails 1 ... 7, space-to-depth at W / 2 != H / 2, im2col at kh != kw and pad_h != pad_w from a slice at
     group 1; one producer per family driven into the clamp;
  F  one launch of more than 2048 x 256 work items (not a multiple of it; N = 2, two groups, H != W) for every grid-stride kernel of both
     files (GPU tier), and a child interpreter that repeats the CPU-tier cases of A - C with SSN_PL_GRID_CAP=1 (CPU tier);
  G  the 2 GiB fall-backs: the same slice at the end of a tensor just above and just below the limit of the 32-bit kernels, bit-identical
     to the call on compact tensors (GPU tier only; skipped only with less than 24 GB free: an MI355X with 288 GB never skips);
  H  the argument errors of these entry points: RuntimeError, the destination untouched.

Conventions of every launch (the run_* helpers): planes operands are slices at channel 8 (16 where source and destination must differ) of
tensors that are wider in front and behind and hold NaN wherever the slice does not; every byte outside a destination slice must come
back bit-identical (int16 views); flat buffers (argmax, fp32 outputs, reduction outputs, workspaces of exactly *_workspace_bytes) carry a
guard of 256 elements that must come back untouched; after every planes producer the amax slot (zeroed) equals max |ref| within 1e-4,
a slot preset to twice that is not lowered, and the repeated launch reproduces the first bit for bit.  Tolerances are those of
tests/test_planes.py, relative to the largest magnitude of the reference: maxpool fwd 2^-21, bwd 2^-20, accumulating 2^-19; avgpool / gap /
relu_bn_bwd / gap_bwd 1e-6; channel_sum 2e-6; BN mean max|z| 2^-21, invstd 5e-6, running 1e-6 / 2e-6, y 1e-5, dgamma / dbeta 1e-5, dz 2e-5.

The GPU tier runs everything.  The CPU tier (host emulator) runs: A (7,10) 3/2/0, (10,7) 3/2/1, (15,16) 3/2/1, (2,3) 3/1/1, (9,12) 3/1/0,
(1,1) 3/2/1, (3,1) 2/2/0, (12,9) 5/2/2; B k = 3 / 5 / 7 at (5,9) with affine + ReLU, k = 3 at (1,1) and (2,1) plain, k = 5 at (9,5) affine
only; C HW = 1 / 64 / 65 / 71 at 136 channels, HW = 49 at 168, HW = 81 at 8; D, E and H entirely; of F the child run only; nothing of G.
bnp_grid of planes_bn.hip has no switch like SSN_PL_GRID_CAP: the second trip of pl_bn_apply_kernel / pl_bn_bwd_apply_kernel is covered by
the GPU tier only (test_large_bn takes 57 s on the emulator, the other large cases 25 - 100 s each).

Wall time of this file as measured: GPU tier, one MI355X, 212 tests in 8.1 s (the slowest 1.2 s; the ten cases of part G 0.1 s each: the wide
tensors are allocated, never filled); CPU tier, host emulator, 79 tests in 87 s (the two 264-channel BatchNorm cases 20 s each, the child
run 11 s).
Worst error observed on the MI355X per part, against its bound:
  A  maxpool fwd 0 (2^-21: a copy), bwd 2.1e-7 (9.5e-7), accumulating 2.2e-7 (1.9e-6), fp32 2.2e-7, pooled mask 1.3e-7 / fp32 6.7e-8 (9.5e-7)
  B  avgpool 2.8e-7 (1e-6)
  C  relu_bn_bwd 1.3e-7, gap_bwd 1.8e-7, gap_fwd 8.3e-7 at HW = 289 (1e-6)
  D  channel_sum 2.3e-7, multi 2.2e-7 (2e-6); BN mean 0.055 of its bound, invstd 6.0e-8 (5e-6), running mean / var 5.0e-8 / 8.2e-8 (1e-6 /
     2e-6), y 1.9e-7 (1e-5), dgamma / dbeta 6.0e-7 / 7.8e-8 (1e-5), dz 2.2e-7 planes and fp32 (2e-5)
  E  from_f32 9.5e-8 (2^-21); under the clamp at most 2.2e-7 (avgpool; 1e-6); to_f32 and im2col bit-exact
  F  maxpool bwd 1.7e-7, pooled 1.4e-7, accumulating 1.3e-7, fp32 1.0e-7; avgpool 2.4e-7; relu_bn_bwd 1.0e-7; gap_bwd 1.1e-7; BN y 1.8e-7,
     dz 1.7e-7, dgamma 1.7e-7; from_f32 8.5e-8
  G  bit-identical to the compact calls on both sides of the limit; maxpool fwd 0, bwd 1.2e-7, avgpool 1.8e-7
"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import action_detection_amd
from action_detection_amd import kernels as K
from action_detection_amd import planes as P

from test_planes import _two_pass, rel_err
from test_conv_pl_edges import amax_close, gen, mask_inputs, tiers

NAN = float("nan")
GUARD = 256
GUARD_FILL = {torch.float32: -7777.25, torch.uint8: 0xA5}
F16_MAX = 65504.0
T_FWD, T_BWD, T_ACC, T_AVG, T_SUM = 2.0 ** -21, 2.0 ** -20, 2.0 ** -19, 1e-6, 2e-6


def _lib():
    return action_detection_amd._lib.get_lib()


def _r8(c):
    return (c + 7) // 8 * 8


def note(part, what, err, bound):
    print("  [%s] %s err %.3g (bound %.3g)" % (part, what, err, bound), flush=True)


# ------------------------------------------------------------------------------------------------------------ operands
def wide(backend, n, c, h, w, front=8, back=8):
    """channels [front, front + c) of a NaN-filled planes tensor that is `front` channels wider in front and `back` behind"""
    t = P.PlaneTensor(n, front + _r8(c) + back, h, w, backend.device)
    t.data.fill_(NAN)
    return P.PSlice(t, front, c)


def store(backend, x, sl, headroom=0):
    """x into the slice with the exact scale of its maximum, lowered by `headroom` bits (room for what a kernel adds or multiplies)"""
    xd = backend.put(x.float().contiguous())
    P.from_f32(xd, sl)
    if headroom:
        sl.t.pool.scale.mul_(2.0 ** -headroom)
        P.from_f32(xd, sl, exact=False)
        sl.t.amax.zero_()


def put_wide(backend, x, front=8, back=8, headroom=0):
    sl = wide(backend, x.shape[0], x.shape[1], x.shape[2], x.shape[3], front, back)
    store(backend, x, sl, headroom)
    return sl


def stored(sl):
    return P.to_f32(sl).cpu().double()


def _groups(sl):
    g0 = sl.c0 // 8
    return g0, g0 + _r8(sl.c) // 8


def outside(sl):
    d = sl.t.data.view(torch.int16)
    g0, g1 = _groups(sl)
    return torch.cat([d[:, :, :g0].reshape(-1), d[:, :, g1:].reshape(-1)]).cpu()


def inside(sl):
    g0, g1 = _groups(sl)
    return sl.t.data.view(torch.int16)[:, :, g0:g1].clone().cpu()


def guarded(backend, shape, dtype=torch.float32, fill=NAN):
    """a flat buffer of exactly this shape with GUARD elements of a distinctive value behind it -> (the view to pass, the guard)"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), GUARD_FILL[dtype], dtype=dtype)
    buf[:numel] = fill
    buf = backend.put(buf)
    return buf[:numel].view(*shape), buf[numel:]


def intact(guard):
    return bool((guard == GUARD_FILL[guard.dtype]).all())


def check_producer(launch, dst, ref, tol, part, what, prep=None):
    """One planes producer under the conventions of this file.  launch(): one launch into the slice dst.  Without prep the delayed-scale
    protocol runs (a pass that only records the maximum, the update, the pass that is checked); with prep() -- which rewrites what the
    launch reads from dst and fixes its scale -- every launch follows a prep.  -> the stored result"""
    t = dst.t
    ref = ref.detach()
    rmax = ref.abs().max().item()
    if prep is not None:
        prep()
    before = outside(dst)
    t.amax.zero_()
    launch()
    if prep is None:
        ok, figs = amax_close(t, rmax)
        assert ok, ("amax of the first pass", part, what, figs)
        t.pool.update()
        assert t.amax.cpu().item() == 0.0
        launch()
    ok, figs = amax_close(t, rmax)
    print("  [%s] %s amax %s" % (part, what, figs), flush=True)
    assert ok, ("amax", part, what, figs)
    first = inside(dst)
    got = stored(dst)
    if prep is not None:
        prep()
    preset = torch.tensor(2.0 * rmax if rmax > 0 else 1.0, dtype=torch.float32)
    t.amax.fill_(preset.item())
    launch()
    assert t.amax.cpu().item() == preset.item(), ("a recorded maximum was lowered or raised", part, what, t.amax.cpu().item(), preset.item())
    assert torch.equal(inside(dst), first), ("not reproducible", part, what)
    assert torch.equal(outside(dst), before), ("wrote outside its slice", part, what)
    assert bool(torch.isfinite(got).all()), ("non-finite values stored", part, what)
    err = rel_err(got, ref)
    note(part, what, err, tol)
    assert err < tol, (part, what, err)
    return got


def mask_factor(actv, msc):
    """the float64 factor a mask stands for, from the STORED activation: 1 on NaN (pass-through) channels, (act > 0) * scale elsewhere"""
    return torch.where(torch.isnan(msc).view(1, -1, 1, 1), torch.ones_like(actv),
                       (actv > 0).double() * torch.nan_to_num(msc).double().view(1, -1, 1, 1))


# ------------------------------------------------------------------------------------------------------------ A: max pool
SHAPES_A = [(1, 1), (2, 3), (3, 1), (7, 10), (10, 7), (9, 12), (12, 9), (15, 16)]
CFG_A = [(3, 2, 0), (3, 2, 1), (3, 1, 1), (3, 1, 0), (2, 2, 0), (5, 2, 2), (5, 1, 2)]
ALL_BWD = ("plain", "acc", "f32", "pooled", "pooled_f32", "misaligned")


def _torch_takes(h, w, k, s, pad):
    try:
        F.max_pool2d(torch.zeros(1, 1, h, w), k, s, pad, ceil_mode=True)
        return True
    except RuntimeError:
        return False


CASES_A = [(h, w, k, s, pad) for (h, w) in SHAPES_A for (k, s, pad) in CFG_A if _torch_takes(h, w, k, s, pad)]
EMU_A = [(7, 10, 3, 2, 0), (10, 7, 3, 2, 1), (15, 16, 3, 2, 1), (2, 3, 3, 1, 1), (9, 12, 3, 1, 0), (1, 1, 3, 2, 1), (3, 1, 2, 2, 0),
         (12, 9, 5, 2, 2)]
_POOL_REF = {}


def pool_reference(backend, n, c, h, w, k, s, pad, signed):
    """inputs of a max pool case, the slices that hold them and the float64 reference of forward, argmax and backward (computed once
    per case, from the stored values)"""
    key = (backend.name, n, c, h, w, k, s, pad, signed)
    g = gen("pool", *key[1:])
    x = torch.randn(n, c, h, w, generator=g) - 1.0 if signed else torch.randn(n, c, h, w, generator=g).clamp(min=0)
    xs = put_wide(backend, x, back=8)
    if key not in _POOL_REF:
        xv = stored(xs).requires_grad_()
        ref, idx = F.max_pool2d(xv, k, s, pad, ceil_mode=True, return_indices=True)
        ho, wo = ref.shape[2], ref.shape[3]
        h0 = torch.arange(ho).view(1, 1, -1, 1) * s - pad
        w0 = torch.arange(wo).view(1, 1, 1, -1) * s - pad
        local = (torch.div(idx, w, rounding_mode="floor") - h0) * k + (idx % w - w0)
        assert int(local.min()) >= 0 and int(local.max()) < k * k
        local = local.view(n, c // 8, 8, ho * wo).permute(0, 1, 3, 2).contiguous().to(torch.uint8)
        gy = torch.randn(ref.shape, generator=g)
        if xv.numel() > (1 << 20):      # (the large cases of part F: one of them at a time)
            for other in [o for o, v in _POOL_REF.items() if v[0].numel() > (1 << 20)]:
                del _POOL_REF[other]
        _POOL_REF[key] = [xv, ref, local, gy, None, None]
    r = _POOL_REF[key]
    gs = put_wide(backend, r[3], back=24)
    if r[4] is None:
        r[4] = stored(gs)
        r[1].backward(r[4])
        r[5] = r[0].grad
        r[1] = r[1].detach()
        r[0] = r[0].detach()
    return x, xs, r[0], r[1], r[2], gs, r[5]


def run_maxpool(backend, n, c, h, w, k, s, pad, signed, part, variants=ALL_BWD):
    what = (h, w, k, s, pad, "signed" if signed else "relu")
    x, xs, xv, ref, local, gs, dref = pool_reference(backend, n, c, h, w, k, s, pad, signed)
    ho, wo = ref.shape[2], ref.shape[3]
    ys = wide(backend, n, c, ho, wo, front=16, back=16)
    am, am_guard = guarded(backend, (n, c // 8, ho * wo, 8), torch.uint8, 0xEE)
    check_producer(lambda: P.maxpool_fwd(xs, ys, am, k, s, pad), ys, ref, T_FWD, part, ("maxpool fwd",) + what)
    assert intact(am_guard), ("wrote behind the argmax", what)
    assert torch.equal(am.cpu(), local), ("argmax", what)
    g = gen("pool bwd", *what)
    msc = torch.randn(c, generator=g)
    msc[::5] = NAN
    mscd = backend.put(msc)
    m = mask_factor(xv, msc)
    if "plain" in variants:
        ds = wide(backend, n, c, h, w, back=16)
        check_producer(lambda: P.maxpool_bwd(gs, am, ds, k, s, pad), ds, dref, T_BWD, part, ("maxpool bwd",) + what)
    if "acc" in variants:
        ds = wide(backend, n, c, h, w, back=16)
        base = torch.randn(n, c, h, w, generator=g)

        def prep():
            store(backend, base, ds, headroom=4)
        prep()
        want = (stored(ds) + dref) * m
        check_producer(lambda: P.maxpool_bwd(gs, am, ds, k, s, pad, accumulate=True, mask=xs, mask_scale=mscd), ds, want, T_ACC, part,
                       ("maxpool bwd acc",) + what, prep=prep)
    masks = [("f32", xs, False)] if "f32" in variants else []
    if (k, s) == (3, 2) and "pooled_f32" in variants:
        masks.append(("pooled_f32", ys, True))
    for name, mk, pooled in masks:
        out = []
        for _ in range(2):
            buf, guard = guarded(backend, (n, c, h, w), fill=7.0)
            dx32 = K.attach_amax(buf)
            P.maxpool_bwd(gs, am, dx32, k, s, pad, mask=mk, mask_scale=mscd, mask_pooled=pooled)
            assert intact(guard), ("wrote behind the fp32 gradient", name, what)
            out.append(dx32.cpu())
        err = rel_err(out[0], dref * m)
        note(part, ("maxpool bwd " + name,) + what, err, T_BWD)
        assert err < T_BWD, (name, what, err)
        assert torch.equal(out[0], out[1]), ("not reproducible", name, what)
        rmax = float((dref * m).abs().max())
        assert abs(float(dx32._ssn_amax) - rmax) <= 1e-4 * rmax, ("fp32 amax", name, what, float(dx32._ssn_amax), rmax)
    if (k, s) == (3, 2) and "pooled" in variants:
        dp = wide(backend, n, c, h, w, back=16)
        check_producer(lambda: P.maxpool_bwd(gs, am, dp, k, s, pad, mask=ys, mask_scale=mscd, mask_pooled=True), dp, dref * m, T_BWD, part,
                       ("maxpool bwd pooled",) + what)
        if "misaligned" in variants:
            # the same call with the scale vector one float into its buffer: the general 2 x 2 block kernel, the same bits
            aligned = inside(dp)
            holder = backend.put(torch.full((c + 8,), NAN))
            holder[1:1 + c].copy_(mscd)
            mis = holder[1:1 + c]
            assert mscd.data_ptr() % 16 == 0 and mis.data_ptr() % 16 == 4
            before = outside(dp)
            dp.t.data.view(torch.int16)[:, :, 1:1 + c // 8].fill_(0x7E00)
            P.maxpool_bwd(gs, am, dp, k, s, pad, mask=ys, mask_scale=mis, mask_pooled=True)
            assert torch.equal(inside(dp), aligned), ("general k3s2 kernel differs from the fast one", what)
            assert torch.equal(outside(dp), before), ("wrote outside its slice", "misaligned", what)
    return ys, am


@pytest.mark.parametrize("backend,h,w,k,s,pad", tiers(CASES_A, EMU_A), indirect=["backend"])
def test_maxpool_every_variant(backend, h, w, k, s, pad):
    """N = 3 images x 24 channels (three groups: dv_g no power of two), signed (randn - 1: a tap that wrongly read 0 would win) and
    post-ReLU inputs (exact-zero ties: the first maximum in scan order routes the gradient)"""
    for signed in (True, False):
        run_maxpool(backend, 3, 24, h, w, k, s, pad, signed, "A")


def test_case_lists():
    assert set(EMU_A) <= set(CASES_A) and len(CASES_A) >= 48, len(CASES_A)
    for (h, w) in SHAPES_A[3:]:      # (every configuration on every shape of more than a window)
        assert all((h, w) + cfg in CASES_A for cfg in CFG_A), (h, w)


# ------------------------------------------------------------------------------------------------------------ B: average pool
SHAPES_B = [(1, 1), (2, 1), (5, 9), (9, 5), (17, 17)]
CASES_B = [(k, h, w, aff, relu) for k in (3, 5, 7) for (h, w) in SHAPES_B for (aff, relu) in ((0, 0), (1, 0), (1, 1), (0, 1))]
EMU_B = [(3, 5, 9, 1, 1), (5, 5, 9, 1, 1), (7, 5, 9, 1, 1), (3, 1, 1, 0, 0), (3, 2, 1, 0, 0), (5, 9, 5, 1, 0)]


def run_avgpool(backend, n, c, h, w, k, aff, relu, part):
    """forward behind a projection (affine, ReLU; negative shifts and a negative scale so the ReLU bites) and, without either, the pool's
    own backward stencil; source at group 1 of a tensor 16 channels wider, destination at group 2 of one 40 wider"""
    g = gen("avg", n, c, h, w, k, aff, relu)
    xs = put_wide(backend, torch.randn(n, c, h, w, generator=g) * 2.0, front=8, back=8)
    sc, sh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3 - 0.3
    sc[1] = -sc[1]
    ref = F.avg_pool2d(stored(xs), k, 1, k // 2, count_include_pad=True)
    if aff:
        ref = ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    if relu:
        assert bool((ref < 0).any())
        ref = F.relu(ref)
    ys = wide(backend, n, c, h, w, front=16, back=24)
    scd, shd = (backend.put(sc), backend.put(sh)) if aff else (None, None)
    check_producer(lambda: P.avgpool_affine(xs, ys, scd, shd, bool(relu), k, k // 2), ys, ref, T_AVG, part, ("avgpool", k, h, w, aff, relu))


@pytest.mark.parametrize("backend,k,h,w,aff,relu", tiers(CASES_B, EMU_B), indirect=["backend"])
def test_avgpool_every_variant(backend, k, h, w, aff, relu):
    run_avgpool(backend, 2, 16, h, w, k, aff, relu, "B")


# ------------------------------------------------------------------------------------------------------------ C: relu_bn_bwd, gap
HW_C = {1: (1, 1), 5: (1, 5), 49: (7, 7), 64: (8, 8), 65: (5, 13), 71: (1, 71), 81: (9, 9), 289: (17, 17)}
CASES_C = [(hw, c) for hw in HW_C for c in (8, 136, 168)]
EMU_C = [(1, 136), (64, 136), (65, 136), (71, 136), (49, 168), (81, 8)]


def run_relu_gap(backend, n, c, h, w, part, gap_fwd=True):
    hw = h * w
    g = gen("C", n, c, h, w)
    act, msc, _ = mask_inputs(n, c, h, w, g)
    acts = put_wide(backend, act, back=16)
    m = mask_factor(stored(acts), msc)
    mscd = backend.put(msc)
    z = torch.randn(n, c, h, w, generator=g)
    gs = wide(backend, n, c, h, w, back=8)

    def prep():
        store(backend, z, gs, headroom=3)
    prep()
    check_producer(lambda: P.relu_bn_bwd(gs, acts, mscd), gs, stored(gs) * m, T_AVG, part, ("relu_bn_bwd", hw, c), prep=prep)
    dfeat = torch.randn(n, c, generator=g)
    dfd = backend.put(dfeat)
    dxs = wide(backend, n, c, h, w, back=24)
    refg = (dfeat.double() / hw).view(n, c, 1, 1) * m
    check_producer(lambda: P.gap_bwd(dfd, dxs, mask=acts, mask_scale=mscd), dxs, refg, T_AVG, part, ("gap_bwd", hw, c))
    if not gap_fwd:
        return
    zs = put_wide(backend, z, back=16)
    out = []
    for _ in range(2):
        feat, guard = guarded(backend, (n, c))
        P.gap_fwd(zs, feat)
        assert intact(guard), ("gap_fwd wrote behind its output", hw, c)
        out.append(feat.cpu())
    err = rel_err(out[0], stored(zs).mean(dim=(2, 3)))
    note(part, ("gap_fwd", hw, c), err, T_AVG)
    assert err < T_AVG, ("gap_fwd", hw, c, err)
    assert torch.equal(out[0], out[1])
    # the sums run in pixel order in fp32 on both kernels: the host repeats them on the stored values and must get the same bits
    sc = np.float32(zs.t.scale.cpu().item())
    st = (P.to_f32(zs).cpu().numpy() * sc).reshape(n, c, hw)      # (power-of-two scale: exact)
    acc = np.zeros((n, c), dtype=np.float32)
    for q in range(hw):
        acc = (acc + st[:, :, q]).astype(np.float32)
    want = acc * (np.float32(1.0) / (np.float32(hw) * sc))
    assert np.array_equal(out[0].numpy(), want), ("global average pool: sums in pixel order", hw, c)


@pytest.mark.parametrize("backend,hw,c", tiers(CASES_C, EMU_C), indirect=["backend"])
def test_relu_bn_gap_every_size(backend, hw, c):
    """HW 64 | 65: the last size the LDS kernel of the global pool takes and the first of the other; 65, 71, 81: its 8-pixel batches end
    inside one; C = 136 / 168: a full 16-group workgroup + one of 1 / of 5"""
    run_relu_gap(backend, 2, c, HW_C[hw][0], HW_C[hw][1], "C")


# ------------------------------------------------------------------------------------------------------------ D: reductions
NHW_D = [(1, 1, 1), (1, 1, 31), (3, 1, 11), (2, 4, 4), (5, 7, 7), (7, 10, 10), (3, 15, 20)]      # 1, 31, 33, 32, 245, 700, 900 positions


@pytest.mark.parametrize("backend,n,h,w", tiers(NHW_D, NHW_D), indirect=["backend"])
def test_channel_sum_ranges(backend, n, h, w):
    """32 shares of N HW positions: empty shares, shares of one or two, a 256-stride that crosses three images at once (HW = 100)"""
    c = 24
    xs = put_wide(backend, torch.randn(n, c, h, w, generator=gen("D sum", n, h, w)) + 0.5, back=16)
    nbytes = P.channel_sum_workspace_bytes(c)
    got = []
    for _ in range(2):
        out, og = guarded(backend, (c,))
        ws, wg = guarded(backend, (nbytes // 4,))
        P.channel_sum(xs, out, ws)
        assert intact(og) and intact(wg), ("channel_sum wrote behind a buffer", n, h, w)
        got.append(out.cpu())
    err = rel_err(got[0], stored(xs).sum(dim=(0, 2, 3)))
    note("D", ("channel_sum", n, h, w), err, T_SUM)
    assert err < T_SUM and torch.equal(got[0], got[1]), (n, h, w, err)


@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_channel_sum_multi_second_table(backend):
    """27 entries (a table takes 24: the second one reuses the workspace and restarts its group prefix) of 8 / 16 / 24 channels and
    differing image sizes, N HW < 32 among them: every entry bit-identical to its single call; the empty list is no error"""
    n = 2
    sizes = [(1, 1), (1, 3), (2, 5), (3, 5), (4, 4), (1, 15), (7, 7), (9, 13), (2, 9)]
    ent, guards = [], []
    for i in range(27):
        c, (h, w) = 8 * (1 + i % 3), sizes[i // 3]
        xs = put_wide(backend, torch.randn(n, c, h, w, generator=gen("D multi", i)) + 0.25, back=8 * (1 + i % 2))
        out, og = guarded(backend, (c,))
        ent.append((xs, out))
        guards.append(og)
    assert len({(sl.c, sl.hw) for sl, _ in ent}) == 27
    wsm, wg = guarded(backend, (P.channel_sum_workspace_bytes(sum(sl.c for sl, _ in ent)) // 4,))
    P.channel_sum_multi(ent, wsm)
    assert intact(wg) and all(intact(og) for og in guards)
    for i, (sl, got) in enumerate(ent):
        one, og = guarded(backend, (sl.c,))
        ws, wg1 = guarded(backend, (P.channel_sum_workspace_bytes(sl.c) // 4,))
        P.channel_sum(sl, one, ws)
        assert intact(og) and intact(wg1)
        assert torch.equal(got.cpu(), one.cpu()), ("entry differs from its single call", i, sl.c, sl.hw)
        err = rel_err(got, stored(sl).sum(dim=(0, 2, 3)))
        note("D", ("channel_sum_multi", i), err, T_SUM)
        assert err < T_SUM, (i, err)
    lib = _lib()
    lib.call("ssn_pl_channel_sum_multi", 0, None, None, None, None, n, None, None, None, None, 0, K._stream(lib, wsm))
    assert intact(wg)


def bn_reference(zv, bias, gamma, beta, rm, rv, relu, eps, mom):
    """float64: F.batch_norm(training=True) (+ ReLU) on z + bias; with one value per channel, where torch refuses, the formula: the
    variance is 0, xhat is 0, and the running variance takes the biased value (the kernel's documented guard)"""
    zd = zv.clone().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    rm_ref, rv_ref = (None, None) if rm is None else (rm.double().clone(), rv.double().clone())
    zb = zd if bias is None else zd + bias.double().view(1, -1, 1, 1)
    if zv.shape[0] * zv.shape[2] * zv.shape[3] > 1:
        pre = F.batch_norm(zb, rm_ref, rv_ref, gd, bd, True, mom, eps)
    else:
        mean = zb.mean(dim=(0, 2, 3), keepdim=True)
        var = ((zb - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        pre = (zb - mean) / (var + eps).sqrt() * gd.view(1, -1, 1, 1) + bd.view(1, -1, 1, 1)
        if rm is not None:
            rm_ref = (1 - mom) * rm_ref + mom * mean.detach().flatten()
            rv_ref = (1 - mom) * rv_ref + mom * var.detach().flatten()
    return zd, gd, bd, (F.relu(pre) if relu else pre), rm_ref, rv_ref


def run_bn(backend, n, c, h, w, part, relu=True, bias=True, running=True, special=False, out32=True):
    what = (n, c, h, w, relu, bias, running, special)
    g = gen("D bn", *what)
    eps, mom = 1e-5, 0.1
    z = torch.randn(n, c, h, w, generator=g) * (torch.rand(c, generator=g) * 3 + 0.5).view(1, -1, 1, 1) \
        + (torch.randn(c, generator=g) * 4).view(1, -1, 1, 1)
    if special:
        z[:, 2] = 3.0                                                   # a constant channel: variance 0
        z[:, 5] = torch.randn(n, h, w, generator=g) * 0.1 + 5.0         # |mean| / sigma = 50
    bias_t = torch.randn(c, generator=g) if bias else None
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    gamma[1] = -gamma[1]
    rm, rv = (torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5) if running else (None, None)
    zs = put_wide(backend, z, back=8)
    zv = stored(zs)
    zd, gd, bd, ref, rm_ref, rv_ref = bn_reference(zv, bias_t, gamma, beta, rm, rv, relu, eps, mom)
    nbytes = P.bn_train_workspace_bytes(c)
    got = []
    for _ in range(2):
        mean, g1 = guarded(backend, (c,))
        invstd, g2 = guarded(backend, (c,))
        rmd, g3 = guarded(backend, (c,), fill=0.0)
        rvd, g4 = guarded(backend, (c,), fill=0.0)
        if running:
            rmd.copy_(rm)
            rvd.copy_(rv)
        ws, g5 = guarded(backend, (nbytes // 4,))
        P.bn_train_stats(zs, backend.put(bias_t), mean, invstd, rmd if running else None, rvd if running else None, eps, mom, ws)
        assert all(intact(x) for x in (g1, g2, g3, g4, g5)), ("bn stats wrote behind a buffer", what)
        got.append((mean.cpu(), invstd.cpu(), rmd.cpu(), rvd.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*got)), ("bn stats not reproducible", what)
    bm, bv = zv.mean(dim=(0, 2, 3)), zv.var(dim=(0, 2, 3), unbiased=False)
    e_mean = (got[0][0].double() - bm).abs().max().item()
    note(part, ("bn mean",) + what, e_mean, zv.abs().max().item() * 2.0 ** -21)
    assert e_mean < zv.abs().max().item() * 2.0 ** -21, ("bn mean", what, e_mean)
    e_inv = rel_err(got[0][1], 1.0 / (bv + eps).sqrt())
    note(part, ("bn invstd",) + what, e_inv, 5e-6)
    assert e_inv < 5e-6, ("bn invstd", what, e_inv)
    if special:
        assert abs(got[0][1][2].item() * math.sqrt(eps) - 1.0) < 1e-6, ("invstd of the constant channel", got[0][1][2].item())
    if running:
        e_rm, e_rv = rel_err(got[0][2], rm_ref), rel_err(got[0][3], rv_ref)
        note(part, ("bn running mean",) + what, e_rm, 1e-6)
        note(part, ("bn running var",) + what, e_rv, 2e-6)
        assert e_rm < 1e-6 and e_rv < 2e-6, ("bn running", what, e_rm, e_rv)
        if n * h * w == 1:
            assert rel_err(got[0][3], (1 - mom) * rv.double()) < 2e-6, "one value per channel: the biased variance (0)"
    else:
        assert bool((got[0][2] == 0).all()) and bool((got[0][3] == 0).all())
    gammad, betad = backend.put(gamma), backend.put(beta)
    ys = wide(backend, n, c, h, w, back=16)
    check_producer(lambda: P.bn_train_apply(zs, ys, mean, invstd, gammad, betad, relu), ys, ref, 1e-5, part, ("bn apply",) + what)
    # backward; without ReLU y is never read: it holds NaN
    gy = torch.randn(ref.shape, generator=g) * 1e-2
    if special:
        gy[:, 2] = 0.01           # with a constant gradient the constant channel's dz is 0: what is stored must be finite and about 0
    gs = put_wide(backend, gy, back=24)
    ref.backward(stored(gs))
    ymask = ys if relu else wide(backend, n, c, h, w, back=16)
    dzs = wide(backend, n, c, h, w, back=8)
    dgm, g1 = guarded(backend, (c,))
    dbt, g2 = guarded(backend, (c,))
    ws, g3 = guarded(backend, (nbytes // 4,))
    dz = check_producer(lambda: P.bn_train_bwd(gs, ymask, zs, mean, invstd, gammad, dgm, dbt, dzs, ws, relu), dzs, zd.grad, 2e-5, part,
                        ("bn dz",) + what)
    assert intact(g1) and intact(g2) and intact(g3), ("bn bwd wrote behind a buffer", what)
    e_g, e_b = rel_err(dgm, gd.grad), rel_err(dbt, bd.grad)
    note(part, ("bn dgamma",) + what, e_g, 1e-5)
    note(part, ("bn dbeta",) + what, e_b, 1e-5)
    assert e_g < 1e-5 and e_b < 1e-5, ("bn bwd params", what, e_g, e_b)
    if special:
        assert float(dz[:, 2].abs().max()) <= 2e-5 * float(zd.grad.abs().max()), ("dz of the constant channel", float(dz[:, 2].abs().max()))
    if out32:
        buf, guard = guarded(backend, (n, c, h, w), fill=7.0)
        dz32 = K.attach_amax(buf)
        P.bn_train_bwd(gs, ymask, zs, mean, invstd, gammad, dgm, dbt, dz32, ws, relu)
        assert intact(guard) and intact(g3), ("bn bwd fp32 wrote behind a buffer", what)
        e32 = rel_err(dz32, zd.grad)
        note(part, ("bn dz fp32",) + what, e32, 2e-5)
        assert e32 < 2e-5, ("bn dz fp32", what, e32)
        rmax = float(zd.grad.abs().max())
        assert abs(float(dz32._ssn_amax) - rmax) <= 1e-4 * rmax, ("bn dz fp32 amax", what)


@pytest.mark.parametrize("backend,n,h,w", tiers(NHW_D, NHW_D), indirect=["backend"])
def test_bn_ranges(backend, n, h, w):
    run_bn(backend, n, 24, h, w, "D")


BN_EXTRA = {      # name: (n, c, h, w, relu, bias, running, special)
    "special": (5, 24, 7, 7, True, True, True, True), "special-norelu": (7, 24, 10, 10, False, True, True, True),
    "nobias": (3, 24, 1, 11, True, False, True, False), "norunning": (2, 24, 4, 4, True, True, False, False),
    "norelu": (3, 24, 3, 5, False, True, True, False), "c264": (2, 264, 4, 4, True, True, True, False),
    "c264-norelu-norunning": (1, 264, 1, 31, False, False, False, False),
}


@pytest.mark.parametrize("backend,name", tiers([(k,) for k in BN_EXTRA], [(k,) for k in BN_EXTRA]), indirect=["backend"])
def test_bn_variants(backend, name):
    """a constant channel (invstd = 1 / sqrt(eps), dz about 0) and one with |mean| / sigma = 50; no conv bias; no running statistics;
    no ReLU (y holds NaN: never read); 264 channels: a second workgroup in the *_final kernels.  gamma[1] is negative everywhere"""
    n, c, h, w, relu, bias, running, special = BN_EXTRA[name]
    run_bn(backend, n, c, h, w, "D", relu=relu, bias=bias, running=running, special=special)


# ------------------------------------------------------------------------------------------------------------ E: layout kernels
def _decode(sl):
    """what the planes hold, decoded on the host: (hi + lo) / scale in fp32 -> [N, r8(C), H, W]"""
    t = sl.t
    g0, g1 = _groups(sl)
    raw = t.data[:, :, g0:g1].cpu().float()
    v = (raw[0] + raw[1]) * (1.0 / t.scale.cpu().item())
    return v.permute(0, 1, 3, 2).reshape(t.n, (g1 - g0) * 8, t.h, t.w)


CASES_E = [(c, h, w) for c in (1, 3, 7, 8, 9, 20) for (h, w) in ((1, 1), (5, 7))]


@pytest.mark.parametrize("backend,c,h,w", tiers(CASES_E, CASES_E), indirect=["backend"])
def test_from_to_f32_channel_tails(backend, c, h, w):
    n = 2
    x = torch.randn(n, c, h, w, generator=gen("E cvt", c, h, w)) * 37.0
    sl = wide(backend, n, c, h, w, back=16)
    before = outside(sl)
    store(backend, x, sl)
    assert torch.equal(outside(sl), before), "from_f32 wrote outside its slice"
    dec = _decode(sl)
    assert rel_err(dec[:, :c], x) < T_FWD, (c, h, w)
    raw = inside(sl)
    if c % 8:
        assert bool((raw[:, :, -1, :, c % 8:] == 0).all()), "tail channels of the last group hold zeros in both planes"
    out, guard = guarded(backend, (n, c, h, w))
    P.to_f32(sl, out)
    assert intact(guard), "to_f32 wrote behind its output"
    assert torch.equal(out.cpu(), dec[:, :c]), "to_f32 of the stored values"
    # the delayed protocol into the same slice: two passes around the update, the slot raised to max |x|, never lowered
    xd = backend.put(x)
    sl.t.pool.scale.fill_(1.0)
    got = check_producer(lambda: P.from_f32(xd, sl, exact=False), sl, x.double(), T_FWD, "E", ("from_f32 delayed", c, h, w))
    assert torch.equal(got.float(), _decode(sl)[:, :c])


@pytest.mark.parametrize("backend,c,h,w", tiers([(c, h, w) for c in (3, 5) for (h, w) in ((8, 6), (2, 10), (6, 2))],
                                                [(c, h, w) for c in (3, 5) for (h, w) in ((8, 6), (2, 10), (6, 2))]), indirect=["backend"])
def test_from_f32_space_to_depth(backend, c, h, w):
    n = 2
    x = torch.randn(n, c, h, w, generator=gen("E s2d", c, h, w))
    ref = torch.zeros(n, 4 * c, h // 2, w // 2)
    for ch in range(c):
        for a in range(2):
            for b in range(2):
                ref[:, (ch * 2 + a) * 2 + b] = x[:, ch, a::2, b::2]
    sl = wide(backend, n, 4 * c, h // 2, w // 2, back=8)
    before = outside(sl)
    P.from_f32(backend.put(x), sl, s2d=True)
    assert torch.equal(outside(sl), before), "from_f32 wrote outside its slice"
    assert rel_err(P.to_f32(sl), ref) < T_FWD, (c, h, w)
    assert bool((inside(sl)[:, :, -1, :, 4:] == 0).all())      # (12 and 20 channels: a tail of four)
    xd = backend.put(x)
    sl.t.pool.scale.fill_(1.0)
    check_producer(lambda: P.from_f32(xd, sl, s2d=True, exact=False), sl, ref.double(), T_FWD, "E", ("from_f32 s2d delayed", c, h, w))


IM2COL = [(3, 3, 2, 0, 0), (1, 7, 1, 0, 3), (7, 1, 1, 3, 0), (3, 5, 2, 1, 2), (2, 2, 2, 0, 0)]


@pytest.mark.parametrize("backend,c,kh,kw,s,ph,pw", tiers([(c,) + k for c in (3, 10) for k in IM2COL], [(c,) + k for c in (3, 10) for k in IM2COL]),
                         indirect=["backend"])
def test_im2col_taps_and_slices(backend, c, kh, kw, s, ph, pw):
    n, h, w = 2, 9, 11
    xs = put_wide(backend, torch.randn(n, c, h, w, generator=gen("E im2col", c, kh, kw)), back=8)
    ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
    kk = c * kh * kw
    before = xs.t.data.view(torch.int16).clone().cpu()
    y = P.im2col(xs, kh, kw, s, ph, pw, ho, wo)
    assert torch.equal(xs.t.data.view(torch.int16).cpu(), before)
    ref = F.unfold(P.to_f32(xs).cpu(), (kh, kw), padding=(ph, pw), stride=s).view(n, kk, ho, wo)
    assert torch.equal(P.to_f32(P.PSlice(y, 0, kk)).cpu(), ref), (c, kh, kw, s, ph, pw)
    assert y.g == (kk + 7) // 8
    if y.g * 8 > kk:
        assert bool((y.data.view(torch.int16).cpu()[:, :, -1, :, kk % 8:] == 0).all()), "the channels that pad K hold zeros"
    y2 = P.im2col(xs, kh, kw, s, ph, pw, ho, wo)
    assert torch.equal(y2.data.view(torch.int16).cpu(), y.data.view(torch.int16).cpu())


CLAMPED = ["maxpool_fwd", "avgpool_affine", "bn_train_apply", "maxpool_bwd", "gap_bwd", "from_f32"]


def clamp_check(launch, dst, ref, tol, what):
    """the destination's scale set so that max |ref| lands 4 - 8 times above the f16 range: what is stored is clamp(ref), finite, and
    the slot holds the TRUE maximum"""
    ref = ref.detach()
    rmax = ref.abs().max().item()
    scale = 2.0 ** math.ceil(math.log2(4 * F16_MAX / rmax))
    assert 64 * rmax * scale > F16_MAX and rmax * scale >= 4 * F16_MAX
    lim = F16_MAX / scale
    assert float((ref.abs() > lim).double().mean()) > 0.01, "nothing to clamp"
    dst.t.pool.scale.fill_(scale)
    dst.t.amax.zero_()
    before = outside(dst)
    launch()
    got = stored(dst)
    assert bool(torch.isfinite(got).all()), ("non-finite values stored", what)
    err = rel_err(got, ref.clamp(-lim, lim))
    note("E", ("clamp", what), err, tol)
    assert err < tol, ("clamp", what, err)
    ok, figs = amax_close(dst.t, rmax)
    assert ok, ("amax under the clamp", what, figs)
    assert torch.equal(outside(dst), before)


@pytest.mark.parametrize("backend,family", tiers([(f,) for f in CLAMPED], [(f,) for f in CLAMPED]), indirect=["backend"])
def test_producers_clamp_and_record_the_true_maximum(backend, family):
    n, c, h, w = 2, 16, 6, 7
    g = gen("E clamp", family)
    x = torch.randn(n, c, h, w, generator=g)
    xs = put_wide(backend, x)
    xv = stored(xs)
    if family == "maxpool_fwd":
        ref = F.max_pool2d(xv - 0.0, 3, 2, 1, ceil_mode=True)
        ys = wide(backend, n, c, ref.shape[2], ref.shape[3], back=16)
        clamp_check(lambda: P.maxpool_fwd(xs, ys, None, 3, 2, 1), ys, ref, T_FWD, family)
    elif family == "avgpool_affine":
        sc, sh = backend.put(torch.rand(c, generator=g) + 0.5), backend.put(torch.randn(c, generator=g))
        ref = F.avg_pool2d(xv, 3, 1, 1, count_include_pad=True) * sc.cpu().double().view(1, -1, 1, 1) + sh.cpu().double().view(1, -1, 1, 1)
        ys = wide(backend, n, c, h, w, back=16)
        clamp_check(lambda: P.avgpool_affine(xs, ys, sc, sh, False, 3, 1), ys, ref, T_AVG, family)
    elif family == "bn_train_apply":
        gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
        mean, invstd = backend.put(torch.empty(c)), backend.put(torch.empty(c))
        ws = backend.put(torch.empty(P.bn_train_workspace_bytes(c) // 4))
        P.bn_train_stats(xs, None, mean, invstd, None, None, 1e-5, 0.1, ws)
        ref = F.batch_norm(xv, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)
        ys = wide(backend, n, c, h, w, back=16)
        clamp_check(lambda: P.bn_train_apply(xs, ys, mean, invstd, backend.put(gamma), backend.put(beta), False), ys, ref, 1e-5, family)
    elif family == "maxpool_bwd":
        xr = xv.clone().requires_grad_()
        out, _ = F.max_pool2d(xr, 3, 2, 1, ceil_mode=True, return_indices=True)
        ys = wide(backend, n, c, out.shape[2], out.shape[3], back=16)
        am = backend.put(torch.zeros((n, c // 8, out.shape[2] * out.shape[3], 8), dtype=torch.uint8))
        _two_pass(lambda: P.maxpool_fwd(xs, ys, am, 3, 2, 1), ys.t)
        gs = put_wide(backend, torch.randn(out.shape, generator=g))
        out.backward(stored(gs))
        ds = wide(backend, n, c, h, w, back=16)
        clamp_check(lambda: P.maxpool_bwd(gs, am, ds, 3, 2, 1), ds, xr.grad, T_BWD, family)
    elif family == "gap_bwd":
        dfeat = torch.randn(n, c, generator=g)
        ds = wide(backend, n, c, h, w, back=16)
        ref = (dfeat.double() / (h * w)).view(n, c, 1, 1).expand(n, c, h, w)
        clamp_check(lambda: P.gap_bwd(backend.put(dfeat), ds), ds, ref, T_AVG, family)
    else:
        ds = wide(backend, n, c, h, w, back=16)
        clamp_check(lambda: P.from_f32(backend.put(x), ds, exact=False), ds, x.double(), T_FWD, family)


# ------------------------------------------------------------------------------------------------------------ F: large launches
TRIP = 2048 * 256      # work items of one trip of a grid-stride loop under the production grid cap
BIG = (2, 16, 363, 362)      # N, C, H, W: 525624 sixteen-byte groups


def _two_trips(items):
    assert items > TRIP and items % TRIP != 0, items


LARGE_POOLS = {      # name: (H, W, k, s, pad, variants): the forward kernel + the backward kernels named
    "k3s2-fast": (725, 723, 3, 2, 1, ("plain",)),                 # fwd k3 fast <2>, bwd k3s2 fast <1, no mask>
    "k3s2-fast-masked": (725, 723, 3, 2, 1, ("pooled",)),         # bwd k3s2 fast <1, mask>
    "k3s2-blocks": (727, 725, 3, 2, 0, ("f32", "acc")),           # bwd k3s2 general <0>: fp32 (odd W) and accumulating planes stores
    "k3s1": (363, 362, 3, 1, 1, ("plain",)),                      # fwd k3 fast <1>, bwd <3, 1>
    "k2s2": (726, 724, 2, 2, 0, ("plain",)),                      # fwd general, bwd <0, 0>
}


@pytest.mark.parametrize("backend,name", tiers([(k,) for k in LARGE_POOLS], []), indirect=["backend"])
def test_large_maxpool(backend, name):
    h, w, k, s, pad, variants = LARGE_POOLS[name]
    n, c = BIG[0], BIG[1]
    ho = F.max_pool2d(torch.zeros(1, 1, h, w), k, s, pad, ceil_mode=True).shape
    _two_trips(n * c // 8 * ho[2] * ho[3])
    _two_trips(n * c // 8 * ((h + 1) // 2) * ((w + 1) // 2) if (k, s) == (3, 2) else n * c // 8 * h * w)
    run_maxpool(backend, n, c, h, w, k, s, pad, True, "F", variants)


@pytest.mark.parametrize("backend,k", tiers([(3,), (5,)], []), indirect=["backend"])
def test_large_avgpool(backend, k):
    _two_trips(BIG[0] * BIG[1] // 8 * BIG[2] * BIG[3])
    run_avgpool(backend, BIG[0], BIG[1], BIG[2], BIG[3], k, 1, 1, "F")


@pytest.mark.parametrize("backend", tiers([()], []), indirect=["backend"])
def test_large_relu_bn_and_gap_bwd(backend):
    run_relu_gap(backend, BIG[0], BIG[1], BIG[2], BIG[3], "F", gap_fwd=False)


@pytest.mark.parametrize("backend", tiers([()], []), indirect=["backend"])
def test_large_bn(backend):
    """pl_bn_apply_kernel, pl_bn_bwd_apply_kernel (planes and fp32 stores) on a second trip of bnp_grid's 2048 workgroups"""
    run_bn(backend, BIG[0], BIG[1], BIG[2], BIG[3], "F")


@pytest.mark.parametrize("backend", tiers([()], []), indirect=["backend"])
def test_large_layout(backend):
    n, c, h, w = BIG
    x = torch.randn(n, c, h, w, generator=gen("F cvt"))
    sl = wide(backend, n, c, h, w, back=8)
    before = outside(sl)
    store(backend, x, sl)
    assert torch.equal(outside(sl), before)
    assert rel_err(_decode(sl), x) < T_FWD
    out, guard = guarded(backend, (n, c, h, w))
    P.to_f32(sl, out)
    assert intact(guard) and torch.equal(out.cpu(), _decode(sl))
    xd = backend.put(x)
    sl.t.pool.scale.fill_(1.0)
    check_producer(lambda: P.from_f32(xd, sl, exact=False), sl, x.double(), T_FWD, "F", "from_f32 delayed")
    # im2col: 2 x 4 groups of K = 27 x 260 x 258 pixels
    n, c, h, w = 2, 3, 260, 258
    _two_trips(n * 4 * h * w)
    xs = put_wide(backend, torch.randn(n, c, h, w, generator=gen("F im2col")), back=8)
    y = P.im2col(xs, 3, 3, 1, 1, 1, h, w)
    ref = F.unfold(P.to_f32(xs).cpu(), 3, padding=1, stride=1).view(n, 27, h, w)
    assert torch.equal(P.to_f32(P.PSlice(y, 0, 27)).cpu(), ref)
    assert bool((y.data.view(torch.int16)[:, :, -1, :, 3:] == 0).all())


CHILD_K = "emu and (test_maxpool_every_variant or test_avgpool_every_variant or test_relu_bn_gap_every_size)"


def test_one_workgroup_grid_gives_the_same_results(emu_library):
    """the CPU-tier cases of parts A - C once more in a fresh interpreter whose grid_for caps every launch of planes_ops.hip at ONE
    workgroup (SSN_PL_GRID_CAP=1, read once per process): every grid-stride loop takes as many trips as the case has work, the per-thread
    maximum is carried across them"""
    env = dict(os.environ, SSN_PL_GRID_CAP="1", SSN_EMU_LIB=os.path.abspath(emu_library.path))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", CHILD_K],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    tail = r.stdout[-3000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= len(EMU_A) + len(EMU_B) + len(EMU_C), tail
    assert not re.search(r"\d+ (failed|error)", r.stdout), tail


# ------------------------------------------------------------------------------------------------------------ G: the 2 GiB fall-backs
G_N, G_C, G_H, G_W = 2, 16, 29, 29


def _fits32(n, img_groups, g, hw):
    return ((n - 1) * img_groups + g) * hw * 16 <= (1 << 31)


def big_slice(backend, h, w, above):
    """the last G_C channels of an N = 2 tensor whose planes end just above / just below what the 32-bit kernels can address"""
    g, hw = G_C // 8, h * w
    lim = (1 << 31) // (hw * 16)
    ig = lim - g + (8 if above else -2)
    assert _fits32(G_N, ig, g, hw) != above and abs((ig + g) * hw * 16 - (1 << 31)) < 16 * 16 * hw
    t = P.PlaneTensor(G_N, ig * 8, h, w, backend.device)
    return P.PSlice(t, (ig - g) * 8, G_C)


def _g_inputs(backend):
    g = gen("G")
    x = torch.randn(G_N, G_C, G_H, G_W, generator=g) - 0.5
    xs = put_wide(backend, x)
    xv = stored(xs).requires_grad_()
    ref, _ = F.max_pool2d(xv, 3, 2, 1, ceil_mode=True, return_indices=True)
    gy = torch.randn(ref.shape, generator=g)
    msc = torch.randn(G_C, generator=g)
    msc[::5] = NAN
    return x, xs, xv, ref, gy, msc


def _like(backend, src, n, c, h, w):
    """a compact NaN-surrounded destination that shares the scale of src"""
    sl = wide(backend, n, c, h, w, back=16)
    sl.t.pool.scale.copy_(src.t.pool.scale)
    return sl


@pytest.mark.parametrize("backend,which,above", tiers([(wh, a) for wh in ("x", "y", "dy", "dx", "mask") for a in (1, 0)], []),
                         indirect=["backend"])
def test_two_gib_predicate_from_both_sides(backend, which, above):
    """one 8.6 GB tensor (allocated, never filled) holds one operand as its last two groups: above the limit every call must take the
    kernels with 64-bit indexing, below it the 32-bit ones; both must give the bytes of the call on compact tensors"""
    if torch.cuda.mem_get_info()[0] < 24e9:
        pytest.skip("less than 24 GB of device memory free")
    try:
        _two_gib_case(backend, which, above)
    finally:
        torch.cuda.empty_cache()      # (the wide tensor is freed before the next case allocates its own)


def _two_gib_case(backend, which, above):
    x, xs, xv, ref, gy, msc = _g_inputs(backend)
    n, c, h, w = G_N, G_C, G_H, G_W
    ho, wo = ref.shape[2], ref.shape[3]
    mscd = backend.put(msc)

    def same(a, b, what):
        assert torch.equal(inside(a), inside(b)), ("differs from the call on compact tensors", which, above, what)
    if which in ("x", "y"):
        if which == "x":
            bx = big_slice(backend, h, w, above)
            store(backend, x, bx)
            assert torch.equal(inside(bx), inside(xs))
        for (k, s, pad) in ((3, 2, 0), (3, 1, 1)) if which == "x" else ():
            r64 = F.max_pool2d(xv.detach(), k, s, pad, ceil_mode=True)
            res = []
            for src in (xs, bx):
                ys = wide(backend, n, c, r64.shape[2], r64.shape[3], back=16)
                if res:
                    ys.t.pool.scale.copy_(res[0][0].t.pool.scale)
                am, guard = guarded(backend, (n, c // 8, r64.shape[2] * r64.shape[3], 8), torch.uint8, 0xEE)
                if res:
                    P.maxpool_fwd(src, ys, am, k, s, pad)
                else:
                    _two_pass(lambda: P.maxpool_fwd(src, ys, am, k, s, pad), ys.t)
                assert intact(guard)
                res.append((ys, am))
            same(res[0][0], res[1][0], ("maxpool fwd", k, s, pad))
            assert torch.equal(res[0][1].cpu(), res[1][1].cpu()), ("argmax", k, s, pad)
            err = rel_err(stored(res[1][0]), r64)
            note("G", ("maxpool fwd", which, above, k, s, pad), err, T_FWD)
            assert err < T_FWD
        r64 = F.avg_pool2d(xv.detach(), 3, 1, 1, count_include_pad=True)
        yc = wide(backend, n, c, h, w, back=16)
        _two_pass(lambda: P.avgpool_affine(xs, yc, None, None, False, 3, 1), yc.t)
        if which == "x":
            yb = _like(backend, yc, n, c, h, w)
            P.avgpool_affine(bx, yb, None, None, False, 3, 1)
        else:
            yb = big_slice(backend, h, w, above)
            yb.t.pool.scale.copy_(yc.t.pool.scale)
            P.avgpool_affine(xs, yb, None, None, False, 3, 1)
        same(yc, yb, "avgpool")
        err = rel_err(stored(yb), r64)
        note("G", ("avgpool", which, above), err, T_AVG)
        assert err < T_AVG
    else:
        k, s, pad = 3, 2, 1
        ys = wide(backend, n, c, ho, wo, back=16)
        am = backend.put(torch.zeros((n, c // 8, ho * wo, 8), dtype=torch.uint8))
        _two_pass(lambda: P.maxpool_fwd(xs, ys, am, k, s, pad), ys.t)
        gs = put_wide(backend, gy)
        ref.backward(stored(gs))
        m = mask_factor(xv.detach(), msc)
        big_gs, big_mask = gs, ys
        if which == "dy":
            big_gs = big_slice(backend, ho, wo, above)
            store(backend, gy, big_gs)
            assert torch.equal(inside(big_gs), inside(gs))
        if which == "mask":
            big_mask = big_slice(backend, ho, wo, above)
            big_mask.t.pool.scale.copy_(ys.t.pool.scale)
            P.maxpool_fwd(xs, big_mask, None, k, s, pad)
            assert torch.equal(inside(big_mask), inside(ys))
        big_dx = big_slice(backend, h, w, above) if which == "dx" else None
        for pooled in ((False, True) if which != "mask" else (True,)):
            kw = dict(mask=ys, mask_scale=mscd, mask_pooled=True) if pooled else {}
            dc = wide(backend, n, c, h, w, back=16)
            _two_pass(lambda: P.maxpool_bwd(gs, am, dc, k, s, pad, **kw), dc.t)
            if pooled:
                kw["mask"] = big_mask
            db = big_dx if big_dx is not None else wide(backend, n, c, h, w, back=16)
            db.t.pool.scale.copy_(dc.t.pool.scale)
            P.maxpool_bwd(big_gs, am, db, k, s, pad, **kw)
            same(dc, db, ("maxpool bwd", "pooled" if pooled else "plain"))
            want = xv.grad * m if pooled else xv.grad
            err = rel_err(stored(db), want)
            note("G", ("maxpool bwd", which, above, pooled), err, T_BWD)
            assert err < T_BWD


# ------------------------------------------------------------------------------------------------------------ H: argument errors
@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_argument_errors(backend):
    n, c, h, w = 1, 16, 6, 6
    x = P.from_f32(backend.put(torch.randn(n, c, h, w, generator=gen("H"))))
    xs = P.pfull(x)

    def dest(hh, ww, cc=c):
        t = P.PlaneTensor(n, cc, hh, ww, backend.device)
        t.data.fill_(7.0)
        return t

    def refused(fn, *dsts):
        with pytest.raises(RuntimeError):
            fn()
        for d in dsts:
            d = d.data if isinstance(d, P.PlaneTensor) else d
            assert bool((d == 7.0).all()), "a refused call wrote to its destination"
    y3, yf = dest(3, 3), dest(h, w)
    am = backend.put(torch.zeros((n, c // 8, 9, 8), dtype=torch.uint8))
    refused(lambda: P.maxpool_fwd(P.PSlice(x, 0, 12), P.PSlice(y3, 0, 12), am, 3, 2, 0), y3)            # C % 8
    refused(lambda: P.maxpool_fwd(xs, P.pfull(y3), am, 16, 2, 0), y3)                                   # k > 15
    refused(lambda: P.maxpool_fwd(xs, P.pfull(y3), am, 3, 0, 0), y3)                                    # s < 1
    refused(lambda: P.avgpool_affine(xs, P.pfull(yf), None, None, False, 3, 0), yf)                     # 2 pad != k - 1
    refused(lambda: P.avgpool_affine(xs, P.pfull(yf), None, None, False, 4, 1), yf)
    one = backend.put(torch.ones(c))
    refused(lambda: P.avgpool_affine(xs, P.pfull(yf), one, None, False, 3, 1), yf)                      # scale without shift
    refused(lambda: P.avgpool_affine(P.PSlice(x, 0, 12), P.PSlice(yf, 0, 12), None, None, False, 3, 1), yf)
    # max pool backward: dy 3 x 3 -> dx 6 x 6
    gy = P.pfull(P.from_f32(backend.put(torch.randn(n, c, 3, 3, generator=gen("H gy")))))
    pooled = P.pfull(P.from_f32(backend.put(torch.randn(n, c, 3, 3, generator=gen("H y")))))
    refused(lambda: P.maxpool_bwd(gy, am, P.pfull(yf), 2, 2, 0, mask=pooled, mask_scale=one, mask_pooled=True), yf)      # pooled mask, k != 3
    refused(lambda: P.maxpool_bwd(gy, am, P.pfull(yf), 3, 2, 0, accumulate=True, mask=pooled, mask_scale=one, mask_pooled=True), yf)
    refused(lambda: P.maxpool_bwd(gy, am, P.pfull(yf), 3, 2, 2, mask=pooled, mask_scale=one, mask_pooled=True), yf)      # pad 2
    refused(lambda: P.maxpool_bwd(gy, am, P.pfull(yf), 3, 2, 0, mask_pooled=True), yf)                                   # no mask at all
    refused(lambda: P.maxpool_bwd(gy, None, P.pfull(yf), 3, 2, 0), yf)                                                  # no argmax
    refused(lambda: P.maxpool_bwd(P.PSlice(gy.t, 0, 12), am, P.PSlice(yf, 0, 12), 3, 2, 0), yf)
    lib = _lib()
    dx32 = backend.put(torch.full((n, c, h, w), 7.0))
    amax = backend.put(torch.zeros(1))
    refused(lambda: lib.call("ssn_pl_maxpool_bwd", gy.hi, gy.lo, gy.groups, am.data_ptr(), None, None, 0, n, c, h, w, 3, 3, 3, 2, 0, 1, None, 0,
                             None, 0, gy.t.scale_ptr, one.data_ptr(), amax.data_ptr(), dx32.data_ptr(), c * h * w, K._stream(lib, dx32)),
            dx32)                                                                                                       # fp32 output + accumulate
    # workspaces one float short
    out = backend.put(torch.full((c,), 7.0))
    out2 = backend.put(torch.full((c,), 7.0))
    short = backend.put(torch.empty(P.channel_sum_workspace_bytes(c) // 4 - 1))
    refused(lambda: P.channel_sum(xs, out, short), out)
    refused(lambda: P.channel_sum_multi([(xs, out), (xs, out2)], backend.put(torch.empty(P.channel_sum_workspace_bytes(2 * c) // 4 - 1))),
            out, out2)
    refused(lambda: P.channel_sum(P.PSlice(x, 0, 12), out, backend.put(torch.empty(1024))), out)
    bshort = backend.put(torch.empty(P.bn_train_workspace_bytes(c) // 4 - 1))
    bws = backend.put(torch.empty(P.bn_train_workspace_bytes(c) // 4))
    mean, invstd = backend.put(torch.full((c,), 7.0)), backend.put(torch.full((c,), 7.0))
    rm = backend.put(torch.full((c,), 7.0))
    refused(lambda: P.bn_train_stats(xs, None, mean, invstd, None, None, 1e-5, 0.1, bshort), mean, invstd)
    refused(lambda: P.bn_train_stats(xs, None, mean, invstd, rm, None, 1e-5, 0.1, bws), mean, invstd, rm)           # running mean alone
    refused(lambda: P.bn_train_stats(P.PSlice(x, 0, 12), None, mean, invstd, None, None, 1e-5, 0.1, bws), mean, invstd)
    refused(lambda: P.bn_train_apply(P.PSlice(x, 0, 12), P.PSlice(yf, 0, 12), one, one, one, one, True), yf)
    dg, dbt = backend.put(torch.full((c,), 7.0)), backend.put(torch.full((c,), 7.0))
    refused(lambda: P.bn_train_bwd(xs, xs, xs, one, one, one, dg, dbt, P.pfull(yf), bshort, True), yf, dg, dbt)
    # layout kernels
    s2 = dest(2, 3, 12)
    refused(lambda: P.from_f32(backend.put(torch.randn(n, 3, 5, 6)), s2, s2d=True, exact=False), s2)                # odd height
    refused(lambda: P.from_f32(backend.put(torch.randn(n, 3, 4, 7)), s2, s2d=True, exact=False), s2)                # odd width
    lib.call("ssn_pl_channel_sum_multi", 0, None, None, None, None, n, None, None, None, None, 0, K._stream(lib, out))
    with pytest.raises(RuntimeError):
        lib.call("ssn_pl_channel_sum_multi", -1, None, None, None, None, n, None, None, None, None, 0, K._stream(lib, out))
