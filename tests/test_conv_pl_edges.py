"""The planes convolution kernels (csrc/conv_pl.hip, conv_pl_epilogue.inc: conv_pl_kernel, conv_pl9_kernel behind ssn_conv_pl_fwd /
ssn_conv_pl_dgrad / ssn_conv_pl_dgrad_s2) at every tile, tap shape and ragged edge, against plain float64 torch on the CPU
(F.conv2d, autograd of it for the gradients).

  A  every (kind, taps, stride, H, tile) class of the autotuned table tuned_tiles_pl.json, launched with its production tile at a batch
     a test can afford, plus the two space-to-depth stems (GPU tier);
  B  every plain tile and every haloed tile at the smallest shapes that have every edge: a ragged last m-tile with an 8-row partial
     block, M = 24, a ragged last pixel tile, tiles that cross images, an 8-channel tail slab, problems of 1 - 3 slabs (fewer than
     the LDS ring has slots);
  C  what the fused launches of the executor pass, on tiles where a row split of 64 falls inside an m-tile: a source slice, no ReLU,
     row split + gap + raw rows, k_split / k_gap of dgrad, stride-2 dgrad between slices of wider tensors;
  D  the recorded maximum must not see padded pixels or rows.

Tolerances are those of tests/test_planes.py (3e-6 forward / plain dgrad, 4e-6 masked or accumulated dgrad, relative to the largest
magnitude of the reference; the recorded maximum within 1e-4).  The CPU tier runs subsets through the host emulator (B: tiles 3, 6, 7
with 1x1 and 3x3 pad 1; C: tile 7; D: tile 3); the GPU tier runs everything.

Wall time of this file as measured: GPU tier, one MI355X, 171 tests in 7.4 s; CPU tier, host emulator, 13 tests in 290 s (the three
test_tile_edges cases take 225 s of it).
"""
import ctypes
import json
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

import action_detection_amd
from action_detection_amd import kernels as K
from action_detection_amd import planes as P
from action_detection_amd import bninception_spec, inceptionv3_spec

from test_planes import HALO_PI_TILES, HALO_TILES, _pack_fwd, _two_pass, rel_err

GPU = pytest.mark.gpu
PLAIN_TILES = list(range(12))


def _cdll():
    return action_detection_amd._lib.get_lib().cdll


def tile_shape(tile):
    bm, bn = ctypes.c_int(0), ctypes.c_int(0)
    assert _cdll().ssn_conv_pl_tile_shape(plain_of(tile), ctypes.byref(bm), ctypes.byref(bn)) == 0
    return bm.value, bn.value


def plain_of(tile):
    return tile - 48 if tile >= 48 else (tile - 32 if tile >= 32 else tile)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def tiers(gpu_cases, emu_cases):
    """parameters (backend, *case): the emulator runs emu_cases, the GPU tier gpu_cases"""
    out = [pytest.param("emu", *c, id="emu-" + "-".join(map(str, c))) for c in emu_cases]
    return out + [pytest.param("gpu", *c, marks=GPU, id="gpu-" + "-".join(map(str, c))) for c in gpu_cases]


def amax_close(t, want):
    got = t.amax.cpu().item()
    return abs(got - want) <= 1e-4 * want, (got, want)


def put_planes(backend, x):
    """x as channels [0, C) of a planes tensor one channel group wider whose last group holds NaN in both planes: what lies behind a
    slice must never reach the matrix cores (the upper half of an 8-channel tail slab would fetch exactly that group; the packed weights
    are zero there, and 0 x NaN is NaN)"""
    n, c, h, w = x.shape
    t = P.PlaneTensor(n, c + 8, h, w, backend.device)
    t.data.fill_(float("nan"))
    P.from_f32(backend.put(x), P.PSlice(t, 0, c))
    return P.PSlice(t, 0, c)


# ------------------------------------------------------------------------------------------------------------ forward
def fwd_inputs(case, g):
    n, cin, h, wd, cout, kh, kw, s, ph, pw = case
    x = torch.randn(n, cin, h, wd, generator=g) * 3.0
    w = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    return x, w, scale, shift


def run_fwd(backend, x, w, scale, shift, s, ph, pw, tile, relu=True, crop=None, src=None, tol=3e-6, what="", ref_check=None):
    """conv + affine (+ ReLU) into channels [16, 16 + cout) of a tensor 48 channels wider that holds 7.0, two passes around the scale
    update; the float64 reference, the recorded maximum of either pass, the bytes outside the slice.  src: the source as a PSlice
    (x then holds the values stored there); ref_check(ref): what the caller asserts of the reference before the kernel runs."""
    n, cin = x.shape[0], x.shape[1]
    cout, _, kh, kw = w.shape
    ref = F.conv2d(x.double(), w.double(), None, s, (ph, pw))
    if crop is not None:
        ref = ref[:, :, :crop, :crop]
    ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if relu:
        ref = F.relu(ref)
    if ref_check is not None:
        ref_check(ref)
    ho, wo = ref.shape[2], ref.shape[3]
    rmax = ref.abs().max().item()
    if src is None:
        src = put_planes(backend, x)
    wp = _pack_fwd(w, backend)
    c0 = 16
    y = P.PlaneTensor(n, cout + 48, ho, wo, backend.device)
    y.data.fill_(7.0)
    for _ in range(2):
        P.conv_fwd(src, wp, backend.put(scale), backend.put(shift), P.PSlice(y, c0, cout), kh, kw, s, ph, pw, relu, tile)
        ok, figs = amax_close(y, rmax)
        print("  fwd amax", what, tile, figs, flush=True)
        assert ok, ("y.amax", what, tile, figs)
        y.pool.update()
    err = rel_err(P.to_f32(P.PSlice(y, c0, cout)), ref)
    print("  fwd err %.3g" % err, what, tile, flush=True)
    assert err < tol, ("fwd", what, tile, err)
    raw = y.data.cpu().float()
    assert (raw[:, :, :c0 // 8] == 7.0).all() and (raw[:, :, (c0 + cout) // 8:] == 7.0).all(), ("wrote outside its slice", what, tile)
    return ref


# ------------------------------------------------------------------------------------------------------------ data gradient
def dgrad_inputs(case, g, gy_fn=None, w_fn=None):
    """weights, dY and the float64 autograd data gradient of F.conv2d"""
    n, cin, h, wd, cout, kh, kw, s, ph, pw = case
    x = torch.zeros(n, cin, h, wd, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, kh, kw, generator=g) * 0.1 if w_fn is None else w_fn((cout, cin, kh, kw))
    y = F.conv2d(x, w.double(), None, s, (ph, pw))
    gy = torch.randn(y.shape, generator=g) * 1e-3 if gy_fn is None else gy_fn(y.shape)
    y.backward(gy.double())
    return w, gy, x.grad.detach()


def pack_dgrad(w, s, backend):
    """as planes_exec._pack_dgrad: parity sections for 3x3 / stride 2, transposed + tap-reversed for the non-square taps, pack mode 1"""
    kh, kw = w.shape[2], w.shape[3]
    if s == 2:
        assert (kh, kw) == (3, 3)
        return K.pack_dgrad_s2(backend.put(w)), False
    if kh == kw and kh in (1, 3):
        return K.pack_weights_multi([([backend.put(w)], 1)], x6=True)[0], False
    return K.pack_dgrad_rect(backend.put(w)), True


def mask_inputs(n, cin, h, wd, g, ones=False):
    """forward activation (about half of it zero), mask scale with NaN (pass-through) channels, the float64 factor they stand for"""
    act = torch.randn(n, cin, h, wd, generator=g).clamp(min=0)
    msc = torch.ones(cin) if ones else torch.randn(cin, generator=g)
    msc[::5] = float("nan")
    m = torch.where(torch.isnan(msc).view(1, -1, 1, 1), torch.ones_like(act),
                    (act > 0).float() * torch.nan_to_num(msc).view(1, -1, 1, 1)).double()
    return act, msc, m


def launch_dgrad(gs, wt, dxs, case, tile, rev, **kw):
    kh, kw_, s, ph, pw = case[5:]
    if s == 2:
        P.conv_dgrad_s2(gs, wt, dxs, ph, tile_cfg=tile, **kw)
    else:
        P.conv_dgrad(gs, wt, dxs, kh, kw_, ph, pw, tile_cfg=tile, taps_reversed=rev, **kw)


def run_dgrad_masked(backend, case, tile, g, what=""):
    """one masked launch (two passes): dx = d * mask"""
    n, cin, h, wd = case[:4]
    w, gy, dref = dgrad_inputs(case, g)
    act, msc, m = mask_inputs(n, cin, h, wd, g)
    wt, rev = pack_dgrad(w, case[7], backend)
    gs, actp = put_planes(backend, gy), P.from_f32(backend.put(act))
    dx = P.PlaneTensor(n, cin, h, wd, backend.device)
    dx.data.fill_(3.0)
    _two_pass(lambda: launch_dgrad(gs, wt, P.pfull(dx), case, tile, rev, mask=P.pfull(actp), mask_scale=backend.put(msc)), dx)
    ref = dref * m
    err = rel_err(P.to_f32(dx), ref)
    ok, figs = amax_close(dx, ref.abs().max().item())
    print("  dgrad masked err %.3g amax" % err, figs, what, tile, flush=True)
    assert err < 4e-6, ("dgrad mask", what, tile, err)
    assert ok, ("dx.amax", what, tile, figs)


def run_dgrad_plain_acc(backend, case, tile, g, what=""):
    """plain (two passes), then accumulate + mask on top of a plain one: dx = 2 d mask, as tests/test_planes.py::test_conv_pl_dgrad"""
    n, cin, h, wd = case[:4]
    w, gy, dref = dgrad_inputs(case, g)
    act, msc, m = mask_inputs(n, cin, h, wd, g)
    wt, rev = pack_dgrad(w, case[7], backend)
    gs, actp = put_planes(backend, gy), P.from_f32(backend.put(act))
    dx = P.PlaneTensor(n, cin, h, wd, backend.device)
    dx.data.fill_(3.0)
    dmax = dref.abs().max().item()
    for _ in range(2):
        launch_dgrad(gs, wt, P.pfull(dx), case, tile, rev)
        ok, figs = amax_close(dx, dmax)
        assert ok, ("dx.amax", what, tile, figs)
        dx.pool.update()
    err = rel_err(P.to_f32(dx), dref)
    print("  dgrad err %.3g" % err, what, tile, flush=True)
    assert err < 3e-6, ("dgrad", what, tile, err)
    ref = 2 * dref * m
    for _ in range(2):
        launch_dgrad(gs, wt, P.pfull(dx), case, tile, rev)                                                      # dx = d
        launch_dgrad(gs, wt, P.pfull(dx), case, tile, rev, accumulate=True, mask=P.pfull(actp),
                     mask_scale=backend.put(msc))                                                                            # dx = mask(2 d)
        ok, figs = amax_close(dx, max(dmax, ref.abs().max().item()))      # (the slot keeps the larger of the two launches)
        assert ok, ("dx.amax accumulate", what, tile, figs)
        dx.pool.update()
    err = rel_err(P.to_f32(dx), ref)
    print("  dgrad acc + mask err %.3g" % err, what, tile, flush=True)
    assert err < 4e-6, ("dgrad mask", what, tile, err)


# ------------------------------------------------------------------------------------------------------------ A: the tuned table
with open(os.path.join(os.path.dirname(P.__file__), "tuned_tiles_pl.json")) as _f:
    _TABLE = json.load(_f)["tiles"]
_BN_OF = {0: 128, 1: 128, 2: 64, 3: 64, 4: 128, 5: 128, 6: 256, 7: 128, 8: 128, 9: 128, 10: 256, 11: 64}      # (asserted against the library below)


def _classes(kind):
    """one row per (kind, kh, kw, stride, H, tile): the one with the smallest cin * cout; rows of the stems (cin % 8) left out"""
    best = {}
    for key, tile in _TABLE.items():
        f = key.split("|")
        if f[0] != kind:
            continue
        cin, cout, kh, kw, s, h = map(int, f[1:])
        if cin % 8:
            continue
        cls = (kh, kw, s, h, int(tile))
        if cls not in best or cin * cout < best[cls][0] * best[cls][1]:
            best[cls] = (cin, cout)
    return [(cin, cout) + cls for cls, (cin, cout) in sorted(best.items())]


def _spec_pads(cin, cout, kh, kw, s, h):
    """paddings the two backbone manifests give a layer of this shape"""
    found = set()
    ops, tensors = inceptionv3_spec.build_manifest()
    for op in ops:
        if op[0] == "conv" and tuple(op[5:10]) == (cin, cout, kh, kw, s) and tensors[op[2]][1] == h:
            found.add((op[10], op[11]))
    ops, tensors = bninception_spec.build_manifest()
    for op in ops:
        if op[0] == "conv" and kh == kw and tuple(op[5:9]) == (cin, cout, kh, s) and tensors[op[2]][1] == h:
            found.add((op[9], op[9]))
    return found


def _pad_of(cin, cout, kh, kw, s, h):
    spec = _spec_pads(cin, cout, kh, kw, s, h)
    assert len(spec) <= 1, spec
    if (kh, kw) == (3, 3) and s == 2:
        rule = (1, 1) if h % 2 == 0 else (0, 0)          # BN-Inception (even sizes, pad 1) / Inception-v3 (odd sizes, pad 0)
    elif (kh, kw) == (3, 3) and h in (7, 14, 28, 35, 56, 8):
        rule = (1, 1)
    elif (kh, kw) == (3, 3):
        assert spec, "a 3x3 layer of the stems: its padding comes from the manifest"
        rule = next(iter(spec))
    else:
        rule = (kh // 2, kw // 2)                          # 1x1, and the same-size 1x3 / 3x1 / 1x7 / 7x1 / 5x5 layers
    assert not spec or spec == {rule}, (spec, rule)       # (fused launches have no manifest row of their own)
    return rule


def _batch(pixels, bn, h):
    if h >= 73:
        return 1
    n = 3
    while n * pixels <= bn:
        n += 1
    return n


FWD_CLASSES, DGRAD_CLASSES = _classes("fwd"), _classes("dgrad")


def test_table_classes_and_tile_list(backend):
    """the class counts of the tuned table (a table change must be noticed) and the tile lists this file is parametrised over"""
    assert len(FWD_CLASSES) == 54 and len(DGRAD_CLASSES) == 50
    assert sum(1 for k in _TABLE if k.startswith("fwd|") and int(k.split("|")[1]) % 8) == 3      # the three stem rows
    assert int(_cdll().ssn_conv_pl_tiles()) == len(PLAIN_TILES)
    for c in PLAIN_TILES:
        assert tile_shape(c)[1] == _BN_OF[c]
        # which tiles have a haloed / per-image haloed variant: a small layer every variant fits
        assert bool(_cdll().ssn_conv_pl_halo_taken(5, 9, 9, 32 + c)) == (32 + c in HALO_TILES)
        assert bool(_cdll().ssn_conv_pl_halo_taken(5, 9, 9, 48 + c)) == (48 + c in HALO_PI_TILES)


class _Gpu:
    name, device, is_gpu = "gpu", "cuda:0", True

    @staticmethod
    def put(t):
        return t.to("cuda:0") if t is not None else None


@GPU
@pytest.mark.parametrize("row", FWD_CLASSES, ids=lambda r: "-".join(map(str, r)))
def test_table_forward(hip_library, row):
    cin, cout, kh, kw, s, h, tile = row
    ph, pw = _pad_of(cin, cout, kh, kw, s, h)
    ho, wo = (h + 2 * ph - kh) // s + 1, (h + 2 * pw - kw) // s + 1
    n = _batch(ho * wo, _BN_OF[plain_of(tile)], h)
    if tile >= 32:      # the table picked a haloed tile: the haloed kernel must be the one that runs
        assert (kh, kw, s, ph, pw) == (3, 3, 1, 1, 1) and _cdll().ssn_conv_pl_halo_taken(n, h, h, tile) == 1, row
    case = (n, cin, h, h, cout, kh, kw, s, ph, pw)
    x, w, scale, shift = fwd_inputs(case, gen("A", row))
    run_fwd(_Gpu, x, w, scale, shift, s, ph, pw, tile, what=case)


@GPU
@pytest.mark.parametrize("cin", [16, 40])
def test_table_forward_stem(hip_library, cin):
    """the space-to-depth stems as the executor launches them: 4x4 taps, pad 2, output cropped to the input's 112 x 112, tile 10 (40 channels: the
    Flow stem, a tail slab)"""
    assert _TABLE["fwd|3|64|7|7|2|224"] == 10 and _TABLE["fwd|10|64|7|7|2|224"] == 10
    case = (3, cin, 112, 112, 64, 4, 4, 1, 2, 2)
    x, w, scale, shift = fwd_inputs(case, gen("A stem", cin))
    run_fwd(_Gpu, x, w, scale, shift, 1, 2, 2, 10, crop=112, what=case)


@GPU
@pytest.mark.parametrize("row", DGRAD_CLASSES, ids=lambda r: "-".join(map(str, r)))
def test_table_dgrad(hip_library, row):
    cin, cout, kh, kw, s, h, tile = row
    ph, pw = _pad_of(cin, cout, kh, kw, s, h)
    # pixels of the enumerated grid: dx's, or the smallest parity class of it
    pixels = h * h if s == 1 else ((h // 2) ** 2)
    n = _batch(pixels, _BN_OF[plain_of(tile)], h)
    if tile >= 32:
        assert (kh, kw, s, ph, pw) == (3, 3, 1, 1, 1) and _cdll().ssn_conv_pl_halo_taken(n, h, h, tile) == 1, row
    case = (n, cin, h, h, cout, kh, kw, s, ph, pw)
    run_dgrad_masked(_Gpu, case, tile, gen("A dgrad", row), what=case)


# ------------------------------------------------------------------------------------------------------------ B: every tile, every edge
TAPS_B = [(9, 1, 1, 1, 0, 0), (9, 3, 3, 1, 1, 1), (9, 3, 3, 1, 0, 0), (10, 3, 3, 2, 1, 1), (9, 1, 7, 1, 0, 3), (9, 4, 4, 1, 2, 2)]      # H, kh, kw, stride, ph, pw
CHANNELS_B = (8, 16, 24, 40)       # 1 - 3 slabs on 1x1; 8, 24, 40: an 8-channel tail slab


def _cases_b(tile, taps):
    """(rows, taps, K channels): rows = BM + 40 (two m-tiles; the second: one full 32-row block + an 8-row partial one) on every tap shape,
    rows = 24 on 1x1 and 3x3"""
    bm, _ = tile_shape(tile)
    out = [(bm + 40, t, c) for t in taps for c in CHANNELS_B]
    out += [(24, t, c) for t in taps if (t[1], t[2]) in ((1, 1), (3, 3)) for c in CHANNELS_B]
    return out


def _run_b(backend, tile, taps):
    for rows, (h, kh, kw, s, ph, pw), c in _cases_b(tile, taps):
        fcase = (5, c, h, h, rows, kh, kw, s, ph, pw)        # forward: rows = Cout, K = Cin
        x, w, scale, shift = fwd_inputs(fcase, gen("B fwd", tile, fcase))
        run_fwd(backend, x, w, scale, shift, s, ph, pw, tile, what=fcase)
        dcase = (5, rows, h, h, c, kh, kw, s, ph, pw)        # dgrad: rows = Cin, K = Cout
        run_dgrad_plain_acc(backend, dcase, tile, gen("B dgrad", tile, dcase), what=dcase)


@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in PLAIN_TILES], [(3,), (6,), (7,)]), indirect=["backend"])
def test_tile_edges(backend, tile):
    """N = 5 images of 9 x 9 (405 pixels: tails of 21 / 21 / 149 pixels behind tiles of 64 / 128 / 256, every tile crosses images); the
    reversed-tap dgrad path (1x7, 4x4) with accumulate + mask runs on every tile, 6 and 10 among them"""
    taps = TAPS_B if backend.is_gpu else TAPS_B[:2]
    _run_b(backend, tile, taps)


@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in HALO_TILES + HALO_PI_TILES], [(35,)]), indirect=["backend"])
def test_haloed_tile_edges(backend, tile):
    """the haloed 3x3 kernel (tile 32 + c; 48 + c: per-image tiles, the last of an image ragged) on the same edges"""
    assert _cdll().ssn_conv_pl_halo_taken(5, 9, 9, tile) == 1, tile
    _run_b(backend, tile, TAPS_B[1:2])


# ------------------------------------------------------------------------------------------------------------ C: fused-launch features
TILES_C = [0, 4, 7, 8, 10]      # a row split of 64 inside an m-tile of 128 / 192 / 96 / 160 rows; one tile 256 pixels wide


@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in TILES_C], [(7,)]), indirect=["backend"])
def test_forward_source_slice(backend, tile):
    """x = channels [24, 64) of a tensor 40 channels wider whose other channels hold 1e4 in both planes: the kernel must stay inside the slice
    (3x3 / pad 1: the first tap of the first pixel sits in FRONT of the slice's first byte)"""
    case = (3, 40, 9, 9, 72, 3, 3, 1, 1, 1)
    x, w, scale, shift = fwd_inputs(case, gen("C1", tile))
    t = P.PlaneTensor(3, 80, 9, 9, backend.device)
    t.data.fill_(1e4)
    P.from_f32(backend.put(x), P.PSlice(t, 24, 40))
    assert rel_err(P.to_f32(P.PSlice(t, 24, 40)), x) < 2.0 ** -21
    run_fwd(backend, x, w, scale, shift, 1, 1, 1, tile, src=P.PSlice(t, 24, 40), what="source slice")
    raw = t.data.cpu().float()
    assert (raw[:, :, :3] == 1e4).all() and (raw[:, :, 8:] == 1e4).all()


@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in TILES_C], [(7,)]), indirect=["backend"])
def test_forward_without_relu(backend, tile):
    """relu = False: about half of the outputs are negative and must survive; the recorded maximum is the largest MAGNITUDE"""
    for case in [(3, 40, 9, 9, 72, 3, 3, 1, 1, 1), (5, 24, 9, 9, 136, 1, 1, 1, 0, 0)]:
        x, w, scale, shift = fwd_inputs(case, gen("C2", tile, case))
        ref = run_fwd(backend, x, w, scale, shift, 1, case[8], case[9], tile, relu=False, what=("no relu",) + case)
        neg = (ref < 0).double().mean().item()
        assert 0.3 < neg < 0.7, neg
        assert -ref.min().item() > 0.5 * ref.abs().max().item()      # (clamping at zero would cost far more than the tolerance)


@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in TILES_C], [(7,)]), indirect=["backend"])
def test_row_split_inside_a_tile(backend, tile):
    """the fused block-input launch on a 1x1 layer of 136 rows: rows >= 64 land 24 channels further up (inside the first m-tile of every tile
    here but 64 x 256), rows >= 96 take no affine / ReLU; the 24 gap channels keep their 7.0.  Reference: as
    tests/test_planes.py::test_conv_pl_raw_rows_and_row_gap"""
    g = gen("C3", tile)
    n, cin, h, cout, split, gap, raw_from = 5, 24, 9, 136, 64, 24, 96
    x = torch.randn(n, cin, h, h, generator=g)
    w = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    ctot = cout + gap
    scale = torch.rand(ctot, generator=g) + 0.5       # indexed by destination channel
    shift = torch.randn(cout, generator=g) * 0.1      # indexed by launch row
    z = F.conv2d(x.double(), w.double())
    ref = torch.zeros(n, ctot, h, h, dtype=torch.float64)
    for m in range(cout):
        d = m if m < split else m + gap
        ref[:, d] = F.relu(z[:, m] * scale[d].double() + shift[m].double()) if m < raw_from else z[:, m]
    real = [c for c in range(ctot) if not split <= c < split + gap]
    xp, wp = P.from_f32(backend.put(x)), _pack_fwd(w, backend)
    y = P.PlaneTensor(n, ctot, h, h, backend.device)
    y.data.fill_(7.0)
    for _ in range(2):
        P.conv_fwd(P.pfull(xp), wp, backend.put(scale), backend.put(shift), P.PSlice(y, 0, cout), 1, 1, 1, 0, 0, True, tile,
                   raw_from=raw_from, row_split=split, row_gap=gap)
        ok, figs = amax_close(y, ref.abs().max().item())
        assert ok, ("y.amax", tile, figs)
        y.pool.update()
    got = P.to_f32(y).cpu()
    err = rel_err(got[:, real], ref[:, real])
    print("  row split err %.3g" % err, tile, flush=True)
    assert err < 3e-6, (tile, err)
    raw = y.data.cpu().float()
    assert (raw[:, :, split // 8:(split + gap) // 8] == 7.0).all(), "wrote into the gap"


@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in TILES_C], [(7,)]), indirect=["backend"])
def test_dgrad_k_split_and_gap(backend, tile):
    """dY of a fused block-input launch: 96 rows as two slices of one planes tensor -- rows [0, 32) at channel 8, rows [32, 96) at channel
    8 + 32 + 24, stored with the first one's scale; the 24 channels between hold 1e4 in both planes -- on a 1x1 and a 3x3 / pad 1 layer (the gap rules
    the haloed kernel out: tile 32 + c must run the plain kernel and give the same), plain and accumulate + mask; then the argument check"""
    n, cin, h, cout, split, gap = 3, 72, 9, 96, 32, 24
    for (kh, ph) in ((1, 0), (3, 1)):
        case = (n, cin, h, h, cout, kh, kh, 1, ph, ph)
        g = gen("C4", tile, kh)
        w, gy, dref = dgrad_inputs(case, g)
        act, msc, m = mask_inputs(n, cin, h, h, g)
        wt, rev = pack_dgrad(w, 1, backend)
        gt = P.PlaneTensor(n, 8 + cout + gap + 8, h, h, backend.device)
        gt.data.fill_(1e4)
        P.from_f32(backend.put(gy[:, :split].contiguous()), P.PSlice(gt, 8, split))
        P.from_f32(backend.put(gy[:, split:].contiguous()), P.PSlice(gt, 8 + split + gap, cout - split), exact=False)
        gs = P.PSlice(gt, 8, cout)
        actp = P.from_f32(backend.put(act))
        dx = P.PlaneTensor(n, cin, h, h, backend.device)
        dmax = dref.abs().max().item()
        for tcfg in ([tile, 32 + tile] if kh == 3 else [tile]):
            dx.data.fill_(3.0)
            for _ in range(2):
                P.conv_dgrad(gs, wt, P.pfull(dx), kh, kh, ph, ph, tile_cfg=tcfg, k_split=split, k_gap=gap)
                ok, figs = amax_close(dx, dmax)
                assert ok, ("dx.amax", kh, tcfg, figs)
                dx.pool.update()
            err = rel_err(P.to_f32(dx), dref)
            print("  k_split dgrad err %.3g" % err, kh, tcfg, flush=True)
            assert err < 3e-6, ("k_split dgrad", kh, tcfg, err)
            ref = 2 * dref * m
            for _ in range(2):
                P.conv_dgrad(gs, wt, P.pfull(dx), kh, kh, ph, ph, tile_cfg=tcfg, k_split=split, k_gap=gap)
                P.conv_dgrad(gs, wt, P.pfull(dx), kh, kh, ph, ph, accumulate=True, tile_cfg=tcfg, mask=P.pfull(actp),
                             mask_scale=backend.put(msc), k_split=split, k_gap=gap)
                ok, figs = amax_close(dx, max(dmax, ref.abs().max().item()))
                assert ok, ("dx.amax accumulate", kh, tcfg, figs)
                dx.pool.update()
            err = rel_err(P.to_f32(dx), ref)
            print("  k_split dgrad acc + mask err %.3g" % err, kh, tcfg, flush=True)
            assert err < 4e-6, ("k_split dgrad mask", kh, tcfg, err)
        if kh == 1:
            with pytest.raises(RuntimeError):      # a split that is no multiple of 16
                P.conv_dgrad(gs, wt, P.pfull(dx), 1, 1, 0, 0, tile_cfg=tile, k_split=24, k_gap=gap)
            with pytest.raises(RuntimeError):      # a split behind the last channel
                P.conv_dgrad(gs, wt, P.pfull(dx), 1, 1, 0, 0, tile_cfg=tile, k_split=cout, k_gap=gap)
            with pytest.raises(RuntimeError):      # Cout no multiple of 16 with a gap
                P.conv_dgrad(P.PSlice(gt, 8, cout - 8), wt, P.pfull(dx), 1, 1, 0, 0, tile_cfg=tile, k_split=split, k_gap=gap)


@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in (0, 2, 3, 7, 8)], [(7,)]), indirect=["backend"])
def test_dgrad_stride2_slices_accumulate_zero_edge(backend, tile):
    """ssn_conv_pl_dgrad_s2 on the tiles production picks for it: pad 1 on 10 x 10, pad 0 on 9 x 9, pad 0 on 10 x 10 (row 9 and column 9 receive
    no gradient and must be WRITTEN as zero over the 3.0 that was there); dx = channels [8, 48) of a wider tensor, the mask a slice of another,
    wider one; masked; then plain + accumulate with the mask = twice the masked gradient"""
    n, cin, cout = 3, 40, 24
    for (h, pad) in ((10, 1), (9, 0), (10, 0)):
        case = (n, cin, h, h, cout, 3, 3, 2, pad, pad)
        g = gen("C5", tile, h, pad)
        w, gy, dref = dgrad_inputs(case, g)
        act, msc, m = mask_inputs(n, cin, h, h, g)
        wt, _ = pack_dgrad(w, 2, backend)
        gs = put_planes(backend, gy)
        at = P.PlaneTensor(n, cin + 32, h, h, backend.device).zero_()
        P.from_f32(backend.put(act), P.PSlice(at, 16, cin))
        dt = P.PlaneTensor(n, cin + 24, h, h, backend.device)
        dt.data.fill_(3.0)
        dxs, ms = P.PSlice(dt, 8, cin), P.PSlice(at, 16, cin)
        dmax = dref.abs().max().item()
        # plain: the pixels without a contributing tap are stored as zeros
        _two_pass(lambda: P.conv_dgrad_s2(gs, wt, dxs, pad, tile_cfg=tile), dt)
        got = P.to_f32(dxs).cpu()
        err = rel_err(got, dref)
        ok, figs = amax_close(dt, dmax)
        print("  s2 dgrad err %.3g amax" % err, figs, (h, pad), tile, flush=True)
        assert err < 3e-6 and ok, ("s2 dgrad", h, pad, tile, err, figs)
        if (h, pad) == (10, 0):
            assert (dref[:, :, 9] == 0).all() and (dref[:, :, :, 9] == 0).all()
            assert (got[:, :, 9] == 0).all() and (got[:, :, :, 9] == 0).all(), "last row / column must be written as zero"
        # masked
        _two_pass(lambda: P.conv_dgrad_s2(gs, wt, dxs, pad, tile_cfg=tile, mask=ms, mask_scale=backend.put(msc)), dt)
        err = rel_err(P.to_f32(dxs), dref * m)
        ok, figs = amax_close(dt, (dref * m).abs().max().item())
        print("  s2 dgrad masked err %.3g amax" % err, figs, (h, pad), tile, flush=True)
        assert err < 4e-6 and ok, ("s2 dgrad mask", h, pad, tile, err, figs)
        # a second call accumulates: (d + d) * mask
        ref = 2 * dref * m

        def twice():
            P.conv_dgrad_s2(gs, wt, dxs, pad, tile_cfg=tile)
            P.conv_dgrad_s2(gs, wt, dxs, pad, accumulate=True, tile_cfg=tile, mask=ms, mask_scale=backend.put(msc))
        _two_pass(twice, dt)
        err = rel_err(P.to_f32(dxs), ref)
        ok, figs = amax_close(dt, max(dmax, ref.abs().max().item()))
        print("  s2 dgrad acc + mask err %.3g amax" % err, figs, (h, pad), tile, flush=True)
        assert err < 4e-6 and ok, ("s2 dgrad accumulate", h, pad, tile, err, figs)
        raw = dt.data.cpu().float()
        assert (raw[:, :, :1] == 3.0).all() and (raw[:, :, 1 + cin // 8:] == 3.0).all(), "wrote outside dx's slice"


# ------------------------------------------------------------------------------------------------------------ D: the recorded maximum
@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in PLAIN_TILES], [(3,)]), indirect=["backend"])
def test_recorded_maximum_ignores_padding(backend, tile):
    """x in [0.5, 1.5], w in [-0.5 / (1.5 cin kh kw), 0], scale 1, shift 1, ReLU: every real output lies in [0.5, 1) (every output sees at
    least one tap) while a padded pixel or row that reached the maximum would record relu(shift) = 1.  Then dgrad: positive dY, negative
    weights, accumulate onto a dx of 0.25 with a mask of scale 1 -- the maximum is that of (0.25 + d) * mask, below what went in"""
    bm, _ = tile_shape(tile)
    n, c, h, rows = 5, 24, 9, bm + 40
    for (kh, ph) in ((3, 1), (1, 0)):
        g = gen("D", tile, kh)
        x = torch.rand(n, c, h, h, generator=g) + 0.5
        w = -torch.rand(rows, c, kh, kh, generator=g) * (0.5 / (1.5 * c * kh * kh))

        def in_range(ref):      # (by construction, asserted before the kernel runs)
            assert 0.5 <= ref.min().item() and ref.max().item() < 0.999
        run_fwd(backend, x, w, torch.ones(rows), torch.ones(rows), 1, ph, ph, tile, what=("amax", kh), ref_check=in_range)
        # dgrad on the same grid: rows = Cin = bm + 40, K = Cout = 24
        case = (n, rows, h, h, c, kh, kh, 1, ph, ph)
        w, gy, dref = dgrad_inputs(case, g, gy_fn=lambda s: torch.rand(s, generator=g) + 0.5,
                                   w_fn=lambda s: -torch.rand(s, generator=g) * (0.2 / (1.5 * c * kh * kh)))
        assert -0.2 <= dref.min().item() and dref.max().item() < 0
        act, msc, m = mask_inputs(n, rows, h, h, g, ones=True)
        wt, rev = pack_dgrad(w, 1, backend)
        gs, actp = put_planes(backend, gy), P.from_f32(backend.put(act))
        dx = P.from_f32(backend.put(torch.full((n, rows, h, h), 0.25)))
        assert dx.amax.cpu().item() == 0.0
        P.conv_dgrad(gs, wt, P.pfull(dx), kh, kh, ph, ph, accumulate=True, tile_cfg=tile, mask=P.pfull(actp),
                     mask_scale=backend.put(msc))
        want = (0.25 + dref) * m
        assert 0.05 <= want.abs().max().item() < 0.25
        ok, figs = amax_close(dx, want.abs().max().item())
        err = rel_err(P.to_f32(dx), want)
        print("  amax dgrad err %.3g amax" % err, figs, kh, tile, flush=True)
        assert ok, ("dx.amax", kh, tile, figs)
        assert err < 4e-6, ("dgrad onto 0.25", kh, tile, err)
