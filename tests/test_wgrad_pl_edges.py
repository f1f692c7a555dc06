"""The planes weight-gradient kernels (csrc/wgrad_pl.hip: wgrad_pl_body, wgrad_pl9_body, wgrad_stem_body behind ssn_conv_wgrad_pl and
ssn_conv_wgrad_pl_group) at every tile, kernel family and ragged edge, against autograd of F.conv2d in float64 on the CPU (the 4x4 stem:
output cropped to the input's size before the backward; db against b.grad).

  A  every wgrad / wgradg key of the autotuned table tuned_tiles_pl.json, launched with its recorded tile at a batch of 2 (rows of >= 56
     pixels) or 3 images, plus the two space-to-depth stems through the grouped launcher (GPU tier);
  B  every tile at the smallest shape that has every edge: the eleven one-tap tiles on M = 200 (ragged against every tile height, a last
     8-row block) x Cin = 40 (an 8-channel tail group, ragged against every tile width) with eight tap shapes on images H != W; the four
     nine-tap tiles on M = 72 at the row lengths where the LDS footprint changes (14 | 15, 30 | 31, 56 | 57: the one-tap kernel); the
     four chunked 1x1 tiles;
  C  ranges of the reduction: P < 16; 1, 2, 3 k-steps and an odd count; images smaller than a k-step or chunk; degenerate nine-tap
     images; several shares in one launch with a short last one (slab counts derived from the workspace size, never hard-coded);
  D  the grouped launcher: every family with one-chunk / two-k-step shares (ssn_conv_wgrad_pl_group_tuning) and with the default
     constants, the family boundaries, the stem with a wrapping X ring, row split + gap on the nine-tap / one-tap / chunked bodies, more
     problems than one launch or one table write takes, independence from the caller's order, the argument errors.

Every launch goes through run_single / run_group: dY and X are slices at channel 8 of planes tensors 8 channels wider at the back that hold
NaN wherever the slices do not (front group, back group, gap channels); the workspace is exactly the bytes the library asked for + a
guard, all NaN, and the guard must come back untouched (4096 floats rather than 64: a store one slab row too far lands inside it instead
of in the heap; a NaN with a payload of its own: such a row is computed from the NaN behind dY's slice and stores NaN); dw / db start at
9.0; rel_err(dw), rel_err(db) < 5e-6 (the tolerance of tests/test_planes.py, relative to the largest magnitude of the reference); a second
identical launch must reproduce the first bit by bit.

The GPU tier runs everything.  The CPU tier (host emulator) runs: B one-tap: 1x1 on tile 6, 3x3 / s2 / p1 on tile 8, 7x1 on tile 4, 4x4 on
tile 9, 5x5 on tile 5; B nine-tap: tile 101 at 14, tile 100 at 15, tile 103 at 31 (with the fall-back of 101 / 102), the row of 57; B
chunked: tile 203; C: everything but tile -1 at P = 16 / 20 / 33 (at P = 47 it stands in for tile 8); D: everything, the 113-problem
group included.

Wall time of this file as measured: GPU tier, one MI355X, 288 tests in 5.7 s (the slowest 1.2 s); CPU tier, host emulator, 96 tests in
173 s (the 113-problem group takes 20 s of it).
Worst error observed on the MI355X per part (dW / db; the bound is 5e-6): A 1.0e-6 / 4.8e-7, B 3.8e-7 / 2.4e-7, C 3.9e-7 / 1.9e-7,
D 4.2e-7 / 2.9e-7.
"""
import json
import os
import random

import pytest
import torch
import torch.nn.functional as F

import action_detection_amd
from action_detection_amd import planes as P

from test_planes import rel_err
from test_conv_pl_edges import _Gpu, _pad_of, gen, tiers

GPU = pytest.mark.gpu
TOL = 5e-6
GUARD = 4096                                   # floats behind the workspace: more than a row of the widest slab here (4033 floats)
DEFAULT_TUNING = (450.0, 150.0, 4, 32)         # g_group_fixed / g_group_min_units of csrc/wgrad_pl.hip
FORCED_TUNING = (1e-3, 1e-3, 1, 1)             # every share one chunk (two k-steps on the one-tap bodies)
NAN = float("nan")
NAN_BITS = 0x7FD5A5A5                          # the workspace's NaN


def _cdll():
    return action_detection_amd._lib.get_lib().cdll


def _r8(c):
    return (c + 7) // 8 * 8


class Problem:
    """One weight-gradient problem: case = (N, Cin, H, W, Cout, kh, kw, stride, ph, pw); dY and X as slices at channel 8 of planes tensors
    that hold NaN everywhere else; rows >= split of dY sit gap channels further up (stored with the scale of the first rows); the float64
    autograd reference.  crop: the output is cropped to the input's size before the backward (the space-to-depth stem)."""

    def __init__(self, backend, case, key, split=0, gap=0, crop=False):
        n, cin, h, wd, cout, kh, kw, s, ph, pw = case
        g = gen(*key)
        x = torch.randn(n, cin, h, wd, generator=g)
        w = (torch.randn(cout, cin, kh, kw, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
        b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x.double(), w, b, s, (ph, pw))
        if crop:
            y = y[:, :, :h, :wd]
        gy = torch.randn(y.shape, generator=g) * 1e-3
        y.backward(gy.double())
        self.case, self.split, self.gap = case, (split if gap else 0), gap
        self.ho, self.wo = y.shape[2], y.shape[3]
        self.dw_ref, self.db_ref = w.grad, b.grad
        self.gt = P.PlaneTensor(n, 8 + _r8(cout) + gap + 8, self.ho, self.wo, backend.device)
        self.gt.data.fill_(NAN)
        if gap:
            P.from_f32(backend.put(gy[:, :split].contiguous()), P.PSlice(self.gt, 8, split))
            P.from_f32(backend.put(gy[:, split:].contiguous()), P.PSlice(self.gt, 8 + split + gap, cout - split), exact=False)
        else:
            P.from_f32(backend.put(gy), P.PSlice(self.gt, 8, cout))
        self.xt = P.PlaneTensor(n, 8 + _r8(cin) + 8, h, wd, backend.device)
        self.xt.data.fill_(NAN)
        P.from_f32(backend.put(x), P.PSlice(self.xt, 8, cin))
        self.g, self.x = P.PSlice(self.gt, 8, cout), P.PSlice(self.xt, 8, cin)

    def dests(self, backend):
        n, cin, h, wd, cout, kh, kw = self.case[:7]
        return backend.put(torch.full((cout, cin, kh, kw), 9.0)), backend.put(torch.full((cout,), 9.0))

    def job(self, backend, hint=-1):
        dw, db = self.dests(backend)
        kh, kw, s, ph, pw = self.case[5:]
        return P.WgradJob(self.g, self.x, dw, db, kh, kw, s, ph, pw, g_row_split=self.split, g_row_gap=self.gap, hint=hint)

    def slabs(self, tile):
        """partial slabs a single launch with this tile asks workspace for"""
        n, cin, h, wd, cout, kh, kw = self.case[:7]
        nbytes = P.wgrad_workspace_bytes(n, cin, cout, self.ho, self.wo, kh, kw, tile)
        assert nbytes % (4 * cout * (cin * kh * kw + 1)) == 0 or tile < 0, (self.case, tile, nbytes)
        return nbytes // (4 * cout * (cin * kh * kw + 1))

    def check(self, dw, db, part, what):
        edw, edb = rel_err(dw, self.dw_ref), rel_err(db, self.db_ref)
        print("  [%s] dW err %.3g db err %.3g" % (part, edw, edb), self.case, what, flush=True)
        assert edw < TOL, ("dW", part, self.case, what, edw)
        assert edb < TOL, ("db", part, self.case, what, edb)


def _guarded(backend, nbytes):
    """a NaN workspace of exactly nbytes + the guard: (the view to pass, the guard).  The NaN has a payload no arithmetic produces, so a
    store into the guard is seen even when it stores NaN (a row behind the slice)"""
    assert nbytes % 4 == 0
    ws = backend.put(torch.full((nbytes // 4 + GUARD,), NAN_BITS, dtype=torch.int32).view(torch.float32))
    assert bool(torch.isnan(ws).all())
    return ws[:nbytes // 4], ws[nbytes // 4:]


def _intact(guard):
    return bool((guard.view(torch.int32) == NAN_BITS).all())


def run_single(backend, prob, tile, part):
    """ssn_conv_wgrad_pl with this tile, twice"""
    n, cin, h, wd, cout, kh, kw, s, ph, pw = prob.case
    nbytes = P.wgrad_workspace_bytes(n, cin, cout, prob.ho, prob.wo, kh, kw, tile)
    out = []
    for _ in range(2):
        ws, guard = _guarded(backend, nbytes)
        dw, db = prob.dests(backend)
        P.conv_wgrad(prob.g, prob.x, dw, db, kh, kw, s, ph, pw, ws, tile, g_row_split=prob.split, g_row_gap=prob.gap)
        assert _intact(guard), ("wrote behind its workspace", prob.case, tile)
        out.append((dw.cpu(), db.cpu()))
    prob.check(out[0][0], out[0][1], part, ("tile", tile))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), ("not reproducible", prob.case, tile)
    return out[0]


def run_group(backend, probs, part, hints=None, min_splits=None):
    """ssn_conv_wgrad_pl_group on these problems as ONE call, twice -> (plan, [(dw, db)]).  min_splits: {problem index: fewest splits the
    plan must give it}"""
    hints = [-1] * len(probs) if hints is None else hints
    out, plan = [], None
    for _ in range(2):
        jobs = [p.job(backend, hint) for p, hint in zip(probs, hints)]
        ws_bytes, tb_bytes, plan = P.wgrad_group_plan(jobs)
        for i, least in (min_splits or {}).items():
            assert plan[i][2] >= least, ("the plan does not split problem", i, probs[i].case, plan[i])
        ws, guard = _guarded(backend, ws_bytes)
        tb = backend.put(torch.zeros(tb_bytes, dtype=torch.uint8))
        P.conv_wgrad_group(jobs, ws, tb)
        assert _intact(guard), ("wrote behind its workspace", plan)
        out.append([(j.dw.cpu(), j.db.cpu()) for j in jobs])
    for i, (p, (dw, db)) in enumerate(zip(probs, out[0])):
        p.check(dw, db, part, ("group", i, "hint", hints[i], "plan", plan[i]))
        assert torch.equal(dw, out[1][i][0]) and torch.equal(db, out[1][i][1]), ("not reproducible", i, p.case, plan[i])
    return plan, out[0]


def plan_of(prob, backend, hint=-1):
    """(family, variant, splits, units per split) the grouped planner gives this problem alone"""
    return P.wgrad_group_plan([prob.job(backend, hint)])[2][0]


@pytest.fixture
def group_tuning(backend):
    """setter of the grouped launcher's planner constants (ssn_conv_wgrad_pl_group_tuning; values <= 0 keep the current one); the
    defaults of the source come back whatever happens"""
    cd = _cdll()
    try:
        yield cd.ssn_conv_wgrad_pl_group_tuning
    finally:
        cd.ssn_conv_wgrad_pl_group_tuning(*DEFAULT_TUNING)


# ------------------------------------------------------------------------------------------------------------ A: the tuned table
with open(os.path.join(os.path.dirname(P.__file__), "tuned_tiles_pl.json")) as _f:
    _TILES = json.load(_f)["tiles"]
WGRAD_KEYS = sorted(k for k in _TILES if k.split("|")[0] in ("wgrad", "wgradg"))
# the 7x7 / 2 rows of the two stems run in their space-to-depth form (test_table_stem); every other row as its key describes it
TABLE_ROWS = [k for k in WGRAD_KEYS if tuple(k.split("|")[3:6]) != ("7", "7", "2")]


def test_table_rows():
    """the rows this file is parametrised over (a table change must be noticed): 86 keys of single launches, none of the grouped launcher;
    the two rows left to test_table_stem"""
    assert len(WGRAD_KEYS) == 86 and len(TABLE_ROWS) == 84
    assert sorted(set(WGRAD_KEYS) - set(TABLE_ROWS)) == ["wgrad|10|64|7|7|2|224", "wgrad|3|64|7|7|2|224"]
    assert {int(_TILES[k]) for k in WGRAD_KEYS} <= set(range(11)) | {100, 101, 102, 103} | {200, 201, 202, 203}


@GPU
@pytest.mark.parametrize("key", TABLE_ROWS, ids=lambda k: k.replace("|", "-"))
def test_table_wgrad(hip_library, key):
    kind = key.split("|")[0]
    cin, cout, kh, kw, s, h = map(int, key.split("|")[1:])
    tile = int(_TILES[key])
    ph, pw = _pad_of(cin, cout, kh, kw, s, h)
    prob = Problem(_Gpu, (2 if h >= 56 else 3, cin, h, h, cout, kh, kw, s, ph, pw), ("A", key))
    if kind == "wgrad":
        run_single(_Gpu, prob, tile, "A")
    else:
        run_group(_Gpu, [prob], "A", hints=[tile])


@GPU
@pytest.mark.parametrize("cin", [12, 40])
def test_table_stem(hip_library, cin):
    """the space-to-depth stems as the executor launches them: 4x4 taps, pad 2, 112 x 112 outputs, 12 (RGB) / 40 (Flow) real channels,
    through the grouped launcher's stem family"""
    prob = Problem(_Gpu, (2, cin, 112, 112, 64, 4, 4, 1, 2, 2), ("A stem", cin), crop=True)
    plan, _ = run_group(_Gpu, [prob], "A")
    assert plan[0][0] == 4, plan


# ------------------------------------------------------------------------------------------------------------ B: every tile, every edge
TAPS_B = {      # H, W, kh, kw, stride, ph, pw, cropped
    "1x1": (5, 7, 1, 1, 1, 0, 0, False), "3x3s2p1": (9, 6, 3, 3, 2, 1, 1, False), "3x3s2p0": (7, 9, 3, 3, 2, 0, 0, False),
    "3x3p0": (6, 5, 3, 3, 1, 0, 0, False), "5x5p2": (5, 4, 5, 5, 1, 2, 2, False), "1x7p03": (3, 8, 1, 7, 1, 0, 3, False),
    "7x1p30": (8, 3, 7, 1, 1, 3, 0, False),
    "4x4p2": (5, 6, 4, 4, 1, 2, 2, True),      # the stem's taps; a single launch never takes the stem body (the grouped launcher's only)
}
ONE_TAP_TILES = list(range(11))
EMU_B1 = [(6, "1x1"), (8, "3x3s2p1"), (4, "7x1p30"), (9, "4x4p2"), (5, "5x5p2")]


def test_tile_lists(backend):
    assert int(_cdll().ssn_conv_wgrad_pl_tiles()) == len(ONE_TAP_TILES)


@pytest.mark.parametrize("backend,tile,taps", tiers([(t, k) for t in ONE_TAP_TILES for k in TAPS_B], EMU_B1), indirect=["backend"])
def test_one_tap_tile_edges(backend, tile, taps):
    """M = 200 (m-tiles of 32 / 64 / 96 / 128 / 192 / 256 rows all end ragged, the last 32-row block holds 8 rows) x Cin = 40 (one full
    32-channel fragment + an 8-channel tail group whatever the tile width), N = 2 images with H != W"""
    h, wd, kh, kw, s, ph, pw, crop = TAPS_B[taps]
    prob = Problem(backend, (2, 40, h, wd, 200, kh, kw, s, ph, pw), ("B1", taps), crop=crop)
    run_single(backend, prob, tile, "B")


NINE_CASES = [(t, w) for w in (14, 15, 30, 31, 56) for t in (100, 101, 102, 103)]
EMU_B9 = [(101, 14), (100, 15), (103, 31)]


def _nine_problem(backend, wd):
    return Problem(backend, (2, 40, 2 + wd % 2, wd, 72, 3, 3, 1, 1, 1), ("B9", wd))


@pytest.mark.parametrize("backend,tile,wd", tiers(NINE_CASES, EMU_B9), indirect=["backend"])
def test_nine_tap_tile_edges(backend, tile, wd):
    """M = 72 (a second m-tile of 8 rows behind 64; one ragged tile of 128) x Cin = 40 on rows of 14 | 15 (XP = 6 | 8), 30 | 31 (XP = 8 | 12)
    and 56 pixels (the widest the nine-tap kernel takes), H = 2 / 3.  XP = 12 has the 64 x 64 tiles only: 101 and 102 run as 100, and
    ask for 100's slabs; 103 (two wave groups) for twice as many"""
    prob = _nine_problem(backend, wd)
    if wd > 30:
        counts = [prob.slabs(t) for t in (100, 101, 102, 103)]
        assert counts[1] == counts[0] and counts[2] == counts[0] and counts[3] == 2 * counts[0], counts
    run_single(backend, prob, tile, "B")


@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_row_of_57_takes_the_one_tap_kernel(backend):
    """rows of 57 pixels do not fit the nine-tap kernel's LDS: tile -1 runs the one-tap kernel (the grouped planner's family 3), a forced
    nine-tap tile is an error"""
    prob = _nine_problem(backend, 57)
    assert plan_of(_nine_problem(backend, 56), backend)[0] == 2 and plan_of(prob, backend)[0] == 3
    run_single(backend, prob, -1, "B")
    dw, db = prob.dests(backend)
    ws = backend.put(torch.full((1 << 20,), NAN))
    with pytest.raises(RuntimeError):
        P.conv_wgrad(prob.g, prob.x, dw, db, 3, 3, 1, 1, 1, ws, 100)


def test_nine_tap_fallback_plans_the_tile_it_runs(backend):
    """rows of > 30 pixels: tiles 101 / 102 run as tile 100, so the workspace they ask for must be tile 100's -- at a size where the
    128-row and the 64-row tiles split the reduction differently, too (host-side planning only)"""
    for (n, cin, cout, hw) in [(32, 40, 72, 56), (16, 64, 192, 56), (8, 40, 72, 31), (64, 96, 128, 35)]:
        want = P.wgrad_workspace_bytes(n, cin, cout, hw, hw, 3, 3, 100)
        for tile in (101, 102):
            assert P.wgrad_workspace_bytes(n, cin, cout, hw, hw, 3, 3, tile) == want, (n, cin, cout, hw, tile)


@pytest.mark.parametrize("backend,tile", tiers([(t,) for t in (200, 201, 202, 203)], [(203,)]), indirect=["backend"])
def test_chunked_tile_edges(backend, tile):
    """the chunked 1x1 kernel: M = 200 x Cin = 40, N = 2 images of 3 x 5 (30 slots: less than one chunk, an image boundary inside it)"""
    run_single(backend, Problem(backend, (2, 40, 3, 5, 200, 1, 1, 1, 0, 0), ("B1x1",)), tile, "B")


# ------------------------------------------------------------------------------------------------------------ C: ranges of the reduction
def _c_case(n, cin, h, wd, cout, k=1, pad=0):
    return (n, cin, h, wd, cout, k, k, 1, pad, pad)


@pytest.mark.parametrize("backend,tile", tiers([(-1,), (0,), (200,)], [(-1,), (0,), (200,)]), indirect=["backend"])
def test_fewer_pixels_than_a_k_step(backend, tile):
    """P = 4: one k-step with 12 empty slots, a chunk with 60"""
    run_single(backend, Problem(backend, _c_case(1, 8, 2, 2, 16), ("C P<16",)), tile, "C")


K_STEP_SHAPES = {16: (1, 4, 4), 20: (1, 4, 5), 33: (3, 1, 11), 47: (1, 1, 47)}      # P -> N, H, W


@pytest.mark.parametrize("backend,pixels,tile", tiers([(p, t) for p in K_STEP_SHAPES for t in (-1, 0, 8, 200)],
                                                      [(p, t) for p in K_STEP_SHAPES for t in (0, 8, 200) if (p, t) != (47, 8)] + [(47, -1)]),
                         indirect=["backend"])
def test_fewer_k_steps_than_ring_slots(backend, pixels, tile):
    """1x1 with P = 16 / 20 / 33 / 47: 1, 2, 3 and 3 k-steps -- fewer than, or as many as, the ring has slots; odd counts run a zero-filled
    surplus half-trip; P = 20, 33, 47 end inside a k-step"""
    n, h, wd = K_STEP_SHAPES[pixels]
    assert n * h * wd == pixels
    run_single(backend, Problem(backend, _c_case(n, 24, h, wd, 40), ("C ksteps", pixels)), tile, "C")


@pytest.mark.parametrize("backend,k,tile", tiers([(1, -1), (1, 0), (1, 200), (3, -1), (3, 0), (3, 100)],
                                                 [(1, -1), (1, 0), (1, 200), (3, -1), (3, 0), (3, 100)]), indirect=["backend"])
def test_images_smaller_than_a_k_step(backend, k, tile):
    """N = 5 images of 3 x 3: a 16-slot k-step and a 64-slot chunk span several images (nine taps: 16 padded slots per image)"""
    run_single(backend, Problem(backend, _c_case(5, 8, 3, 3, 16, k, k // 2), ("C small images", k)), tile, "C")


@pytest.mark.parametrize("backend,h,wd,tile", tiers([(h, w, t) for (h, w) in ((1, 1), (1, 9), (9, 1)) for t in (100, 0)],
                                                    [(h, w, t) for (h, w) in ((1, 1), (1, 9), (9, 1)) for t in (100, 0)]), indirect=["backend"])
def test_degenerate_nine_tap_images(backend, h, wd, tile):
    """3x3 / pad 1 on images of 1 x 1, 1 x 9 and 9 x 1: most taps of most pixels fall off the image"""
    run_single(backend, Problem(backend, _c_case(3, 8, h, wd, 16, 3, 1), ("C degenerate", h, wd)), tile, "C")


SHARE_CASES = [(19, 19, 3, 0), (19, 19, 3, 100), (19, 19, 3, 103), (19, 19, 1, 0), (19, 19, 1, 200), (13, 29, 3, 100), (13, 29, 3, 103)]


@pytest.mark.parametrize("backend,h,wd,k,tile", tiers(SHARE_CASES, SHARE_CASES), indirect=["backend"])
def test_several_shares_in_one_launch(backend, h, wd, k, tile):
    """a reduction range the planner splits: the launch writes several slabs, the last share is shorter than the others or ends inside
    its last k-step / chunk.  The slab count is the library's own (workspace bytes / slab bytes)"""
    prob = Problem(backend, _c_case(3, 8, h, wd, 16, k, k // 2), ("C shares", h, wd, k))
    slabs = prob.slabs(tile)
    print("  slabs", slabs, (h, wd, k, tile), flush=True)
    assert slabs >= 2, (h, wd, k, tile, slabs)
    run_single(backend, prob, tile, "C")


# ------------------------------------------------------------------------------------------------------------ D: the grouped launcher
FAMILIES = {      # name: (case, hint, cropped, family, variant)
    "nine-xp6": ((2, 40, 3, 14, 72, 3, 3, 1, 1, 1), -1, False, 0, 0),
    "nine-xp8": ((2, 40, 3, 30, 72, 3, 3, 1, 1, 1), -1, False, 1, 0),
    "nine-xp12": ((2, 40, 3, 56, 72, 3, 3, 1, 1, 1), -1, False, 2, 0),
    "one-tap-128x128": ((3, 40, 7, 8, 200, 3, 3, 1, 0, 0), 3, False, 3, 0),
    "one-tap-96x128": ((3, 40, 7, 8, 200, 3, 3, 1, 0, 0), 8, False, 3, 1),
    "one-tap-64x64": ((3, 40, 7, 8, 200, 3, 3, 1, 0, 0), 0, False, 3, 2),
    "chunked": ((3, 40, 6, 7, 200, 1, 1, 1, 0, 0), 200, False, 3, 3),
    "stem": ((2, 12, 6, 9, 72, 4, 4, 1, 2, 2), -1, True, 4, 0),
    "stem-by-hint": ((2, 40, 6, 9, 72, 4, 4, 1, 2, 2), 300, True, 4, 0),
    "row7": ((2, 40, 3, 10, 72, 1, 7, 1, 0, 3), -1, False, 5, 0),
    "col7": ((2, 40, 10, 5, 72, 7, 1, 1, 3, 0), -1, False, 6, 0),
}
_FAMILY_CASES = [(name, forced) for name in FAMILIES for forced in (1, 0)]


@pytest.mark.parametrize("backend,name,forced", tiers(_FAMILY_CASES, _FAMILY_CASES), indirect=["backend"])
def test_group_family(backend, name, forced, request):
    """every kernel family of the grouped launcher on a problem with ragged tiles, once with shares of one chunk (two k-steps on the
    one-tap bodies: as many short shares per tile as the range has) and once under the default constants"""
    case, hint, crop, family, variant = FAMILIES[name]
    if forced:
        request.getfixturevalue("group_tuning")(*FORCED_TUNING)
    prob = Problem(backend, case, ("D family", name), crop=crop)
    plan, _ = run_group(backend, [prob], "D", hints=[hint], min_splits={0: 2} if forced else None)
    assert plan[0][:2] == (family, variant), plan
    if forced:
        assert plan[0][3] == (2 if family == 3 and variant < 3 else 1), plan


def _boundary_problem(backend, kind, wd):
    if kind == "col7":
        return Problem(backend, (1, 8, 4, wd, 16, 7, 1, 1, 3, 0), ("D boundary", kind, wd))
    if kind == "stem":      # (114: real rows in three chunks or more -- only rows this wide look back over 2 (W + 2) + 2 = 234 of the ring's 256 slots)
        n, h = (2, 3) if wd <= 114 else (1, 2)
        return Problem(backend, (n, 12, h, wd, 16, 4, 4, 1, 2, 2), ("D boundary", kind, wd), crop=True)
    return Problem(backend, (1, 8, 2, wd, 16, 3, 3, 1, 1, 1), ("D boundary", kind, wd))


BOUNDARIES = [("col7", 21, 6), ("col7", 22, 3), ("stem", 114, 4), ("stem", 115, 3), ("nine", 14, 0), ("nine", 15, 1), ("nine", 30, 1),
              ("nine", 31, 2), ("nine", 56, 2), ("nine", 57, 3)]


@pytest.mark.parametrize("backend,kind,wd,family", tiers(BOUNDARIES, BOUNDARIES), indirect=["backend"])
def test_family_boundaries(backend, kind, wd, family):
    """the widest row every multi-tap family takes, and the next one: read from the plan, then launched"""
    prob = _boundary_problem(backend, kind, wd)
    plan, _ = run_group(backend, [prob], "D")
    assert plan[0][0] == family, (kind, wd, plan)


STEMS = [(2, 12, 6, 9, 72, 0), (1, 40, 5, 7, 72, 0), (3, 12, 20, 20, 64, 0), (3, 12, 20, 20, 64, 1)]


@pytest.mark.parametrize("backend,n,cin,h,wd,cout,one_share", tiers(STEMS, STEMS), indirect=["backend"])
def test_stem(backend, n, cin, h, wd, cout, one_share, request):
    """the stem body: 12 / 40 real channels (one / three 16-channel sub-blocks, the last with 8 channels behind the slice), 72 rows, H != W,
    rows that are no multiple of 4; and 3 images of 20 x 20 = 1452 padded slots.  Under the default constants this problem, alone in its
    group, makes two shares of 768 slots (the second crosses slot 1024 of the X ring); with a fixed cost per share that outweighs any
    split (one_share) it is ONE share of twelve chunks: more slots than the ring has"""
    if one_share:
        request.getfixturevalue("group_tuning")(1e6, 0.0, 0, 0)
    prob = Problem(backend, (n, cin, h, wd, cout, 4, 4, 1, 2, 2), ("D stem", n, cin, h, wd), crop=True)
    plan, _ = run_group(backend, [prob], "D")
    assert plan[0][0] == 4, plan
    if (n, h, wd) == (3, 20, 20):
        slots = n * (h + 2) * (wd + 2)
        assert slots > 1024 and plan[0][2] * plan[0][3] * 128 >= slots, plan
        assert (plan[0][2] == 1 and plan[0][3] * 128 > 1024) if one_share else plan[0][3] * 128 < 1024, plan


ROW_GAP = (2, 40, 4, 6, 72, 3, 3, 1, 1, 1)
ROW_GAP_1X1 = (2, 40, 3, 5, 200, 1, 1, 1, 0, 0)
_GAP_CASES = [("nine", "group", -1), ("nine", "group", 0), ("nine", "group", 8), ("nine", "single", 100), ("nine", "single", 101),
              ("nine", "single", 0), ("nine", "single", 8), ("1x1", "single", 201), ("1x1", "single", 200), ("1x1", "group", 200)]


@pytest.mark.parametrize("backend,shape,how,tile", tiers(_GAP_CASES, _GAP_CASES), indirect=["backend"])
def test_row_split_and_gap(backend, shape, how, tile):
    """a fused block-input problem: rows >= 32 of dY sit 16 channels further up (NaN between them) -- on the nine-tap body through the
    group, on the one-tap bodies by hint, as single launches; rows >= 64 sit 8 channels further up on the chunked body (inside the m-tile
    of tile 201)"""
    if shape == "nine":
        prob = Problem(backend, ROW_GAP, ("D gap",), split=32, gap=16)
    else:
        prob = Problem(backend, ROW_GAP_1X1, ("D gap 1x1",), split=64, gap=8)
    if how == "single":
        run_single(backend, prob, tile, "D")
    else:
        plan, _ = run_group(backend, [prob], "D", hints=[tile])
        assert plan[0][0] == (0 if tile == -1 else 3), plan


def _many_problems(backend, n_small, n_nine):
    probs = []
    for i in range(n_small):
        cout = 8 + 8 * (i % 5)
        case = (1, 8, 2, 2, cout, 1, 1, 1, 0, 0) if i % 2 == 0 else (1, 8, 5, 5, cout, 3, 3, 2, 1, 1)
        probs.append(Problem(backend, case, ("D many", i)))
    for i in range(n_nine):
        probs.append(Problem(backend, (1, 8, 2, 2 + i, 16 + 8 * (i % 3), 3, 3, 1, 1, 1), ("D many nine", i)))
    return probs


@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_more_problems_than_a_launch_takes(backend):
    """100 problems of the one-tap / chunked family (96 per launch: a second launch of four problems; nine table writes of 12 entries) and
    13 nine-tap problems (a second table write of one entry) in ONE call; every problem has its own data and is checked"""
    probs = _many_problems(backend, 100, 13)
    plan, _ = run_group(backend, probs, "D")
    assert [f for f, _, _, _ in plan] == [3] * 100 + [0] * 13
    assert {v for f, v, _, _ in plan if f == 3} == {2, 3}      # (the 1x1 problems take the chunked body, the stride-2 ones 64 x 64 one-tap)


@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_callers_order_does_not_matter(backend):
    """the same problems in another order: other workspace regions, other table positions, the same bits"""
    probs = _many_problems(backend, 14, 3) + [Problem(backend, FAMILIES["stem"][0], ("D order stem",), crop=True)]
    _, first = run_group(backend, probs, "D")
    order = list(range(len(probs)))
    random.Random(7).shuffle(order)
    assert order != sorted(order)
    _, second = run_group(backend, [probs[i] for i in order], "D")
    for pos, i in enumerate(order):
        assert torch.equal(first[i][0], second[pos][0]) and torch.equal(first[i][1], second[pos][1]), (i, pos, probs[i].case)


@pytest.mark.parametrize("backend", tiers([()], [()]), indirect=["backend"])
def test_argument_errors(backend):
    s2 = Problem(backend, (1, 8, 5, 5, 16, 3, 3, 2, 1, 1), ("D err s2",))
    nine = Problem(backend, (1, 8, 4, 5, 16, 3, 3, 1, 1, 1), ("D err nine",))
    one = Problem(backend, (1, 8, 4, 5, 16, 1, 1, 1, 0, 0), ("D err 1x1",))
    for prob, hint in ((s2, 100), (nine, 300), (one, 201)):
        with pytest.raises(RuntimeError):
            P.wgrad_group_plan([prob.job(backend, hint)])
        with pytest.raises(RuntimeError):
            P.conv_wgrad_group([prob.job(backend, hint)])
    # a workspace one byte short: the group, and every kind of single launch
    job = nine.job(backend)
    ws_bytes, tb_bytes, _ = P.wgrad_group_plan([job])
    tb = backend.put(torch.zeros(tb_bytes, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        P.conv_wgrad_group([job], backend.put(torch.zeros(ws_bytes - 1, dtype=torch.uint8)), tb)
    for prob, tile in ((nine, 100), (nine, 0), (one, 200)):
        n, cin, h, wd, cout, kh, kw, s, ph, pw = prob.case
        nbytes = P.wgrad_workspace_bytes(n, cin, cout, prob.ho, prob.wo, kh, kw, tile)
        dw, db = prob.dests(backend)
        with pytest.raises(RuntimeError):
            P.conv_wgrad(prob.g, prob.x, dw, db, kh, kw, s, ph, pw, backend.put(torch.zeros(nbytes - 1, dtype=torch.uint8)), tile)
        assert bool((dw == 9.0).all()) and bool((db == 9.0).all())
