"""TV-L1 optical flow (csrc/flow.hip, optical_flow.py, tools/extract_flow.py) against the float64 referee tests/flow_referee.py,
through the host emulator and on the GPU.

Tolerances.  A float64 referee cannot tell a kernel bug from fp32 rounding without a yardstick; the yardstick is the referee
itself run in float32 against float64 on the same input (the kernels differ from numpy float32 only by summation order -- they
are compiled without contraction).  Every bound below is 4 x that value, written as ``4 * yardstick`` with the yardstick as
measured by ``python tests/test_optical_flow.py``, which prints all of them (no device needed).  The known-motion and iterate
cases that depend on the tile shape were measured at the 44 x 44 interior the kernel exports; a different tile moves those
inputs and wants a new measurement.
"""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_referee as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 44                       # the interior the yardsticks below were measured with (asserted against the library)

# ------------------------------------------------------------------------------------------------------------------ bounds
# resize 33x47 -> 26x38 and 26x38 -> 33x47 (values up to 255, multipliers 0.8 / 1.25), max abs difference
# (uniform noise is the harshest input: the fp32 source coordinate is off by a few 1e-6 px, times up to 255 per px)
RESIZE_BOUND = {"down": 4 * 5.18e-4, "up": 4 * 3.67e-4}       # yardsticks: float32 referee vs float64
# warp constants at 33x47 with a random flow of +-3 px: relative to the largest magnitude of each field
WARP_BOUND = {"gx": 4 * 1.26e-6, "gy": 4 * 6.32e-7, "grad": 4 * 6.55e-7, "rho_c": 4 * 4.74e-7}
# one chunk (10 iterations) from a random state, max abs difference over the six fields
ITERATE_BOUND = {(2 * TILE + 3, 2 * TILE + 5): 4 * 2.24e-7, (19, 24): 4 * 1.71e-7}
# known motion: `yard` = the yardstick over the whole image, max abs flow difference in px (the bound is 4 x); `ref_err` = the float64
# referee's own error against the true shift inside a 6 px margin.  The float32 and float64 referees run the same schedule in all
# four cases (740 / 840 / 690 / 900 iterations) and quantise to the same images.
MOTION_CASES = {
    "shift_2_-1_48x64": dict(size=(48, 64), shift=(2.0, -1.0), seed=11, yard=1.73e-3, ref_err=0.0584),
    "shift_-1.5_0.75_40x56": dict(size=(40, 56), shift=(-1.5, 0.75), seed=12, yard=1.54e-4, ref_err=0.0603),
    "shift_0.5_0.5_33x47": dict(size=(33, 47), shift=(0.5, 0.5), seed=13, yard=3.47e-5, ref_err=0.0763),
    "shift_1_1.5_tiles": dict(size=(2 * TILE + 3, 2 * TILE + 5), shift=(1.0, 1.5), seed=14, yard=9.76e-5, ref_err=0.0868),
}
# motion boundary: `yard` = yardstick >= 8 px from the seam and >= 6 px from the border; `share` = the float32 referee's share of
# pixels off by more than 0.01 px over the whole image (fp32 and float64 legitimately part at the seam: 0.56 px there with the
# defaults, 960 iterations; the fixed 750 iterations stay within 0.0058 px everywhere, so no pixel may be off there)
BOUNDARY = {"default": dict(params={}, yard=3.99e-3, share=0.0218),
            "fixed": dict(params=dict(epsilon=0.0, iterations=30), yard=3.43e-5, share=0.0)}


# ------------------------------------------------------------------------------------------------------------------ inputs
def iterate_inputs(h, w, seed):
    rs = np.random.RandomState(seed)
    state = np.stack([rs.normal(0, 1, (h, w)), rs.normal(0, 1, (h, w))] + [rs.uniform(-0.5, 0.5, (h, w)) for _ in range(4)])
    gx, gy = rs.normal(0, 5, (h, w)), rs.normal(0, 5, (h, w))
    flat = rs.uniform(0, 1, (h, w)) < 0.1          # cells without gradient: the d = 0 branch
    gx[flat], gy[flat] = 0.0, 0.0
    gx, gy = gx.astype(np.float32), gy.astype(np.float32)
    cst = np.stack([gx, gy, gx * gx + gy * gy, rs.normal(0, 3, (h, w)).astype(np.float32)])
    return state.astype(np.float32), cst.astype(np.float32)


def boundary_pair():
    """48x64, left half moves (2, 0), right half (-1, 1.5), Gaussian noise sigma 2 on both frames."""
    h, w = 48, 64
    tex = R.texture(h, w, 21)
    left = np.arange(w)[None, :] < w // 2
    dx = np.where(left, 2.0, -1.0) * np.ones((h, 1))
    dy = np.where(left, 0.0, 1.5) * np.ones((h, 1))
    rs = np.random.RandomState(22)
    prev = R.sample_texture(tex, h, w, 0.0, 0.0) + rs.normal(0, 2, (h, w))
    nxt = R.sample_texture(tex, h, w, -dx, -dy) + rs.normal(0, 2, (h, w))
    return np.clip(np.rint(prev), 0, 255).astype(np.uint8), np.clip(np.rint(nxt), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def motion_reference(name):
    c = MOTION_CASES[name]
    prev, nxt = R.shifted_pair(c["size"][0], c["size"][1], c["shift"], c["seed"])
    f64, it64 = R.tvl1(prev, nxt)
    return prev, nxt, f64, it64


@functools.lru_cache(maxsize=None)
def boundary_reference(variant):
    prev, nxt = boundary_pair()
    f64, it64 = R.tvl1(prev, nxt, **BOUNDARY[variant]["params"])
    return prev, nxt, f64, it64


def seam_masks(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    inner = (xs >= 6) & (xs < w - 6) & (ys >= 6) & (ys < h - 6)
    return inner & (np.abs(xs - (w // 2 - 0.5)) >= 8)


def margin(a, m=6):
    return a[..., m:-m, m:-m]


# ------------------------------------------------------------------------------------------------------------------ helpers
def of():
    from action_detection_amd import optical_flow
    return optical_flow


def kernels():
    from action_detection_amd import kernels as K
    return K


def run_tvl1(backend, pairs, **params):
    """pairs: list of (prev, nxt) uint8 arrays of one size -> (flow [B, 2, H, W], iterations [levels, warps, B]) as numpy."""
    prev = backend.put(torch.from_numpy(np.stack([p for p, _ in pairs])))
    nxt = backend.put(torch.from_numpy(np.stack([n for _, n in pairs])))
    res = of().TVL1(**params)(prev, nxt)
    return res.flow.cpu().numpy(), res.iterations.cpu().numpy()


def run_iterate(backend, state, cst, splits, part=False):
    """The launches `splits` (iterations each) on one pair from `state`; -> the six fields after the last one."""
    K = kernels()
    h, w = state.shape[1:]
    st = backend.put(torch.zeros((2, 1, 6, h, w)))
    st[0, 0] = backend.put(torch.from_numpy(state))
    c = backend.put(torch.from_numpy(cst[None]).contiguous())
    ctl = backend.put(torch.zeros((2, 1, 4), dtype=torch.int32))
    iters = backend.put(torch.zeros(1, dtype=torch.int32))
    th, tw, _ = K.tvl1_tile_shape()
    parts = backend.put(torch.zeros((1, -(-h // th) * -(-w // tw))))
    p = R.DEFAULTS
    for k, n in enumerate(splits):
        K.tvl1_iterate(st, c, n, p["lambda_"] * p["theta"], p["theta"], p["tau"] / p["theta"], 0.0, ctl[k & 1], ctl[(k + 1) & 1],
                       None, parts if k == len(splits) - 1 else None, iters)
    assert int(iters[0]) == sum(splits) and ctl[len(splits) & 1, 0].tolist() == [0, len(splits), sum(splits), 0]
    return st[len(splits) & 1, 0].cpu().numpy(), float(parts.double().sum())


# ------------------------------------------------------------------------------------------------------------------ 1. exact pieces
def test_gray_is_exact(backend):
    rs = np.random.RandomState(0)
    rgb = rs.randint(0, 256, (3, 37, 53, 3)).astype(np.uint8)
    rgb[0, 0, :4] = [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 0, 255]]
    got = of().rgb_to_gray(backend.put(torch.from_numpy(rgb)))
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(R.gray(rgb)))


def test_quantiser_is_exact(backend):
    rs = np.random.RandomState(1)
    # bound 2: both saturated ends; the kernel's own float input goes to the numpy restatement
    v = rs.normal(0, 2.5, (2, 2, 31, 45)).astype(np.float32)
    v[0, 0, 0, :4] = [2.0, -2.0, np.nextafter(np.float32(2), np.float32(3)), np.nextafter(np.float32(-2), np.float32(-3))]
    got = of().flow_to_uint8(backend.put(torch.from_numpy(v)), bound=2)
    want = R.quantize(v, 2)
    assert want.min() == 0 and want.max() == 255 and (v > 2).any() and (v < -2).any()
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    # bound 127.5 with integer flows: 255 (v + 127.5) / 255 = v + 127.5, every value an exact .5 tie -> half to even
    ints = np.arange(-128, 129, dtype=np.float32).reshape(1, 1, 1, -1)
    got = of().flow_to_uint8(backend.put(torch.from_numpy(ints)), bound=127.5).cpu().numpy().ravel()
    want = R.quantize(ints, 127.5).ravel()
    assert np.array_equal(got, want)
    inside = np.abs(ints.ravel()) <= 127
    assert (want[inside] % 2 == 0).all() and want[inside][0] == 0 and want[inside][-1] == 254      # .5 ties went to even
    # the default bound on ordinary flows
    v = rs.normal(0, 8, (1, 2, 20, 33)).astype(np.float32)
    assert torch.equal(of().flow_to_uint8(backend.put(torch.from_numpy(v))).cpu(), torch.from_numpy(R.quantize(v, 20)))


def resize_inputs():
    rs = np.random.RandomState(2)
    return rs.uniform(0, 255, (2, 2, 33, 47)).astype(np.float32)


def warp_inputs():
    rs = np.random.RandomState(3)
    i0, i1 = (R.sample_texture(R.texture(33, 47, s), 33, 47, 0.0, 0.0).astype(np.float32) for s in (4, 5))
    u = rs.uniform(-3, 3, (2, 33, 47)).astype(np.float32)
    u[:, 0, 0] = [-5.0, 40.0]          # far outside: clamped coordinates
    return i0, i1, u


def test_resize_and_warp_at_ragged_sizes(backend):
    K = kernels()
    a = resize_inputs()
    down = K.flow_resize(backend.put(torch.from_numpy(a)), (26, 38), 38 / 47.0, 26 / 33.0)
    want = np.stack([R.resize(a[:, 0], (26, 38), 38 / 47.0), R.resize(a[:, 1], (26, 38), 26 / 33.0)], axis=1)
    err = np.abs(down.cpu().numpy() - want).max()
    print("resize down: max abs err %.3g (bound %.3g)" % (err, RESIZE_BOUND["down"]))
    assert err <= RESIZE_BOUND["down"]
    up = K.flow_resize(down, (33, 47), 47 / 38.0, 33 / 26.0)
    d = down.cpu().numpy()
    want = np.stack([R.resize(d[:, 0], (33, 47), 47 / 38.0), R.resize(d[:, 1], (33, 47), 33 / 26.0)], axis=1)
    err = np.abs(up.cpu().numpy() - want).max()
    print("resize up: max abs err %.3g (bound %.3g)" % (err, RESIZE_BOUND["up"]))
    assert err <= RESIZE_BOUND["up"]
    same = K.flow_resize(down, (26, 38))          # the same size is a copy, bit for bit
    assert torch.equal(same, down)

    i0, i1, u = warp_inputs()
    st = backend.put(torch.zeros((2, 1, 6, 33, 47)))
    st[0, 0, :2] = backend.put(torch.from_numpy(u))
    cst = backend.put(torch.zeros((1, 4, 33, 47)))
    ctl = backend.put(torch.full((2, 1, 4), 7, dtype=torch.int32))
    K.tvl1_warp(backend.put(torch.from_numpy(i0[None])), backend.put(torch.from_numpy(i1[None])), st, cst, None, ctl[1])
    assert ctl[1, 0].tolist() == [0, 0, 0, 0] and ctl[0, 0].tolist() == [7, 7, 7, 7]
    want = R.warp(i0.astype(np.float64), i1.astype(np.float64), u[0].astype(np.float64), u[1].astype(np.float64))
    got = cst.cpu().numpy()[0]
    for name, g, r in zip(("gx", "gy", "grad", "rho_c"), got, want):
        err = np.abs(g - r).max() / np.abs(r).max()
        print("warp %s: rel err %.3g (bound %.3g)" % (name, err, WARP_BOUND[name]))
        assert err <= WARP_BOUND[name], name


# ------------------------------------------------------------------------------------------------------------------ 2. one chunk
@pytest.mark.parametrize("size", sorted(ITERATE_BOUND), ids=lambda s: "%dx%d" % s)
def test_one_chunk_from_a_random_state(backend, size):
    K = kernels()
    th, tw, halo = K.tvl1_tile_shape()
    assert (th, tw) == (TILE, TILE) and halo >= 1, "the tile changed: re-measure the yardsticks that were placed on its seams"
    h, w = size
    state, cst = iterate_inputs(h, w, 31)
    assert (cst[2] == 0).any()
    p = R.DEFAULTS
    want, want_err = R.iterate(tuple(state.astype(np.float64)), tuple(cst.astype(np.float64)), 10, p["lambda_"] * p["theta"],
                               p["theta"], p["tau"] / p["theta"])
    tvl1 = of().TVL1()
    splits = []                                     # the first chunk as the launcher splits it
    for n, _, ends in tvl1.launch_plan():
        splits.append(n)
        if ends:
            break
    assert sum(splits) == 10
    got, got_err = run_iterate(backend, state, cst, splits)
    err = max(np.abs(g - r).max() for g, r in zip(got, want))
    print("iterate %dx%d: max abs err %.3g (bound %.3g); chunk error %.6g vs %.6g" % (h, w, err, ITERATE_BOUND[size], got_err, want_err))
    assert err <= ITERATE_BOUND[size]
    assert abs(got_err - want_err) <= 1e-4 * want_err          # (a sum of h w positive fp32 terms)
    single, single_err = run_iterate(backend, state, cst, [1] * 10)
    assert np.array_equal(got.view(np.int32), single.view(np.int32)) and got_err == single_err
    uneven, _ = run_iterate(backend, state, cst, [4, 3, 3])
    assert np.array_equal(got.view(np.int32), uneven.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ 3. known motion
def check_against_reference(flow, iters, f64, it64, yard, label):
    assert np.array_equal(iters, it64), (label, iters.tolist(), it64.tolist())
    err = np.abs(flow - f64).max()
    print("%s: %d iterations, max abs flow err vs float64 %.3g px (bound %.3g)" % (label, iters.sum(), err, 4 * yard))
    assert err <= 4 * yard, label
    q, q64 = R.quantize(flow, 20), R.quantize(f64.astype(np.float32), 20)
    off = q.astype(np.int32) - q64.astype(np.int32)
    print("%s: %d of %d quantised pixels differ" % (label, (off != 0).sum(), off.size))
    assert (off != 0).mean() <= 0.005 and np.abs(off).max() <= 1, label


@pytest.mark.parametrize("name", sorted(MOTION_CASES))
def test_known_motion_end_to_end(backend, name):
    c = MOTION_CASES[name]
    prev, nxt, f64, it64 = motion_reference(name)
    flow, iters = run_tvl1(backend, [(prev, nxt)])
    if name == "shift_0.5_0.5_33x47":
        assert iters.shape[0] == 4          # 33 -> 26 -> 21 -> 17 -> (14): four levels
    check_against_reference(flow[0], iters[:, :, 0], f64, it64, c["yard"], name)
    true = np.array(c["shift"])[:, None, None]
    err = np.abs(margin(flow[0]) - true).max()
    print("%s: max err vs the true shift inside a 6 px margin %.3g px (referee %.3g)" % (name, err, c["ref_err"]))
    assert err <= c["ref_err"] + 4 * c["yard"]


# ------------------------------------------------------------------------------------------------------------------ 4. motion boundary
@pytest.mark.parametrize("variant", sorted(BOUNDARY))
def test_motion_boundary(backend, variant):
    c = BOUNDARY[variant]
    prev, nxt, f64, it64 = boundary_reference(variant)
    flow, iters = run_tvl1(backend, [(prev, nxt)], **c["params"])
    assert np.array_equal(iters[:, :, 0], it64)
    if variant == "fixed":
        assert iters.sum() == 750 and (iters == 30).all()
    diff = np.abs(flow[0] - f64).max(axis=0)
    away = seam_masks(*diff.shape)
    share = (diff > 0.01).mean()
    print("boundary %s: %d iterations, away from the seam max %.3g px (bound %.3g), share off by > 0.01 px %.4f (bound %.4f)"
          % (variant, iters.sum(), diff[away].max(), 4 * c["yard"], share, 4 * c["share"]))
    assert diff[away].max() <= 4 * c["yard"]
    assert share <= 4 * c["share"]


# ------------------------------------------------------------------------------------------------------------------ 5. batch
def test_batch_is_bit_identical_to_single_pairs(backend):
    prev, nxt = boundary_pair()
    mp, mn = R.shifted_pair(48, 64, (2.0, -1.0), 11)
    pairs = [(prev, prev), (mp, mn), (prev, nxt)]
    flow, iters = run_tvl1(backend, pairs)
    for i, pair in enumerate(pairs):
        f1, it1 = run_tvl1(backend, [pair])
        assert np.array_equal(flow[i].view(np.int32), f1[0].view(np.int32)), i
        assert np.array_equal(iters[:, :, i], it1[:, :, 0]), i
    assert (flow[0] == 0).all() and (iters[:, :, 0] == R.DEFAULTS["check_every"]).all()
    assert iters[:, :, 1].sum() > iters[:, :, 0].sum()
    again, it_again = run_tvl1(backend, pairs)
    assert np.array_equal(flow.view(np.int32), again.view(np.int32)) and np.array_equal(iters, it_again)


# ------------------------------------------------------------------------------------------------------------------ 6. no host read
@pytest.mark.gpu
def test_extract_is_capturable(hip_library):
    """FlowExtractor.extract holds no host read: it can be captured in a graph (one stream) and replayed on new frames."""
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(5)

    def clip(seed):
        tex = R.texture(32, 40, seed)
        g = np.stack([R.sample_texture(tex, 32, 40, 0.7 * t, -0.4 * t) for t in range(3)]).astype(np.uint8)
        return torch.from_numpy(np.stack([g, g // 2 + rs.randint(0, 60, g.shape).astype(np.uint8), 255 - g], axis=-1))

    ex = of().FlowExtractor(of().TVL1(iterations=40), bound=20, pair_batch=2)
    first, second = clip(41).to(dev), clip(42).to(dev)
    eager_first, eager_second = ex.extract(first), ex.extract(second)
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = ex.extract(static)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert out.shape == (2, 2, 32, 40) and torch.equal(out, eager_first)
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_second) and not torch.equal(eager_first, eager_second)


# ------------------------------------------------------------------------------------------------------------------ 7. files
def test_extract_flow_tool_writes_what_the_reader_reads(emu, tmp_path):
    from PIL import Image
    from action_detection_amd.train_data import FrameDirReader
    tex = R.texture(32, 40, 51)
    src, dst = tmp_path / "frames", tmp_path / "flow"
    os.makedirs(src / "video_a")
    frames = []
    for t in range(4):
        g = R.sample_texture(tex, 32, 40, -2.0 * t, 1.0 * t).astype(np.uint8)          # moves by (2, -1) per frame
        frames.append(np.stack([g, g, g], axis=-1))
        Image.fromarray(frames[-1]).save(str(src / "video_a" / ("img_%05d.jpg" % (t + 1))), quality=100, subsampling=0)
    spec = importlib.util.spec_from_file_location("extract_flow_tool", os.path.join(ROOT, "tools", "extract_flow.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main([str(src), str(dst), "--bound", "20", "--flow-prefix", "flow_", "--iterations", "40"]) == 0
    names = sorted(os.listdir(str(dst / "video_a")))
    assert names == ["flow_x_%05d.jpg" % i for i in (1, 2, 3)] + ["flow_y_%05d.jpg" % i for i in (1, 2, 3)]
    reader = FrameDirReader(str(dst), modality="Flow", flow_prefix="flow_")
    read = reader("video_a", [1, 2, 3])
    assert read.shape == (6, 32, 40, 1) and read.dtype == np.uint8
    # the same frames through the library: JPEG is lossy, so the files agree with the stack to a few levels -- and x (about
    # 127.5 + 2 * 6.375) and y (127.5 - 6.375) are far enough apart to tell a swapped order
    decoded = np.stack([np.asarray(Image.open(str(src / "video_a" / ("img_%05d.jpg" % (t + 1)))).convert("RGB")) for t in range(4)])
    flow = of().FlowExtractor(of().TVL1(iterations=40), bound=20).extract(torch.from_numpy(decoded))
    assert flow.shape == (3, 2, 32, 40)
    stack = of().stack_flow(flow, [0], new_length=3)
    assert stack.shape == (1, 6, 32, 40)
    assert torch.equal(stack[0, 0::2], flow[:, 0]) and torch.equal(stack[0, 1::2], flow[:, 1])
    diff = np.abs(stack[0].numpy().astype(np.int32) - read[..., 0].astype(np.int32))
    assert diff.mean() < 2.0
    centre = stack[0, :, 8:-8, 8:-8].numpy().astype(np.float64)
    assert abs(centre[0::2].mean() - (127.5 + 2 * 6.375)) < 2 and abs(centre[1::2].mean() - (127.5 - 6.375)) < 2
    two = of().stack_flow(flow, [0, 1], new_length=2)
    assert torch.equal(two[1, 0], flow[1, 0]) and torch.equal(two[1, 3], flow[2, 1])
    with pytest.raises(ValueError):
        of().stack_flow(flow, [2], new_length=2)


# ------------------------------------------------------------------------------------------------------------------ yardsticks
def _measure():
    """Print every yardstick of this file: the float32 referee against the float64 referee."""
    a = resize_inputs()
    d64 = np.stack([R.resize(a[:, 0], (26, 38), 38 / 47.0), R.resize(a[:, 1], (26, 38), 26 / 33.0)], axis=1)
    d32 = np.stack([R.resize(a[:, 0], (26, 38), 38 / 47.0, np.float32), R.resize(a[:, 1], (26, 38), 26 / 33.0, np.float32)], axis=1)
    u64 = np.stack([R.resize(d32[:, 0], (33, 47), 47 / 38.0), R.resize(d32[:, 1], (33, 47), 33 / 26.0)], axis=1)
    u32 = np.stack([R.resize(d32[:, 0], (33, 47), 47 / 38.0, np.float32), R.resize(d32[:, 1], (33, 47), 33 / 26.0, np.float32)], axis=1)
    print("resize: down %.3g, up %.3g" % (np.abs(d32 - d64).max(), np.abs(u32 - u64).max()))
    i0, i1, u = warp_inputs()
    w64 = R.warp(i0.astype(np.float64), i1.astype(np.float64), u[0].astype(np.float64), u[1].astype(np.float64))
    w32 = R.warp(i0, i1, u[0], u[1])
    print("warp (relative): " + ", ".join("%.3g" % (np.abs(g - r).max() / np.abs(r).max()) for g, r in zip(w32, w64)))
    p = R.DEFAULTS
    for size in sorted(ITERATE_BOUND):
        state, cst = iterate_inputs(size[0], size[1], 31)
        args = (10, p["lambda_"] * p["theta"], p["theta"], p["tau"] / p["theta"])
        s64, _ = R.iterate(tuple(state.astype(np.float64)), tuple(cst.astype(np.float64)), *args)
        s32, _ = R.iterate(tuple(state), tuple(cst), *args)
        print("iterate %s: %.3g" % (size, max(np.abs(g - r).max() for g, r in zip(s32, s64))))
    for name in sorted(MOTION_CASES):
        c = MOTION_CASES[name]
        prev, nxt, f64, it64 = motion_reference(name)
        f32, it32 = R.tvl1(prev, nxt, dtype=np.float32)
        q = (R.quantize(f32, 20) != R.quantize(f64.astype(np.float32), 20)).sum()
        print("%s: iterations %d (float32 %d, schedules equal: %s), levels %d, yardstick %.3g px, referee vs true shift %.3g px, "
              "quantised pixels that differ %d" % (name, it64.sum(), it32.sum(), np.array_equal(it32, it64), it64.shape[0],
                                                   np.abs(f32 - f64).max(),
                                                   np.abs(margin(f64) - np.array(c["shift"])[:, None, None]).max(), q))
    for variant in sorted(BOUNDARY):
        prev, nxt, f64, it64 = boundary_reference(variant)
        f32, it32 = R.tvl1(prev, nxt, dtype=np.float32, **BOUNDARY[variant]["params"])
        diff = np.abs(f32 - f64).max(axis=0)
        print("boundary %s: iterations %d (schedules equal: %s), whole image max %.3g, away from the seam %.3g, share > 0.01 px %.4f"
              % (variant, it64.sum(), np.array_equal(it32, it64), diff.max(), diff[seam_masks(*diff.shape)].max(), (diff > 0.01).mean()))


if __name__ == "__main__":
    _measure()
