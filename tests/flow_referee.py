"""Referee for the TV-L1 optical flow kernels (csrc/flow.hip): a plain numpy restatement of the algorithm DESIGN.md section 3.9
fixes, in float64 by default.  Every function takes ``dtype``; run in float32 it is the yardstick for what fp32 arithmetic alone
does to a result (the kernels differ from it only by summation order), which is where the tests' tolerances come from.
Not a port of any implementation: there is no OpenCV here and no flow code in the reference tree.
"""
import numpy as np

DEFAULTS = dict(tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, iterations=300, scale_step=0.8,
                check_every=10)


def gray(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def quantize(v, bound):
    """dense_flow's CAST on a float32 array, in float32, in the kernel's order of operations."""
    v = np.asarray(v, dtype=np.float32)
    b = np.float32(bound)
    mid = np.rint(np.float32(255.0) * (v + b) / (np.float32(2.0) * b))
    return np.where(v > b, 255, np.where(v < -b, 0, mid)).astype(np.uint8)


def pyramid_sizes(h, w, nscales, scale_step, min_side=16):
    sizes = [(int(h), int(w))]
    while len(sizes) < nscales:
        nh, nw = int(sizes[-1][0] * scale_step + 0.5), int(sizes[-1][1] * scale_step + 0.5)
        if nh < min_side or nw < min_side:
            break
        sizes.append((nh, nw))
    return sizes


def _axis(src, dst, dtype):
    s = np.maximum(dtype(src) / dtype(dst) * (np.arange(dst).astype(dtype) + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = np.minimum(s.astype(np.int64), src - 1)
    return i0, np.minimum(i0 + 1, src - 1), (s - i0.astype(dtype)).astype(dtype)


def resize(img, size, mul=1.0, dtype=np.float64):
    """Bilinear, source coordinate (d + 0.5) * src / dst - 0.5 with clamped indices, on the last two axes; times ``mul``."""
    dtype = np.dtype(dtype).type
    img = np.asarray(img, dtype=dtype)
    hs, ws = img.shape[-2:]
    y0, y1, fy = _axis(hs, size[0], dtype)
    x0, x1, fx = _axis(ws, size[1], dtype)
    fy = fy[:, None]
    one = dtype(1)
    top = (one - fx) * img[..., y0[:, None], x0[None, :]] + fx * img[..., y0[:, None], x1[None, :]]
    bot = (one - fx) * img[..., y1[:, None], x0[None, :]] + fx * img[..., y1[:, None], x1[None, :]]
    return (((one - fy) * top + fy * bot) * dtype(mul)).astype(dtype)


def gradient(img):
    """Centred differences 0.5 * (I[x + 1] - I[x - 1]) with clamped indices -> (Ix, Iy)."""
    h, w = img.shape
    half = img.dtype.type(0.5)
    xs, ys = np.arange(w), np.arange(h)
    ix = half * (img[:, np.minimum(xs + 1, w - 1)] - img[:, np.maximum(xs - 1, 0)])
    iy = half * (img[np.minimum(ys + 1, h - 1), :] - img[np.maximum(ys - 1, 0), :])
    return ix, iy


def sample(img, cx, cy):
    """Bilinear sample at coordinates already clamped to the image."""
    h, w = img.shape
    t = img.dtype.type
    x0 = np.minimum(cx.astype(np.int64), w - 1)
    y0 = np.minimum(cy.astype(np.int64), h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = cx - x0.astype(t), cy - y0.astype(t)
    one = t(1)
    return (one - fy) * ((one - fx) * img[y0, x0] + fx * img[y0, x1]) + fy * ((one - fx) * img[y1, x0] + fx * img[y1, x1])


def warp(i0, i1, u1, u2):
    """Per-warp constants (gx, gy, grad, rho_c) of one pair at the flow (u1, u2)."""
    h, w = i1.shape
    t = i1.dtype.type
    ix, iy = gradient(i1)
    xs, ys = np.meshgrid(np.arange(w).astype(t), np.arange(h).astype(t))
    cx = np.minimum(np.maximum(xs + u1, t(0)), t(w - 1))
    cy = np.minimum(np.maximum(ys + u2, t(0)), t(h - 1))
    i1w, gx, gy = sample(i1, cx, cy), sample(ix, cx, cy), sample(iy, cx, cy)
    return gx, gy, gx * gx + gy * gy, ((i1w - gx * u1) - gy * u2) - i0


def _backward(p, axis):
    """p[i] - p[i - 1] with p[-1] = 0."""
    d = p.copy()
    if axis == 1:
        d[:, 1:] -= p[:, :-1]
    else:
        d[1:, :] -= p[:-1, :]
    return d


def _forward(u, axis):
    """u[i + 1] - u[i], zero in the last column / row."""
    d = np.zeros_like(u)
    if axis == 1:
        d[:, :-1] = u[:, 1:] - u[:, :-1]
    else:
        d[:-1, :] = u[1:, :] - u[:-1, :]
    return d


def iterate(state, consts, n, l_t, theta, taut):
    """``n`` iterations from ``state`` = (u1, u2, p11, p12, p21, p22) with ``consts`` = (gx, gy, grad, rho_c).
    -> (new state, error of the last iteration)."""
    u1, u2, p11, p12, p21, p22 = (a.copy() for a in state)
    gx, gy, grad, rho_c = consts
    t = u1.dtype.type
    l_t, theta, taut = t(l_t), t(theta), t(taut)
    err = 0.0
    safe = np.where(grad > t(1e-9), grad, t(1))
    for _ in range(n):
        rho = (rho_c + gx * u1) + gy * u2
        thr = l_t * grad
        lo, hi = rho < -thr, rho > thr
        mid = ~lo & ~hi & (grad > t(1e-9))
        fi = np.where(mid, -rho / safe, t(0))
        d1 = np.where(lo, l_t * gx, np.where(hi, -l_t * gx, fi * gx))
        d2 = np.where(lo, l_t * gy, np.where(hi, -l_t * gy, fi * gy))
        n1 = (u1 + d1) + theta * (_backward(p11, 1) + _backward(p12, 0))
        n2 = (u2 + d2) + theta * (_backward(p21, 1) + _backward(p22, 0))
        err = float(np.sum((n1 - u1) ** 2 + (n2 - u2) ** 2))
        u1, u2 = n1, n2
        u1x, u1y, u2x, u2y = _forward(u1, 1), _forward(u1, 0), _forward(u2, 1), _forward(u2, 0)
        q1 = t(1) + taut * np.sqrt(u1x * u1x + u1y * u1y)
        q2 = t(1) + taut * np.sqrt(u2x * u2x + u2y * u2y)
        p11, p12 = (p11 + taut * u1x) / q1, (p12 + taut * u1y) / q1
        p21, p22 = (p21 + taut * u2x) / q2, (p22 + taut * u2y) / q2
    return (u1, u2, p11, p12, p21, p22), err


def tvl1(prev, nxt, dtype=np.float64, **params):
    """One pair of gray images [H, W] -> (flow [2, H, W], iterations int32 [levels, warps], level 0 the coarsest)."""
    p = dict(DEFAULTS, **params)
    t = np.dtype(dtype).type
    h, w = prev.shape
    sizes = pyramid_sizes(h, w, p["nscales"], p["scale_step"])
    i0, i1 = [np.asarray(prev, dtype=t)], [np.asarray(nxt, dtype=t)]
    for s in sizes[1:]:
        i0.append(resize(i0[-1], s, dtype=t))
        i1.append(resize(i1[-1], s, dtype=t))
    l_t, taut = p["lambda_"] * p["theta"], p["tau"] / p["theta"]
    iters = np.zeros((len(sizes), p["warps"]), dtype=np.int32)
    u1 = u2 = None
    for level in range(len(sizes) - 1, -1, -1):
        lh, lw = sizes[level]
        if u1 is None:
            u1, u2 = np.zeros((lh, lw), dtype=t), np.zeros((lh, lw), dtype=t)
        else:
            ph, pw = sizes[level + 1]
            u1 = resize(u1, (lh, lw), lw / float(pw), dtype=t)
            u2 = resize(u2, (lh, lw), lh / float(ph), dtype=t)
        state = (u1, u2) + tuple(np.zeros((lh, lw), dtype=t) for _ in range(4))
        thresh = p["epsilon"] * p["epsilon"] * lh * lw
        for wi in range(p["warps"]):
            consts = warp(i0[level], i1[level], state[0], state[1])
            done = 0
            while done < p["iterations"]:
                n = min(p["check_every"], p["iterations"] - done)
                state, err = iterate(state, consts, n, l_t, p["theta"], taut)
                done += n
                if err < thresh:
                    break
            iters[len(sizes) - 1 - level, wi] = done
        u1, u2 = state[0], state[1]
    return np.stack([u1, u2]), iters


# ---------------------------------------------------------------------------------------------------------------- test inputs
def texture(h, w, seed, margin=8):
    """Seeded uniform noise blurred twice with the 5-tap binomial filter, scaled to [0, 255]; ``margin`` extra pixels all round
    so that shifted samples stay inside.  float64 [h + 2 margin, w + 2 margin]."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(0.0, 1.0, (h + 2 * margin, w + 2 * margin))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for _ in range(2):
        a = np.apply_along_axis(lambda r: np.convolve(np.pad(r, 2, mode="edge"), k, mode="valid"), 1, a)
        a = np.apply_along_axis(lambda r: np.convolve(np.pad(r, 2, mode="edge"), k, mode="valid"), 0, a)
    a -= a.min()
    return a * (255.0 / a.max())


def sample_texture(tex, h, w, dx, dy, margin=8):
    """The [h, w] window of ``tex`` sampled bilinearly at (x + dx, y + dy) (dx, dy scalars or [h, w] arrays), rounded to
    integers -> float64 in [0, 255]."""
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    cx, cy = xs + margin + dx, ys + margin + dy
    return np.clip(np.rint(sample(tex, cx, cy)), 0, 255)


def shifted_pair(h, w, shift, seed):
    """(prev, nxt) uint8 with nxt(x + shift) = prev(x): the true flow is ``shift`` = (x, y) everywhere."""
    tex = texture(h, w, seed)
    prev = sample_texture(tex, h, w, 0.0, 0.0)
    nxt = sample_texture(tex, h, w, -shift[0], -shift[1])
    return prev.astype(np.uint8), nxt.astype(np.uint8)
