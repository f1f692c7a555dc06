"""TV-L1 optical flow on the GPU: the "Extract Frames and Optical Flow Images" stage of the reference's workflow, which the
reference hands to ``dense_flow`` (OpenCV's CUDA ``OpticalFlowDual_TVL1``).  ``FlowExtractor`` turns the RGB frames of a
video into the ``flow_x`` / ``flow_y`` uint8 images ``FrameDirReader(modality="Flow")`` reads, ``stack_flow`` into the
``[n, 2 * new_length, H, W]`` stacks the Flow model takes; ``tools/extract_flow.py`` is the driver over frame directories.

The algorithm is the published TV-L1 (Zach, Pock, Bischof 2007; Sanchez et al., IPOL 2013) with the defaults of
``cuda::OpticalFlowDual_TVL1::create()``, restated in DESIGN.md section 3.9 and checked against a float64 referee
(tests/flow_referee.py).  Agreement with ``dense_flow``'s own files is NOT pinned: there is no OpenCV to compare with.

Nothing is read back while a batch of pairs runs: the host enqueues the worst-case number of ``ssn_tvl1_iterate`` launches
and every pair keeps its own ``done`` flag and iteration count on the device (csrc/flow.hip), so a call can be captured
in a graph.
"""
from collections import namedtuple

import torch

from . import kernels as K

FlowResult = namedtuple("FlowResult", "flow iterations")
FlowResult.__doc__ = """flow float32 [B, 2, H, W] (x then y, pixels of the full-size image); iterations int32 [levels, warps,
B] on the device: the iterations every warp of every pair ran, level 0 the coarsest."""


def pyramid_sizes(h, w, nscales, scale_step, min_side=16):
    """[(H, W)] from the full size down: a level is floor(previous * scale_step + 0.5) per axis; the pyramid stops before a
    level with a side below `min_side`."""
    sizes = [(int(h), int(w))]
    while len(sizes) < nscales:
        nh, nw = int(sizes[-1][0] * scale_step + 0.5), int(sizes[-1][1] * scale_step + 0.5)
        if nh < min_side or nw < min_side:
            break
        sizes.append((nh, nw))
    return sizes


def rgb_to_gray(rgb):
    """uint8 [..., H, W, 3] -> uint8 [..., H, W]: (4899 R + 9617 G + 1868 B + 8192) >> 14, exact."""
    return K.flow_gray(rgb.contiguous())


def flow_to_uint8(flow, bound=20):
    """dense_flow's CAST in float32: v > bound -> 255, v < -bound -> 0, else rint(255 (v + bound) / (2 bound)), half to even."""
    return K.flow_quantize(flow.contiguous(), bound)


class TVL1:
    """``TVL1(**params)(prev, nxt)`` -> ``FlowResult``.  prev / nxt: gray uint8 or float32 [B, H, W] on the device.

    ``check_every``: the error is tested after every chunk of that many iterations (of the chunk's last iteration, against
    ``epsilon ** 2 * H * W`` of the level); ``epsilon=0`` runs fixed counts.  ``iterations_per_launch`` limits how many
    iterations one ``ssn_tvl1_iterate`` launch advances (default: what the kernel's halo allows); results do not depend on
    it -- 1 is the one-launch-per-iteration baseline of tools/bench_flow.py."""

    def __init__(self, tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, iterations=300, scale_step=0.8,
                 check_every=10, iterations_per_launch=None):
        if not (nscales >= 1 and warps >= 1 and iterations >= 1 and check_every >= 1 and 0 < scale_step < 1 and epsilon >= 0):
            raise ValueError("TVL1: bad parameters")
        self.tau, self.lambda_, self.theta = float(tau), float(lambda_), float(theta)
        self.nscales, self.warps, self.iterations = int(nscales), int(warps), int(iterations)
        self.epsilon, self.scale_step, self.check_every = float(epsilon), float(scale_step), int(check_every)
        self.iterations_per_launch = iterations_per_launch

    def launch_plan(self):
        """[(n_iter, starts_chunk, ends_chunk)] of one warp: chunks of check_every (the last one shorter), each split into
        launches of at most the halo."""
        halo = K.tvl1_tile_shape()[2]
        per = halo if self.iterations_per_launch is None else max(1, min(int(self.iterations_per_launch), halo))
        plan = []
        for c0 in range(0, self.iterations, self.check_every):
            n = min(self.check_every, self.iterations - c0)
            for j in range(0, n, per):
                plan.append((min(per, n - j), j == 0, j + per >= n))
        return plan

    @torch.no_grad()
    def __call__(self, prev, nxt):
        if prev.shape != nxt.shape or prev.dim() != 3 or prev.dtype != nxt.dtype or prev.dtype not in (torch.uint8, torch.float32):
            raise ValueError("TVL1: prev and nxt must both be uint8 or float32 [B, H, W]")
        dev = prev.device
        b, h, w = prev.shape
        sizes = pyramid_sizes(h, w, self.nscales, self.scale_step)
        i0 = [prev.to(torch.float32).contiguous().unsqueeze(1)]
        i1 = [nxt.to(torch.float32).contiguous().unsqueeze(1)]
        for s in sizes[1:]:
            i0.append(K.flow_resize(i0[-1], s))
            i1.append(K.flow_resize(i1[-1], s))
        th, tw, _ = K.tvl1_tile_shape()
        plan = self.launch_plan()
        l_t, taut = self.lambda_ * self.theta, self.tau / self.theta
        iterations = torch.zeros((len(sizes), self.warps, b), device=dev, dtype=torch.int32)
        ctl = torch.zeros((2, b, 4), device=dev, dtype=torch.int32)
        k = 0                      # control records are read in slot k & 1 and written in the other one
        state = None
        for level in range(len(sizes) - 1, -1, -1):
            lh, lw = sizes[level]
            new = torch.zeros((2, b, 6, lh, lw), device=dev, dtype=torch.float32)
            if state is not None:      # the coarser level's flow, resampled and scaled to this size
                ph, pw = sizes[level + 1]
                K.flow_resize(state[0][:, 0:2], (lh, lw), lw / float(pw), lh / float(ph), out=new[0][:, 0:2],
                              src1=state[1][:, 0:2], ctl=ctl[k & 1])
            state = new
            cst = torch.empty((b, 4, lh, lw), device=dev, dtype=torch.float32)
            part = torch.zeros((2, b, -(-lh // th) * -(-lw // tw)), device=dev, dtype=torch.float32)
            thresh = self.epsilon * self.epsilon * lh * lw
            a0, a1 = i0[level][:, 0], i1[level][:, 0]
            for wi in range(self.warps):
                K.tvl1_warp(a0, a1, state, cst, None if wi == 0 else ctl[k & 1], ctl[(k + 1) & 1])
                k += 1
                it = iterations[len(sizes) - 1 - level, wi]
                chunk = -1
                for n_iter, starts, ends in plan:
                    chunk += starts
                    K.tvl1_iterate(state, cst, n_iter, l_t, self.theta, taut, thresh, ctl[k & 1], ctl[(k + 1) & 1],
                                   part[(chunk - 1) & 1] if starts and chunk > 0 else None, part[chunk & 1] if ends else None, it)
                    k += 1
        flow = K.flow_resize(state[0][:, 0:2], (h, w), src1=state[1][:, 0:2], ctl=ctl[k & 1])      # (same size: a copy)
        return FlowResult(flow, iterations)


class FlowExtractor:
    """``FlowExtractor(tvl1, bound=20, pair_batch=16).extract(frames)``: uint8 RGB frames [T, H, W, 3] on the device -> uint8
    [T - 1, 2, H, W], the quantised x and y flow of the consecutive pairs (frame t -> t + 1), ``pair_batch`` pairs per TVL1
    call.  Nothing leaves the GPU."""

    def __init__(self, tvl1=None, bound=20, pair_batch=16):
        self.tvl1 = tvl1 if tvl1 is not None else TVL1()
        self.bound = float(bound)
        self.pair_batch = int(pair_batch)
        if self.pair_batch < 1 or not self.bound > 0:
            raise ValueError("FlowExtractor: pair_batch >= 1 and bound > 0")

    @torch.no_grad()
    def extract(self, frames):
        if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8 or frames.shape[0] < 2:
            raise ValueError("FlowExtractor.extract: uint8 [T >= 2, H, W, 3] expected")
        gray = rgb_to_gray(frames)
        t = gray.shape[0]
        out = torch.empty((t - 1, 2, gray.shape[1], gray.shape[2]), device=frames.device, dtype=torch.uint8)
        for s in range(0, t - 1, self.pair_batch):
            e = min(s + self.pair_batch, t - 1)
            out[s:e] = flow_to_uint8(self.tvl1(gray[s:e], gray[s + 1:e + 1]).flow, self.bound)
        return out


def stack_flow(flow_u8, start_indices, new_length=5):
    """The Flow model's input stacks from extracted flow: flow_u8 [P, 2, H, W], the images of pairs 0 .. P - 1 (pair p is
    ``flow_x/y_%05d`` with number p + 1); for every start index s (0-based pair) the ``new_length`` consecutive pairs from
    s, interleaved x, y, x, y, ... as ``FrameDirReader(modality="Flow")`` stacks them -> [n, 2 * new_length, H, W]."""
    if flow_u8.dim() != 4 or flow_u8.shape[1] != 2:
        raise ValueError("stack_flow: [P, 2, H, W] expected")
    idx = torch.as_tensor(start_indices, device=flow_u8.device, dtype=torch.long).reshape(-1)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) + new_length > flow_u8.shape[0]):
        raise ValueError("stack_flow: a stack of %d pairs does not fit behind every start index" % new_length)
    rows = idx[:, None] + torch.arange(new_length, device=flow_u8.device)[None, :]
    picked = flow_u8[rows]                                   # [n, new_length, 2, H, W]
    return picked.reshape(idx.numel(), 2 * new_length, flow_u8.shape[2], flow_u8.shape[3])
