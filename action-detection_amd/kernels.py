"""Thin tensor-level wrappers over the C ABI (include/ssn_hip.h).

Every function launches on the caller's current HIP stream and writes into caller-provided
tensors (PyTorch owns all device memory).  ``ChanSlice`` addresses a channel range of an NCHW
tensor, which is how the concat-free Inception block outputs are written and read.
"""
import ctypes
from collections import namedtuple

import torch

from . import _lib
from ._lib import SsnStppTable, STPP_MAX_PARTS


class ChanSlice(namedtuple("ChanSlice", "t c0 c")):
    """Channels [c0, c0+c) of a contiguous NCHW tensor ``t``."""

    @property
    def ptr(self):
        _, _, h, w = self.t.shape
        return self.t.data_ptr() + 4 * self.c0 * h * w

    @property
    def img_stride(self):
        _, ct, h, w = self.t.shape
        return ct * h * w

    @property
    def n(self):
        return self.t.shape[0]

    @property
    def hw(self):
        return self.t.shape[2], self.t.shape[3]


def full(t):
    return ChanSlice(t, 0, t.shape[1])


def _check(*tensors):
    lib = _lib.get_lib()
    for t in tensors:
        if t is None:
            continue
        tt = t.t if isinstance(t, ChanSlice) else t
        if not tt.is_contiguous():
            raise ValueError("SSN HIP ops need contiguous tensors")
        if not lib.is_emulator and not tt.is_cuda:
            raise RuntimeError("SSN HIP ops need HIP (cuda) tensors; there is no CPU fallback")
    return lib


def _stream(lib, t):
    if lib.is_emulator:
        return None
    tt = t.t if isinstance(t, ChanSlice) else t
    return torch.cuda.current_stream(tt.device).cuda_stream


def _p(t):
    if t is None:
        return None
    return t.ptr if isinstance(t, ChanSlice) else t.data_ptr()


# ------------------------------------------------------------------------------------ amax slots
# The split-operand ("x6") kernels scale every operand tensor by a power of two derived from an upper bound of its
# largest magnitude (include/ssn_hip.h: "amax slots").  The association tensor -> slot lives on the torch tensor
# object (attribute `_ssn_amax`, a 1-element fp32 view): producers hand the slot of their OUTPUT tensor to the kernel,
# which raises it; consumers hand the slot of their INPUT tensor.  Executors attach zeroed slots to the tensors they
# allocate (attach_amax); a tensor without a slot (test inputs, the caller's frames) is measured on the spot.
def attach_amax(t, slot=None):
    """Give tensor `t` an amax slot (a zeroed 1-element tensor, or the given view of a zeroed pool)."""
    t._ssn_amax = torch.zeros(1, device=t.device, dtype=torch.float32) if slot is None else slot
    return t


def _tensor_of(x):
    return x.t if isinstance(x, ChanSlice) else x


def attach_amax_ext(t, slot, first_channel):
    """Second amax slot for the channels >= first_channel of `t` (a block-output tensor that also holds the block's reduce
    rows): the two regions are written and read by concurrent launches, so each has its own slot -- a slot is then always
    complete before anything reads it (results stay bit-deterministic)."""
    t._ssn_amax_ext = (slot, int(first_channel))
    return t


def _slot_of(x):
    """The amax slot that covers ChanSlice / tensor x (None: not tracked)."""
    t = _tensor_of(x)
    ext = getattr(t, "_ssn_amax_ext", None)
    if ext is not None and isinstance(x, ChanSlice) and x.c0 >= ext[1]:
        return ext[0]
    return getattr(t, "_ssn_amax", None)


def _slot_ext(x):
    ext = getattr(_tensor_of(x), "_ssn_amax_ext", None)
    return None if ext is None else ext[0]


def _amax_out(x):
    """Slot pointer of the tensor (region) a kernel writes (None: not tracked)."""
    return _p(_slot_of(x))


def tensor_amax(t, slot=None):
    """Measure max |t| into `slot` (a fresh zeroed one by default) and return the slot."""
    lib = _check(t)
    if slot is None:
        slot = torch.zeros(1, device=t.device, dtype=torch.float32)
    lib.call("ssn_tensor_amax", _p(t), t.numel(), _p(slot), _stream(lib, t))
    return slot


def _amax_in(x):
    """Slot (tensor, kept alive by the caller) of the tensor a split kernel reads; untracked tensors are measured now."""
    slot = _slot_of(x)
    return slot if slot is not None else tensor_amax(_tensor_of(x))


# Measurement hook (bench.py): when a list is installed here, the wrappers of the HBM-bound kernels of the path (STPP,
# heads, row selection, losses) bracket their launch with HIP events on the launch stream and append
# (kernel name, algorithmic bytes = operands read + results written, start event, end event).
HBM_PROFILER = None
HBM_PROFILER_REPEATS = 16


def _hbm_timed(fn):
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kw):
        prof = HBM_PROFILER
        if prof is None:
            return fn(*args, **kw)
        flat = [b for a in args for b in (a if isinstance(a, (list, tuple)) else (a,))]
        tens = [a for a in flat if torch.is_tensor(a)]
        slices = [a for a in args if isinstance(a, ChanSlice)]
        first = tens[0] if tens else (slices[0].t if slices else None)
        if first is None or not first.is_cuda:
            return fn(*args, **kw)
        nbytes = sum(t.numel() * t.element_size() for t in tens)
        nbytes += sum(c.n * c.c * c.hw[0] * c.hw[1] * c.t.element_size() for c in slices)
        # an event pair around ONE launch of a 2-5 us kernel reads 15-25 us (the pair's own granularity): the launch is
        # repeated back to back -- these kernels are pure functions of their operands (no atomics, nothing accumulated unless
        # asked) -- and the pair divided by the count
        reps = HBM_PROFILER_REPEATS
        if kw.get("accumulate") or kw.get("accumulate_dx") or (fn.__name__ == "gap_bwd" and len(args) > 2 and args[2]) or \
                (fn.__name__ == "linear_bwd" and len(args) > 6 and args[6]):
            reps = 1
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn(*args, **kw)
        for _ in range(reps - 1):
            fn(*args, **kw)
        e.record()
        prof.append((fn.__name__, nbytes, s, e, reps))
        return out
    return wrapper


# ------------------------------------------------------------------------------------ backbone
def bn_fold(conv_bias, gamma, beta, mean, var, eps, scale, shift):
    lib = _check(conv_bias, gamma, beta, mean, var, scale, shift)
    lib.call("ssn_bn_fold", _p(conv_bias), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), _p(scale),
             _p(shift), gamma.numel(), _stream(lib, gamma))


def packed_floats(cout, cin, ksize, transposed, x6=False):
    fn = _lib.get_lib().cdll.ssn_conv_x6_packed_floats if x6 else _lib.get_lib().cdll.ssn_conv_packed_floats
    return int(fn(cout, cin, ksize, int(bool(transposed))))


def dgrad_layout(ksize, stride, pad, h, w):
    """Packed-weight layout ssn_conv_dgrad wants for this conv (2 = parity-ordered stride-2 path, else 1)."""
    return int(_lib.get_lib().cdll.ssn_conv_dgrad_layout(ksize, stride, pad, h, w))


def pack_weights(w, transposed, out=None):
    """Re-lay a torch-layout weight [Cout, Cin, k, k] into the slab/lane-half order the conv kernels read.

    transposed=False/0 -> forward operand, True/1 -> dgrad operand, 2 -> parity-ordered stride-2 dgrad operand
    (use dgrad_layout() to choose between 1 and 2).
    """
    lib = _check(w, out)
    cout, cin, k, _ = w.shape
    n = packed_floats(cout, cin, k, transposed)
    if out is None:
        out = torch.empty(n, device=w.device, dtype=torch.float32)
    assert out.numel() >= n
    lib.call("ssn_conv_pack_weights", _p(w), _p(out), cout, cin, k, int(transposed), _stream(lib, w))
    return out


_PACK_BATCH = None      # the open PackBatch, if any


def _pack_alloc(nfloats, device):
    """Operand buffer of a packing call: fresh, or -- inside a PackBatch -- the persistent one of this position in the batch."""
    if _PACK_BATCH is not None:
        return _PACK_BATCH.take(int(nfloats), device)
    return torch.empty(int(nfloats), device=device, dtype=torch.float32)


class PackBatch:
    """``with PackBatch(state, device):`` -- the x6 / planes weight-packing calls inside (pack_weights_multi(x6=True), pack_rect_multi,
    pack_weights_rect, pack_dgrad_s2, pack_dgrad_rect, s2d_weights' output) are only RECORDED; leaving the block issues all of them
    in three launches through a device-resident plan (ssn_conv_x6_pack_batch_end).  `state` is a dict the caller keeps (one per
    backbone and kind of pass): it holds the operand buffers -- the k-th allocation of a batch gets the same buffer every time, so
    the recorded entries repeat from step to step and the plan is written once -- and the plan buffer.  The returned operands are
    valid after the block; they are overwritten by the next batch on the same state (same weights -> same contents).

    `side` (a torch.cuda.Stream) with leading entries marked by stem_done() (or given as `n_first`): leaving the block issues those
    leading entries on the current stream and all others on `side` (ssn_conv_x6_pack_batch_end_lanes); the operands recorded behind
    the mark are valid on the current stream only after pack_batch_join().  No mark or no `side`: one stream."""

    def __init__(self, state, device, n_first=None, side=None):
        self.state, self.device, self.k = state, device, 0
        self.n_first, self.side = n_first, side

    def stem_done(self):
        """everything recorded so far belongs to the launches that run beside the side stream's part"""
        self.n_first = int(self.lib.cdll.ssn_conv_x6_pack_batch_entries())

    def take(self, nfloats, device):
        bufs = self.state.setdefault("bufs", [])
        if self.k < len(bufs) and bufs[self.k].numel() == nfloats and bufs[self.k].device == device:
            t = bufs[self.k]
        else:
            t = torch.empty(nfloats, device=device, dtype=torch.float32)
            del bufs[self.k:]
            bufs.append(t)
        self.k += 1
        return t

    def __enter__(self):
        global _PACK_BATCH
        assert _PACK_BATCH is None, "PackBatch blocks do not nest"
        self.lib = _lib.get_lib()
        self.lib.call("ssn_conv_x6_pack_batch_begin")
        _PACK_BATCH = self
        return self

    def __exit__(self, et, ev, tb):
        global _PACK_BATCH
        _PACK_BATCH = None
        if et is not None:
            self.lib.cdll.ssn_conv_x6_pack_batch_abort()
            return False
        need = int(self.lib.cdll.ssn_conv_x6_pack_batch_entries()) * int(self.lib.cdll.ssn_conv_x6_pack_entry_bytes())
        plan, fresh = self.state.get("plan"), 0
        if need and (plan is None or plan.numel() < need or plan.device != self.device):
            plan = self.state["plan"] = torch.empty(max(need, 1 << 16), device=self.device, dtype=torch.uint8)
            fresh = 1
        stream = _stream(self.lib, plan) if plan is not None else None
        if self.side is not None and self.n_first is not None and plan is not None:
            # (the emulator has no streams: any non-null value splits the launches)
            side = 1 if self.lib.is_emulator else self.side.cuda_stream
            self.lib.call("ssn_conv_x6_pack_batch_end_lanes", _p(plan), plan.numel(), fresh, int(self.n_first), stream, side)
        else:
            self.lib.call("ssn_conv_x6_pack_batch_end", _p(plan), plan.numel() if plan is not None else 0, fresh, stream)
        return False


def pack_batch_join(device):
    """The current stream of `device` waits for the side part of the last split PackBatch (nothing pending: nothing happens)."""
    lib = _lib.get_lib()
    lib.call("ssn_conv_x6_pack_batch_join", None if lib.is_emulator else torch.cuda.current_stream(device).cuda_stream)


def pack_weights_multi(entries, x6=False):
    """entries: list of (weights, mode) with weights = [w], [wA, wB] (fused pair) or -- x6 only -- [wA, wB, wC]
    ... [wA, wB, wC, wD] (concatenated output channels).

    Returns one packed tensor per entry (views of a single flat buffer); ceil(len / 40) launches in total.
    x6=True: scale + split every weight into two f16 planes for the conv_x6 kernels (modes 0/1, ksize 1/3 only).
    """
    if not entries:
        return []
    n = len(entries)
    lib = _check(*[w for ws, _ in entries for w in ws])
    first = entries[0][0][0]
    couts = [sum(w.shape[0] for w in ws) for ws, _ in entries]
    cins = [ws[0].shape[1] for ws, _ in entries]
    kss = [ws[0].shape[2] for ws, _ in entries]
    sizes = [packed_floats(co, ci, k, m, x6) for co, ci, k, (_, m) in zip(couts, cins, kss, entries)]
    flat = _pack_alloc(sum(sizes), first.device) if x6 else torch.empty(sum(sizes), device=first.device, dtype=torch.float32)
    outs, off = [], 0
    for sz in sizes:
        outs.append(flat[off:off + sz])
        off += sz
    w0 = _ptr_array([ws[0] for ws, _ in entries])
    w1 = _ptr_array([ws[1] if len(ws) > 1 else None for ws, _ in entries])
    po = _ptr_array(outs)
    ia = lambda vals: (ctypes.c_int * n)(*[int(v) for v in vals])   # noqa: E731
    a_cout, a_cin, a_ks = ia(couts), ia(cins), ia(kss)
    a_mode = ia([m for _, m in entries])
    a_split = ia([ws[0].shape[0] if len(ws) > 1 else co for (ws, _), co in zip(entries, couts)])
    if x6:
        assert all(len(ws) <= 4 for ws, _ in entries)
        w2 = _ptr_array([ws[2] if len(ws) > 2 else None for ws, _ in entries])
        w3 = _ptr_array([ws[3] if len(ws) > 3 else None for ws, _ in entries])
        cum = lambda ws, k: sum(w.shape[0] for w in ws[:k])   # noqa: E731
        a_split2 = ia([cum(ws, 2) if len(ws) > 2 else co for (ws, _), co in zip(entries, couts)])
        a_split3 = ia([cum(ws, 3) if len(ws) > 3 else co for (ws, _), co in zip(entries, couts)])
        lib.call("ssn_conv_x6_pack_weights_multi", n, ctypes.addressof(w0), ctypes.addressof(w1), ctypes.addressof(w2),
                 ctypes.addressof(w3), ctypes.addressof(po), ctypes.addressof(a_cout), ctypes.addressof(a_cin),
                 ctypes.addressof(a_ks), ctypes.addressof(a_mode), ctypes.addressof(a_split), ctypes.addressof(a_split2),
                 ctypes.addressof(a_split3), _stream(lib, first))
    else:
        assert all(len(ws) <= 2 for ws, _ in entries)
        lib.call("ssn_conv_pack_weights_multi", n, ctypes.addressof(w0), ctypes.addressof(w1), ctypes.addressof(po),
                 ctypes.addressof(a_cout), ctypes.addressof(a_cin), ctypes.addressof(a_ks), ctypes.addressof(a_mode),
                 ctypes.addressof(a_split), _stream(lib, first))
    return outs


def conv_fwd(x, w_packed, scale, shift, y, ksize, stride, pad, relu=True, tile_cfg=-1):
    """x, y: ChanSlice.  w_packed: pack_weights(w, transposed=False)."""
    lib = _check(x, w_packed, scale, shift, y)
    h, wd = x.hw
    ho, wo = y.hw
    assert w_packed.numel() >= packed_floats(y.c, x.c, ksize, False)
    lib.call("ssn_conv_bn_relu_fwd", _p(x), _p(w_packed), _p(scale), _p(shift), _p(y), x.n, x.c, h, wd,
             x.img_stride, y.c, ho, wo, y.img_stride, ksize, stride, pad, int(relu), tile_cfg, _amax_out(y),
             _stream(lib, w_packed))


def guard_bytes(cs):
    """Readable bytes in front of a ChanSlice: the channels below it, plus the pad of tensors from `guarded_empty`."""
    base = cs.t.untyped_storage().data_ptr()
    return int(min(cs.ptr - base, 1 << 20)) if base else 0


def guarded_empty(shape, device, guard_floats=64):
    """torch.empty with `guard_floats` readable floats in front of element 0 (see ssn_conv_x6_fwd: x_guard_bytes)."""
    n = 1
    for d in shape:
        n *= int(d)
    flat = torch.empty(n + guard_floats, device=device, dtype=torch.float32)
    return flat[guard_floats:].view(*shape)


def conv_x6_fwd(x, w_packed, scale, shift, y, ksize, stride, pad, relu=True, tile_cfg=-1, raw_from=0, row_split=0, row_gap=0):
    """conv_fwd on the f16 matrix cores (2-way split, fp32-class accuracy).  w_packed: pack_weights_multi(x6=True).
    raw_from > 0: output channels >= raw_from take neither the affine nor the ReLU.  row_gap > 0: output channels >= row_split
    are stored row_gap channels further up y's tensor (y: the ChanSlice of the first row_split channels' home)."""
    lib = _check(x, w_packed, scale, shift, y)
    h, wd = x.hw
    ho, wo = y.hw
    assert w_packed.numel() >= packed_floats(y.c, x.c, ksize, False, True)
    xa = _amax_in(x)
    lib.call("ssn_conv_x6_fwd", _p(x), _p(w_packed), _p(scale), _p(shift), _p(y), x.n, x.c, h, wd,
             x.img_stride, y.c, ho, wo, y.img_stride, ksize, stride, pad, int(relu), guard_bytes(x), tile_cfg,
             _p(xa), _amax_out(y), int(raw_from), int(row_split), int(row_gap),
             _p(_slot_ext(y)) if row_gap else None, _stream(lib, w_packed))


def pack_weights_rect(w):
    """Split + pack one [cout, cin, kh, kw] forward weight for conv_x6_fwd_rect."""
    lib = _check(w)
    cout, cin, kh, kw = w.shape
    out = _pack_alloc(int(lib.cdll.ssn_conv_x6_packed_floats_rect(cout, cin, kh, kw)), w.device)
    lib.call("ssn_conv_x6_pack_weights_rect", _p(w.contiguous()), _p(out), cout, cin, kh, kw, _stream(lib, w))
    return out


def conv_x6_fwd_rect(x, w_packed, scale, shift, y, kh, kw, pad_h, pad_w, relu=True, tile_cfg=-1):
    """Stride-1 forward convolution with kh x kw taps (5x5, 1x7, 7x1, 1x3, 3x1) on the split kernel."""
    lib = _check(x, w_packed, scale, shift, y)
    h, wd = x.hw
    ho, wo = y.hw
    xa = _amax_in(x)
    lib.call("ssn_conv_x6_fwd_rect", _p(x), _p(w_packed), _p(scale), _p(shift), _p(y), x.n, x.c, h, wd,
             x.img_stride, y.c, ho, wo, y.img_stride, kh, kw, pad_h, pad_w, int(relu), guard_bytes(x), tile_cfg,
             _p(xa), _amax_out(y), _stream(lib, w_packed))


def conv_x6_dgrad(dy, wt, dx, ksize, pad, accumulate, tile_cfg=-1, mask_y=None, mask_scale=None, k_split=0, k_gap=0):
    """Stride-1 conv_dgrad on the f16 matrix cores.  wt: pack_weights_multi([... mode 1], x6=True).
    k_gap > 0: channels >= k_split of dy sit k_gap channels further up its tensor (dy.c counts the channels read)."""
    lib = _check(dy, wt, dx, mask_y, mask_scale)
    assert wt.numel() >= packed_floats(dy.c, dx.c, ksize, True, True)
    ho, wo = dy.hw
    h, w = dx.hw
    ga = _amax_in(dy)
    lib.call("ssn_conv_x6_dgrad", _p(dy), _p(wt), _p(dx), dy.n, dy.c, ho, wo, dy.img_stride, dx.c, h, w,
             dx.img_stride, ksize, pad, int(accumulate), _p(mask_y),
             mask_y.img_stride if mask_y is not None else 0, _p(mask_scale), guard_bytes(dy), tile_cfg,
             _p(ga), _amax_out(dx), int(k_split), int(k_gap), _p(_slot_ext(dy)) if k_gap else None, _stream(lib, wt))


def pack_dgrad_s2(w):
    """dgrad operand of a 3x3 / stride-2 / pad-1 conv for conv_x6_dgrad_s2 (four parity-class sections)."""
    lib = _check(w)
    cout, cin = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (3, 3)
    out = _pack_alloc(int(lib.cdll.ssn_conv_x6_dgrad_s2_packed_floats(cout, cin)), w.device)
    lib.call("ssn_conv_x6_pack_dgrad_s2", _p(w.contiguous()), _p(out), cout, cin, _stream(lib, w))
    return out


def pack_dgrad_rect(w):
    """dgrad operand of a stride-1 layer with rectangular taps for conv_x6_dgrad_rect (transposed, taps reversed)."""
    lib = _check(w)
    cout, cin, kh, kw = w.shape
    out = _pack_alloc(int(lib.cdll.ssn_conv_x6_packed_floats_dgrad_rect(cout, cin, kh, kw)), w.device)
    lib.call("ssn_conv_x6_pack_dgrad_rect", _p(w.contiguous()), _p(out), cout, cin, kh, kw, _stream(lib, w))
    return out


def pack_rect_multi(ws, dgrad=False):
    """Rectangular-tap weights [cout, cin, kh, kw] -> their packed operands (views of one flat buffer) in ceil(len / 40) x 3
    launches: forward operands (pack_weights_rect) or, with dgrad, the transposed tap-reversed ones (pack_dgrad_rect)."""
    if not ws:
        return []
    lib = _check(*ws)
    n = len(ws)
    size_fn = lib.cdll.ssn_conv_x6_packed_floats_dgrad_rect if dgrad else lib.cdll.ssn_conv_x6_packed_floats_rect
    sizes = [int(size_fn(*w.shape)) for w in ws]
    flat = _pack_alloc(sum(sizes), ws[0].device)
    outs, off = [], 0
    for sz in sizes:
        outs.append(flat[off:off + sz])
        off += sz
    ws = [w.contiguous() for w in ws]
    ia = lambda vals: (ctypes.c_int * n)(*[int(v) for v in vals])   # noqa: E731
    pw, po = _ptr_array(ws), _ptr_array(outs)
    a_cout, a_cin, a_kh, a_kw = (ia([w.shape[d] for w in ws]) for d in range(4))
    a_mode = ia([2 if dgrad else 0] * n)
    lib.call("ssn_conv_x6_pack_rect_multi", n, ctypes.addressof(pw), ctypes.addressof(po), ctypes.addressof(a_cout),
             ctypes.addressof(a_cin), ctypes.addressof(a_kh), ctypes.addressof(a_kw), ctypes.addressof(a_mode), _stream(lib, ws[0]))
    return outs


def conv_x6_dgrad_rect(dy, wt, dx, kh, kw, pad_h, pad_w, accumulate, tile_cfg=-1, mask_y=None, mask_scale=None):
    """dgrad of a stride-1 same-size layer with kh x kw taps on the f16 matrix cores.  wt: pack_dgrad_rect(w)."""
    lib = _check(dy, wt, dx, mask_y, mask_scale)
    h, w = dx.hw
    assert dy.hw == dx.hw
    ga = _amax_in(dy)
    lib.call("ssn_conv_x6_dgrad_rect", _p(dy), _p(wt), _p(dx), dy.n, dy.c, h, w, dy.img_stride, dx.c, dx.img_stride,
             kh, kw, pad_h, pad_w, int(accumulate), _p(mask_y), mask_y.img_stride if mask_y is not None else 0,
             _p(mask_scale), guard_bytes(dy), tile_cfg, _p(ga), _amax_out(dx), _stream(lib, wt))


def conv_x6_dgrad_s2(dy, wt, dx, accumulate, tile_cfg=-1, mask_y=None, mask_scale=None, pad=1):
    """dgrad of a 3x3 / stride-2 conv on the f16 matrix cores: pad 1 (even input size) or pad 0.  wt: pack_dgrad_s2(w)."""
    lib = _check(dy, wt, dx, mask_y, mask_scale)
    ho, wo = dy.hw
    h, w = dx.hw
    ga = _amax_in(dy)
    lib.call("ssn_conv_x6_dgrad_s2", _p(dy), _p(wt), _p(dx), dy.n, dy.c, ho, wo, dy.img_stride, dx.c, h, w,
             dx.img_stride, int(accumulate), _p(mask_y), mask_y.img_stride if mask_y is not None else 0,
             _p(mask_scale), guard_bytes(dy), tile_cfg, _p(ga), _amax_out(dx), int(pad), _stream(lib, wt))


def relu_bn_bwd(dy, y, scale):
    """In place: dy <- dy * (y > 0) * scale[c].  dy, y: ChanSlice with equal channel counts."""
    lib = _check(dy, y, scale)
    h, w = y.hw
    lib.call("ssn_relu_bn_bwd", _p(dy), _p(y), _p(scale), y.n, y.c, h * w, dy.img_stride, y.img_stride,
             _amax_out(dy), _stream(lib, scale))


def conv_dgrad(dy, wt, dx, ksize, stride, pad, accumulate, tile_cfg=-1, mask_y=None, mask_scale=None, wt_layout=1):
    """dy: ChanSlice (grad of conv output), dx: ChanSlice (grad of conv input), wt: pack_weights(w, True).

    mask_y (ChanSlice like dx) + mask_scale [dx.c]: fuse the ReLU+frozen-BN backward of dx's tensor into the store.
    """
    lib = _check(dy, wt, dx, mask_y, mask_scale)
    assert wt.numel() >= packed_floats(dy.c, dx.c, ksize, True)
    ho, wo = dy.hw
    h, w = dx.hw
    lib.call("ssn_conv_dgrad", _p(dy), _p(wt), _p(dx), dy.n, dy.c, ho, wo, dy.img_stride, dx.c, h, w,
             dx.img_stride, ksize, stride, pad, int(accumulate), _p(mask_y),
             mask_y.img_stride if mask_y is not None else 0, _p(mask_scale), int(wt_layout), tile_cfg,
             _amax_out(dx), _stream(lib, wt))


def wgrad_workspace_bytes(n, cin, cout, ho, wo, ksize, tile_cfg=-1):
    return _lib.get_lib().wgrad_workspace_bytes(n, cin, cout, ho, wo, ksize, tile_cfg)


def conv_wgrad(g, x, dw, db, ksize, stride, pad, workspace, tile_cfg=-1):
    """g: ChanSlice (masked grad of conv output), x: ChanSlice (conv input); dw [Cout,Cin,k,k], db [Cout] or None."""
    lib = _check(g, x, dw, db, workspace)
    ho, wo = g.hw
    h, w = x.hw
    lib.call("ssn_conv_wgrad", _p(g), _p(x), _p(dw), _p(db), x.n, x.c, h, w, x.img_stride, g.c, ho, wo,
             g.img_stride, ksize, stride, pad, _p(workspace), workspace.numel() * workspace.element_size(),
             tile_cfg, _stream(lib, dw))


def wgrad_x6_supported(ksize, stride, pad, h, w, guard_bytes=256):
    """Layers the x6 weight-gradient kernel takes (the others stay on the exact-f32 kernel); guard_bytes: the readable bytes
    in front of the layer's input."""
    return ksize in (1, 3) and stride == 1 and 2 * pad == ksize - 1 and (pad * w + pad) * 4 <= guard_bytes


def space_to_depth2(x, guard_floats=256):
    """x [N, C, H, W] -> xs [N, 4C, H/2, W/2] (tracked: amax slot attached; `guard_floats` readable floats in front)."""
    lib = _check(x)
    n, c, h, w = x.shape
    xs = attach_amax(guarded_empty((n, 4 * c, h // 2, w // 2), x.device, guard_floats))
    lib.call("ssn_space_to_depth2", _p(x), _p(xs), n, c, h, w, _amax_out(xs), _stream(lib, x))
    return xs


def s2d_weights(w):
    """[Cout, C, k, k] (k odd, stride-2 layer) -> [Cout, 4C, (k+1)/2, (k+1)/2] for the space-to-depth input."""
    lib = _check(w)
    cout, c, k, _ = w.shape
    # (inside a PackBatch the result is an operand of a recorded packing call: it gets a persistent buffer like the packed ones)
    w2 = _pack_alloc(cout * 4 * c * ((k + 1) // 2) ** 2, w.device).view(cout, 4 * c, (k + 1) // 2, (k + 1) // 2)
    lib.call("ssn_s2d_weights", _p(w.contiguous()), _p(w2), cout, c, k, _stream(lib, w))
    return w2


def s2d_weights_bwd(dw2, dw):
    """Gradient of s2d_weights: gathers dw [Cout, C, k, k] out of dw2 [Cout, 4C, (k+1)/2, (k+1)/2]."""
    lib = _check(dw2, dw)
    cout, c, k, _ = dw.shape
    lib.call("ssn_s2d_weights_bwd", _p(dw2), _p(dw), cout, c, k, _stream(lib, dw))


def wgrad_x6_workspace_bytes(n, cin, cout, h, w, ksize, tile_cfg=-1):
    return int(_lib.get_lib().cdll.ssn_conv_wgrad_x6_workspace_bytes(n, cin, cout, h, w, ksize, tile_cfg))


def conv_wgrad_x6(g, x, dw, db, ksize, pad, workspace, tile_cfg=-1, g_row_split=0, g_row_gap=0):
    """conv_wgrad on the f16 matrix cores (stride 1, same size).  x needs >= 256 readable bytes in front of it.
    g_row_gap > 0: rows >= g_row_split of g sit g_row_gap channels further up its tensor (g.c counts the rows read)."""
    lib = _check(g, x, dw, db, workspace)
    h, w = x.hw
    assert g.hw == x.hw
    ga, xa = _amax_in(g), _amax_in(x)
    lib.call("ssn_conv_wgrad_x6", _p(g), _p(x), _p(dw), _p(db), x.n, x.c, h, w, x.img_stride, g.c, g.img_stride,
             ksize, pad, guard_bytes(x), _p(workspace), workspace.numel() * workspace.element_size(), tile_cfg,
             _p(ga), _p(xa), int(g_row_split), int(g_row_gap), _p(_slot_ext(g)) if g_row_gap else None, _stream(lib, dw))


def wgrad_x6_rect_workspace_bytes(n, cin, cout, h, w, kh, kw, tile_cfg=-1):
    return int(_lib.get_lib().cdll.ssn_conv_wgrad_x6_rect_workspace_bytes(n, cin, cout, h, w, kh, kw, tile_cfg))


def wgrad_x6_rect_guard_floats(pad_h, pad_w, w):
    """Readable floats conv_wgrad_x6_rect needs in front of x (the taps in front of a pixel reach that far)."""
    return max(64, ((pad_h * w + pad_w) * 4 + 255) // 256 * 64)


def conv_wgrad_x6_rect(g, x, dw, db, kh, kw, pad_h, pad_w, workspace, tile_cfg=-1):
    """conv_wgrad of a stride-1 same-size layer with kh x kw taps on the f16 matrix cores; dw [Cout, Cin, kh, kw]."""
    lib = _check(g, x, dw, db, workspace)
    h, w = x.hw
    assert g.hw == x.hw
    ga, xa = _amax_in(g), _amax_in(x)
    lib.call("ssn_conv_wgrad_x6_rect", _p(g), _p(x), _p(dw), _p(db), x.n, x.c, h, w, x.img_stride, g.c, g.img_stride,
             kh, kw, pad_h, pad_w, guard_bytes(x), _p(workspace), workspace.numel() * workspace.element_size(), tile_cfg,
             _p(ga), _p(xa), _stream(lib, dw))


def pool_fwd(kind, x, y, argmax, ksize, stride, pad):
    lib = _check(x, y, argmax)
    h, w = x.hw
    ho, wo = y.hw
    lib.call("ssn_pool_fwd", int(kind == "max"), _p(x), _p(y), _p(argmax), x.n, x.c, h, w, x.img_stride, ho, wo,
             y.img_stride, ksize, stride, pad, _amax_out(y), _stream(lib, x))


def pool_bwd(kind, dy, argmax, dx, ksize, stride, pad, accumulate, mask_y=None, mask_scale=None):
    lib = _check(dy, dx, argmax, mask_y, mask_scale)
    h, w = dx.hw
    ho, wo = dy.hw
    lib.call("ssn_pool_bwd", int(kind == "max"), _p(dy), _p(argmax), _p(dx), dx.n, dx.c, h, w, dx.img_stride, ho,
             wo, dy.img_stride, ksize, stride, pad, int(accumulate), _p(mask_y),
             mask_y.img_stride if mask_y is not None else 0, _p(mask_scale), _amax_out(dx), _stream(lib, dx))


def avgpool_affine_fwd(x, y, scale, shift, relu, ksize, stride, pad):
    """y = relu?(scale[c] * avgpool(x) + shift[c]) on ChanSlices (see ssn_avgpool_affine_fwd)."""
    lib = _check(x, y, scale, shift)
    h, w = x.hw
    ho, wo = y.hw
    lib.call("ssn_avgpool_affine_fwd", _p(x), _p(y), _p(scale), _p(shift), int(bool(relu)), x.n, x.c, h, w,
             x.img_stride, ho, wo, y.img_stride, ksize, stride, pad, _amax_out(y), _stream(lib, y))


def channel_sum_workspace_bytes(n, c):
    return 4 * c * int(_lib.get_lib().cdll.ssn_channel_sum_shares(n))


def channel_sum(g, out, workspace):
    """out[c] = sum over images and pixels of the ChanSlice g (two passes through `workspace`, fixed order)."""
    lib = _check(g, out, workspace)
    h, w = g.hw
    lib.call("ssn_channel_sum", _p(g), _p(out), g.n, g.c, h * w, g.img_stride, _p(workspace),
             workspace.numel() * workspace.element_size(), _stream(lib, out))


def bn_train_workspace_floats(n, c):
    fn = _lib.get_lib().cdll.ssn_bn_train_workspace_floats
    fn.restype = ctypes.c_long
    return int(fn(int(n), int(c)))


def bn_train_stats(z, conv_bias, mean, invstd, running_mean, running_var, eps, momentum, workspace):
    """Batch statistics of the ChanSlice z (the convolution WITHOUT its bias) + running-statistics update."""
    global PARAM_EPOCH
    PARAM_EPOCH += 1        # (the running statistics are written through raw pointers)
    lib = _check(z, conv_bias, mean, invstd, running_mean, running_var, workspace)
    h, w = z.hw
    lib.call("ssn_bn_train_stats", _p(z), _p(conv_bias), _p(mean), _p(invstd), _p(running_mean), _p(running_var), z.n,
             z.c, h * w, z.img_stride, float(eps), float(momentum), _p(workspace),
             workspace.numel() * workspace.element_size(), _stream(lib, mean))


def bn_train_apply(z, y, mean, invstd, gamma, beta, relu=True):
    """y = relu?(gamma * (z - mean) * invstd + beta) on ChanSlices."""
    lib = _check(z, y, mean, invstd, gamma, beta)
    h, w = z.hw
    lib.call("ssn_bn_train_apply", _p(z), _p(y), _p(mean), _p(invstd), _p(gamma), _p(beta), int(bool(relu)), z.n, z.c,
             h * w, z.img_stride, y.img_stride, _amax_out(y), _stream(lib, mean))


def bn_train_bwd(dy, y, z, mean, invstd, gamma, dgamma, dbeta, dz, workspace, relu=True):
    """Backward of bn_train_apply(bn_train_stats(z)): dgamma, dbeta [C] and dz (ChanSlice)."""
    lib = _check(dy, y, z, mean, invstd, gamma, dgamma, dbeta, dz, workspace)
    h, w = z.hw
    lib.call("ssn_bn_train_bwd", _p(dy), _p(y), _p(z), _p(mean), _p(invstd), _p(gamma), _p(dgamma), _p(dbeta), _p(dz),
             int(bool(relu)), z.n, z.c, h * w, dy.img_stride, y.img_stride, z.img_stride, dz.img_stride, _p(workspace),
             workspace.numel() * workspace.element_size(), _amax_out(dz), _stream(lib, mean))


@_hbm_timed
def gap_fwd(x, y):
    lib = _check(x, y)
    h, w = x.hw
    lib.call("ssn_global_avgpool_fwd", _p(x), _p(y), x.n, x.c, h * w, x.img_stride, _stream(lib, y))


@_hbm_timed
def gap_bwd(dy, dx, accumulate=False):
    lib = _check(dy, dx)
    h, w = dx.hw
    lib.call("ssn_global_avgpool_bwd", _p(dy), _p(dx), dx.n, dx.c, h * w, dx.img_stride, int(accumulate),
             _amax_out(dx), _stream(lib, dy))


@_hbm_timed
def dropout_fwd(x, y, mask, p, seed, counter=None):
    """counter: optional int64[1] device tensor; it is mixed into the Philox key and incremented by the call."""
    lib = _check(x, y, mask, counter)
    lib.call("ssn_dropout_fwd", _p(x), _p(y), _p(mask), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
             _p(counter), _stream(lib, x))


@_hbm_timed
def dropout_bwd(dy, mask, dx, p):
    lib = _check(dy, mask, dx)
    lib.call("ssn_dropout_bwd", _p(dy), _p(mask), _p(dx), dy.numel(), float(p), _stream(lib, dy))


# ------------------------------------------------------------------------------------ STPP / heads / losses
def make_stpp_table(parts, n_seg, act_lo, act_hi):
    """parts: list of (lo, hi, norm, col)."""
    if len(parts) > STPP_MAX_PARTS:
        raise ValueError("STPP config has %d parts (max %d)" % (len(parts), STPP_MAX_PARTS))
    t = SsnStppTable()
    t.n_parts, t.n_seg, t.act_lo, t.act_hi = len(parts), n_seg, act_lo, act_hi
    for i, (lo, hi, norm, col) in enumerate(parts):
        t.lo[i], t.hi[i], t.norm[i], t.col[i] = lo, hi, norm, col
    return t


@_hbm_timed
def stpp_fwd(ft, scaling, act_ft, stpp_ft, table):
    lib = _check(ft, scaling, act_ft, stpp_ft)
    lib.call("ssn_stpp_fwd", _p(ft), _p(scaling), _p(act_ft), _p(stpp_ft), act_ft.shape[0], ft.shape[1],
             ctypes.addressof(table), _stream(lib, ft))


@_hbm_timed
def stpp_bwd(d_act, d_stpp, scaling, d_ft, table):
    lib = _check(d_act, d_stpp, scaling, d_ft)
    lib.call("ssn_stpp_bwd", _p(d_act), _p(d_stpp), _p(scaling), _p(d_ft), d_stpp.shape[0], d_ft.shape[1],
             ctypes.addressof(table), _stream(lib, d_ft))


def _heads_tables(ws, bs, pos, idx, outs):
    arr3 = ctypes.c_void_p * 3
    ci3 = ctypes.c_int * 3
    return (arr3(*[None if t is None else t.data_ptr() for t in ws]), arr3(*[None if t is None else t.data_ptr() for t in bs]),
            arr3(*[None if t is None else t.data_ptr() for t in pos]), arr3(*[None if t is None else t.data_ptr() for t in idx]),
            arr3(*[None if t is None else t.data_ptr() for t in outs]),
            ci3(*[0 if w is None else int(w.shape[0]) for w in ws]), ci3(*[0 if t is None else int(t.numel()) for t in idx]))


@_hbm_timed
def heads_fwd(ft, scaling, ws, bs, pos, idx, outs, act_ft, stpp_ft, table):
    """STPP + the three Linear heads + the prop_type row selection in one launch (ssn_heads_fwd).  ws / bs / pos / idx / outs:
    lists of 3 (activity, completeness, regression; entries of an absent regression head None)."""
    lib = _check(ft, scaling, act_ft, stpp_ft, *[t for t in list(ws) + list(bs) + list(outs) if t is not None])
    tabs = _heads_tables(ws, bs, pos, idx, outs)
    lib.call("ssn_heads_fwd", _p(ft), _p(scaling), *[ctypes.addressof(t) for t in tabs], _p(act_ft), _p(stpp_ft),
             act_ft.shape[0], ft.shape[1], ctypes.addressof(table), _stream(lib, ft))


@_hbm_timed
def heads_bwd(scaling, ws, bs, pos, idx, douts, act_ft, stpp_ft, table, d_ft, dws, dbs):
    lib = _check(scaling, act_ft, stpp_ft, d_ft, *[t for t in list(ws) + list(douts) + list(dws) + list(dbs) if t is not None])
    tabs = _heads_tables(ws, bs, pos, idx, douts)
    arr3 = ctypes.c_void_p * 3
    pdw = arr3(*[None if t is None else t.data_ptr() for t in dws])
    pdb = arr3(*[None if t is None else t.data_ptr() for t in dbs])
    lib.call("ssn_heads_bwd", None, _p(scaling), *[ctypes.addressof(t) for t in tabs], _p(act_ft), _p(stpp_ft), act_ft.shape[0],
             d_ft.shape[1], ctypes.addressof(table), _p(d_ft), ctypes.addressof(pdw), ctypes.addressof(pdb), _stream(lib, d_ft))


def stpp_reorg(scores, ranges, act_range, scaling, part_scale_col, act_len, comp_len, reg_len, out_act, out_comp,
               out_reg):
    lib = _check(ranges, act_range, scaling, part_scale_col, out_act, out_comp, out_reg)
    # scores: [T, D], or a column range of one (rows D_total apart): the kernel addresses row r at r * (row stride)
    assert scores.dim() == 2 and scores.stride(1) == 1 and scores.dtype == torch.float32
    assert scores.stride(0) >= act_len + ranges.shape[1] * (comp_len + (reg_len if out_reg is not None else 0))
    lib.call("ssn_stpp_reorg", _p(scores), scores.shape[0], scores.stride(0), _p(ranges), _p(act_range),
             _p(scaling), _p(part_scale_col), ranges.shape[0], ranges.shape[1], act_len, comp_len, reg_len,
             _p(out_act), _p(out_comp), _p(out_reg), _stream(lib, scores))


def crop_mean(x, num_crop, out):
    """x [num_crop * T, D] (crop-major) -> out [T, D] = mean over the crops (ssn_test.py:85)."""
    lib = _check(x, out)
    t = out.shape[0]
    assert x.shape[0] == num_crop * t and x.shape[1] == out.shape[1]
    lib.call("ssn_crop_mean", _p(x), _p(out), num_crop, t, out.shape[1], _stream(lib, x))


def reg_denorm(reg, mean0, std0, mean1, std1):
    """reg [..., 2] in place: reg[..., k] * std[k] + mean[k] (ssn_test.py:88-90)."""
    lib = _check(reg)
    assert reg.shape[-1] == 2 and reg.is_contiguous()
    lib.call("ssn_reg_denorm", _p(reg), reg.numel() // 2, float(mean0), float(std0), float(mean1), float(std1),
             _stream(lib, reg))


def frames_crop_normalize(src, dst, crops, roll, invert_even, mean, std):
    """src uint8 [n_img, Hs, Ws, C] -> dst fp32 [n_crops, n_img, C, ch, cw]; crops = [(off_x, off_y, flip), ...];
    mean / std: device float tensors (repeat over the stacked channels like GroupNormalize)."""
    import ctypes
    lib = _check(src, dst, mean, std)
    assert src.dtype == torch.uint8 and src.dim() == 4 and dst.dim() == 5 and src.is_contiguous() and dst.is_contiguous()
    n_img, hs, ws, c = src.shape
    nc, _, _, ch, cw = dst.shape
    assert nc == len(crops) and dst.shape[1] == n_img and dst.shape[2] == c
    arr = ctypes.c_int * nc
    ox, oy, fl = arr(*[int(t[0]) for t in crops]), arr(*[int(t[1]) for t in crops]), arr(*[int(bool(t[2])) for t in crops])
    lib.call("ssn_frames_crop_normalize", _p(src), _p(dst), n_img, hs, ws, c, ch, cw, nc,
             ctypes.cast(ox, ctypes.c_void_p), ctypes.cast(oy, ctypes.c_void_p), ctypes.cast(fl, ctypes.c_void_p),
             int(roll), int(invert_even), _p(mean), mean.numel(), _p(std), std.numel(), _stream(lib, src))


def frames_crop_resize_normalize(src, boxes, flips, out_hw, roll, invert_even, mean, std, dst=None):
    """The training augmentation in two launches (ssn_frames_crop_resize_normalize): src uint8 [n_img, Hs, Ws, C] decoded frames
    -> fp32 [n_img, C, out_h, out_w] = normalise(roll(flip(PIL-bilinear-resize(crop)))).  boxes: [n_img, 4] ints (x0, y0, crop_w,
    crop_h) -- host list / array (validated and uploaded here) or a device int32 tensor the caller vouches for; flips likewise."""
    lib = _check(src, mean, std)
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.is_contiguous()
    n_img, hs, ws, c = src.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if not torch.is_tensor(boxes):
        import numpy as np
        b = np.asarray(boxes, dtype=np.int64).reshape(n_img, 4)
        if (b[:, 0] < 0).any() or (b[:, 1] < 0).any() or (b[:, 2] < 1).any() or (b[:, 3] < 1).any() \
                or (b[:, 0] + b[:, 2] > ws).any() or (b[:, 1] + b[:, 3] > hs).any():
            raise ValueError("crop box outside the %dx%d frame" % (ws, hs))
        if (b[:, 2] > 3 * ow).any() or (b[:, 3] > 3 * oh).any():
            raise ValueError("crop more than 3x the output size (the resize kernel holds 7 taps per axis)")
        boxes = torch.from_numpy(b.astype(np.int32)).to(src.device)
    if not torch.is_tensor(flips):
        flips = torch.tensor([int(bool(f)) for f in flips], dtype=torch.int32).to(src.device)
    assert boxes.dtype == torch.int32 and flips.dtype == torch.int32 and boxes.numel() == 4 * n_img and flips.numel() == n_img
    if dst is None:
        dst = torch.empty((n_img, c, oh, ow), device=src.device, dtype=torch.float32)
    ws_bytes = int(lib.cdll.ssn_frames_resize_workspace_bytes(n_img, oh, ow))
    wsp = torch.empty(max(ws_bytes, 4) // 4, device=src.device, dtype=torch.int32)
    lib.call("ssn_frames_crop_resize_normalize", _p(src), _p(dst), n_img, hs, ws, c, oh, ow, _p(boxes), _p(flips), int(roll),
             int(invert_even), _p(mean), mean.numel(), _p(std), std.numel(), _p(wsp), ws_bytes, _stream(lib, src))
    return dst


FRAMES_SCALE_MAX_RATIO = 6      # csrc/frames.hip: 13 taps per axis


def frames_scale_supported(hs, ws, oh, ow):
    """What ssn_frames_scale takes: the axis with the smaller in / out ratio (the side GroupScale sets) shrinks by at most 6; the other
    one, whose length GroupScale truncates to an integer, stays below the 13-tap capacity (ratio 6.5)."""
    r = FRAMES_SCALE_MAX_RATIO
    return (hs <= r * oh or ws <= r * ow) and 2 * hs < (2 * r + 1) * oh and 2 * ws < (2 * r + 1) * ow


def frames_scale(src, out_hw, dst=None):
    """GroupScale's resize of whole frames (ssn_frames_scale): src uint8 [n_img, Hs, Ws, C], C = 1 or 3, -> uint8 [n_img, out_h, out_w, C],
    bit-identical to ``img.resize((out_w, out_h), Image.BILINEAR)``.  ValueError (nothing launched) beyond the kernel's ratio of 6."""
    if src.dtype != torch.uint8 or src.dim() != 4:
        raise ValueError("frames_scale: uint8 [n_img, H, W, C]")
    src = src.contiguous()
    lib = _check(src)
    n_img, hs, ws, c = src.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if oh < 1 or ow < 1:
        raise ValueError("frames_scale: empty output %d x %d" % (ow, oh))
    if not frames_scale_supported(hs, ws, oh, ow):
        raise ValueError("frames_scale: %d x %d -> %d x %d shrinks by more than %d" % (ws, hs, ow, oh, FRAMES_SCALE_MAX_RATIO))
    if dst is None:
        dst = torch.empty((n_img, oh, ow, c), device=src.device, dtype=torch.uint8)
    assert dst.dtype == torch.uint8 and tuple(dst.shape) == (n_img, oh, ow, c) and dst.is_contiguous() and dst.device == src.device
    ws_bytes = int(lib.cdll.ssn_frames_scale_workspace_bytes(oh, ow))
    wsp = torch.empty(ws_bytes // 4, device=src.device, dtype=torch.int32)
    lib.call("ssn_frames_scale", _p(src), _p(dst), n_img, hs, ws, c, oh, ow, _p(wsp), ws_bytes, _stream(lib, src))
    return dst


def frame_diff(x, new_length, channels=3):
    """RGBDiff input (SSN._get_diff): x [..., (new_length + 1) * channels * k, H, W] stacked frames per segment ->
    [n_segments, new_length * channels, H, W] differences of consecutive frames."""
    lib = _check(x)
    h, w = x.shape[-2:]
    per_in = (new_length + 1) * channels
    assert x.numel() % (per_in * h * w) == 0
    n_seg = x.numel() // (per_in * h * w)
    out = torch.empty((n_seg, new_length * channels, h, w), device=x.device, dtype=torch.float32)
    lib.call("ssn_frame_diff", _p(x), _p(out), n_seg, int(new_length), int(channels), h * w, _stream(lib, x))
    return out


def detections(act, comp, reg, rel_prop, top_k, include_bg, nms_thresh, regress):
    """One video: -> (combined [P, C] fp32, dets [C, max_det, 5] fp64, counts [C] int32).  See ssn_detections
    (include_bg: 0 softmax over the class scores, 1 / True over all C + 1 scores, 2 no softmax)."""
    lib = _check(act, comp, reg, rel_prop)
    p, c = comp.shape
    assert act.shape == (p, c + 1) and rel_prop.shape == (p, 2) and rel_prop.dtype == torch.float64
    dev = act.device
    max_det = max(1, p)
    combined = torch.empty((p, c), device=dev, dtype=torch.float32)
    dets = torch.zeros((c, max_det, 5), device=dev, dtype=torch.float64)
    counts = torch.zeros(c, device=dev, dtype=torch.int32)
    ws_bytes = int(lib.cdll.ssn_detections_workspace_bytes(p, c))
    ws = torch.zeros((ws_bytes + 3) // 4, device=dev, dtype=torch.int32)
    lib.call("ssn_detections", _p(act), _p(comp), _p(reg), _p(rel_prop), _p(combined), _p(dets), _p(counts), _p(ws),
             ws_bytes, p, c, max_det, int(top_k), int(include_bg), float(nms_thresh), int(bool(regress)),
             _stream(lib, act))
    return combined, dets, counts


def detections_batch_check_sizes(total_p, v, c):
    """The size limit of the batched path, on shapes alone (before anything is concatenated or allocated)."""
    if int(total_p) * int(c) >= 2 ** 31 or int(v) * int(c) >= 2 ** 31:
        raise ValueError("detections_batch: %d proposals of %d videos x %d classes do not fit int32 indices, split the batch"
                         % (total_p, v, c))


def detections_batch(act, comp, rel_prop, h_p_off, d_p_off, report, top_k, include_bg, nms_thresh):
    """All videos of a batch, stages scores / select / nms / offsets (ssn_detections_batch): act [total_p, C + 1], comp
    [total_p, C] fp32, rel_prop [total_p, 2] fp64, h_p_off / d_p_off [V + 1] int32 (host / device copy), report [V, C] uint8
    or None -> (combined [total_p, C] fp32, kept [total_p * C] int32, row_off [V * C + 1] int32), all on the device."""
    lib = _check(act, comp, rel_prop, d_p_off, report)
    total_p, c = comp.shape
    if h_p_off.is_cuda or h_p_off.dtype != torch.int32 or d_p_off.dtype != torch.int32 or h_p_off.dim() != 1 \
            or h_p_off.shape != d_p_off.shape or h_p_off.numel() < 2 or not h_p_off.is_contiguous():
        raise ValueError("detections_batch: offsets must be int32 [V + 1], once on the host and once on the device")
    v = h_p_off.numel() - 1
    if c < 1 or act.shape != (total_p, c + 1) or rel_prop.shape != (total_p, 2) or rel_prop.dtype != torch.float64 \
            or act.dtype != torch.float32 or comp.dtype != torch.float32 or int(h_p_off[-1]) != total_p:
        raise ValueError("detections_batch: act must be float32 [P, C + 1], comp float32 [P, C], rel_prop float64 [P, 2], "
                         "P the last offset")
    if report is not None and (report.shape != (v, c) or report.dtype != torch.uint8):
        raise ValueError("detections_batch: report must be uint8 [V, C]")
    detections_batch_check_sizes(total_p, v, c)
    dev = comp.device
    # workspace entries of the videos whose candidates do not fit in LDS (host arithmetic on the offsets alone)
    sizes = (h_p_off[1:] - h_p_off[:-1]).to(torch.int64)
    pow2 = torch.ones_like(sizes)
    while bool((pow2 < sizes).any()):
        pow2 = torch.where(pow2 < sizes, pow2 * 2, pow2)
    big_off = torch.zeros(v + 1, dtype=torch.int64)
    big_off[1:] = torch.cumsum(torch.where(sizes > 2048, pow2 * c, torch.zeros_like(sizes)), 0)
    big_entries = int(big_off[-1])
    combined = torch.empty((total_p, c), device=dev, dtype=torch.float32)
    kept = torch.empty(total_p * c, device=dev, dtype=torch.int32)
    counts = torch.empty(v * c, device=dev, dtype=torch.int32)
    row_off = torch.empty(v * c + 1, device=dev, dtype=torch.int32)
    ws_bytes = int(lib.cdll.ssn_detections_batch_workspace_bytes(v, big_entries))
    ws = torch.empty((ws_bytes + 3) // 4, device=dev, dtype=torch.int32)
    lib.call("ssn_detections_batch", _p(act) if total_p else None, _p(comp) if total_p else None,
             _p(rel_prop) if total_p else None, h_p_off.data_ptr(), _p(d_p_off), _p(report), _p(big_off.to(dev)), big_entries,
             v, c, int(top_k), int(include_bg), float(nms_thresh), _p(combined) if total_p else None,
             _p(kept) if total_p else None, _p(counts), _p(row_off), _p(ws), ws_bytes, _stream(lib, comp))
    return combined, kept, row_off


def detections_batch_fill(rel_prop, combined, reg, d_p_off, kept, row_off, n, regress):
    """Stage fill (ssn_detections_batch_fill) for the n = row_off[-1] kept rows: -> rows [n, 5] fp64 (start, end, score, loc,
    dur), cls, vid, prop [n] int32 on the device."""
    lib = _check(rel_prop, combined, reg, d_p_off, kept, row_off)
    total_p, c = combined.shape
    v = d_p_off.numel() - 1
    if reg is not None and (reg.shape != (total_p, c, 2) or reg.dtype != torch.float32):
        raise ValueError("detections_batch_fill: reg must be float32 [P, C, 2]")
    if row_off.shape != (v * c + 1,) or kept.shape != (total_p * c,) or rel_prop.shape != (total_p, 2):
        raise ValueError("detections_batch_fill: tables of another batch")
    dev = combined.device
    n = int(n)
    rows = torch.empty((n, 5), device=dev, dtype=torch.float64)
    cls = torch.empty(n, device=dev, dtype=torch.int32)
    vid = torch.empty(n, device=dev, dtype=torch.int32)
    prop = torch.empty(n, device=dev, dtype=torch.int32)
    lib.call("ssn_detections_batch_fill", _p(rel_prop) if n else None, _p(combined) if n else None,
             _p(reg) if (n and reg is not None) else None, _p(d_p_off), _p(kept) if n else None, _p(row_off), v, c, total_p, n,
             int(bool(regress)), _p(rows) if n else None, _p(cls) if n else None, _p(vid) if n else None,
             _p(prop) if n else None, _stream(lib, combined))
    return rows, cls, vid, prop


def tag_count(scores, h_offsets, d_offsets, thresholds, bw, want_labels=False):
    """Counting phase of ssn_tag_count for a batch of videos: scores [N, 2] fp32 (the videos one after the other),
    h_offsets / d_offsets [V + 1] int32 (host / device copy), thresholds [n_thr] fp32 ->
    (smoothed [N] fp32, labels [n_thr, N] uint8 or None, runs [V, n_thr] int32)."""
    lib = _check(scores, d_offsets, thresholds)
    if scores.dim() != 2 or scores.shape[1] != 2 or scores.dtype != torch.float32:
        raise ValueError("tag_count: scores must be float32 [N, 2], got %s %s" % (scores.dtype, tuple(scores.shape)))
    if h_offsets.is_cuda or h_offsets.dtype != torch.int32 or d_offsets.dtype != torch.int32 or h_offsets.dim() != 1 \
            or h_offsets.shape != d_offsets.shape or h_offsets.numel() < 2 or not h_offsets.is_contiguous():
        raise ValueError("tag_count: offsets must be int32 [V + 1], once on the host and once on the device")
    if thresholds.dim() != 1 or thresholds.dtype != torch.float32 or thresholds.numel() < 1:
        raise ValueError("tag_count: thresholds must be float32 [n_thr]")
    n, v, n_thr = scores.shape[0], h_offsets.numel() - 1, thresholds.numel()
    dev = scores.device
    prob = torch.empty(n, device=dev, dtype=torch.float32)
    smoothed = torch.empty(n, device=dev, dtype=torch.float32)
    labels = torch.zeros((n_thr, n), device=dev, dtype=torch.uint8) if want_labels else None
    runs = torch.zeros((v, n_thr), device=dev, dtype=torch.int32)
    lib.call("ssn_tag_count", _p(scores), h_offsets.data_ptr(), _p(d_offsets), v, n, _p(thresholds), n_thr, float(bw),
             _p(prob), _p(smoothed), _p(labels), _p(runs), _stream(lib, scores))
    return smoothed, labels, runs


def tag_lds_candidates():
    return int(_lib.get_lib().cdll.ssn_tag_lds_candidates())


def tag_generate(scores, smoothed, d_offsets, durations, thresholds, tolerances, run_off, sort_off, total_runs, sort_entries,
                 nms_thresh, minimum_len):
    """Generating phase (ssn_tag_generate).  run_off [V * n_thr + 1] int32 and sort_off [V + 1] int64 on the device, their
    last entries as total_runs / sort_entries.  -> dict of device tensors indexed like the candidates (cand_box [C, 2],
    cand_score [C], kept_box [C, 2], kept_score [C], seconds [C, 2], longer [C]) and kept_count [V]."""
    lib = _check(scores, smoothed, d_offsets, durations, thresholds, tolerances, run_off, sort_off)
    v, n_thr, n_tol = d_offsets.numel() - 1, thresholds.numel(), tolerances.numel()
    n = scores.shape[0]
    if scores.dim() != 2 or scores.shape[1] != 2 or scores.dtype != torch.float32 or smoothed.shape != (n,) \
            or smoothed.dtype != torch.float32:
        raise ValueError("tag_generate: scores must be float32 [N, 2] and smoothed float32 [N]")
    if d_offsets.dim() != 1 or d_offsets.dtype != torch.int32 or v < 1 or thresholds.dim() != 1 \
            or thresholds.dtype != torch.float32 or tolerances.dim() != 1:
        raise ValueError("tag_generate: offsets must be int32 [V + 1], thresholds float32 [n_thr], tolerances [n_tol]")
    if durations.shape != (v,) or durations.dtype != torch.float64 or tolerances.dtype != torch.float64:
        raise ValueError("tag_generate: durations must be float64 [V] and tolerances float64")
    if run_off.shape != (v * n_thr + 1,) or run_off.dtype != torch.int32 or sort_off.shape != (v + 1,) \
            or sort_off.dtype != torch.int64:
        raise ValueError("tag_generate: run_off must be int32 [V * n_thr + 1] and sort_off int64 [V + 1]")
    dev = scores.device
    c = 2 * n_tol * int(total_runs)
    out = {"cand_box": torch.zeros((c, 2), device=dev, dtype=torch.int32),
           "cand_score": torch.zeros(c, device=dev, dtype=torch.float32),
           "kept_box": torch.zeros((c, 2), device=dev, dtype=torch.int32),
           "kept_score": torch.zeros(c, device=dev, dtype=torch.float32),
           "seconds": torch.zeros((c, 2), device=dev, dtype=torch.float64),
           "longer": torch.zeros(c, device=dev, dtype=torch.uint8),
           "kept_count": torch.zeros(v, device=dev, dtype=torch.int32)}
    ws_bytes = int(lib.cdll.ssn_tag_workspace_bytes(int(total_runs), int(sort_entries)))
    ws = torch.zeros((ws_bytes + 3) // 4, device=dev, dtype=torch.int32)
    lib.call("ssn_tag_generate", _p(scores), _p(smoothed), _p(d_offsets), _p(durations), v, scores.shape[0], _p(thresholds),
             n_thr, _p(tolerances), n_tol, _p(run_off), _p(sort_off), int(total_runs), int(sort_entries), float(nms_thresh),
             float(minimum_len), _p(out["cand_box"]), _p(out["cand_score"]), _p(out["kept_box"]), _p(out["kept_score"]),
             _p(out["seconds"]), _p(out["longer"]), _p(out["kept_count"]), _p(ws), ws_bytes, _stream(lib, scores))
    return out


def tag_name_proposals(gt_span, gt_label, gt_off, prop, prop_off, thresh=0.0):
    """ssn_tag_name_proposals: gt_span [G, 2] fp64, gt_label [G] int32, gt_off [V + 1] int32, prop [P, 2] fp64, prop_off
    [V + 1] int32 -> (label [P] int32, iou [P] fp64, overlap_self [P] fp64)."""
    lib = _check(gt_span, gt_label, gt_off, prop, prop_off)
    g, p, v = gt_span.shape[0], prop.shape[0], gt_off.numel() - 1
    if gt_span.shape != (g, 2) or gt_span.dtype != torch.float64 or gt_label.shape != (g,) or gt_label.dtype != torch.int32 \
            or prop.shape != (p, 2) or prop.dtype != torch.float64 or gt_off.dtype != torch.int32 \
            or prop_off.dtype != torch.int32 or prop_off.shape != gt_off.shape:
        raise ValueError("tag_name_proposals: bad shapes / dtypes")
    dev = prop.device
    label = torch.zeros(p, device=dev, dtype=torch.int32)
    iou = torch.zeros(p, device=dev, dtype=torch.float64)
    own = torch.zeros(p, device=dev, dtype=torch.float64)
    lib.call("ssn_tag_name_proposals", _p(gt_span) if g else None, _p(gt_label) if g else None, _p(gt_off), g,
             _p(prop) if p else None, _p(prop_off), v, p, float(thresh), _p(label) if p else None, _p(iou) if p else None,
             _p(own) if p else None, _stream(lib, prop))
    return label, iou, own


def eval_lds_gt():
    return int(_lib.get_lib().cdll.ssn_eval_lds_gt())


def eval_count(pred_score, pred_cls, num_class):
    """ssn_eval_count: pred_score [N] fp64, pred_cls [N] int32 -> counts [C + 1] int32 (device): predictions per class,
    and in the last entry the rows that cannot be evaluated (class out of range, score not finite)."""
    lib = _check(pred_score, pred_cls)
    n = pred_score.shape[0]
    if pred_score.shape != (n,) or pred_score.dtype != torch.float64 or pred_cls.shape != (n,) or pred_cls.dtype != torch.int32:
        raise ValueError("eval_count: pred_score must be float64 [N] and pred_cls int32 [N]")
    counts = torch.zeros(int(num_class) + 1, device=pred_score.device, dtype=torch.int32)
    lib.call("ssn_eval_count", _p(pred_score) if n else None, _p(pred_cls) if n else None, n, int(num_class), _p(counts),
             _stream(lib, counts))
    return counts


def eval_ap(pred_seg, pred_score, pred_cls, pred_vid, gt_seg, groups, npos, thresholds, pred_off, sort_off, sort_entries,
            big_units):
    """ssn_eval_ap (see include/ssn_hip.h) -> (order [N] int32, tp [T, N] uint8, ap [C, T] fp64), all on the device."""
    lib = _check(pred_seg, pred_score, pred_cls, pred_vid, gt_seg, groups, npos, thresholds, pred_off, sort_off)
    n, g, ng, c, t = pred_score.shape[0], gt_seg.shape[0], groups.shape[0], npos.shape[0], thresholds.shape[0]
    if pred_seg.shape != (n, 2) or pred_seg.dtype != torch.float64 or pred_score.dtype != torch.float64 \
            or pred_cls.shape != (n,) or pred_cls.dtype != torch.int32 or pred_vid.shape != (n,) or pred_vid.dtype != torch.int32:
        raise ValueError("eval_ap: predictions must be float64 [N, 2] / [N] and int32 [N] class / video")
    if gt_seg.shape != (g, 2) or gt_seg.dtype != torch.float64 or groups.shape != (ng, 5) or groups.dtype != torch.int32 \
            or npos.dtype != torch.int32 or thresholds.dtype != torch.float64 or thresholds.dim() != 1:
        raise ValueError("eval_ap: ground truth must be float64 [G, 2], int32 [NG, 5] groups and int32 [C] counts")
    if pred_off.shape != (c + 1,) or pred_off.dtype != torch.int32 or sort_off.shape != (c + 1,) or sort_off.dtype != torch.int64:
        raise ValueError("eval_ap: pred_off must be int32 [C + 1] and sort_off int64 [C + 1]")
    dev = thresholds.device
    order = torch.zeros(n, device=dev, dtype=torch.int32)
    tp = torch.zeros((t, n), device=dev, dtype=torch.uint8)
    ap = torch.zeros((c, t), device=dev, dtype=torch.float64)
    ws_bytes = int(lib.cdll.ssn_eval_workspace_bytes(int(sort_entries), int(big_units), c))
    ws = torch.zeros((ws_bytes + 7) // 8, device=dev, dtype=torch.int64)
    lib.call("ssn_eval_ap", _p(pred_seg) if n else None, _p(pred_score) if n else None, _p(pred_cls) if n else None,
             _p(pred_vid) if n else None, n, _p(gt_seg) if ng else None, _p(groups) if ng else None, ng, g, _p(npos),
             _p(thresholds), t, c, _p(pred_off), _p(sort_off), int(sort_entries), int(big_units), _p(order) if n else None,
             _p(tp) if n else None, _p(ap), _p(ws), ws_bytes, _stream(lib, thresholds))
    return order, tp, ap


def eval_recall(gt_span, gt_off, prop, prop_off, thresholds):
    """ssn_eval_recall: gt_span [G, 2] fp64, gt_off [V + 1] int32, prop [P, 2] fp64, prop_off [V + 1] int32, thresholds [T]
    fp64 -> hits [V, T] int32."""
    lib = _check(gt_span, gt_off, prop, prop_off, thresholds)
    g, p, v, t = gt_span.shape[0], prop.shape[0], gt_off.numel() - 1, thresholds.numel()
    if gt_span.shape != (g, 2) or gt_span.dtype != torch.float64 or prop.shape != (p, 2) or prop.dtype != torch.float64 \
            or gt_off.dtype != torch.int32 or prop_off.dtype != torch.int32 or prop_off.shape != gt_off.shape \
            or thresholds.dtype != torch.float64 or thresholds.dim() != 1 or v < 1:
        raise ValueError("eval_recall: bad shapes / dtypes")
    hits = torch.zeros((v, t), device=thresholds.device, dtype=torch.int32)
    lib.call("ssn_eval_recall", _p(gt_span) if g else None, _p(gt_off), g, _p(prop) if p else None, _p(prop_off), p, v,
             _p(thresholds), t, _p(hits), _stream(lib, thresholds))
    return hits


def proposal_eval_max_points():
    return int(_lib.get_lib().cdll.ssn_proposal_eval_max_points())


def proposal_eval_rank(score, prop_off, sort_off, sort_entries):
    """ssn_proposal_eval_rank: score [P] fp64, prop_off [V + 1] int32, sort_off [V + 1] int64 (see include/ssn_hip.h) ->
    order [P] int32: per video the flat indices in descending score, equal scores lower index first."""
    lib = _check(score, prop_off, sort_off)
    p, v = score.numel(), prop_off.numel() - 1
    if score.shape != (p,) or score.dtype != torch.float64 or v < 1 or prop_off.shape != (v + 1,) or prop_off.dtype != torch.int32 \
            or sort_off.shape != (v + 1,) or sort_off.dtype != torch.int64:
        raise ValueError("proposal_eval_rank: score must be float64 [P], prop_off int32 [V + 1] and sort_off int64 [V + 1]")
    sort_entries = int(sort_entries)
    if sort_entries < p or sort_entries >= 2 ** 31:
        raise ValueError("proposal_eval_rank: %d sort entries for %d proposals" % (sort_entries, p))
    dev = prop_off.device
    order = torch.zeros(p, device=dev, dtype=torch.int32)
    ws_bytes = int(lib.cdll.ssn_proposal_eval_workspace_bytes(sort_entries))
    ws = torch.zeros((ws_bytes + 7) // 8, device=dev, dtype=torch.int64)
    lib.call("ssn_proposal_eval_rank", _p(score) if p else None, _p(prop_off), p, v, _p(sort_off), sort_entries,
             _p(order) if p else None, _p(ws), ws_bytes, _stream(lib, prop_off))
    return order


def proposal_eval_ar_an(gt_span, gt_off, prop, prop_off, nr, thresholds, pcn, per_video, order=None):
    """ssn_proposal_eval_ar_an: gt_span [G, 2] fp64, gt_off [V + 1] int32, prop [P, 2] fp64, prop_off [V + 1] int32, nr [V]
    int32, thresholds [T] fp64, pcn [J] fp64, order [P] int32 or None -> (first_hit [G, T] int32, matches [T, J] int32,
    curves [T * J + 2 J + 1] fp64 = recall, avg_recall, proposals_per_video, auc), all on the device."""
    lib = _check(gt_span, gt_off, prop, prop_off, nr, thresholds, pcn, order)
    g, p, v, t, j = gt_span.shape[0], prop.shape[0], gt_off.numel() - 1, thresholds.numel(), pcn.numel()
    if gt_span.shape != (g, 2) or gt_span.dtype != torch.float64 or prop.shape != (p, 2) or prop.dtype != torch.float64 \
            or gt_off.dtype != torch.int32 or prop_off.dtype != torch.int32 or prop_off.shape != gt_off.shape or v < 1 or g < 1:
        raise ValueError("proposal_eval_ar_an: spans must be float64 [G >= 1, 2] / [P, 2], gt_off / prop_off int32 [V + 1]")
    if nr.shape != (v,) or nr.dtype != torch.int32 or thresholds.dtype != torch.float64 or thresholds.dim() != 1 \
            or pcn.dtype != torch.float64 or pcn.dim() != 1:
        raise ValueError("proposal_eval_ar_an: nr must be int32 [V], thresholds and pcn float64 vectors")
    if order is not None and (order.shape != (p,) or order.dtype != torch.int32):
        raise ValueError("proposal_eval_ar_an: order must be int32 [P]")
    if t < 1 or t > 32:
        raise ValueError("proposal_eval_ar_an: between 1 and 32 tIoU thresholds in one call, got %d" % t)
    if j < 1 or j > proposal_eval_max_points():
        raise ValueError("proposal_eval_ar_an: between 1 and %d curve points in one call, got %d" % (proposal_eval_max_points(), j))
    dev = thresholds.device
    first_hit = torch.zeros((g, t), device=dev, dtype=torch.int32)
    matches = torch.zeros((t, j), device=dev, dtype=torch.int32)
    curves = torch.zeros(t * j + 2 * j + 1, device=dev, dtype=torch.float64)
    lib.call("ssn_proposal_eval_ar_an", _p(gt_span), _p(gt_off), g, _p(prop) if p else None, _p(prop_off), p, v, _p(nr),
             _p(order) if order is not None and p else None, _p(thresholds), t, _p(pcn), j, float(per_video), _p(first_hit),
             _p(matches), _p(curves), _stream(lib, thresholds))
    return first_hit, matches, curves


# ------------------------------------------------------------------------------------ proposal lists
def _sw_levels(spans, steps, who):
    """Host int32 arrays of the per-level span / step tables (kept alive by the caller for the duration of the call)."""
    spans, steps = [int(x) for x in spans], [int(x) for x in steps]
    if len(spans) < 1 or len(spans) > 31 or len(spans) != len(steps):
        raise ValueError("%s: 1 ... 31 levels with one span and one step each, got %d / %d" % (who, len(spans), len(steps)))
    if min(spans) < 1 or min(steps) < 1 or max(spans) >= 2 ** 31 or max(steps) >= 2 ** 31:
        raise ValueError("%s: spans and steps must be int32 >= 1, got %r / %r" % (who, spans, steps))
    n = len(spans)
    return (ctypes.c_int * n)(*spans), (ctypes.c_int * n)(*steps), n


def sw_count(durations, spans, steps):
    """ssn_sw_count: durations [V] fp64 (device), spans / steps: host lists of the per-level t_span and step ->
    counts [V, L] int32 (device)."""
    lib = _check(durations)
    if durations.dim() != 1 or durations.dtype != torch.float64 or durations.numel() < 1:
        raise ValueError("sw_count: durations must be float64 [V >= 1], got %s %s" % (durations.dtype, tuple(durations.shape)))
    h_spans, h_steps, n = _sw_levels(spans, steps, "sw_count")
    v = durations.numel()
    counts = torch.zeros((v, n), device=durations.device, dtype=torch.int32)
    lib.call("ssn_sw_count", _p(durations), v, ctypes.addressof(h_spans), ctypes.addressof(h_steps), n, _p(counts),
             _stream(lib, durations))
    return counts


def sw_fill(offsets, spans, steps, total):
    """ssn_sw_fill: offsets [V * L + 1] int32 (device, exclusive prefix sums of the counts, last entry `total`) ->
    windows [total, 2] fp64 (device)."""
    lib = _check(offsets)
    h_spans, h_steps, n = _sw_levels(spans, steps, "sw_fill")
    total = int(total)
    if offsets.dim() != 1 or offsets.dtype != torch.int32 or offsets.numel() < n + 1 or (offsets.numel() - 1) % n:
        raise ValueError("sw_fill: offsets must be int32 [V * L + 1], got %s %s for %d levels"
                         % (offsets.dtype, tuple(offsets.shape), n))
    if total < 0 or total >= 2 ** 30:
        raise ValueError("sw_fill: %d windows in one batch, split it" % total)
    windows = torch.zeros((total, 2), device=offsets.device, dtype=torch.float64)
    lib.call("ssn_sw_fill", _p(offsets), (offsets.numel() - 1) // n, ctypes.addressof(h_spans), ctypes.addressof(h_steps), n,
             total, _p(windows) if total else None, _stream(lib, offsets))
    return windows


def proposal_list_rows(gt_span, gt_off, prop, prop_off, frame_cnt, durations):
    """ssn_proposal_list_rows: gt_span [G, 2] fp64, gt_off [V + 1] int32, prop [P, 2] fp64, prop_off [V + 1] int32, frame_cnt
    [V] int32, durations [V] fp64 -> (gt_frames [G, 2] int32, frames [P, 2] int32, status [V] int32)."""
    lib = _check(gt_span, gt_off, prop, prop_off, frame_cnt, durations)
    g, p, v = gt_span.shape[0], prop.shape[0], durations.numel()
    if gt_span.shape != (g, 2) or gt_span.dtype != torch.float64 or prop.shape != (p, 2) or prop.dtype != torch.float64:
        raise ValueError("proposal_list_rows: spans must be float64 [G, 2] / [P, 2]")
    if v < 1 or durations.shape != (v,) or durations.dtype != torch.float64 or frame_cnt.shape != (v,) \
            or frame_cnt.dtype != torch.int32:
        raise ValueError("proposal_list_rows: durations must be float64 [V >= 1] and frame_cnt int32 [V]")
    if gt_off.shape != (v + 1,) or gt_off.dtype != torch.int32 or prop_off.shape != (v + 1,) or prop_off.dtype != torch.int32:
        raise ValueError("proposal_list_rows: gt_off / prop_off must be int32 [V + 1]")
    dev = durations.device
    gt_frames = torch.zeros((g, 2), device=dev, dtype=torch.int32)
    frames = torch.zeros((p, 2), device=dev, dtype=torch.int32)
    status = torch.zeros(v, device=dev, dtype=torch.int32)
    lib.call("ssn_proposal_list_rows", _p(gt_span) if g else None, _p(gt_off), g, _p(prop) if p else None, _p(prop_off), p,
             _p(frame_cnt), _p(durations), v, _p(gt_frames) if g else None, _p(frames) if p else None, _p(status),
             _stream(lib, durations))
    return gt_frames, frames, status


_PROPOSAL_TEXT_BLOCK = 256


class ProposalTextInputs(namedtuple("ProposalTextInputs", "gt_label gt_frames gt_off label iou overlap_self frames prop_off "
                                    "frame_cnt paths path_off write item_off n_items first_index")):
    """What ssn_proposal_text_size / _fill read (include/ssn_hip.h), ANY device arrays of these shapes: gt_label [G] int32 as
    written, gt_frames [G, 2] int32, gt_off [V + 1] int32, label [P] int32, iou / overlap_self [P] fp64, frames [P, 2] int32,
    prop_off [V + 1] int32, frame_cnt [V] int32, paths uint8 (the records' path bytes back to back), path_off [W + 1] int32,
    write [W] int32 (the video of every record), item_off [W + 1] int32 (prefix sums of 3 + n_gt + K over the records),
    n_items (their total, a host int), first_index."""

    def check(self, who):
        g, p, v, w = self.gt_label.numel(), self.label.numel(), self.frame_cnt.numel(), self.write.numel()
        i32 = [(self.gt_label, (g,)), (self.gt_frames, (g, 2)), (self.gt_off, (v + 1,)), (self.label, (p,)), (self.frames, (p, 2)),
               (self.prop_off, (v + 1,)), (self.frame_cnt, (v,)), (self.path_off, (w + 1,)), (self.write, (w,)),
               (self.item_off, (w + 1,))]
        if v < 1 or w < 1 or any(t.dtype != torch.int32 or tuple(t.shape) != s for t, s in i32):
            raise ValueError("%s: the integer inputs must be int32 of the shapes of ProposalTextInputs, V >= 1 and W >= 1" % who)
        if self.iou.dtype != torch.float64 or self.iou.shape != (p,) or self.overlap_self.dtype != torch.float64 \
                or self.overlap_self.shape != (p,) or self.paths.dtype != torch.uint8 or self.paths.dim() != 1:
            raise ValueError("%s: iou / overlap_self must be float64 [P] and paths uint8 [bytes]" % who)
        n, first = int(self.n_items), int(self.first_index)
        if n < 3 * w or n >= 2 ** 31 or first < 0 or first + w >= 2 ** 31 or self.paths.numel() >= 2 ** 30:
            raise ValueError("%s: %d items for %d records, first index %d, %d path bytes" % (who, n, w, first, self.paths.numel()))
        return g, p, v, w, n, first

    def head(self, g, p, v):
        """the arguments both entries begin with"""
        return (_p(self.gt_label) if g else None, _p(self.gt_frames) if g else None, _p(self.gt_off), g,
                _p(self.label) if p else None, _p(self.iou) if p else None, _p(self.overlap_self) if p else None,
                _p(self.frames) if p else None, _p(self.prop_off), p, _p(self.frame_cnt), v)


def proposal_text_items(gt_off, prop_off, write):
    """item_off of ProposalTextInputs on the HOST: gt_off / prop_off [V + 1] and write [W], numpy -> int64 [W + 1]."""
    import numpy as np
    gt_off, prop_off, write = (np.asarray(x, dtype=np.int64) for x in (gt_off, prop_off, write))
    per_record = 3 + (gt_off[1:] - gt_off[:-1])[write] + (prop_off[1:] - prop_off[:-1])[write]
    return np.concatenate([[0], np.cumsum(per_record)]).astype(np.int64)


def proposal_text_size(inp, status=None):
    """ssn_proposal_text_size: -> (bp [ceil(n_items / 256) + 1] int32 whose last word is the byte count of the text, or -1
    for 2^31 and more; status [V] int32 with bit 2 set for the videos that hold a float '%.4f' is not formed of on the
    device).  status given: ORed into."""
    lib = _check(*[t for t in inp if torch.is_tensor(t)])
    g, p, v, w, n, first = inp.check("proposal_text_size")
    dev = inp.write.device
    if status is None:
        status = torch.zeros(v, device=dev, dtype=torch.int32)
    elif status.shape != (v,) or status.dtype != torch.int32 or not status.is_contiguous():
        raise ValueError("proposal_text_size: status must be int32 [V]")
    bp = torch.zeros((n + _PROPOSAL_TEXT_BLOCK - 1) // _PROPOSAL_TEXT_BLOCK + 1, device=dev, dtype=torch.int32)
    lib.call("ssn_proposal_text_size", *(inp.head(g, p, v) + (_p(inp.path_off), inp.paths.numel(), _p(inp.write), _p(inp.item_off),
                                                             w, n, first, _p(bp), _p(status), _stream(lib, inp.write))))
    return bp, status


def proposal_text_fill(inp, bp, out):
    """ssn_proposal_text_fill: bp of proposal_text_size, out uint8 [bytes of the text or more] (a contiguous view at any
    alignment; only the text's bytes are written) -> rec_off [W + 1] int32."""
    lib = _check(bp, out, *[t for t in inp if torch.is_tensor(t)])
    g, p, v, w, n, first = inp.check("proposal_text_fill")
    if bp.dtype != torch.int32 or bp.shape != ((n + _PROPOSAL_TEXT_BLOCK - 1) // _PROPOSAL_TEXT_BLOCK + 1,) \
            or out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < 1 or out.numel() >= 2 ** 31:
        raise ValueError("proposal_text_fill: bp must be what proposal_text_size returned and out uint8 [1 ... 2^31 - 1]")
    rec_off = torch.zeros(w + 1, device=inp.write.device, dtype=torch.int32)
    lib.call("ssn_proposal_text_fill", *(inp.head(g, p, v) + (_p(inp.paths) if inp.paths.numel() else None, _p(inp.path_off),
                                                             inp.paths.numel(), _p(inp.write), _p(inp.item_off), w, n, first,
                                                             _p(bp), _p(out), out.numel(), _p(rec_off), _stream(lib, inp.write))))
    return rec_off


# ------------------------------------------------------------------------------------ test table
TEST_TABLE_MAX_PARTS = 16
_TEST_TABLE_BLOCK = 256


def _test_table_inputs(who, frames, p_off, frame_cnt):
    p, v = frames.shape[0], frame_cnt.numel()
    if frames.shape != (p, 2) or frames.dtype != torch.int32:
        raise ValueError("%s: frames must be int32 [P, 2], got %s %s" % (who, frames.dtype, tuple(frames.shape)))
    if v < 1 or frame_cnt.shape != (v,) or frame_cnt.dtype != torch.int32 or p_off.shape != (v + 1,) or p_off.dtype != torch.int32:
        raise ValueError("%s: frame_cnt must be int32 [V >= 1] and p_off int32 [V + 1]" % who)
    if p >= 2 ** 30:
        raise ValueError("%s: %d proposals in one batch (2^30 or more), split it" % (who, p))
    return p, v


def test_table_stages(stpp_cfg):
    """The STPP configuration ``(starting, course, ending)`` (ints or tuples of ints) as the host arrays ssn_test_table_fill
    takes: (levels per stage [3], parts per level, parts in total); more than 16 parts are refused."""
    if len(stpp_cfg) != 3:
        raise ValueError("test_table: the STPP configuration has three stages, got %r" % (stpp_cfg,))
    stages = [(int(c),) if isinstance(c, int) else tuple(int(x) for x in c) for c in stpp_cfg]
    parts = [x for st in stages for x in st]
    if any(len(st) < 1 for st in stages) or min(parts) < 1:
        raise ValueError("test_table: every stage needs at least one level of at least one part, got %r" % (stpp_cfg,))
    if sum(parts) > TEST_TABLE_MAX_PARTS:
        raise ValueError("test_table: %d parts in total, at most %d supported" % (sum(parts), TEST_TABLE_MAX_PARTS))
    return [len(st) for st in stages], parts, sum(parts)


test_table_stages.__test__ = False      # (library functions whose names start with "test": not test cases)


def test_table_mark(frames, p_off, frame_cnt):
    """ssn_test_table_mark: frames [P, 2] int32, p_off [V + 1] int32, frame_cnt [V] int32 (device) -> (keep [P], pre [P],
    bp [ceil(P / 256) + 1], counts [V]) int32: the keep flags, their prefix sums, and the rows of every video in the table
    (-1: the video holds a negative frame number)."""
    lib = _check(frames, p_off, frame_cnt)
    p, v = _test_table_inputs("test_table_mark", frames, p_off, frame_cnt)
    dev = frame_cnt.device
    # (every element is written: keep / pre by the lane of their row, bp by its block and the scan, counts by the entry's memset)
    keep = torch.empty(p, device=dev, dtype=torch.int32)
    pre = torch.empty(p, device=dev, dtype=torch.int32)
    bp = torch.empty((p + _TEST_TABLE_BLOCK - 1) // _TEST_TABLE_BLOCK + 1, device=dev, dtype=torch.int32)
    counts = torch.empty(v, device=dev, dtype=torch.int32)
    lib.call("ssn_test_table_mark", _p(frames) if p else None, _p(p_off), p, _p(frame_cnt), v, _p(keep) if p else None,
             _p(pre) if p else None, _p(bp), _p(counts), _stream(lib, frame_cnt))
    return keep, pre, bp, counts


test_table_mark.__test__ = False


def test_table_fill(frames, p_off, frame_cnt, n_rows, keep, pre, bp, k_off, total, stpp_cfg):
    """ssn_test_table_fill: the inputs and outputs of ``test_table_mark``, n_rows [V] int32, k_off [V + 1] int32 (device;
    exclusive prefix sums of the counts, last entry ``total``) and the STPP configuration (host) -> (src [K] int32, rel
    [K, 2] fp64, ticks [K, 4] int32, scaling [K, 2] fp64, ranges [K, n_parts, 2] int32, act [K, 2] int32)."""
    lib = _check(frames, p_off, frame_cnt, n_rows, keep, pre, bp, k_off)
    p, v = _test_table_inputs("test_table_fill", frames, p_off, frame_cnt)
    stage_entries, parts, n_parts = test_table_stages(stpp_cfg)
    total = int(total)
    if n_rows.shape != (v,) or n_rows.dtype != torch.int32 or k_off.shape != (v + 1,) or k_off.dtype != torch.int32:
        raise ValueError("test_table_fill: n_rows must be int32 [V] and k_off int32 [V + 1]")
    if keep.shape != (p,) or pre.shape != (p,) or bp.numel() != (p + _TEST_TABLE_BLOCK - 1) // _TEST_TABLE_BLOCK + 1 \
            or any(t.dtype != torch.int32 for t in (keep, pre, bp)):
        raise ValueError("test_table_fill: keep / pre / bp are not the outputs of test_table_mark for these frames")
    if total < v or total > p + v:
        raise ValueError("test_table_fill: %d rows for %d videos and %d proposals" % (total, v, p))
    dev = frame_cnt.device
    src = torch.zeros(total, device=dev, dtype=torch.int32)
    rel = torch.zeros((total, 2), device=dev, dtype=torch.float64)
    ticks = torch.zeros((total, 4), device=dev, dtype=torch.int32)
    scaling = torch.zeros((total, 2), device=dev, dtype=torch.float64)
    ranges = torch.zeros((total, n_parts, 2), device=dev, dtype=torch.int32)
    act = torch.zeros((total, 2), device=dev, dtype=torch.int32)
    h_stage = (ctypes.c_int * 3)(*stage_entries)
    h_parts = (ctypes.c_int * len(parts))(*parts)
    lib.call("ssn_test_table_fill", _p(frames) if p else None, _p(p_off), p, _p(frame_cnt), _p(n_rows), v,
             _p(keep) if p else None, _p(pre) if p else None, _p(bp), _p(k_off), total, ctypes.addressof(h_stage),
             ctypes.addressof(h_parts), len(parts), _p(src), _p(rel), _p(ticks), _p(scaling), _p(ranges), _p(act),
             _stream(lib, frame_cnt))
    return src, rel, ticks, scaling, ranges, act


test_table_fill.__test__ = False


# ------------------------------------------------------------------------------------ video-level classification
def vcls_lds_rows():
    return int(_lib.get_lib().cdll.ssn_vcls_lds_rows())


def _vcls_offsets(h_offsets, total, device, who, name="offsets"):
    """A HOST int32 offset table [n + 1], checked here (ascending from 0 to `total`) -> its copy on `device`."""
    if not torch.is_tensor(h_offsets) or h_offsets.is_cuda or h_offsets.dtype != torch.int32 or h_offsets.dim() != 1 \
            or h_offsets.numel() < 2:
        raise ValueError("%s: %s must be a host int32 tensor [n + 1], n >= 1" % (who, name))
    if int(h_offsets[0]) != 0 or int(h_offsets[-1]) != int(total) or bool((h_offsets[1:] < h_offsets[:-1]).any()):
        raise ValueError("%s: %s must ascend from 0 to %d" % (who, name, int(total)))
    return h_offsets.contiguous().to(device)


def _vcls_rows(x, rank, who, name="rows"):
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != rank or min(x.shape[1:]) < 1:
        raise ValueError("%s: %s must be float32 of rank %d with C >= 1, got %s %s" % (
            who, name, rank, getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))


def vcls_status(x, h_offsets):
    """ssn_vcls_status: x float32 [N, ...] ragged by the host offsets [V + 1] -> status [V] int32 on the device (1: a
    non-finite value among the video's rows, 2: no rows)."""
    lib = _check(x)
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() < 2 or min(x.shape[1:]) < 1:
        raise ValueError("vcls_status: x must be float32 [N, ..., C >= 1]")
    n = x.shape[0]
    off = _vcls_offsets(h_offsets, n, x.device, "vcls_status")
    v = off.numel() - 1
    status = torch.empty(v, device=x.device, dtype=torch.int32)
    lib.call("ssn_vcls_status", _p(x) if n else None, _p(off), v, n, x.shape[1:].numel(), _p(status), _stream(lib, x))
    return status


def vcls_crop_reduce(raw, use_max=False, out=None):
    """ssn_vcls_crop_reduce: raw float32 [N, crops, C] -> [N, C], the crops' mean (added in order, one division) or maximum."""
    lib = _check(raw, out)
    _vcls_rows(raw, 3, "vcls_crop_reduce", "raw")
    n, crops, c = raw.shape
    if out is None:
        out = torch.empty((n, c), device=raw.device, dtype=torch.float32)
    if out.shape != (n, c) or out.dtype != torch.float32:
        raise ValueError("vcls_crop_reduce: out must be float32 [%d, %d]" % (n, c))
    lib.call("ssn_vcls_crop_reduce", _p(raw) if n else None, _p(out) if n else None, n, crops, c, int(bool(use_max)),
             _stream(lib, raw))
    return out


def vcls_window_max(frm, h_offsets, h_win_off, spans, steps, out=None):
    """ssn_vcls_window_max: frm float32 [N, C] ragged by the host offsets [V + 1]; spans / steps int32 [S] on the device;
    h_win_off host int32 [V * S + 1] -> the window maxima [W, C], W = h_win_off[-1]."""
    lib = _check(frm, spans, steps, out)
    _vcls_rows(frm, 2, "vcls_window_max", "frm")
    n, c = frm.shape
    s = spans.numel()
    if spans.dtype != torch.int32 or steps.dtype != torch.int32 or spans.dim() != 1 or steps.shape != spans.shape or s < 1:
        raise ValueError("vcls_window_max: spans and steps must be int32 [S]")
    off = _vcls_offsets(h_offsets, n, frm.device, "vcls_window_max")
    v = off.numel() - 1
    w = int(h_win_off[-1]) if torch.is_tensor(h_win_off) and h_win_off.numel() else -1
    win = _vcls_offsets(h_win_off, w, frm.device, "vcls_window_max", "win_off")
    if win.numel() != v * s + 1:
        raise ValueError("vcls_window_max: win_off must hold V * S + 1 = %d entries" % (v * s + 1))
    if out is None:
        out = torch.empty((w, c), device=frm.device, dtype=torch.float32)
    if out.shape != (w, c) or out.dtype != torch.float32:
        raise ValueError("vcls_window_max: out must be float32 [%d, %d]" % (w, c))
    lib.call("ssn_vcls_window_max", _p(frm) if n else None, _p(off), _p(win), _p(spans), _p(steps), v, s, n, c, w,
             _p(out) if w else None, _stream(lib, frm))
    return out


def vcls_topk_mean(rows, h_seg_off, h_ks, out=None):
    """ssn_vcls_topk_mean: rows float32 [N, C], host seg_off int32 [G + 1] and ks int32 [G] (each >= 1) -> [G, C]: per
    class the mean of the min(k, n) largest rows of the segment."""
    lib = _check(rows, out)
    _vcls_rows(rows, 2, "vcls_topk_mean")
    n, c = rows.shape
    seg = _vcls_offsets(h_seg_off, n, rows.device, "vcls_topk_mean", "seg_off")
    g = seg.numel() - 1
    if not torch.is_tensor(h_ks) or h_ks.is_cuda or h_ks.dtype != torch.int32 or h_ks.shape != (g,):
        raise ValueError("vcls_topk_mean: ks must be a host int32 tensor [%d]" % g)
    if bool((h_ks < 1).any()):
        raise ValueError("vcls_topk_mean: every k must be >= 1")
    ks = h_ks.contiguous().to(rows.device)
    if out is None:
        out = torch.empty((g, c), device=rows.device, dtype=torch.float32)
    if out.shape != (g, c) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("vcls_topk_mean: out must be contiguous float32 [%d, %d]" % (g, c))
    lib.call("ssn_vcls_topk_mean", _p(rows) if n else None, _p(seg), _p(ks), g, n, c, _p(out), _stream(lib, rows))
    return out


def vcls_tpp(frm, h_offsets, num_class, out=None):
    """ssn_vcls_tpp: frm float32 [N, stages * num_class] -> [V, num_class]."""
    lib = _check(frm, out)
    _vcls_rows(frm, 2, "vcls_tpp", "frm")
    n, width = frm.shape
    c = int(num_class)
    if c < 1 or width % c:
        raise ValueError("vcls_tpp: %d columns are not a multiple of num_class = %d" % (width, c))
    off = _vcls_offsets(h_offsets, n, frm.device, "vcls_tpp")
    v = off.numel() - 1
    if out is None:
        out = torch.empty((v, c), device=frm.device, dtype=torch.float32)
    if out.shape != (v, c) or out.dtype != torch.float32:
        raise ValueError("vcls_tpp: out must be float32 [%d, %d]" % (v, c))
    lib.call("ssn_vcls_tpp", _p(frm) if n else None, _p(off), v, n, c, width // c, _p(out), _stream(lib, frm))
    return out


def vcls_finish(terms, video_axis, weights=None, status=None, divide=False, softmax=False, out=None):
    """ssn_vcls_finish: terms float32 [V, S, C] (video_axis 0) or [S, V, C] (video_axis 1) -> [V, C]: the S terms of a
    video added in order (terms 1 ... S - 1 times weights [S - 1] when given), divided by S when `divide`, NaN where
    status [V] is not zero, then the optional softmax along C."""
    lib = _check(terms, weights, status, out)
    _vcls_rows(terms, 3, "vcls_finish", "terms")
    if video_axis not in (0, 1):
        raise ValueError("vcls_finish: video_axis must be 0 or 1")
    v, s = (terms.shape[0], terms.shape[1]) if video_axis == 0 else (terms.shape[1], terms.shape[0])
    c = terms.shape[2]
    if v < 1 or s < 1:
        raise ValueError("vcls_finish: no videos or no terms")
    stride_v, stride_s = (s * c, c) if video_axis == 0 else (c, v * c)
    if weights is not None and (weights.dtype != torch.float32 or weights.shape != (s - 1,)):
        raise ValueError("vcls_finish: weights must be float32 [%d]" % (s - 1))
    if status is not None and (status.dtype != torch.int32 or status.shape != (v,)):
        raise ValueError("vcls_finish: status must be int32 [%d]" % v)
    if out is None:
        out = torch.empty((v, c), device=terms.device, dtype=torch.float32)
    if out.shape != (v, c) or out.dtype != torch.float32:
        raise ValueError("vcls_finish: out must be float32 [%d, %d]" % (v, c))
    lib.call("ssn_vcls_finish", _p(terms), _p(weights) if weights is not None and s > 1 else None, _p(status), v, s, c,
             stride_v, stride_s, int(bool(divide)), int(bool(softmax)), _p(out), _stream(lib, terms))
    return out


def vcls_metrics(scores, gt, label, top_ks):
    """ssn_vcls_metrics: scores float32 [V, C], gt uint8 [V, C], label int32 [V] or None, top_ks int32 [K], all on the
    device -> (counts int32 [K + 3 C], ap float64 [C], results float64 [K + 2]) on the device."""
    lib = _check(scores, gt, label, top_ks)
    _vcls_rows(scores, 2, "vcls_metrics", "scores")
    v, c = scores.shape
    if v < 1 or gt.shape != (v, c) or gt.dtype != torch.uint8 or top_ks.dtype != torch.int32 or top_ks.dim() != 1 \
            or (label is not None and (label.shape != (v,) or label.dtype != torch.int32)):
        raise ValueError("vcls_metrics: need V >= 1 videos, gt uint8 [V, C], label int32 [V], top_ks int32 [K]")
    k = top_ks.numel()
    dev = scores.device
    counts = torch.empty(k + 3 * c, device=dev, dtype=torch.int32)
    ap = torch.empty(c, device=dev, dtype=torch.float64)
    results = torch.empty(k + 2, device=dev, dtype=torch.float64)
    ws_bytes = int(lib.cdll.ssn_vcls_metrics_workspace_bytes(v, c))
    ws = torch.empty((ws_bytes + 7) // 8, device=dev, dtype=torch.int64)
    lib.call("ssn_vcls_metrics", _p(scores), _p(gt), _p(label), _p(top_ks) if k else None, v, c, k, _p(counts), _p(ap),
             _p(results), _p(ws), ws_bytes, _stream(lib, scores))
    return counts, ap, results


def actionness_fc(feat, w, b, raw_true, tick0, num_crop):
    """ssn_actionness_fc: feat [num_crop * ticks, D] (crop-major backbone output of one call), w [C, D], b [C] or None ->
    raw_true[tick0 + t, c, :] = logits of feature row c * ticks + t; raw_true [T, num_crop, C] is the video's staging tensor."""
    lib = _check(feat, w, b, raw_true)
    if feat.dim() != 2 or w.dim() != 2 or feat.shape[1] != w.shape[1] or feat.dtype != torch.float32 or w.dtype != torch.float32:
        raise ValueError("actionness_fc: feat must be float32 [R, D] and w float32 [C, D]")
    c, d = w.shape
    if raw_true.dim() != 3 or raw_true.shape[1] != num_crop or raw_true.shape[2] != c or raw_true.dtype != torch.float32:
        raise ValueError("actionness_fc: raw_true must be float32 [T, %d, %d], got %s" % (num_crop, c, tuple(raw_true.shape)))
    if feat.shape[0] % num_crop or (b is not None and (b.shape != (c,) or b.dtype != torch.float32)):
        raise ValueError("actionness_fc: %d feature rows are not a multiple of %d crops, or bad bias" % (feat.shape[0], num_crop))
    ticks = feat.shape[0] // num_crop
    lib.call("ssn_actionness_fc", _p(feat) if ticks else None, _p(w), _p(b), _p(raw_true) if ticks else None, ticks,
             int(num_crop), c, d, int(tick0), raw_true.shape[0], _stream(lib, raw_true))


def actionness_group(raw_true, ref_batch, raw=None):
    """ssn_actionness_group: raw_true [T, crops, C] -> (raw [T, crops, C], mean [T, C]).  ref_batch 0: raw is raw_true
    (no copy unless `raw` is given); ref_batch g > 0: the rows binary_test.py writes with g ticks per generator batch."""
    lib = _check(raw_true, raw)
    if raw_true.dim() != 3 or raw_true.dtype != torch.float32 or raw_true.shape[1] < 1 or raw_true.shape[2] < 1:
        raise ValueError("actionness_group: raw_true must be float32 [T, crops >= 1, C >= 1]")
    t, crops, c = raw_true.shape
    if raw is None:
        raw = raw_true if int(ref_batch) == 0 else torch.empty_like(raw_true)
    if raw.shape != raw_true.shape or raw.dtype != torch.float32:
        raise ValueError("actionness_group: raw must be float32 %s" % (tuple(raw_true.shape),))
    mean = torch.empty((t, c), device=raw_true.device, dtype=torch.float32)
    lib.call("ssn_actionness_group", _p(raw_true) if t else None, _p(raw) if t else None, _p(mean) if t else None, t, crops, c,
             int(ref_batch), _stream(lib, raw_true))
    return raw, mean


def actionness_merge(rows, offsets, weights, out_offsets, out_rows, out=None):
    """ssn_actionness_merge: rows [N, C] fp32 (stream-major), offsets [S * V + 1] int32, weights [S] fp32, out_offsets
    [V + 1] int32, all on the device -> out [out_rows, C] (zeros where the tables of a video are inconsistent)."""
    lib = _check(rows, offsets, weights, out_offsets, out)
    s, v = weights.numel(), out_offsets.numel() - 1
    if rows.dim() != 2 or rows.dtype != torch.float32 or weights.dtype != torch.float32 or weights.dim() != 1 or s < 1:
        raise ValueError("actionness_merge: rows must be float32 [N, C] and weights float32 [S]")
    if offsets.dtype != torch.int32 or out_offsets.dtype != torch.int32 or v < 1 or offsets.shape != (s * v + 1,) \
            or out_offsets.dim() != 1:
        raise ValueError("actionness_merge: offsets must be int32 [S * V + 1] and out_offsets int32 [V + 1]")
    c = rows.shape[1]
    if out is None:
        out = torch.zeros((int(out_rows), c), device=rows.device, dtype=torch.float32)
    if out.shape != (int(out_rows), c) or out.dtype != torch.float32:
        raise ValueError("actionness_merge: out must be float32 [%d, %d]" % (int(out_rows), c))
    lib.call("ssn_actionness_merge", _p(rows) if rows.shape[0] else None, _p(offsets), _p(weights), _p(out_offsets),
             _p(out) if out_rows else None, s, v, c, rows.shape[0], int(out_rows), _stream(lib, rows))
    return out


@_hbm_timed
def linear_fwd(x, w, b, out):
    lib = _check(x, w, b, out)
    lib.call("ssn_linear_fwd", _p(x), _p(w), _p(b), _p(out), x.shape[0], w.shape[0], w.shape[1], _stream(lib, x))


@_hbm_timed
def linear_bwd(dout, x, w, dx, dw, db, accumulate_dx=False):
    lib = _check(dout, x, w, dx, dw, db)
    lib.call("ssn_linear_bwd", _p(dout), _p(x), _p(w), _p(dx), _p(dw), _p(db), x.shape[0], w.shape[0], w.shape[1],
             int(accumulate_dx), _stream(lib, x))


@_hbm_timed
def row_gather(src, index, dst):
    lib = _check(src, index, dst)
    width = src[0].numel() if src.shape[0] else 0
    lib.call("ssn_row_gather", _p(src), _p(index), _p(dst), index.numel(), width, _stream(lib, src))


@_hbm_timed
def row_scatter(src, index, dst):
    lib = _check(src, index, dst)
    width = dst[0].numel()
    lib.call("ssn_row_scatter", _p(src), _p(index), _p(dst), index.numel(), dst.shape[0], width, _stream(lib, dst))


@_hbm_timed
def ce_loss_fwd(logits, target, loss, workspace):
    lib = _check(logits, target, loss, workspace)
    lib.call("ssn_ce_loss_fwd", _p(logits), _p(target), _p(loss), _p(workspace), logits.shape[0], logits.shape[1],
             _stream(lib, logits))


@_hbm_timed
def ce_loss_bwd(logits, target, lse, gout, dlogits):
    lib = _check(logits, target, lse, gout, dlogits)
    lib.call("ssn_ce_loss_bwd", _p(logits), _p(target), _p(lse), _p(gout), _p(dlogits), logits.shape[0],
             logits.shape[1], _stream(lib, logits))


@_hbm_timed
def completeness_loss_fwd(pred, labels, loss, coef, workspace, group, split, keep_pos, keep_neg, den):
    lib = _check(pred, labels, loss, coef, workspace)
    lib.call("ssn_completeness_loss_fwd", _p(pred), _p(labels), _p(loss), _p(coef), _p(workspace), pred.shape[0],
             pred.shape[1], group, split, keep_pos, keep_neg, float(den), _stream(lib, pred))


@_hbm_timed
def completeness_loss_bwd(labels, coef, gout, dpred, den):
    lib = _check(labels, coef, gout, dpred)
    lib.call("ssn_completeness_loss_bwd", _p(labels), _p(coef), _p(gout), _p(dpred), dpred.shape[0], dpred.shape[1],
             float(den), _stream(lib, dpred))


@_hbm_timed
def cw_smoothl1_fwd(pred, labels, targets, loss, diff):
    lib = _check(pred, labels, targets, loss, diff)
    lib.call("ssn_cw_smoothl1_fwd", _p(pred), _p(labels), _p(targets), _p(loss), _p(diff), pred.shape[0],
             pred.shape[1], _stream(lib, pred))


@_hbm_timed
def cw_smoothl1_bwd(labels, diff, gout, dpred):
    lib = _check(labels, diff, gout, dpred)
    lib.call("ssn_cw_smoothl1_bwd", _p(labels), _p(diff), _p(gout), _p(dpred), dpred.shape[0], dpred.shape[1],
             _stream(lib, dpred))


@_hbm_timed
def total_loss_fwd(act, act_t, comp, comp_t, reg, reg_lbl, reg_t, group, split, keep_pos, keep_neg, den, w_comp, w_reg, losses, lse, coef,
                   diff, scratch):
    """ssn_total_loss_fwd: losses[4] = activity CE, completeness, regression, act + w_comp * comp + w_reg * reg (reg may be None)."""
    lib = _check(act, act_t, comp, comp_t, reg, reg_lbl, reg_t, losses, lse, coef, diff, scratch)
    has = reg is not None
    lib.call("ssn_total_loss_fwd", _p(act), _p(act_t), act.shape[0], act.shape[1], _p(comp), _p(comp_t), comp.shape[0], comp.shape[1],
             group, split, keep_pos, keep_neg, float(den), _p(reg), _p(reg_lbl) if has else None, _p(reg_t) if has else None,
             reg.shape[0] if has else 0, reg.shape[1] if has else 0, float(w_comp), float(w_reg), _p(losses), _p(lse), _p(coef),
             _p(diff), _p(scratch), _stream(lib, act))


@_hbm_timed
def total_loss_bwd(act, act_t, comp_t, comp_shape, reg_lbl, reg_shape, den, w_comp, w_reg, lse, coef, diff, gout, d_act, d_comp, d_reg):
    lib = _check(act, act_t, comp_t, reg_lbl, lse, coef, diff, gout, d_act, d_comp, d_reg)
    has = d_reg is not None
    lib.call("ssn_total_loss_bwd", _p(act), _p(act_t), act.shape[0], act.shape[1], _p(comp_t), comp_shape[0], comp_shape[1], float(den),
             _p(reg_lbl) if has else None, reg_shape[0] if has else 0, reg_shape[1] if has else 0, float(w_comp), float(w_reg), _p(lse),
             _p(coef), _p(diff), _p(gout), _p(d_act), _p(d_comp), _p(d_reg), _stream(lib, act))


def label_select(target, reg_target, idx, outs, out_reg):
    """target[idx[k]] -> outs[k] (k = 0, 1, and 2 with reg_target[idx[2]] -> out_reg when idx[2] is not None): one launch."""
    lib = _check(target, reg_target, *[t for t in list(idx) + list(outs) + [out_reg] if t is not None])
    n = [0 if i is None else i.numel() for i in idx]
    lib.call("ssn_label_select", _p(target), _p(reg_target), _p(idx[0]), n[0], _p(idx[1]), n[1], _p(idx[2]), n[2], _p(outs[0]), _p(outs[1]),
             _p(outs[2]), _p(out_reg), _stream(lib, target))


class ParamChecksum(object):
    """Device-side fingerprint of a set of tensors (csrc/elementwise.hip: ssn_param_checksum): recorded once, checked later WITHOUT a
    host read -- a mismatch raises `bit` in a device flag word (the planes path's fault word: the pass that used the stale derivative is
    then repeated by the range guard's poll, see planes_exec.run_forward)."""

    def __init__(self, tensors, device):
        import numpy as np
        self.tensors = [t for t in tensors]      # (kept alive: the table holds raw pointers)
        tab = np.zeros((len(self.tensors), 2), dtype=np.int64)
        for i, t in enumerate(self.tensors):
            assert t.is_contiguous() and t.element_size() == 4, "checksummed tensors are contiguous 32-bit"
            tab[i] = (t.data_ptr(), t.numel())
        self.table = torch.from_numpy(tab).to(device)
        self.expected = torch.zeros(1, device=device, dtype=torch.int64)
        self.fresh = torch.zeros(1, device=device, dtype=torch.int64)
        self.ptrs = tuple(int(v) for v in tab[:, 0])
        lib = _lib.get_lib()
        lib.call("ssn_param_checksum", _p(self.table), len(self.tensors), _p(self.expected), None, None, 0, _stream(lib, self.table))

    def same_storage(self, tensors):
        return self.ptrs == tuple(t.data_ptr() for t in tensors)

    def check(self, flag, bit):
        lib = _lib.get_lib()
        lib.call("ssn_param_checksum", _p(self.table), len(self.tensors), _p(self.fresh), _p(self.expected), _p(flag), int(bit),
                 _stream(lib, self.table))


# ------------------------------------------------------------------------------------ optimiser
# Counts the in-place parameter updates issued through this module (they go through raw pointers: torch's version counters do not
# see them).  planes_exec keys its inference cache of packed weights on it.
PARAM_EPOCH = 0


def sgd_step(w, grad, buf, lr, momentum, weight_decay, grad_scale=1.0, first_step=False, skip_flag=None):
    global PARAM_EPOCH
    PARAM_EPOCH += 1
    lib = _check(w, grad, buf)
    lib.call("ssn_sgd_step", _p(w), _p(grad), _p(buf), w.numel(), float(lr), float(momentum), float(weight_decay),
             float(grad_scale), int(first_step), _p(skip_flag), _stream(lib, w))


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def sgd_step_multi(ws, grads, bufs, lrs, wds, momentum, grad_scale=1.0, first_step=False, skip_flag=None):
    """One fused launch (per 48 tensors) of the SGD update for many parameter tensors.  skip_flag: device int32 tensor; the
    update is skipped while its first word is non-zero (the range guard of the planes path, planes_exec.PlanesState)."""
    if not ws:
        return
    global PARAM_EPOCH
    PARAM_EPOCH += 1
    lib = _check(*ws, *grads, *bufs)
    n = len(ws)
    sizes = (ctypes.c_long * n)(*[w.numel() for w in ws])
    lr = (ctypes.c_float * n)(*[float(v) for v in lrs])
    wd = (ctypes.c_float * n)(*[float(v) for v in wds])
    pw, pg, pb = _ptr_array(ws), _ptr_array(grads), _ptr_array(bufs)   # keep the arrays alive across the call
    lib.call("ssn_sgd_step_multi", n, ctypes.addressof(pw), ctypes.addressof(pg), ctypes.addressof(pb),
             ctypes.addressof(sizes), ctypes.addressof(lr), ctypes.addressof(wd), float(momentum), float(grad_scale),
             int(first_step), _p(skip_flag), _stream(lib, ws[0]))


def sgd_step_multi_dev(ws, grads, bufs, lrs, wds, momentum, grad_scale_dev, first_step=False, skip_flag=None):
    """sgd_step_multi with the gradient scale read from the device: grad_scale_dev is a fp32 tensor whose first element is the
    scale (``sumsq_multi(...)[1:]``).  Same update, same launches, nothing read by the host."""
    if not ws:
        return
    global PARAM_EPOCH
    PARAM_EPOCH += 1
    lib = _check(*ws, *grads, *bufs, grad_scale_dev)
    n = len(ws)
    sizes = (ctypes.c_long * n)(*[w.numel() for w in ws])
    lr = (ctypes.c_float * n)(*[float(v) for v in lrs])
    wd = (ctypes.c_float * n)(*[float(v) for v in wds])
    pw, pg, pb = _ptr_array(ws), _ptr_array(grads), _ptr_array(bufs)   # keep the arrays alive across the call
    lib.call("ssn_sgd_step_multi_dev", n, ctypes.addressof(pw), ctypes.addressof(pg), ctypes.addressof(pb),
             ctypes.addressof(sizes), ctypes.addressof(lr), ctypes.addressof(wd), float(momentum), _p(grad_scale_dev),
             int(first_step), _p(skip_flag), _stream(lib, ws[0]))


def sumsq_multi_workspace_floats(sizes):
    lib = _lib.get_lib()
    n = len(sizes)
    arr = (ctypes.c_long * max(n, 1))(*[int(v) for v in sizes])
    return int(lib.cdll.ssn_sumsq_multi_workspace_floats(n, ctypes.addressof(arr)))


def sumsq_multi(xs, pre_scale=1.0, max_norm=0.0, out=None, workspace=None):
    """2-norm over the fp32 tensors ``xs`` (contiguous, any 4-byte alignment, empty ones allowed) in ceil(len / 48) + 1 launches,
    deterministic.  Returns the device tensor ``out`` [2]: out[0] = norm * pre_scale, out[1] = the gradient scale of
    /root/reference/ssn_train.py:239-248 (pre_scale, times max_norm / (out[0] + 1e-6) when that is below 1; max_norm <= 0: no
    clipping).  No host read; nothing is allocated when ``out`` and ``workspace`` (>= sumsq_multi_workspace_floats) are given."""
    if not xs:
        raise ValueError("sumsq_multi needs at least one tensor")
    lib = _check(*xs, out, workspace)
    n = len(xs)
    sizes = (ctypes.c_long * n)(*[x.numel() for x in xs])
    if workspace is None:
        workspace = torch.empty(int(lib.cdll.ssn_sumsq_multi_workspace_floats(n, ctypes.addressof(sizes))), device=xs[0].device,
                                dtype=torch.float32)
    if out is None:
        out = torch.empty(2, device=xs[0].device, dtype=torch.float32)
    if out.dtype != torch.float32 or out.numel() < 2 or workspace.dtype != torch.float32:
        raise ValueError("sumsq_multi: out must be fp32 [2], workspace fp32")
    px = _ptr_array(xs)      # kept alive across the call
    lib.call("ssn_sumsq_multi", n, ctypes.addressof(px), ctypes.addressof(sizes), _p(workspace), workspace.numel(),
             float(pre_scale), float(max_norm), _p(out), _stream(lib, xs[0]))
    return out


def step_meters(logits, target, losses, loss_weight, state, skip_flag=None):
    """AverageMeter.update of every meter of one training / validation step in one launch (csrc/train_step.hip).  logits fp32
    [rows, cols] (rows may be strided), target int64 [rows], losses fp32 [n_losses <= 4] or None, state float64
    [(n_losses + 3) * 4 + 1] updated in place."""
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.dtype != torch.float32:
        raise ValueError("step_meters: logits must be fp32 [rows, cols] with unit column stride")
    if target.dtype != torch.int64 or target.numel() != logits.shape[0] or not target.is_contiguous():
        raise ValueError("step_meters: target must be contiguous int64 [rows]")
    n_losses = 0 if losses is None else losses.numel()
    if losses is not None and losses.dtype != torch.float32:
        raise ValueError("step_meters: losses must be fp32")
    if state.dtype != torch.float64 or state.numel() != (n_losses + 3) * 4 + 1:
        raise ValueError("step_meters: state must be float64 [(n_losses + 3) * 4 + 1]")
    lib = _check(target, losses, state, skip_flag)
    if not lib.is_emulator and not logits.is_cuda:
        raise RuntimeError("SSN HIP ops need HIP (cuda) tensors; there is no CPU fallback")
    rows, cols = logits.shape
    lib.call("ssn_step_meters", _p(logits), logits.stride(0) if rows > 1 else cols, _p(target), rows, cols, _p(losses), n_losses,
             float(loss_weight), _p(state), _p(skip_flag), _stream(lib, logits))


def train_step_launches(reset=False):
    """Kernel launches issued by step_meters / sumsq_multi / sgd_step_multi_dev on this thread since the last reset."""
    return int(_lib.get_lib().cdll.ssn_train_step_launches(1 if reset else 0))


def wgrad_reduce(part, dw, db, splits, taps=1):
    """dw [M, K] (any trailing shape), db [M] or None <- sum over the `splits` partial slabs part [splits, M, K + 1] in a fixed
    order (column K = bias).  taps > 1: the slabs' columns are tap-major (column t * (K / taps) + ci holds dW[m][ci][t]), the
    layout of the nine-tap planes weight gradient."""
    lib = _check(part, dw, db)
    m = dw.shape[0]
    k = dw.numel() // m
    assert part.numel() >= splits * m * (k + 1)
    lib.call("ssn_wgrad_reduce_taps", _p(part), _p(dw), _p(db), m, k, int(splits), int(taps), _stream(lib, part))


def bn_fold_multi(biases, gammas, betas, means, variances, eps, scales, shifts):
    """ssn_bn_fold for many layers in one launch per 48 layers."""
    if not gammas:
        return
    lib = _check(*gammas, *scales, *shifts)
    n = len(gammas)
    e = (ctypes.c_float * n)(*[float(v) for v in eps])
    c = (ctypes.c_int * n)(*[g.numel() for g in gammas])
    arrs = [_ptr_array(x) for x in (biases, gammas, betas, means, variances, scales, shifts)]   # kept alive
    lib.call("ssn_bn_fold_multi", n, ctypes.addressof(arrs[0]), ctypes.addressof(arrs[1]), ctypes.addressof(arrs[2]),
             ctypes.addressof(arrs[3]), ctypes.addressof(arrs[4]), ctypes.addressof(e), ctypes.addressof(arrs[5]),
             ctypes.addressof(arrs[6]), ctypes.addressof(c), _stream(lib, gammas[0]))


def sumsq(x, out, accumulate, workspace):
    lib = _check(x, out, workspace)
    lib.call("ssn_sumsq", _p(x), x.numel(), _p(out), int(accumulate), _p(workspace), _stream(lib, x))


def embed_planes(g, out):
    """out (ChanSlice / tensor [N, C, H, W]) <- g (ChanSlice [N, C, Ho, Wo]) in the top-left corner of every plane, zero elsewhere;
    out shares g's amax slot (same values)."""
    lib = _check(g, out)
    out_s = out if isinstance(out, ChanSlice) else full(out)
    ho, wo = g.hw
    h, w = out_s.hw
    lib.call("ssn_embed_planes", _p(g), _p(out_s), g.n, g.c, ho, wo, g.img_stride, h, w, out_s.img_stride, _stream(lib, _tensor_of(out_s)))
    attach_amax(_tensor_of(out_s), _amax_in(g))
    return out


def add_(dst, src):
    """dst += src (flat fp32 buffers of equal length)."""
    lib = _check(dst, src)
    assert dst.numel() == src.numel()
    lib.call("ssn_add_inplace", _p(dst), _p(src), dst.numel(), _stream(lib, dst))


def scale_(x, coef_dev=None, coef=1.0):
    lib = _check(x, coef_dev)
    lib.call("ssn_scale", _p(x), x.numel(), _p(coef_dev), float(coef), _stream(lib, x))


# ------------------------------------------------------------------------------------ TV-L1 optical flow (csrc/flow.hip)
def tvl1_tile_shape():
    """(th, tw, halo): the interior a workgroup of ssn_tvl1_iterate owns, and the most iterations one launch advances."""
    lib = _lib.get_lib()
    th, tw, halo = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.call("ssn_tvl1_tile_shape", ctypes.byref(th), ctypes.byref(tw), ctypes.byref(halo))
    return th.value, tw.value, halo.value


def flow_gray(rgb):
    """uint8 [..., H, W, 3] -> gray uint8 [..., H, W], (4899 R + 9617 G + 1868 B + 8192) >> 14."""
    lib = _check(rgb)
    if rgb.dtype != torch.uint8 or rgb.dim() < 3 or rgb.shape[-1] != 3:
        raise ValueError("flow_gray: uint8 [..., H, W, 3] expected, got %s %s" % (rgb.dtype, tuple(rgb.shape)))
    out = torch.empty(rgb.shape[:-1], device=rgb.device, dtype=torch.uint8)
    n = out.numel()
    lib.call("ssn_flow_gray", _p(rgb) if n else None, _p(out) if n else None, n, _stream(lib, rgb))
    return out


def flow_resize(src, size, mul_x=1.0, mul_y=1.0, out=None, src1=None, ctl=None):
    """Bilinear resize (align_corners=False) of float32 [B, C, Hs, Ws] to [B, C, Hd, Wd]; plane c is multiplied by mul_x (c
    even) or mul_y (c odd).  `src` / `out` may be channel-prefix views of wider contiguous [B, C', H, W] tensors.  With `ctl`
    (int32 [B, 4]) batch element b is read from `src1` when its record says its state is in buffer 1."""
    lib = _check(ctl)
    for t in (src, src1, out):
        if t is not None and (t.dim() != 4 or t.dtype != torch.float32 or t.stride(3) != 1 or t.stride(2) != t.shape[3]
                              or t.stride(1) != t.shape[2] * t.shape[3]):
            raise ValueError("flow_resize: float32 [B, C, H, W] with contiguous planes expected")
        if t is not None and not lib.is_emulator and not t.is_cuda:
            raise RuntimeError("SSN HIP ops need HIP (cuda) tensors; there is no CPU fallback")
    b, c, hs, ws = src.shape
    hd, wd = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((b, c, hd, wd), device=src.device, dtype=torch.float32)
    if out.shape != (b, c, hd, wd):
        raise ValueError("flow_resize: out must be [%d, %d, %d, %d]" % (b, c, hd, wd))
    if (ctl is None) != (src1 is None) or (src1 is not None and (src1.shape != src.shape or src1.stride() != src.stride())):
        raise ValueError("flow_resize: ctl and src1 come together, src1 laid out like src")
    if ctl is not None and (ctl.dtype != torch.int32 or ctl.shape != (b, 4)):
        raise ValueError("flow_resize: ctl must be int32 [B, 4]")
    lib.call("ssn_flow_resize", _p(src), _p(src1), _p(ctl), _p(out), b, c, src.stride(0), out.stride(0), hs, ws, hd, wd,
             float(mul_x), float(mul_y), _stream(lib, src))
    return out


def _tvl1_check(state, cst, ctl_in, ctl_out):
    if state.dim() != 5 or state.shape[0] != 2 or state.shape[2] != 6 or state.dtype != torch.float32:
        raise ValueError("tvl1: state must be float32 [2, B, 6, H, W]")
    b, h, w = state.shape[1], state.shape[3], state.shape[4]
    if cst.shape != (b, 4, h, w) or cst.dtype != torch.float32:
        raise ValueError("tvl1: cst must be float32 [B, 4, H, W]")
    for t in (ctl_in, ctl_out):
        if t is not None and (t.dtype != torch.int32 or t.shape != (b, 4)):
            raise ValueError("tvl1: a control record is int32 [B, 4]")
    return b, h, w


def tvl1_warp(i0, i1, state, cst, ctl_in, ctl_out):
    """ssn_tvl1_warp: start a warp of every pair.  i0, i1 float32 [B, H, W]; state [2, B, 6, H, W]; cst [B, 4, H, W] (written);
    ctl_in None: the state is in state[0]."""
    lib = _check(i0, i1, state, cst, ctl_in, ctl_out)
    b, h, w = _tvl1_check(state, cst, ctl_in, ctl_out)
    if i0.shape != (b, h, w) or i1.shape != (b, h, w) or i0.dtype != torch.float32 or i1.dtype != torch.float32:
        raise ValueError("tvl1_warp: images must be float32 [B, H, W]")
    lib.call("ssn_tvl1_warp", _p(i0), _p(i1), _p(state[0]), _p(state[1]), _p(cst), _p(ctl_in), _p(ctl_out), b, h, w,
             _stream(lib, state))


def tvl1_iterate(state, cst, n_iter, l_t, theta, taut, err_thresh, ctl_in, ctl_out, part_in, part_out, iters):
    """ssn_tvl1_iterate: n_iter iterations of every pair that is not done (see include/ssn_hip.h).  part_in / part_out float32
    [B, tiles] or None; iters int32 [B]."""
    lib = _check(state, cst, ctl_in, ctl_out, part_in, part_out, iters)
    b, h, w = _tvl1_check(state, cst, ctl_in, ctl_out)
    th, tw, _ = tvl1_tile_shape()
    tiles = -(-h // th) * -(-w // tw)
    for t in (part_in, part_out):
        if t is not None and (t.dtype != torch.float32 or t.shape != (b, tiles)):
            raise ValueError("tvl1_iterate: error partials must be float32 [%d, %d]" % (b, tiles))
    if iters.dtype != torch.int32 or iters.shape != (b,):
        raise ValueError("tvl1_iterate: iters must be int32 [B]")
    lib.call("ssn_tvl1_iterate", _p(state[0]), _p(state[1]), _p(cst), b, h, w, int(n_iter), float(l_t), float(theta), float(taut),
             float(err_thresh), _p(ctl_in), _p(ctl_out), _p(part_in), _p(part_out), _p(iters), _stream(lib, state))


def flow_quantize(flow, bound):
    """dense_flow's CAST: float32 flow -> uint8 of the same shape."""
    lib = _check(flow)
    if flow.dtype != torch.float32:
        raise ValueError("flow_quantize: float32 expected")
    out = torch.empty(flow.shape, device=flow.device, dtype=torch.uint8)
    n = flow.numel()
    lib.call("ssn_flow_quantize", _p(flow) if n else None, _p(out) if n else None, n, float(bound), _stream(lib, flow))
    return out


# ------------------------------------------------------------------------------------ baseline JPEG decoding (csrc/jpeg.hip)
def jpeg_layout():
    """(desc_ints, unit_ints, table_words, lds_sets): row sizes of the tables jpeg_decode.py builds, and the table sets a workgroup
    of ssn_jpeg_entropy holds."""
    lib = _lib.get_lib()
    v = [ctypes.c_int() for _ in range(4)]
    lib.call("ssn_jpeg_layout", *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def _jpeg_desc(desc):
    if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != jpeg_layout()[0] or desc.shape[0] < 1:
        raise ValueError("jpeg: desc must be int32 [images, %d]" % jpeg_layout()[0])
    return desc.shape[0]


def jpeg_entropy(bits, desc, units, tables, coef, status):
    """ssn_jpeg_entropy: bits uint8 [bytes]; desc int32 [images, desc_ints]; units int32 [64 k, unit_ints]; tables int32
    [sets, 4, table_words]; coef int16 [blocks, 64] and status int32 [images] are zeroed, then written."""
    lib = _check(bits, desc, units, tables, coef, status)
    n = _jpeg_desc(desc)
    _, unit_ints, table_words, _ = jpeg_layout()
    if bits.dtype != torch.uint8 or bits.dim() != 1:
        raise ValueError("jpeg_entropy: bits must be uint8 [bytes]")
    if units.dtype != torch.int32 or units.dim() != 2 or units.shape[1] != unit_ints or units.shape[0] < 64 or units.shape[0] % 64:
        raise ValueError("jpeg_entropy: units must be int32 [64 k, %d]" % unit_ints)
    if tables.dtype != torch.int32 or tables.dim() != 3 or tables.shape[1:] != (4, table_words) or tables.shape[0] < 1:
        raise ValueError("jpeg_entropy: tables must be int32 [sets, 4, %d]" % table_words)
    if coef.dtype != torch.int16 or coef.dim() != 2 or coef.shape[1] != 64 or coef.shape[0] < 1:
        raise ValueError("jpeg_entropy: coef must be int16 [blocks, 64]")
    if status.dtype != torch.int32 or status.shape != (n,):
        raise ValueError("jpeg_entropy: status must be int32 [images]")
    lib.call("ssn_jpeg_entropy", _p(bits) if bits.numel() else None, bits.numel(), _p(desc), n, _p(units), units.shape[0], _p(tables),
             tables.shape[0], _p(coef), coef.shape[0], _p(status), _stream(lib, coef))


def jpeg_idct(coef, desc, max_blocks, quant, planes):
    """ssn_jpeg_idct: coef int16 [blocks, 64]; quant int16 [n, 64] (the 8-bit tables, natural order); planes uint8 [bytes] (written)."""
    lib = _check(coef, desc, quant, planes)
    n = _jpeg_desc(desc)
    if coef.dtype != torch.int16 or coef.dim() != 2 or coef.shape[1] != 64 or coef.shape[0] < 1:
        raise ValueError("jpeg_idct: coef must be int16 [blocks, 64]")
    if quant.dtype != torch.int16 or quant.dim() != 2 or quant.shape[1] != 64 or quant.shape[0] < 1:
        raise ValueError("jpeg_idct: quant must be int16 [n, 64]")
    if planes.dtype != torch.uint8 or planes.dim() != 1 or planes.numel() < 64 or planes.data_ptr() % 8:
        raise ValueError("jpeg_idct: planes must be uint8 [bytes], 8-byte aligned, at least one block")
    if int(max_blocks) < 1:
        raise ValueError("jpeg_idct: max_blocks must be positive")
    lib.call("ssn_jpeg_idct", _p(coef), coef.shape[0], _p(desc), n, int(max_blocks), _p(quant), quant.shape[0], _p(planes),
             planes.numel(), _stream(lib, planes))


def jpeg_pixels(planes, desc, max_pixels, out_c, out):
    """ssn_jpeg_pixels: planes uint8 [bytes]; out uint8 [bytes] (written: [H, W, out_c] per image at its offset)."""
    lib = _check(planes, desc, out)
    n = _jpeg_desc(desc)
    if planes.dtype != torch.uint8 or planes.dim() != 1 or planes.numel() < 64:
        raise ValueError("jpeg_pixels: planes must be uint8 [bytes]")
    if out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < 1:
        raise ValueError("jpeg_pixels: out must be uint8 [bytes]")
    if out_c not in (1, 3) or int(max_pixels) < 1:
        raise ValueError("jpeg_pixels: out_c is 1 or 3, max_pixels positive")
    lib.call("ssn_jpeg_pixels", _p(planes), planes.numel(), _p(desc), n, int(max_pixels), int(out_c), _p(out), out.numel(),
             _stream(lib, out))


def jpeg_index(bits, desc, units, refused):
    """ssn_jpeg_index: bits uint8 [bytes], 16-byte aligned, every file from its first scan byte to its end; desc int32 [images,
    desc_ints] with columns 15 .. 18 (first byte, end byte, first unit row, units) filled; units int32 [64 k, unit_ints] (begin / end
    of the files' rows are written); refused int32 [images] (written: 16 or 0)."""
    lib = _check(bits, desc, units, refused)
    n = _jpeg_desc(desc)
    unit_ints = jpeg_layout()[1]
    if bits.dtype != torch.uint8 or bits.dim() != 1 or bits.numel() >= 1 << 31:
        raise ValueError("jpeg_index: bits must be uint8 [bytes], less than 2 GiB")
    if bits.numel() and bits.data_ptr() % 16:
        raise ValueError("jpeg_index: bits must be 16-byte aligned")
    if units.dtype != torch.int32 or units.dim() != 2 or units.shape[1] != unit_ints or units.shape[0] < 64 or units.shape[0] % 64:
        raise ValueError("jpeg_index: units must be int32 [64 k, %d]" % unit_ints)
    if refused.dtype != torch.int32 or refused.shape != (n,):
        raise ValueError("jpeg_index: refused must be int32 [images]")
    lib.call("ssn_jpeg_index", _p(bits) if bits.numel() else None, bits.numel(), _p(desc), n, _p(units), units.shape[0], _p(refused),
             _stream(lib, units))


def jpeg_index_status(refused, status):
    """ssn_jpeg_index_status: status |= refused, both int32 [images]; after jpeg_entropy, which zeroes status."""
    lib = _check(refused, status)
    if refused.dtype != torch.int32 or status.dtype != torch.int32 or refused.dim() != 1 or refused.shape != status.shape or not refused.numel():
        raise ValueError("jpeg_index_status: refused and status must be int32 [images]")
    lib.call("ssn_jpeg_index_status", _p(refused), _p(status), refused.numel(), _stream(lib, status))


# ------------------------------------------------------------------------------------ baseline JPEG encoding (csrc/jpeg_encode.hip)
def jpeg_enc_layout():
    """(desc_ints, block_bits): ints of a desc row jpeg_encode.py builds, and the most bits the codes of one block take."""
    lib = _lib.get_lib()
    v = [ctypes.c_int() for _ in range(2)]
    lib.call("ssn_jpeg_enc_layout", *[ctypes.byref(x) for x in v])
    return tuple(x.value for x in v)


def _jpeg_enc_common(who, desc, coef=None, tables=None, blkbits=None, ivals=None, rawlen=None, status=None, raw=None):
    """Shape and dtype checks the encoder wrappers share -> number of images."""
    if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != jpeg_enc_layout()[0] or not 1 <= desc.shape[0] <= 65535:
        raise ValueError("%s: desc must be int32 [images, %d], 1 .. 65535 images" % (who, jpeg_enc_layout()[0]))
    n = desc.shape[0]
    if coef is not None and (coef.dtype != torch.int16 or coef.dim() != 2 or coef.shape[1] != 64 or not 1 <= coef.shape[0] < (1 << 25)
                             or coef.data_ptr() % 4):
        raise ValueError("%s: coef must be int16 [blocks, 64], fewer than 2^25 blocks" % who)
    if tables is not None and (tables.dtype != torch.int32 or tuple(tables.shape) != (4, 256)):
        raise ValueError("%s: tables must be int32 [4, 256]" % who)
    if blkbits is not None and (blkbits.dtype != torch.int32 or blkbits.dim() != 1 or (coef is not None and blkbits.shape[0] != coef.shape[0])
                                or not 1 <= blkbits.shape[0] < (1 << 25)):
        raise ValueError("%s: blkbits must be int32 [blocks]" % who)
    if ivals is not None and (ivals.dtype != torch.int32 or ivals.dim() != 1 or ivals.shape[0] < 1):
        raise ValueError("%s: ivals must be int32 [intervals]" % who)
    for name, t in (("rawlen", rawlen), ("status", status)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (n,)):
            raise ValueError("%s: %s must be int32 [images]" % (who, name))
    if raw is not None and (raw.dtype != torch.uint8 or raw.dim() != 1 or raw.numel() < 4 or raw.numel() % 4 or raw.numel() >= (1 << 31)
                            or raw.data_ptr() % 4):
        raise ValueError("%s: raw must be uint8 [bytes], a multiple of 4 below 2^31, 4-byte aligned" % who)
    return n


def jpeg_enc_blocks(pix, desc, max_blocks, quant, coef):
    """ssn_jpeg_enc_blocks: pix uint8 [bytes]; quant int16 [2, 64] (natural order, 1 .. 255); coef int16 [blocks, 64] (written)."""
    lib = _check(pix, desc, quant, coef)
    n = _jpeg_enc_common("jpeg_enc_blocks", desc, coef=coef)
    if pix.dtype != torch.uint8 or pix.dim() != 1 or not 1 <= pix.numel() < (1 << 31):
        raise ValueError("jpeg_enc_blocks: pix must be uint8 [bytes], fewer than 2^31")
    if quant.dtype != torch.int16 or tuple(quant.shape) != (2, 64):
        raise ValueError("jpeg_enc_blocks: quant must be int16 [2, 64]")
    if int(max_blocks) < 1:
        raise ValueError("jpeg_enc_blocks: max_blocks must be positive")
    lib.call("ssn_jpeg_enc_blocks", _p(pix), pix.numel(), _p(desc), n, int(max_blocks), _p(quant), _p(coef), coef.shape[0], _stream(lib, coef))


def jpeg_enc_count(coef, desc, max_blocks, tables, blkbits, status):
    """ssn_jpeg_enc_count: status int32 [images] is zeroed; blkbits int32 [blocks] (written)."""
    lib = _check(coef, desc, tables, blkbits, status)
    n = _jpeg_enc_common("jpeg_enc_count", desc, coef=coef, tables=tables, blkbits=blkbits, status=status)
    if int(max_blocks) < 1:
        raise ValueError("jpeg_enc_count: max_blocks must be positive")
    lib.call("ssn_jpeg_enc_count", _p(coef), coef.shape[0], _p(desc), n, int(max_blocks), _p(tables), _p(blkbits), _p(status),
             _stream(lib, coef))


def jpeg_enc_scan(desc, blkbits, ivals, rawlen, status):
    """ssn_jpeg_enc_scan: blkbits -> bit offsets in place; ivals int32 [intervals] and rawlen int32 [images] (written)."""
    lib = _check(desc, blkbits, ivals, rawlen, status)
    n = _jpeg_enc_common("jpeg_enc_scan", desc, blkbits=blkbits, ivals=ivals, rawlen=rawlen, status=status)
    if ivals.shape[0] > blkbits.shape[0]:
        raise ValueError("jpeg_enc_scan: more intervals than blocks")
    lib.call("ssn_jpeg_enc_scan", _p(desc), n, _p(blkbits), blkbits.shape[0], _p(ivals), ivals.shape[0], _p(rawlen), _p(status),
             _stream(lib, blkbits))


def jpeg_enc_pack(coef, desc, max_blocks, tables, blkbits, ivals, rawlen, raw, status):
    """ssn_jpeg_enc_pack: raw uint8 [bytes] is zeroed, then written."""
    lib = _check(coef, desc, tables, blkbits, ivals, rawlen, raw, status)
    n = _jpeg_enc_common("jpeg_enc_pack", desc, coef=coef, tables=tables, blkbits=blkbits, ivals=ivals, rawlen=rawlen, status=status, raw=raw)
    if int(max_blocks) < 1:
        raise ValueError("jpeg_enc_pack: max_blocks must be positive")
    lib.call("ssn_jpeg_enc_pack", _p(coef), coef.shape[0], _p(desc), n, int(max_blocks), _p(tables), _p(blkbits), _p(ivals), ivals.shape[0],
             _p(rawlen), _p(raw), raw.numel(), _p(status), _stream(lib, raw))


def jpeg_enc_assemble(raw, desc, ivals, rawlen, headers, ffcount, data, offsets, lengths, status):
    """ssn_jpeg_enc_assemble: headers uint8 [bytes]; ffcount int32 [images] (scratch); data uint8 [bytes], offsets int64 [images] and
    lengths int32 [images] (written)."""
    lib = _check(raw, desc, ivals, rawlen, headers, ffcount, data, offsets, lengths, status)
    n = _jpeg_enc_common("jpeg_enc_assemble", desc, ivals=ivals, rawlen=rawlen, status=status, raw=raw)
    if headers.dtype != torch.uint8 or headers.dim() != 1 or headers.numel() < 1:
        raise ValueError("jpeg_enc_assemble: headers must be uint8 [bytes]")
    if data.dtype != torch.uint8 or data.dim() != 1 or data.numel() < 1:
        raise ValueError("jpeg_enc_assemble: data must be uint8 [bytes]")
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (n,):
        raise ValueError("jpeg_enc_assemble: offsets must be int64 [images]")
    for name, t in (("ffcount", ffcount), ("lengths", lengths)):
        if t.dtype != torch.int32 or tuple(t.shape) != (n,):
            raise ValueError("jpeg_enc_assemble: %s must be int32 [images]" % name)
    lib.call("ssn_jpeg_enc_assemble", _p(raw), raw.numel(), _p(desc), n, _p(ivals), ivals.shape[0], _p(rawlen), _p(headers), headers.numel(),
             _p(ffcount), _p(data), data.numel(), _p(offsets), _p(lengths), _p(status), _stream(lib, data))


# ------------------------------------------------------------------------------------ lossless JPEG transcoding (csrc/jpeg_transcode.hip)
def jpeg_transcode_layout():
    """ints of a desc row jpeg_transcode.py builds: ncomp, hs, vs, mcux, mcuy, first source block, first destination block, blocks."""
    lib = _lib.get_lib()
    v = ctypes.c_int()
    lib.call("ssn_jpeg_transcode_layout", ctypes.byref(v))
    return v.value


def jpeg_transcode_blocks(src, desc, max_blocks, dst, status):
    """ssn_jpeg_transcode_blocks: src int16 [blocks, 64] (what jpeg_entropy writes: natural order, planar blocks); dst int16
    [blocks, 64] (written: what jpeg_enc_count reads: zigzag order, blocks in scan order); status int32 [images] is zeroed, bit 4 marks
    an unusable desc row."""
    lib = _check(src, desc, dst, status)
    ints = jpeg_transcode_layout()
    if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != ints or not 1 <= desc.shape[0] <= 65535:
        raise ValueError("jpeg_transcode_blocks: desc must be int32 [images, %d], 1 .. 65535 images" % ints)
    for name, t in (("src", src), ("dst", dst)):
        if t.dtype != torch.int16 or t.dim() != 2 or t.shape[1] != 64 or not 1 <= t.shape[0] < (1 << 25) or t.data_ptr() % 16:
            raise ValueError("jpeg_transcode_blocks: %s must be int16 [blocks, 64], fewer than 2^25 blocks, 16-byte aligned" % name)
    if src.data_ptr() == dst.data_ptr():
        raise ValueError("jpeg_transcode_blocks: src and dst must be different buffers")
    if status.dtype != torch.int32 or tuple(status.shape) != (desc.shape[0],):
        raise ValueError("jpeg_transcode_blocks: status must be int32 [images]")
    if int(max_blocks) < 1:
        raise ValueError("jpeg_transcode_blocks: max_blocks must be positive")
    lib.call("ssn_jpeg_transcode_blocks", _p(src), src.shape[0], _p(desc), desc.shape[0], int(max_blocks), _p(dst), dst.shape[0],
             _p(status), _stream(lib, dst))


# ------------------------------------------------------------------------------------ gray JPEG round trip (csrc/jpeg_roundtrip.hip)
def jpeg_roundtrip_gray(src, quant64, out=None):
    """ssn_jpeg_roundtrip_gray: src uint8 [N, H, W]; quant64 int32 [64] on the device (natural order, 1 .. 255); out uint8 [N, H, W]
    (written; may be src itself; allocated when None) -> out."""
    if out is None:
        out = torch.empty_like(src)
    lib = _check(src, quant64, out)
    if src.dtype != torch.uint8 or src.dim() != 3 or min(src.shape) < 1 or src.shape[1] > 65535 or src.shape[2] > 65535:
        raise ValueError("jpeg_roundtrip_gray: src must be uint8 [N, H, W], N >= 1, H and W 1 .. 65535")
    if out.dtype != torch.uint8 or out.shape != src.shape or out.device != src.device:
        raise ValueError("jpeg_roundtrip_gray: out must be uint8 of src's shape on src's device")
    if quant64.dtype != torch.int32 or tuple(quant64.shape) != (64,) or quant64.device != src.device:
        raise ValueError("jpeg_roundtrip_gray: quant64 must be int32 [64] on src's device")
    n, h, w = src.shape
    if n >= 1 << 31:
        raise ValueError("jpeg_roundtrip_gray: too many images")
    lib.call("ssn_jpeg_roundtrip_gray", _p(src), _p(out), n, h, w, _p(quant64), _stream(lib, out))
    return out
