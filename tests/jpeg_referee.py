"""A plain numpy restatement of a baseline JPEG decoder, the referee of tests/test_jpeg_decode.py.

It shares no code with action_detection_amd/jpeg_decode.py or csrc/jpeg.hip: its own marker walk, a bit-by-bit Huffman decoder
(the canonical mincode / maxcode / valptr procedure of ITU-T T.81 annex F.2.2.3), the "islow" inverse DCT (13-bit constants, two
passes, descales of 11 and 18 bits), libjpeg's "fancy" triangle upsampling and its 16-bit fixed-point colour conversion.  The
stages are separate functions so that a test can compare the coefficients, the component planes and the pixels one by one:

    hdr = parse(data)            marker walk -> Header
    coefs = entropy(data, hdr)   [component] -> int16 [blocks down, blocks across, 64] in natural order
    planes = idct_planes(hdr, coefs)   [component] -> uint8 [8 * blocks down, 8 * blocks across] (padded to whole MCUs)
    pixels(hdr, planes, mode)    uint8 [H, W, 3] ("RGB") or [H, W] ("L"), what PIL's .convert(mode) gives

tests/test_jpeg_decode.py first holds it against PIL on every file it later referees.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


class Header(object):
    pass


def parse(data):
    """Marker walk of a baseline file with one interleaved scan."""
    h = Header()
    h.qt, h.dc, h.ac, h.restart = {}, {}, {}, 0
    assert data[:2] == b"\xff\xd8"
    p = 2
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        n = (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + n]
        if m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                h.qt[seg[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                vals = list(seg[q + 17:q + 17 + sum(counts)])
                (h.ac if seg[q] >> 4 else h.dc)[seg[q] & 15] = (counts, vals)
                q += 17 + sum(counts)
        elif m == 0xC0:
            assert seg[0] == 8
            h.height, h.width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            h.comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
        elif m == 0xDD:
            h.restart = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            assert seg[0] == len(h.comps)
            h.sel = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
            h.scan = p + 2 + n
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not baseline"
        p += 2 + n
    if len(h.comps) == 1:
        h.comps = [(h.comps[0][0], 1, 1, h.comps[0][3])]      # a one-component scan is not interleaved: its factors do not matter
    h.hmax, h.vmax = max(c[1] for c in h.comps), max(c[2] for c in h.comps)
    h.mcux, h.mcuy = -(-h.width // (8 * h.hmax)), -(-h.height // (8 * h.vmax))
    return h


class _Bits(object):
    def __init__(self, data, pos):
        self.data, self.pos, self.acc, self.n = data, pos, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.data[self.pos]
            self.pos += 1
            if b == 0xFF:
                assert self.data[self.pos] == 0, "marker inside a restart interval"
                self.pos += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def restart(self, number):
        self.n = 0
        assert self.data[self.pos] == 0xFF and self.data[self.pos + 1] == 0xD0 + (number & 7)
        self.pos += 2


def _canonical(counts, vals):
    """{(length, code): symbol}"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _symbol(bits, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | bits.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise AssertionError("undefined Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def entropy(data, h):
    coefs = [np.zeros((h.mcuy * v, h.mcux * hh, 64), np.int16) for _, hh, v, _ in h.comps]
    dc = [_canonical(*h.dc[s[0]]) for s in h.sel]
    ac = [_canonical(*h.ac[s[1]]) for s in h.sel]
    bits = _Bits(data, h.scan)
    pred = [0] * len(h.comps)
    for m in range(h.mcux * h.mcuy):
        if h.restart and m and m % h.restart == 0:
            bits.restart(m // h.restart - 1)
            pred = [0] * len(h.comps)
        my, mx = divmod(m, h.mcux)
        for c, (_, hh, v, _) in enumerate(h.comps):
            for by in range(v):
                for bx in range(hh):
                    blk = coefs[c][my * v + by, mx * hh + bx]
                    s = _symbol(bits, dc[c])
                    pred[c] += _extend(bits.bits(s), s)
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = _symbol(bits, ac[c])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        blk[ZIGZAG[k]] = _extend(bits.bits(s), s)
                        k += 1
    return coefs


def _idct_pass(x, shift):
    """One pass of jidctint.c's jpeg_idct_islow over axis 0 of int32 x [8, ...]."""
    x = x.astype(np.int64)
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[0] + x[4]) << 13
    tmp1 = (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3])
    return ((out + (1 << (shift - 1))) >> shift).astype(np.int32)


def idct_planes(h, coefs):
    planes = []
    for (_, _, _, tq), cf in zip(h.comps, coefs):
        bh, bw, _ = cf.shape
        x = cf.astype(np.int32) * h.qt[tq]                       # [bh, bw, 64]
        x = x.reshape(bh, bw, 8, 8).transpose(2, 3, 0, 1)         # [row, col, bh, bw]
        ws = _idct_pass(x, 11)                                    # columns: along the rows axis
        px = _idct_pass(ws.transpose(1, 0, 2, 3), 18)             # rows: along the columns axis -> [col, row, bh, bw]
        px = np.clip(px + 128, 0, 255).astype(np.uint8)
        planes.append(px.transpose(2, 1, 3, 0).reshape(bh * 8, bw * 8))
    return planes


def _upsample(plane, hh, v, h):
    """libjpeg's fancy upsampling of a chroma plane (factors 1 x 1) to the luma grid (hmax x vmax), from its true extent."""
    cw, ch = -(-h.width * hh // h.hmax), -(-h.height * v // h.vmax)
    s = plane[:ch, :cw].astype(np.int32)
    fx, fy = h.hmax // hh, h.vmax // v
    if fx == 1 and fy == 1:
        return s
    if cw <= 2:                                                   # jdsample.c: the triangle filter needs more than two columns
        return np.repeat(np.repeat(s, fy, axis=0), fx, axis=1)
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    if fy == 1:
        out = np.empty((ch, 2 * cw), np.int32)
        out[:, 0::2] = (3 * s + left + 1) >> 2
        out[:, 1::2] = (3 * s + right + 2) >> 2
        return out
    out = np.empty((2 * ch, 2 * cw), np.int32)
    up = np.concatenate([s[:1], s[:-1]], axis=0)
    down = np.concatenate([s[1:], s[-1:]], axis=0)
    for row, far in ((0, up), (1, down)):
        col = 3 * s + far
        cl = np.concatenate([col[:, :1], col[:, :-1]], axis=1)
        cr = np.concatenate([col[:, 1:], col[:, -1:]], axis=1)
        out[row::2, 0::2] = (3 * col + cl + 8) >> 4
        out[row::2, 1::2] = (3 * col + cr + 7) >> 4
    return out


def pixels(h, planes, mode="RGB"):
    H, W = h.height, h.width
    y = planes[0][:H, :W].astype(np.int32)
    if len(planes) == 1:
        g = y.astype(np.uint8)
        return g if mode == "L" else np.repeat(g[:, :, None], 3, axis=2)
    cb = _upsample(planes[1], h.comps[1][1], h.comps[1][2], h)[:H, :W] - 128
    cr = _upsample(planes[2], h.comps[2][1], h.comps[2][2], h)[:H, :W] - 128
    r = np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255)
    g = np.clip(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255)
    b = np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)
    if mode == "L":
        return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).astype(np.uint8)
    return np.stack([r, g, b], axis=2).astype(np.uint8)


def decode(data, mode="RGB"):
    h = parse(data)
    return pixels(h, idct_planes(h, entropy(data, h)), mode)
