"""A plain numpy baseline JPEG encoder, written the way libjpeg is organised (whole component planes: convert, pad, downsample,
pad, transform; then one sequential Huffman pass over the MCUs) and sharing no code with the product, which works block by block.
It takes the Annex K tables from the yardstick itself: from the DQT / DHT segments of a quality-50 file PIL writes (at quality 50
the scale factor is 100 %, so the quantisation tables in the file ARE the base tables).  tests/test_jpeg_encode.py first holds it
against PIL on every file of its grid; only then does it referee the stages.
"""
import functools
import io

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
FACTORS = {None: (1, 1), 0: (1, 1), 1: (2, 1), 2: (2, 2)}


@functools.lru_cache(maxsize=None)
def annex_k():
    """-> (base quantisation tables [luma, chroma] in natural order, {(class, id): (counts, symbols)}) read from a PIL file."""
    from PIL import Image
    b = io.BytesIO()
    Image.new("RGB", (8, 8)).save(b, "JPEG", quality=50)
    data = b.getvalue()
    quant, huff, p = {}, {}, 2
    while data[p + 1] != 0xDA:
        length = (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + length]
        if data[p + 1] == 0xDB:
            while seg:
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(seg[1:65])
                quant[seg[0] & 15] = t
                seg = seg[65:]
        elif data[p + 1] == 0xC4:
            while seg:
                counts = list(seg[1:17])
                huff[(seg[0] >> 4, seg[0] & 15)] = (counts, list(seg[17:17 + sum(counts)]))
                seg = seg[17 + sum(counts):]
        p += 2 + length
    return [quant[0], quant[1]], huff


def quant_tables(quality):
    base, _ = annex_k()
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((b * scale + 50) // 100, 1, 255) for b in base]


@functools.lru_cache(maxsize=None)
def codes(cls, ident):
    """{symbol: (code, length)} of a standard table."""
    counts, symbols = annex_k()[1][(cls, ident)]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def planes(a, hs, vs):
    """The component planes libjpeg hands to its transform: [(plane, real blocks across, real blocks down)], luma first."""
    a = np.asarray(a).astype(np.int64)
    if a.ndim == 2 or a.shape[2] == 1:
        comps = [a.reshape(a.shape[0], a.shape[1])]
    else:
        r, g, b = a[:, :, 0], a[:, :, 1], a[:, :, 2]
        comps = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                 (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                 (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]
    h, w = comps[0].shape
    out = []
    for c, p in enumerate(comps):
        fh, fv = (1, 1) if c == 0 else (hs, vs)                  # how much this component is reduced
        bw, bh = -(-w // (8 * fh)), -(-h // (8 * fv))            # its real blocks
        p = np.pad(p, ((0, -h % fv), (0, bw * 8 * fh - w)), mode="edge")
        if fh == 2 and fv == 2:
            bias = np.tile([1, 2], p.shape[1] // 4 + 1)[:p.shape[1] // 2]
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif fh == 2:
            bias = np.tile([0, 1], p.shape[1] // 4 + 1)[:p.shape[1] // 2]
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        p = np.pad(p, ((0, bh * 8 - p.shape[0]), (0, 0)), mode="edge")
        out.append((p, bw, bh))
    return out


def _pass(d, first):
    """jfdctint.c, one pass over the LAST axis of d [..., 8]."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15

    def descale(x, bits):
        return (x + (1 << (bits - 1))) >> bits
    o = np.zeros_like(d)
    if first:
        o[..., 0], o[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[..., 0], o[..., 4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[..., 2], o[..., 6] = descale(z1 + t13 * 6270, n), descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7], o[..., 5], o[..., 3], o[..., 1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return o


def transform(plane, q):
    """plane [8 bh, 8 bw] -> quantised coefficients [bh, bw, 64] in zigzag order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    d = _pass(d, True)                                            # rows
    d = _pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)      # columns
    d = d.reshape(bh, bw, 64)
    c = np.sign(d) * ((np.abs(d) + 4 * q) // (8 * q))
    return c[:, :, ZIGZAG]


def coefficients(a, quality, subsampling):
    """int16 [blocks, 64]: zigzag rows in the scan's MCU order, dummy blocks included -> (coef, mcux, mcuy, ncomp, hs, vs)."""
    a = np.asarray(a)
    ncomp = 1 if a.ndim == 2 or a.shape[2] == 1 else 3
    hs, vs = FACTORS[subsampling] if ncomp == 3 else (1, 1)
    q = quant_tables(quality)
    comps = [(transform(p, q[0 if c == 0 else 1]), bw, bh) for c, (p, bw, bh) in enumerate(planes(a, hs, vs))]
    h, w = a.shape[:2]
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    rows = []
    for my in range(mcuy):
        for mx in range(mcux):
            for c, (co, bw, bh) in enumerate(comps):
                nh, nv = (hs, vs) if c == 0 else (1, 1)
                for v in range(nv):
                    for u in range(nh):
                        bx, by = mx * nh + u, my * nv + v
                        if bx < bw and by < bh:
                            rows.append(co[by, bx])
                        else:                                     # a dummy block: the DC of the block written just before it
                            d = np.zeros(64, np.int64)
                            d[0] = rows[-1][0]
                            rows.append(d)
    return np.array(rows).astype(np.int16), mcux, mcuy, ncomp, hs, vs


def _size(v):
    return int(abs(int(v))).bit_length()


def scan(coef, ncomp, hs, vs, restart=0):
    """The entropy-coded data of coef [blocks, 64] (MCU order) -> (bytes with stuffing and RSTn, [(table class, symbol, code length)])."""
    bpm = 1 if ncomp == 1 else hs * vs + 2
    nmcu = len(coef) // bpm
    out, symbols = bytearray(), []
    acc = nbits = 0

    def put(value, length):
        nonlocal acc, nbits
        acc, nbits = (acc << length) | value, nbits + length

    def flush():
        nonlocal acc, nbits
        if nbits % 8:
            put((1 << (-nbits % 8)) - 1, -nbits % 8)
        for byte in acc.to_bytes(nbits // 8, "big"):
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
        acc = nbits = 0
    pred = [0, 0, 0]
    for m in range(nmcu):
        if restart and m and m % restart == 0:
            flush()
            out.extend([0xFF, 0xD0 + (m // restart - 1) % 8])
            pred = [0, 0, 0]
        for j in range(bpm):
            c = 0 if ncomp == 1 or j < hs * vs else j - hs * vs + 1
            dc, ac = codes(0, min(c, 1)), codes(1, min(c, 1))
            blk = [int(x) for x in coef[m * bpm + j]]
            diff, pred[c] = blk[0] - pred[c], blk[0]
            s = _size(diff)
            put(*dc[s])
            symbols.append((0, s, dc[s][1]))
            if s:
                put((diff if diff > 0 else diff - 1) & ((1 << s) - 1), s)
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    put(*ac[0xF0])
                    symbols.append((1, 0xF0, ac[0xF0][1]))
                    run -= 16
                s = _size(v)
                put(*ac[(run << 4) | s])
                symbols.append((1, (run << 4) | s, ac[(run << 4) | s][1]))
                put((v if v > 0 else v - 1) & ((1 << s) - 1), s)
                run = 0
            if run:
                put(*ac[0])
                symbols.append((1, 0, ac[0][1]))
    flush()
    return bytes(out), symbols


def _segment(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def header(w, h, ncomp, hs, vs, quality, restart=0):
    q, (_, huff) = quant_tables(quality), annex_k()
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(1 if ncomp == 1 else 2):
        out += _segment(0xDB, [t] + [int(q[t][z]) for z in ZIGZAG])
    sof = [8, h >> 8, h & 255, w >> 8, w & 255, ncomp, 1, (hs << 4) | vs, 0]
    sos = [ncomp, 1, 0x00]
    if ncomp == 3:
        sof += [2, 0x11, 1, 3, 0x11, 1]
        sos += [2, 0x11, 3, 0x11]
    out += _segment(0xC0, sof)
    for ident in range(1 if ncomp == 1 else 2):
        for cls in (0, 1):
            counts, symbols = huff[(cls, ident)]
            out += _segment(0xC4, [(cls << 4) | ident] + counts + symbols)
    if restart:
        out += _segment(0xDD, [restart >> 8, restart & 255])
    return out + _segment(0xDA, sos + [0, 63, 0])


def encode(a, quality, subsampling=None, restart=0):
    """The whole file, as bytes."""
    a = np.asarray(a)
    coef, _, _, ncomp, hs, vs = coefficients(a, quality, subsampling)
    body, _ = scan(coef, ncomp, hs, vs, restart)
    return header(a.shape[1], a.shape[0], ncomp, hs, vs, quality, restart) + body + b"\xff\xd9"


def symbols_of(a, quality, subsampling=None, restart=0):
    coef, _, _, ncomp, hs, vs = coefficients(a, quality, subsampling)
    return scan(coef, ncomp, hs, vs, restart)[1]
