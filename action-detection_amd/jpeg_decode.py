"""Baseline JPEG decoding on the device: the first thing every stage of the workflow does with a frame, which the reference does
with PIL in its loader workers (``Image.open(path).convert('RGB')``, ssn_dataset.py:208-215 of the reference).

The host only walks the markers (``parse_jpeg``): sizes, sampling, quantisation and Huffman tables, and the byte range of every
restart interval.  ``JpegDecoder.decode`` uploads the scans of a batch of files and the tables that describe them in ONE copy and
enqueues three launches (csrc/jpeg.hip: entropy decode, inverse DCT, upsample + colour conversion + crop) on the caller's stream,
without a host read.  Files the kernels do not take (progressive, CMYK, 4:1:1, ...) are decoded by PIL on the host and uploaded
instead; ``JpegDecoder.fallbacks`` counts them.  The pixels are PIL's, bit for bit, for the libjpeg PIL links.
With ``JpegDecoder(index="device")`` the host reads the headers only (``parse_jpeg_header``) and a fourth launch in front of the
others (``ssn_jpeg_index``) finds the restart intervals in the uploaded bytes.
"""
import io
import re

import numpy as np
import torch

from . import kernels as K
from .input_pipeline import TrainingBatchPrefetcher

_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                    54, 47, 55, 62, 63])
_LUT_BITS = 9
_SOF_OTHER = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential", 0xC6: "differential progressive",
              0xC7: "differential lossless", 0xC9: "arithmetic coding", 0xCA: "arithmetic coding", 0xCB: "arithmetic coding",
              0xCD: "arithmetic coding", 0xCE: "arithmetic coding", 0xCF: "arithmetic coding"}


class JpegHeader(object):
    """What ``parse_jpeg`` found.  ``supported`` says whether the kernels take the file; ``reason`` why not.

    width, height; components [(id, h, v, quantisation table id)]; hs, vs: the luma sampling factors (1 x 1 for a gray file);
    qtables {id: uint16 [64], natural order}; huffman {(class, id): (counts bytes[16], symbols bytes)}; selectors [(dc id, ac id)]
    per component; restart_interval (MCUs, 0: none); scan (begin, end) byte range of the entropy-coded data; units [(begin, end,
    first MCU, MCUs)] one per restart interval (one for the whole scan without restart markers)."""

    def __init__(self):
        self.supported, self.reason = False, ""
        self.width = self.height = 0
        self.components, self.selectors, self.units = [], [], []
        self.qtables, self.huffman = {}, {}
        self.restart_interval, self.scan = 0, (0, 0)
        self.hs = self.vs = 1

    @property
    def mcus(self):
        return -(-self.width // (8 * self.hs)), -(-self.height // (8 * self.vs))

    def _no(self, reason):
        self.supported, self.reason = False, reason
        return self


def _check_huffman(counts, symbols, is_dc):
    """None if (counts, symbols) is a usable table, else the reason."""
    code = 0
    for length in range(1, 17):
        code += counts[length - 1]
        if code > (1 << length):
            return "Huffman table assigns more codes than %d bits hold" % length
        code <<= 1
    if is_dc and any(s > 15 for s in symbols):
        return "DC Huffman table with a category above 15"
    return None


_header_cache = {}
_MARKER = re.compile(b"\xff[^\x00\xff]")


def _scan_begin(data, n):
    """Offset of the first scan's entropy-coded data (segments skipped by their lengths), or -1."""
    p = 2
    while p + 4 <= n and data[p] == 0xFF:
        m = data[p + 1]
        if m == 0xFF:
            p += 1
        elif m == 0x01 or 0xD0 <= m <= 0xD7:
            p += 2
        else:
            p += 2 + ((data[p + 2] << 8) | data[p + 3])
            if m == 0xDA:
                return p if p <= n else -1
            if m == 0xD9:
                return -1
    return -1


def parse_jpeg(data):
    """Marker walk of one file (host only; every index is checked against ``len(data)``) -> ``JpegHeader``.  The frames of a data
    set share their headers byte for byte (one encoder, one size, one quality), so what the bytes in front of the scan say is
    kept per distinct header and only the scan is walked per file."""
    import copy
    data = bytes(data)
    n = len(data)
    begin = _scan_begin(data, n) if n >= 4 and data[0] == 0xFF and data[1] == 0xD8 else -1
    key = data[:begin] if begin > 0 else None
    h = _header_cache.get(key) if key is not None else None
    if h is None:
        h = _parse_header(data, n)
        if key is not None and h.supported:
            if len(_header_cache) > 256:
                _header_cache.clear()
            _header_cache[key] = h
    return _parse_scan(copy.copy(h), data, n, begin) if h.supported else h


_last_header = [None]      # (header bytes, JpegHeader) of the last supported file parse_jpeg_header saw


def parse_jpeg_header(data):
    """The header part of ``parse_jpeg`` without the scan walk -> ``JpegHeader`` with ``scan = (begin, len(data))`` and no units:
    what ``JpegDecoder(index="device")`` needs of the host (the kernel finds the restart intervals and the scan's end).  The last
    header is tried first: a file that starts with the very bytes of that header, up to and including its SOS segment, has that
    header, and costs one comparison instead of a segment walk."""
    import copy
    data = bytes(data)
    n = len(data)
    last = _last_header[0]
    if last is not None and data.startswith(last[0]):
        h = copy.copy(last[1])
        h.scan, h.units = (len(last[0]), n), []
        return h
    begin = _scan_begin(data, n) if n >= 4 and data[0] == 0xFF and data[1] == 0xD8 else -1
    key = data[:begin] if begin > 0 else None
    h = _header_cache.get(key) if key is not None else None
    if h is None:
        h = _parse_header(data, n)
        if key is not None and h.supported:
            if len(_header_cache) > 256:
                _header_cache.clear()
            _header_cache[key] = h
    if not h.supported:
        return h
    if key is None:
        return copy.copy(h)._no("no scan")
    _last_header[0] = (key, h)
    h = copy.copy(h)
    h.scan, h.units = (begin, n), []
    return h


def _parse_header(data, n):
    h = JpegHeader()
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return h._no("not a JPEG file (no SOI marker)")
    p, sof, jfif, adobe = 2, False, False, None
    while True:
        if p + 4 > n:
            return h._no("the file ends inside its header")
        if data[p] != 0xFF:
            return h._no("bytes between marker segments")
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            p += 2
            continue
        if m == 0xD9:
            return h._no("end of image before any scan")
        length = (data[p + 2] << 8) | data[p + 3]
        if length < 2 or p + 2 + length > n:
            return h._no("the file ends inside its header")
        seg = data[p + 4:p + 2 + length]
        if m in _SOF_OTHER:
            return h._no("%s (SOF%d), not baseline" % (_SOF_OTHER[m], m - 0xC0))
        if m == 0xC0:
            if sof:
                return h._no("two frame headers")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                return h._no("bad frame header")
            if seg[0] != 8:
                return h._no("%d-bit samples" % seg[0])
            h.height, h.width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            if h.height == 0 or h.width == 0:
                return h._no("empty image (or height given by a DNL marker)")
            h.components = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
            sof = True
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                if seg[q] >> 4:
                    return h._no("16-bit quantisation table")
                if (seg[q] & 15) > 3 or q + 65 > len(seg):
                    return h._no("bad quantisation table segment")
                t = np.zeros(64, np.uint16)
                t[_ZIGZAG] = np.frombuffer(seg, np.uint8, 64, q + 1)
                h.qtables[seg[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg) or (seg[q] >> 4) > 1 or (seg[q] & 15) > 3:
                    return h._no("bad Huffman table segment")
                counts = seg[q + 1:q + 17]
                total = sum(counts)
                if total > 256 or q + 17 + total > len(seg):
                    return h._no("bad Huffman table segment")
                symbols = seg[q + 17:q + 17 + total]
                why = _check_huffman(counts, symbols, (seg[q] >> 4) == 0)
                if why:
                    return h._no(why)
                h.huffman[(seg[q] >> 4, seg[q] & 15)] = (counts, symbols)
                q += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                return h._no("bad restart interval segment")
            h.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            if not sof:
                return h._no("scan before the frame header")
            break
        p += 2 + length
    nc = len(h.components)
    if nc == 4:
        return h._no("four components (CMYK / YCCK)")
    if nc not in (1, 3):
        return h._no("%d components" % nc)
    if nc == 3:
        if adobe is not None and adobe != 1:
            return h._no("Adobe colour transform %d, not YCbCr" % adobe)
        if adobe is None and not jfif and tuple(c[0] for c in h.components) == (82, 71, 66):
            return h._no("RGB components, not YCbCr")
        (_, hs, vs, _), c1, c2 = h.components
        if (c1[1], c1[2]) != (1, 1) or (c2[1], c2[2]) != (1, 1) or (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
            return h._no("sampling %s, not 1x1 / 2x1 / 2x2 with 1x1 chroma" % ",".join("%dx%d" % (c[1], c[2]) for c in h.components))
        h.hs, h.vs = hs, vs
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        return h._no("bad scan header")
    if seg[0] != nc:
        return h._no("a scan of %d of %d components (more than one scan)" % (seg[0], nc))
    for i in range(nc):
        if seg[1 + 2 * i] != h.components[i][0]:
            return h._no("scan components out of order")
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if td > 1 or ta > 1:
            return h._no("Huffman table id above 1")
        if (0, td) not in h.huffman or (1, ta) not in h.huffman:
            return h._no("the scan names a Huffman table the file does not define")
        if h.components[i][3] not in h.qtables:
            return h._no("a component names a quantisation table the file does not define")
        h.selectors.append((td, ta))
    if seg[1 + 2 * nc] != 0 or seg[2 + 2 * nc] != 63 or seg[3 + 2 * nc] != 0:
        return h._no("spectral selection / successive approximation in a sequential scan")
    h.table_key = tuple(h.huffman.get((cls, t)) for t in (0, 1) for cls in (0, 1))
    h.quant_keys = [h.qtables[c[3]].tobytes() for c in h.components]
    h.table_select = sum((td << (2 * c)) | (ta << (2 * c + 1)) for c, (td, ta) in enumerate(h.selectors))
    h.supported = True
    return h


def _parse_scan(h, data, n, begin):
    h.supported = False
    # the entropy-coded data: up to the first marker that is neither a stuffed FF 00, a fill FF FF nor a restart marker
    bounds, end = [begin], n
    for found in _MARKER.finditer(data, begin):
        pos, mk = found.start(), data[found.start() + 1]
        if 0xD0 <= mk <= 0xD7:
            bounds += [pos, pos + 2]
        else:
            end = pos
            break
    bounds.append(end)
    h.scan = (begin, end)
    q = end                      # what follows the scan: anything but another scan
    while q + 4 <= n and data[q] == 0xFF and data[q + 1] != 0xD9:
        if data[q + 1] == 0xDA:
            return h._no("more than one scan")
        if data[q + 1] == 0xDC:
            return h._no("DNL marker")
        q += 1 if data[q + 1] == 0xFF else 2 + ((data[q + 2] << 8) | data[q + 3])
    mx, my = h.mcus
    total, ri = mx * my, h.restart_interval
    pieces = [(bounds[i], bounds[i + 1]) for i in range(0, len(bounds), 2)]
    if ri == 0:
        if len(pieces) != 1:
            return h._no("restart markers without a restart interval")
        h.units = [(begin, end, 0, total)]
    else:
        want = -(-total // ri)
        if len(pieces) > want:
            return h._no("more restart markers than the restart interval allows")
        pieces += [(end, end)] * (want - len(pieces))      # (a truncated file: the missing intervals run out of data at once)
        h.units = [(b, e, i * ri, min(ri, total - i * ri)) for i, (b, e) in enumerate(pieces)]
    h.supported = True
    return h


_table_cache = {}


def _table_words(counts, symbols, words):
    """One Huffman table in the layout csrc/jpeg.hip stages: 512 16-bit first-level entries, maxcode[17], valoff[17], 256 symbols."""
    key = (bytes(counts), bytes(symbols), words)
    t = _table_cache.get(key)
    if t is not None:
        return t
    lut = np.zeros(1 << _LUT_BITS, np.uint16)
    maxcode = np.full(17, -1, np.int32)
    valoff = np.zeros(17, np.int32)
    code = k = 0
    for length in range(1, 17):
        c = counts[length - 1]
        if c:
            valoff[length] = k - code
            if length <= _LUT_BITS:
                for i in range(c):
                    lo = (code + i) << (_LUT_BITS - length)
                    lut[lo:lo + (1 << (_LUT_BITS - length))] = (length << 8) | symbols[k + i]
            code += c
            k += c
            maxcode[length] = code - 1
        code <<= 1
    vals = np.zeros(256, np.uint8)
    vals[:len(symbols)] = np.frombuffer(bytes(symbols), np.uint8)
    t = np.zeros(words, np.int32)
    t[:256] = lut.view(np.int32)
    t[256:273] = maxcode
    t[273:290] = valoff
    t[290:354] = vals.view(np.int32)
    if len(_table_cache) > 4096:
        _table_cache.clear()
    _table_cache[key] = t
    return t


def _pil_pixels(blob, mode):
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        a = np.array(im.convert(mode))
    return a if a.ndim == 3 else a[:, :, None]


def _align(n, a=16):
    return -(-n // a) * a


class CoefficientBatch(object):
    """What ``JpegDecoder.coefficients`` returns.  ``headers``: the ``JpegHeader`` of every file (``supported`` False: the file has no
    coefficients here).  ``coef``: int16 [blocks, 64] on the device, natural order, absolute DC; the blocks of file i are rows
    ``rows[i, 7]`` .. ``+ rows[i, 8]``, planar: luma in raster order over the padded MCU grid, then Cb, then Cr.  ``desc``: the
    decoder's descriptor rows on the device, ``rows`` the same on the host.  ``status``: int32 [files] on the device, non-zero for a
    damaged scan (``JpegDecoder``).  ``coef``, ``desc`` and ``rows`` are None if no file is supported."""

    def __init__(self, headers, coef, desc, status, max_blocks, rows=None):
        self.headers, self.coef, self.desc, self.status, self.max_blocks, self.rows = headers, coef, desc, status, max_blocks, rows

    def blocks(self, i):
        """The coefficients of file i: int16 [its blocks, 64] (a view)."""
        off, n = int(self.rows[i, 7]), int(self.rows[i, 8])
        return self.coef[off:off + n]


class JpegDecoder(object):
    """``decode(blobs, mode)``: the files' pixels as device tensors, uint8 [H, W, 3] ("RGB") or [H, W, 1] ("L") each -- what
    ``np.asarray(Image.open(f).convert(mode))`` holds.  Everything is enqueued on the current stream of ``device``; nothing is
    read back.  ``status`` (int32 [files], on the device) is non-zero for a file whose scan was damaged: 1 it ran out of data,
    2 an undefined Huffman code, 4 a coefficient past the end of a block, 8 an unusable table row.  ``check()`` is the one optional
    host read: it looks at ``status`` and replaces the damaged files of the last batch by PIL's decoding.  ``fallbacks`` counts the
    files PIL decoded on the host: the ones ``parse_jpeg`` does not support, and after ``check()`` the damaged ones.

    ``index`` says who finds the restart intervals.  "host" (the default): ``parse_jpeg`` walks every scan.  "device": the host
    reads the headers only (``parse_jpeg_header``), copies every file once, from its first scan byte to its end, into the pinned
    upload buffer, and ``ssn_jpeg_index`` searches the markers and fills the unit table in front of the entropy launch; the host
    does a constant amount of work per file and none per restart interval or per byte.  The one difference in behaviour: what the
    host walk refuses by looking at the scan (restart markers that do not fit the header's interval, a second scan, a DNL marker)
    the device finds after the call has returned, so such a file is not decoded by PIL inside ``decode`` -- it gets bit 16 in
    ``status``, unspecified pixels, and is decoded by PIL and counted in ``fallbacks`` by ``check()``, like a damaged file."""

    def __init__(self, device="cuda:0", index="host"):
        if index not in ("host", "device"):
            raise ValueError("JpegDecoder: index is 'host' or 'device'")
        self.index = index
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.fallbacks = 0
        self.status = None
        self.uploaded_bytes = 0             # of the last batch: what went over PCIe
        self.profile = None                 # a list: decode() appends (stage, start event, end event) of upload and the three launches
        self._last = None
        self._pinned = [None, None]
        self._event = [None, None]
        self._turn = 0
        self.desc_ints, self.unit_ints, self.table_words, self.lds_sets = K.jpeg_layout()

    # -- host: the tables of a batch ---------------------------------------------------------------------------------------
    def _plan(self, blobs, headers, out_c):
        """-> (staging uint8 array, section offsets, sizes) for the supported files; fallback files get an empty desc row."""
        n = len(blobs)
        desc = np.zeros((n, self.desc_ints), np.int32)
        sets, set_rows, quant, quant_rows = {}, [], {}, []
        units, pieces = [], []
        bits_off = coef_off = plane_off = 0
        out_off = self._out_off
        max_blocks = max_pixels = 0
        for i, (blob, h) in enumerate(zip(blobs, headers)):
            if h is None:
                continue
            mx, my = h.mcus
            nc = len(h.components)
            luma, chroma = mx * h.hs * my * h.vs, mx * my
            nblocks = luma + (2 * chroma if nc == 3 else 0)
            qi = []
            for c, key in zip(h.components, h.quant_keys):
                if key not in quant:
                    quant[key] = len(quant_rows)
                    quant_rows.append(h.qtables[c[3]])
                qi.append(quant[key])
            qi += [0] * (3 - nc)
            tsel, key = h.table_select, h.table_key
            if key not in sets:
                sets[key] = len(set_rows)
                row = np.zeros((4, self.table_words), np.int32)
                for j, tab in enumerate(key):
                    if tab is not None:
                        row[j] = _table_words(tab[0], tab[1], self.table_words)
                set_rows.append(row)
            s = sets[key]
            b0, b1 = h.scan
            shift = bits_off - b0
            for (ub, ue, m0, nm) in h.units:
                units.append((s, i, ub + shift, ue + shift, m0, nm))
            pieces.append(blob[b0:b1])
            desc[i, :15] = (h.width, h.height, nc, h.hs, h.vs, mx, my, coef_off, nblocks, plane_off, out_off[i], qi[0], qi[1], qi[2], tsel)
            bits_off += b1 - b0
            coef_off += nblocks
            plane_off += nblocks * 64
            max_blocks, max_pixels = max(max_blocks, nblocks), max(max_pixels, h.width * h.height)
        if coef_off >= (1 << 25) or bits_off >= (1 << 31) or out_off[-1] >= (1 << 31):
            raise ValueError("JpegDecoder: the batch is too large for one call (2^25 blocks, 2 GiB of scans or of pixels)")
        # unit rows: sorted by table set, packed into workgroups of 64 lanes that span at most lds_sets sets
        units.sort(key=lambda u: u[0])
        rows, first, wg_sets = [], 0, []
        for u in units:
            if len(rows) - first == 64 or (len(rows) > first and u[0] - rows[first][5] >= self.lds_sets):
                rows += [(-1, 0, 0, 0, 0, 0)] * (first + 64 - len(rows))
                first = len(rows)
            rows.append((u[1], u[2], u[3], u[4], u[5], u[0]))
        rows += [(-1, 0, 0, 0, 0, 0)] * (_align(len(rows), 64) - len(rows))
        urows = np.zeros((len(rows), self.unit_ints), np.int32)
        urows[:, :6] = np.array(rows, np.int64).reshape(-1, 6)
        for w in range(0, len(rows), 64):
            live = urows[w:w + 64][urows[w:w + 64, 0] >= 0]
            urows[w, 6] = live[:, 5].min()
            urows[w, 7] = live[:, 5].max() - live[:, 5].min() + 1
        sections = [np.frombuffer(b"".join(pieces), np.uint8), desc.view(np.uint8).reshape(-1), urows.view(np.uint8).reshape(-1),
                    np.stack(set_rows).view(np.uint8).reshape(-1), np.stack(quant_rows).view(np.uint8).reshape(-1)]
        offs, total = [], 0
        for sec in sections:
            offs.append(total)
            total += _align(max(sec.size, 1))
        staging = np.zeros(total, np.uint8)
        for o, sec in zip(offs, sections):
            staging[o:o + sec.size] = sec
        sizes = dict(bits=bits_off, units=len(rows), sets=len(set_rows), quant=len(quant_rows), blocks=coef_off, planes=plane_off,
                     max_blocks=max_blocks, max_pixels=max_pixels)
        return staging, offs, sizes

    def _plan_device(self, blobs, headers):
        """``_plan`` for ``index="device"``: per file one desc row (columns 15 .. 18: where ``ssn_jpeg_index`` finds the file's bytes
        and its unit rows) and ONE copy of its bytes, from the first scan byte to the file's end, into the upload buffer; the unit
        rows -- everything but begin / end, which the kernel fills -- with numpy, whatever the number of restart intervals.
        -> (upload buffer, section offsets, sizes, the desc rows)."""
        n = len(blobs)
        desc = np.zeros((n, self.desc_ints), np.int32)
        sets, set_rows, quant, quant_rows = {}, [], {}, []
        image, fset, fcount, fri, fmcus, spans = [], [], [], [], [], []
        bits_off = coef_off = plane_off = 0
        out_off = self._out_off
        max_blocks = max_pixels = 0
        for i, (blob, h) in enumerate(zip(blobs, headers)):
            if h is None:
                continue
            mx, my = h.mcus
            nc = len(h.components)
            luma, chroma = mx * h.hs * my * h.vs, mx * my
            nblocks = luma + (2 * chroma if nc == 3 else 0)
            qi = []
            for c, key in zip(h.components, h.quant_keys):
                if key not in quant:
                    quant[key] = len(quant_rows)
                    quant_rows.append(h.qtables[c[3]])
                qi.append(quant[key])
            qi += [0] * (3 - nc)
            key = h.table_key
            if key not in sets:
                sets[key] = len(set_rows)
                row = np.zeros((4, self.table_words), np.int32)
                for j, tab in enumerate(key):
                    if tab is not None:
                        row[j] = _table_words(tab[0], tab[1], self.table_words)
                set_rows.append(row)
            ri, size = h.restart_interval, len(blob) - h.scan[0]
            count = -(-chroma // ri) if ri else 1
            desc[i, :19] = (h.width, h.height, nc, h.hs, h.vs, mx, my, coef_off, nblocks, plane_off, out_off[i], qi[0], qi[1], qi[2],
                            h.table_select, bits_off, bits_off + size, 0, count)
            image.append(i)
            fset.append(sets[key])
            fcount.append(count)
            fri.append(ri)
            fmcus.append(chroma)
            spans.append((bits_off, h.scan[0], size))
            bits_off += _align(size)
            coef_off += nblocks
            plane_off += nblocks * 64
            max_blocks, max_pixels = max(max_blocks, nblocks), max(max_pixels, h.width * h.height)
        if coef_off >= (1 << 25) or bits_off >= (1 << 31) or out_off[-1] >= (1 << 31):
            raise ValueError("JpegDecoder: the batch is too large for one call (2^25 blocks, 2 GiB of scans or of pixels)")
        # the files' rows, as _plan lays its sorted units out: by table set, in workgroups of 64 rows that span at most lds_sets sets.
        # A file's units share its set, so a break the sets force falls in front of a file: one step per FILE decides the rows.
        image, fset, fcount = np.array(image, np.int64), np.array(fset, np.int64), np.array(fcount, np.int64)
        order = np.argsort(fset, kind="stable")
        row0 = [0] * len(order)
        pos = first = first_set = 0
        for j, s, k in zip(order.tolist(), fset[order].tolist(), fcount[order].tolist()):
            if pos > first and s - first_set >= self.lds_sets:
                pos = first = first + 64
            if pos == first:
                first_set = s
            row0[j] = pos
            pos += k
            if pos - first >= 64:
                first, first_set = first + (pos - first) // 64 * 64, s
        row0 = np.array(row0, np.int64)
        desc[image, 17] = row0
        nrows = _align(pos, 64)
        if nrows >= (1 << 31) // (4 * self.unit_ints):
            raise ValueError("JpegDecoder: too many restart intervals for one call")
        counts = fcount[order]
        rep = np.repeat(np.arange(len(order)), counts)                          # the (sorted) file of every unit
        k = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)      # its number inside the file
        at = row0[order][rep] + k
        ri, mcus = np.array(fri, np.int64)[order][rep], np.array(fmcus, np.int64)[order][rep]
        urows = np.zeros((nrows, self.unit_ints), np.int32)
        urows[:, 0] = -1
        urows[at, 0] = image[order][rep]
        urows[at, 3] = k * ri
        urows[at, 4] = np.where(ri > 0, np.minimum(ri, mcus - k * ri), mcus)
        urows[at, 5] = fset[order][rep]
        live = urows[:, 0].reshape(-1, 64) >= 0
        wg = urows[:, 5].reshape(-1, 64)
        lo = np.where(live, wg, 1 << 30).min(axis=1)
        urows[::64, 6] = lo
        urows[::64, 7] = np.where(live, wg, -1).max(axis=1) - lo + 1
        sections = [None, desc.view(np.uint8).reshape(-1), urows.view(np.uint8).reshape(-1),
                    np.stack(set_rows).view(np.uint8).reshape(-1), np.stack(quant_rows).view(np.uint8).reshape(-1)]
        offs, total = [0], _align(max(bits_off, 1))
        for sec in sections[1:]:
            offs.append(total)
            total += _align(max(sec.size, 1))
        staging = self._staging(total)
        flat = staging.numpy()
        for blob, (o, b0, size) in zip((blobs[i] for i in image.tolist()), spans):
            flat[o:o + size] = np.frombuffer(blob, np.uint8, size, b0)
        for o, sec in zip(offs[1:], sections[1:]):
            flat[o:o + sec.size] = sec
        sizes = dict(bits=bits_off, units=nrows, sets=len(set_rows), quant=len(quant_rows), blocks=coef_off, planes=plane_off,
                     max_blocks=max_blocks, max_pixels=max_pixels)
        return staging, offs, sizes, desc

    def _staging(self, nbytes):
        """The buffer the next batch is assembled in: a slice of one of the two pinned buffers (host memory on a non-HIP device)."""
        if not self.cuda:
            return torch.empty(nbytes, dtype=torch.uint8)
        turn = self._turn
        if self._event[turn] is not None:
            self._event[turn].synchronize()      # the copy that last read this pinned buffer is done
        if self._pinned[turn] is None or self._pinned[turn].numel() < nbytes:
            self._pinned[turn] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
        return self._pinned[turn][:nbytes]

    def _send(self, staging):
        """Start the copy of what ``_staging`` handed out."""
        if not self.cuda:
            return staging
        turn = self._turn
        self._turn ^= 1
        dev = staging.to(self.device, non_blocking=True)
        self._event[turn] = torch.cuda.Event()
        self._event[turn].record(torch.cuda.current_stream(self.device))
        return dev

    def _upload(self, staging):
        t = torch.from_numpy(staging)
        if not self.cuda:
            return t
        turn = self._turn
        self._turn ^= 1
        if self._event[turn] is not None:
            self._event[turn].synchronize()      # the copy that last read this pinned buffer is done
        if self._pinned[turn] is None or self._pinned[turn].numel() < t.numel():
            self._pinned[turn] = torch.empty(max(t.numel(), 1 << 20), dtype=torch.uint8, pin_memory=True)
        pinned = self._pinned[turn][:t.numel()]
        pinned.copy_(t)
        dev = pinned.to(self.device, non_blocking=True)
        self._event[turn] = torch.cuda.Event()
        self._event[turn].record(torch.cuda.current_stream(self.device))
        return dev

    def _timed(self, stage, fn, *args):
        if self.profile is None or not self.cuda:
            return fn(*args)
        stream = torch.cuda.current_stream(self.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        r = fn(*args)
        end.record(stream)
        self.profile.append((stage, start, end))
        return r

    def _alloc(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _entropy(self, bits, desc, units, tables, coef):
        """The entropy launch; with ``index="device"`` between the index launch, which completes the unit rows, and the launch
        that ORs its verdicts into ``status`` (the entropy launch zeroes ``status``)."""
        if self.index == "device":
            refused = self._alloc((desc.shape[0],), torch.int32)
            self._timed("index", K.jpeg_index, bits, desc, units, refused)
        self._timed("entropy", K.jpeg_entropy, bits, desc, units, tables, coef, self.status)
        if self.index == "device":
            self._timed("verdicts", K.jpeg_index_status, refused, self.status)

    # -- decode ------------------------------------------------------------------------------------------------------------
    def decode(self, blobs, mode="RGB", stack=False):
        if mode not in ("RGB", "L"):
            raise ValueError("JpegDecoder: mode is 'RGB' or 'L'")
        blobs = [bytes(b) for b in blobs]
        if not blobs:
            raise ValueError("JpegDecoder: no files")
        out_c = 3 if mode == "RGB" else 1
        headers, host, shapes = [], {}, []
        parse = parse_jpeg_header if self.index == "device" else parse_jpeg
        for i, blob in enumerate(blobs):
            h = parse(blob)
            if h.supported:
                headers.append(h)
                shapes.append((h.height, h.width))
            else:
                host[i] = _pil_pixels(blob, mode)      # (a file PIL cannot open either raises what PIL raises)
                headers.append(None)
                shapes.append(host[i].shape[:2])
        if stack and len(set(shapes)) != 1:
            raise ValueError("JpegDecoder: stack=True needs files of one size, got %s" % sorted(set(shapes)))
        self.fallbacks += len(host)
        n = len(blobs)
        self._out_off = [0]
        for hh, ww in shapes:
            self._out_off.append(self._out_off[-1] + hh * ww * out_c)
        out = self._alloc((self._out_off[-1],), torch.uint8)
        self.status = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.uploaded_bytes = 0
        if len(host) < n:
            if self.index == "device":
                staging, offs, sz, _ = self._plan_device(blobs, headers)
                self.uploaded_bytes = staging.numel()
                dev = self._timed("upload", self._send, staging)
            else:
                staging, offs, sz = self._plan(blobs, headers, out_c)
                self.uploaded_bytes = staging.size
                dev = self._timed("upload", self._upload, staging)
            bits = dev[offs[0]:offs[0] + sz["bits"]]
            desc = dev[offs[1]:offs[1] + n * self.desc_ints * 4].view(torch.int32).view(n, self.desc_ints)
            units = dev[offs[2]:offs[2] + sz["units"] * self.unit_ints * 4].view(torch.int32).view(-1, self.unit_ints)
            tables = dev[offs[3]:offs[3] + sz["sets"] * 16 * self.table_words].view(torch.int32).view(-1, 4, self.table_words)
            quant = dev[offs[4]:offs[4] + sz["quant"] * 128].view(torch.int16).view(-1, 64)
            coef = self._alloc((sz["blocks"], 64), torch.int16)
            planes = self._alloc((sz["planes"],), torch.uint8)
            self._entropy(bits, desc, units, tables, coef)
            self._timed("idct", K.jpeg_idct, coef, desc, sz["max_blocks"], quant, planes)
            self._timed("pixels", K.jpeg_pixels, planes, desc, sz["max_pixels"], out_c, out)
            self._stages = (desc, coef, planes, quant, sz)      # (kept for the stage-level tests)
            self._unit_rows = units
        views = [out[self._out_off[i]:self._out_off[i + 1]].view(shapes[i][0], shapes[i][1], out_c) for i in range(n)]
        for i, a in host.items():
            self.uploaded_bytes += a.size
            views[i].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self._last = (blobs, mode, views)
        if stack:
            return out.view(n, shapes[0][0], shapes[0][1], out_c)
        return views

    def coefficients(self, blobs):
        """The marker walk, the upload and the entropy launch of ``decode`` and nothing after them -> ``CoefficientBatch``: the
        quantised coefficients of the files as the entropy stage leaves them (the launch zero-fills the buffer first: it writes the
        non-zero coefficients only).  What lossless transcoding starts from (jpeg_transcode.py).  Nothing is read back."""
        blobs = [bytes(b) for b in blobs]
        if not blobs:
            raise ValueError("JpegDecoder: no files")
        parse = parse_jpeg_header if self.index == "device" else parse_jpeg
        parsed = [parse(blob) for blob in blobs]
        headers = [h if h.supported else None for h in parsed]
        n = len(blobs)
        self._out_off = [0] * (n + 1)      # (no pixels: the rows' output offsets are not used)
        self.status = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.uploaded_bytes = 0
        self._last = None
        if all(h is None for h in headers):
            return CoefficientBatch(parsed, None, None, self.status, 0)
        if self.index == "device":
            staging, offs, sz, rows = self._plan_device(blobs, headers)
            self.uploaded_bytes = staging.numel()
            dev = self._timed("upload", self._send, staging)
        else:
            staging, offs, sz = self._plan(blobs, headers, 1)
            self.uploaded_bytes = staging.size
            dev = self._timed("upload", self._upload, staging)
            rows = np.frombuffer(staging, np.int32, n * self.desc_ints, offs[1]).reshape(n, self.desc_ints)
        bits = dev[offs[0]:offs[0] + sz["bits"]]
        desc = dev[offs[1]:offs[1] + n * self.desc_ints * 4].view(torch.int32).view(n, self.desc_ints)
        units = dev[offs[2]:offs[2] + sz["units"] * self.unit_ints * 4].view(torch.int32).view(-1, self.unit_ints)
        tables = dev[offs[3]:offs[3] + sz["sets"] * 16 * self.table_words].view(torch.int32).view(-1, 4, self.table_words)
        coef = self._alloc((sz["blocks"], 64), torch.int16)
        self._entropy(bits, desc, units, tables, coef)
        return CoefficientBatch(parsed, coef, desc, self.status, sz["max_blocks"], rows)

    def check(self):
        """Read ``status`` (a host synchronisation) and decode the damaged files of the last batch with PIL, in place.
        -> their indices."""
        if self._last is None:
            return []
        blobs, mode, views = self._last
        bad = [int(i) for i in torch.nonzero(self.status.cpu()).flatten()]
        for i in bad:
            a = _pil_pixels(blobs[i], mode)
            if tuple(a.shape) != tuple(views[i].shape):
                raise ValueError("JpegDecoder: PIL decodes file %d to %s, its header says %s" % (i, a.shape, tuple(views[i].shape)))
            views[i].copy_(torch.from_numpy(np.ascontiguousarray(a)))
            self.fallbacks += 1
        return bad


class CompressedBatchPrefetcher(TrainingBatchPrefetcher):
    """``TrainingBatchPrefetcher`` for sources that yield the FILES of a batch (``train_data.compressed_ssn_batches``): ``frames`` is
    a list (videos) of lists of ``bytes``.  The side stream uploads the scans and their tables, decodes them there and hands the
    uint8 frames to the same transform; about 14 times fewer bytes cross PCIe than with decoded frames.  On a non-HIP device it
    degrades to the synchronous loop, as the parent class does."""

    def __init__(self, source, transform, depth=2, group_size=None, index="host"):
        self.decoder = JpegDecoder(transform.mean.device, index=index)
        self.mode = "L" if transform.is_flow else "RGB"
        super().__init__(source, transform, depth=depth, group_size=group_size)

    def _stage(self, slot, item):
        files, scaling, target, reg_target, prop_type = item
        v, n_img = len(files), len(files[0])
        if any(len(f) != n_img for f in files):
            raise ValueError("frames: the same number of files for every video")
        flat = [b for f in files for b in f]
        small = [torch.as_tensor(t) for t in (scaling, target, reg_target, prop_type)]
        if not self.cuda:
            frames = self.decoder.decode(flat, self.mode, stack=True)
            out = self._transform(frames)
            return (out.reshape(v, n_img * frames.shape[-1], out.shape[-2], out.shape[-1]),) + tuple(t.to(self.device) for t in small), None
        with torch.cuda.stream(self._stream):
            frames = self.decoder.decode(flat, self.mode, stack=True)
            out = self._transform(frames)
            out = out.reshape(v, n_img * frames.shape[-1], out.shape[-2], out.shape[-1])
            rest = tuple(t.pin_memory().to(self.device, non_blocking=True) for t in small)
            ready = torch.cuda.Event()
            ready.record(self._stream)
        return (out,) + rest, ready
