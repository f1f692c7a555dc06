"""Baseline JPEG encoding on the device: the stage between flow extraction and the data sets, which the tool did with
``PIL.Image.fromarray(a).save(f, quality=95)`` on one host thread.

``JpegEncoder.encode`` takes uint8 images that are already on the device, enqueues a constant number of launches for the whole batch
(csrc/jpeg_encode.hip: blocks, count, scan, pack, assemble) on the caller's stream and reads nothing in between; the only host reads
are of the finished lengths and bytes.  The host prepares what does not depend on a pixel: the quantisation tables of the quality,
the header bytes and the geometry of every image.  The files are PIL's, byte for byte, for the libjpeg PIL links.
"""
import numpy as np
import torch

from . import kernels as K

_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                    54, 47, 55, 62, 63])
# ITU-T T.81 Annex K: quantisation tables (K.1, K.2; natural order) and Huffman tables (K.3 - K.6; code counts per length, symbols)
_QUANT_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
               80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
               95, 98, 112, 100, 103, 99]
_QUANT_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
                 99, 99] + [99] * 32
_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))


_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
            [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
             0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
             0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
             0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
             0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
             0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
             0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
             0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
              [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
               0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
               0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
               0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
               0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
               0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
               0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
               0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
               0xF9, 0xFA])
_HUFFMAN = [_DC_LUMA, _AC_LUMA, _DC_CHROMA, _AC_CHROMA]      # the order of the device table and of the DHT segments

ST_CAPACITY, ST_RANGE, ST_DESC = 1, 2, 4
_SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}                # PIL's subsampling= -> luma sampling factors


def quant_tables(quality):
    """(luma, chroma) uint16 [64] in natural order: Annex K scaled by libjpeg's quality rule, clamped to 1 .. 255."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((np.array(b, np.int64) * s + 50) // 100, 1, 255).astype(np.uint16) for b in (_QUANT_LUMA, _QUANT_CHROMA)]


def code_table():
    """int32 [4, 256]: length << 16 | code for every symbol of the four standard tables (0: no code)."""
    t = np.zeros((4, 256), np.int32)
    for i, (counts, symbols) in enumerate(_HUFFMAN):
        code = k = 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                t[i, symbols[k]] = (length << 16) | code
                code += 1
                k += 1
            code <<= 1
    return t


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header_bytes(width, height, ncomp, hs, vs, qtabs, restart_interval):
    """SOI, APP0 (JFIF 1.01, no units, 1 x 1), a DQT per table, SOF0, a DHT per table, DRI with restarts only, SOS."""
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")]
    for i in range(1 if ncomp == 1 else 2):
        out.append(_segment(0xDB, bytes([i]) + bytes(qtabs[i][_ZIGZAG].astype(np.uint8))))
    comps = [(1, hs, vs, 0)] + ([(2, 1, 1, 1), (3, 1, 1, 1)] if ncomp == 3 else [])
    out.append(_segment(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([ncomp]) +
                        b"".join(bytes([c, (h << 4) | v, q]) for c, h, v, q in comps)))
    for i in range(2 if ncomp == 1 else 4):
        counts, symbols = _HUFFMAN[i]
        out.append(_segment(0xC4, bytes([((i & 1) << 4) | (i >> 1)]) + bytes(counts) + bytes(symbols)))
    if restart_interval:
        out.append(_segment(0xDD, restart_interval.to_bytes(2, "big")))
    out.append(_segment(0xDA, bytes([ncomp]) + b"".join(bytes([c, 0x00 if c == 1 else 0x11]) for c, _, _, _ in comps) + b"\0\x3f\0"))
    return b"".join(out)


class EncodedBatch(object):
    """The files of one ``encode`` call, on the device: ``data`` uint8 [bytes] holds file i at ``offsets[i]`` (int64) with
    ``lengths[i]`` (int32) bytes, back to back.  ``status`` (int32) bits: 1 the image does not fit its capacity, 4 an unusable table
    row (either way no file: length 0); 2 a coefficient the standard tables have no code for was coded as zero (the first stage
    cannot produce one)."""

    def __init__(self, data, offsets, lengths, status):
        self.data, self.offsets, self.lengths, self.status = data, offsets, lengths, status

    def check(self):
        """Read ``status`` (a host synchronisation); raises if an image was not written as asked."""
        bad = [(int(i), int(s)) for i, s in enumerate(self.status.cpu().tolist()) if s]
        if bad:
            raise RuntimeError("JpegEncoder: images not written (index, status): %s" % bad)
        return self

    def to_bytes(self):
        """The two host reads: the lengths, then exactly the bytes of the files."""
        self.check()
        lengths = self.lengths.cpu().tolist()
        total = sum(lengths)
        blob = self.data[:total].cpu().numpy().tobytes()
        out, o = [], 0
        for n in lengths:
            out.append(blob[o:o + n])
            o += n
        return out


class JpegEncoder(object):
    """``encode(images, quality=95, subsampling=None, restart_blocks=0, as_bytes=True)``: what
    ``Image.fromarray(a).save(f, "JPEG", quality=, subsampling=, restart_marker_blocks=)`` writes for every image.

    images: one uint8 device tensor [N, H, W] / [N, H, W, 1] (gray) or [N, H, W, 3] (RGB), or a list of [H, W] / [H, W, 1] /
    [H, W, 3] tensors of any sizes and one mode (one set of launches either way).  subsampling: None is gray for one channel and
    4:2:0 for RGB; 0, 1, 2 are 4:4:4, 4:2:2, 4:2:0.  restart_blocks=k: a DRI segment with an interval of k MCUs.  capacity: bytes
    a file may take at most (default: the worst case of DESIGN.md 3.11, which no picture exceeds); an image that does not fit gets
    status 1 and no file.  -> a list of ``bytes``, or with as_bytes=False an ``EncodedBatch`` and no host read at all."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.desc_ints, self.block_bits = K.jpeg_enc_layout()
        self.block_bytes = -(-self.block_bits // 8)
        self.profile = None          # a list: encode() appends (stage, start event, end event)
        self.downloaded_bytes = 0    # of the last to_bytes(): what came over PCIe
        self._tables = None
        self._stages = None

    def _alloc(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

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

    # -- host: arguments and the tables of a batch ---------------------------------------------------------------------------
    def _images(self, images):
        """-> (list of contiguous uint8 [H, W, C] views, C, the flat pixel tensor or None if it has to be gathered)"""
        if torch.is_tensor(images):
            if images.dim() == 3:
                images = images.unsqueeze(-1)
            if images.dim() != 4:
                raise ValueError("JpegEncoder: a tensor of images is [N, H, W], [N, H, W, 1] or [N, H, W, 3]")
            stacked = images.contiguous()
            views = list(stacked)
        else:
            stacked = None
            views = list(images)
            if not views or not all(torch.is_tensor(v) for v in views):
                raise ValueError("JpegEncoder: images is a tensor or a non-empty list of tensors")
            for v in views:
                if v.dim() not in (2, 3):
                    raise ValueError("JpegEncoder: an image of a list is [H, W], [H, W, 1] or [H, W, 3]")
            views = [(v.unsqueeze(-1) if v.dim() == 2 else v).contiguous() for v in views]
        if not views:
            raise ValueError("JpegEncoder: no images")
        for v in views:
            if v.dtype != torch.uint8:
                raise ValueError("JpegEncoder: images are uint8, got %s" % v.dtype)
            if v.device != views[0].device:
                raise ValueError("JpegEncoder: images on different devices")
            if v.shape[-1] not in (1, 3):
                raise ValueError("JpegEncoder: images have 1 (gray) or 3 (RGB) channels, got %d" % v.shape[-1])
            if not (1 <= v.shape[0] <= 65535 and 1 <= v.shape[1] <= 65535):
                raise ValueError("JpegEncoder: image sizes are 1 .. 65535, got %d x %d" % (v.shape[1], v.shape[0]))
        if len({v.shape[-1] for v in views}) != 1:
            raise ValueError("JpegEncoder: gray and RGB images in one batch (mixed modes)")
        return views, views[0].shape[-1], (stacked.reshape(-1) if stacked is not None else None)

    def _plan(self, shapes, ncomp, hs, vs, quality, restart_blocks, capacity):
        qtabs = quant_tables(quality)
        return self._plan_specs([(h, w, ncomp, hs, vs, qtabs, restart_blocks) for (h, w) in shapes], qtabs, capacity)

    def _plan_specs(self, specs, quant, capacity, pixels=True):
        """specs: per image (height, width, components, luma hs, vs, [luma, chroma] quantisation tables for its header, restart
        interval in MCUs or 0).  quant: the two tables the first stage divides by (not looked at when coefficients are given).  pixels=False:
        there are none (the rows' pixel offsets stay 0 and do not count against the 2 GiB)."""
        n = len(specs)
        desc = np.zeros((n, self.desc_ints), np.int64)
        headers, cache = [], {}
        pix_off = blk_off = int_off = raw_off = hdr_off = out_total = max_blocks = 0
        for i, (h, w, ncomp, hs, vs, qtabs, restart_blocks) in enumerate(specs):
            bpm = 1 if ncomp == 1 else hs * vs + 2
            mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
            nblocks = mx * my * bpm
            if nblocks * self.block_bits >= (1 << 31):
                raise ValueError("JpegEncoder: a %d x %d image is too large (its scan may pass 2^31 bits)" % (w, h))
            ri = min(restart_blocks, mx * my) if restart_blocks else mx * my
            nint = -(-(mx * my) // ri)
            key = (h, w, ncomp, hs, vs, restart_blocks, qtabs[0].tobytes(), qtabs[-1].tobytes())
            if key not in cache:
                cache[key] = header_bytes(w, h, ncomp, hs, vs, qtabs, restart_blocks)
            hdr = cache[key]
            # the worst case: every block takes block_bytes, every byte of the scan is an FF
            raw_worst = self.block_bytes * nblocks
            out_worst = len(hdr) + 2 * raw_worst + 2 * (nint - 1) + 2
            out_cap = out_worst if capacity is None else min(out_worst, capacity)
            raw_cap = -(-min(raw_worst, out_cap) // 4) * 4
            desc[i, :18] = (w, h, ncomp, hs, vs, mx, my, pix_off, blk_off, nblocks, ri, int_off, nint, raw_off, raw_cap, hdr_off, len(hdr),
                            out_cap)
            headers.append(hdr)
            pix_off += h * w * ncomp if pixels else 0
            blk_off += nblocks
            int_off += nint
            raw_off += raw_cap
            hdr_off += len(hdr)
            out_total += out_cap
            max_blocks = max(max_blocks, nblocks)
        if blk_off >= (1 << 25) or pix_off >= (1 << 31) or raw_off >= (1 << 31) or n > 65535:
            raise ValueError("JpegEncoder: the batch is too large for one call (65535 images, 2^25 blocks, 2 GiB of pixels or of scans); "
                             "split it or give a capacity")
        qtabs = quant
        sections = [desc.astype(np.int32).view(np.uint8).reshape(-1), np.stack(qtabs).astype(np.int16).view(np.uint8).reshape(-1),
                    np.frombuffer(b"".join(headers), np.uint8)]
        offs, total = [], 0
        for sec in sections:
            offs.append(total)
            total += -(-sec.size // 16) * 16
        staging = np.zeros(total, np.uint8)
        for o, sec in zip(offs, sections):
            staging[o:o + sec.size] = sec
        sizes = dict(blocks=blk_off, intervals=int_off, raw=max(raw_off, 4), data=max(out_total, 1), headers=hdr_off, max_blocks=max_blocks)
        return staging, offs, sizes

    # -- encode ----------------------------------------------------------------------------------------------------------------
    def encode(self, images, quality=95, subsampling=None, restart_blocks=0, as_bytes=True, capacity=None, **options):
        for name, value in options.items():
            if name in ("progressive", "optimize", "qtables", "exif", "icc_profile", "restart_marker_rows", "smooth", "streamtype",
                        "comment", "dpi", "keep_rgb"):
                if value is None or value is False or (name in ("exif", "icc_profile", "comment") and not value):
                    continue
                raise ValueError("JpegEncoder: %s= is not supported (baseline files with the standard tables only)" % name)
            raise ValueError("JpegEncoder: unknown option %s=" % name)
        if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
            raise ValueError("JpegEncoder: quality is an integer 1 .. 100, got %r" % (quality,))
        if isinstance(restart_blocks, bool) or not isinstance(restart_blocks, int) or not 0 <= restart_blocks <= 65535:
            raise ValueError("JpegEncoder: restart_blocks is 0 (none) .. 65535 MCUs")
        if capacity is not None and (not isinstance(capacity, int) or capacity < 1):
            raise ValueError("JpegEncoder: capacity is a positive number of bytes")
        views, ncomp, flat = self._images(images)
        if ncomp == 1:
            if subsampling is not None:
                raise ValueError("JpegEncoder: subsampling= applies to RGB images only")
            hs = vs = 1
        else:
            if subsampling is None:
                subsampling = 2
            if isinstance(subsampling, bool) or subsampling not in _SAMPLING:
                raise ValueError("JpegEncoder: subsampling is None, 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got %r" % (subsampling,))
            hs, vs = _SAMPLING[subsampling]
        if views[0].device != self.device and not (views[0].device.type == self.device.type == "cuda" and self.device.index is None):
            raise ValueError("JpegEncoder: images are on %s, the encoder on %s" % (views[0].device, self.device))
        shapes = [(int(v.shape[0]), int(v.shape[1])) for v in views]
        staging, offs, sz = self._plan(shapes, ncomp, hs, vs, quality, restart_blocks, capacity)
        if flat is None:
            flat = torch.cat([v.reshape(-1) for v in views]) if len(views) > 1 else views[0].reshape(-1)
        return self._run(flat, staging, offs, sz, len(views), as_bytes)

    def plan_coefficients(self, specs, capacity=None):
        """The tables of a batch whose coefficients exist already (lossless transcoding, jpeg_transcode.py).  specs: per image
        ``(height, width, components, hs, vs, [luma, chroma] uint16 [64] natural-order tables, restart interval)``; images of one
        batch may differ in all of them.  The header of every file carries the given tables and, with a restart interval k > 0, a DRI
        segment of k; the Huffman tables are the standard ones.  -> a plan for ``encode_coefficients``; ``plan["desc"]`` (host, int64
        [images, desc_ints]) says where the coefficients of every image go: its blocks are rows ``desc[i, 8]`` .. ``+ desc[i, 9]``."""
        specs = list(specs)
        if not specs:
            raise ValueError("JpegEncoder: no images")
        for (h, w, ncomp, hs, vs, qtabs, restart) in specs:
            if ncomp not in (1, 3) or (hs, vs) not in _SAMPLING.values() or (ncomp == 1 and (hs, vs) != (1, 1)):
                raise ValueError("JpegEncoder: gray, or 3 components with luma sampling 1x1, 2x1 or 2x2")
            if not (1 <= h <= 65535 and 1 <= w <= 65535):
                raise ValueError("JpegEncoder: image sizes are 1 .. 65535, got %d x %d" % (w, h))
            if not 0 <= restart <= 65535:
                raise ValueError("JpegEncoder: restart_blocks is 0 (none) .. 65535 MCUs")
            if len(qtabs) < (1 if ncomp == 1 else 2) or any(np.asarray(q).shape != (64,) or np.asarray(q).min() < 1 or
                                                             np.asarray(q).max() > 255 for q in qtabs):
                raise ValueError("JpegEncoder: quantisation tables are [64] entries of 1 .. 255 (8-bit tables)")
        staging, offs, sz = self._plan_specs(specs, quant_tables(50), capacity, pixels=False)
        desc = np.frombuffer(staging, np.int32, len(specs) * self.desc_ints, offs[0]).reshape(len(specs), self.desc_ints).astype(np.int64)
        return dict(staging=staging, offs=offs, sizes=sz, n=len(specs), desc=desc)

    def encode_coefficients(self, plan, coef, as_bytes=True):
        """The count, scan, pack and assemble stages on given coefficients: coef int16 [plan["sizes"]["blocks"], 64] on the device,
        zigzag order, rows in scan order (what the first stage would have written)."""
        if coef.dtype != torch.int16 or tuple(coef.shape) != (plan["sizes"]["blocks"], 64):
            raise ValueError("JpegEncoder: coef must be int16 [%d, 64]" % plan["sizes"]["blocks"])
        return self._run(None, plan["staging"], plan["offs"], plan["sizes"], plan["n"], as_bytes, coef=coef)

    def _run(self, flat, staging, offs, sz, n, as_bytes, coef=None):
        """The launches.  coef: coefficients to code instead of the ones the first stage computes (the stage-level tests)."""
        dev = torch.from_numpy(staging).to(self.device, non_blocking=True)
        desc = dev[offs[0]:offs[0] + n * self.desc_ints * 4].view(torch.int32).view(n, self.desc_ints)
        quant = dev[offs[1]:offs[1] + 256].view(torch.int16).view(2, 64)
        headers = dev[offs[2]:offs[2] + sz["headers"]]
        if self._tables is None:
            self._tables = torch.from_numpy(code_table()).to(self.device)
        i32 = torch.int32
        blkbits, ivals = self._alloc((sz["blocks"],), i32), self._alloc((sz["intervals"],), i32)
        rawlen, status, ffcount, lengths = (self._alloc((n,), i32) for _ in range(4))
        offsets = self._alloc((n,), torch.int64)
        raw = self._alloc((sz["raw"],), torch.uint8)
        data = self._alloc((sz["data"],), torch.uint8)
        if coef is None:
            coef = self._alloc((sz["blocks"], 64), torch.int16)
            self._timed("blocks", K.jpeg_enc_blocks, flat, desc, sz["max_blocks"], quant, coef)
        self._timed("count", K.jpeg_enc_count, coef, desc, sz["max_blocks"], self._tables, blkbits, status)
        self._timed("scan", K.jpeg_enc_scan, desc, blkbits, ivals, rawlen, status)
        self._timed("pack", K.jpeg_enc_pack, coef, desc, sz["max_blocks"], self._tables, blkbits, ivals, rawlen, raw, status)
        self._timed("assemble", K.jpeg_enc_assemble, raw, desc, ivals, rawlen, headers, ffcount, data, offsets, lengths, status)
        self._stages = dict(desc=desc, coef=coef, blkbits=blkbits, ivals=ivals, rawlen=rawlen, raw=raw, sizes=sz)
        batch = EncodedBatch(data, offsets, lengths, status)
        if not as_bytes:
            return batch
        files = batch.to_bytes()
        self.downloaded_bytes = sum(len(f) for f in files) + 8 * n
        return files


_ROUNDTRIP_TABLES = {}      # (quality, device) -> int32 [64] on that device


def roundtrip_gray(images, quality=95, out=None):
    """The pixels of gray images after ``Image.fromarray(a).save(f, "JPEG", quality=quality)`` and ``Image.open(f).convert("L")``,
    bit for bit, without the file and without the entropy coding in between (csrc/jpeg_roundtrip.hip): one launch.

    images: uint8 [N, H, W] or [N, H, W, 1] on the device, contiguous or not (a non-contiguous tensor is copied first).  out: where to
    write (same shape, contiguous; ``images`` itself for an in-place call).  -> uint8 of the shape of ``images``."""
    from . import _lib
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("roundtrip_gray: quality is an integer 1 .. 100, got %r" % (quality,))
    if not torch.is_tensor(images) or images.dtype != torch.uint8:
        raise ValueError("roundtrip_gray: images are a uint8 tensor, got %s" % (images.dtype if torch.is_tensor(images) else type(images)))
    if images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[-1] != 1):
        raise ValueError("roundtrip_gray: images are [N, H, W] or [N, H, W, 1], got %s" % (tuple(images.shape),))
    if not images.is_cuda and not _lib.emulator_active():
        raise ValueError("roundtrip_gray: images must be on the device (there is no CPU path)")
    if min(images.shape) < 1 or images.shape[1] > 65535 or images.shape[2] > 65535:
        raise ValueError("roundtrip_gray: N >= 1, H and W 1 .. 65535, got %s" % (tuple(images.shape),))
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.shape != images.shape or out.device != images.device
                            or not out.is_contiguous()):
        raise ValueError("roundtrip_gray: out must be a contiguous uint8 tensor of the shape and device of images")
    shape = images.shape
    src = images.reshape(shape[:3]).contiguous()
    key = (quality, src.device)
    table = _ROUNDTRIP_TABLES.get(key)
    if table is None:
        table = _ROUNDTRIP_TABLES[key] = torch.from_numpy(quant_tables(quality)[0].astype(np.int32)).to(src.device)
    res = K.jpeg_roundtrip_gray(src, table, None if out is None else out.view(shape[:3]))
    return res.view(shape)
