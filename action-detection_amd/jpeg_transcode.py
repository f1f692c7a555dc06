"""Lossless JPEG transcoding on the device: ``jpegtran -restart`` for a whole frame store.

The decoder's Huffman stage walks a file without restart markers as ONE sequential chain on one lane; with restart markers it
takes one lane per interval.  Frames written by dense_flow, OpenCV or PIL carry none.  ``JpegTranscoder.transcode``
reads such files, keeps every quantised coefficient and writes the same pictures with a restart marker every K MCUs:

  ``JpegDecoder.coefficients``   marker walk, upload, entropy launch: the coefficients, natural order, blocks planar
  ``ssn_jpeg_transcode_blocks``  csrc/jpeg_transcode.hip: the same values in zigzag order, blocks in scan order
  ``JpegEncoder.encode_coefficients``   count, scan, pack, assemble: the files, with the SOURCE's quantisation tables in the header

No coefficient and no quantisation table changes, so a decoder computes the same pixels from the output as from the source
(DESIGN.md 3.13); the Huffman tables of the output are the standard ones whatever the source used.  The output header is the
encoder's (PIL's default header + the source's tables + DRI): the source's APPn and COM segments -- EXIF, ICC profile, comments,
pixel density -- are NOT carried over.
"""
import numpy as np
import torch

from . import kernels as K
from .jpeg_decode import JpegDecoder
from .jpeg_encode import ST_CAPACITY, ST_DESC, ST_RANGE, EncodedBatch, JpegEncoder

ST_SOURCE = 8      # EncodedBatch.status of a transcoded batch: the source's scan was damaged (the decoder's status was non-zero)

REASON_RANGE = "a coefficient the standard Huffman tables cannot code"
REASON_CHROMA = "Cb and Cr use different quantisation tables"
REASON_QUANT = "a quantisation table with an entry of 0"


def _restart_argument(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= value <= 65535:
        raise ValueError("JpegTranscoder: %s is an integer 0 (no markers) .. 65535, got %r" % (name, value))
    return int(value)


class JpegTranscoder(object):
    """``transcode(blobs, restart_blocks=None, restart_rows=None, as_bytes=True)``: every file of ``blobs`` (baseline JPEG, ``bytes``)
    again, the same coefficients and quantisation tables, with the restart interval asked for -> a list of ``bytes``.

    Exactly one of the two arguments is given.  ``restart_blocks=K``: K MCUs per interval (PIL's ``restart_marker_blocks``);
    ``restart_rows=R``: K = R x the MCUs of a row of each image (PIL's ``restart_marker_rows``).  K = 0 writes no DRI segment and
    no markers (restart markers the source had are removed).  A K larger than an image's MCU count is CLAMPED as libjpeg clamps it:
    the scan is one interval without a marker and the DRI segment still states K -- the bytes PIL writes for that K.

    A file of PIL (libjpeg's standard Huffman tables, ``optimize=False``) comes back as the bytes
    ``Image.save(..., restart_marker_blocks=K)`` writes for the same picture, quality and subsampling.

    Files that are not transcoded come back UNCHANGED, byte for byte, and ``skipped`` lists them as ``(index, reason)``: files
    ``parse_jpeg`` does not support (progressive, CMYK, 4:1:1, 4:4:0, 16-bit quantisation tables, an Adobe APP14 segment that says
    RGB or YCCK, ...: the output header is JFIF, which means YCbCr, so only files ``parse_jpeg`` found to be YCbCr or gray are
    taken); files whose Cb and Cr name different quantisation tables (the output header has one chroma table); files whose scan is
    damaged; files with a coefficient the standard tables have no code for.  The other files of the batch are not affected.  The
    last two cases are found by ONE host read of the status words at the end of the call.

    Metadata: the output header is PIL's default one (JFIF 1.01, no units, density 1 x 1).  The source's APPn / COM segments (EXIF,
    ICC profile, comments, density) are dropped.

    ``as_bytes=False``: no host read at all -> an ``EncodedBatch`` over ALL files of ``blobs``, as ``JpegEncoder`` returns one.  A
    file skipped on the host has length 0 and is in ``skipped``; a file found unusable on the device has length 0 and a non-zero
    status (2: coefficient out of range, 8: damaged source scan): take the source file for both."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.decoder = JpegDecoder(device)
        self.encoder = JpegEncoder(device)
        self.desc_ints = K.jpeg_transcode_layout()
        self.skipped = []
        self.profile = None          # a list: transcode() appends (stage, start event, end event) of every launch it enqueues
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

    @staticmethod
    def _tables_of(h):
        """-> ([luma, chroma] tables for the output header, None) or (None, the reason the file is not taken)"""
        tabs = [h.qtables[c[3]] for c in h.components]
        if len(tabs) == 3 and h.quant_keys[1] != h.quant_keys[2]:
            return None, REASON_CHROMA
        tabs = tabs[:2]
        if any(int(t.min()) < 1 for t in tabs):
            return None, REASON_QUANT
        return tabs, None

    def transcode(self, blobs, restart_blocks=None, restart_rows=None, as_bytes=True):
        if (restart_blocks is None) == (restart_rows is None):
            raise ValueError("JpegTranscoder: give exactly one of restart_blocks= and restart_rows=")
        if restart_blocks is not None:
            restart_blocks = _restart_argument("restart_blocks", restart_blocks)
        else:
            restart_rows = _restart_argument("restart_rows", restart_rows)
        blobs = [bytes(b) for b in blobs]
        if not blobs:
            raise ValueError("JpegTranscoder: no files")
        n = len(blobs)
        self.skipped = []
        self.decoder.profile = self.encoder.profile = self.profile
        batch = self.decoder.coefficients(blobs)
        kept, specs = [], []
        for i, h in enumerate(batch.headers):
            if not h.supported:
                self.skipped.append((i, "unsupported: %s" % h.reason))
                continue
            tabs, why = self._tables_of(h)
            if why:
                self.skipped.append((i, why))
                continue
            k = restart_blocks if restart_blocks is not None else restart_rows * h.mcus[0]
            if k > 65535:
                raise ValueError("JpegTranscoder: restart_rows=%d is %d MCUs in file %d, a restart interval holds 65535 at most"
                                 % (restart_rows, k, i))
            kept.append(i)
            specs.append((h.height, h.width, len(h.components), h.hs, h.vs, tabs, k))
        if not kept:
            self._stages = None
            if as_bytes:
                return blobs
            zero = torch.zeros(n, dtype=torch.int32, device=self.device)
            return EncodedBatch(self._alloc((1,), torch.uint8), torch.zeros(n, dtype=torch.int64, device=self.device), zero, zero.clone())
        plan = self.encoder.plan_coefficients(specs)
        rows = np.zeros((len(kept), self.desc_ints), np.int32)
        for j, i in enumerate(kept):
            h = batch.headers[i]
            mx, my = h.mcus
            src_off, nblocks = int(batch.rows[i, 7]), int(batch.rows[i, 8])
            if nblocks != int(plan["desc"][j, 9]):
                raise RuntimeError("JpegTranscoder: file %d has %d blocks for the decoder and %d for the encoder"
                                   % (i, nblocks, int(plan["desc"][j, 9])))
            rows[j] = (len(h.components), h.hs, h.vs, mx, my, src_off, int(plan["desc"][j, 8]), nblocks)
        desc = torch.from_numpy(rows).to(self.device, non_blocking=True)
        coef = self._alloc((plan["sizes"]["blocks"], 64), torch.int16)      # (every row belongs to one image: all of it is written)
        layout_status = self._alloc((len(kept),), torch.int32)
        self._timed("layout", K.jpeg_transcode_blocks, batch.coef, desc, plan["sizes"]["max_blocks"], coef, layout_status)
        out = self.encoder.encode_coefficients(plan, coef, as_bytes=False)
        index = torch.tensor(kept, dtype=torch.int64).to(self.device, non_blocking=True)
        damaged = (batch.status[index] != 0).to(torch.int32) * ST_SOURCE
        status = out.status | layout_status | damaged
        self._stages = dict(source=batch, desc=desc, coef=coef, plan=plan, kept=kept, encoded=out)
        if not as_bytes:
            full_status = torch.zeros(n, dtype=torch.int32, device=self.device)
            full_lengths = torch.zeros(n, dtype=torch.int32, device=self.device)
            full_offsets = torch.zeros(n, dtype=torch.int64, device=self.device)
            full_status[index] = status
            full_lengths[index] = torch.where(status != 0, torch.zeros_like(out.lengths), out.lengths)
            full_offsets[index] = out.offsets
            return EncodedBatch(out.data, full_offsets, full_lengths, full_status)
        # the host reads: the status words and lengths, then exactly the bytes of the files
        words = torch.stack([status, out.lengths, batch.status[index]]).cpu().numpy()
        lengths = words[1].tolist()
        blob = out.data[:sum(lengths)].cpu().numpy().tobytes()
        files, o = list(blobs), 0
        for j, i in enumerate(kept):
            st = int(words[0, j])
            if st & (ST_CAPACITY | ST_DESC):
                raise RuntimeError("JpegTranscoder: file %d was not written (status %d)" % (i, st))
            if st & ST_SOURCE:
                self.skipped.append((i, "damaged scan (decoder status %d)" % int(words[2, j])))
            elif st & ST_RANGE:
                self.skipped.append((i, REASON_RANGE))
            else:
                files[i] = blob[o:o + lengths[j]]
            o += lengths[j]
        self.skipped.sort()
        return files
