"""The restart-interval index on the device (``ssn_jpeg_index`` in csrc/jpeg.hip, ``JpegDecoder(index="device")``) against the host
walk it replaces (``jpeg_decode._parse_scan`` / ``JpegDecoder._plan``).  Every criterion is equality.

The kernel is first held, on synthetic "scans", against ``host_walk`` below: a restatement of ``_parse_scan`` in a dozen lines of
Python that shares no code with the product.  The scans are seeded random bytes without any FF, with markers planted by hand at
the positions where the kernel changes hands: the last byte of a lane's 16, of a wave's 1024 and of a workgroup's chunk of 4096.
The synthetic strings are a few KB; one spans three chunks.  Then the decoder on real files (at most 64 x 48 pixels) against PIL
and against the host index: pixels, coefficients and the unit table row for row.
"""
import functools
import io
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import action_detection_amd  # noqa: F401
from action_detection_amd import jpeg_decode as J
from action_detection_amd import kernels as K
from action_detection_amd.jpeg_decode import CompressedBatchPrefetcher, JpegDecoder, parse_jpeg, parse_jpeg_header

LANE, WAVE, CHUNK = 16, 1024, 4096
REFUSED = 16


# ----------------------------------------------------------------------------------------------- the host walk, restated
def host_walk(data, units):
    """-> ([(begin, end)] * units, refused) of one file's bytes from its first scan byte on, as ``_parse_scan`` decides them.  For
    a file with too many restart markers the rows are what fits: the first ``units`` pieces."""
    n, i, cuts, end = len(data), 0, [], None
    while i + 1 < n:
        if data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF):
            if 0xD0 <= data[i + 1] <= 0xD7:
                cuts.append(i)
                i += 2                      # (the regex search does not overlap: FF Dn is consumed; Dn is no FF, so nothing is lost)
                continue
            end = i
            break
        i += 1
    end = n if end is None else end
    refused = len(cuts) > units - 1
    q = end
    while q + 4 <= n and data[q] == 0xFF and data[q + 1] != 0xD9:
        if data[q + 1] in (0xDA, 0xDC):
            refused = True
            break
        q += 1 if data[q + 1] == 0xFF else 2 + ((data[q + 2] << 8) | data[q + 3])
    bounds = [0] + [b for c in cuts for b in (c, c + 2)] + [end]
    pieces = [(bounds[k], bounds[k + 1]) for k in range(0, len(bounds), 2)]
    pieces += [(end, end)] * (units - len(pieces))
    return pieces[:units], refused


def test_host_walk_is_the_regex_walk():
    """The restatement against the product's own ``_parse_scan`` on real files: the same pieces."""
    for f in real_files():
        h = parse_jpeg(f)
        assert h.supported
        b0 = h.scan[0]
        pieces, refused = host_walk(f[b0:], len(h.units))
        assert not refused and [(b + b0, e + b0) for b, e in pieces] == [(u[0], u[1]) for u in h.units]


def noise(n, seed):
    """n seeded bytes, none of them FF."""
    return bytearray(np.random.RandomState(seed).randint(0, 255, n).astype(np.uint8).tobytes())


def plant(buf, at, *values):
    buf[at:at + len(values)] = bytes(values)
    return buf


class Batch(object):
    """Synthetic files -> the tables ``ssn_jpeg_index`` takes, laid out as ``JpegDecoder._plan_device`` lays them out (every file one
    table set unless ``sets`` says otherwise), inside guard bands when ``guard`` is set (host memory only)."""

    def __init__(self, backend, files, units, sets=None, guard=0):
        self.backend, self.files, self.units_of = backend, [bytes(f) for f in files], list(units)
        desc_ints, unit_ints, _, self.lds_sets = K.jpeg_layout()
        n = len(files)
        sets = list(sets) if sets is not None else [0] * n
        desc = np.zeros((n, desc_ints), np.int32)
        off = 0
        for i, f in enumerate(self.files):
            desc[i, 15], desc[i, 16] = off, off + len(f)
            off += -(-len(f) // 16) * 16
        bits = np.full(max(off, 16), 0xFF, np.uint8)      # (padding of FF: a read past a file's end would find a marker)
        for i, f in enumerate(self.files):
            bits[desc[i, 15]:desc[i, 16]] = np.frombuffer(f, np.uint8)
        rows, first = [], 0
        for i in sorted(range(n), key=lambda i: sets[i]):
            for k in range(self.units_of[i]):
                if len(rows) - first == 64 or (len(rows) > first and sets[i] - rows[first][5] >= self.lds_sets):
                    rows += [(-1, 0, 0, 0, 0, 0)] * (first + 64 - len(rows))
                    first = len(rows)
                if k == 0:
                    desc[i, 17] = len(rows)
                rows.append((i, 0, 0, k, 1, sets[i]))
            desc[i, 18] = self.units_of[i]
        rows += [(-1, 0, 0, 0, 0, 0)] * (-(-max(len(rows), 1) // 64) * 64 - len(rows))
        urows = np.zeros((len(rows), unit_ints), np.int32)
        urows[:, :6] = np.array(rows, np.int64)
        self.desc_host, self.urows_host = desc, urows.copy()
        self.bands = []
        self.bits = self.place(torch.from_numpy(bits), guard)
        self.desc = backend.put(torch.from_numpy(desc.copy()))
        self.units = self.place(torch.from_numpy(urows), guard)
        self.refused = self.place(torch.full((n,), 0x5A5A, dtype=torch.int32), guard)

    def place(self, t, guard):
        if not guard:
            return self.backend.put(t)
        big = torch.full((t.numel() + 2 * guard,), 0x5A, dtype=t.dtype)
        big[guard:guard + t.numel()] = t.reshape(-1)
        self.bands.append((big, guard, t.numel()))
        return big[guard:guard + t.numel()].view(t.shape)

    def run(self, desc=None):
        K.jpeg_index(self.bits, self.desc if desc is None else desc, self.units, self.refused)
        return self.units.cpu().numpy(), self.refused.cpu().numpy()

    def guards_intact(self):
        return all((big[:g] == 0x5A).all() and (big[g + n:] == 0x5A).all() for big, g, n in self.bands)

    def expected(self):
        """The unit table the host walk gives, and its verdicts."""
        want, refused = self.urows_host.copy(), []
        for i, f in enumerate(self.files):
            pieces, no = host_walk(f, self.units_of[i])
            refused.append(REFUSED if no else 0)
            r0, b0 = self.desc_host[i, 17], self.desc_host[i, 15]
            for k, (b, e) in enumerate(pieces):
                want[r0 + k, 1:3] = (b + b0, e + b0)
        return want, np.array(refused, np.int32)

    def check(self):
        got, refused = self.run()
        want, verdicts = self.expected()
        assert np.array_equal(refused, verdicts), (refused.tolist(), verdicts.tolist())
        assert np.array_equal(got, want), "rows %r differ" % np.nonzero((got != want).any(axis=1))[0].tolist()
        return got, refused


# ----------------------------------------------------------------------------------------------- the kernel on synthetic scans
def test_markers_across_lane_wave_and_chunk_edges(backend):
    """1. FF in the last byte of a lane's 16, of a wave's span and of a chunk, Dn (or the ending marker's code) in the next."""
    n = 2 * CHUNK + 700                                  # (the one string that spans three chunks)
    restart = noise(n, 1)
    edges = [LANE - 1, 5 * LANE - 1, WAVE - 1, 3 * WAVE - 1, CHUNK - 1, 2 * CHUNK - 1]
    for k, e in enumerate(edges):
        plant(restart, e, 0xFF, 0xD0 + k % 8)
    plant(restart, n - 40, 0xFF, 0xD9)
    files, units = [restart], [len(edges) + 1]
    for e in edges:                                      # the ending marker on every such edge, restart markers on both sides of it
        f = noise(e + 300, 2 + e)
        plant(f, 7, 0xFF, 0xD0)
        plant(f, e, 0xFF, 0xD9)
        plant(f, e + 100, 0xFF, 0xD1)
        files.append(f)
        units.append(2)
    got, refused = Batch(backend, files, units).check()
    assert not refused.any()
    assert [int(x) for x in got[:len(edges), 2]] == edges          # (file 0 lies at offset 0: its units end at the edges)


def test_stuffing_fill_bytes_and_ends(backend):
    """2. FF 00 next to a marker, FF FF Dn, FF as the last byte, no marker at all, an empty scan."""
    stuffed = plant(plant(noise(600, 3), 100, 0xFF, 0x00, 0xFF, 0xD0, 0xFF, 0x00), 300, 0xFF, 0x00, 0xFF, 0xD9)
    fill = plant(plant(noise(600, 4), 15, 0xFF, 0xFF, 0xD0), 200, 0xFF, 0xFF, 0xFF, 0xD9)
    last_ff = plant(plant(noise(LANE * 3, 5), 20, 0xFF, 0xD0), LANE * 3 - 1, 0xFF)
    last_ff_edge = plant(noise(CHUNK, 6), CHUNK - 1, 0xFF)
    no_marker = noise(1000, 7)
    empty = b""
    only_eoi = bytes([0xFF, 0xD9])
    files = [stuffed, fill, last_ff, last_ff_edge, no_marker, empty, only_eoi]
    b = Batch(backend, files, [2, 2, 2, 1, 3, 2, 1])
    got, refused = b.check()
    assert not refused.any()
    r = [int(x) for x in b.desc_host[:, 17]]
    o = [int(x) for x in b.desc_host[:, 15]]
    assert tuple(got[r[0], 1:3] - o[0]) == (0, 102) and tuple(got[r[0] + 1, 1:3] - o[0]) == (104, 302)
    assert tuple(got[r[1], 1:3] - o[1]) == (0, 16) and tuple(got[r[1] + 1, 1:3] - o[1]) == (18, 202)      # the fill byte stays
    assert tuple(got[r[2] + 1, 1:3] - o[2]) == (22, LANE * 3)
    assert tuple(got[r[3], 1:3] - o[3]) == (0, CHUNK)
    assert [tuple(x - o[4]) for x in got[r[4]:r[4] + 3, 1:3]] == [(0, 1000), (1000, 1000), (1000, 1000)]
    assert [tuple(x - o[5]) for x in got[r[5]:r[5] + 2, 1:3]] == [(0, 0), (0, 0)]


def test_what_lies_behind_the_scan(backend):
    """3. Restart markers behind the end are ignored; a fake SOS or a DNL among the segments behind it refuses the file."""
    ignored = plant(plant(plant(noise(900, 8), 50, 0xFF, 0xD0), 400, 0xFF, 0xD9), 600, 0xFF, 0xD1)
    app = bytes([0xFF, 0xE1, 0x00, 0x06, 1, 2, 3, 4])
    sos = plant(noise(500, 9), 300, *(app + bytes([0xFF, 0xFF, 0xDA, 0x00, 0x08])))      # (a fill byte in front of the SOS)
    dnl = plant(noise(500, 10), 300, *(app + bytes([0xFF, 0xDC, 0x00, 0x04, 0, 9])))
    harmless = plant(noise(500, 11), 300, *(app + bytes([0xFF, 0xD9, 0xFF, 0xDA, 0, 8])))      # the walk stops at EOI
    short = plant(noise(303, 12), 300, 0xFF, 0xDA, 0x00)                                        # no room for a segment: not walked
    got, refused = Batch(backend, [ignored, sos, dnl, harmless, short], [2, 1, 1, 1, 1]).check()
    assert refused.tolist() == [0, REFUSED, REFUSED, 0, 0]


def test_marker_counts_against_the_header(backend):
    """4. Fewer markers than promised, exactly as many, one more, and markers without an interval."""
    def with_markers(m, seed):
        f = noise(2000, seed)
        for k in range(m):
            plant(f, 100 + 90 * k, 0xFF, 0xD0 + k % 8)
        return plant(f, 1900, 0xFF, 0xD9)
    files = [with_markers(3, 13), with_markers(6, 14), with_markers(7, 15), with_markers(2, 16), with_markers(0, 17)]
    b = Batch(backend, files, [7, 7, 7, 1, 1])
    got, refused = b.check()
    assert refused.tolist() == [0, 0, REFUSED, REFUSED, 0]
    o, r = int(b.desc_host[0, 15]), int(b.desc_host[0, 17])
    assert [tuple(x - o) for x in got[r + 4:r + 7, 1:3]] == [(1900, 1900)] * 3
    r3 = int(b.desc_host[3, 17])                          # the refused files wrote their own rows only
    assert tuple(got[r3 + 1, 1:3] - int(b.desc_host[4, 15])) == (0, 1900)


@pytest.mark.parametrize("units", [1, 63, 64, 65, 130])
def test_unit_counts_at_the_row_boundaries(backend, units):
    """5a. A file whose units end at, and cross, the rows of 64 of the unit table."""
    f = noise(3 * units + 50, 18 + units)
    for k in range(units - 1):
        plant(f, 3 * k + 1, 0xFF, 0xD0 + k % 8)
    got, refused = Batch(backend, [f], [units]).check()
    assert not refused.any() and len(got) == -(-units // 64) * 64


def test_files_sharing_workgroups_and_more_sets_than_lds(backend):
    """5b. Several files in the rows of one workgroup; more table sets than a workgroup holds, so that padding rows appear."""
    files, units = [], []
    for i in range(12):
        m = [3, 1, 40, 7][i % 4]
        f = noise(200 + 3 * m, 40 + i)
        for k in range(m - 1):
            plant(f, 10 + 3 * k, 0xFF, 0xD0 + k % 8)
        files.append(f)
        units.append(m)
    sets = [(5 * i) % 12 for i in range(12)]
    b = Batch(backend, files, units, sets=sets)
    assert 12 > b.lds_sets
    got, refused = b.check()
    assert not refused.any()
    pad = got[got[:, 0] < 0]
    assert len(pad) and not pad[:, 1:].any()              # padding rows: (-1, 0, 0, 0, 0, 0, 0, 0), as _plan writes them
    assert len({int(b.desc_host[i, 17]) // 64 for i in range(12)}) < 12      # (rows of several files in one workgroup)


def test_bad_file_rows_are_clamped(emu):
    """6. Emulator only: table, bits and verdicts inside guard bands; rows that lie about their ranges write nothing outside."""
    class Host(object):
        device = "cpu"

        def put(self, t):
            return t
    f = noise(600, 60)
    for k in range(5):
        plant(f, 50 + 20 * k, 0xFF, 0xD0 + k)
    good = plant(noise(300, 61), 100, 0xFF, 0xD0)
    lies = [(15, 1 << 20), (16, 1 << 30), (15, -16), (16, -5), (15, 7), (18, 1000), (18, -3), (17, 1 << 20), (17, -1), (17, 64),
            (17, 60), (17, 0), (18, (1 << 31) - 1), (17, -(1 << 31))]
    for col, value in lies:
        b = Batch(Host(), [good, f, good], [2, 6, 2], guard=4096)
        desc = b.desc.clone()
        desc[1, col] = value
        got, refused = b.run(desc)
        assert b.guards_intact(), "column %d = %d wrote a guard band" % (col, value)
        assert refused[1] & (8 | REFUSED), (col, value)
        assert refused[0] == 0 and refused[2] == 0
        want, _ = b.expected()
        for i in (0, 2):                                  # the neighbours' rows are what they would have been
            r = int(b.desc_host[i, 17])
            assert np.array_equal(got[r:r + 2], want[r:r + 2]), (col, value)
    b = Batch(Host(), [good, f, good], [2, 6, 2], guard=4096)
    b.check()
    assert b.guards_intact()


def test_wrapper_validates_before_any_launch(backend):
    """7. dtype, shape, alignment and row counts."""
    b = Batch(backend, [noise(100, 70)], [1])
    K.jpeg_index(b.bits, b.desc, b.units, b.refused)
    with pytest.raises(ValueError):
        K.jpeg_index(b.bits.to(torch.int32), b.desc, b.units, b.refused)
    with pytest.raises(ValueError):
        K.jpeg_index(b.bits, b.desc[:, :8].contiguous(), b.units, b.refused)
    with pytest.raises(ValueError):
        K.jpeg_index(b.bits, b.desc, b.units[:63].contiguous(), b.refused)
    with pytest.raises(ValueError):
        K.jpeg_index(b.bits, b.desc, b.units.to(torch.int64), b.refused)
    with pytest.raises(ValueError):
        K.jpeg_index(b.bits, b.desc, b.units, b.refused.to(torch.int16))
    with pytest.raises(ValueError):
        K.jpeg_index(b.bits, b.desc, b.units, torch.cat([b.refused, b.refused]))
    with pytest.raises(ValueError):
        K.jpeg_index(b.bits[1:], b.desc, b.units, b.refused)      # (a view that starts one byte in: misaligned)
    with pytest.raises(ValueError):
        K.jpeg_index_status(b.refused, b.refused.to(torch.int64))
    with pytest.raises(ValueError):
        K.jpeg_index_status(b.refused, torch.cat([b.refused, b.refused]))


# ----------------------------------------------------------------------------------------------- the decoder on real files
def picture(h, w, gray, seed=0):
    rs = np.random.RandomState(seed * 7 + h * 131 + w)
    c = 1 if gray else 3
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(xx / 7.0 + k) * np.cos(yy / 5.0 - k) for k in range(c)], 2) + rs.randint(-20, 20, (h, w, c))
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a[:, :, 0] if gray else a


@functools.lru_cache(maxsize=None)
def jpeg(h, w, sampling, quality=75, **extra):
    b = io.BytesIO()
    kw = dict(quality=quality, **extra)
    if sampling is not None:
        kw["subsampling"] = sampling
    Image.fromarray(picture(h, w, sampling is None, quality)).save(b, "JPEG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def pil(data, mode):
    a = np.asarray(Image.open(io.BytesIO(data)).convert(mode))
    a = a if a.ndim == 3 else a[:, :, None]
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def real_files():
    """Gray, 4:4:4, 4:2:2, 4:2:0; sizes that are no multiple of the MCU; restart intervals of 1, 3 and more than the image's MCUs,
    of one MCU row, and none; optimised tables for a second table set."""
    out = []
    for s in (None, 0, 1, 2):
        out += [jpeg(37, 53, s), jpeg(37, 53, s, restart_marker_blocks=1), jpeg(37, 53, s, restart_marker_blocks=3),
                jpeg(37, 53, s, restart_marker_blocks=1000), jpeg(48, 64, s, 90, restart_marker_rows=1),
                jpeg(31, 15, s, 95, optimize=True, restart_marker_blocks=3), jpeg(17, 33, s, 50, optimize=True)]
    return tuple(out)


def test_real_files_are_what_they_claim():
    hs = [parse_jpeg(f) for f in real_files()]
    assert all(h.supported for h in hs)
    assert {h.restart_interval for h in hs} >= {0, 1, 3, 1000}
    assert len({h.table_key for h in hs}) >= 3 and max(len(h.units) for h in hs) >= 35
    assert {(len(h.components), h.hs, h.vs) for h in hs} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}


def test_decode_equals_pil_and_the_host_index(backend):
    """8. Pixels in both modes, stack=True included, and the coefficients."""
    files = list(real_files())
    for mode in ("RGB", "L"):
        host, dev = JpegDecoder(backend.device), JpegDecoder(backend.device, index="device")
        a, b = host.decode(files, mode), dev.decode(files, mode)
        assert dev.fallbacks == 0 and not dev.status.cpu().any()
        for f, x, y in zip(files, a, b):
            assert torch.equal(x, y) and np.array_equal(y.cpu().numpy(), pil(f, mode))
        same = [f for f in files if pil(f, "L").shape == (37, 53, 1)]
        a, b = host.decode(same, mode, stack=True), dev.decode(same, mode, stack=True)
        assert b.shape == (len(same), 37, 53, 3 if mode == "RGB" else 1) and torch.equal(a, b)
        assert all(np.array_equal(y.cpu().numpy(), pil(f, mode)) for f, y in zip(same, b))
    host, dev = JpegDecoder(backend.device), JpegDecoder(backend.device, index="device")
    a, b = host.coefficients(files), dev.coefficients(files)
    assert torch.equal(a.coef, b.coef) and torch.equal(a.desc[:, :15], b.desc[:, :15]) and np.array_equal(a.rows[:, :15], b.rows[:, :15])
    assert a.max_blocks == b.max_blocks and not b.status.cpu().any()
    assert all(h.supported and h.units == [] and h.scan == (parse_jpeg(f).scan[0], len(f)) for f, h in zip(files, b.headers))
    for i in range(len(files)):
        assert torch.equal(a.blocks(i), b.blocks(i))


def test_unit_table_equals_the_host_plan(backend):
    """9. Row for row, begin / end relative to each file's first scan byte."""
    files = list(real_files())
    random.Random(3).shuffle(files)
    host, dev = JpegDecoder(backend.device), JpegDecoder(backend.device, index="device")
    host.decode(files, "L")
    dev.decode(files, "L")
    tables = []
    for d in (host, dev):
        u = d._unit_rows.cpu().numpy().copy()
        assert len(u) > 128                               # (more than two workgroups of rows)
        first = {}
        for r in u:                                       # (a file's first row is its unit 0: the file's first scan byte)
            if r[0] >= 0 and r[0] not in first:
                first[r[0]] = r[1]
        for r in u:
            if r[0] >= 0:
                r[1:3] -= first[r[0]]
        tables.append(u)
    assert len({tuple(sorted(parse_jpeg(f).huffman.items())) for f in files}) > 1
    assert np.array_equal(tables[0], tables[1])


def progressive_file():
    b = io.BytesIO()
    Image.fromarray(picture(37, 53, False)).save(b, "JPEG", quality=75, progressive=True)
    return b.getvalue()


def test_one_batch_mixing_verdicts(backend):
    """10. Good files, a progressive one, a second SOS behind the scan, one restart marker too many, a truncated file."""
    good = [jpeg(37, 53, 2), jpeg(48, 64, None, 90, restart_marker_rows=1), jpeg(37, 53, 1, restart_marker_blocks=3)]
    prog = progressive_file()
    base = jpeg(37, 53, 0, restart_marker_blocks=3)
    assert base.endswith(b"\xff\xd9")
    second_scan = base[:-2] + bytes([0xFF, 0xDA, 0x00, 0x08, 1, 1, 0, 0, 63, 0]) + b"\x12\x34" + b"\xff\xd9"
    h = parse_jpeg(base)
    b1, e1 = h.units[1][:2]
    mid = (b1 + e1) // 2
    one_more = base[:mid] + b"\xff\xd3" + base[mid:]
    cut = base[:(h.units[2][0] + h.units[2][1]) // 2]
    assert "more than one scan" in parse_jpeg(second_scan).reason and "more restart markers" in parse_jpeg(one_more).reason
    assert parse_jpeg(cut).supported
    files = [good[0], prog, second_scan, good[1], one_more, cut, good[2]]
    dec = JpegDecoder(backend.device, index="device")
    out = dec.decode(files, "RGB")
    assert dec.fallbacks == 1                             # the progressive file, at decode time
    status = dec.status.cpu().tolist()
    assert [bool(s & REFUSED) for s in status] == [False, False, True, False, True, False, False]
    assert status[5] & 1 and [status[i] for i in (0, 1, 3, 6)] == [0, 0, 0, 0]
    for i in (0, 1, 3, 6):
        assert np.array_equal(out[i].cpu().numpy(), pil(files[i], "RGB"))
    for f in (second_scan, cut):                          # PIL opens neither of these: check() raises what PIL raises
        with pytest.raises(OSError):
            pil(f, "RGB")
    with pytest.raises(OSError):
        dec.check()
    # the files of these that PIL can open, and a DNL segment behind the scan (libjpeg skips it) in the second scan's place
    dnl = base[:-2] + bytes([0xFF, 0xDC, 0x00, 0x04, 0, 37]) + b"\xff\xd9"
    assert "DNL" in parse_jpeg(dnl).reason
    files = [good[0], prog, dnl, good[1], one_more, good[2]]
    dec = JpegDecoder(backend.device, index="device")
    out = dec.decode(files, "RGB")
    assert dec.fallbacks == 1 and [s & REFUSED for s in dec.status.cpu().tolist()] == [0, 0, REFUSED, 0, REFUSED, 0]
    assert dec.check() == [2, 4] and dec.fallbacks == 3
    for f, o in zip(files, out):
        assert np.array_equal(o.cpu().numpy(), pil(f, "RGB"))


def test_parse_jpeg_header_agrees_with_parse_jpeg():
    """11. Every header field; and a file that starts like the last one but has another header is parsed, not served."""
    fields = ("supported", "width", "height", "components", "selectors", "huffman", "restart_interval", "hs", "vs", "table_key",
              "quant_keys", "table_select")
    files = list(real_files())
    for f in files + files[::-1] + [files[0], files[0]]:
        a, b = parse_jpeg(f), parse_jpeg_header(f)
        for name in fields:
            assert getattr(a, name) == getattr(b, name), name
        assert set(a.qtables) == set(b.qtables) and all(np.array_equal(a.qtables[k], b.qtables[k]) for k in a.qtables)
        assert b.scan == (a.scan[0], len(f)) and b.units == []
    a, b = jpeg(37, 53, 2), jpeg(37, 61, 2)               # same encoder, quality and tables: equal up to the frame header
    common = os.path.commonprefix([a, b])
    assert 20 < len(common) < parse_jpeg(a).scan[0]
    assert parse_jpeg_header(a).width == 53 and parse_jpeg_header(b).width == 61 and parse_jpeg_header(a).width == 53
    assert not parse_jpeg_header(progressive_file()).supported and "progressive" in parse_jpeg_header(progressive_file()).reason
    assert not parse_jpeg_header(b"GIF89a" + bytes(40)).supported
    for n in range(0, len(a), 7):                         # every prefix answers, none raises
        h = parse_jpeg_header(a[:n])
        assert h.supported or h.reason


class Proposal(object):
    def __init__(self, video_id, frame_indices):
        self.video_id, self.frame_indices = video_id, frame_indices


class Sampler(object):
    """Two proposals of three snippets per video, fixed."""

    def __init__(self, videos):
        self.videos = videos

    def __len__(self):
        return len(self.videos)

    def sample_video(self, index):
        rs = np.random.RandomState(index)
        props = [Proposal(self.videos[index], [1, 3, 4]), Proposal(self.videos[index], [2, 2, 5])]
        return props, dict(scaling=rs.rand(2, 2).astype(np.float32), labels=np.array([1, 0]), reg_targets=rs.randn(2, 2).astype(np.float32),
                           prop_type=np.array([0, 2]))


@pytest.mark.parametrize("modality", ["RGB", "Flow"])
def test_prefetcher_with_the_device_index(backend, modality, tmp_path):
    """12. The tensors of the host-index prefetcher, on a small synthetic frame directory."""
    from action_detection_amd import train_data as D
    from action_detection_amd.input_pipeline import GpuTrainAugment
    videos = ["video_a", "video_b", "video_c", "video_d"]
    for v, name in enumerate(videos):
        os.makedirs(str(tmp_path / name))
        for i in range(1, 6):
            if modality == "RGB":
                Image.fromarray(picture(40, 52, False, seed=10 * v + i)).save(str(tmp_path / name / ("img_%05d.jpg" % i)), quality=75,
                                                                              subsampling=2, restart_marker_rows=1)
            else:
                for k, axis in enumerate("xy"):
                    Image.fromarray(picture(40, 52, True, seed=100 * v + 2 * i + k)).save(
                        str(tmp_path / name / ("flow_%s_%05d.jpg" % (axis, i))), quality=95, restart_marker_rows=1)
    flow = modality == "Flow"
    aug = GpuTrainAugment(32, [128] if flow else [104, 117, 128], [1], [1, .875, .75], roll=True, is_flow=flow, device=backend.device)
    group = 3 * (2 if flow else 1)
    sampler = Sampler(videos)
    got = {}
    for index in ("host", "device"):
        random.seed(21)
        pre = CompressedBatchPrefetcher(D.compressed_ssn_batches(sampler, D.CompressedFrameDirReader(str(tmp_path), modality, "flow_"), 2),
                                        aug, group_size=group, index=index)
        assert pre.decoder.index == index
        got[index] = list(pre)
        assert pre.decoder.fallbacks == 0 and not pre.decoder.status.cpu().any()
    assert len(got["host"]) == len(got["device"]) == 2
    for g, w in zip(got["device"], got["host"]):
        assert g[0].shape == (2, 2 * group * (1 if flow else 3), 32, 32)
        for a, b in zip(g, w):
            assert a.device == b.device and torch.equal(a.cpu(), b.cpu())


def test_host_work_does_not_grow_with_the_units(emu, monkeypatch):
    """13. CPU only.  With index="device" neither ``_parse_scan`` nor a regex search runs, and the Python-level calls of planning a
    batch are as many for a file of 130 units as for a file of one."""
    def forbidden(*a, **k):
        raise AssertionError("the host walked a scan")
    monkeypatch.setattr(J, "_parse_scan", forbidden)

    class NoSearch(object):
        def finditer(self, *a, **k):
            forbidden()
        search = match = findall = finditer
    monkeypatch.setattr(J, "_MARKER", NoSearch())      # (re.Pattern itself cannot be patched: the module's one pattern is replaced)
    one = jpeg(48, 64, None, 90)
    many = jpeg(80, 104, None, 90, restart_marker_blocks=1)
    assert len(many) < 8192
    dec = JpegDecoder("cpu", index="device")
    counts = {}
    for name, f in (("warm", many), ("one", one), ("many", many), ("one again", one)):
        headers = [parse_jpeg_header(f)] * 3
        dec._out_off = [0, 1, 2, 3]
        calls = [0]

        def count(frame, event, arg):
            if event in ("call", "c_call"):
                calls[0] += 1
        sys.setprofile(count)
        try:
            _, _, sz, _ = dec._plan_device([f] * 3, headers)
        finally:
            sys.setprofile(None)
        counts[name] = (calls[0], sz["units"])
    assert counts["one"][1] == 64 and counts["many"][1] == -(-3 * 130 // 64) * 64
    assert counts["one"][0] == counts["many"][0] == counts["one again"][0], counts
    out = dec.decode([one, many], "L")
    assert dec.fallbacks == 0 and not dec.status.any()
    assert np.array_equal(out[0].numpy(), pil(one, "L")) and np.array_equal(out[1].numpy(), pil(many, "L"))
