"""Lossless JPEG transcoding on the device (csrc/jpeg_transcode.hip, jpeg_transcode.py): the same coefficients, new restart intervals.

Every criterion is exact.  Where PIL can write the wanted file itself the criterion is ``bytes == PIL's bytes``: a PIL file without
restart markers, transcoded to an interval of K MCUs, is the file PIL writes for the same picture with ``restart_marker_blocks=K``
(libjpeg computes the same coefficients for both and its standard Huffman tables are the encoder's).  Where it cannot (optimised
Huffman tables, custom quantisation tables), the criterion is what lossless means: PIL decodes output and source to the same pixels,
the quantisation tables are the source's and the coefficients the device decoder reads from the two files are equal.  Pictures and
shapes are those of tests/test_jpeg_encode.py (the smallest at which each mechanism can fail).
"""
import functools
import importlib.util
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import action_detection_amd  # noqa: F401
from action_detection_amd import kernels as K
from action_detection_amd.jpeg_decode import JpegDecoder, parse_jpeg
from action_detection_amd.jpeg_transcode import REASON_RANGE, JpegTranscoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 33), (31, 15), (40, 9), (37, 53), (64, 80)]
SAMPLINGS = [None, 0, 1, 2]          # gray, 4:4:4, 4:2:2, 4:2:0
FACTORS = {None: (1, 1), 0: (1, 1), 1: (2, 1), 2: (2, 2)}
QUALITIES = [10, 75, 100]
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


@functools.lru_cache(maxsize=None)
def picture(h, w, sampling, seed=0):
    rs = np.random.RandomState(seed * 7 + h * 131 + w)
    c = 1 if sampling is None else 3
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(xx / 7.0 + k) * np.cos(yy / 5.0 - k) for k in range(c)], 2) + rs.randint(-20, 20, (h, w, c))
    a = np.clip(a, 0, 255).astype(np.uint8)
    a = a[:, :, 0] if c == 1 else a
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pil_file(h, w, sampling, quality=75, blocks=0, rows=0, **more):
    """The yardstick (and the sources), made once per case and shared."""
    kw = dict(quality=quality, **more)
    if sampling is not None:
        kw["subsampling"] = sampling
    if blocks:
        kw["restart_marker_blocks"] = blocks
    if rows:
        kw["restart_marker_rows"] = rows
    b = io.BytesIO()
    Image.fromarray(picture(h, w, sampling, quality)).save(b, "JPEG", **kw)
    return b.getvalue()


def mcus(h, w, sampling):
    hs, vs = FACTORS[sampling]
    return -(-w // (8 * hs)), -(-h // (8 * vs))


def pil_pixels(blob):
    return np.asarray(Image.open(io.BytesIO(blob)))


def first_difference(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n)


def assert_files_equal(got, want, cases):
    assert len(got) == len(want) == len(cases)
    for g, w, case in zip(got, want, cases):
        assert g == w, (case, len(g), len(w), first_difference(g, w))


# ---------------------------------------------------------------------------------------------------------------- 1. the byte oracle
@pytest.mark.parametrize("restart", [1, 3, 8])
def test_mixed_batch_equals_pils_restart_files(backend, restart):
    """Every shape, sampling and quality in ONE call."""
    cases = [(h, w, s, q) for (h, w) in SHAPES for s in SAMPLINGS for q in QUALITIES if np.prod(mcus(h, w, s)) >= restart]
    assert len({c[:2] for c in cases}) >= (8 if restart == 1 else 5) and len({c[2] for c in cases}) == 4
    t = JpegTranscoder(backend.device)
    got = t.transcode([pil_file(*c) for c in cases], restart_blocks=restart)
    assert t.skipped == []
    assert_files_equal(got, [pil_file(*c, blocks=restart) for c in cases], cases)


def test_the_oracle_is_sound():
    """On PIL's files alone: the two files of a case hold the same picture and differ in the DRI segment and the scan only."""
    for case in [(37, 53, 2, 75), (64, 80, None, 100), (17, 33, 1, 10)]:
        plain, cut = pil_file(*case), pil_file(*case, blocks=3)
        assert np.array_equal(pil_pixels(plain), pil_pixels(cut))
        dri = cut.index(b"\xff\xdd\x00\x04\x00\x03")
        assert plain[:dri] == cut[:dri] and plain[dri:dri + 10] == cut[dri + 6:dri + 16]      # (the scan header follows in both)


# ---------------------------------------------------------------------------------------------------------------- 2. restart_rows
@pytest.mark.parametrize("rows", [1, 2])
def test_restart_rows_equals_pils(backend, rows):
    cases = [(h, w, s, 75) for (h, w) in [(37, 53), (64, 80), (31, 15), (40, 9), (17, 33)] for s in SAMPLINGS]
    assert len({mcus(*c[:3])[0] for c in cases}) >= 4      # (intervals of different lengths in one batch)
    t = JpegTranscoder(backend.device)
    got = t.transcode([pil_file(*c) for c in cases], restart_rows=rows)
    assert t.skipped == []
    assert_files_equal(got, [pil_file(*c, rows=rows) for c in cases], cases)


# ---------------------------------------------------------------------------------------------------------------- 3. identity, re-cutting
def test_identity_recutting_and_clamping(backend):
    cases = [(h, w, s, 75) for (h, w) in [(37, 53), (64, 80), (8, 8)] for s in SAMPLINGS]
    t = JpegTranscoder(backend.device)
    plain = [pil_file(*c) for c in cases]
    assert_files_equal(t.transcode(plain, restart_blocks=0), plain, cases)                     # a PIL default file is its own transcoding
    large = [c for c in cases if np.prod(mcus(*c[:3])) >= 5]
    assert len(large) == 8
    cut2 = [pil_file(*c, blocks=2) for c in large]
    assert_files_equal(t.transcode(cut2, restart_blocks=5), [pil_file(*c, blocks=5) for c in large], large)
    assert_files_equal(t.transcode(cut2, restart_blocks=0), [pil_file(*c) for c in large], large)
    # an interval longer than the image is clamped as libjpeg clamps it: one interval, no marker, the DRI segment states K
    small = [c for c in cases if np.prod(mcus(*c[:3])) < 30]
    assert len(small) >= 5
    got = t.transcode([pil_file(*c) for c in small], restart_blocks=30)
    assert_files_equal(got, [pil_file(*c, blocks=30) for c in small], small)
    for g in got:
        assert b"\xff\xdd\x00\x04\x00\x1e" in g and len(parse_jpeg(g).units) == 1
    assert t.skipped == []


# ---------------------------------------------------------------------------------------------------------------- 4. no byte oracle
CUSTOM_TABLES = [[min(255, 3 + 2 * i) for i in range(64)], [min(255, 9 + 3 * i) for i in range(64)]]


@functools.lru_cache(maxsize=None)
def other_sources():
    out = []
    for (h, w) in [(37, 53), (64, 80), (17, 33)]:
        for s in SAMPLINGS:
            out.append(pil_file(h, w, s, 75, optimize=True))
            out.append(pil_file(h, w, s, 75, blocks=2))
            b = io.BytesIO()
            kw = {} if s is None else dict(subsampling=s)
            Image.fromarray(picture(h, w, s)).save(b, "JPEG", qtables=CUSTOM_TABLES[:1 if s is None else 2], **kw)
            out.append(b.getvalue())
    return tuple(out)


def component_tables(blob):
    h = parse_jpeg(blob)
    assert h.supported, h.reason
    return [h.qtables[c[3]].tolist() for c in h.components]


def test_sources_pil_cannot_rewrite_keep_pixels_tables_and_coefficients(backend):
    sources = list(other_sources())
    assert any(parse_jpeg(s).table_key != parse_jpeg(pil_file(37, 53, 2)).table_key for s in sources), "no optimised Huffman tables"
    assert component_tables(sources[2]) != component_tables(sources[0]) and component_tables(sources[5]) != component_tables(sources[3])
    t = JpegTranscoder(backend.device)
    outputs = t.transcode(sources, restart_rows=1)
    assert t.skipped == []
    dec = JpegDecoder(backend.device)
    a = dec.coefficients(sources)
    ca = [a.blocks(i).cpu().numpy() for i in range(len(sources))]
    assert not a.status.cpu().any()
    b = dec.coefficients(outputs)
    assert not b.status.cpu().any()
    for i, (src, out) in enumerate(zip(sources, outputs)):
        assert out != src, i
        h = parse_jpeg(out)
        assert h.restart_interval == h.mcus[0] and len(h.units) == h.mcus[1], i
        assert np.array_equal(pil_pixels(out), pil_pixels(src)), i
        assert component_tables(out) == component_tables(src), i
        assert ca[i].shape[0] > 0 and np.array_equal(b.blocks(i).cpu().numpy(), ca[i]), i


# ---------------------------------------------------------------------------------------------------------------- 5. the layout kernel
GUARD = -23131          # 0xA5A5


def layout_reference(src, rows, dst):
    """Index arithmetic in numpy, from the statement of the two layouts (the header of csrc/jpeg_transcode.hip)."""
    for ncomp, hs, vs, mx, my, so, do, nb in rows:
        lb = 0
        for mcu_y in range(my):
            for mcu_x in range(mx):
                planar = [(mcu_y * vs + j // hs) * (mx * hs) + mcu_x * hs + j % hs for j in range(hs * vs)]
                if ncomp == 3:
                    planar += [mx * my * hs * vs + c * mx * my + mcu_y * mx + mcu_x for c in range(2)]
                for sb in planar:
                    dst[do + lb] = src[so + sb][ZIGZAG]
                    lb += 1
        assert lb == nb


def test_layout_kernel_against_index_arithmetic(backend):
    ints = K.jpeg_transcode_layout()
    assert ints == 8
    geometry = [(1, 1, 1, 5, 3), (3, 1, 1, 5, 3), (3, 2, 1, 5, 3), (3, 2, 2, 5, 3), (3, 2, 2, 1, 1), (1, 1, 1, 1, 1), (3, 2, 1, 1, 2), (3, 1, 1, 7, 5)]
    rows, so, do = [], 3, 0          # (3 source blocks nobody names in front; the images' destinations are in another order below)
    for ncomp, hs, vs, mx, my in geometry:
        nb = mx * my * (1 if ncomp == 1 else hs * vs + 2)
        rows.append([ncomp, hs, vs, mx, my, so, 0, nb])
        so += nb
    for r in sorted(rows, key=lambda r: -r[7]):
        r[6] = do
        do += r[7] + 1               # (one destination block nobody names behind every image)
    n_src, n_dst = so + 2, do
    assert max(r[7] for r in rows) == 105 > 3 * 32 and n_src * 64 < 32767
    # rows that must be refused: past the source, past the destination, a block count that is not the geometry's, bad sampling,
    # a negative offset
    bad = [[3, 2, 2, 5, 3, n_src - 89, 0, 90], [3, 2, 2, 5, 3, 3, n_dst - 89, 90], [3, 2, 2, 5, 3, 3, 0, 89], [3, 1, 2, 5, 3, 3, 0, 90],
           [1, 2, 1, 5, 3, 3, 0, 15], [1, 1, 1, 5, 3, -1, 0, 15], [1, 1, 1, 5, 3, 0, -1, 15], [2, 1, 1, 5, 3, 0, 0, 30], [1, 1, 1, 0, 3, 0, 0, 0]]
    table = rows[:4] + bad[:5] + rows[4:] + bad[5:]
    is_bad = [r in bad for r in table]
    src = (np.arange(n_src * 64, dtype=np.int64) + 1).astype(np.int16).reshape(n_src, 64)      # every value is its own flat index + 1
    want = np.full((n_dst, 64), GUARD, np.int16)
    layout_reference(src, [r for r in table if r not in bad], want)
    assert (want == GUARD).sum() == len(geometry) * 64 and len(np.unique(want)) == (n_src - 5) * 64 + 1

    def run():
        pad = 4                      # guard blocks on either side of the destination
        buf = backend.put(torch.full((n_dst + 2 * pad, 64), GUARD, dtype=torch.int16))
        status = backend.put(torch.full((len(table),), 77, dtype=torch.int32))
        K.jpeg_transcode_blocks(backend.put(torch.from_numpy(src.copy())), backend.put(torch.tensor(table, dtype=torch.int32)), 105,
                                buf[pad:pad + n_dst], status)
        return buf.cpu().numpy(), status.cpu().tolist()
    got, status = run()
    assert status == [4 if b else 0 for b in is_bad]
    assert (got[:4] == GUARD).all() and (got[-4:] == GUARD).all(), "wrote outside the destination"
    assert np.array_equal(got[4:-4], want), np.argwhere(got[4:-4] != want)[:4]
    again, status2 = run()
    assert np.array_equal(again, got) and status2 == status


def test_layout_wrapper_refuses_bad_tensors(emu):
    src, dst = torch.zeros(6, 64, dtype=torch.int16), torch.zeros(8, 64, dtype=torch.int16)
    desc, status = torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for args in [(src.int(), desc, 1, dst, status), (src, desc.long(), 1, dst, status), (src, desc[:, :7].contiguous(), 1, dst, status),
                 (src, desc, 1, dst[:, :32].contiguous(), status), (src, desc, 0, dst, status), (src, desc, 1, dst, status[:1]),
                 (src, desc, 1, src, status), (src, desc, 1, torch.zeros(2 * 64 + 4, dtype=torch.int16)[4:].view(2, 64), status)]:
        with pytest.raises(ValueError, match="jpeg_transcode_blocks"):
            K.jpeg_transcode_blocks(*args)


# ---------------------------------------------------------------------------------------------------------------- 6. files it does not take
def test_files_it_does_not_take_come_back_unchanged(backend, monkeypatch):
    good = [pil_file(37, 53, 2), pil_file(64, 80, None), pil_file(17, 33, 0)]
    b = io.BytesIO()
    Image.fromarray(picture(37, 53, 2)).save(b, "JPEG", progressive=True)
    progressive = b.getvalue()
    whole = pil_file(64, 80, 2, 100)
    begin = parse_jpeg(whole).scan[0]
    truncated = whole[:begin + (len(whole) - begin) // 2]
    b = io.BytesIO()
    Image.fromarray(picture(16, 16, 2)).convert("CMYK").save(b, "JPEG")
    cmyk = b.getvalue()
    victim = pil_file(31, 15, 1)
    batch = [good[0], progressive, good[1], truncated, victim, cmyk, good[2], b"no jpeg at all"]
    # the seam for a coefficient the standard tables cannot code: one is written into the victim's blocks behind the layout kernel
    real = K.jpeg_transcode_blocks

    t = JpegTranscoder(backend.device)

    def poke(src, desc, max_blocks, dst, status):
        real(src, desc, max_blocks, dst, status)
        rows = desc.cpu().numpy()
        j = [i for i in range(rows.shape[0]) if tuple(rows[i, :5]) == (3, 2, 1, 1, 4)]
        assert len(j) == 1
        dst[int(rows[j[0], 6]) + 2, 9] = 1024            # an AC coefficient of 11 bits
    monkeypatch.setattr(K, "jpeg_transcode_blocks", poke)
    got = t.transcode(batch, restart_blocks=2)
    monkeypatch.setattr(K, "jpeg_transcode_blocks", real)
    reasons = dict(t.skipped)
    assert sorted(reasons) == [1, 3, 4, 5, 7]
    assert "progressive" in reasons[1] and reasons[1].startswith("unsupported")
    assert reasons[3].startswith("damaged scan")
    assert reasons[4] == REASON_RANGE
    assert "CMYK" in reasons[5] and "SOI" in reasons[7]
    for i in reasons:
        assert got[i] == batch[i], i
    assert got[0] == pil_file(37, 53, 2, blocks=2) and got[2] == pil_file(64, 80, None, blocks=2) and got[6] == pil_file(17, 33, 0, blocks=2)
    # without the poke the victim is an ordinary file
    assert t.transcode([victim], restart_blocks=2) == [pil_file(31, 15, 1, blocks=2)] and t.skipped == []
    # nothing to transcode at all: the files come back, no launch is needed
    assert t.transcode([progressive, cmyk], restart_rows=1) == [progressive, cmyk] and [i for i, _ in t.skipped] == [0, 1]


def test_chroma_tables_that_differ_are_skipped(backend):
    src = bytearray(pil_file(37, 53, 2))
    # a third quantisation table, one entry away from the second, that Cr names: the output header has one chroma table
    sof = src.index(b"\xff\xc0")
    assert src[sof + 16] == 3 and src[sof + 18] == 1      # component 3 -> table 1
    dqt = src.index(b"\xff\xdb", src.index(b"\xff\xdb") + 2)
    extra = bytearray(src[dqt:dqt + 69])
    extra[4], extra[10] = 2, extra[10] + 1
    src[sof + 18] = 2
    blob = bytes(src[:dqt]) + bytes(extra) + bytes(src[dqt:])
    assert parse_jpeg(blob).supported
    Image.open(io.BytesIO(blob)).load()
    t = JpegTranscoder(backend.device)
    got = t.transcode([blob, pil_file(37, 53, 2)], restart_blocks=3)
    assert got[0] == blob and [i for i, _ in t.skipped] == [0] and "different quantisation tables" in t.skipped[0][1]
    assert got[1] == pil_file(37, 53, 2, blocks=3)


def test_device_side_batch_and_arguments(backend):
    t = JpegTranscoder(backend.device)
    b = io.BytesIO()
    Image.fromarray(picture(37, 53, 2)).save(b, "JPEG", progressive=True)
    whole = pil_file(64, 80, 2, 100)
    truncated = whole[:parse_jpeg(whole).scan[0] + 200]
    files = [pil_file(37, 53, 2), b.getvalue(), truncated, pil_file(64, 80, None)]
    batch = t.transcode(files, restart_rows=1, as_bytes=False)
    assert [i for i, _ in t.skipped] == [1]
    status, lengths, offsets = batch.status.cpu().tolist(), batch.lengths.cpu().tolist(), batch.offsets.cpu().tolist()
    assert status[0] == status[1] == status[3] == 0 and status[2] == 8 and lengths[1] == lengths[2] == 0
    data = batch.data.cpu().numpy().tobytes()
    assert data[offsets[0]:offsets[0] + lengths[0]] == pil_file(37, 53, 2, rows=1)
    assert data[offsets[3]:offsets[3] + lengths[3]] == pil_file(64, 80, None, rows=1)
    for kw in (dict(), dict(restart_blocks=1, restart_rows=1), dict(restart_blocks=-1), dict(restart_rows=65536), dict(restart_blocks=2.0),
               dict(restart_rows=True)):
        with pytest.raises(ValueError, match="restart"):
            t.transcode(files, **kw)
    with pytest.raises(ValueError, match="no files"):
        t.transcode([], restart_rows=1)


# ---------------------------------------------------------------------------------------------------------------- 7. the point of it
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_the_decoder_gets_one_unit_per_interval_and_pils_pixels(backend, sampling):
    src = pil_file(64, 80, sampling)
    assert len(parse_jpeg(src).units) == 1
    out, = JpegTranscoder(backend.device).transcode([src], restart_rows=1)
    h = parse_jpeg(out)
    mx, my = mcus(64, 80, sampling)
    assert h.supported and h.restart_interval == mx and len(h.units) == my > 1
    assert [(u[2], u[3]) for u in h.units] == [(r * mx, mx) for r in range(my)]
    dec = JpegDecoder(backend.device)
    got, = dec.decode([out], "L" if sampling is None else "RGB")
    assert dec.fallbacks == 0 and not dec.status.cpu().any()
    want = pil_pixels(src)
    assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)


# ---------------------------------------------------------------------------------------------------------------- 8. the tool
def _tool():
    spec = importlib.util.spec_from_file_location("transcode_frames_tool", os.path.join(ROOT, "tools", "transcode_frames.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for name in files:
            p = os.path.join(d, name)
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = (f.read(), os.stat(p).st_mtime_ns)
    return out


def test_tool_mirrors_a_tree(backend, tmp_path, capsys):
    from action_detection_amd import _lib
    if backend.is_gpu:
        assert not _lib.emulator_active()
    src = tmp_path / "frames"
    b = io.BytesIO()
    Image.fromarray(picture(37, 53, 2)).save(b, "JPEG", progressive=True)
    files = {os.path.join("video_a", "img_00001.jpg"): pil_file(37, 53, 2), os.path.join("video_a", "img_00002.jpg"): pil_file(37, 53, 2, 10),
             os.path.join("video_a", "img_00003.jpg"): b.getvalue(), os.path.join("video_b", "flow", "flow_x_00001.JPEG"): pil_file(64, 80, None),
             os.path.join("video_b", "notes.txt"): b"not a picture", "top.jpg": pil_file(17, 33, 0)}
    for rel, data in files.items():
        os.makedirs(os.path.dirname(str(src / rel)), exist_ok=True)
        with open(str(src / rel), "wb") as f:
            f.write(data)
        os.utime(str(src / rel), ns=(10 ** 18, 10 ** 18))
    before = _tree(str(src))
    tool = _tool()
    out = tmp_path / "out"
    assert tool.main([str(src), str(out), "--verify", "--batch", "2"]) == 0
    summary = capsys.readouterr().out.strip().splitlines()[-1]
    assert summary.startswith("4 files transcoded, 1 copied unchanged") and "progressive" in summary and "verified" in summary
    assert _tree(str(src)) == before, "the source tree changed"
    got = {rel: data for rel, (data, _) in _tree(str(out)).items()}
    assert sorted(got) == sorted(files)
    assert got[os.path.join("video_a", "img_00003.jpg")] == files[os.path.join("video_a", "img_00003.jpg")]
    assert got[os.path.join("video_b", "notes.txt")] == b"not a picture"
    assert got[os.path.join("video_a", "img_00001.jpg")] == pil_file(37, 53, 2, rows=1)
    assert got[os.path.join("video_a", "img_00002.jpg")] == pil_file(37, 53, 2, 10, rows=1)
    assert got[os.path.join("video_b", "flow", "flow_x_00001.JPEG")] == pil_file(64, 80, None, rows=1)
    assert got["top.jpg"] == pil_file(17, 33, 0, rows=1)
    out2 = tmp_path / "out2"
    assert tool.main([str(src), str(out2), "--restart-blocks", "3", "--quiet"]) == 0
    with open(str(out2 / "top.jpg"), "rb") as f:
        assert f.read() == pil_file(17, 33, 0, blocks=3)
    for inside in (str(src), str(src / "video_a" / "rst"), str(src / "new")):
        with pytest.raises(SystemExit):
            tool.main([str(src), inside])
    with pytest.raises(SystemExit):
        tool.main([str(src), str(tmp_path / "y"), "--restart-rows", "1", "--restart-blocks", "2"])
    assert _tree(str(src)) == before and not os.path.exists(str(src / "new"))
