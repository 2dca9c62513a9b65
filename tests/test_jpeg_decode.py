"""host_models.jpeg_decode_rgb8 - the definition of float_jpg_decode - against Pillow (libjpeg-turbo): bitwise.  The same files
through float_jpg_decode_host, the kernels' rule header compiled for the host; the plan's refusals; damaged scans; the AVI reader."""
import functools
import io
import itertools

import numpy as np
import pytest
from PIL import Image

from tests.util import load_pkg

pkg = load_pkg()
hm, J = pkg.host_models, pkg.jpeg
SUBS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
SIZES = [(1, 1), (8, 8), (17, 13), (33, 47), (48, 64)]  # below one MCU, one block, partial MCUs on both axes, several MCU rows


@functools.lru_cache(None)
def image(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)], -1)
    return np.clip(base + np.random.RandomState(3).normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def pil_file(h, w, sub, quality=90, restart=None, **kw):
    """restart: None, "row" (one MCU row) or "mcu" (one MCU)."""
    img = image(h, w)
    if sub != "grey":
        kw["subsampling"] = SUBS[sub]
    if restart:
        kw["restart_marker_rows" if restart == "row" else "restart_marker_blocks"] = 1
    if quality is not None:  # with a quality Pillow scales qtables= and clamps them to 8 bits
        kw["quality"] = quality
    b = io.BytesIO()
    Image.fromarray(img[..., 1] if sub == "grey" else img).save(b, "JPEG", **kw)
    return b.getvalue()


def pillow(f):
    return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def case_files(sub, size):
    """The files of one (subsampling, size): quality x restart, plus the file's own Huffman and quantiser tables, 8- and 16-bit."""
    files = [pil_file(*size, sub, q, r) for q, r in itertools.product((25, 90), (None, "row", "mcu"))]
    wide = pil_file(*size, sub, None, "row", qtables=[[300] + [2] * 63, [3] * 64])  # an entry above 255: libjpeg writes Pq = 1 and SOF1
    assert wide[wide.index(b"\xff\xdb") + 4] >> 4 == 1
    return files + [pil_file(*size, sub, 90, "row", optimize=True), pil_file(*size, sub, 25, None, qtables=[list(range(1, 65)), [3] * 64]),
                    wide.replace(b"\xff\xc1", b"\xff\xc0", 1)]  # the same frame under SOF0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("sub", ["4:4:4", "4:2:2", "4:2:0", "grey"])
def test_definition_and_host_rule_are_pillow(sub, size):
    files = case_files(sub, size)
    got, status = J.decode_jpeg_host(files)  # one call: table sets and restart intervals differ from frame to frame
    assert status.tolist() == [0] * len(files)
    for i, f in enumerate(files):
        want = pillow(f)
        rgb, st = hm.jpeg_decode_rgb8(f, status=True)
        assert st == 0 and np.array_equal(rgb, want), (i, np.abs(rgb.astype(int) - want).max())
        assert np.array_equal(got[i].numpy(), want), i


@pytest.mark.parametrize("restart", [0, None, 1])
def test_own_encoder_round_trip_is_pillow(restart):
    for f in hm.jpeg_encode_rgb8(np.stack([image(48, 64), image(48, 64)[::-1]]), 90, restart):
        assert np.array_equal(hm.jpeg_decode_rgb8(f), pillow(f)) and np.array_equal(J.decode_jpeg_host([f])[0][0].numpy(), pillow(f))


def _save(mode, **kw):
    b = io.BytesIO()
    Image.fromarray(image(16, 16)).convert(mode).save(b, "JPEG", **kw)
    return b.getvalue()


def _luma_4x1():
    f = bytearray(pil_file(16, 16, "4:2:0"))
    f[f.index(b"\xff\xc0") + 11] = 0x41  # the first component's sampling factors in SOF0
    return bytes(f)


def _oversubscribed_dht():
    f = bytearray(pil_file(16, 16, "4:2:0"))
    at = f.index(b"\xff\xc4") + 5  # BITS of the first table, DC 0: (0, 1, 5, 1, ...)
    f[at], f[at + 2] = 3, 2  # three codes of length 1, still 12 values
    return bytes(f)


REFUSED = {"oversubscribed dht": (_oversubscribed_dht(), "over-subscribed"), "progressive": (_save("RGB", progressive=True), "progressive"), "cmyk": (_save("CMYK"), "4 components"),
           "sampling": (_luma_4x1(), "sampling factors"), "truncated header": (pil_file(16, 16, "4:2:0")[:150], "truncated header"),
           "no huffman table": (pil_file(16, 16, "4:2:0").replace(b"\xff\xc4", b"\xff\xec"), "missing Huffman table")}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_name_the_reason(name):
    file, word = REFUSED[name]
    with pytest.raises(ValueError, match=word):
        hm.jpeg_decode_rgb8(file)
    with pytest.raises(ValueError, match="frame 1: .*" + word):
        J.JpegPlan(*J.host_files([pil_file(16, 16, "4:2:0"), file]))


def test_mixed_sizes_in_one_call_are_refused():
    with pytest.raises(ValueError, match="frame 1 is 8 x 8"):
        J.JpegPlan(*J.host_files([pil_file(16, 16, "4:2:0"), pil_file(8, 8, "4:2:0")]))


@pytest.mark.parametrize("restart", [None, "row"])
def test_truncated_scan_zero_fill_and_status(restart):
    """A scan cut inside an interval: bits past the end are zero, later intervals have no segment and decode to all-zero
    coefficients (mid grey), the status word says so - and the host rule gives the definition's pixels."""
    f = pil_file(48, 64, "4:2:0", 90, restart)
    hdr = hm.jpeg_parse_header(f)
    cut = f[:hdr["scan_start"] + (hdr["scan_end"] - hdr["scan_start"]) // 2]  # inside the second of three MCU rows
    rgb, st = hm.jpeg_decode_rgb8(cut, status=True)
    assert st == (hm.JPEG_DEC_PAST_END | (hm.JPEG_DEC_RESTARTS if restart else 0))
    if restart:
        # the last MCU row is missing, the first is whole; rows 15 and 32 take chroma from the damaged row between them
        assert (rgb[33:] == 128).all() and np.array_equal(rgb[:15], pillow(f)[:15])
    got, status = J.decode_jpeg_host([f, cut])
    assert status.tolist() == [0, st] and np.array_equal(got[1].numpy(), rgb)
    flipped = bytearray(f)
    flipped[hdr["scan_start"] + 40] ^= 0x10  # a wrong bit in the first interval
    rgb, st = hm.jpeg_decode_rgb8(bytes(flipped), status=True)
    got, status = J.decode_jpeg_host([bytes(flipped)])
    assert int(status[0]) == st and np.array_equal(got[0].numpy(), rgb)


def test_avi_reader_returns_what_the_writer_was_given():
    files = hm.jpeg_encode_rgb8(np.stack([image(48, 64)] * 3), 90) + [pil_file(48, 64, "4:2:0")]
    audio = np.linspace(-1, 1, 1000)
    buf = io.BytesIO()
    with hm.AviMjpegWriter(buf, 64, 48, 29.97, audio_rate=16000) as w:
        w.write(files[:2])
        w.write_audio(audio[:600])
        w.write(files[2:])
        w.write_audio(audio[600:])
    for strip_index in (False, True):
        raw = buf.getvalue()
        raw = raw[:raw.rindex(b"idx1")] if strip_index else raw  # without idx1 the `movi` list is walked
        with hm.AviMjpegReader(io.BytesIO(raw)) as rd:
            assert (len(rd), rd.width, rd.height, rd.fps, rd.audio_rate, rd.audio_channels) == (4, 64, 48, hm.y4m_rate(29.97), 16000, 1)
            assert [bytes(f) for f in rd.read()] == files and [bytes(f) for c in rd.chunks(3) for f in c] == files
            assert rd.audio_pcm.tobytes() == hm.pcm16(audio)
    bare = files[3][:files[3].index(b"\xff\xc4")] + files[3][files[3].index(b"\xff\xda"):]  # Motion-JPEG style: no DHT
    buf = io.BytesIO()
    with hm.AviMjpegWriter(buf, 64, 48, 25) as w:
        w.write([bare])
    with pytest.raises(ValueError, match="missing Huffman table"):
        hm.jpeg_decode_rgb8(bare)
    assert np.array_equal(hm.jpeg_decode_rgb8(next(iter(hm.AviMjpegReader(io.BytesIO(buf.getvalue()))))), pillow(files[3]))
