"""host_models.AviMjpegWriter on the CPU: a RIFF walker written here (tests/jpeg_util.py) checks the container byte for byte."""
import fractions
import io
import struct

import numpy as np
import pytest

from tests.jpeg_util import avi_parts, fixtures, riff_walk
from tests.util import load_pkg

pkg = load_pkg()
HM = pkg.host_models
FIX = fixtures()


def _frames():
    """Seven 64 x 64 JPEG files of different (odd and even) lengths."""
    names = ("smooth", "noise", "extremes", "patch", "smooth_noise", "noise", "smooth")
    out = [HM.jpeg_encode_rgb8(FIX[n], q)[0] for n, q in zip(names, (90, 90, 100, 50, 90, 100, 50))]
    assert len({len(f) % 2 for f in out}) == 2  # word alignment is exercised
    return out


def _samples(n, seed=3):
    return np.random.RandomState(seed).uniform(-1.1, 1.1, n).astype(np.float32)  # beyond [-1, 1]: clipped


def test_layout_with_audio_in_several_blocks(tmp_path):
    frames, pcm = _frames(), _samples(4481)
    path = str(tmp_path / "clip.avi")
    with HM.AviMjpegWriter(path, 64, 64, 25, audio_rate=16000) as w:
        assert w.write(frames[:3]) == 3
        assert w.write_audio(pcm[:1921]) == 1921
        assert w.write(iter(memoryview(f) for f in frames[3:])) == 7
        assert w.write_audio(pcm[1921:]) == 4481
    data = open(path, "rb").read()
    form, chunks = riff_walk(data)  # every chunk size, word alignment, the RIFF size
    assert form == "AVI " and [c[1] for c in chunks if c[0] == ""] == ["LIST:hdrl", "LIST:movi", "idx1"]
    p = avi_parts(data)
    assert p["video"] == frames and b"".join(p["audio"]) == HM.pcm16(pcm) and [len(a) for a in p["audio"]] == [3842, 5120]
    usec, _, _, flags, total, _, streams, sugg, width, height = p["avih"][:10]
    assert (usec, flags & 0x10, total, streams, width, height) == (40000, 0x10, 7, 2, 64, 64) and sugg == max(map(len, frames))
    v, a = p["strh"]
    assert v[:2] == (b"vids", b"MJPG") and (v[6], v[7], v[9]) == (1, 25, 7)          # dwScale, dwRate, dwLength
    assert a[0] == b"auds" and (a[6], a[7], a[9], a[12]) == (2, 32000, 4481, 2)    # block align, bytes / s, samples, sample size
    bi = struct.unpack("<IiiHH4sI", p["strf"][0][:24])
    assert bi == (40, 64, 64, 1, 24, b"MJPG", 64 * 64 * 3)
    assert struct.unpack("<HHIIHH", p["strf"][1]) == (1, 1, 16000, 32000, 2, 16)
    # idx1: every entry points at its chunk, counted from the `movi` fourcc
    assert [e[0] for e in p["idx"]] == [b"00dc"] * 3 + [b"01wb"] + [b"00dc"] * 4 + [b"01wb"]
    vi = 0
    for cc, fl, off, size in p["idx"]:
        at = p["movi_at"] + off
        assert data[at:at + 4] == cc and struct.unpack("<I", data[at + 4:at + 8])[0] == size and fl == 0x10
        if cc == b"00dc":
            assert data[at + 8:at + 8 + size] == frames[vi]
            vi += 1
    assert vi == 7


def test_pillow_decodes_the_frames_of_the_file():
    Image = pytest.importorskip("PIL.Image")
    f = io.BytesIO()
    w = HM.AviMjpegWriter(f, 64, 64, 29.97)
    w.write(_frames())
    w.close()
    assert not f.closed  # a file object given in is left open
    p = avi_parts(f.getvalue())
    assert len(p["strh"]) == 1 and p["avih"][6] == 1 and p["audio"] == []
    assert (p["strh"][0][6], p["strh"][0][7]) == (1001, 30000) and HM.y4m_rate(29.97) == fractions.Fraction(30000, 1001)
    for payload in p["video"]:
        im = Image.open(io.BytesIO(payload))
        im.load()
        assert im.size == (64, 64)


def test_pcm16():
    x = np.array([0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.25], np.float32)
    assert np.frombuffer(HM.pcm16(x), "<i2").tolist() == [0, 32767, -32767, 32767, -32767, 16384, -8192]


def test_write_after_close_and_unseekable_sink(tmp_path):
    w = HM.AviMjpegWriter(str(tmp_path / "a.avi"), 64, 64, 25, audio_rate=16000)
    w.close()
    w.close()  # idempotent
    with pytest.raises(ValueError, match="after close"):
        w.write(_frames()[:1])
    with pytest.raises(ValueError, match="after close"):
        w.write_audio(_samples(10))

    class Pipe(io.RawIOBase):
        def writable(self):
            return True

        def seekable(self):
            return False

        def write(self, b):
            return len(b)

    with pytest.raises(ValueError, match="seekable"):
        HM.AviMjpegWriter(Pipe(), 64, 64, 25)
    with pytest.raises(ValueError, match="audio_rate"):
        HM.AviMjpegWriter(io.BytesIO(), 64, 64, 25).write_audio(_samples(4))


def test_size_limit(monkeypatch):
    frames = _frames()
    assert HM.AviMjpegWriter.LIMIT == 2**31 - 2**20
    monkeypatch.setattr(HM.AviMjpegWriter, "LIMIT", 9000)
    f = io.BytesIO()
    w = HM.AviMjpegWriter(f, 64, 64, 25)
    n = 0
    with pytest.raises(ValueError, match="would pass"):
        for fr in frames * 4:
            w.write([fr])
            n += 1
    assert 0 < n < len(frames) * 4
    w.close()  # what was written is a complete file below the limit
    data = f.getvalue()
    assert len(data) <= 9000 and avi_parts(data)["video"] == (frames * 4)[:n]
