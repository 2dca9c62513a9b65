"""The PNG definition (host_models.png_encode_rgb8 and what stands beside it), the APNG writer and the argument checks of
float_png_encode: no GPU.  Pillow and zlib are the references, and every comparison is exact."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from tests.jpeg_util import fixtures
from tests.util import load_pkg

pkg = load_pkg()
HM = pkg.host_models
FIX = fixtures()
SIG = b"\x89PNG\r\n\x1a\n"


def chunks(data):
    """[(type, body)] of a PNG file; every chunk's CRC is checked against zlib.crc32."""
    data = bytes(data)
    assert data[:8] == SIG
    out, i = [], 8
    while i < len(data):
        n, cc = struct.unpack(">I", data[i:i + 4])[0], data[i + 4:i + 8]
        body = data[i + 8:i + 8 + n]
        assert struct.unpack(">I", data[i + 8 + n:i + 12 + n])[0] == zlib.crc32(cc + body), cc
        out.append((cc, body))
        i += 12 + n
    assert i == len(data) and out[-1] == (b"IEND", b"")
    return out


def decoded(data):
    return np.array(Image.open(io.BytesIO(bytes(data))).convert("RGB"))


def check_file(data, img, band):
    h, w, _ = img.shape
    ch = chunks(data)
    assert [c for c, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert ch[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    z = ch[1][1]
    rows = HM.png_filter_rows(img)
    assert z[:2] == b"\x78\x01" and z[-9:-4] == b"\x01\x00\x00\xff\xff" and struct.unpack(">I", z[-4:])[0] == zlib.adler32(rows)
    assert zlib.decompress(z) == rows
    assert HM.png_idat(data) == (41, len(z)) and bytes(data[41:41 + len(z)]) == z
    assert np.array_equal(decoded(data), img)


@pytest.mark.parametrize("name", sorted(FIX))
def test_fixtures_decode_to_the_frame(name):
    img = FIX[name]
    for band in (1, 3, 8, img.shape[0]):
        (f,) = HM.png_encode_rgb8(img, band)
        check_file(f, img, band)
    assert HM.png_encode_rgb8(img) == HM.png_encode_rgb8(img, HM.png_default_band(*img.shape[:2])) == HM.png_encode_rgb8(img, 0)


def test_batch_and_torch_input():
    import torch
    batch = np.stack([FIX["noise"], FIX["extremes"], FIX["smooth_noise"]])
    files = HM.png_encode_rgb8(torch.from_numpy(batch), 3)
    assert files == [HM.png_encode_rgb8(b, 3)[0] for b in batch]


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1)])
def test_tiny_frames(shape):
    img = np.random.RandomState(3).randint(0, 256, shape + (3,)).astype(np.uint8)
    (f,) = HM.png_encode_rgb8(img)
    check_file(f, img, None)


def _filter_of(img, y):
    w = img.shape[1]
    return HM.png_filter_rows(img)[y * (1 + 3 * w)]


def test_the_filter_of_hand_made_rows():
    rng = np.random.RandomState(5)
    w = 16
    # None: a first row of alternating 255 and 0 pixels costs 1 per 255 unfiltered and 1 per byte under Sub; on a first row Up
    # equals None and Paeth equals Sub, and both ties go to the smaller type
    row = np.zeros((1, w, 3), np.uint8)
    row[0, ::2] = 255
    assert _filter_of(row, 0) == 0
    # a constant row of 7: None costs 7 per byte, Sub only the first pixel's 21: Sub; Paeth ties with Sub on a first row, Sub wins
    assert _filter_of(np.full((1, w, 3), 7, np.uint8), 0) == 1
    # Up: a noise row repeated
    noise = rng.randint(0, 256, (1, w, 3)).astype(np.uint8)
    assert _filter_of(np.concatenate([noise, noise]), 1) == 2
    # Average: the row is floor((left + up) / 2) exactly, built pixel by pixel
    up = rng.randint(0, 256, (w, 3)).astype(np.int64)
    cur = np.zeros((w, 3), np.int64)
    for x in range(w):
        cur[x] = ((cur[x - 1] if x else 0) + up[x]) >> 1
    img = np.stack([up, cur]).astype(np.uint8)
    assert _filter_of(img, 1) == 3
    # Paeth: behind a first pixel 60 above its upper neighbour, the row is the Paeth predictor of (left, up, upper left) exactly,
    # built pixel by pixel over a noise row in 60 ... 190: now left, now up is the nearest, so Sub, Up and Average all pay
    up = rng.randint(60, 191, (w, 3)).astype(np.int64)
    cur = np.zeros((w, 3), np.int64)
    cur[0] = up[0] + 60
    for x in range(1, w):
        a, b, c = cur[x - 1], up[x], up[x - 1]
        q = a + b - c
        pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
        cur[x] = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    assert cur.min() >= 0 and cur.max() <= 255 and _filter_of(np.stack([up, cur]).astype(np.uint8), 1) == 4
    # ties go to the smallest type: a zero frame costs 0 under every filter
    assert HM.png_filter_rows(np.zeros((2, w, 3), np.uint8)) == bytes(2 * (1 + 3 * w))


def test_code_lengths():
    tabs = HM.png_code_lengths()
    assert len(tabs) == 8 and all(len(t) == 257 for t in tabs)
    for t in tabs:
        assert sum(1 << (15 - n) for n in t) == 1 << 15 and 1 <= min(t) and max(t) <= 15  # the Kraft sum is exactly 1
    assert max(tabs[7]) == 9 and [i for i, n in enumerate(tabs[7]) if n == 9] == [128, 256] and set(tabs[7]) == {8, 9}
    for t in tabs[:7]:  # short codes near 0 and 255, longer towards 128
        assert t[0] == min(t) and t[0] < t[128] and t[255] < t[128] and t[1] <= t[64] and t[255] <= t[192]


def test_crc32_combine():
    rng = np.random.RandomState(9)
    a = rng.randint(0, 256, 1000).astype(np.uint8).tobytes()
    for n in (0, 1, 7, 65537):
        b = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        assert HM.crc32_combine(zlib.crc32(a), zlib.crc32(b), n) == zlib.crc32(a + b)
    assert HM.crc32_combine(zlib.crc32(b""), zlib.crc32(a), len(a)) == zlib.crc32(a)


def smooth_noise_512():
    """The size test's frame: 127.5 + 100 sin(x / 40) cos(y / 50), (x + y) / 4, 127.5 + 110 sin((x + y) / 60), rounded, plus
    RandomState(0).randint(-3, 4), clipped to 0 ... 255."""
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float64)
    img = np.stack([127.5 + 100 * np.sin(xx / 40) * np.cos(yy / 50), (xx + yy) / 4.0, 127.5 + 110 * np.sin((xx + yy) / 60)], -1)
    return np.clip(np.rint(img) + np.random.RandomState(0).randint(-3, 4, img.shape), 0, 255).astype(np.uint8)


def test_size_against_pillow_level_1():
    img = smooth_noise_512()
    (f,) = HM.png_encode_rgb8(img, 8)
    ref = io.BytesIO()
    Image.fromarray(img).save(ref, "PNG", compress_level=1)
    print("this design %d bytes, Pillow level 1 %d bytes: %.3f" % (len(f), len(ref.getvalue()), len(f) / len(ref.getvalue())))
    assert len(f) <= len(ref.getvalue())
    assert np.array_equal(decoded(f), img)


def test_noise_stays_inside_the_slot():
    img = FIX["noise"]
    h, w, _ = img.shape
    rows = HM.png_filter_rows(img)
    stride = 1 + 3 * w
    for band in (1, 3, 8, h):
        for r in range(0, h, band):
            n = min(band, h - r)
            piece = HM.png_band_bytes(rows[r * stride:(r + n) * stride])
            assert len(piece) <= HM.png_slot_bytes(n, w) and len(piece) * 8 <= HM.PNG_HEADER_BITS + 9 * n * stride + 15 + 3 + 7 + 32
    (f,), chosen = HM.png_encode_rgb8(img, 8, stats=True)
    assert set(chosen) == {7}  # noise takes the flat table


def test_band_rule():
    assert HM.png_default_band(512, 512) == 8 and HM.png_default_band(3, 512) == 3 and HM.png_default_band(64, 16384) == 1
    assert HM.png_default_band(16384, 16384) == 1 and HM.png_check_band(16384, 1, 16384) == 16384
    for h, w, band in ((8, 8, 9), (8, 8, -1), (64, 16384, 2), (0, 8, 1), (8, 16385, 1)):
        with pytest.raises(ValueError):
            HM.png_check_band(h, w, band)
    with pytest.raises(ValueError):
        HM.png_encode_rgb8(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        HM.png_encode_rgb8(np.zeros((4, 4, 3), np.float32))


# --------------------------------------------------------------------------------------------------------------------------- APNG
def _clip():
    frames = np.stack([FIX["smooth"], FIX["noise"], FIX["patch"], FIX["extremes"]])
    files = HM.png_encode_rgb8(frames)
    return frames, files, [zlib.crc32(f[41:-16]) for f in files]


@pytest.mark.parametrize("fps, duration", [(25, 40.0), (12.5, 80.0), (50, 20.0)])
def test_apng_writer(fps, duration, tmp_path):
    frames, files, crcs = _clip()
    sink = io.BytesIO()
    sink.write(b"junk")  # the writer starts where the file object stands
    with HM.ApngWriter(sink, 64, 64, fps) as w:
        assert w.write(files[:1], crcs[:1]) == 1
        assert w.write(files[1:], np.array(crcs[1:])) == 4
    data = sink.getvalue()[4:]
    ch = chunks(data)  # every CRC in the file is right, the combined ones included
    assert [c for c, _ in ch] == [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * 3 + [b"IEND"]
    assert ch[1][1] == struct.pack(">II", 4, 0)
    seq = [struct.unpack(">I", b[:4])[0] for c, b in ch if c in (b"fcTL", b"fdAT")]
    assert seq == list(range(7))
    im = Image.open(io.BytesIO(data))
    assert im.n_frames == 4 and im.is_animated
    for t in range(4):
        im.seek(t)
        assert np.array_equal(np.array(im.convert("RGB")), frames[t]) and im.info["duration"] == duration
    path = str(tmp_path / "clip.png")
    with HM.ApngWriter(path, 64, 64, fps) as w:
        w.write(files, crcs)
    assert open(path, "rb").read() == data


def test_apng_writer_refusals(tmp_path):
    frames, files, crcs = _clip()
    w = HM.ApngWriter(io.BytesIO(), 64, 64, 25)
    with pytest.raises(ValueError, match="no frame"):  # an APNG holds at least one frame
        w.close()
    w.close()  # idempotent
    with pytest.raises(ValueError, match="after close"):
        w.write(files, crcs)
    with pytest.raises(ValueError, match="crcs"):
        HM.ApngWriter(io.BytesIO(), 64, 64, 25).write(files)
    with pytest.raises(ValueError, match="32 x 64"):
        HM.ApngWriter(io.BytesIO(), 32, 64, 25).write(files, crcs)

    class Pipe(io.RawIOBase):
        def writable(self):
            return True

        def write(self, b):
            return len(b)

    with pytest.raises(ValueError, match="seekable"):
        HM.ApngWriter(Pipe(), 64, 64, 25)


# ------------------------------------------------------------------------------------------------- the native library, no GPU
def test_native_tables_are_the_definitions():
    L = pkg.native.lib()
    assert L.float_hip_abi_version() == 6
    for name in ("float_png_work_bytes", "float_png_encode", "float_png_tables"):
        assert hasattr(L, name) and name in pkg.native.EXPORTS
    buf = (C.c_int32 * (8 * 257))()
    assert L.float_png_tables(buf) == 0
    assert tuple(tuple(buf[k * 257:(k + 1) * 257]) for k in range(8)) == HM.png_code_lengths()
    assert L.float_png_tables(None) == 1 and b"float_png_tables" in L.float_last_error()


def test_native_work_bytes_and_invalid_arguments():
    L = pkg.native.lib()
    need = L.float_png_work_bytes(3, 64, 48, 8)
    items = 3 * 8
    assert need == ((items * 24 + 15) & ~15) + 256 + items * HM.png_slot_bytes(8, 48)
    assert L.float_png_work_bytes(3, 64, 48, 0) == need  # 0: the default band, 8 rows here
    assert L.float_png_work_bytes(40, 64, 48, 8) == L.float_png_work_bytes(16, 64, 48, 8)  # groups of 16 share it
    for bad in ((0, 64, 48, 8), (1, 0, 48, 8), (1, 64, 16385, 1), (1, 64, 48, 65), (1, 64, 16384, 2), (1, 64, 48, -1)):
        assert L.float_png_work_bytes(*bad) == 0, bad
    # every refusal comes before any HIP call: the pointers are never used (no GPU here), only looked at
    mem = (C.c_uint8 * 64)()
    base = (C.addressof(mem) + 15) & ~15
    p = C.c_void_p(base)

    def call(n=1, h=64, w=48, band=8, x=p, out=p, off=p, crcs=None, work=p, wb=need):
        return L.float_png_encode(x, n, h, w, band, out, 64, off, crcs, work, wb, None), L.float_last_error()

    for kw, word in ((dict(x=None), b"null"), (dict(out=None), b"null"), (dict(off=None), b"null"), (dict(work=None), b"null"),
                     (dict(n=0), b"n_frames"), (dict(h=0), b"sides h x w"), (dict(w=16385), b"sides h x w"), (dict(band=65), b"band"),
                     (dict(band=-1), b"band"), (dict(w=16384, band=2), b"band"), (dict(wb=L.float_png_work_bytes(1, 64, 48, 8) - 1), b"work_bytes"),
                     (dict(off=C.c_void_p(base + 4)), b"offsets"), (dict(work=C.c_void_p(base + 8)), b"work"),
                     (dict(crcs=C.c_void_p(base + 2)), b"crcs")):
        rc, msg = call(**kw)
        assert rc == 1 and word in msg and b"float_png_encode" in msg, (kw, msg)
