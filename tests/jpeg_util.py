"""Helpers shared by the JPEG / AVI tests: the seeded fixtures, a JPEG segment parser and a RIFF walker."""
import struct

import numpy as np


def fixtures():
    """{name: (H, W, 3) uint8}: the frames the JPEG definition and the device encoder are tested on."""
    rng = np.random.RandomState(1234)
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    smooth = np.stack([127.5 + 100 * np.sin(xx / 9.0) * np.cos(yy / 13.0), xx * 255.0 / 63.0, 127.5 + 110 * np.sin((xx + yy) / 7.0)], -1)
    noise = lambda *shape: rng.randint(0, 256, shape).astype(np.uint8)  # noqa: E731
    out = {"smooth": np.rint(smooth).astype(np.uint8)}
    out["smooth_noise"] = np.clip(np.rint(smooth) + rng.randint(-6, 7, smooth.shape), 0, 255).astype(np.uint8)
    out["noise"] = noise(64, 64, 3)
    out["noise_32x48"] = noise(32, 48, 3)
    patch = out["smooth"].copy()
    patch[16:48, 16:48] = noise(32, 32, 3)
    out["patch"] = patch
    out["const200"] = np.full((16, 16, 3), 200, np.uint8)
    out["const255"] = np.full((16, 16, 3), 255, np.uint8)
    ext = np.zeros((64, 64, 3), np.uint8)
    yi, xi = np.mgrid[0:64, 0:64]
    ext[:, :32] = ((((yi // 8) + (xi // 8)) % 2) * 255)[:, :32, None]  # 8 x 8 blocks alternating 0 / 255
    ext[:, 32:] = (((yi + xi) % 2) * 255)[:, 32:, None]                # a one-pixel checkerboard
    out["extremes"] = ext
    return out


def restarts(w):
    """The restart intervals of the CPU tests for a frame w wide: none, 1, 3, 5 MCUs and one MCU row."""
    return (0, 1, 3, 5, w // 16)


def jpeg_segments(data):
    """[(marker, payload)] of the segments in front of the scan data of a JPEG file (SOI excluded, SOS included)."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        out.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return out


def jpeg_tables_of(data):
    """({table id: 64 zigzag-order steps}, {class << 4 | id: (BITS, HUFFVAL)}) parsed from a file's DQT and DHT segments (one or
    several tables per segment)."""
    dqt, dht = {}, {}
    for m, p in jpeg_segments(data):
        if m == 0xDB:
            while p:
                assert p[0] >> 4 == 0  # 8-bit
                dqt[p[0] & 15] = tuple(p[1:65])
                p = p[65:]
        elif m == 0xC4:
            while p:
                bits = tuple(p[1:17])
                dht[p[0]] = (bits, bytes(p[17:17 + sum(bits)]))
                p = p[17 + sum(bits):]
    return dqt, dht


def riff_walk(data):
    """Walk a RIFF file: returns (form type, [(path, fourcc, offset of the payload, size)]) for every chunk, depth first, lists
    included (as `LIST:xxxx`); asserts that every chunk starts on an even offset, lies inside its parent, and that the RIFF size
    is the file's."""
    data = bytes(data)
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    chunks = []

    def walk(lo, hi, path):
        i = lo
        while i < hi:
            assert i % 2 == 0 and i + 8 <= hi, (path, i)
            cc, n = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])[0]
            assert i + 8 + n <= hi, (path, cc, n)
            if cc == b"LIST":
                kind = data[i + 8:i + 12].decode()
                chunks.append((path, "LIST:" + kind, i + 8, n))
                walk(i + 12, i + 8 + n, path + "/" + kind)
            else:
                chunks.append((path, cc.decode(), i + 8, n))
            i += 8 + n + (n & 1)
        assert i == hi or i == hi + 1, (path, i, hi)

    walk(12, len(data), "")
    return data[8:12].decode(), chunks


def avi_parts(data):
    """What the tests read of an AVI file: dict(avih, strh [per stream], strf [per stream], video [payloads of the 00dc chunks],
    audio [payloads of the 01wb chunks], idx [(fourcc, flags, offset, size)], movi_at [offset of the `movi` fourcc])."""
    data = bytes(data)
    form, chunks = riff_walk(data)
    assert form == "AVI "
    out = dict(strh=[], strf=[], video=[], audio=[], idx=[])
    for path, cc, at, n in chunks:
        body = data[at:at + n]
        if cc == "avih":
            out["avih"] = struct.unpack("<14I", body)
        elif cc == "strh":
            out["strh"].append(struct.unpack("<4s4sIHHIIIIIIII4h", body))
        elif cc == "strf":
            out["strf"].append(body)
        elif cc == "LIST:movi":
            out["movi_at"] = at
        elif cc == "00dc" and path == "/movi":
            out["video"].append(body)
        elif cc == "01wb" and path == "/movi":
            out["audio"].append(body)
        elif cc == "idx1":
            out["idx"] = [struct.unpack("<4sIII", body[i:i + 16]) for i in range(0, n, 16)]
    return out
