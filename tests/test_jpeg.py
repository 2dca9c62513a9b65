"""The JPEG definition (host_models.jpeg_tables / jpeg_header / jpeg_encode_rgb8) on the CPU: its streams are valid baseline JPEG
(Pillow decodes every one), the restart interval does not change a decoded pixel, and quality, size and tables sit where
Pillow's own encoder (libjpeg) puts them.  tests/golden/jpeg_def.npz pins the bytes where Pillow is absent."""
import io
import math
import os

import numpy as np
import pytest
import torch

from tests.jpeg_util import fixtures, jpeg_tables_of, restarts
from tests.util import GOLDEN, load_pkg

pkg = load_pkg()
HM = pkg.host_models
FIX = fixtures()
QUALITIES = (50, 90, 100)
_cache = {}


def encoded(name, q, r):
    """(file, stats) of the definition for one case, computed once."""
    key = (name, q, r)
    if key not in _cache:
        files, st = HM.jpeg_encode_rgb8(FIX[name], q, r, stats=True)
        assert len(files) == 1
        _cache[key] = (files[0], st)
    return _cache[key]


def psnr(a, b):
    mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
    return math.inf if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def pil_decode(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(bytes(data)))
    im.load()
    return im


def pil_encode(img, q):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=2, optimize=False)
    return b.getvalue()


@pytest.mark.parametrize("name", sorted(FIX))
def test_every_stream_opens_and_restart_does_not_change_a_pixel(name):
    pytest.importorskip("PIL")
    img = FIX[name]
    for q in QUALITIES:
        first = None
        for r in restarts(img.shape[1]):
            im = pil_decode(encoded(name, q, r)[0])
            assert im.size == (img.shape[1], img.shape[0]) and im.mode == "RGB"
            px = np.asarray(im)
            if first is None:
                first = px
            assert np.array_equal(px, first), (name, q, r)


def test_psnr_and_size_against_pillow():
    """PSNR against the source no more than 0.25 dB below Pillow's encoder at the same quality and 4:2:0; size without restart
    markers within 1 % of Pillow's (constant frames: within 2 bytes, and decoded exactly).  Worst cases measured here, both on `smooth` at
    quality 100: PSNR 0.16 dB below Pillow (45.13 against 45.29 dB), size 0.76 % above Pillow's (2776 against 2755 bytes)."""
    pytest.importorskip("PIL")
    worst_db, worst_size = 0.0, 0.0
    for name in sorted(FIX):
        img = FIX[name]
        for q in QUALITIES:
            mine = encoded(name, q, 0)[0]
            theirs = pil_encode(img, q)
            p_mine = psnr(np.asarray(pil_decode(mine)), img)
            p_theirs = psnr(np.asarray(pil_decode(theirs)), img)
            print("%-12s q%-3d psnr %.2f dB (Pillow %.2f dB)  size %d (Pillow %d)" % (name, q, p_mine, p_theirs, len(mine), len(theirs)))
            if name.startswith("const"):
                assert p_mine == math.inf and abs(len(mine) - len(theirs)) <= 2
                continue
            if p_theirs != math.inf:
                worst_db = max(worst_db, p_theirs - p_mine)
                assert p_mine >= p_theirs - 0.25, (name, q, p_mine, p_theirs)
            worst_size = max(worst_size, abs(len(mine) - len(theirs)) / len(theirs))
            assert abs(len(mine) - len(theirs)) <= 0.01 * len(theirs), (name, q, len(mine), len(theirs))
    print("worst: %.3f dB below Pillow, size %.2f %% from Pillow's" % (worst_db, 100 * worst_size))


@pytest.mark.parametrize("q", [10, 25, 50, 75, 90, 95, 100])
def test_tables_are_pillows(q):
    pytest.importorskip("PIL")
    dqt, dht = jpeg_tables_of(HM.jpeg_header(16, 16, q, 0) + b"")
    dqt_p, dht_p = jpeg_tables_of(pil_encode(FIX["const200"], q))
    assert dqt == dqt_p and dht == dht_p
    ql, qc = HM.jpeg_tables(q)
    assert tuple(int(ql[z]) for z in HM.JPEG_ZIGZAG) == dqt[0] and tuple(int(qc[z]) for z in HM.JPEG_ZIGZAG) == dqt[1]


def test_fixtures_exercise_every_branch_of_the_entropy_coder():
    tot = dict(stuffed_bytes=0, zrl=0, blocks_without_eob=0, max_dc_category=0, max_ac_category=0)
    for name in FIX:
        for q in QUALITIES:
            for r in restarts(FIX[name].shape[1]):
                st = encoded(name, q, r)[1]
                for k in ("stuffed_bytes", "zrl", "blocks_without_eob"):
                    tot[k] += st[k]
                for k in ("max_dc_category", "max_ac_category"):
                    tot[k] = max(tot[k], st[k])
    print(tot)
    assert tot["stuffed_bytes"] >= 1 and tot["zrl"] >= 1 and tot["blocks_without_eob"] >= 1
    assert tot["max_dc_category"] == 11 and tot["max_ac_category"] == 10
    data, st = encoded("noise", 90, 1)
    assert st["restart_markers"] == 15  # 16 MCUs: RST0 ... RST7, then RST0 ... RST6 again
    assert [data.count(bytes((0xFF, 0xD0 + k))) >= 1 for k in range(8)] == [True] * 8


def test_header_layout():
    h = HM.jpeg_header(32, 48, 90, 3)
    assert h[:4] == b"\xff\xd8\xff\xe0" and h[6:11] == b"JFIF\0" and len(h) == 629
    assert len(HM.jpeg_header(32, 48, 90, 0)) == 623 and b"\xff\xdd" not in HM.jpeg_header(32, 48, 90, 0)
    assert HM.jpeg_header(32, 48, 90, None) == HM.jpeg_header(32, 48, 90, 3)
    data = encoded("noise_32x48", 90, 3)[0]
    assert data.startswith(h) and data.endswith(b"\xff\xd9")
    sof = h[h.index(b"\xff\xc0"):]
    assert sof[4:19] == bytes((8, 0, 32, 0, 48, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))


def test_batches_tensors_and_arrays_agree():
    batch = np.stack([FIX["noise"], FIX["extremes"], FIX["smooth"]])
    files = HM.jpeg_encode_rgb8(torch.from_numpy(batch), 90)
    assert files == [encoded(n, 90, 4)[0] for n in ("noise", "extremes", "smooth")]
    assert HM.jpeg_encode_rgb8(batch[1], 90, None) == files[1:2]


def test_argument_errors():
    ok = np.zeros((16, 16, 3), np.uint8)
    for shape in ((16, 24, 3), (8, 16, 3), (17, 16, 3), (16, 16, 4), (16, 16)):
        with pytest.raises(ValueError):
            HM.jpeg_encode_rgb8(np.zeros(shape, np.uint8))
    for q in (0, 101):
        with pytest.raises(ValueError):
            HM.jpeg_encode_rgb8(ok, q)
        with pytest.raises(ValueError):
            HM.jpeg_tables(q)
    with pytest.raises(ValueError):
        HM.jpeg_encode_rgb8(ok.astype(np.float32))
    with pytest.raises(ValueError):
        HM.jpeg_encode_rgb8(torch.zeros(16, 16, 3))
    with pytest.raises(ValueError):
        HM.jpeg_header(16, 20, 90, 0)


def test_definition_holds_the_golden_bytes():
    """tests/golden/jpeg_def.npz (tools/make_jpeg_golden.py, written only after Pillow decoded every stream): an edit of the
    definition cannot drift where Pillow is absent."""
    z = np.load(os.path.join(GOLDEN, "jpeg_def.npz"))
    for name in ("extremes", "smooth_noise"):
        assert np.array_equal(z[name], FIX[name])  # the fixtures are the ones the bytes were made from
        assert HM.jpeg_encode_rgb8(z[name], 90, None)[0] == z[name + "_q90_row"].tobytes()
        assert HM.jpeg_encode_rgb8(z[name], 100, 1)[0] == z[name + "_q100_r1"].tobytes()
