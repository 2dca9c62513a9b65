"""The JPEG definition under pad="edge" on the CPU (host_models.jpeg_encode_rgb8 / jpeg_header / _jpeg_geometry): frames of any
size, the last row and column replicated into the partial MCUs, SOF0 carrying the true sides.

The exact statement is consequence 2 of the rule: the file of an H x W frame is the file the unpadded definition gives for the
edge-extended frame, with the four size bytes of SOF0 replaced.  The extended frame is built HERE by index clamping, not by the
definition.  Consequence 1: sides that are multiples of 16 give bitwise the file of pad=None.  Pillow (libjpeg) opens every file
at the true size, and the PSNR against the source over the visible area is held to the limit of tests/test_jpeg.py, 0.25 dB
below Pillow's own encoder.  The SIZE against Pillow is printed, not asserted: libjpeg codes blocks that lie wholly outside the
image as DC-only dummies, plain replication does not, which costs a few per cent on small frames."""
import ctypes as C
import io
import math

import numpy as np
import pytest

from tests.jpeg_util import fixtures
from tests.util import load_pkg

pkg = load_pkg()
HM = pkg.host_models
FIX = fixtures()
QUALITIES = (50, 90, 100)
RESTARTS = (0, 1, 3, None)


def _big():
    yy, xx = np.mgrid[0:135, 0:240].astype(np.float64)
    base = np.stack([127.5 + 100 * np.sin(xx / 19.0) * np.cos(yy / 13.0), 255.0 * xx / 239.0, 127.5 + 110 * np.sin((xx + yy) / 17.0)], -1)
    return np.clip(np.rint(base) + np.random.RandomState(5).randint(-6, 7, base.shape), 0, 255).astype(np.uint8)


BIG = _big()
CPU_SET = {
    "smooth_noise_50x37": FIX["smooth_noise"][:50, :37],
    "noise_17x33": FIX["noise"][:17, :33],
    "patch_63x63": FIX["patch"][:63, :63],
    "extremes_33x49": FIX["extremes"][:33, 15:64],
    "smooth_noise_16x17": FIX["smooth_noise"][:16, :17],
    "smooth_noise_5x64": FIX["smooth_noise"][:5, :64],
    "noise_1x1": FIX["noise"][:1, :1],
    "big_135x240": BIG,
}
ASSERTED = dict(CPU_SET, big_90x67=BIG[:90, :67])            # what cases 1 and 4 run on
OPENED = dict(ASSERTED, smooth_24x40=FIX["smooth"][:24, :40])  # what Pillow opens (case 3)
_cache = {}


def padded(name, q, r):
    """The definition's file of OPENED[name] under pad="edge", computed once."""
    key = (name, q, r)
    if key not in _cache:
        (_cache[key],) = HM.jpeg_encode_rgb8(OPENED[name], q, r, pad="edge")
    return _cache[key]


def edge_extended(img):
    """img with the last row and column repeated up to the next multiples of 16: index clamping, nothing of the definition."""
    H, W = img.shape[:2]
    yy = np.minimum(np.arange(-(-H // 16) * 16), H - 1)
    xx = np.minimum(np.arange(-(-W // 16) * 16), W - 1)
    return np.ascontiguousarray(img[yy[:, None], xx[None, :]])


def with_sof0_sides(data, H, W):
    """data with the four size bytes of its SOF0 segment replaced by (H, W), big-endian."""
    at = data.index(b"\xff\xc0\x00\x11\x08") + 5
    return data[:at] + bytes((H >> 8, H & 255, W >> 8, W & 255)) + data[at + 4:]


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
    Image.fromarray(np.ascontiguousarray(img)).save(b, "JPEG", quality=q, subsampling=2, optimize=False)
    return b.getvalue()


@pytest.mark.parametrize("name", sorted(ASSERTED))
def test_file_is_the_extended_frames_with_the_true_sides(name):
    """Consequence 2."""
    img = ASSERTED[name]
    H, W = img.shape[:2]
    ext = edge_extended(img)
    assert ext.shape[0] % 16 == 0 and ext.shape[1] % 16 == 0 and np.array_equal(ext[:H, :W], img)
    assert (ext[H:] == ext[H - 1]).all() and (ext[:, W:] == ext[:, W - 1:W]).all()
    for q in QUALITIES:
        for r in RESTARTS:
            (want,) = HM.jpeg_encode_rgb8(ext, q, r)
            got = padded(name, q, r)
            assert got == with_sof0_sides(want, H, W), (name, q, r)
            assert (H, W) == ext.shape[:2] or got != want  # the header differs whenever something was padded


@pytest.mark.parametrize("name", ["smooth", "noise_32x48"])
def test_whole_mcus_give_the_unpadded_file(name):
    """Consequence 1."""
    img = FIX[name]
    for q in QUALITIES:
        for r in RESTARTS:
            assert HM.jpeg_encode_rgb8(img, q, r, pad="edge") == HM.jpeg_encode_rgb8(img, q, r), (name, q, r)
    assert HM.jpeg_header(32, 48, 90, None, pad="edge") == HM.jpeg_header(32, 48, 90, None)
    files, st = HM.jpeg_encode_rgb8(img, 90, 1, stats=True, pad="edge")
    assert (files, st) == HM.jpeg_encode_rgb8(img, 90, 1, stats=True)


def test_batches_and_tensors():
    import torch
    batch = np.stack([BIG[:50, :37], BIG[40:90, 30:67]])
    files = HM.jpeg_encode_rgb8(torch.from_numpy(batch), 90, None, pad="edge")
    assert files == [HM.jpeg_encode_rgb8(b, 90, 3, pad="edge")[0] for b in batch] and files[0] != files[1]


@pytest.mark.parametrize("name", sorted(OPENED))
def test_pillow_opens_every_file_at_the_true_size_and_restart_changes_no_pixel(name):
    pytest.importorskip("PIL")
    H, W = OPENED[name].shape[:2]
    for q in QUALITIES:
        first = None
        for r in RESTARTS:
            im = pil_decode(padded(name, q, r))
            assert im.size == (W, H) and im.mode == "RGB", (name, q, r, im.size, im.mode)
            px = np.asarray(im)
            if first is None:
                first = px
            assert np.array_equal(px, first), (name, q, r)


def test_psnr_against_pillow_and_sizes_printed():
    """PSNR against the source over the visible area no more than 0.25 dB below Pillow's encoder at the same quality and 4:2:0 -
    the limit of tests/test_jpeg.py.  Sizes (without restart markers) are printed beside Pillow's and NOT asserted."""
    pytest.importorskip("PIL")
    worst_db, best_db, sizes = -math.inf, math.inf, []
    for name in sorted(ASSERTED):
        img = ASSERTED[name]
        for q in QUALITIES:
            mine, theirs = padded(name, q, 0), pil_encode(img, q)
            p_mine, p_theirs = psnr(np.asarray(pil_decode(mine)), img), psnr(np.asarray(pil_decode(theirs)), img)
            rel = 100.0 * (len(mine) - len(theirs)) / len(theirs)
            sizes.append(rel)
            print("%-20s q%-3d psnr %.3f dB (Pillow %.3f dB)  size %d (Pillow %d, %+.2f %%)" % (name, q, p_mine, p_theirs, len(mine), len(theirs), rel))
            if p_mine != math.inf and p_theirs != math.inf:
                worst_db, best_db = max(worst_db, p_theirs - p_mine), min(best_db, p_theirs - p_mine)
            assert p_mine >= p_theirs - 0.25, (name, q, p_mine, p_theirs)
    print("PSNR: at most %.3f dB below Pillow, at best %.3f dB above; size %+.2f ... %+.2f %% of Pillow's" % (worst_db, -best_db, min(sizes), max(sizes)))


def test_refusals_under_edge():
    ok = np.zeros((5, 7, 3), np.uint8)
    assert len(HM.jpeg_encode_rgb8(ok, pad="edge")) == 1
    for shape in ((0, 16, 3), (16, 0, 3), (1, 16385, 3), (16385, 1, 3)):
        with pytest.raises(ValueError):
            HM.jpeg_encode_rgb8(np.zeros(shape, np.uint8), pad="edge")
        with pytest.raises(ValueError):
            HM.jpeg_header(shape[0], shape[1], 90, 0, pad="edge")
        with pytest.raises(ValueError):
            HM._jpeg_geometry(shape[0], shape[1], None, "edge")
    assert HM._jpeg_geometry(16384, 16384, None, "edge") == (16384, 16384, 1024) and HM._jpeg_geometry(1, 1, None, "edge") == (1, 1, 1)
    for word in ("Edge", "zero", "", True, 16):
        with pytest.raises(ValueError):
            HM.jpeg_encode_rgb8(ok, pad=word)
        with pytest.raises(ValueError):
            HM.jpeg_header(16, 16, 90, 0, pad=word)
        with pytest.raises(ValueError):
            HM._jpeg_geometry(16, 16, 0, word)
    for q in (0, 101):
        with pytest.raises(ValueError):
            HM.jpeg_encode_rgb8(ok, q, pad="edge")
    with pytest.raises(ValueError):
        HM.jpeg_encode_rgb8(ok, 90, 70000, pad="edge")
    with pytest.raises(ValueError):
        HM.jpeg_encode_rgb8(ok)  # the default still refuses


def test_geometry_of_1080p():
    h = HM.jpeg_header(1080, 1920, 90, None, pad="edge")
    at = h.index(b"\xff\xc0")
    assert h[at + 4:at + 9] == bytes((8, 0x04, 0x38, 0x07, 0x80))
    dri = h.index(b"\xff\xdd")
    assert h[dri + 2:dri + 6] == bytes((0, 4, 0, 120))
    assert HM._jpeg_geometry(1080, 1920, None, "edge") == (1080, 1920, 120)
    assert HM._jpeg_geometry(90, 67, None, "edge")[2] == 5 and HM._jpeg_geometry(90, 67, 0, "edge")[2] == 0
    with pytest.raises(ValueError):
        HM.jpeg_header(1080, 1920, 90, None)


def test_python_layers_take_the_keyword():
    J, I = pkg.jpeg, pkg.image
    assert J.default_restart(67) == 4 and J.pad_restart(67) == 4 and J.pad_restart(67, "edge") == 5 and J.pad_restart(1920, "edge") == 120
    assert J.check_pad(None) is None and J.check_pad("edge") == "edge"
    with pytest.raises(ValueError):
        J.check_pad("zero")
    I.require_jpeg_sides("t", 1080, 1920, pad="edge")
    I.require_jpeg_sides("t", 1088, 1920)
    with pytest.raises(ValueError, match="multiples of 16"):
        I.require_jpeg_sides("t", 1080, 1920)
    with pytest.raises(ValueError, match="multiples of 16"):
        I.require_jpeg_sides("t", 1080, 1920, None)
    with pytest.raises(ValueError, match="pad"):
        I.require_jpeg_sides("t", 1088, 1920, pad="zero")


def test_padded_entry_points_check_their_arguments_without_a_gpu():
    """float_jpg_work_bytes_padded is host arithmetic, and float_jpg_encode_padded checks its arguments before any HIP call."""
    L = pkg.native.lib()
    wb, wbp = L.float_jpg_work_bytes, L.float_jpg_work_bytes_padded
    slot = lambda span: (span * 6 * 208 * 2 + 15) & ~15  # noqa: E731
    assert wb(1, 24, 32, 2) == 0 and wbp(1, 24, 32, 2) == ((2 * 12 + 15) & ~15) + 2 * slot(2)  # 2 x 2 MCUs, intervals of 2
    assert wbp(1, 1, 1, 0) == 16 + slot(1) and wbp(19, 33, 49, 4) == ((16 * 3 * 12 + 15) & ~15) + 16 * 3 * slot(4)
    for t, h, w, r in ((1, 64, 64, 4), (3, 512, 512, 32), (20, 32, 48, 0), (1, 16384, 16384, 1024)):
        assert wbp(t, h, w, r) == wb(t, h, w, r) > 0
    for t, h, w, r in ((0, 32, 32, 2), (1, 0, 32, 2), (1, 32, 0, 2), (1, 16385, 32, 2), (1, 32, 16385, 2), (1, 32, 32, -1), (1, 32, 32, 70000)):
        assert wbp(t, h, w, r) == 0
    assert wbp(1, 16384, 16384, 0) == 0  # one interval of 2^20 MCUs: a slot beyond 2 GiB
    one = C.c_void_p(4096)  # never dereferenced: every call below returns at a check
    for kw, word in ((dict(h=0), b"1 ... 16384"), (dict(w=16385), b"1 ... 16384"), (dict(q=0), b"quality"), (dict(r=70000), b"restart"),
                     (dict(x=None), b"null"), (dict(of=C.c_void_p(4100)), b"8-byte"), (dict(wk=C.c_void_p(4104)), b"16-byte"),
                     (dict(wbytes=15), b"float_jpg_work_bytes_padded(1, 33, 49, 4)"), (dict(h=16384, w=16384, r=0), b"2 GiB")):
        a = dict(x=one, h=33, w=49, q=90, r=4, of=one, wk=one, wbytes=1 << 20)
        a.update(kw)
        rc = L.float_jpg_encode_padded(a["x"], 1, a["h"], a["w"], a["q"], a["r"], one, 0, a["of"], a["wk"], a["wbytes"], None)
        msg = L.float_last_error()
        assert rc == 1 and word in msg and b"float_jpg_encode_padded" in msg, (kw, msg)
