"""The colour matrices of the I420 outputs (ids 0 / 2 / 4 / 6: BT.601 / BT.709, limited / full range), the part that needs no GPU:
the table the kernels use (float_yuv_matrix) against host_models.YUV_MATRICES, the table's properties over all 256^3 RGB triples,
the names, the Y4M tag, the ffmpeg arguments and the format rules of the Python layers.

Bounds.  The distance of the integer planes from the float64 formulas of the standards is held to 1.25 levels: the largest one
over all triples, ids and planes is 1.17 (U of id 2, whose G coefficient is -86 instead of the rounded -87 so that the row sums to
0), rounded up; the test prints every maximum.  Pillow's YCbCr is JFIF's full-range BT.601 in its own fixed point: 1 level."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

from tests.util import ROOT, load_pkg

pkg = load_pkg()
H = pkg.host_models
IDS = (0, 2, 4, 6)
NAMES = {"bt601": 0, "bt709": 2, "bt601-full": 4, "bt709-full": 6}
TABLE = {
    0: ((66, 129, 25, 128, 16), (-38, -74, 112, 128, 128), (112, -94, -18, 128, 128)),
    2: ((47, 157, 16, 128, 16), (-26, -86, 112, 128, 128), (112, -102, -10, 128, 128)),
    4: ((77, 150, 29, 128, 0), (-43, -85, 128, 127, 128), (128, -107, -21, 127, 128)),
    6: ((54, 183, 19, 128, 0), (-29, -99, 128, 127, 128), (128, -116, -12, 127, 128)),
}


def test_the_table_is_the_one_the_issue_fixed():
    assert {k: tuple(tuple(r) for r in v) for k, v in H.YUV_MATRICES.items()} == TABLE


def test_float_yuv_matrix_is_exported_declared_and_returns_the_table():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    declared = set(re.findall(r"\b(float_[a-z_0-9]+)\s*\(", hdr))
    L = pkg.native.lib()
    assert "float_yuv_matrix" in pkg.native.EXPORTS and "float_yuv_matrix" in declared and hasattr(L, "float_yuv_matrix")
    assert L.float_hip_abi_version() == pkg.native.ABI_VERSION == 6  # a new symbol only: the version does not move
    for name, val in (("BT601_LIMITED", 0), ("BT709_LIMITED", 2), ("BT601_FULL", 4), ("BT709_FULL", 6)):
        for fam in ("DEC", "IMG"):
            assert re.search(r"\bFLOAT_%s_MATRIX_%s = %d\b" % (fam, name, val), hdr), (fam, name)
    assert "the only one" not in hdr
    for m in IDS:
        t = (C.c_int32 * 15)(*([-999] * 15))
        assert L.float_yuv_matrix(m, t) == 0
        assert tuple(t) == tuple(v for row in H.YUV_MATRICES[m] for v in row), m
    for m in (1, 3, 8, -1, 709):
        t = (C.c_int32 * 15)(*([-999] * 15))
        assert L.float_yuv_matrix(m, t) == 1
        msg = L.float_last_error()
        assert b"matrix" in msg and b"float_yuv_matrix" in msg
        assert set(t) == {-999}  # nothing written


def test_unknown_ids_are_refused_by_the_i420_entry_points_without_a_gpu():
    """5, 7, 3 and 8 join 1, -1 and 709 (tests/test_dec_i420.py, tests/test_img_paste_i420.py); the message lists the valid ids."""
    L = pkg.native.lib()
    buf = (C.c_float * 4)()
    p = C.c_void_p(C.addressof(buf))  # never dereferenced
    for m in (1, 3, 5, 7, 8, -1, 709):
        assert L.float_dec_frames_i420(buf, buf, buf, 1, m, buf, None) == 1
        msg = L.float_last_error()
        assert b"matrix" in msg and b"float_dec_frames_i420" in msg and b"6 = BT.709 full" in msg
        assert L.float_dec_frames_host_i420(buf, buf, buf, 1, m, buf, buf, None, None) == 1
        msg = L.float_last_error()
        assert b"matrix" in msg and b"float_dec_frames_host_i420" in msg and b"6 = BT.709 full" in msg
        assert L.float_img_paste_i420(p, 34, 50, p, 2, 64, 64, 7, 5, 21, 19, 4, m, p, None) == 1
        msg = L.float_last_error()
        assert b"matrix" in msg and b"float_img_paste_i420" in msg and b"6 = BT.709 full" in msg


def _float_planes(m, r, g, b):
    """The float64 formulas of the standards for 8-bit R'G'B' in 0 ... 255"""
    kr, kb = (0.2126, 0.0722) if m & 2 else (0.299, 0.114)
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    pb, pr = 0.5 * (b - y) / (1.0 - kb), 0.5 * (r - y) / (1.0 - kr)
    if m & 4:
        return y, 128.0 + pb, 128.0 + pr
    return 16.0 + 219.0 / 255.0 * y, 128.0 + 224.0 / 255.0 * pb, 128.0 + 224.0 / 255.0 * pr


@pytest.mark.parametrize("m", IDS)
def test_all_rgb_triples(m):
    """Over all 256^3 triples: the exact output ranges (no clamp is needed), and the distance from the float64 formulas."""
    rows = H.YUV_MATRICES[m]
    g, b = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    lo, hi, far = [10 ** 6] * 3, [-10 ** 6] * 3, [0.0] * 3
    for r in range(256):
        want = _float_planes(m, float(r), g.astype(np.float64), b.astype(np.float64))
        for p, (cr, cg, cb, rnd, off) in enumerate(rows):
            v = ((cr * r + cg * g + cb * b + rnd) >> 8) + off
            lo[p], hi[p] = min(lo[p], int(v.min())), max(hi[p], int(v.max()))
            far[p] = max(far[p], float(np.abs(v - want[p]).max()))
    print("  id %d: Y [%d, %d] U [%d, %d] V [%d, %d]; max distance from float64: Y %.3f U %.3f V %.3f"
          % (m, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], far[0], far[1], far[2]))
    if m & 4:
        assert (lo, hi) == ([0, 0, 0], [255, 255, 255])
    else:
        assert (lo, hi) == ([16, 16, 16], [235, 240, 240])
    assert max(far) <= 1.25
    # every grey level: U = V = 128 exactly, and Y runs over the whole range
    for p, (cr, cg, cb, rnd, off) in enumerate(rows):
        k = np.arange(256, dtype=np.int32)
        v = (((cr + cg + cb) * k + rnd) >> 8) + off
        if p:
            assert (v == 128).all()
        else:
            assert v[0] == (0 if m & 4 else 16) and v[255] == (255 if m & 4 else 235)


@pytest.mark.parametrize("m", IDS)
def test_rgb8_to_i420_applies_the_rows(m):
    """rgb8_to_i420(x, m) against the rows written out in numpy on random frames (block means included), grey frames and the
    primaries; every spelling of the matrix gives the same bytes."""
    rs = np.random.RandomState(40 + m)
    x = rs.randint(0, 256, size=(3, 6, 10, 3)).astype(np.uint8)
    x[1, :2, :4] = (0, 0, 255)
    x[1, 2:4, :4] = (255, 0, 0)
    x[2] = np.arange(60, dtype=np.uint8).reshape(6, 10, 1) * 4 + 3  # greys
    xi = x.astype(np.int32)
    ky, ku, kv = H.YUV_MATRICES[m]
    plane = lambda k, c: ((k[0] * c[..., 0] + k[1] * c[..., 1] + k[2] * c[..., 2] + k[3]) >> 8) + k[4]  # noqa: E731
    mean = (xi.reshape(3, 3, 2, 5, 2, 3).sum(axis=(2, 4)) + 2) >> 2
    want = np.concatenate([plane(ky, xi).reshape(3, -1), plane(ku, mean).reshape(3, -1), plane(kv, mean).reshape(3, -1)], axis=1)
    assert want.min() >= 0 and want.max() <= 255
    got = H.rgb8_to_i420(torch.from_numpy(x), m)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 9, 10)
    assert np.array_equal(got.numpy().reshape(3, -1), want.astype(np.uint8))
    assert (got[2, 6:] == 128).all()
    name = [k for k, v in NAMES.items() if v == m][0]
    assert torch.equal(H.rgb8_to_i420(torch.from_numpy(x), matrix=name), got)
    assert torch.equal(H.rgb8_to_i420(torch.from_numpy(x[0]), matrix=m), got[0])


def test_id_0_and_none_are_the_formula_of_the_docstring():
    x = torch.from_numpy(np.random.RandomState(3).randint(0, 256, size=(4, 16, 12, 3)).astype(np.uint8))
    xi = x.to(torch.int32)
    r, g, b = xi[..., 0], xi[..., 1], xi[..., 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    mm = (xi.reshape(4, 8, 2, 6, 2, 3).sum(dim=(2, 4)) + 2) >> 2
    mr, mg, mb = mm[..., 0], mm[..., 1], mm[..., 2]
    u = ((-38 * mr - 74 * mg + 112 * mb + 128) >> 8) + 128
    v = ((112 * mr - 94 * mg - 18 * mb + 128) >> 8) + 128
    want = torch.cat([y.reshape(4, -1), u.reshape(4, -1), v.reshape(4, -1)], dim=1).to(torch.uint8).reshape(4, 24, 12)
    assert torch.equal(H.rgb8_to_i420(x), want)
    assert torch.equal(H.rgb8_to_i420(x, matrix=None), want)
    assert torch.equal(H.rgb8_to_i420(x, matrix=0), want)
    assert torch.equal(H.rgb8_to_i420(x, matrix="bt601"), want)


def test_full_range_bt601_is_pillows_ycbcr_within_one_level():
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(8)
    small = rs.randint(0, 256, size=(32, 32, 3)).astype(np.uint8)
    small[0, :8] = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)]
    x = np.repeat(np.repeat(small, 2, axis=0), 2, axis=1)  # 2 x 2-constant: the block mean is the sample
    got = H.rgb8_to_i420(torch.from_numpy(x), 4).numpy().astype(np.int32)
    ref = np.asarray(Image.fromarray(small, "RGB").convert("YCbCr")).astype(np.int32)
    y, u, v = got[:64], got[64:80].reshape(32, 32), got[80:].reshape(32, 32)
    d = [int(np.abs(y[::2, ::2] - ref[..., 0]).max()), int(np.abs(u - ref[..., 1]).max()), int(np.abs(v - ref[..., 2]).max())]
    print("  id 4 against Pillow's YCbCr: max |d| Y %d Cb %d Cr %d" % tuple(d))
    assert max(d) <= 1
    assert np.array_equal(y[::2, ::2], y[1::2, 1::2])


def test_names_ids_and_auto():
    assert H.yuv_matrix_id(None) == 0
    for name, m in NAMES.items():
        assert H.yuv_matrix_id(name) == m and H.yuv_matrix_id(m) == m
        assert H.yuv_matrix_id(name, 1920, 1080) == m  # a stated matrix does not look at the size
    for (w, h), m in (((512, 512), 0), ((1024, 576), 0), ((1280, 720), 2), ((1920, 1080), 2), ((720, 578), 2), ((1279, 576), 0)):
        assert H.yuv_matrix_id("auto", w, h) == m, (w, h)
        assert H.yuv_matrix_id("auto", width=w, height=h) == m
    for bad in ("auto", "bt2020", "BT709", "", 1, 3, 5, 7, 8, -1, 709, 2.0, True, "2"):
        with pytest.raises(ValueError):
            H.yuv_matrix_id(bad)
    with pytest.raises(ValueError):
        H.yuv_matrix_id("auto", 1280)  # half a size is no size
    with pytest.raises(ValueError):
        H.rgb8_to_i420(torch.zeros(2, 2, 3, dtype=torch.uint8), matrix="auto")
    assert "untagged" in H.yuv_matrix_id.__doc__ and "convention" in H.yuv_matrix_id.__doc__


def test_paste_i420_takes_the_matrix():
    rs = np.random.RandomState(12)
    src = torch.from_numpy(rs.randint(0, 256, size=(34, 50, 3)).astype(np.uint8))
    frames = torch.from_numpy(rs.randint(0, 256, size=(2, 16, 16, 3)).astype(np.uint8))
    rgb = H.paste_rgb8(src, frames, (7, 5, 21, 19), 4)
    assert torch.equal(H.paste_i420(src, frames, (7, 5, 21, 19), 4), H.rgb8_to_i420(rgb))
    for m in IDS:
        assert torch.equal(H.paste_i420(src, frames, (7, 5, 21, 19), 4, matrix=m), H.rgb8_to_i420(rgb, m))
    assert not torch.equal(H.paste_i420(src, frames, (7, 5, 21, 19), 4, matrix=6), H.paste_i420(src, frames, (7, 5, 21, 19), 4))


def test_y4m_range_tag():
    frames = H.rgb8_to_i420(torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(3, 8, 8, 3)).astype(np.uint8)), 6)
    old = b"YUV4MPEG2 W8 H8 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    for m, tag in ((None, b"LIMITED"), (0, b"LIMITED"), (2, b"LIMITED"), (4, b"FULL"), (6, b"FULL"), ("bt709", b"LIMITED"),
                   ("bt601-full", b"FULL"), ("auto", b"LIMITED")):
        f = io.BytesIO()
        with H.Y4MWriter(f, 8, 8, 25, matrix=m) as w:
            head = f.getvalue()
            w.write(frames)
        assert head == old.replace(b"LIMITED", tag), m
        g = io.BytesIO()
        H.write_y4m(g, frames, 25, matrix=m)
        assert g.getvalue() == f.getvalue()
        assert g.getvalue().count(b"XCOLORRANGE") == 1
    f = io.BytesIO()
    H.Y4MWriter(f, 8, 8, 25).close()
    assert f.getvalue() == old  # no keyword: today's header, byte for byte
    g = io.BytesIO()
    H.write_y4m(g, frames, 25)
    assert g.getvalue().startswith(old)
    with pytest.raises(ValueError):
        H.Y4MWriter(io.BytesIO(), 8, 8, 25, matrix=1)


def test_ffmpeg_arguments():
    want = {0: ("smpte170m", "tv"), 2: ("bt709", "tv"), 4: ("smpte170m", "pc"), 6: ("bt709", "pc")}
    for m, (name, rng) in want.items():
        exp = ["-colorspace", name, "-color_primaries", name, "-color_trc", name, "-color_range", rng]
        assert H.yuv_ffmpeg_args(m) == exp
        assert H.yuv_ffmpeg_args([k for k, v in NAMES.items() if v == m][0]) == exp
    assert H.yuv_ffmpeg_args(None) == H.yuv_ffmpeg_args(0)
    for bad in ("auto", 1, "bt2020"):
        with pytest.raises(ValueError):
            H.yuv_ffmpeg_args(bad)


def test_a_matrix_with_rgb_frames_is_refused_without_a_gpu():
    R = pkg.pipeline.resolve_out_format
    assert R(None, None, "i420", "bt709") == (torch.uint8, "i420")
    assert R(None, None, "i420", 6) == (torch.uint8, "i420")
    assert R(None, None, "i420", "auto") == (torch.uint8, "i420")
    assert R(None, None, "i420") == R(None, None, "i420", None) == (torch.uint8, "i420")
    assert R(torch.empty(2, 96, 64, dtype=torch.uint8), None, None, "bt709-full") == (torch.uint8, "i420")
    for kw in (dict(out_format="rgb"), dict(out_format=None), dict(out_format="rgb", out_dtype=torch.uint8),
               dict(out_format=None, out_dtype=torch.float32), dict(out_format=None, out_dtype=torch.uint8),
               dict(out=torch.empty(2, 64, 64, 3, dtype=torch.uint8), out_format=None)):
        args = (kw.get("out"), kw.get("out_dtype"), kw.get("out_format"))
        assert R(*args)[1] == "rgb"
        for m in ("bt709", 0, 2, "auto"):
            with pytest.raises(ValueError, match="matrix"):
                R(*args, m)
    for bad in (1, "bt2020", 709):
        with pytest.raises(ValueError, match="matrix"):
            R(None, None, "i420", bad)
    # the same rule one layer down, where there is no GPU to touch either
    for fmt in ("rgb", "jpeg"):
        with pytest.raises(ValueError, match="matrix"):
            H.yuv_matrix_for("a call", "bt709", fmt, 64, 64)
        assert H.yuv_matrix_for("a call", None, fmt, 64, 64) == 0
    assert H.yuv_matrix_for("a call", "auto", "i420", 1920, 1080) == 2
    assert H.yuv_matrix_for("a call", "auto", "i420", 64, 64) == 0
    with pytest.raises(ValueError, match="matrix"):
        pkg.image.paste_frames_device(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(1, 2, 2, 3, dtype=torch.uint8), (0, 0, 2, 2),
                                      out_format="rgb", matrix="bt709")
