"""Planar YUV 4:2:0 frames (I420), the part that needs no GPU: the two entry points on both sides of the boundary, the format's
definition in torch integer ops (host_models.rgb8_to_i420), the Y4M writer and the Python side's format rules.

The float BT.601 limited-range definition the integer one is held to is written out here independently.  Bounds: the integer
coefficients are the float ones times 256 rounded, which over all 256^3 triples stays within 0.76 (Y) / 0.99 (U) / 0.93 (V) of the
float value, i.e. within 1 level of its rounding; chroma takes the integer mean of the 2 x 2 block first, which adds at most
0.5 RGB level x 0.875 of coefficient mass, so U and V are held to 2 levels."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

from tests.util import ROOT, load_pkg

pkg = load_pkg()
NEW = ("float_dec_frames_i420", "float_dec_frames_host_i420")


def test_i420_entry_points_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    declared = set(re.findall(r"\b(float_[a-z_0-9]+)\s*\(", hdr))
    L = pkg.native.lib()
    for name in NEW:
        assert name in pkg.native.EXPORTS and name in declared
        assert hasattr(L, name)
    assert L.float_hip_abi_version() == pkg.native.ABI_VERSION == 6  # new symbols only: the version does not move


def test_i420_entry_points_refuse_null_arguments_and_unknown_matrices_without_a_gpu():
    L = pkg.native.lib()
    assert L.float_dec_frames_i420(None, None, None, 1, 0, None, None) == 1
    assert b"null argument" in L.float_last_error() and b"float_dec_frames_i420" in L.float_last_error()
    assert L.float_dec_frames_host_i420(None, None, None, 1, 0, None, None, None, None) == 1
    assert b"null argument" in L.float_last_error() and b"float_dec_frames_host_i420" in L.float_last_error()
    # every pointer set but the handle is still a null argument (nothing is dereferenced)
    buf = (C.c_float * 4)()
    assert L.float_dec_frames_i420(None, buf, buf, 1, 0, buf, None) == 1 and b"null argument" in L.float_last_error()
    assert L.float_dec_frames_host_i420(buf, buf, buf, 1, 0, buf, None, None, None) == 1 and b"null argument" in L.float_last_error()
    # a matrix other than 0 (BT.601 limited range) is FLOAT_E_INVALID, refused before the handle is looked at
    for m in (1, -1, 709):
        assert L.float_dec_frames_i420(buf, buf, buf, 1, m, buf, None) == 1
        assert b"matrix" in L.float_last_error() and b"float_dec_frames_i420" in L.float_last_error()
        assert L.float_dec_frames_host_i420(buf, buf, buf, 1, m, buf, buf, None, None) == 1
        assert b"matrix" in L.float_last_error() and b"float_dec_frames_host_i420" in L.float_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------
def _planes(i420, R):
    """(T, 3R/2, R) -> Y (T, R, R), U, V (T, R/2, R/2)"""
    flat = i420.reshape(i420.shape[0], -1)
    n = R * R
    return (flat[:, :n].reshape(-1, R, R), flat[:, n:n + n // 4].reshape(-1, R // 2, R // 2),
            flat[:, n + n // 4:].reshape(-1, R // 2, R // 2))


def _float_bt601(rgb):
    """BT.601 limited range in float64 from (T, R, R, 3) 8-bit samples: Y per pixel, Cb / Cr of the float mean of each 2 x 2 block."""
    x = rgb.astype(np.float64)
    kr, kb = 0.299, 0.114
    kg = 1.0 - kr - kb

    def ycc(p):
        y = kr * p[..., 0] + kg * p[..., 1] + kb * p[..., 2]
        cb, cr = (p[..., 2] - y) / (2 * (1 - kb)), (p[..., 0] - y) / (2 * (1 - kr))
        return 16 + 219 * y / 255, 128 + 224 * cb / 255, 128 + 224 * cr / 255

    T, R = x.shape[0], x.shape[1]
    mean = x.reshape(T, R // 2, 2, R // 2, 2, 3).mean(axis=(2, 4))
    return ycc(x)[0], ycc(mean)[1], ycc(mean)[2]


def test_rgb8_to_i420_ranges_on_the_corner_colours():
    f = pkg.host_models.rgb8_to_i420
    corners = torch.tensor([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=torch.uint8)
    img = corners.reshape(8, 1, 1, 3).expand(8, 2, 2, 3).contiguous()  # one flat 2 x 2 frame per colour
    out = f(img)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (8, 3, 2)
    y, u, v = _planes(out, 2)
    assert int(y.min()) == 16 and int(y.max()) == 235
    assert int(u.min()) == 16 and int(u.max()) == 240 and int(v.min()) == 16 and int(v.max()) == 240
    assert y[0].unique().tolist() == [16] and y[7].unique().tolist() == [235]  # black, white
    assert int(u[0]) == int(v[0]) == int(u[7]) == int(v[7]) == 128
    assert tuple(f(img[3]).shape) == (3, 2) and torch.equal(f(img[3]), out[3])  # a single frame


def test_rgb8_to_i420_grey_ramp_has_neutral_chroma():
    ramp = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    y, u, v = _planes(pkg.host_models.rgb8_to_i420(ramp), 16)
    assert u.unique().tolist() == [128] and v.unique().tolist() == [128]
    assert int(y[0, 0, 0]) == 16 and int(y[0, 15, 15]) == 235 and bool((y.reshape(-1)[1:] >= y.reshape(-1)[:-1]).all())


def test_rgb8_to_i420_against_the_float_definition():
    rgb = torch.from_numpy(np.random.RandomState(420).randint(0, 256, size=(2, 8, 8, 3)).astype(np.uint8))
    out = pkg.host_models.rgb8_to_i420(rgb)
    assert tuple(out.shape) == (2, 12, 8)
    y, u, v = (p.numpy().astype(np.float64) for p in _planes(out, 8))
    fy, fu, fv = _float_bt601(rgb.numpy())
    dy, du, dv = np.abs(y - np.rint(fy)).max(), np.abs(u - np.rint(fu)).max(), np.abs(v - np.rint(fv)).max()
    print("max |integer - rint(float BT.601)|: Y %g, U %g, V %g" % (dy, du, dv))
    assert dy <= 1 and du <= 2 and dv <= 2
    # the block mean is the rounded integer mean: a block of (1, 1, 1, 0) rounds up, (1, 0, 0, 0) down
    blk = torch.zeros(1, 2, 2, 3, dtype=torch.uint8)
    blk[0, 0, 0, 2] = blk[0, 0, 1, 2] = blk[0, 1, 0, 2] = 200
    assert int(_planes(pkg.host_models.rgb8_to_i420(blk), 2)[1]) == ((112 * 150 + 128) >> 8) + 128


def test_rgb8_to_i420_refuses_odd_sizes_and_other_inputs():
    f = pkg.host_models.rgb8_to_i420
    for shape in ((1, 7, 8, 3), (1, 8, 7, 3), (3, 3, 3)):
        with pytest.raises(ValueError):
            f(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError):
        f(torch.zeros(1, 8, 8, 3))  # fp32
    with pytest.raises(ValueError):
        f(torch.zeros(1, 8, 8, 4, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------------------
# Y4M
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps,rate", [(25, "F25:1"), (29.97, "F30000:1001"), (30000 / 1001, "F30000:1001"), (12.5, "F25:2")])
def test_write_y4m(fps, rate):
    T, R = 3, 8
    rgb = torch.from_numpy(np.random.RandomState(7).randint(0, 256, size=(T, R, R, 3)).astype(np.uint8))
    frames = pkg.host_models.rgb8_to_i420(rgb)
    f = io.BytesIO()
    pkg.host_models.write_y4m(f, frames, fps)
    data = f.getvalue()
    header = ("YUV4MPEG2 W8 H8 %s Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % rate).encode()
    assert data.startswith(header)
    payload = data[len(header):]
    fb = 3 * R * R // 2
    assert len(payload) == T * (6 + fb)
    for t in range(T):
        rec = payload[t * (6 + fb):(t + 1) * (6 + fb)]
        assert rec[:6] == b"FRAME\n"
        assert torch.equal(torch.frombuffer(bytearray(rec[6:]), dtype=torch.uint8).reshape(3 * R // 2, R), frames[t])


def test_y4m_rate_rules():
    """The NTSC shorthands mean n * 1000 / 1001; everything else is the closest fraction with a denominator up to 1001."""
    from fractions import Fraction as Fr
    rate = pkg.host_models.y4m_rate
    for fps, want in ((23.976, Fr(24000, 1001)), (29.97, Fr(30000, 1001)), (59.94, Fr(60000, 1001)), (30000 / 1001, Fr(30000, 1001)),
                      (24000 / 1001, Fr(24000, 1001)),
                      # near misses do not snap
                      (29.9, Fr(299, 10)), (30.0, Fr(30)), (30, Fr(30)), (29.98, Fr(1499, 50)), (29.96, Fr(749, 25)), (24, Fr(24)),
                      (23.98, Fr(1199, 50)), (59.9, Fr(599, 10)), (25, Fr(25)), (12.5, Fr(25, 2)), (0.5, Fr(1, 2)),
                      # a Fraction is taken as it is (up to the denominator limit)
                      (Fr(2997, 100), Fr(2997, 100)), (Fr(30000, 1001), Fr(30000, 1001))):
        assert rate(fps) == want, (fps, rate(fps), want)


def test_write_y4m_to_a_path_and_argument_rules(tmp_path):
    frames = pkg.host_models.rgb8_to_i420(torch.zeros(2, 4, 4, 3, dtype=torch.uint8))
    p = tmp_path / "clip.y4m"
    pkg.host_models.write_y4m(str(p), frames, 25)
    assert p.read_bytes().startswith(b"YUV4MPEG2 W4 H4 F25:1 ") and p.stat().st_size == len(b"YUV4MPEG2 W4 H4 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n") + 2 * (6 + 24)
    with pytest.raises(ValueError):
        pkg.host_models.write_y4m(io.BytesIO(), torch.zeros(2, 4, 4, 3, dtype=torch.uint8), 25)  # RGB, not I420


# ---------------------------------------------------------------------------------------------------------------------------
# the Python side's format rules
# ---------------------------------------------------------------------------------------------------------------------------
def test_frame_format_rules_need_no_gpu():
    P = pkg.pipeline
    u8, f32 = torch.uint8, torch.float32
    rgb8, yuv, fp = torch.empty(2, 8, 8, 3, dtype=u8), torch.empty(2, 12, 8, dtype=u8), torch.empty(2, 8, 8, 3)
    R = P.resolve_out_format
    assert R(None, None, None) == (f32, "rgb")
    assert R(None, None, "rgb") == (f32, "rgb")
    assert R(None, u8, None) == (u8, "rgb") and R(None, u8, "rgb") == (u8, "rgb")
    assert R(None, None, "i420") == (u8, "i420") and R(None, u8, "i420") == (u8, "i420")  # "i420" implies uint8
    assert R(rgb8, None, None) == (u8, "rgb") and R(rgb8, None, "rgb") == (u8, "rgb")
    assert R(fp, None, None) == (f32, "rgb") and R(fp, f32, "rgb") == (f32, "rgb")
    assert R(yuv, None, None) == (u8, "i420") and R(yuv, u8, "i420") == (u8, "i420")  # `out` fixes the format
    for args in ((None, f32, "i420"),      # I420 is uint8
                 (fp, None, "i420"),       # an fp32 destination
                 (rgb8, None, "i420"),     # a destination of the other format
                 (yuv, None, "rgb"),
                 (yuv, f32, None),         # dtype contradiction, as before
                 (None, torch.float16, "i420"),
                 (None, None, "nv12"),
                 (None, None, "I420")):
        with pytest.raises(ValueError):
            R(*args)
    # _resolve_out_dtype keeps its behaviour
    assert P._resolve_out_dtype(None, None) == f32 and P._resolve_out_dtype(None, u8) == u8
    assert P._resolve_out_dtype(rgb8, None) == u8 and P._resolve_out_dtype(fp, f32) == f32
    with pytest.raises(ValueError):
        P._resolve_out_dtype(rgb8, f32)
    with pytest.raises(ValueError):
        P._resolve_out_dtype(None, torch.float16)
