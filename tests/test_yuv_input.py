"""YUV 4:2:0 as INPUT on the CPU: the YUV_INVERSE table against its float64 rule, host_models.yuv420_to_rgb8 (layouts, chroma
rules, refusals), the round trip through rgb8_to_i420, and Y4MReader on what write_y4m writes."""
import io

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm = pkg.host_models
IDS = (0, 2, 4, 6)
H, W = 10, 14


def _float_rule(i):
    """(yoff, cy, crv, cgu, cgv, cbu) of id i in float64"""
    kr, kb = (0.2126, 0.0722) if i & 2 else (0.299, 0.114)
    kg, full = 1.0 - kr - kb, bool(i & 4)
    s, crv, cbu = 1.0 if full else 255 / 224, 2 * (1 - kr), 2 * (1 - kb)
    return 0 if full else 16, 1.0 if full else 255 / 219, crv * s, cbu * s * kb / kg, crv * s * kr / kg, cbu * s


def _frames(seed=3, t=2):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (t, 3 * H // 2, W)).astype(np.uint8))


@pytest.mark.parametrize("i", IDS)
def test_inverse_table_is_the_rounded_float_rule_and_stays_within_its_bound(i):
    f = _float_rule(i)
    row = hm.YUV_INVERSE[i]
    assert row == (f[0],) + tuple(round(16384 * c) for c in f[1:])
    if i == 0:
        assert row == (16, 19077, 26149, 6419, 13320, 33050)
    yoff, cy, crv, cgu, cgv, cbu = row
    bound = 0.5 + 3 * 255 * 0.5 / 16384  # the final rounding plus the coefficients' roundings: derived, not measured
    v = np.arange(256, dtype=np.int64)
    y, u, c = (v - yoff)[:, None, None], (v - 128)[None, :, None], (v - 128)[None, None, :]
    for got, want in (((cy * y + crv * c + 8192) >> 14, f[1] * y + f[2] * c),
                      ((cy * y - cgu * u - cgv * c + 8192) >> 14, f[1] * y - f[3] * u - f[4] * c),
                      ((cy * y + cbu * u + 8192) >> 14, f[1] * y + f[5] * u)):
        worst = float(np.abs(got - want).max())  # all 2^24 triples by broadcasting
        print("id %d: %.4f of %.4f" % (i, worst, bound))
        assert worst <= bound


@pytest.mark.parametrize("i", IDS)
def test_nearest_is_the_formula_on_replicated_chroma_and_nv12_is_i420_reinterleaved(i):
    x = _frames()
    yoff, cy, crv, cgu, cgv, cbu = hm.YUV_INVERSE[i]
    y = x[:, :H].long() - yoff
    u, v = (x[:, H:].reshape(2, 2, H // 2, W // 2)[:, k].long().repeat_interleave(2, 1).repeat_interleave(2, 2) - 128 for k in (0, 1))
    want = torch.stack([(cy * y + crv * v + 8192) >> 14, (cy * y - cgu * u - cgv * v + 8192) >> 14, (cy * y + cbu * u + 8192) >> 14], -1)
    assert torch.equal(hm.yuv420_to_rgb8(x, "i420", i), want.clamp(0, 255).to(torch.uint8))
    assert torch.equal(hm.yuv420_to_rgb8(x[0], "i420", i), hm.yuv420_to_rgb8(x, "i420", i)[0])
    uv = x[:, H:].reshape(2, 2, H // 2, W // 2).permute(0, 2, 3, 1).reshape(2, H // 2, W)
    nv12 = torch.cat([x[:, :H], uv], 1)
    for chroma in ("nearest", "centre"):
        assert torch.equal(hm.yuv420_to_rgb8(nv12, "nv12", i, chroma), hm.yuv420_to_rgb8(x, "i420", i, chroma))


def test_centre_is_the_jpeg_definitions_upsampled_planes():
    x = _frames(t=1)
    planes = x[0, H:].reshape(2, H // 2, W // 2).numpy().astype(np.int32)
    up = [hm.jpeg_upsample_plane(p, 2, 2) for p in planes]  # H x W each
    yoff, cy, crv, cgu, cgv, cbu = hm.YUV_INVERSE[0]
    y, u, v = x[0, :H].long() - yoff, torch.from_numpy(up[0]).long() - 128, torch.from_numpy(up[1]).long() - 128
    want = torch.stack([(cy * y + crv * v + 8192) >> 14, (cy * y - cgu * u - cgv * v + 8192) >> 14, (cy * y + cbu * u + 8192) >> 14], -1)
    assert torch.equal(hm.yuv420_to_rgb8(x[0], chroma="centre"), want.clamp(0, 255).to(torch.uint8))
    assert not torch.equal(hm.yuv420_to_rgb8(x[0], chroma="centre"), hm.yuv420_to_rgb8(x[0]))


@pytest.mark.parametrize("shape", [(13, 14), (14, 14), (15, 7), (2, 9, 6, 3)])  # no whole H; H = 9.33; odd W; RGB
def test_odd_sizes_and_wrong_shapes_raise(shape):
    with pytest.raises(ValueError):
        hm.yuv420_to_rgb8(torch.zeros(shape, dtype=torch.uint8))


def test_unknown_layout_chroma_and_matrix_raise():
    for kw in (dict(layout="nv21"), dict(chroma="left"), dict(matrix="bt2020")):
        with pytest.raises(ValueError):
            hm.yuv420_to_rgb8(_frames(), **kw)


@pytest.mark.parametrize("i", IDS)
def test_round_trip_through_rgb8_to_i420(i):
    """Frames constant per 2 x 2 block (chroma siting plays no part) over a grid of RGB that includes the corners of the cube:
    measured on the CPU, the worst |back - rgb| is 3 levels for the two limited-range ids (0, 2) and 2 for the two full-range ids (4, 6);
    asserted with one level more, for the two roundings of the forward table's 1.17-level error (test_yuv_matrix.py)."""
    measured = {0: 3, 2: 3, 4: 2, 6: 2}
    g = torch.tensor(list(range(0, 256, 5)), dtype=torch.uint8)
    rgb = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, 52, 52 * 52, 3)
    rgb = rgb.repeat_interleave(2, 1).repeat_interleave(2, 2)
    back = hm.yuv420_to_rgb8(hm.rgb8_to_i420(rgb, i), matrix=i)
    worst = int((back.int() - rgb.int()).abs().max())
    print("id %d: round trip within %d levels" % (i, worst))
    assert worst <= measured[i] + 1


@pytest.mark.parametrize("matrix", [0, 6])
def test_y4m_reader_returns_what_write_y4m_was_given(matrix, tmp_path):
    x = torch.from_numpy(np.random.RandomState(8).randint(0, 256, (5, 3 * W // 2, W)).astype(np.uint8))  # write_y4m takes square frames
    path = str(tmp_path / "clip.y4m")
    hm.write_y4m(path, x, 29.97, matrix)
    with hm.Y4MReader(path) as r:
        assert (len(r), r.width, r.height, r.chroma_tag) == (5, W, W, "420jpeg")
        assert r.fps == hm.y4m_rate(29.97) and r.full_range == bool(matrix & 4) and r.matrix == (matrix & 4)
        assert torch.equal(r.read(), x) and torch.equal(r.read(3, 9), x[3:]) and [c.shape[0] for c in r.chunks(2)] == [2, 2, 1]
    buf = io.BytesIO(b"YUV4MPEG2 W4 H4 F25:1 Ip C422\n")
    with pytest.raises(ValueError, match="C422"):
        hm.Y4MReader(buf)
    with pytest.raises(ValueError, match="interlaced"):
        hm.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H4 F25:1 It C420\n"))
    long = hm.Y4MReader(io.BytesIO(b"YUV4MPEG2 W4 H2 F25:1 Ip " + b"XCOMMENT=" + b"x" * 400 + b" XCOLORRANGE=FULL\nFRAME\n" + bytes(range(12))))
    assert (len(long), long.full_range) == (1, True) and long.read(0, 1, pin=False).flatten().tolist() == list(range(12))  # a header past 256 bytes
