"""host_models.yuv_planes_to_rgb8 / image.PlanarYuv on the CPU: the definition float_img_front_frames_planes is held to, tied to
yuv420_to_rgb8 at 8 bits and to the float64 matrix formula above that, and the refusals of the record and of the C call."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.util import load_pkg
from tests.yuv_planes_fill import fill_planes

pkg = load_pkg()
hm, image, native = pkg.host_models, pkg.image, pkg.native


@pytest.mark.parametrize("matrix", [0, 2, 4, 6])
@pytest.mark.parametrize("chroma", hm.YUV_CHROMA)
@pytest.mark.parametrize("layout", hm.YUV_LAYOUTS)
@pytest.mark.parametrize("h,w", [(14, 12), (6, 4)])  # 4 wide: "centre" replicates, as libjpeg does
def test_packed_8_bit_420_is_yuv420_to_rgb8(h, w, layout, chroma, matrix):
    frames = torch.from_numpy(np.random.RandomState(h).randint(0, 256, (3, 3 * h // 2, w)).astype(np.uint8))
    fmt = hm.yuv_planes_format(h, w, "420", semi=layout == "nv12", matrix=matrix, chroma=chroma)
    assert torch.equal(hm.yuv_planes_to_rgb8(frames.reshape(-1), fmt), hm.yuv420_to_rgb8(frames, layout, matrix, chroma))


@pytest.mark.parametrize("matrix", [0, 2, 4, 6])
@pytest.mark.parametrize("depth", [10, 12])
def test_deep_samples_are_within_1_of_the_float64_formula(depth, matrix):
    """Bound 1: before the clamp the integer rule is within 0.5 (its rounding) + 3 * 256 * 0.5 / 16384 = 0.52 of the float64
    value (three 14-bit coefficients, operands below 256 in 8-bit units), and round() moves that value by at most 0.5: two
    integers less than 1.03 apart differ by at most 1."""
    fmt = hm.yuv_planes_format(33, 17, "444", depth, matrix=matrix)
    data, (y, u, v) = fill_planes(fmt, 1, depth + matrix, extremes=True)
    s = depth - 8
    kr, kb = (0.2126, 0.0722) if matrix & 2 else (0.299, 0.114)
    yf, cf, yoff = (255.0, 255.0, 0) if matrix & 4 else (219.0, 224.0, 16)
    Y, U, V = (y - (yoff << s)) / (yf * 2 ** s), (u - (128 << s)) / (cf * 2 ** s), (v - (128 << s)) / (cf * 2 ** s)
    R, B = Y + 2 * (1 - kr) * V, Y + 2 * (1 - kb) * U
    G = (Y - kr * R - kb * B) / (1 - kr - kb)
    want = np.round(np.clip(np.stack([R, G, B], axis=-1) * 255.0, 0, 255))
    worst = float(np.abs(hm.yuv_planes_to_rgb8(data, fmt).numpy().astype(np.float64) - want).max())
    print("depth %d matrix %d: worst difference %g" % (depth, matrix, worst))
    assert worst <= 1


@pytest.mark.parametrize("sub,semi", [("420", True), ("422", False), ("444", False)])
@pytest.mark.parametrize("chroma", hm.YUV_CHROMA)
def test_pitch_offsets_and_high_alignment_do_not_change_a_pixel(sub, semi, chroma):
    h, w, T = 9, 13, 2
    plain = hm.yuv_planes_format(h, w, sub, 10, chroma=chroma)
    hs, vs = hm.YUV_SUBSAMPLING[sub]
    cw, ch = -(-w // hs), -(-h // vs)
    y_pitch, c_pitch = 2 * w + 6, cw * (4 if semi else 2) + 10
    v_off = 18 + h * y_pitch + 6  # V first (swap_uv), a gap after the luma rows; planar U a gap after V's rows
    kw = dict(sub=sub, depth=10, shift=6, semi=semi, swap_uv=True, y_pitch=y_pitch, c_pitch=c_pitch, y_off=18, v_off=v_off,
              u_off=None if semi else v_off + ch * c_pitch + 4, frame_stride=2000, chroma=chroma)
    loose = hm.yuv_planes_format(h, w, **kw)
    a, values = fill_planes(plain, T, 3)
    b, _ = fill_planes(loose, T, 4, values)
    frames = image.PlanarYuv(b, h, w, **kw)
    assert len(frames) == T and frames.fmt == loose and (loose.u_off - loose.v_off == 2) == semi
    assert torch.equal(frames.to_rgb8(), hm.yuv_planes_to_rgb8(a, plain))
    assert torch.equal(frames[1:2].to_rgb8(), frames.to_rgb8()[1:2]) and torch.equal(frames.take([1, 0]).to_rgb8(), frames.to_rgb8()[[1, 0]])


H, W = 8, 10
BAD = {  # keyword changes to a packed yuv420p10le record of 8 x 10 that must be refused
    "planes overlap": dict(u_off=2 * W * H - 2),
    "pitch below a row": dict(y_pitch=2 * W - 2),
    "odd offset at 16 bits": dict(y_off=1),
    "depth 16": dict(depth=16),
    "4:4:0": dict(sub="440"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_the_record_refuses(case):
    kw = dict(dict(sub="420", depth=10), **BAD[case])
    with pytest.raises(ValueError):
        image.PlanarYuv(torch.zeros(4096, dtype=torch.uint8), H, W, **kw)


def test_a_buffer_one_byte_short_is_refused():
    need = hm.yuv_planes_format(H, W, "420", 10).last_end
    assert len(image.PlanarYuv.of("yuv420p10le", torch.zeros(need, dtype=torch.uint8), H, W)) == 1
    with pytest.raises(ValueError):
        image.PlanarYuv.of("yuv420p10le", torch.zeros(need - 1, dtype=torch.uint8), H, W)
    with pytest.raises(ValueError):
        image.PlanarYuv.of("yuv440p", torch.zeros(need, dtype=torch.uint8), H, W)


def _c_call(planes, data_bytes):
    L = native.lib()
    host = (C.c_uint8 * 16)()  # never dereferenced: every refusal comes before any HIP call
    rect = (C.c_int32 * 4)(0, 0, W, H)
    return L.float_img_front_frames_planes(C.cast(host, C.c_void_p), data_bytes, 1, H, W, C.byref(planes), 0, 0, rect, 0, 0, C.cast(host, C.c_void_p),
                                           4, 4, None), L.float_last_error().decode()


def test_the_c_call_refuses_the_same_without_a_gpu():
    f = hm.yuv_planes_format(H, W, "420", 10)
    good = lambda: native.ImgPlanes(f.hs, f.vs, f.depth, f.shift, f.y_off, f.u_off, f.v_off, f.y_pitch, f.c_pitch, f.c_step, f.frame_stride)  # noqa: E731
    cases = {"overlap": dict(u_off=f.u_off - 2), "pitch": dict(y_pitch=f.y_pitch - 2), "even": dict(y_off=1), "depth": dict(depth=16),
             "geometry": dict(hs=1, vs=2)}
    for word, change in cases.items():
        p = good()
        for k, v in change.items():
            setattr(p, k, v)
        rc, msg = _c_call(p, 1 << 20)
        assert rc == 1 and word in msg, (word, rc, msg)
    rc, msg = _c_call(good(), f.last_end - 1)
    assert rc == 1 and "data holds" in msg, msg
