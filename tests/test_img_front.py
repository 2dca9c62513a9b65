"""The definition of the image front end (host_models.hex_to_rgb8 / image_to_rgb8 / resize_rgb8), on the CPU.

image_to_rgb8 is pinned to the reference: tests/golden/img_front.npz holds what the reference's img_tensor_2_np_array made of
small RGBA / RGB images (tools/make_img_front_golden.py), and every entry must come out bitwise.
resize_rgb8 is checked against a brute-force evaluation of its stated rule with fractions.Fraction, one output sample at a
time, no matrices: exact rationals, so the comparison is equality."""
import ctypes as C
import logging
import os
import re
from fractions import Fraction
from math import floor, gcd

import numpy as np
import pytest
import torch

from tests.util import GOLDEN, ROOT, load_pkg

pkg = load_pkg()
hm = pkg.host_models


# ---------------------------------------------------------------------------------------------------------------------------
# stage 1 and 2: colour string, quantiser, RGBA conversion
# ---------------------------------------------------------------------------------------------------------------------------
def test_hex_to_rgb8(caplog):
    assert hm.hex_to_rgb8("#3fa07c") == (0x3F, 0xA0, 0x7C) and hm.hex_to_rgb8("00FF00") == (0, 255, 0)
    with caplog.at_level(logging.WARNING):
        assert hm.hex_to_rgb8("#fff") == (0, 0, 0)        # short
        assert hm.hex_to_rgb8("#12345g") == (0, 0, 0)     # a character that is no hexadecimal digit
    assert len([r for r in caplog.records if r.levelno == logging.WARNING]) == 2


def test_image_to_rgb8_equals_the_reference_bitwise():
    z = np.load(os.path.join(GOLDEN, "img_front.npz"))
    names, strategies, bkgs = [str(s) for s in z["names"]], [str(s) for s in z["strategies"]], [str(s) for s in z["bkgs"]]
    assert len(names) >= 4 and len(strategies) == 3 and len(bkgs) == 2
    checked = 0
    for name in names:
        img = torch.from_numpy(z["img_" + name])
        assert img.shape[0] <= 24 and img.shape[1] <= 20
        if img.shape[-1] == 3:
            want = torch.from_numpy(z["out_" + name])
            for st in strategies:  # the strategy is about alpha only
                assert torch.equal(hm.image_to_rgb8(img, st, (1, 2, 3)), want), name
            checked += 1
            continue
        outs = z["out_" + name]  # [strategy, background]
        assert outs.shape == (3, 2) + tuple(img.shape[:2]) + (3,)
        for i, st in enumerate(strategies):
            for j, bk in enumerate(bkgs):
                want = torch.from_numpy(outs[i, j])
                got = hm.image_to_rgb8(img, st, hm.hex_to_rgb8(bk))
                assert got.dtype == torch.uint8 and torch.equal(got, want), (name, st, bk, int((got != want).sum()))
                checked += 1
    assert checked >= 3 * 6 + 2
    # the fixture covers what it claims: values below 0 and above 1, alpha 0, 1 / 255 and 1
    a = z["img_rgba_noise"]
    assert a.min() < 0 and a.max() > 1 and (a[..., 3] == 0).any() and (a[..., 3] == 1).any()
    assert (a[..., 3] == np.float32(1.0) / np.float32(255.0)).any()


def test_image_to_rgb8_choices(caplog):
    """NaN gives 0 (this project's choice); an unknown strategy warns and discards alpha, as in the reference."""
    img = torch.tensor([[[float("nan"), 0.5, 2.0, 0.0], [0.25, -1.0, 1.0, 1.0]]])
    assert hm.image_to_rgb8(img, "discard_alpha").tolist() == [[[0, 127, 255], [63, 0, 255]]]
    with caplog.at_level(logging.WARNING):
        assert torch.equal(hm.image_to_rgb8(img, "premultiply"), hm.image_to_rgb8(img, "discard_alpha"))
    assert any("premultiply" in r.getMessage() for r in caplog.records)
    assert hm.image_to_rgb8(img, "replace_with_color", (9, 8, 7)).tolist() == [[[9, 8, 7], [63, 0, 255]]]
    with pytest.raises(ValueError):
        hm.image_to_rgb8(torch.zeros(4, 4, 2))


# ---------------------------------------------------------------------------------------------------------------------------
# stage 3: the resize, against exact rationals
# ---------------------------------------------------------------------------------------------------------------------------
def round_half_even(fr):
    q = floor(fr)
    r = fr - q
    return q + 1 if (r > Fraction(1, 2) or (r == Fraction(1, 2) and q % 2 == 1)) else q


def axis_taps(d, n, dst, scale, linear):
    """[(window sample, weight)] and the divisor of destination index d on one axis, as the issue states the rule"""
    num, den = scale if scale is not None else (n, dst)
    g = gcd(num, den)
    P, Q = num // g, den // g
    if linear:
        sx = (d * P) // Q
        m = (d + 1) * P - (sx + 1) * Q
        f = 0 if m <= 0 else m % P
        if sx >= n - 1:
            sx, f = n - 1, 0
        return [(sx, P - f), (min(sx + 1, n - 1), f)], P
    c0, c1 = d * P, min((d + 1) * P, n * Q)
    taps = []
    for i in range(n):
        ov = min((i + 1) * Q, c1) - max(i * Q, c0)
        if ov > 0:
            taps.append((i, ov))
    return taps, c1 - c0


def brute(rgb8, rect, dst_h, dst_w, scale=None):
    H, W, _ = rgb8.shape
    x0, y0, w, h = rect if rect is not None else (0, 0, W, H)

    def is_linear(n, dst):
        num, den = scale if scale is not None else (n, dst)
        return num < den  # P < Q

    linear = is_linear(w, dst_w) or is_linear(h, dst_h)
    src = rgb8.tolist()
    out = torch.zeros(dst_h, dst_w, 3, dtype=torch.uint8)
    for dy in range(dst_h):
        ty, Dy = axis_taps(dy, h, dst_h, scale, linear)
        for dx in range(dst_w):
            tx, Dx = axis_taps(dx, w, dst_w, scale, linear)
            for c in range(3):
                acc = Fraction(0)
                for iy, wy in ty:
                    for ix, wx in tx:
                        yy, xx = y0 + iy, x0 + ix
                        v = src[yy][xx][c] if (0 <= yy < H and 0 <= xx < W) else 0
                        acc += Fraction(v * wx * wy)
                out[dy, dx, c] = round_half_even(acc / (Dx * Dy))
    return out


def noise8(seed, h, w):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8))


# (H, W) -> (dst_h, dst_w), rect, scale
RESIZE_CASES = {
    "area_fractional_7x5_to_3x2": ((7, 5), (3, 2), None, None),
    "integer_factor_8x8_to_4x4": ((8, 8), (4, 4), None, None),
    "linear_5x4_to_8x7": ((5, 4), (8, 7), None, None),
    "mixed_5x9_to_7x7": ((5, 9), (7, 7), None, None),
    "identity_9x9": ((9, 9), (9, 9), None, None),
    "rect_3_outside_on_two_sides": ((10, 12), (4, 5), (-3, -3, 11, 9), None),
    "shared_scale_9x7_at_9_4_to_4x3": ((9, 7), (4, 3), None, (9, 4)),
}


@pytest.mark.parametrize("case", sorted(RESIZE_CASES))
def test_resize_rgb8_equals_the_rule_in_exact_rationals(case):
    (H, W), (dh, dw), rect, scale = RESIZE_CASES[case]
    img = noise8(sum(map(ord, case)), H, W)
    got = hm.resize_rgb8(img, rect, dh, dw, scale)
    want = brute(img, rect, dh, dw, scale)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (dh, dw, 3)
    assert torch.equal(got, want), (got.int() - want.int()).abs().max()
    if case.startswith("identity"):
        assert torch.equal(got, img)
    if case.startswith("integer_factor"):  # the rounded-half-even block mean
        s = img.to(torch.int64).reshape(4, 2, 4, 2, 3).sum(dim=(1, 3))
        mean = s // 4 + (((s % 4) == 3) | (((s % 4) == 2) & ((s // 4) % 2 == 1))).to(torch.int64)
        assert torch.equal(got.to(torch.int64), mean)
        assert int(((s % 4) == 2).sum()) > 0  # exact ties are among them
    if case.startswith("rect"):
        assert torch.equal(hm.resize_rgb8(img, (50, 50, 6, 6), 3, 3), torch.zeros(3, 3, 3, dtype=torch.uint8))  # wholly outside


def test_resize_rgb8_argument_rules():
    img = noise8(1, 6, 6)
    with pytest.raises(ValueError):
        hm.resize_rgb8(img, None, 4, 4, scale=(3, 1))  # cell 3 starts at 9 of 6
    with pytest.raises(ValueError):
        hm.resize_rgb8(img.float(), None, 3, 3)
    with pytest.raises(ValueError):
        hm.resize_rgb8(img, (0, 0, 0, 3), 3, 3)


def test_model_input_is_the_reference_expression():
    q = torch.arange(256, dtype=torch.uint8).reshape(16, 16, 1).repeat(1, 1, 3)
    want = (q.numpy().astype(np.float32) / 127.5) - 1.0  # CustomTransform, in numpy as the reference runs it
    got = hm.rgb8_to_model_input(q)
    assert tuple(got.shape) == (1, 3, 16, 16) and got.dtype == torch.float32
    assert np.array_equal(got[0].permute(1, 2, 0).numpy(), want)


def test_process_img_front_hook_returns_the_rect():
    """With `front`, process_img reads the shape only and returns the crop window; without a detector that is the centre
    square, which is also the bbox it returns today."""
    img = torch.rand(720, 800, 3)
    crop, bbox = hm.process_img(img, 64)
    calls = []

    def front(view_h):  # asked for only when a detector is installed
        calls.append(view_h)
        return torch.zeros(view_h, 400, 3, dtype=torch.uint8)

    rect, bbox2 = hm.process_img(torch.empty(720, 800, 3, device="meta"), 64, front=front)
    assert rect == bbox2 == bbox == (40, 0, 720, 720) and calls in ([], [360])
    # 360 px or less: the cubic route, `front` is ignored and the host crop comes back
    small = torch.rand(200, 200, 3)
    a, _ = hm.process_img(small, 64, front=lambda vh: 1 / 0)
    b, _ = hm.process_img(small, 64)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# the C boundary
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    sig = pkg.native._SIGNATURES
    for name in ("float_img_front_work_bytes", "float_img_front"):
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in sig and len(sig[name][1]) == n_args, (name, n_args)
    assert "float_img_front_len" not in sig  # two functions: the output size is the caller's
    for const in ("FLOAT_IMG_RGBA_DISCARD = 0", "FLOAT_IMG_RGBA_BLEND = 1", "FLOAT_IMG_RGBA_REPLACE = 2", "FLOAT_IMG_OUT_NCHW_PM1 = 0",
                  "FLOAT_IMG_OUT_HWC_U8 = 1"):
        assert const in hdr
    N = pkg.native
    assert N.IMG_RGBA_MODES == {"discard_alpha": 0, "blend_with_color": 1, "replace_with_color": 2}
    assert (N.IMG_OUT_NCHW_PM1, N.IMG_OUT_HWC_U8) == (0, 1)
    assert sig["float_img_front_work_bytes"][0] is C.c_size_t and sig["float_img_front"][0] is C.c_int


def test_argument_validation_needs_no_gpu():
    """Every rule is checked before any HIP call: status 1 and a message naming the function and the argument."""
    L = pkg.native.lib()
    assert L.float_img_front_work_bytes(2160, 3840, 512, 512) == 2160 * 512 * 12
    assert L.float_img_front_work_bytes(0, 8, 8, 8) == 0 and L.float_img_front_work_bytes(8, 8, 8, 4097) == 0
    assert L.float_img_front_work_bytes(16385, 8, 8, 8) == 0
    buf = (C.c_float * 1024)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)  # never dereferenced: every call below fails validation

    def call(src=(8, 8), ch=3, rect=(0, 0, 8, 8), scale=(0, 0), mode=0, bkg=(0, 0, 0), out_mode=1, dst=(4, 4), work_bytes=1 << 20,
             img=p, out=p, work=p):
        rc = L.float_img_front(img, src[0], src[1], ch, rect[0], rect[1], rect[2], rect[3], scale[0], scale[1], mode, bkg[0], bkg[1],
                               bkg[2], out_mode, out, dst[0], dst[1], work, work_bytes, None)
        return rc, L.float_last_error().decode()

    for kw, word in ((dict(img=None), "null"), (dict(ch=2), "channels"), (dict(src=(0, 8)), "source sides"),
                     (dict(src=(8, 16385)), "source sides"), (dict(dst=(4, 4097)), "destination sides"), (dict(dst=(0, 4)), "destination sides"),
                     (dict(rect=(0, 0, 0, 8)), "window extents"), (dict(scale=(3, 0)), "scale_num"), (dict(scale=(0, 2)), "scale_num"),
                     (dict(scale=(3, 1)), "starts outside the window"), (dict(mode=3), "rgba_mode"), (dict(bkg=(0, 256, 0)), "background"),
                     (dict(out_mode=2), "out_mode"), (dict(work_bytes=8 * 4 * 12 - 1), "work_bytes"),
                     (dict(ch=4, img=C.c_void_p(p.value + 4)), "aligned"), (dict(out_mode=0, out=C.c_void_p(p.value + 2)), "aligned"),
                     (dict(work=C.c_void_p(p.value + 2)), "aligned")):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("float_img_front:") and word in msg, (kw, rc, msg)
