"""host_models.paste_rgb8, the definition `float_img_paste` is held to: the generated frames resized into the box by the rule of
the image front end, a feather weight on the box's open sides, an integer blend.  Held here to a per-sample evaluation in exact
rationals (fractions.Fraction) that shares no code with it, and to the identities the form was chosen for.  CPU only; every
comparison is exact."""
import functools
import math
from fractions import Fraction

import pytest
import torch

from tests.util import load_pkg

hm = load_pkg().host_models


@functools.lru_cache(maxsize=None)
def noise(seed, *shape):
    """seeded uint8 noise; computed once, shared, never modified"""
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------------
# the rule, sample by sample, in exact rationals
# ---------------------------------------------------------------------------------------------------------------------------
def _round_half_even(q):
    fl = math.floor(q)
    r = q - fl
    return fl + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl % 2 == 1) else 0)


def _axis_weights(n, dst, d, linear):
    """{sample: weight} of destination index d on an axis of n samples resized to dst; the weights sum to 1"""
    s = Fraction(n, dst)  # samples per destination cell
    if linear:
        sx = math.floor(d * s)
        fx = (d + 1) - (sx + 1) / s  # cv2's INTER_AREA magnification taps
        fx = Fraction(0) if fx <= 0 else fx - math.floor(fx)
        if sx >= n - 1:
            sx, fx = n - 1, Fraction(0)
        w = {sx: 1 - fx}
        s1 = min(sx + 1, n - 1)
        w[s1] = w.get(s1, 0) + fx
        return w
    lo, hi = d * s, min((d + 1) * s, Fraction(n))
    return {i: (min(Fraction(i + 1), hi) - max(Fraction(i), lo)) / (hi - lo) for i in range(math.floor(lo), math.ceil(hi))}


def face_sample(frame, h, w, v, u, c):
    fh, fw = frame.shape[0], frame.shape[1]
    linear = fw < w or fh < h
    wy, wx = _axis_weights(fh, h, v, linear), _axis_weights(fw, w, u, linear)
    return _round_half_even(sum(Fraction(int(frame[i, j, c])) * a * b for i, a in wy.items() for j, b in wx.items()))


def alpha_sample(H, W, rect, feather, v, u):
    x0, y0, w, h = rect
    sides = []
    if x0 > 0:
        sides.append(u)
    if x0 + w < W:
        sides.append(w - 1 - u)
    if y0 > 0:
        sides.append(v)
    if y0 + h < H:
        sides.append(h - 1 - v)
    if not sides or feather == 0:
        return 255
    return min(255, math.floor(Fraction(255 * (min(sides) + 1), feather + 1)))


def paste_by_samples(src, frames, rect, feather):
    H, W = src.shape[0], src.shape[1]
    x0, y0, w, h = rect
    out = src[None].repeat(frames.shape[0], 1, 1, 1).clone()
    for t in range(frames.shape[0]):
        for y in range(max(0, y0), min(H, y0 + h)):
            for x in range(max(0, x0), min(W, x0 + w)):
                a = alpha_sample(H, W, rect, feather, y - y0, x - x0)
                for c in range(3):
                    f = face_sample(frames[t], h, w, y - y0, x - x0, c)
                    q = Fraction(a * f + (255 - a) * int(src[y, x, c]), 255)
                    assert (q - math.floor(q)) != Fraction(1, 2)  # 255 is odd: no ties
                    out[t, y, x, c] = math.floor(q + Fraction(1, 2))
    return out


# name -> (source (H, W), frame (h, w), rect, feather): boxes of at most 12 x 12
CASES = {
    "shrink_all_open": ((20, 18), (16, 16), (3, 4, 7, 7), 1),
    "shrink_fractional": ((20, 18), (16, 16), (2, 2, 11, 9), 5),
    "enlarge_all_open": ((20, 18), (5, 6), (3, 4, 12, 11), 1),
    "mixed_axes": ((20, 18), (16, 4), (3, 4, 12, 5), 0),           # x enlarges, y shrinks: the linear rule on both
    "scale_one": ((20, 18), (8, 8), (5, 6, 8, 8), 5),
    "left_closed": ((20, 18), (16, 16), (0, 4, 7, 7), 5),
    "right_closed": ((20, 18), (16, 16), (11, 4, 7, 7), 5),
    "top_closed": ((20, 18), (16, 16), (3, 0, 7, 7), 1),
    "bottom_closed": ((20, 18), (16, 16), (3, 13, 7, 7), 5),
    "beyond_left_and_top": ((20, 18), (16, 16), (-3, -5, 9, 9), 5),
    "beyond_right_and_bottom": ((20, 18), (16, 16), (12, 14, 10, 10), 1),
    "whole_image": ((10, 12), (16, 16), (0, 0, 12, 10), 5),
    "beyond_all_four": ((8, 9), (16, 16), (-1, -2, 12, 12), 5),
    "feather_larger_than_box": ((20, 18), (16, 16), (3, 4, 7, 7), 40),
    "feather_zero": ((20, 18), (16, 16), (3, 4, 7, 7), 0),
    "one_cell": ((20, 18), (16, 16), (9, 9, 1, 1), 5),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_paste_rgb8_equals_the_rule_in_exact_rationals(case):
    (H, W), (fh, fw), rect, feather = CASES[case]
    src, frames = noise(1, H, W, 3), noise(2, 2, fh, fw, 3)
    got = hm.paste_rgb8(src, frames, rect, feather)
    want = paste_by_samples(src, frames, rect, feather)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, H, W, 3)
    assert torch.equal(got, want), "%s: %d bytes differ" % (case, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------------
# the identities the form was chosen for
# ---------------------------------------------------------------------------------------------------------------------------
def test_box_of_the_frames_own_size_over_a_source_of_that_size_returns_the_frames():
    frames = noise(3, 3, 64, 64, 3)
    for feather in (0, 9):
        assert torch.equal(hm.paste_rgb8(noise(4, 64, 64, 3), frames, (0, 0, 64, 64), feather), frames)


def test_whole_image_is_a_plain_resize_for_any_feather():
    src, frames = noise(5, 90, 67, 3), noise(6, 2, 64, 64, 3)
    for feather in (0, 1, 9, 1000):
        got = hm.paste_rgb8(src, frames, (0, 0, 67, 90), feather)
        for t in range(2):
            assert torch.equal(got[t], hm.resize_rgb8(frames[t], None, 90, 67))


def test_box_outside_the_image_returns_the_source():
    src, frames = noise(5, 90, 67, 3), noise(6, 2, 64, 64, 3)
    for rect in ((200, 0, 5, 5), (-5, 0, 5, 5), (0, -9, 5, 9), (0, 90, 5, 5), (67, 3, 40, 40)):
        assert torch.equal(hm.paste_rgb8(src, frames, rect, 3), src[None].expand(2, -1, -1, -1)), rect


def test_one_by_one_box_changes_one_pixel():
    src = noise(5, 90, 67, 3)
    frames = (255 - src[40, 30])[None, None, None].expand(1, 64, 64, 3).contiguous()  # constant, and no channel equals the source's
    for feather in (0, 3):  # d = 0 on every side: alpha 255 // (feather + 1)
        got = hm.paste_rgb8(src, frames, (30, 40, 1, 1), feather)
        changed = (got[0] != src).any(-1)
        assert int(changed.sum()) == 1 and bool(changed[40, 30])
    assert torch.equal(hm.paste_rgb8(src, frames, (30, 40, 1, 1), 0)[0, 40, 30], frames[0, 0, 0])  # the mean of a constant frame


def test_blending_equal_values_is_exact_for_every_alpha():
    a = torch.arange(256)[:, None]
    x = torch.arange(256)[None, :]
    assert bool((((a * x + (255 - a) * x + 127) // 255) == x).all())
    same = noise(7, 30, 30, 3)
    frames = same[5:25, 5:25][None].contiguous()  # scale 1: the face equals the source under it
    assert torch.equal(hm.paste_rgb8(same, frames, (5, 5, 20, 20), 7)[0], same)


# ---------------------------------------------------------------------------------------------------------------------------
# the feather weight
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feather", [1, 5, 7, 100])
def test_alpha_is_non_decreasing_towards_the_centre_and_full_at_d_equal_feather(feather):
    a = hm.paste_alpha(200, 200, (20, 30, 37, 37), feather)
    assert tuple(a.shape) == (37, 37) and int(a.min()) >= 0 and int(a.max()) <= 255
    c = 18
    for line in (a[c, :c + 1], a[c, c:].flip(0), a[:c + 1, c], a[c:, c].flip(0)):  # from a side to the centre
        assert bool((line[1:] >= line[:-1]).all())
    d = torch.minimum(torch.minimum(torch.arange(37)[:, None], 36 - torch.arange(37)[:, None]),
                      torch.minimum(torch.arange(37)[None, :], 36 - torch.arange(37)[None, :]))
    assert bool((a[d >= feather] == 255).all())
    if feather <= 18:
        assert int(a[feather, c]) == 255 and int(a[feather - 1, c]) < 255  # reached at d = feather, not before
    assert int(a[0, c]) == 255 // (feather + 1)


def test_a_closed_side_leaves_the_full_value_at_the_images_edge():
    a = hm.paste_alpha(100, 100, (0, 30, 37, 37), 7)  # the left side lies on the image's edge
    assert bool((a[18, :19] == 255).all()) and int(a[18, 36]) < 255 and int(a[0, 18]) < 255
    a = hm.paste_alpha(100, 100, (-5, 30, 37, 37), 7)  # beyond it
    assert bool((a[18, :19] == 255).all())
    a = hm.paste_alpha(67, 37, (0, 30, 37, 37), 7)  # left and right closed, bottom on the edge: only the top feathers
    assert bool((a[36] == 255).all()) and bool((a[0] == 255 // 8).all())
    assert bool((hm.paste_alpha(37, 37, (0, 0, 37, 37), 7) == 255).all())
    assert bool((hm.paste_alpha(100, 100, (20, 30, 37, 37), 0) == 255).all())


def test_default_feather_is_a_sixteenth_of_the_box_width():
    assert hm.default_feather((3, 4, 160, 99)) == 10 and hm.default_feather((0, 0, 15, 15)) == 0


def test_bad_shapes_and_dtypes_raise():
    src, frames = noise(5, 90, 67, 3), noise(6, 2, 64, 64, 3)
    bad = [(src.float(), frames, (0, 0, 5, 5), 0), (src, frames.float(), (0, 0, 5, 5), 0), (src[..., :2], frames, (0, 0, 5, 5), 0),
           (src, frames[0], (0, 0, 5, 5), 0), (src[None], frames, (0, 0, 5, 5), 0), (src, frames[:0], (0, 0, 5, 5), 0),
           (src, frames, (0, 0, 0, 5), 0), (src, frames, (0, 0, 5, -1), 0), (src, frames, (0, 0, 5), 0), (src, frames, (0, 0, 5, 5), -1)]
    for args in bad:
        with pytest.raises(ValueError):
            hm.paste_rgb8(*args)
