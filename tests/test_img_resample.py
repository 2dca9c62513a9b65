"""host_models.resample_coeffs / resample_rgb8, the definition `float_img_resample` is held to, and the `resample=` form of paste_rgb8 /
paste_i420.  The outside witness is Pillow's Image.resize, deterministic fixed-point arithmetic for 8-bit images: every comparison
here is exact.  Pillow 12.2.0 is the version the definition was written against (src/libImaging/Resample.c: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc).  The planner of the library (float_img_resample_plan) is host
code: it is loaded and called here without a GPU.  CPU only."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from tests.util import load_pkg

pkg = load_pkg()
hm = pkg.host_models

FILTERS = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
# (source (w, h), destination (w, h))
SIZE_PAIRS = [((64, 64), (97, 97)), ((64, 64), (128, 131)), ((7, 5), (16, 33)), ((1, 1), (9, 4)), ((64, 48), (41, 29)),
              ((512, 512), (640, 640)), ((33, 64), (33, 100)), ((64, 64), (3, 1)), ((16, 16), (255, 17)), ((50, 50), (50, 50))]
KINDS = ("noise", "smooth", "binary")


@functools.lru_cache(maxsize=None)
def picture(kind, w, h):
    """(h, w, 3) uint8, seeded; computed once, shared, never modified"""
    g = torch.Generator().manual_seed({"noise": 11, "smooth": 12, "binary": 13}[kind] * 100003 + 17 * w + h)
    if kind == "noise":
        return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g)
    if kind == "binary":
        return (torch.randint(0, 2, (h, w, 3), generator=g) * 255).to(torch.uint8)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    ph = torch.rand(3, generator=g, dtype=torch.float64) * 6.28
    f = torch.stack([3.0 * torch.sin(0.11 * x + 0.07 * y + ph[c]) for c in range(3)], dim=-1)  # a smooth field of +-3 levels
    return (128 + f.round()).to(torch.uint8)


def pillow(img, w, h, filter):
    return torch.from_numpy(np.asarray(Image.fromarray(img.numpy()).resize((w, h), FILTERS[filter])).copy())


def beyond_limit(n_in, n_out, filter):
    try:
        hm.resample_ksize(n_in, n_out, filter)
        return False
    except ValueError:
        return True


def resample_unlimited(img, h, w, filter):
    """resample_rgb8's two passes from the same private pieces, at any number of taps"""
    fid = hm.RESAMPLE_FILTERS[filter]
    x = img[None].to(torch.int64)
    if w != img.shape[1]:
        x = hm._resample_axis(x, 2, hm._resample_table(int(img.shape[1]), w, fid, 0, w))
    if h != img.shape[0]:
        x = hm._resample_axis(x, 1, hm._resample_table(int(img.shape[0]), h, fid, 0, h))
    return x[0].to(torch.uint8)


@pytest.mark.parametrize("filter", sorted(FILTERS))
@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=lambda p: "%dx%d_to_%dx%d" % (p[0] + p[1]))
def test_resample_rgb8_is_pillow_bit_for_bit(pair, filter):
    """All ten size pairs, three image kinds each.  One pair, 64 x 64 -> 3 x 1, shrinks its rows 64-fold: 257 (bicubic) and 385
    (Lanczos) taps per sample, beyond the stated limit of 255.  There the public call must refuse, and the rule itself - the same
    private table and pass functions resample_rgb8 is made of, without the limit - is still held to Pillow, so no pair goes unchecked."""
    (sw, sh), (dw, dh) = pair
    over = beyond_limit(sh, dh, filter) or beyond_limit(sw, dw, filter)
    assert over == (pair == ((64, 64), (3, 1)))
    for kind in KINDS:
        img = picture(kind, sw, sh)
        want = pillow(img, dw, dh, filter)
        if over:
            with pytest.raises(ValueError):
                hm.resample_rgb8(img[None], dh, dw, filter)
            got = resample_unlimited(img, dh, dw, filter)
        else:
            got = hm.resample_rgb8(img[None], dh, dw, filter)[0]
        assert got.dtype == torch.uint8 and tuple(got.shape) == (dh, dw, 3)
        assert torch.equal(got, want), (pair, filter, kind, int((got != want).sum()))


def test_several_frames_are_resampled_one_by_one():
    frames = torch.stack([picture("noise", 64, 48), picture("binary", 64, 48)])
    got = hm.resample_rgb8(frames, 29, 41, "lanczos")
    assert torch.equal(got[0], pillow(frames[0], 41, 29, "lanczos")) and torch.equal(got[1], pillow(frames[1], 41, 29, "lanczos"))


@pytest.mark.parametrize("filter", sorted(FILTERS))
def test_a_window_is_the_slice_of_the_whole(filter):
    for (sw, sh), (dw, dh), win in ((((64, 64), (97, 97), (0, 0, 40, 31))), ((64, 64), (97, 97), (60, 70, 37, 27)), ((64, 48), (41, 29), (5, 3, 30, 20)),
                                    ((33, 64), (33, 100), (4, 50, 20, 50)), ((64, 33), (100, 33), (50, 4, 50, 20)), ((50, 50), (50, 50), (3, 4, 40, 41)),
                                    ((7, 5), (16, 33), (15, 32, 1, 1))):
        frames = torch.stack([picture("noise", sw, sh), picture("smooth", sw, sh)])
        whole = hm.resample_rgb8(frames, dh, dw, filter)
        xa, ya, wc, hc = win
        part = hm.resample_rgb8(frames, dh, dw, filter, win)
        assert tuple(part.shape) == (2, hc, wc, 3) and torch.equal(part, whole[:, ya:ya + hc, xa:xa + wc]), (sw, sh, dw, dh, win)
    # a box far larger than anything that could be formed: only the window exists
    big = 1 << 30
    part = hm.resample_rgb8(picture("noise", 64, 64)[None], big, big, filter, (big // 2 - 3, big - 5, 6, 5))
    assert tuple(part.shape) == (1, 5, 6, 3)
    for bad in ((-1, 0, 5, 5), (0, 0, 98, 5), (0, 93, 5, 5), (0, 0, 0, 5), (0, 0, 5)):
        with pytest.raises(ValueError):
            hm.resample_rgb8(picture("noise", 64, 64)[None], 97, 97, filter, bad)


def as_table(coeffs):
    xmin, n, k = coeffs
    return torch.cat([xmin[:, None], n[:, None], k], dim=1).to(torch.int32)


@pytest.mark.parametrize("filter", sorted(FILTERS))
def test_planner_of_the_library_equals_resample_coeffs(filter):
    """float_img_resample_plan (C double, libm's sin) against resample_coeffs (Python floats, math.sin), integer for integer: every
    axis of the ten size pairs, and a window of a box of side 2^30.  The definition itself is held to Pillow 12.2.0 above."""
    axes = sorted({(s[i], d[i]) for s, d in SIZE_PAIRS for i in (0, 1)})
    for n_in, n_out in axes:
        if beyond_limit(n_in, n_out, filter):
            with pytest.raises(ValueError):
                pkg.image.resample_table(n_in, n_out, filter)
            continue
        got = pkg.image.resample_table(n_in, n_out, filter)
        want = as_table(hm.resample_coeffs(n_in, n_out, filter))
        assert got.dtype == torch.int32 and got.shape == want.shape and torch.equal(got, want), (n_in, n_out)
        assert int(got[:, 1].max()) <= got.shape[1] - 2 and bool((got[:, 0] + got[:, 1] <= n_in).all()) and bool((got[:, 0] >= 0).all())
    big = 1 << 30
    for first, count in ((0, 33), (big // 2 - 16, 40), (big - 40, 40), (123456789, 7)):
        got = pkg.image.resample_table(64, big, filter, first, count)
        assert torch.equal(got, as_table(hm.resample_coeffs(64, big, filter, first, count))), (first, count)
    got = pkg.image.resample_table(512, 640, filter, 100, 50)
    assert torch.equal(got, as_table(hm.resample_coeffs(512, 640, filter))[100:150])


def test_planner_refusals_need_no_gpu():
    L = pkg.native.lib()
    buf = (C.c_int32 * 4096)()

    def plan(n_in=64, n_out=97, filter=0, first=0, count=8, table=buf, ints=4096):
        rc = L.float_img_resample_plan(n_in, n_out, filter, first, count, table, ints)
        return rc, L.float_last_error().decode("utf-8", "replace") if rc else ""

    assert plan() == (0, "")
    assert L.float_img_resample_plan_ints(64, 97, 0, 8) == 8 * 7 and L.float_img_resample_plan_ints(64, 97, 1, 8) == 8 * 9
    assert L.float_img_resample_plan_ints(64, 32, 1, 32) == 32 * 15
    for kw, word in ((dict(filter=2), "filter"), (dict(filter=-1), "filter"), (dict(n_in=0), "n_in"), (dict(n_out=0), "n_out"),
                     (dict(n_in=64, n_out=1), "ksize"), (dict(n_in=4300, n_out=100, filter=1), "ksize"), (dict(first=-1), "first"),
                     (dict(first=90, count=8), "count"), (dict(count=0), "count"), (dict(table=None), "null"), (dict(ints=8 * 7 - 1), "table_ints")):
        rc, msg = plan(**kw)
        assert rc == 1 and "float_img_resample_plan" in msg and word in msg, (kw, rc, msg)
    for args in ((0, 97, 0, 8), (64, 0, 0, 8), (64, 97, 2, 8), (64, 1, 0, 1), (64, 97, 0, 0), (64, 97, 0, 98)):
        assert L.float_img_resample_plan_ints(*args) == 0, args
    # 4200 -> 100 with Lanczos is 42 x: ksize 253, inside; the call that sizes the device scratch refuses the same things
    assert L.float_img_resample_plan_ints(4200, 100, 1, 100) == 100 * 255
    assert L.float_img_resample_work_bytes(3, 64, 64, 97, 97, 0, 0, 0, 97, 97) >= 3 * 64 * 300
    for args in ((0, 64, 64, 97, 97, 0, 0, 0, 97, 97), (3, 64, 64, 97, 97, 2, 0, 0, 97, 97), (3, 64, 64, 97, 97, 0, 1, 0, 97, 97),
                 (3, 64, 64, 1, 97, 0, 0, 0, 97, 1), (3, 0, 64, 97, 97, 0, 0, 0, 97, 97), (3, 64, 64, 97, 97, 0, 0, 0, 0, 97)):
        assert L.float_img_resample_work_bytes(*args) == 0, args


def test_refusals_of_the_definition():
    img = picture("noise", 64, 64)[None]
    for call in (lambda: hm.resample_rgb8(img, 97, 97, "nearest"), lambda: hm.resample_rgb8(img, 97, 97, None),
                 lambda: hm.resample_rgb8(img, 97, 97, 1), lambda: hm.resample_coeffs(64, 97, "cubic"),
                 lambda: hm.resample_rgb8(img, 1, 97, "bicubic"),            # 64 -> 1: 257 taps
                 lambda: hm.resample_coeffs(4300, 100, "lanczos"),           # 43 x: 259 taps
                 lambda: hm.resample_rgb8(img, 0, 97, "bicubic"), lambda: hm.resample_rgb8(img, 97, 0, "lanczos"),
                 lambda: hm.resample_coeffs(0, 5, "bicubic"), lambda: hm.resample_coeffs(5, 0, "bicubic"),
                 lambda: hm.resample_coeffs(64, 97, "bicubic", 90, 8), lambda: hm.resample_coeffs(64, 97, "bicubic", -1, 8),
                 lambda: hm.resample_rgb8(img[0], 97, 97, "bicubic"), lambda: hm.resample_rgb8(img.float(), 97, 97, "bicubic")):
        with pytest.raises(ValueError):
            call()
    assert hm.resample_ksize(4200, 100, "lanczos") == 253 and hm.resample_ksize(64, 97, "bicubic") == 5
    xmin, n, k = hm.resample_coeffs(64, 97, "lanczos")
    assert tuple(k.shape) == (97, 7) and int(n.max()) <= 7 and bool((k.sum(dim=1) - (1 << 22)).abs().max() <= 7)  # rows sum to one, to rounding


# ---------------------------------------------------------------------------------------------------------------------------
# the paste with resample=
# ---------------------------------------------------------------------------------------------------------------------------
SRC_HW = (96, 128)  # the portrait: 96 rows, 128 columns
# name -> rect (x0, y0, w, h) of the box over it; crops are 3 frames of 64 x 64
RECTS = {
    "inside": (20, 10, 75, 70),
    "flush_left_top": (0, 0, 80, 70),
    "flush_right_bottom": (58, 19, 70, 77),
    "beyond_left": (-13, 10, 75, 70),
    "beyond_right": (70, 10, 75, 70),
    "beyond_top": (20, -9, 75, 70),
    "beyond_bottom": (20, 40, 75, 70),
    "larger_than_the_portrait": (-20, -30, 170, 150),
    "wholly_outside": (128, 10, 75, 70),
}
FEATHERS = (None, 0, 40)  # 40 is more than half of every box's shorter side but one


@functools.lru_cache(maxsize=None)
def noise(seed, *shape):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def operands():
    return noise(1, *SRC_HW, 3), noise(2, 3, 64, 64, 3)


def feather_of(rect, feather):
    return hm.default_feather(rect) if feather is None else feather


def composed(src, frames, rect, feather, filter):
    """the paste written out: the whole face by resample_rgb8, the whole alpha, the blend, cell by cell of box & image"""
    H, W = src.shape[0], src.shape[1]
    x0, y0, w, h = rect
    out = src[None].repeat(frames.shape[0], 1, 1, 1).clone()
    a = hm.paste_alpha(H, W, rect, feather)
    face = hm.resample_rgb8(frames, h, w, filter).to(torch.int64)
    for y in range(max(0, y0), min(H, y0 + h)):
        for x in range(max(0, x0), min(W, x0 + w)):
            al = int(a[y - y0, x - x0])
            out[:, y, x] = ((al * face[:, y - y0, x - x0] + (255 - al) * src[y, x].to(torch.int64) + 127) // 255).to(torch.uint8)
    return out


@pytest.mark.parametrize("filter", sorted(FILTERS))
@pytest.mark.parametrize("name", sorted(RECTS))
def test_paste_rgb8_with_resample_is_the_composition(name, filter):
    src, frames = operands()
    rect = RECTS[name]
    for feather in FEATHERS:
        f = feather_of(rect, feather)
        got = hm.paste_rgb8(src, frames, rect, f, resample=filter)
        assert torch.equal(got, composed(src, frames, rect, f, filter)), (name, feather)
    if name == "wholly_outside":
        assert torch.equal(got, src[None].expand(3, -1, -1, -1))
    else:
        assert not torch.equal(got, hm.paste_rgb8(src, frames, rect, f))  # another face than the front end's rule gives


@pytest.mark.parametrize("name", sorted(RECTS))
def test_clipped_rect_identity(name):
    """The two facts the device route rests on (image.paste_frames_device): resize_rgb8 at equal sizes is the identity, and the alpha
    of the clipped rect is the slice of the unclipped rect's - so the paste of the box-sized window at the clipped rect with the
    unclipped rect's feather, by the UNCHANGED paste_rgb8, is the paste with resample=."""
    src, frames = operands()
    H, W = SRC_HW
    rect = RECTS[name]
    x0, y0, w, h = rect
    win = pkg.image.paste_window(H, W, rect)
    if name == "wholly_outside":
        assert win is None
        return
    xa, ya, xb, yb = win
    clipped = (xa, ya, xb - xa, yb - ya)
    for hh, ww in ((1, 1), (5, 7), (64, 64), (100, 33), (yb - ya, xb - xa)):
        img = noise(3, hh, ww, 3)
        assert torch.equal(hm.resize_rgb8(img, None, hh, ww), img)
    for feather in FEATHERS:
        f = feather_of(rect, feather)  # of the UNCLIPPED rect
        assert torch.equal(hm.paste_alpha(H, W, clipped, f), hm.paste_alpha(H, W, rect, f)[ya - y0:yb - y0, xa - x0:xb - x0]), (name, feather)
        for filter in sorted(FILTERS):
            window = hm.resample_rgb8(frames, h, w, filter, (xa - x0, ya - y0, xb - xa, yb - ya))
            assert torch.equal(hm.paste_rgb8(src, window, clipped, f), hm.paste_rgb8(src, frames, rect, f, resample=filter)), (name, feather, filter)


@pytest.mark.parametrize("matrix", [None, "bt709-full"])
def test_paste_i420_with_resample_is_the_conversion_of_the_rgb_paste(matrix):
    src, frames = operands()
    for name in ("inside", "beyond_right", "larger_than_the_portrait", "wholly_outside"):
        for filter in sorted(FILTERS):
            got = hm.paste_i420(src, frames, RECTS[name], 5, matrix=matrix, resample=filter)
            assert tuple(got.shape) == (3, 144, 128)
            assert torch.equal(got, hm.rgb8_to_i420(hm.paste_rgb8(src, frames, RECTS[name], 5, resample=filter), matrix)), (name, filter)


def test_resample_none_gives_the_old_outputs():
    """resample=None is the call without the keyword; the rule of that call is pinned sample by sample in tests/test_img_paste.py."""
    src, frames = operands()
    for name in sorted(RECTS):
        rect = RECTS[name]
        x0, y0, w, h = rect
        old = hm.paste_rgb8(src, frames, rect, 5)
        assert torch.equal(hm.paste_rgb8(src, frames, rect, 5, resample=None), old) and torch.equal(hm.paste_rgb8(src, frames, rect, 5, None), old)
        # ... and that call still resizes by the front end's rule
        ya, yb, xa, xb = max(0, y0), min(96, y0 + h), max(0, x0), min(128, x0 + w)
        if yb > ya and xb > xa:
            a = hm.paste_alpha(96, 128, rect, 5)[ya - y0:yb - y0, xa - x0:xb - x0, None]
            face = hm.resize_rgb8(frames[1], None, h, w)[ya - y0:yb - y0, xa - x0:xb - x0].to(torch.int64)
            assert torch.equal(old[1, ya:yb, xa:xb], ((a * face + (255 - a) * src[ya:yb, xa:xb].to(torch.int64) + 127) // 255).to(torch.uint8))
        for matrix in (None, "bt709-full"):
            assert torch.equal(hm.paste_i420(src, frames, rect, 5, matrix, None), hm.paste_i420(src, frames, rect, 5, matrix))
    with pytest.raises(ValueError):
        hm.paste_rgb8(src, frames, RECTS["inside"], 5, resample="linear")
    with pytest.raises(ValueError):
        hm.paste_i420(src, frames, RECTS["inside"], 5, resample="nearest")


def test_python_layers_take_resample_and_default_to_none():
    import importlib
    import inspect
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    A, G = gen.InferenceAgent, pkg.pipeline.FloatHotPath
    for fn in (hm.paste_rgb8, hm.paste_i420, pkg.image.paste_frames_device, G.generate_pasted, G.stream_to_host_pasted, G.generate_to_jpeg,
               G.stream_to_jpeg, G.generate_to_png, G.stream_to_png, A.infer_pasted, A.stream_pasted, A.infer_pasted_jpeg, A.stream_pasted_jpeg,
               A.infer_pasted_png, A.stream_pasted_png, A.write_video, A.write_y4m_matrix, A.write_apng):
        assert inspect.signature(fn).parameters["resample"].default is None, fn
    assert hm.RESAMPLE_FILTERS == {"bicubic": pkg.native.IMG_FILTER_BICUBIC, "lanczos": pkg.native.IMG_FILTER_LANCZOS}
