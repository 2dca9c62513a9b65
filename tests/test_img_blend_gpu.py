"""float_img_blend on the GPU through image.paste_frames_device(..., blend="multiband"): the multi-band paste.  The kernels work in
integers, so every comparison is torch.equal with the definition on the CPU, host_models.paste_multiband_rgb8 (tests/test_img_blend.py
pins its properties) - no tolerance anywhere in this file.

Crops are T = 3 different 64 x 64 frames of seeded noise, halved and raised by 100 so that face and portrait differ in the mean and
every pyramid level carries something.  The up kernel's tile is 16 x 64 cells of the frame, the down kernel's 16 x 32 cells of the
coarser level; the cases are the smallest at which tiling, clamping or the odd halving can go wrong."""
import functools

import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm = pkg.host_models
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def portrait(H, W):
    return torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))


@functools.lru_cache(maxsize=None)
def crops():
    return torch.randint(0, 256, (3, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)) // 2 + 100


# name -> (portrait (H, W), rect (x0, y0, w, h), inset, levels, resample)
CASES = {
    "window_1x1_levels_1": ((5, 7), (3, 2, 1, 1), 0, 1, None),                   # clamping only
    "window_1x1_levels_3": ((5, 7), (3, 2, 1, 1), 0, 3, None),
    "window_5x3_levels_1": ((6, 9), (1, 1, 5, 3), 1, 1, None),
    "window_5x3_levels_3": ((6, 9), (1, 1, 5, 3), 1, 3, None),
    "window_33x31_odd_halvings": ((40, 41), (4, 2, 33, 31), 6, 5, None),          # 33 17 9 5 3 2 by 31 16 8 4 2 1
    "one_past_a_tile": ((52, 132), (64, 16, 65, 33), 8, 2, None),                 # 65 x 33 on a tile's corner; level 1 is 33 x 17
    "tiles_3x2_ragged_odd_origin": ((40, 172), (7, 5, 150, 30), 9, 3, "lanczos"),  # dword stores, odd win_x
    "clipped_left_and_top": ((50, 60), (-10, -8, 40, 36), 6, 2, None),            # closed sides, win_x = 0
    "outside_on_all_sides": ((30, 44), (-5, -6, 60, 50), 8, 1, None),             # no open side: the face itself
    "byte_stores_odd_origin": ((37, 67), (11, 5, 40, 25), 4, 2, None),            # W % 4 = 3
    "default_inset_and_levels": ((70, 100), (10, 8, 80, 56), None, None, None),   # inset 5, one level
}


@pytest.mark.parametrize("name", CASES)
def test_blend_is_the_definition(name):
    hw, rect, inset, levels, resample = CASES[name]
    src, frames = portrait(*hw), crops()
    want = hm.paste_multiband_rgb8(src, frames, rect, inset, levels, resample)
    kw = dict(blend="multiband", inset=inset, levels=levels, resample=resample)
    got = pkg.image.paste_frames_device(src.cuda(), frames.cuda(), rect, **kw).cpu()
    bad = int((got != want).sum())
    print("%s: %d of %d bytes differ from the definition" % (name, bad, want.numel()))
    assert torch.equal(got, want)
    assert torch.equal(pkg.image.paste_frames_device(src.cuda(), frames.cuda(), rect, **kw).cpu(), got)  # two calls, equal bytes
    order = [2, 0, 1]  # no frame depends on its neighbours
    assert torch.equal(pkg.image.paste_frames_device(src.cuda(), frames[order].cuda(), rect, **kw).cpu(), want[order])
    if name == "outside_on_all_sides":
        assert torch.equal(got, hm.paste_rgb8(src, frames, rect, 0))


def test_default_route_is_untouched():
    src, frames, rect = portrait(40, 172), crops(), (7, 5, 150, 30)
    got = pkg.image.paste_frames_device(src.cuda(), frames.cuda(), rect, 9).cpu()
    assert torch.equal(got, hm.paste_rgb8(src, frames, rect, 9))
    with pytest.raises(ValueError, match="feather"):
        pkg.image.paste_frames_device(src.cuda(), frames.cuda(), rect, 9, blend="multiband")
