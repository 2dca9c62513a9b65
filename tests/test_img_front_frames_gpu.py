"""float_img_front_frames on the GPU: one call over block + 1 = 17 frames of 97 x 131 with a different window on every frame,
bitwise against the definition on the CPU, host_models.resize_rgb8(host_models.image_to_rgb8(frame), rect, dst_h, dst_w), against
the single-frame call and against float_img_front.  Integers from the quantiser on: no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm = pkg.host_models
pytestmark = pytest.mark.gpu

T, H, W = 17, 97, 131
BKG = "#3fa07c"
GUARD = 256
# (12, 12): the 96-px window at 8 : 1; (45, 61): a detector view; (33, 65): one row and one column more than a 32 x 64 tile
DSTS = [(12, 12), (16, 16), (45, 61), (33, 65)]
KINDS = [("f32", 3), ("f32", 4), ("u8", 3), ("u8", 4)]


def rects(dst_h, dst_w):
    return [(20, 10, 80, 60), (-15, 10, 60, 60), (30, -20, 50, 50), (100, 20, 60, 50), (40, 70, 50, 50),  # inside; over each edge
            (200, 300, 40, 40), (7, 5, dst_w, dst_h), (50, 40, 9, 9), (11, 13, 37, 37), (3, 0, 96, 96),  # outside, 1 : 1, up, 37, 8 : 1 at 12 px
            (0, 0, W, H), (-10, -10, 160, 120), (60, 30, 33, 17), (0, 0, 1, 1), (-40, 90, 100, 30), (130, 96, 5, 5),
            (3, 0, 128, 128)]  # 8 : 1 at 16 px, over the bottom edge


@functools.lru_cache(maxsize=None)
def frames(kind, ch):
    """seeded frames, shared and never modified: fp32 noise in [-0.1, 1.1] or bytes; alpha 0 and 1 in a tenth of the pixels each"""
    rs = np.random.RandomState(ch)
    u = rs.uniform(size=(T, H, W))
    if kind == "f32":
        x = rs.uniform(-0.1, 1.1, size=(T, H, W, ch)).astype(np.float32)
        lo, hi = 0.0, 1.0
    else:
        x = rs.randint(0, 256, size=(T, H, W, ch)).astype(np.uint8)
        lo, hi = 0, 255
    if ch == 4:
        x[..., 3][u < 0.1] = lo
        x[..., 3][u > 0.9] = hi
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def rgb8(kind, ch, t):
    return hm.image_to_rgb8(frames(kind, ch)[t], "blend_with_color", hm.hex_to_rgb8(BKG))


def call(x, rr, dst):
    """front_frames_device into a guarded buffer; the output on the host, bands checked"""
    n = x.shape[0] * dst[0] * dst[1] * 3
    big = torch.full((n + 2 * GUARD,), 77, dtype=torch.uint8, device="cuda:0")
    out = big[GUARD:GUARD + n].view(x.shape[0], dst[0], dst[1], 3)
    assert pkg.image.front_frames_device(x, rr, dst[0], dst[1], "blend_with_color", BKG, out=out) is out
    big = big.cpu()
    assert bool((big[:GUARD] == 77).all()) and bool((big[GUARD + n:] == 77).all()), "guard band of out written"
    return big[GUARD:GUARD + n].view(x.shape[0], dst[0], dst[1], 3)


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("kind,ch", KINDS)
def test_stack_equals_the_definition(kind, ch, dst):
    rr = rects(*dst)
    got = call(frames(kind, ch).cuda(), rr, dst)
    for t in range(T):
        want = hm.resize_rgb8(rgb8(kind, ch, t), rr[t], dst[0], dst[1])
        bad = int((got[t] != want).sum())
        print("%s x%d -> %s frame %d rect %s: %d bytes differ" % (kind, ch, dst, t, rr[t], bad))
        assert bad == 0, (t, rr[t])
    assert int(got[5].max()) == 0 and int(got[0].max()) > 0  # the window that misses the image is black


@pytest.mark.parametrize("kind,ch", KINDS)
def test_frame_alone_and_the_single_image_front_end(kind, ch):
    dst, rr, x = (45, 61), rects(45, 61), frames(kind, ch).cuda()
    got = call(x, rr, dst)
    assert torch.equal(call(x, rr, dst), got)  # two calls give equal bytes
    for t in range(T):
        assert torch.equal(call(x[t:t + 1], rr[t:t + 1], dst)[0], got[t]), t  # 8-bit RGB: an unaligned frame pointer
        if kind == "f32":
            assert torch.equal(pkg.image.image_front_device(x[t], dst[0], dst[1], rr[t], None, "blend_with_color", BKG, True).cpu(), got[t]), t


def test_views_equal_the_single_image_views():
    x = frames("f32", 4)[:3].cuda()
    got = pkg.image.detector_views_device(x, 36, "blend_with_color", BKG)
    assert tuple(got.shape) == (3, 36, 49, 3)
    for t in range(3):
        assert torch.equal(got[t], pkg.image.detector_view_device(x[t], 36, "blend_with_color", BKG))


def test_invalid_rect_names_the_frame_and_launches_nothing():
    x = frames("u8", 3).cuda()
    rr = rects(16, 16)
    rr[3] = (5, 5, 0, 9)
    out = torch.full((T, 16, 16, 3), 77, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="frame 3"):
        pkg.image.front_frames_device(x, rr, 16, 16, out=out)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
