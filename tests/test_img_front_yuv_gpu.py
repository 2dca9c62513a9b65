"""float_img_front_frames_yuv on the GPU: 17 frames (block + 1) of 98 x 134 YUV 4:2:0 - chroma rows of 67 bytes, so their alignment
changes from row to row - with a different window on every frame, bitwise against the definition on the CPU,
host_models.resize_rgb8(host_models.yuv420_to_rgb8(frame, layout, matrix, chroma), rect, dst_h, dst_w).  Integers throughout: no
tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm, image = pkg.host_models, pkg.image
pytestmark = pytest.mark.gpu

T, H, W = 17, 98, 134
GUARD = 256
DSTS = [(12, 12), (45, 61), (33, 65)]  # 8 : 1 of a 96-px window; a detector view; one row and one column more than a 32 x 64 tile
LAYOUTS, CHROMAS = ("i420", "nv12"), ("nearest", "centre")


def rects(dst_h, dst_w):
    return [(20, 10, 80, 60), (-15, 10, 60, 60), (30, -20, 50, 50), (101, 21, 60, 50), (41, 71, 50, 50),  # inside; over each edge (odd origins)
            (200, 300, 40, 40), (7, 5, dst_w, dst_h), (51, 41, 9, 9), (11, 13, 37, 37), (3, 1, 96, 96),  # outside, 1 : 1, up, 37, 8 : 1 at 12 px
            (0, 0, W, H), (-10, -10, 160, 120), (61, 30, 33, 17), (0, 0, 1, 1), (-40, 91, 100, 30), (133, 97, 5, 5),
            (1, 1, 132, 96)]


@functools.lru_cache(maxsize=None)
def planes(layout, h=H, w=W, t=T):
    """seeded bytes, shared and never modified"""
    return torch.from_numpy(np.random.RandomState(len(layout) + h).randint(0, 256, (t, 3 * h // 2, w)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def rgb8(layout, chroma, matrix, t, h=H, w=W):
    return hm.yuv420_to_rgb8(planes(layout, h, w, 1 if h != H else T)[t], layout, matrix, chroma)


def call(frames, rr, dst):
    """front_frames_device into a guarded buffer; the output on the host, bands checked"""
    n = len(frames) * dst[0] * dst[1] * 3
    big = torch.full((n + 2 * GUARD,), 77, dtype=torch.uint8, device="cuda:0")
    out = big[GUARD:GUARD + n].view(len(frames), dst[0], dst[1], 3)
    assert image.front_frames_device(frames, rr, dst[0], dst[1], out=out) is out
    big = big.cpu()
    assert bool((big[:GUARD] == 77).all()) and bool((big[GUARD + n:] == 77).all()), "guard band of out written"
    return big[GUARD:GUARD + n].view(len(frames), dst[0], dst[1], 3)


@functools.lru_cache(maxsize=None)
def planes_dev(layout):
    return planes(layout).cuda()


def stack(layout, chroma, matrix, t0=0, t1=T):
    """a view of the one device stack: frames of 19698 bytes, so an odd t0 begins, and an odd t1 ends, 2 bytes off a dword"""
    return image.YuvFrames(planes_dev(layout)[t0:t1], H, W, layout, matrix, chroma)


@pytest.mark.parametrize("dst", DSTS)
@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_stack_equals_the_definition(layout, chroma, dst):
    matrix = 2 * ((LAYOUTS.index(layout) * 2 + CHROMAS.index(chroma) + DSTS.index(dst)) % 4)  # the four ids in turn
    rr = rects(*dst)
    got = call(stack(layout, chroma, matrix), rr, dst)
    for t in range(T):
        want = hm.resize_rgb8(rgb8(layout, chroma, matrix, t), rr[t], dst[0], dst[1])
        bad = int((got[t] != want).sum())
        print("%s %s matrix %d -> %s frame %d rect %s: %d bytes differ" % (layout, chroma, matrix, dst, t, rr[t], bad))
        assert bad == 0, (t, rr[t])
    assert int(got[5].max()) == 0 and int(got[0].max()) > 0  # the window that misses the image is black, not converted zeros


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_span_wider_than_a_staging_chunk(layout, chroma):
    """4 x 8200 to 2 x 64: a tile's span is the whole row, four chunks of 2048 and a rest; the second rect begins on an odd column"""
    h, w = 4, 8200
    for rect in ((0, 0, w, h), (1, 1, w - 2, h - 2)):
        frames = image.YuvFrames(planes(layout, h, w, 1).cuda(), h, w, layout, 4, chroma)
        got = call(frames, [rect], (2, 64))
        assert torch.equal(got[0], hm.resize_rgb8(rgb8(layout, chroma, 4, 0, h, w), rect, 2, 64)), rect


@pytest.mark.parametrize("chroma", CHROMAS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_frame_alone_and_the_detector_views(layout, chroma):
    dst, rr = (45, 61), rects(45, 61)
    got = call(stack(layout, chroma, 6), rr, dst)
    for t in range(T):
        alone = stack(layout, chroma, 6, t, t + 1)
        assert alone.data.data_ptr() % 4 == 2 * (t % 2)  # the block's base pointer, and its end at the other parity
        assert torch.equal(call(alone, rr[t:t + 1], dst)[0], got[t]), t
        # the block's first 4 luma bytes and the last 4 bytes of its last chroma row (NV12): no dword load may cover them
        for rect in ((0, 0, 4, 2), (130, 96, 4, 2)):
            assert torch.equal(call(alone, [rect], (2, 2))[0], hm.resize_rgb8(rgb8(layout, chroma, 6, t), rect, 2, 2)), (t, rect)
    views = image.detector_views_device(stack(layout, chroma, 6, 0, 3), 36)
    assert tuple(views.shape) == (3, 36, 49, 3)
    for t in range(3):
        assert torch.equal(views[t].cpu(), hm.resize_rgb8(rgb8(layout, chroma, 6, t), None, 36, 49, scale=(49, 18)))


def test_invalid_input_names_the_problem_and_launches_nothing():
    rr = rects(16, 16)
    rr[3] = (5, 5, 0, 9)
    out = torch.full((T, 16, 16, 3), 77, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="frame 3"):
        image.front_frames_device(stack("i420", "nearest", 0), rr, 16, 16, out=out)
    odd = image.YuvFrames(planes("i420")[:, :96].cuda(), 64, W, "i420")
    odd.w, odd.data = W - 1, odd.data[:, :, :W - 1].contiguous()  # an odd width past the constructor's check: the library's own
    with pytest.raises(ValueError, match="even"):
        image.front_frames_device(odd, rects(16, 16), 16, 16, out=out)
    with pytest.raises(ValueError, match="even"):
        image.YuvFrames(planes("i420")[:, :, :W - 1], H, W - 1)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
