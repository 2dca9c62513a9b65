"""float_img_front_frames_planes on the GPU: 5 frames of 98 x 134 and of 97 x 133 planar YUV with pitched rows (luma rows 6 bytes
longer than their samples, chroma rows 2, 2 bytes between frames: rows and frames begin off a dword), bitwise against the
definition on the CPU, host_models.resize_rgb8(host_models.yuv_planes_to_rgb8(data, fmt)[t], rect, dst_h, dst_w).  Integers
throughout: no tolerance anywhere."""
import functools

import pytest
import torch

from tests.util import load_pkg
from tests.yuv_planes_fill import fill_planes

pkg = load_pkg()
hm, image = pkg.host_models, pkg.image
pytestmark = pytest.mark.gpu

T, GUARD = 5, 256
SIZES = [(98, 134), (97, 133)]
SAMPLES = [(8, 0, False), (10, 0, False), (12, 0, False), (10, 6, True)]  # depth, shift, semi-planar
CASES = [(sub, s, c) for sub in ("420", "422", "444") for s in SAMPLES for c in hm.YUV_CHROMA if not (sub == "444" and c == "centre")]


def rects(h, w, dst):
    """five windows per destination size: (16, 16) inside, over the left and top edges from an odd origin, outside, 1 : 1, 8 : 1;
    (37, 23) over the right and bottom edges, enlarging, the last pixel alone, the whole frame, the right edge from an odd origin"""
    if dst == (16, 16):
        return [(20, 10, 80, 60), (-15, -11, 60, 60), (200, 300, 40, 40), (7, 5, 16, 16), (3, 1, 128, 128)]
    return [(101, 71, 60, 50), (51, 41, 9, 9), (w - 1, h - 1, 1, 1), (0, 0, w, h), (w - 31, 21, 60, 50)]


@functools.lru_cache(maxsize=None)
def clip(h, w, sub, depth, shift, semi, chroma, matrix=6, frames=T):
    """(PlanarYuv on the device, the definition's RGB frames on the host): seeded, shared and never modified"""
    b, (hs, _) = (1 if depth == 8 else 2), hm.YUV_SUBSAMPLING[sub]
    kw = dict(sub=sub, depth=depth, shift=shift, semi=semi, y_pitch=w * b + 6, c_pitch=-(-w // hs) * b * (2 if semi else 1) + 2, matrix=matrix,
              chroma=chroma)
    end = hm.yuv_planes_format(h, w, **kw).last_end
    host = image.PlanarYuv(fill_planes(hm.yuv_planes_format(h, w, frame_stride=end + 2, **kw), frames, h + depth)[0], h, w, frame_stride=end + 2, **kw)
    return host.like(host.data.cuda()), host.to_rgb8()


def call(frames, rr, dst):
    """front_frames_device into a guarded buffer; the output on the host, bands checked"""
    n = len(frames) * dst[0] * dst[1] * 3
    big = torch.full((n + 2 * GUARD,), 77, dtype=torch.uint8, device="cuda:0")
    out = big[GUARD:GUARD + n].view(len(frames), dst[0], dst[1], 3)
    assert image.front_frames_device(frames, rr, dst[0], dst[1], out=out) is out
    big = big.cpu()
    assert bool((big[:GUARD] == 77).all()) and bool((big[GUARD + n:] == 77).all()), "guard band of out written"
    return big[GUARD:GUARD + n].view(len(frames), dst[0], dst[1], 3)


@pytest.mark.parametrize("sub,samples,chroma", CASES)
@pytest.mark.parametrize("h,w", SIZES)
def test_stack_equals_the_definition(h, w, sub, samples, chroma):
    frames, rgb = clip(h, w, sub, *samples, chroma)
    for dst in ((16, 16), (37, 23)):
        rr = rects(h, w, dst)
        got = call(frames, rr, dst)
        for t in range(T):
            want = hm.resize_rgb8(rgb[t], rr[t], dst[0], dst[1])
            bad = int((got[t] != want).sum())
            print("%s %s %s %d x %d -> %s frame %d rect %s: %d bytes differ" % (sub, samples, chroma, h, w, dst, t, rr[t], bad))
            assert bad == 0, (t, rr[t])


@pytest.mark.parametrize("sub,samples,chroma", [c for c in CASES if c[1] in (SAMPLES[0], SAMPLES[3]) and c[2] == ("nearest" if c[0] == "444" else "centre")])
@pytest.mark.parametrize("h,w", SIZES)
def test_every_frame_alone(h, w, sub, samples, chroma):
    """frames[t:t + 1] is a view that begins at frame t's first byte and ends with its last plane: the first and the last bytes of
    `data` may not be covered by a dword load, and the windows below read exactly those"""
    frames, rgb = clip(h, w, sub, *samples, chroma)
    for t in range(T):
        alone = frames[t:t + 1]
        assert alone.data.data_ptr() == frames.data.data_ptr() + t * frames.fmt.frame_stride and alone.data.numel() == frames.fmt.last_end
        for rect in ((0, 0, 4, 2), (w - 4, h - 2, 4, 2), (0, 0, w, h)):
            assert torch.equal(call(alone, [rect], (2, 2))[0], hm.resize_rgb8(rgb[t], rect, 2, 2)), (t, rect)


def test_a_span_of_several_staging_chunks_from_an_odd_column():
    """4 x 4100 at 16 bits, 4:2:2 centre, to 2 x 64: a tile's span is the whole row, four chunks of 1024 pixels and a rest"""
    h, w = 4, 4100
    frames, rgb = clip(h, w, "422", 10, 0, False, "centre", 4, 1)
    rect = (1, 1, w - 2, h - 2)
    assert torch.equal(call(frames, [rect], (2, 64))[0], hm.resize_rgb8(rgb[0], rect, 2, 64))


def test_a_bad_rect_names_its_frame_and_launches_nothing():
    frames, _ = clip(98, 134, "422", 10, 0, False, "centre")
    rr = rects(98, 134, (16, 16))
    rr[3] = (5, 5, 0, 9)
    out = torch.full((T, 16, 16, 3), 77, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ValueError, match="frame 3"):
        image.front_frames_device(frames, rr, 16, 16, out=out)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
