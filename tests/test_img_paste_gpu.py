"""float_img_paste on the GPU: the generated 8-bit frames back in the source portrait, in HBM.  The kernel works in integers, so every
comparison is torch.equal with the definition on the CPU, host_models.paste_rgb8 (tests/test_img_paste.py pins that definition to
the rule in exact rationals) - no tolerance anywhere in this file.

Inputs are seeded uint8 noise; frames are 64 x 64 unless the case says otherwise; `out` sits between guard bands of 256 bytes.  The
cases are the smallest that break an alignment or tap-range mistake: 3 W and 3 H W that are no multiples of 4 (frames after the
first start misaligned), rows longer than a workgroup's span, every scale regime, boxes on and beyond every edge."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

from tests.jpeg_util import avi_parts
from tests.test_img_front_gpu import _agent, _audio, image
from tests.util import load_pkg

pkg = load_pkg()
hm = pkg.host_models
pytestmark = pytest.mark.gpu

GUARD = 256  # bytes of guard band on each side of `out`
FILL = 77


@functools.lru_cache(maxsize=None)
def noise(seed, *shape):
    """seeded uint8 noise; computed once, shared, never modified"""
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def definition(src_hw, n_frames, frame_hw, rect, feather):
    return hm.paste_rgb8(noise(1, *src_hw, 3), noise(2, n_frames, *frame_hw, 3), rect, feather)


def paste_raw(src, frames, rect, feather, shift=0, expect=0):
    """float_img_paste on device tensors with guard bands around `out`, which starts `shift` bytes past a 256-byte boundary;
    returns (return code, message, the output on the host) after checking the bands."""
    L = pkg.native.lib()
    T, H, Wd = int(frames.shape[0]), int(src.shape[0]), int(src.shape[1])
    n = T * H * Wd * 3
    buf = torch.full((n + 2 * GUARD + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    at = GUARD + shift
    rc = L.float_img_paste(C.c_void_p(src.data_ptr()), H, Wd, C.c_void_p(frames.data_ptr()), T, int(frames.shape[1]), int(frames.shape[2]),
                           *rect, feather, C.c_void_p(buf.data_ptr() + at), pkg.native.stream_ptr(buf.device))
    msg = L.float_last_error().decode("utf-8", "replace") if rc else ""
    assert rc == expect, (rc, msg)
    buf = buf.cpu()
    assert bool((buf[:at] == FILL).all()) and bool((buf[at + n:] == FILL).all()), "guard band of out written"
    return rc, msg, buf[at:at + n].reshape(T, H, Wd, 3)


def held(tag, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    bad = int((got != want).sum())
    print("%s: %d of %d bytes differ from the definition" % (tag, bad, want.numel()))
    assert torch.equal(got, want), tag


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel against the definition, bitwise
# ---------------------------------------------------------------------------------------------------------------------------
F64 = (64, 64)
# name -> (source (H, W), T, frame (h, w), rect (x0, y0, w, h), feather)
CASES = {
    "misaligned_frames_90x67_T3": ((90, 67), 3, F64, (10, 20, 37, 37), 7),  # 3 W = 201, 3 H W = 2 mod 4
    "source_64x64": ((64, 64), 2, F64, (10, 12, 37, 37), 7),
    "source_1x1_box_on_it": ((1, 1), 3, F64, (0, 0, 1, 1), 0),              # a frame is 3 bytes: head and tail only
    "source_1x1_box_around_it": ((1, 1), 3, F64, (-3, -3, 7, 7), 2),
    "source_33x17": ((33, 17), 3, F64, (2, 3, 10, 12), 2),
    "long_row_70x1030": ((70, 1030), 2, F64, (500, 10, 37, 37), 7),         # a row of 3090 bytes spans workgroups
    "shrink_37x37": ((90, 67), 2, F64, (10, 20, 37, 37), 0),
    "enlarge_100x100_in_130x150": ((130, 150), 2, F64, (20, 15, 100, 100), 7),
    "two_factors_50x23": ((90, 67), 2, F64, (5, 7, 50, 23), 1),             # 32 : 25 by 64 : 23, cells that straddle samples
    "mixed_axes_70x23": ((90, 80), 2, F64, (5, 7, 70, 23), 1),              # x enlarges, y shrinks: the linear rule on both
    "mixed_axes_frame_40x56_to_50x23": ((90, 67), 2, (40, 56), (5, 7, 50, 23), 1),  # 56 -> 50 shrinks, 40 -> 23 shrinks; and
    "mixed_axes_frame_56x40_to_50x23": ((90, 67), 2, (56, 40), (5, 7, 50, 23), 1),  # 40 -> 50 enlarges, 56 -> 23 shrinks
    "scale_one_at_an_offset": ((90, 67), 2, F64, (2, 20, 64, 64), 7),
    "box_3x3": ((90, 67), 2, F64, (30, 31, 3, 3), 1),                       # 22 taps per axis
    "box_1x1": ((90, 67), 2, F64, (30, 31, 1, 1), 0),                       # 64 x 64 taps
    "whole_image": ((90, 67), 2, F64, (0, 0, 67, 90), 9),
    "beyond_left": ((90, 67), 2, F64, (-13, 20, 37, 37), 7),
    "beyond_right": ((90, 67), 2, F64, (40, 20, 37, 37), 7),
    "beyond_top": ((90, 67), 2, F64, (10, -9, 37, 37), 7),
    "beyond_bottom": ((90, 67), 2, F64, (10, 60, 37, 37), 7),
    "beyond_all_four": ((90, 67), 2, F64, (-5, -6, 100, 110), 7),
    "feather_0_open": ((90, 67), 1, F64, (10, 20, 37, 37), 0),
    "feather_1_open": ((90, 67), 1, F64, (10, 20, 37, 37), 1),
    "feather_100_open": ((90, 67), 1, F64, (10, 20, 37, 37), 100),
    "feather_1_left_closed": ((90, 67), 1, F64, (0, 20, 37, 37), 1),
    "feather_7_right_and_top_closed": ((90, 67), 1, F64, (30, 0, 37, 37), 7),
    "feather_100_bottom_closed": ((90, 67), 1, F64, (10, 53, 37, 37), 100),
    "frame_40x56": ((90, 67), 2, (40, 56), (10, 20, 37, 37), 7),
    "frame_side_limit_1024_to_1023": ((1030, 1030), 1, (1024, 1024), (3, 4, 1023, 1023), 7),
    "one_frame": ((90, 67), 1, F64, (10, 20, 37, 37), 7),
    "seventeen_frames": ((90, 67), 17, F64, (10, -4, 37, 37), 7),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_equals_the_definition(case):
    src_hw, T, frame_hw, rect, feather = CASES[case]
    src, frames = noise(1, *src_hw, 3).cuda(), noise(2, T, *frame_hw, 3).cuda()
    _, _, got = paste_raw(src, frames, rect, feather)
    held(case, got, definition(src_hw, T, frame_hw, rect, feather))


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_out_at_every_alignment(shift):
    src_hw, T, frame_hw, rect, feather = CASES["misaligned_frames_90x67_T3"]
    _, _, got = paste_raw(noise(1, *src_hw, 3).cuda(), noise(2, T, *frame_hw, 3).cuda(), rect, feather, shift=shift)
    held("out + %d" % shift, got, definition(src_hw, T, frame_hw, rect, feather))


@pytest.mark.parametrize("rect", [(67, 3, 40, 40), (-40, 3, 40, 40), (3, -40, 40, 40), (3, 90, 40, 40)])
def test_box_wholly_outside_the_image_gives_the_source(rect):
    src = noise(1, 90, 67, 3)
    _, _, got = paste_raw(src.cuda(), noise(2, 2, 64, 64, 3).cuda(), rect, 3)
    held("outside %r" % (rect,), got, src[None].expand(2, -1, -1, -1))


def test_identities():
    frames = noise(2, 3, 64, 64, 3)
    _, _, got = paste_raw(noise(1, 64, 64, 3).cuda(), frames.cuda(), (0, 0, 64, 64), 9)
    held("a box of the frames' own size over a source of that size", got, frames)
    _, _, got = paste_raw(noise(1, 90, 67, 3).cuda(), frames.cuda(), (0, 0, 67, 90), 5)
    held("rect = whole image is the plain resize", got, torch.stack([hm.resize_rgb8(frames[t], None, 90, 67) for t in range(3)]))


def test_two_runs_give_equal_bytes():
    src_hw, T, frame_hw, rect, feather = CASES["beyond_left"]
    src, frames = noise(1, *src_hw, 3).cuda(), noise(2, T, *frame_hw, 3).cuda()
    assert torch.equal(paste_raw(src, frames, rect, feather)[2], paste_raw(src, frames, rect, feather)[2])


def test_bad_arguments_raise_and_launch_nothing():
    """paste_raw checks that `out` and its guard bands stay at their fill: nothing was launched."""
    src, frames = noise(1, 90, 67, 3).cuda(), noise(2, 2, 64, 64, 3).cuda()
    L = pkg.native.lib()
    out = torch.full((2 * 90 * 67 * 3,), FILL, dtype=torch.uint8, device="cuda:0")

    def call(src_hw=(90, 67), T=2, fr=(64, 64), rect=(10, 20, 37, 37), feather=7, null=None):
        p = [C.c_void_p(src.data_ptr()), C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr())]
        if null is not None:
            p[null] = None
        rc = L.float_img_paste(p[0], src_hw[0], src_hw[1], p[1], T, fr[0], fr[1], *rect, feather, p[2], pkg.native.stream_ptr(out.device))
        return rc, L.float_last_error().decode("utf-8", "replace") if rc else ""

    for kw, word in ((dict(src_hw=(0, 67)), "src_h"), (dict(src_hw=(90, 16385)), "src_w"), (dict(T=0), "n_frames"),
                     (dict(fr=(1025, 64)), "fr_h"), (dict(fr=(64, 0)), "fr_w"), (dict(rect=(10, 20, 0, 37)), "rect_w"),
                     (dict(rect=(10, 20, 37, 16385)), "rect_h"), (dict(feather=-1), "feather"), (dict(feather=16385), "feather"),
                     (dict(null=0), "null"), (dict(null=1), "null"), (dict(null=2), "null")):
        rc, msg = call(**kw)
        assert rc == 1 and "float_img_paste" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    with pytest.raises(ValueError) as e:
        pkg.native.check(call(feather=-1)[0])
    assert "feather" in str(e.value)
    assert call() == (0, "")
    assert torch.equal(out.cpu().reshape(2, 90, 67, 3), definition((90, 67), 2, F64, (10, 20, 37, 37), 7))


# ---------------------------------------------------------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------------------------------------------------------
def test_mirror_takes_host_and_device_tensors():
    src, frames, rect = noise(1, 90, 67, 3), noise(2, 2, 64, 64, 3), (10, 20, 37, 37)
    want = definition((90, 67), 2, F64, rect, 7)
    for s, f in ((src, frames), (src.cuda(), frames), (src, frames.cuda()), (src.cuda(), frames.cuda())):
        got = pkg.image.paste_frames_device(s, f, rect, 7)
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    assert torch.equal(pkg.image.paste_frames_device(src, frames, rect).cpu(), hm.paste_rgb8(src, frames, rect, 37 // 16))  # the default feather
    out = torch.empty(2, 90, 67, 3, dtype=torch.uint8, device="cuda:0")
    assert pkg.image.paste_frames_device(src, frames, rect, 7, out=out) is out and torch.equal(out.cpu(), want)
    for args in ((src.float(), frames, rect), (src, frames[0], rect), (src, frames, rect[:3]), (src, frames, (0, 0, 0, 5)),
                 (src, frames, rect, -1), (src, frames, rect, 7, out[:1]), (src, frames, rect, 7, out.cpu())):
        with pytest.raises(ValueError):
            pkg.image.paste_frames_device(*args)


def test_source_rgb8_device_equals_the_definition():
    for ch, mode, bkg in ((3, "blend_with_color", "#000000"), (4, "blend_with_color", "#3fa07c"), (4, "replace_with_color", "#3fa07c"),
                          (4, "discard_alpha", "#3fa07c")):
        img = image(7, 90, 70, ch)
        got = pkg.image.source_rgb8_device(img[None], mode, bkg, device="cuda:0")
        assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
        held("source_rgb8_device %d %s" % (ch, mode), got.cpu(), hm.image_to_rgb8(img, mode, hm.hex_to_rgb8(bkg)))
    wide = image(20, 2, 4100, 4)  # beyond float_img_front's destination limit: the host definition and one upload
    held("4100 columns", pkg.image.source_rgb8_device(wide, "blend_with_color", "#3fa07c", device="cuda:0").cpu(),
         hm.image_to_rgb8(wide, "blend_with_color", hm.hex_to_rgb8("#3fa07c")))


# ---------------------------------------------------------------------------------------------------------------------------
# through the product: the synthetic 64-px agent of tests/test_img_front_gpu.py, a 1.4-s clip (35 frames)
# ---------------------------------------------------------------------------------------------------------------------------
SEED = 5
BOX = (100.0, 40.0, 250.0, 200.0, 0.99)  # the stub detector's box in the 360-px view of a 400 x 300 portrait


def _stub_detector(monkeypatch):
    class Detector:
        def detect_from_image(self, arr):
            return [BOX]

    class FA:
        face_detector = Detector()

    monkeypatch.setattr(hm, "_FA", FA())


def _face_rect():
    mult = 360.0 / 400
    x1, y1, x2, y2 = (int(v / mult) for v in BOX[:4])
    bs = int(max(int((y2 - y1) / 2), int((x2 - x1) / 2)) * 1.6)
    return (int((x1 + x2) / 2) - bs, int((y1 + y2) / 2) - bs, 2 * bs, 2 * bs)


_clips = {}


def _face_clip(monkeypatch):
    """(img, rect, infer_pasted of it) on the face-crop route, computed once and left unchanged"""
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    _stub_detector(monkeypatch)
    img = image(12, 400, 300, 3)
    if "face" not in _clips:
        _clips["face"] = _agent().infer_pasted(img[None], _audio(), emo="happy", no_crop=False, seed=SEED).clone()
    return img, _face_rect(), _clips["face"]


def test_agent_infer_pasted_equals_the_definition(monkeypatch):
    agent = _agent()
    img, rect, got = _face_clip(monkeypatch)
    assert rect[0] + rect[2] > 300  # the crop reaches past the right edge
    s, a, place = agent.host_inputs_placed(img[None], _audio(), no_crop=False)
    assert tuple(place.rect) == rect and place.src8.is_cuda and torch.equal(place.src8.cpu(), hm.image_to_rgb8(img))
    crops = agent.infer_device(s, a, emo="happy", seed=SEED, out_dtype=torch.uint8)
    assert tuple(crops.shape) == (35, 64, 64, 3)
    assert got.dtype == torch.uint8 and not got.is_cuda and tuple(got.shape) == (35, 400, 300, 3)
    held("infer_pasted", got, hm.paste_rgb8(hm.image_to_rgb8(img), crops, rect, hm.default_feather(rect)))
    wide = agent.infer_pasted(img[None], _audio(), emo="happy", no_crop=False, seed=SEED, feather=40)
    held("infer_pasted, feather 40", wide, hm.paste_rgb8(hm.image_to_rgb8(img), crops, rect, 40))
    assert not torch.equal(wide, got)


def test_agent_host_inputs_is_unchanged(monkeypatch):
    agent = _agent()
    _stub_detector(monkeypatch)
    for img, no_crop in ((image(12, 400, 300, 3), False), (image(12, 400, 300, 3), True), (image(11, 128, 128, 4), True),
                         (image(1, 64, 64, 3), True), (image(7, 90, 70, 4), False)):
        for front in ("1", "0"):
            monkeypatch.setenv("FLOAT_AMD_IMAGE_FRONT", front)
            two = agent.host_inputs(img[None], _audio(), no_crop)
            three = agent.host_inputs_placed(img[None], _audio(), no_crop)
            assert len(two) == 2 and len(three) == 3
            assert torch.equal(two[0], three[0]) and torch.equal(two[1], three[1])
            H, Wd = int(img.shape[0]), int(img.shape[1])
            assert tuple(three[2].src8.shape) == (H, Wd, 3)
            if no_crop:
                assert tuple(three[2].rect) == (0, 0, Wd, H)
            else:
                assert tuple(three[2].rect) == hm.process_img(img[..., :3], 64, 1.6)[1]  # the bbox of the host route, same stub


def test_agent_stream_pasted_concatenates_to_infer_pasted(monkeypatch):
    agent = _agent()
    img, rect, want = _face_clip(monkeypatch)
    blocks = [(b.first, b.last, b.frames.clone()) for b in agent.stream_pasted(img[None], _audio(), emo="happy", no_crop=False, seed=SEED)]
    assert [(f, l) for f, l, _ in blocks] == [(0, 35)]
    held("stream_pasted", torch.cat([fr for _, _, fr in blocks]), want)
    audio = {"waveform": pkg.weights.synth_waveform(2.4, seed=10).reshape(1, 1, -1), "sample_rate": 16000}  # 60 frames: two windows
    whole = agent.infer_pasted(img[None], audio, emo="happy", no_crop=False, seed=SEED)
    blocks = [(b.first, b.last, b.frames.clone()) for b in agent.stream_pasted(img[None], audio, emo="happy", no_crop=False, seed=SEED, slots=2)]
    assert [(f, l) for f, l, _ in blocks] == [(0, 50), (50, 60)]
    held("stream_pasted, two windows", torch.cat([fr for _, _, fr in blocks]), whole)
    with pytest.raises(ValueError):
        agent.stream_pasted(img[None], _audio(), emo="happy", slots=1)


def test_agent_rgba_portrait_honours_the_background_colour_outside_the_box(monkeypatch):
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    _stub_detector(monkeypatch)
    agent = _agent()
    monkeypatch.setattr(agent.opt, "bkg_color_hex", "#00ff00")
    monkeypatch.setattr(agent.opt, "rgba_conversion", "blend_with_color")
    img = image(21, 400, 300, 4).clone()
    img[:, :40, 3] = 0.0  # a transparent strip left of the box
    rect = _face_rect()
    assert rect[0] > 40
    got = agent.infer_pasted(img[None], _audio(), emo="happy", no_crop=False, seed=SEED)
    src8 = hm.image_to_rgb8(img, "blend_with_color", (0, 255, 0))
    assert torch.equal(got[:, :, :40], torch.tensor([0, 255, 0], dtype=torch.uint8).expand(35, 400, 40, 3))
    s, a, place = agent.host_inputs_placed(img[None], _audio(), no_crop=False)
    held("rgba portrait", got, hm.paste_rgb8(src8, agent.infer_device(s, a, emo="happy", seed=SEED, out_dtype=torch.uint8), rect,
                                             hm.default_feather(rect)))


def test_agent_no_crop_is_the_plain_resize_and_jpeg_is_the_definitions(monkeypatch, tmp_path):
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    agent = _agent()
    img = image(22, 96, 80, 3)
    s, a = agent.host_inputs(img[None], _audio(), no_crop=True)
    crops = agent.infer_device(s, a, emo="happy", seed=SEED, out_dtype=torch.uint8)
    pasted = agent.infer_pasted(img[None], _audio(), emo="happy", no_crop=True, seed=SEED)
    held("no_crop", pasted, torch.stack([hm.resize_rgb8(crops[t], None, 96, 80) for t in range(crops.shape[0])]))
    files = agent.infer_pasted_jpeg(img[None], _audio(), emo="happy", no_crop=True, seed=SEED)
    want = hm.jpeg_encode_rgb8(pasted, 90, 80 // 16)
    assert [bytes(f) for f in files] == [bytes(f) for f in want]
    streamed = [bytes(f) for b in agent.stream_pasted_jpeg(img[None], _audio(), emo="happy", no_crop=True, seed=SEED) for f in b.frames]
    assert streamed == [bytes(f) for f in want]
    f = io.BytesIO()
    assert agent.write_video(f, img[None], _audio(), emo="happy", no_crop=True, seed=SEED, paste_back=True) == 35
    p = avi_parts(f.getvalue())
    assert (p["avih"][8], p["avih"][9]) == (80, 96) and p["video"][0] == bytes(want[0]) and len(p["video"]) == 35


def test_agent_jpeg_refuses_sides_that_are_no_multiples_of_16(tmp_path):
    agent = _agent()
    img = image(23, 90, 67, 3)
    path = tmp_path / "never.avi"
    for call in (lambda: agent.infer_pasted_jpeg(img[None], _audio(), emo="happy", no_crop=True, seed=SEED),
                 lambda: agent.stream_pasted_jpeg(img[None], _audio(), emo="happy", no_crop=True, seed=SEED),
                 lambda: agent.write_video(str(path), img[None], _audio(), emo="happy", no_crop=True, seed=SEED, paste_back=True)):
        with pytest.raises(ValueError) as e:
            call()
        assert "multiples of 16" in str(e.value)
    assert not path.exists()
    assert tuple(agent.infer_pasted(img[None], _audio(), emo="happy", no_crop=True, seed=SEED).shape) == (35, 90, 67, 3)  # frames are fine
