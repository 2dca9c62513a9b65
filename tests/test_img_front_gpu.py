"""float_img_front on the GPU: RGBA conversion, zero-bordered window, area / linear resize, 8-bit rounding and normalisation of an
IMAGE tensor in HBM.  The kernels work in integers from the quantiser on, so every comparison is torch.equal with the definition
on the CPU, host_models.resize_rgb8(host_models.image_to_rgb8(...)) (tests/test_img_front.py pins that definition to the
reference's RGBA conversion and to the resize rule in exact rationals) - no tolerance anywhere in this file.

Inputs are seeded noise in [-0.1, 1.1] (both clamps of the quantiser are hit); RGBA inputs carry alpha 0 and 1 in a tenth of the
pixels each.  Destinations are 64 px unless the case says otherwise."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm, W = pkg.host_models, pkg.weights
pytestmark = pytest.mark.gpu

MODES = ("discard_alpha", "blend_with_color", "replace_with_color")
GUARD = 256  # elements of guard band on each side of `out` and `work`


@functools.lru_cache(maxsize=None)
def image(seed, h, w, ch):
    """seeded (h, w, ch) fp32 noise in [-0.1, 1.1]; computed once, shared, never modified"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-0.1, 1.1, size=(h, w, ch)).astype(np.float32)
    if ch == 4:
        u = rs.uniform(size=(h, w))
        x[..., 3][u < 0.1] = 0.0
        x[..., 3][u > 0.9] = 1.0
    return torch.from_numpy(x)


@functools.lru_cache(maxsize=None)
def definition(seed, h, w, ch, dst, rect=None, scale=None, mode="blend_with_color", bkg="#000000"):
    return hm.resize_rgb8(hm.image_to_rgb8(image(seed, h, w, ch), mode, hm.hex_to_rgb8(bkg)), rect, dst[0], dst[1], scale)


def front(x, dst, rect=None, scale=None, mode="blend_with_color", bkg="#000000", out_u8=True, work_bytes=None, channels=None):
    """float_img_front on a contiguous (H, W, C) fp32 device tensor, with guard bands around `out` and `work`; returns the output
    on the host after checking the bands."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    L = pkg.native.lib()
    H, Wd, ch = (int(v) for v in x.shape)
    x0, y0, w, h = rect if rect is not None else (0, 0, Wd, H)
    sn, sd = scale if scale is not None else (0, 0)
    need = int(L.float_img_front_work_bytes(H, Wd, dst[0], dst[1]))
    assert need == H * dst[1] * 12
    n_out = dst[0] * dst[1] * 3
    out = torch.full((n_out + 2 * GUARD,), 77 if out_u8 else -7.0, dtype=torch.uint8 if out_u8 else torch.float32, device=x.device)
    work = torch.full((need // 4 + 2 * GUARD,), -123456789, dtype=torch.int32, device=x.device)  # no zeroing needed
    r, g, b = hm.hex_to_rgb8(bkg)
    pkg.native.check(L.float_img_front(C.c_void_p(x.data_ptr()), H, Wd, ch if channels is None else channels, x0, y0, w, h, sn, sd,
                                       MODES.index(mode), r, g, b, pkg.native.IMG_OUT_HWC_U8 if out_u8 else pkg.native.IMG_OUT_NCHW_PM1,
                                       C.c_void_p(out[GUARD:].data_ptr()), dst[0], dst[1], C.c_void_p(work[GUARD:].data_ptr()),
                                       need if work_bytes is None else work_bytes, pkg.native.stream_ptr(x.device)))
    out, work = out.cpu(), work.cpu()
    fill = 77 if out_u8 else -7.0
    assert bool((out[:GUARD] == fill).all()) and bool((out[GUARD + n_out:] == fill).all()), "guard band of out written"
    assert bool((work[:GUARD] == -123456789).all()) and bool((work[GUARD + need // 4:] == -123456789).all()), "guard band of work written"
    body = out[GUARD:GUARD + n_out]
    return body.reshape(dst[0], dst[1], 3) if out_u8 else body.reshape(1, 3, dst[0], dst[1])


def held(tag, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    bad = int((got != want).sum())
    print("%s: %d of %d bytes differ from the definition" % (tag, bad, want.numel()))
    assert torch.equal(got, want), tag


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels against the definition, bitwise
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (seed, H, W, channels, (dst_h, dst_w), rect, scale)
CASES = {
    "identity_64x64x3": (1, 64, 64, 3, (64, 64), None, None),                       # the quantiser alone
    "fractional_97x131x3": (2, 97, 131, 3, (64, 64), None, None),                   # prime extents, last cells clipped
    "many_tiles_1031x1543x4_to_512": (3, 1031, 1543, 4, (512, 512), None, None),    # 64-bit sums, two column tiles, odd row length
    "linear_40x40x3": (4, 40, 40, 3, (64, 64), None, None),
    "mixed_axes_50x90x3": (5, 50, 90, 3, (64, 64), None, None),                     # linear on both axes
    "zero_border_100x80x3": (6, 100, 80, 3, (64, 64), (-13, 20, 90, 90), None),
    # a zero border wider than a column tile (256 outputs): the window runs more than a tile's span past an edge of the 100-wide
    # image, so one of the two tiles lies wholly in the border (nothing to stage) and the other straddles the edge
    "border_tile_right_80x100x3_to_64x512": (13, 80, 100, 3, (64, 512), (50, 0, 1000, 80), None),      # tile 1 reads columns 550 ...
    "border_tile_left_80x100x4_to_64x512": (14, 80, 100, 4, (64, 512), (-600, 0, 1000, 80), None),     # tile 0 reads columns -600 ... -100
    "border_tile_both_80x100x3_to_64x768": (15, 80, 100, 3, (64, 768), (-550, -7, 1500, 90), None),    # tiles 0 and 2 border only
    "border_tile_right_linear_40x100x3_to_64x512": (16, 40, 100, 3, (64, 512), (50, 0, 300, 40), None),
    "border_tile_left_linear_40x100x3_to_64x512": (17, 40, 100, 3, (64, 512), (-200, 0, 300, 40), None),
    "detector_view_90x70x4":(7, 90, 70, 4, (36, 28), None, (90, 36)),              # one scale on both axes
    "degenerate_33x17x4_to_5x3": (8, 33, 17, 4, (5, 3), None, None),
    "degenerate_1x1x3": (9, 1, 1, 3, (1, 1), None, None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernels_equal_the_definition(case):
    seed, h, w, ch, dst, rect, scale = CASES[case]
    got = front(image(seed, h, w, ch).cuda(), dst, rect, scale)
    held(case, got, definition(seed, h, w, ch, dst, rect, scale))
    if case.startswith("identity"):
        assert torch.equal(got, hm.image_to_rgb8(image(seed, h, w, ch)))


@pytest.mark.parametrize("bkg", ["#000000", "#3fa07c"])
@pytest.mark.parametrize("mode", MODES)
def test_rgba_strategies_at_an_integer_factor(mode, bkg):
    """128 x 128 x 4 -> 64: the fp32 blend per source pixel, then 2 x 2 block means, a quarter of them exact ties."""
    got = front(image(10, 128, 128, 4).cuda(), (64, 64), mode=mode, bkg=bkg)
    held("128x128x4 %s %s" % (mode, bkg), got, definition(10, 128, 128, 4, (64, 64), None, None, mode, bkg))
    s = hm.image_to_rgb8(image(10, 128, 128, 4), mode, hm.hex_to_rgb8(bkg)).to(torch.int64).reshape(64, 2, 64, 2, 3).sum(dim=(1, 3))
    assert 0.15 < float(((s % 4) == 2).float().mean()) < 0.35  # the ties are there


def test_strategies_differ_where_they_should():
    x = image(10, 128, 128, 4).cuda()
    outs = {(m, b): front(x, (64, 64), mode=m, bkg=b) for m in MODES for b in ("#000000", "#3fa07c")}
    assert torch.equal(outs[("discard_alpha", "#000000")], outs[("discard_alpha", "#3fa07c")])
    assert not torch.equal(outs[("blend_with_color", "#000000")], outs[("blend_with_color", "#3fa07c")])
    assert not torch.equal(outs[("replace_with_color", "#000000")], outs[("replace_with_color", "#3fa07c")])
    assert not torch.equal(outs[("blend_with_color", "#000000")], outs[("discard_alpha", "#000000")])


def test_window_outside_the_image_gives_zeros():
    x = image(6, 100, 80, 3).cuda()
    for rect in ((200, 300, 90, 90), (-200, 10, 90, 90), (10, -90, 90, 90)):
        got = front(x, (64, 64), rect)
        assert int(got.max()) == 0, rect


def test_model_input_layout_and_values():
    """FLOAT_IMG_OUT_NCHW_PM1: bitwise q / 127.5 - 1 in fp32, planar."""
    seed, h, w, ch, dst, rect, scale = CASES["fractional_97x131x3"]
    got = front(image(seed, h, w, ch).cuda(), dst, out_u8=False)
    held("NCHW_PM1", got, hm.rgb8_to_model_input(definition(seed, h, w, ch, dst)))
    seed, h, w, ch, dst, rect, scale = CASES["identity_64x64x3"]  # every level 0 ... 255 occurs
    q = definition(seed, h, w, ch, dst)
    assert int(q.unique().numel()) == 256
    held("NCHW_PM1, all levels", front(image(seed, h, w, ch).cuda(), dst, out_u8=False), hm.rgb8_to_model_input(q))


def test_two_runs_give_equal_bytes():
    seed, h, w, ch, dst, rect, scale = CASES["zero_border_100x80x3"]
    x = image(seed, h, w, ch).cuda()
    assert torch.equal(front(x, dst, rect), front(x, dst, rect))


def test_bad_arguments_raise_and_launch_nothing():
    """The guard bands and the output stay untouched: nothing was launched."""
    x = image(1, 64, 64, 3).cuda()
    L = pkg.native.lib()
    need = int(L.float_img_front_work_bytes(64, 64, 64, 64))
    out = torch.full((64 * 64 * 3,), 77, dtype=torch.uint8, device="cuda:0")
    work = torch.full((need // 4,), -5, dtype=torch.int32, device="cuda:0")

    def call(channels=3, scale=(0, 0), work_bytes=need):
        pkg.native.check(L.float_img_front(C.c_void_p(x.data_ptr()), 64, 64, channels, 0, 0, 64, 64, scale[0], scale[1], 0, 0, 0, 0,
                                           pkg.native.IMG_OUT_HWC_U8, C.c_void_p(out.data_ptr()), 64, 64, C.c_void_p(work.data_ptr()),
                                           work_bytes, pkg.native.stream_ptr(x.device)))

    for kw, word in ((dict(work_bytes=need - 1), "work_bytes"), (dict(channels=2), "channels"), (dict(scale=(3, 2)), "starts outside")):
        with pytest.raises(ValueError) as e:
            call(**kw)
        assert word in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((work == -5).all())
    call()
    assert torch.equal(out.cpu().reshape(64, 64, 3), definition(1, 64, 64, 3, (64, 64)))


# ---------------------------------------------------------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------------------------------------------------------
def test_mirror_takes_host_and_device_tensors_of_any_float_dtype():
    img = image(2, 97, 131, 3)
    want = hm.rgb8_to_model_input(definition(2, 97, 131, 3, (64, 64)))
    for form in (img, img[None], img.cuda(), img.double()):
        got = pkg.image.preprocess_image_device(form, 64, device="cuda:0")
        assert got.is_cuda and tuple(got.shape) == (1, 3, 64, 64) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), want)
    half = img.half()  # the definition reads the same fp16 values
    want16 = hm.rgb8_to_model_input(hm.resize_rgb8(hm.image_to_rgb8(half), None, 64, 64))
    assert torch.equal(pkg.image.preprocess_image_device(half, 64, device="cuda:0").cpu(), want16)
    view = pkg.image.detector_view_device(image(7, 90, 70, 4), 36, device="cuda:0")
    assert view.dtype == torch.uint8 and tuple(view.shape) == (36, 28, 3)
    assert torch.equal(view.cpu(), definition(7, 90, 70, 4, (36, 28), None, (90, 36)))
    with pytest.raises(ValueError):
        pkg.image.preprocess_image_device(torch.zeros(2, 8, 8, 3), 8, device="cuda:0")


def test_mirror_crop_centred_beyond_the_image_edge():
    """A 512-px crop whose centre lies right of a 120 x 90 image: the second column tile is border only."""
    img = image(18, 90, 120, 3)
    rect = (100, -300, 700, 700)
    want = hm.rgb8_to_model_input(hm.resize_rgb8(hm.image_to_rgb8(img), rect, 512, 512))
    got = pkg.image.preprocess_image_device(img, 512, rect, device="cuda:0")
    held("crop beyond the edge", got.cpu(), want)
    assert bool((got.cpu()[..., 256:] == -1.0).all())  # columns 256 ... read source columns 450 ...: black


# ---------------------------------------------------------------------------------------------------------------------------
# through the product: the synthetic 64-px agent of tests/test_dec_u8_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _agent():
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.input_size, opt.nfe = 64, 6
    cfg = pkg.config.FmtConfig.from_options(opt)
    acfg = pkg.config.small_audio_config()
    acfg.dim_w = opt.dim_w
    parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
                 audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
    return gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8)


def _audio():
    return {"waveform": W.synth_waveform(1.4, seed=9).reshape(1, 1, -1), "sample_rate": 16000}


def test_agent_transparent_portrait_gets_the_background_colour(monkeypatch):
    """The left half is transparent with white under the transparency: the node's widgets decide what the model sees there."""
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    agent = _agent()
    monkeypatch.setattr(agent.opt, "bkg_color_hex", "#00ff00")
    monkeypatch.setattr(agent.opt, "rgba_conversion", "blend_with_color")
    img = image(11, 128, 128, 4).clone()
    img[:, :64, :3] = 1.0
    img[:, :64, 3] = 0.0
    s, _ = agent.host_inputs(img[None], _audio())
    want = hm.rgb8_to_model_input(hm.resize_rgb8(hm.image_to_rgb8(img, "blend_with_color", (0, 255, 0)), None, 64, 64))
    assert s.is_cuda and torch.equal(s.cpu(), want)
    green = torch.tensor([-1.0, 1.0, -1.0]).reshape(1, 3, 1, 1).expand(1, 3, 64, 32)
    assert torch.equal(s.cpu()[..., :32], green)
    monkeypatch.setenv("FLOAT_AMD_IMAGE_FRONT", "0")  # read at the call: today's route, alpha discarded
    s0, _ = agent.host_inputs(img[None], _audio())
    assert torch.equal(s0.cpu(), hm.preprocess_image(img[..., :3].cuda(), 64).cpu())
    assert torch.equal(s0.cpu()[..., :32], torch.ones(1, 3, 64, 32))


def test_agent_rgb_portrait_at_the_model_size_is_unchanged(monkeypatch):
    agent = _agent()
    img = image(1, 64, 64, 3)
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    s_on, _ = agent.host_inputs(img[None], _audio())
    monkeypatch.setenv("FLOAT_AMD_IMAGE_FRONT", "0")
    s_off, _ = agent.host_inputs(img[None], _audio())
    assert torch.equal(s_on, s_off) and torch.equal(s_on.cpu(), hm.preprocess_image(img.cuda(), 64).cpu())


def test_agent_keeps_the_host_route_beyond_the_size_limits(monkeypatch):
    """A 12 : 1 panorama with face_align: the detector's 360-px copy would be 4320 columns wide, more than float_img_front's
    4096, so host_inputs takes the host route, as with the switch off, instead of raising."""
    ft = pkg.image.front_takes
    assert ft(400, 4800, 64) and not ft(400, 4800, 64, crop=True) and ft(400, 4400, 64, crop=True)
    assert ft(16384, 8, 64) and not ft(16385, 8, 64) and not ft(8, 16385, 64) and not ft(64, 64, 4097)
    agent = _agent()
    img = image(19, 400, 4800, 3)

    class FA:
        class face_detector:
            @staticmethod
            def detect_from_image(arr):
                return [(2000.0, 100.0, 2200.0, 300.0, 0.99)]

    monkeypatch.setattr(hm, "_FA", FA())
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    s_on, _ = agent.host_inputs(img[None], _audio(), no_crop=False)
    monkeypatch.setenv("FLOAT_AMD_IMAGE_FRONT", "0")
    s_off, _ = agent.host_inputs(img[None], _audio(), no_crop=False)
    assert tuple(s_on.shape) == (1, 3, 64, 64) and torch.equal(s_on, s_off)


def test_agent_face_crop_route(monkeypatch):
    """face_align with a detector: the detector sees the definition's 360-px view, the model the definition's crop of the
    zero-bordered image at margin 1.6, and the bbox is the one process_img returns today for that box."""
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    agent = _agent()
    seen = []
    box = (100.0, 40.0, 250.0, 200.0, 0.99)  # in the 360-px view; the crop reaches past the right edge of the image

    class Detector:
        def detect_from_image(self, arr):
            seen.append(arr.copy())
            return [box]

    class FA:
        face_detector = Detector()

    monkeypatch.setattr(hm, "_FA", FA())
    img = image(12, 400, 300, 3)
    _, bbox_today = hm.process_img(img, 64, 1.6)  # today's host route with the same stub
    assert len(seen) == 1
    s, _ = agent.host_inputs(img[None], _audio(), no_crop=False)
    assert len(seen) == 2
    view = hm.resize_rgb8(hm.image_to_rgb8(img), None, 360, 270, scale=(10, 9))
    assert seen[1].dtype == np.uint8 and np.array_equal(seen[1], view.numpy())
    mult = 360.0 / 400
    x1, y1, x2, y2 = (int(v / mult) for v in box[:4])
    bs = int(max(int((y2 - y1) / 2), int((x2 - x1) / 2)) * 1.6)
    rect = (int((x1 + x2) / 2) - bs, int((y1 + y2) / 2) - bs, 2 * bs, 2 * bs)
    assert rect == bbox_today and (rect[0] + rect[2] > 300 or rect[0] < 0 or rect[1] < 0)  # it does reach outside
    want = hm.rgb8_to_model_input(hm.resize_rgb8(hm.image_to_rgb8(img), rect, 64, 64))
    assert torch.equal(s.cpu(), want)
    rect_dev, bbox_dev = hm.process_img(img, 64, 1.6, front=lambda vh: pkg.image.detector_view_device(img, vh, device="cuda:0"))
    assert rect_dev == bbox_dev == bbox_today
