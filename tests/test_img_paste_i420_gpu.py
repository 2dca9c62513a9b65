"""float_img_paste_i420 on the GPU: the generated 8-bit frames pasted back into the source portrait and converted to planar YUV 4:2:0
in one kernel.  The kernel works in integers, so every comparison is torch.equal with the definition on the CPU,
host_models.paste_i420 = rgb8_to_i420(paste_rgb8(...)) (tests/test_img_paste_i420.py writes its chroma rule out per sample) - no
tolerance anywhere in this file.

Inputs are seeded uint8 noise; `out` sits between guard bands of 256 bytes.  The cases are the smallest that break a chroma-siting,
alignment or plane-offset mistake: odd box offsets and sides (2 x 2 blocks that straddle the box edge and the feather), widths
with W % 4 == 2 (the byte-store path, and a last cell of two columns), a U plane of odd size (V at an odd address), a row longer
than a workgroup's cells, every scale regime, boxes on and beyond every edge."""
import ctypes as C
import functools
import io

import pytest
import torch

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
    return hm.paste_i420(noise(1, *src_hw, 3), noise(2, n_frames, *frame_hw, 3), rect, feather)


def paste_raw(src, frames, rect, feather, shift=0, expect=0, matrix=0):
    """float_img_paste_i420 on device tensors with guard bands around `out`, which starts `shift` bytes past a 256-byte boundary;
    returns (return code, message, the output on the host) after checking that the bytes around the frames are unchanged."""
    L = pkg.native.lib()
    T, H, Wd = int(frames.shape[0]), int(src.shape[0]), int(src.shape[1])
    n = T * (3 * H // 2) * Wd
    buf = torch.full((n + 2 * GUARD + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 256 == 0
    at = GUARD + shift
    rc = L.float_img_paste_i420(C.c_void_p(src.data_ptr()), H, Wd, C.c_void_p(frames.data_ptr()), T, int(frames.shape[1]), int(frames.shape[2]),
                                *rect, feather, matrix, C.c_void_p(buf.data_ptr() + at), pkg.native.stream_ptr(buf.device))
    msg = L.float_last_error().decode("utf-8", "replace") if rc else ""
    assert rc == expect, (rc, msg)
    buf = buf.cpu()
    assert bool((buf[:at] == FILL).all()) and bool((buf[at + n:] == FILL).all()), "bytes around the frames written"
    return rc, msg, buf[at:at + n].reshape(T, 3 * H // 2, Wd)


def held(tag, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.shape, want.shape)
    bad = int((got != want).sum())
    print("%s: %d of %d bytes differ from the definition" % (tag, bad, want.numel()))
    assert torch.equal(got, want), tag


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel against the definition, bitwise
# ---------------------------------------------------------------------------------------------------------------------------
F64 = (64, 64)
# name -> (source (H, W), T, frame (h, w), rect (x0, y0, w, h), feather)
CASES = {
    "01_odd_box_34x50_byte_path": ((34, 50), 3, F64, (7, 5, 21, 19), 4),      # blocks straddle all four edges and the feather; W % 4 = 2
    "02_fast_path_36x40_area": ((36, 40), 2, F64, (5, 3, 16, 12), 2),
    "03_linear_130x152": ((130, 152), 2, F64, (21, 15, 100, 100), 7),
    "04_mixed_axes_90x80": ((90, 80), 2, F64, (5, 7, 70, 23), 1),
    "05_beyond_all_four_90x68": ((90, 68), 2, F64, (-5, -6, 100, 110), 7),
    "06_beyond_left_odd_offsets_90x68": ((90, 68), 2, F64, (-13, 21, 37, 37), 7),
    "07_box_misses_12x18": ((12, 18), 2, (8, 8), (40, 40, 4, 4), 3),           # every frame is rgb8_to_i420(src)
    "08_source_2x2": ((2, 2), 3, (4, 4), (-1, -1, 4, 4), 0),                   # a 6-byte frame with 1-byte chroma planes
    "09_odd_u_plane_6x70": ((6, 70), 3, (8, 8), (3, 1, 5, 3), 1),              # U plane of 105 bytes: V starts at an odd address
    "10_long_row_6x2052": ((6, 2052), 1, F64, (1000, 1, 37, 4), 3),            # a row of 513 cells spans workgroups
    "11_seventeen_frames_34x52": ((34, 52), 17, F64, (10, -4, 37, 37), 7),
    "12_feather_0_90x68": ((90, 68), 1, F64, (10, 20, 37, 37), 0),
    "12_feather_100_90x68": ((90, 68), 1, F64, (10, 20, 37, 37), 100),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_equals_the_definition(case):
    src_hw, T, frame_hw, rect, feather = CASES[case]
    src, frames = noise(1, *src_hw, 3).cuda(), noise(2, T, *frame_hw, 3).cuda()
    _, _, got = paste_raw(src, frames, rect, feather)
    held(case, got, definition(src_hw, T, frame_hw, rect, feather))


def test_box_that_misses_the_image_gives_the_converted_source():
    src_hw, T, frame_hw, rect, feather = CASES["07_box_misses_12x18"]
    want = hm.rgb8_to_i420(noise(1, *src_hw, 3))[None].expand(T, -1, -1)
    assert torch.equal(definition(src_hw, T, frame_hw, rect, feather), want)
    _, _, got = paste_raw(noise(1, *src_hw, 3).cuda(), noise(2, T, *frame_hw, 3).cuda(), rect, feather)
    held("box misses", got, want.contiguous())


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("case", ["02_fast_path_36x40_area", "01_odd_box_34x50_byte_path"])
def test_out_at_every_alignment(case, shift):
    """case 2 at offset 0 takes the dword / 16-bit stores, at 1 ... 3 the byte stores; case 1 takes the byte stores everywhere"""
    src_hw, T, frame_hw, rect, feather = CASES[case]
    _, _, got = paste_raw(noise(1, *src_hw, 3).cuda(), noise(2, T, *frame_hw, 3).cuda(), rect, feather, shift=shift)
    held("%s, out + %d" % (case, shift), got, definition(src_hw, T, frame_hw, rect, feather))


def test_whole_image_is_the_converted_plain_resize():
    frames = noise(2, 3, 64, 64, 3)
    for H, Wd in ((36, 40), (34, 50)):
        _, _, got = paste_raw(noise(1, H, Wd, 3).cuda(), frames.cuda(), (0, 0, Wd, H), 5)
        held("rect = whole image, %d x %d" % (H, Wd), got,
             hm.rgb8_to_i420(torch.stack([hm.resize_rgb8(frames[t], None, H, Wd) for t in range(3)])))


def test_two_runs_give_equal_bytes():
    src_hw, T, frame_hw, rect, feather = CASES["06_beyond_left_odd_offsets_90x68"]
    src, frames = noise(1, *src_hw, 3).cuda(), noise(2, T, *frame_hw, 3).cuda()
    assert torch.equal(paste_raw(src, frames, rect, feather)[2], paste_raw(src, frames, rect, feather)[2])


def test_bad_arguments_raise_and_launch_nothing():
    """`out` is poisoned and stays so: nothing was launched."""
    src, frames = noise(1, 34, 50, 3).cuda(), noise(2, 3, 64, 64, 3).cuda()
    L = pkg.native.lib()
    out = torch.full((3 * 51 * 50,), FILL, dtype=torch.uint8, device="cuda:0")

    def call(src_hw=(34, 50), T=3, fr=(64, 64), rect=(7, 5, 21, 19), feather=4, matrix=0, null=None):
        p = [C.c_void_p(src.data_ptr()), C.c_void_p(frames.data_ptr()), C.c_void_p(out.data_ptr())]
        if null is not None:
            p[null] = None
        rc = L.float_img_paste_i420(p[0], src_hw[0], src_hw[1], p[1], T, fr[0], fr[1], *rect, feather, matrix, p[2],
                                    pkg.native.stream_ptr(out.device))
        return rc, L.float_last_error().decode("utf-8", "replace") if rc else ""

    for kw, word in ((dict(src_hw=(33, 50)), "src_h"), (dict(src_hw=(34, 49)), "src_w"), (dict(src_hw=(0, 50)), "src_h"),
                     (dict(src_hw=(34, 16386)), "src_w"), (dict(matrix=1), "matrix"), (dict(T=0), "n_frames"), (dict(fr=(1025, 64)), "fr_h"),
                     (dict(fr=(64, 0)), "fr_w"), (dict(rect=(7, 5, 0, 19)), "rect_w"), (dict(rect=(7, 5, 21, 16385)), "rect_h"),
                     (dict(feather=-1), "feather"), (dict(feather=16385), "feather"), (dict(null=0), "null"), (dict(null=1), "null"),
                     (dict(null=2), "null")):
        rc, msg = call(**kw)
        assert rc == 1 and "float_img_paste_i420" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    with pytest.raises(ValueError) as e:
        pkg.native.check(call(matrix=1)[0])
    assert "matrix" in str(e.value)
    assert call() == (0, "")
    assert torch.equal(out.cpu().reshape(3, 51, 50), definition((34, 50), 3, F64, (7, 5, 21, 19), 4))


# ---------------------------------------------------------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------------------------------------------------------
def test_mirror_takes_host_and_device_tensors():
    src, frames, rect = noise(1, 36, 40, 3), noise(2, 2, 64, 64, 3), (5, 3, 16, 12)
    want = definition((36, 40), 2, F64, rect, 2)
    P = pkg.image.paste_frames_device
    for s, f in ((src, frames), (src.cuda(), frames), (src, frames.cuda()), (src.cuda(), frames.cuda())):
        got = P(s, f, rect, 2, out_format="i420")
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (2, 54, 40) and torch.equal(got.cpu(), want)
    assert torch.equal(P(src, frames, (5, 3, 33, 12), out_format="i420").cpu(), hm.paste_i420(src, frames, (5, 3, 33, 12), 33 // 16))  # default feather
    out = torch.empty(2, 54, 40, dtype=torch.uint8, device="cuda:0")
    assert P(src, frames, rect, 2, out=out, out_format="i420") is out and torch.equal(out.cpu(), want)
    rgb = torch.empty(2, 36, 40, 3, dtype=torch.uint8, device="cuda:0")
    for fmt in (None, "rgb"):  # the default is what it was
        assert P(src, frames, rect, 2, out=rgb, out_format=fmt) is rgb and torch.equal(rgb.cpu(), hm.paste_rgb8(src, frames, rect, 2))
    assert torch.equal(hm.rgb8_to_i420(rgb.cpu()), want)
    odd = noise(1, 90, 67, 3)
    for kw in (dict(out=rgb), dict(out=out[:1]), dict(out=out.cpu()), dict(out=out.reshape(2, 40, 54)), dict(src8=odd),
               dict(src8=noise(1, 35, 40, 3)), dict(out_format="nv12")):
        args = dict(src8=src, frames8=frames, rect=rect, feather=2, out_format="i420")
        args.update(kw)
        with pytest.raises(ValueError):
            P(**args)
    with pytest.raises(ValueError) as e:
        P(odd, frames, rect, 2, out_format="i420")
    assert "even" in str(e.value) and "90 x 67" in str(e.value)
    with pytest.raises(ValueError):
        P(src, frames, rect, 2, out=out)  # an I420-shaped out with the RGB format
    assert tuple(P(odd, frames, rect, 2).shape) == (2, 90, 67, 3)  # RGB keeps taking odd sides


# ---------------------------------------------------------------------------------------------------------------------------
# through the product: the synthetic 64-px agent of tests/test_img_front_gpu.py, the stub detector and the 400 x 300 portrait of
# tests/test_img_paste_gpu.py, a 1.4-s clip (35 frames)
# ---------------------------------------------------------------------------------------------------------------------------
SEED = 5
BOX = (100.0, 40.0, 250.0, 200.0, 0.99)  # the stub detector's box in the 360-px view of a 400 x 300 portrait
KW = dict(emo="happy", no_crop=False, seed=SEED)


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


def _audio60():
    return {"waveform": pkg.weights.synth_waveform(2.4, seed=10).reshape(1, 1, -1), "sample_rate": 16000}  # 60 frames: two windows


_clips = {}


def _face_clip(monkeypatch):
    """(img, infer_pasted(out_format="i420") of it, the definition's frames) on the face-crop route, computed once, never modified"""
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    _stub_detector(monkeypatch)
    img = image(12, 400, 300, 3)
    if "face" not in _clips:
        agent = _agent()
        got = agent.infer_pasted(img[None], _audio(), out_format="i420", **KW)
        pinned = got.is_pinned()
        s, a, place = agent.host_inputs_placed(img[None], _audio(), no_crop=False)
        crops = agent.infer_device(s, a, emo="happy", seed=SEED, out_dtype=torch.uint8)
        rect = _face_rect()
        assert tuple(place.rect) == rect
        want = hm.paste_i420(hm.image_to_rgb8(img), crops, rect, hm.default_feather(rect))
        _clips["face"] = (got.clone(), pinned, want)
    return (img,) + _clips["face"]


def test_agent_infer_pasted_i420_is_the_converted_rgb_clip(monkeypatch):
    img, got, pinned, want = _face_clip(monkeypatch)
    assert got.dtype == torch.uint8 and not got.is_cuda and pinned and tuple(got.shape) == (35, 600, 300)
    rgb = _agent().infer_pasted(img[None], _audio(), **KW)
    assert tuple(rgb.shape) == (35, 400, 300, 3)  # the default is what it was
    held("infer_pasted(out_format='i420') against rgb8_to_i420(infer_pasted())", got, hm.rgb8_to_i420(rgb))
    held("infer_pasted(out_format='i420') against the definition", got, want)
    out = torch.empty(35, 600, 300, dtype=torch.uint8, pin_memory=True)
    assert _agent().infer_pasted(img[None], _audio(), out=out, out_format="i420", **KW) is out and torch.equal(out, want)
    with pytest.raises(ValueError):
        _agent().infer_pasted(img[None], _audio(), out=torch.empty(35, 400, 300, 3, dtype=torch.uint8), out_format="i420", **KW)
    with pytest.raises(ValueError):
        _agent().infer_pasted(img[None], _audio(), out_format="nv12", **KW)


@pytest.mark.parametrize("slots", [2, 3])
def test_agent_stream_pasted_i420_concatenates_to_the_whole_clip(monkeypatch, slots):
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    _stub_detector(monkeypatch)
    agent, img = _agent(), image(12, 400, 300, 3)
    if "whole60" not in _clips:
        _clips["whole60"] = agent.infer_pasted(img[None], _audio60(), out_format="i420", **KW).clone()
    whole = _clips["whole60"]
    assert tuple(whole.shape) == (60, 600, 300)
    pinned, empty = [], torch.empty

    def spy(*a, **k):  # the ring's slots: what the stream allocates in pinned memory
        t = empty(*a, **k)
        if k.get("pin_memory") and t.dtype == torch.uint8 and t.dim() >= 3:
            pinned.append(t)
        return t

    monkeypatch.setattr(torch, "empty", spy)
    blocks = []
    for b in agent.stream_pasted(img[None], _audio60(), slots=slots, out_format="i420", **KW):
        assert b.frames.is_pinned() and b.frames.data_ptr() in {t.data_ptr() for t in pinned}
        blocks.append((b.first, b.last, b.frames.clone()))
    monkeypatch.setattr(torch, "empty", empty)
    assert [(f, l) for f, l, _ in blocks] == [(0, 50), (50, 60)]
    held("stream_pasted(out_format='i420'), %d slots" % slots, torch.cat([fr for _, _, fr in blocks]), whole)
    assert len(pinned) == slots and len({t.data_ptr() for t in pinned}) == slots  # exactly `slots` distinct pinned addresses
    assert all(tuple(t.shape) == (50, 600, 300) and t.dtype == torch.uint8 for t in pinned)  # 3 H W / 2 bytes per frame
    with pytest.raises(ValueError):
        agent.stream_pasted(img[None], _audio(), slots=1, out_format="i420", **KW)


def test_agent_write_y4m_pasted(monkeypatch):
    img, _, _, want = _face_clip(monkeypatch)
    agent = _agent()
    f = io.BytesIO()
    assert agent.write_y4m(f, img[None], _audio(), paste_back=True, **KW) == 35
    ref = io.BytesIO()
    with hm.Y4MWriter(ref, 300, 400, agent.opt.fps) as w:
        w.write(want)
    assert f.getvalue() == ref.getvalue()
    header = f.getvalue().partition(b"\n")[0].split()
    assert header[0] == b"YUV4MPEG2" and b"W300" in header and b"H400" in header
    assert len(f.getvalue()) == len(b" ".join(header)) + 1 + 35 * (6 + 600 * 300)


def test_agent_write_y4m_at_the_models_size(monkeypatch):
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    _stub_detector(monkeypatch)
    agent, img = _agent(), image(12, 400, 300, 3)
    s, a = agent.host_inputs(img[None], _audio(), no_crop=False)
    want = agent.infer_device(s, a, emo="happy", seed=SEED, out_format="i420")
    assert tuple(want.shape) == (35, 96, 64)
    f, ref = io.BytesIO(), io.BytesIO()
    assert agent.write_y4m(f, img[None], _audio(), fps=30, **KW) == 35
    hm.write_y4m(ref, want, 30)
    assert f.getvalue() == ref.getvalue() and b"W64 H64 F30:1" in f.getvalue()[:64]


def test_agent_i420_refuses_an_odd_sided_portrait(tmp_path):
    agent = _agent()
    img = image(23, 90, 67, 3)
    path = tmp_path / "never.y4m"
    kw = dict(emo="happy", no_crop=True, seed=SEED)
    for call in (lambda: agent.infer_pasted(img[None], _audio(), out_format="i420", **kw),
                 lambda: agent.stream_pasted(img[None], _audio(), out_format="i420", **kw),
                 lambda: agent.write_y4m(str(path), img[None], _audio(), paste_back=True, **kw)):
        with pytest.raises(ValueError) as e:
            call()
        assert "even" in str(e.value) and "90 x 67" in str(e.value)
    assert not path.exists()
    assert tuple(agent.infer_pasted(img[None], _audio(), **kw).shape) == (35, 90, 67, 3)  # the RGB form keeps taking it
