"""float_img_resample on the GPU, and the paste routes with resample=: bicubic / Lanczos resampling of the generated 8-bit frames by
Pillow's fixed-point rule.  The kernels work in integers, so every comparison is torch.equal with the definition on the CPU,
host_models.resample_rgb8 / paste_rgb8 / paste_i420 (tests/test_img_resample.py holds those to Pillow itself) - no tolerance anywhere
in this file.

Crops are T = 3 frames of seeded uint8 noise, 64 x 64 unless the case says otherwise; `out` and `work` sit between guard bands.  The
cases are the smallest at which the two kernels can go wrong: a fractional phase, both passes and each one alone, wide taps
(shrinking), widths that are no multiple of the four pixels a lane stores (the byte-store path), windows on every edge of the box,
`out` at every byte offset from a dword boundary."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests.test_img_front_gpu import _agent, _audio, image
from tests.test_img_paste_gpu import SEED, _face_clip
from tests.util import load_pkg

pkg = load_pkg()
hm = pkg.host_models
pytestmark = pytest.mark.gpu

GUARD = 256  # bytes of guard band on each side of `out` and of `work`
FILL = 77
FILTERS = ("bicubic", "lanczos")


@functools.lru_cache(maxsize=None)
def noise(seed, *shape):
    """seeded uint8 noise; computed once, shared, never modified"""
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def resampled(T, frame_hw, h, w, filter, window=None):
    return hm.resample_rgb8(noise(2, T, *frame_hw, 3), h, w, filter, window)


def held(tag, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    bad = int((got != want).sum())
    print("%s: %d of %d bytes differ from the definition" % (tag, bad, want.numel()))
    assert torch.equal(got, want), tag


def resample_raw(frames, h, w, filter, window=None, shift=0, expect=0, override=()):
    """float_img_resample on a device tensor with guard bands around `out` - which starts `shift` bytes past a 256-byte boundary - and
    around `work`; returns (return code, message, the output on the host) after checking the bands.  override: arguments of the C
    call to replace, as a dict (for the refusals)."""
    L = pkg.native.lib()
    T, fh, fw = (int(v) for v in frames.shape[:3])
    xa, ya, wc, hc = (0, 0, w, h) if window is None else window
    fid = hm.RESAMPLE_FILTERS[filter]
    tab_x = pkg.image.resample_table(fw, w, filter, xa, wc).cuda() if fw != w else None
    tab_y = pkg.image.resample_table(fh, h, filter, ya, hc).cuda() if fh != h else None
    need = int(L.float_img_resample_work_bytes(T, fh, fw, h, w, fid, xa, ya, wc, hc))
    assert need >= 16 and need % 16 == 0
    n = T * hc * wc * 3
    buf = torch.full((n + 2 * GUARD + 8,), FILL, dtype=torch.uint8, device="cuda:0")
    work = torch.full((need + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    at = GUARD + shift
    a = dict(frames8=C.c_void_p(frames.data_ptr()), n_frames=T, fr_h=fh, fr_w=fw, box_h=h, box_w=w, filter=fid, win_x=xa, win_y=ya, win_w=wc,
             win_h=hc, tab_x=C.c_void_p(tab_x.data_ptr()) if tab_x is not None else None,
             tab_y=C.c_void_p(tab_y.data_ptr()) if tab_y is not None else None, work=C.c_void_p(work.data_ptr() + GUARD), work_bytes=need,
             out=C.c_void_p(buf.data_ptr() + at), stream=pkg.native.stream_ptr(buf.device))
    a.update(dict(override))
    rc = L.float_img_resample(*a.values())
    msg = L.float_last_error().decode("utf-8", "replace") if rc else ""
    assert rc == expect, (rc, msg)
    buf, work = buf.cpu(), work.cpu()
    assert bool((buf[:at] == FILL).all()) and bool((buf[at + n:] == FILL).all()), "guard band of out written"
    assert bool((work[:GUARD] == FILL).all()) and bool((work[GUARD + need:] == FILL).all()), "guard band of work written"
    if expect:
        assert bool((buf == FILL).all()) and bool((work == FILL).all()), "a refused call wrote"
    return rc, msg, buf[at:at + n].reshape(T, hc, wc, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels against the definition, bitwise
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (T, frame (h, w), result (h, w), window (xa, ya, wc, hc) or None)
CASES = {
    "fractional_phase_64_to_97": (3, (64, 64), (97, 97), None),
    "64_to_131x128": (3, (64, 64), (131, 128), None),                     # 64 x 64 -> 128 wide by 131 high: dword stores
    "shrink_48x64_to_29x41": (3, (48, 64), (29, 41), None),               # 64 x 48 -> 41 x 29: 9 and 11 taps
    "vertical_only_64x33_to_100x33": (3, (64, 33), (100, 33), None),      # 33 x 64 -> 33 x 100: the horizontal pass is dropped
    "horizontal_only_33x64_to_33x100": (3, (33, 64), (33, 100), None),    # 64 x 33 -> 100 x 33: the vertical pass is dropped
    "1x1_to_4x9": (3, (1, 1), (4, 9), None),
    "odd_frame_5x7_to_33x16": (3, (5, 7), (33, 16), None),                # 7 x 5 -> 16 x 33: rows of the frames at odd addresses
    "odd_width_64_to_50x23": (3, (64, 64), (50, 23), None),               # 23 columns: the byte-store path with both passes
    "one_frame": (1, (64, 64), (97, 97), None),
    "window_off_left_top": (3, (64, 64), (97, 97), (0, 0, 41, 30)),
    "window_off_right_bottom": (3, (64, 64), (97, 97), (57, 66, 40, 31)),
    "window_inside_dword_width": (3, (64, 64), (97, 97), (13, 17, 44, 29)),
    "window_of_a_huge_box": (3, (64, 64), (1 << 30, 1 << 30), ((1 << 29) - 20, (1 << 30) - 33, 40, 33)),
    "identity_window_is_a_copy": (3, (64, 64), (64, 64), (5, 6, 40, 31)),
    "two_blocks_of_cells_64_to_5x1100": (1, (64, 64), (5, 1100), (0, 0, 1100, 5)),  # 275 cells: more than one workgroup per row
}


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernels_equal_the_definition(case, filter):
    T, frame_hw, (h, w), window = CASES[case]
    _, _, got = resample_raw(noise(2, T, *frame_hw, 3).cuda(), h, w, filter, window)
    held("%s %s" % (case, filter), got, resampled(T, frame_hw, h, w, filter, window))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_out_at_every_alignment(shift):
    for case in ("64_to_131x128", "horizontal_only_33x64_to_33x100", "window_inside_dword_width"):  # widths that take dword stores at shift 0
        T, frame_hw, (h, w), window = CASES[case]
        _, _, got = resample_raw(noise(2, T, *frame_hw, 3).cuda(), h, w, "lanczos", window, shift=shift)
        held("%s, out + %d" % (case, shift), got, resampled(T, frame_hw, h, w, "lanczos", window))


def test_two_runs_give_equal_bytes():
    frames = noise(2, 3, 64, 64, 3).cuda()
    assert torch.equal(resample_raw(frames, 97, 97, "bicubic")[2], resample_raw(frames, 97, 97, "bicubic")[2])


def test_bad_arguments_raise_and_launch_nothing():
    """resample_raw checks that `out`, `work` and their guard bands stay at their fill: nothing was launched."""
    frames = noise(2, 3, 64, 64, 3).cuda()
    for kw, word in ((dict(n_frames=0), "n_frames"), (dict(fr_h=0), "fr_h"), (dict(fr_w=16385), "fr_w"), (dict(box_h=0), "box_h"),
                     (dict(box_w=(1 << 30) + 1), "box_w"), (dict(filter=2), "filter"), (dict(win_x=-1), "win_x"), (dict(win_y=1), "win_y"),
                     (dict(win_w=98), "win_w"), (dict(win_h=0), "win_h"), (dict(box_h=1, win_h=1), "255 taps"), (dict(frames8=None), "null"),
                     (dict(out=None), "null"), (dict(work=None), "null"), (dict(tab_x=None), "tab_x"), (dict(tab_y=None), "tab_y"),
                     (dict(work_bytes=15), "work_bytes")):
        rc, msg, _ = resample_raw(frames, 97, 97, "lanczos", expect=1, override=kw)
        assert "float_img_resample" in msg and word in msg, (kw, msg)
    with pytest.raises(ValueError) as e:
        pkg.native.check(resample_raw(frames, 97, 97, "lanczos", expect=1, override=dict(filter=7))[0])
    assert "filter" in str(e.value)
    held("after the refusals", resample_raw(frames, 97, 97, "lanczos")[2], resampled(3, (64, 64), 97, 97, "lanczos"))


def test_mirror_takes_host_and_device_tensors():
    frames = noise(2, 3, 64, 64, 3)
    want = resampled(3, (64, 64), 97, 97, "bicubic")
    for f in (frames, frames.cuda()):
        got = pkg.image.resample_frames_device(f, 97, 97, "bicubic")
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    win = (57, 66, 40, 31)
    out = torch.empty(3, 31, 40, 3, dtype=torch.uint8, device="cuda:0")
    assert pkg.image.resample_frames_device(frames, 97, 97, "bicubic", win, out=out) is out
    held("window, out=", out.cpu(), want[:, 66:97, 57:97])
    n_tables = len(pkg.image._resample_tables)
    pkg.image.resample_frames_device(frames, 97, 97, "bicubic", win, out=out)
    assert len(pkg.image._resample_tables) == n_tables  # the tables of a (sizes, window, filter) are made and uploaded once
    for args in ((frames.float(), 97, 97, "bicubic"), (frames[0], 97, 97, "bicubic"), (frames, 97, 97, "nearest"), (frames, 0, 97, "bicubic"),
                 (frames, 1, 97, "bicubic"), (frames, 97, 97, "bicubic", (0, 0, 98, 5)), (frames, 97, 97, "bicubic", None, out),
                 (frames, 97, 97, "bicubic", win, out.cpu())):
        with pytest.raises(ValueError):
            pkg.image.resample_frames_device(*args)


# ---------------------------------------------------------------------------------------------------------------------------
# paste_frames_device(..., resample=) against paste_rgb8 / paste_i420: portrait 96 x 128, crops 3 x 64 x 64
# ---------------------------------------------------------------------------------------------------------------------------
SRC_HW = (96, 128)
RECTS = {
    "inside": (20, 10, 75, 70),                       # four open sides
    "flush_left_top": (0, 0, 80, 70),
    "flush_right_bottom": (58, 19, 70, 77),
    "beyond_left": (-13, 10, 75, 70),
    "beyond_right": (70, 10, 75, 70),
    "beyond_top": (20, -9, 75, 70),
    "beyond_bottom": (20, 40, 75, 70),
    "larger_than_the_portrait": (-20, -30, 170, 150),
    "wholly_outside": (128, 10, 75, 70),
}
FEATHERS = (None, 0, 40)  # 40: more than half of the boxes' 70 rows


@functools.lru_cache(maxsize=None)
def pasted(rect, feather, filter):
    f = hm.default_feather(rect) if feather is None else feather
    return hm.paste_rgb8(noise(1, *SRC_HW, 3), noise(2, 3, 64, 64, 3), rect, f, resample=filter)


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("name", sorted(RECTS))
def test_paste_with_resample_equals_the_definition(name, filter, monkeypatch):
    src, frames, rect = noise(1, *SRC_HW, 3).cuda(), noise(2, 3, 64, 64, 3).cuda(), RECTS[name]
    calls = []
    real = pkg.image.resample_frames_device
    monkeypatch.setattr(pkg.image, "resample_frames_device", lambda *a, **k: calls.append(1) or real(*a, **k))
    for feather in FEATHERS:
        want = pasted(rect, feather, filter)
        got = pkg.image.paste_frames_device(src, frames, rect, feather, resample=filter)
        held("%s %s feather %r" % (name, filter, feather), got.cpu(), want)
        for matrix, mid in ((None, 0), ("bt709-full", 6)):
            yuv = pkg.image.paste_frames_device(src, frames, rect, feather, out_format="i420", matrix=matrix, resample=filter)
            held("%s %s feather %r i420 matrix %d" % (name, filter, feather, mid), yuv.cpu(), hm.rgb8_to_i420(want, mid))
    if name == "wholly_outside":  # the source comes back and nothing new is launched
        assert not calls
        held("outside", got.cpu(), noise(1, *SRC_HW, 3)[None].expand(3, -1, -1, -1))
    else:
        assert len(calls) == 9


def test_paste_i420_definition_and_scratch():
    """paste_i420 itself (not its RGB composition) for one case, and the caller-owned scratch: sized once, used for fewer frames."""
    src, frames, rect = noise(1, *SRC_HW, 3), noise(2, 3, 64, 64, 3), RECTS["beyond_right"]
    scratch = pkg.image.paste_scratch(SRC_HW, (64, 64), rect, 3, "lanczos", torch.device("cuda:0"))
    assert tuple(scratch.face.shape) == (3, 70, 58, 3)
    for n in (3, 2):
        got = pkg.image.paste_frames_device(src, frames[:n], rect, 5, out_format="i420", matrix=6, resample="lanczos", scratch=scratch)
        held("paste_i420, %d frames" % n, got.cpu(), hm.paste_i420(src, frames[:n], rect, 5, matrix="bt709-full", resample="lanczos"))
    assert pkg.image.paste_scratch(SRC_HW, (64, 64), RECTS["wholly_outside"], 3, "lanczos", torch.device("cuda:0")) is None
    assert pkg.image.paste_scratch(SRC_HW, (64, 64), rect, 3, None, torch.device("cuda:0")) is None
    other = pkg.image.paste_scratch(SRC_HW, (64, 64), RECTS["inside"], 3, "lanczos", torch.device("cuda:0"))
    for args, kw in (((src, frames, rect, 5), dict(resample="nearest")), ((src, frames, rect, 5), dict(resample="lanczos", scratch=other)),
                     ((src, frames, rect, 5), dict(resample="lanczos", scratch=pkg.image.paste_scratch(SRC_HW, (64, 64), rect, 2, "lanczos",
                                                                                                       torch.device("cuda:0"))))):
        with pytest.raises(ValueError):
            pkg.image.paste_frames_device(*args, **kw)
    assert torch.equal(pkg.image.paste_frames_device(src, frames, rect, 5, resample=None).cpu(), hm.paste_rgb8(src, frames, rect, 5))


def test_box_larger_than_the_paste_kernel_s_frame_limit():
    """A window of more than 1024 columns: the paste entry takes frames of the box's own size beyond its 1024-px frame limit."""
    src, frames = noise(4, 8, 1100, 3), noise(2, 1, 64, 64, 3)
    rect = (-10, -2, 1200, 12)
    got = pkg.image.paste_frames_device(src, frames, rect, 3, resample="bicubic")
    held("1100 columns", got.cpu(), hm.paste_rgb8(src, frames, rect, 3, resample="bicubic"))


# ---------------------------------------------------------------------------------------------------------------------------
# through the product: the synthetic 64-px agent of tests/test_img_front_gpu.py, a 1.4-s clip (35 frames)
# ---------------------------------------------------------------------------------------------------------------------------
_crops = {}


def _face_crops(monkeypatch):
    """(img, rect, the clip's uint8 crops) on the face-crop route, computed once and left unchanged"""
    img, rect, _ = _face_clip(monkeypatch)
    if "face" not in _crops:
        agent = _agent()
        s, a, place = agent.host_inputs_placed(img[None], _audio(), no_crop=False)
        assert tuple(place.rect) == rect
        _crops["face"] = agent.infer_device(s, a, emo="happy", seed=SEED, out_dtype=torch.uint8).cpu()
    return img, rect, _crops["face"]


def test_agent_infer_pasted_with_resample_equals_the_definition(monkeypatch):
    agent = _agent()
    img, rect, crops = _face_crops(monkeypatch)
    assert rect[2] > 64 and rect[0] + rect[2] > 300  # the box enlarges the crop and reaches past the right edge
    src8 = hm.image_to_rgb8(img)
    want = hm.paste_rgb8(src8, crops, rect, hm.default_feather(rect), resample="lanczos")
    got = agent.infer_pasted(img[None], _audio(), emo="happy", no_crop=False, seed=SEED, resample="lanczos")
    assert got.dtype == torch.uint8 and not got.is_cuda
    held("infer_pasted lanczos", got, want)
    assert not torch.equal(got, _face_clip(monkeypatch)[2])
    blocks = [b.frames.clone() for b in agent.stream_pasted(img[None], _audio(), emo="happy", no_crop=False, seed=SEED, resample="lanczos")]
    held("stream_pasted lanczos", torch.cat(blocks), want)


def test_agent_i420_with_resample_equals_paste_i420(monkeypatch):
    agent = _agent()
    img, rect, crops = _face_crops(monkeypatch)
    got = agent.infer_pasted(img[None], _audio(), emo="happy", no_crop=False, seed=SEED, out_format="i420", matrix="bt709-full", resample="bicubic")
    held("infer_pasted i420 bicubic", got, hm.paste_i420(hm.image_to_rgb8(img), crops, rect, hm.default_feather(rect), matrix="bt709-full",
                                                         resample="bicubic"))


def test_agent_resample_none_is_the_call_without_the_keyword(monkeypatch):
    agent = _agent()
    img, rect, old = _face_clip(monkeypatch)
    kw = dict(emo="happy", no_crop=False, seed=SEED)
    held("infer_pasted", agent.infer_pasted(img[None], _audio(), resample=None, **kw), old)
    held("stream_pasted", torch.cat([b.frames.clone() for b in agent.stream_pasted(img[None], _audio(), resample=None, **kw)]), old)
    held("i420", agent.infer_pasted(img[None], _audio(), out_format="i420", resample=None, **kw),
         agent.infer_pasted(img[None], _audio(), out_format="i420", **kw))


def test_agent_files_with_resample(monkeypatch):
    """JPEG and PNG files of a 96 x 80 portrait with no_crop: the box is the whole image, 64 -> 80 by 64 -> 96."""
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    agent = _agent()
    img = image(22, 96, 80, 3)
    kw = dict(emo="happy", no_crop=True, seed=SEED)
    s, a = agent.host_inputs(img[None], _audio(), no_crop=True)
    crops = agent.infer_device(s, a, emo="happy", seed=SEED, out_dtype=torch.uint8).cpu()
    want = hm.paste_rgb8(hm.image_to_rgb8(img), crops, (0, 0, 80, 96), 5, resample="lanczos")
    held("no_crop is the plain resample", want, hm.resample_rgb8(crops, 96, 80, "lanczos"))
    files = agent.infer_pasted_jpeg(img[None], _audio(), resample="lanczos", **kw)
    assert [bytes(f) for f in files] == [bytes(f) for f in hm.jpeg_encode_rgb8(want, 90, 80 // 16)]
    pngs = agent.infer_pasted_png(img[None], _audio(), resample="lanczos", **kw)
    assert len(pngs) == 35
    for i, f in enumerate(pngs):
        assert np.array_equal(np.array(Image.open(io.BytesIO(bytes(f))).convert("RGB")), want[i].numpy()), i


def test_agent_files_with_resample_none_are_the_old_files(monkeypatch):
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    agent = _agent()
    img = image(22, 96, 80, 3)
    kw = dict(emo="happy", no_crop=True, seed=SEED)
    assert [bytes(f) for f in agent.infer_pasted_jpeg(img[None], _audio(), resample=None, **kw)] == \
        [bytes(f) for f in agent.infer_pasted_jpeg(img[None], _audio(), **kw)]
    assert [bytes(f) for f in agent.infer_pasted_png(img[None], _audio(), resample=None, **kw)] == \
        [bytes(f) for f in agent.infer_pasted_png(img[None], _audio(), **kw)]


def test_agent_refuses_resample_at_the_call(tmp_path):
    agent = _agent()
    img = image(22, 96, 80, 3)
    kw = dict(emo="happy", no_crop=True, seed=SEED)
    paths = [tmp_path / n for n in ("never.avi", "never.y4m", "never.png")]
    calls = [lambda r: agent.infer_pasted(img[None], _audio(), resample=r, **kw), lambda r: agent.stream_pasted(img[None], _audio(), resample=r, **kw),
             lambda r: agent.infer_pasted_jpeg(img[None], _audio(), resample=r, **kw),
             lambda r: agent.stream_pasted_jpeg(img[None], _audio(), resample=r, **kw),
             lambda r: agent.infer_pasted_png(img[None], _audio(), resample=r, **kw),
             lambda r: agent.stream_pasted_png(img[None], _audio(), resample=r, **kw),
             lambda r: agent.write_video(str(paths[0]), img[None], _audio(), paste_back=True, resample=r, **kw),
             lambda r: agent.write_y4m_matrix(str(paths[1]), img[None], _audio(), paste_back=True, resample=r, **kw),
             lambda r: agent.write_apng(str(paths[2]), img[None], _audio(), paste_back=True, resample=r, **kw)]
    for call in calls:
        with pytest.raises(ValueError) as e:
            call("nearest")
        assert "resample" in str(e.value)
    for call in (lambda: agent.write_video(str(paths[0]), img[None], _audio(), paste_back=False, resample="lanczos", **kw),
                 lambda: agent.write_y4m_matrix(str(paths[1]), img[None], _audio(), paste_back=False, resample="lanczos", **kw),
                 lambda: agent.write_apng(str(paths[2]), img[None], _audio(), paste_back=False, resample="lanczos", **kw)):
        with pytest.raises(ValueError) as e:
            call()
        assert "paste_back" in str(e.value)
    assert not any(p.exists() for p in paths)
    agent.G.require_no_stream("after the refusals")  # nothing was left open
    f = io.BytesIO()
    assert agent.write_video(f, img[None], _audio(), paste_back=True, resample="bicubic", **kw) == 35
