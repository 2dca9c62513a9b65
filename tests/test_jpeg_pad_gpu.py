"""float_jpg_encode_padded and the layers above it on the GPU: frames whose sides are no multiples of 16.  Every comparison is
bytes equality with the host definition under pad="edge", host_models.jpeg_encode_rgb8(..., pad="edge") (tests/test_jpeg_pad.py
pins that definition): there is no tolerance.

The shapes are the smallest at which the padded first stage can go wrong: sides that leave 1, 8, 9 and 15 of an MCU (8: Y blocks
wholly outside the image), one pixel, intervals that wrap around MCU rows ending in a partial MCU, a second pass that is the one
partial MCU, the geometry of 1080p, odd row and frame strides, frames at odd addresses, more frames than one group."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from tests.jpeg_util import avi_parts, fixtures
from tests.test_img_front_gpu import _agent, _audio, image
from tests.util import load_pkg

pkg = load_pkg()
HM = pkg.host_models
J = pkg.jpeg
pytestmark = pytest.mark.gpu
FIX = fixtures()
SEED = 5


def noise(seed, *shape):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def files_of(data, offsets):
    data, off = data.cpu().numpy(), offsets.cpu().tolist()
    assert off[0] == 0 and all(b > a for a, b in zip(off, off[1:]))
    return [data[a:b].tobytes() for a, b in zip(off, off[1:])]


def same_files(got, want):
    assert [len(g) for g in got] == [len(w) for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            first = next(k for k in range(len(w)) if g[k] != w[k])
            raise AssertionError("frame %d differs from byte %d of %d on" % (i, first, len(w)))


def check(frames, q, r, dev=None):
    """Device bytes of `frames` ((T, H, W, 3) or (H, W, 3) uint8 array; dev: the same frames already on the device) against the
    definition under pad="edge"."""
    want = HM.jpeg_encode_rgb8(frames, q, r, pad="edge")
    x = dev if dev is not None else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    got = files_of(*J.encode_jpeg_device(x, q, r, pad="edge"))
    same_files(got, want)
    return got


def at_odd_address(frames):
    """The frames on the device, contiguous, starting one byte past an allocation's base."""
    buf = torch.empty(frames.size + 1, dtype=torch.uint8, device="cuda")
    x = buf[1:].view(*frames.shape)
    x.copy_(torch.from_numpy(frames))
    assert x.data_ptr() % 2 == 1 and x.is_contiguous()
    return x


@pytest.mark.parametrize("q", [90, 100])
@pytest.mark.parametrize("hw", [(17, 33), (31, 47), (24, 40), (25, 41), (1, 1), (16, 17), (5, 64)])
def test_size_classes(hw, q):
    (f,) = check(noise(3, hw[0], hw[1], 3), q, None)
    at = f.index(b"\xff\xc0") + 5
    assert f[at:at + 4] == bytes((hw[0] >> 8, hw[0] & 255, hw[1] >> 8, hw[1] & 255))  # SOF0 carries the true sides


@pytest.mark.parametrize("r", [0, 1, 3, 5, None])
def test_intervals_wrap_around_rows_that_end_in_a_partial_mcu(r):
    check(noise(4, 33, 49, 3), 90, r)  # 3 x 4 MCUs, the last row and the last column partial


def test_second_pass_is_the_one_partial_mcu():
    check(noise(5, 17, 261, 3), 90, None)  # 17 MCUs per row: a pass of 16, then the partial one
    check(noise(5, 17, 261, 3), 100, 0)    # one interval of 34 MCUs: three passes, bits carried between them


def test_the_geometry_of_1080p_on_24_lines():
    check(noise(6, 24, 1920, 3), 90, None)  # 120 MCUs per row, H = 8 mod 16


def test_one_1080p_frame():
    yy, xx = np.mgrid[0:1080, 0:1920].astype(np.float64)
    img = np.stack([127.5 + 100 * np.sin(xx / 97.0) * np.cos(yy / 61.0), xx * 255.0 / 1919.0, 127.5 + 110 * np.sin((xx + yy) / 131.0)], -1)
    img = np.clip(np.rint(img) + np.random.RandomState(8).randint(-6, 7, img.shape), 0, 255).astype(np.uint8)
    (f,) = check(img, 90, None)
    assert f[:629] == HM.jpeg_header(1080, 1920, 90, 120, pad="edge")  # 68 intervals of one MCU row, 8 lines of the last one padding


def test_two_groups_odd_strides_and_odd_addresses():
    """19 frames of 33 x 49: two groups (16 + 3); 3 H W = 4851 is odd, so every second frame starts at an odd address."""
    batch = noise(9, 19, 33, 49, 3)
    first = check(batch, 90, None)
    assert check(batch, 90, None, dev=at_odd_address(batch)) == first  # and the other frames are the odd ones


def test_whole_mcus_at_an_odd_address():
    """Sides that are multiples of 16 from an odd address: the byte-load kernel, and the bytes of float_jpg_encode."""
    batch = np.stack([FIX["noise_32x48"], FIX["noise_32x48"][::-1].copy()])
    got = check(batch, 90, None, dev=at_odd_address(batch))
    assert got == HM.jpeg_encode_rgb8(batch, 90, None)


def test_reads_stay_inside_the_frames_that_are_encoded():
    """The first T frames of T + 1: a read past a row's end would pick up the next row, one past a frame the next frame."""
    batch = noise(10, 3, 17, 33, 3)
    x = torch.from_numpy(batch).cuda()
    want = HM.jpeg_encode_rgb8(batch[:2], 100, None, pad="edge")
    same_files(files_of(*J.encode_jpeg_device(x[:2], 100, None, pad="edge")), want)
    x[2] = 255 - x[2]  # whatever follows the encoded frames has no say
    same_files(files_of(*J.encode_jpeg_device(x[:2], 100, None, pad="edge")), want)
    same_files(files_of(*J.encode_jpeg_device(x[1:], 100, None, pad="edge")), HM.jpeg_encode_rgb8(x[1:].cpu(), 100, None, pad="edge"))


def test_whole_mcus_give_the_bytes_of_float_jpg_encode():
    big = noise(11, 512, 512, 3)
    for img, q in ((FIX["noise"], 90), (FIX["noise"], 100), (big, 100)):
        x = torch.from_numpy(img).cuda()
        for r in (None, 3):
            plain = files_of(*J.encode_jpeg_device(x, q, r))
            same_files(files_of(*J.encode_jpeg_device(x, q, r, pad="edge")), plain)
    same_files(plain, HM.jpeg_encode_rgb8(big, 100, 3))


def _raw(x, q, r, out, cap, offsets):
    L = pkg.native.lib()
    T, H, Wd, _ = x.shape
    work = torch.empty(int(L.float_jpg_work_bytes_padded(T, H, Wd, r)), dtype=torch.uint8, device="cuda")
    return L.float_jpg_encode_padded(C.c_void_p(x.data_ptr()), T, H, Wd, q, r, C.c_void_p(out.data_ptr()), cap, C.c_void_p(offsets.data_ptr()),
                                     C.c_void_p(work.data_ptr()), work.numel(), pkg.native.stream_ptr("cuda:0"))


def test_capacity_rule():
    batch = noise(12, 3, 33, 49, 3)
    want = HM.jpeg_encode_rgb8(batch, 90, None, pad="edge")
    blob = b"".join(want)
    x = torch.from_numpy(batch).cuda()
    cap = len(blob) // 2
    out = torch.full((len(blob) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert _raw(x, 90, 4, out, cap, offsets) == 0
    torch.cuda.synchronize()
    assert offsets.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()  # exact although nothing fits
    got = out.cpu().numpy()
    assert (got[cap:] == 0xA5).all()            # nothing at or beyond out + out_cap
    assert got[:cap].tobytes() == blob[:cap]    # what lies below is the files' prefix
    out.fill_(0xA5)
    assert _raw(x, 90, 4, out, 0, offsets) == 0  # no room at all
    torch.cuda.synchronize()
    assert offsets.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist() and (out.cpu() == 0xA5).all()
    # the wrapper: one read of the offsets, then once more with room
    small = torch.empty(cap, dtype=torch.uint8, device="cuda")
    data, off = J.encode_jpeg_device(x, 90, None, out=small, pad="edge")
    assert data is not small and data.numel() == len(blob) and files_of(data, off) == want
    roomy = torch.empty(len(blob) + 100, dtype=torch.uint8, device="cuda")
    data, off = J.encode_jpeg_device(x, 90, None, out=roomy, pad="edge")
    assert data is roomy and files_of(data, off) == want
    host = J.encode_jpeg_host(x, 90, None, pad="edge")
    assert [bytes(f) for f in host] == want


def test_two_calls_give_equal_bytes():
    x = torch.from_numpy(noise(13, 2, 33, 49, 3)).cuda()
    a, oa = J.encode_jpeg_device(x, 100, 1, pad="edge")
    b, ob = J.encode_jpeg_device(x, 100, 1, pad="edge")
    n = int(oa[-1])
    assert torch.equal(oa, ob) and torch.equal(a[:n], b[:n])


def test_invalid_arguments_are_refused_without_a_launch():
    L = pkg.native.lib()
    x = torch.zeros(1, 33, 49, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(int(L.float_jpg_work_bytes_padded(1, 33, 49, 2)), dtype=torch.uint8, device="cuda")
    assert work.numel() > 0
    st = pkg.native.stream_ptr("cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(h=33, w=49, q=90, r=2, xs=p(x), o=p(out), of=p(off), wk=p(work), wb=work.numel()):
        return L.float_jpg_encode_padded(xs, 1, h, w, q, r, o, out.numel(), of, wk, wb, st), L.float_last_error()

    for kw, word in ((dict(h=0), b"1 ... 16384"), (dict(w=0), b"1 ... 16384"), (dict(h=16385), b"1 ... 16384"), (dict(w=-16), b"1 ... 16384"),
                     (dict(q=0), b"quality"), (dict(q=101), b"quality"), (dict(xs=None), b"null"), (dict(o=None), b"null"),
                     (dict(of=None), b"null"), (dict(wk=None), b"null"), (dict(wb=work.numel() - 1), b"work_bytes"),
                     (dict(r=-1), b"restart"), (dict(r=70000), b"restart"), (dict(of=C.c_void_p(off.data_ptr() + 4)), b"8-byte"),
                     (dict(wk=C.c_void_p(work.data_ptr() + 8)), b"16-byte")):
        rc, msg = call(**kw)
        assert rc == 1 and word in msg and b"float_jpg_encode_padded" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all() and (off.cpu() == -1).all()  # nothing ran
    with pytest.raises(ValueError):
        J.encode_jpeg_device(x)  # the default still refuses
    with pytest.raises(ValueError):
        J.encode_jpeg_device(x, pad="zero")
    with pytest.raises(ValueError):
        J.encode_jpeg_device(x, quality=0, pad="edge")
    with pytest.raises(ValueError):
        J.encode_jpeg_device(x.cpu(), pad="edge")


# ---------------------------------------------------------------------------------------------------------------------------
# through the product: the synthetic 64-px agent of tests/test_img_front_gpu.py, the 90 x 67 portrait that
# tests/test_img_paste_gpu.py sees refused, a 1.4-s clip (35 frames)
# ---------------------------------------------------------------------------------------------------------------------------
def test_agent_pasted_jpeg_of_a_90_x_67_portrait(monkeypatch, tmp_path):
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    agent = _agent()
    img = image(23, 90, 67, 3)
    kw = dict(emo="happy", no_crop=True, seed=SEED)
    pasted = agent.infer_pasted(img[None], _audio(), **kw)
    assert tuple(pasted.shape) == (35, 90, 67, 3)
    want = HM.jpeg_encode_rgb8(pasted, 90, None, pad="edge")
    files = [bytes(f) for f in agent.infer_pasted_jpeg(img[None], _audio(), pad="edge", **kw)]
    same_files(files, want)
    streamed = [bytes(f) for b in agent.stream_pasted_jpeg(img[None], _audio(), pad="edge", **kw) for f in b.frames]
    same_files(streamed, want)
    q50 = [bytes(f) for f in agent.infer_pasted_jpeg(img[None], _audio(), quality=50, restart=3, pad="edge", **kw)]
    same_files(q50, HM.jpeg_encode_rgb8(pasted, 50, 3, pad="edge"))
    f = io.BytesIO()
    assert agent.write_video(f, img[None], _audio(), paste_back=True, pad="edge", **kw) == 35
    p = avi_parts(f.getvalue())
    assert (p["avih"][8], p["avih"][9]) == (67, 90) and p["video"][0] == want[0] and len(p["video"]) == 35
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(p["video"][0]))
    im.load()
    assert im.size == (67, 90) and im.mode == "RGB"


def test_agent_overflow_re_encode_pads_too(monkeypatch):
    """Room for 1024 bytes per slot and per whole-clip call: both routes take their second encode, under the same padding."""
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    agent = _agent()
    img = image(23, 90, 67, 3)
    kw = dict(emo="happy", no_crop=True, seed=SEED, pad="edge")
    want = [bytes(f) for f in agent.infer_pasted_jpeg(img[None], _audio(), **kw)]
    monkeypatch.setattr(pkg.jpeg, "default_capacity", lambda *a: 1024)
    assert [bytes(f) for b in agent.stream_pasted_jpeg(img[None], _audio(), **kw) for f in b.frames] == want
    assert [bytes(f) for f in agent.infer_pasted_jpeg(img[None], _audio(), **kw)] == want


def test_agent_without_the_keyword_still_refuses(tmp_path):
    agent = _agent()
    img = image(23, 90, 67, 3)
    path = tmp_path / "never.avi"
    kw = dict(emo="happy", no_crop=True, seed=SEED)
    for call in (lambda: agent.infer_pasted_jpeg(img[None], _audio(), **kw),
                 lambda: agent.stream_pasted_jpeg(img[None], _audio(), **kw),
                 lambda: agent.write_video(str(path), img[None], _audio(), paste_back=True, **kw),
                 lambda: agent.infer_pasted_jpeg(img[None], _audio(), pad=None, **kw)):
        with pytest.raises(ValueError) as e:
            call()
        assert "multiples of 16" in str(e.value)
    for call in (lambda: agent.infer_pasted_jpeg(img[None], _audio(), pad="zero", **kw),
                 lambda: agent.stream_pasted_jpeg(img[None], _audio(), pad="zero", **kw),
                 lambda: agent.write_video(str(path), img[None], _audio(), paste_back=True, pad="zero", **kw)):
        with pytest.raises(ValueError) as e:
            call()
        assert "pad" in str(e.value)
    assert not path.exists()
