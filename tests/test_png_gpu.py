"""float_png_encode on the GPU.  Every comparison is bytes equality with the host definition host_models.png_encode_rgb8
(tests/test_png.py pins that definition against Pillow and zlib): there is no tolerance.

The shapes are the smallest at which the kernels can go wrong: the 64 x 64 fixtures at one row, three rows (a short last band),
the default and the whole frame per band (12352 bytes: four passes of 4096, the last one short); one pixel; odd sizes whose rows
are no multiples of 4 bytes; more frames than one group of 16; a band of 16 rows x 2048 pixels (98320 bytes would pass the band
limit, so it is cut at 10 rows: 61450 bytes, sixteen passes)."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.jpeg_util import fixtures
from tests.util import golden, load_pkg

pkg = load_pkg()
W = pkg.weights
HM = pkg.host_models
P = pkg.png
pytestmark = pytest.mark.gpu
FIX = fixtures()


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


def check(frames, band, dev=None):
    """Device bytes, offsets and CRCs of `frames` ((T, H, W, 3) or (H, W, 3) uint8 array; dev: the same frames already on the
    device) against the definition."""
    want = HM.png_encode_rgb8(frames, band)
    x = dev if dev is not None else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    data, offsets, crcs = P.encode_png_device(x, band)
    got = files_of(data, offsets)
    same_files(got, want)
    assert offsets.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()
    assert (crcs.cpu().to(torch.int64) & 0xFFFFFFFF).tolist() == [zlib.crc32(w[41:-16]) for w in want]
    return got


@pytest.mark.parametrize("name", sorted(FIX))
def test_fixtures_are_the_definitions_bytes(name):
    img = FIX[name]
    for band in (1, 3, None, img.shape[0]):
        check(img, band)


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (33, 17)])
def test_odd_sizes(shape):
    img = noise(21, *shape, 3)
    for band in (1, 2, None, shape[0]):
        check(img, min(band, shape[0]) if band else band)
    smooth = (np.add.outer(np.arange(shape[0]) * 5, np.arange(shape[1]) * 3)[..., None] + np.array([0, 40, 90])).astype(np.uint8)
    check(smooth, None)


def test_more_frames_than_one_group():
    """17 frames: two groups of the operator (16 + 1) sharing its scratch; the second group's offsets continue the first's."""
    base = FIX["noise_32x48"]
    batch = np.stack([np.roll(base, 3 * i, axis=1) if i % 2 else np.roll(FIX["smooth"][:32, :48], i, axis=0) for i in range(17)])
    check(batch, None)
    check(batch, 5)


def test_a_band_of_several_passes():
    """16 x 2048: a row is 6145 bytes, more than one pass of 4096; the default band is 8 rows (49160 bytes, 13 passes) and 10 rows
    is the most the band limit takes (61450 bytes)."""
    yy, xx = np.mgrid[0:16, 0:2048]
    img = np.stack([xx // 8 + yy, (xx * 7 + yy * 3) // 16, 255 - xx // 9], -1).astype(np.int64)
    img = np.clip(img % 256 + np.random.RandomState(4).randint(-2, 3, img.shape), 0, 255).astype(np.uint8)
    img[4:6] = noise(5, 2, 2048, 3)  # two rows that take the flat table's long codes
    check(img, None)
    check(img, 10)
    assert HM.png_default_band(16, 2048) == 8
    with pytest.raises(ValueError):
        P.encode_png_device(torch.from_numpy(img).cuda(), 11)


def _raw(x, band, out, cap, offsets, crcs=None):
    L = pkg.native.lib()
    T, H, Wd, _ = x.shape
    work = torch.empty(int(L.float_png_work_bytes(T, H, Wd, band)), dtype=torch.uint8, device="cuda")
    return L.float_png_encode(C.c_void_p(x.data_ptr()), T, H, Wd, band, C.c_void_p(out.data_ptr()), cap, C.c_void_p(offsets.data_ptr()),
                              C.c_void_p(crcs.data_ptr()) if crcs is not None else None, C.c_void_p(work.data_ptr()), work.numel(),
                              pkg.native.stream_ptr("cuda:0"))


def test_capacity_rule():
    batch = np.stack([FIX["noise"], FIX["patch"], FIX["extremes"]])
    want = HM.png_encode_rgb8(batch, 8)
    blob = b"".join(want)
    x = torch.from_numpy(batch).cuda()
    cap = len(blob) // 2 + 1
    out = torch.full((len(blob) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert _raw(x, 8, out, cap, offsets) == 0  # crcs is optional
    torch.cuda.synchronize()
    assert offsets.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()  # exact although not everything fits
    got = out.cpu().numpy()
    assert (got[cap:] == 0xA5).all()            # nothing at or beyond out + out_cap
    assert got[:cap].tobytes() == blob[:cap]    # what lies below is the files' prefix
    out.fill_(0xA5)
    assert _raw(x, 8, out, 0, offsets) == 0     # no room at all
    torch.cuda.synchronize()
    assert offsets.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist() and (out.cpu() == 0xA5).all()
    # the wrapper: one read of the offsets, then once more with room - the second call completes
    small = torch.empty(cap, dtype=torch.uint8, device="cuda")
    data, off, crcs = P.encode_png_device(x, 8, out=small)
    assert data is not small and data.numel() == len(blob) and files_of(data, off) == want
    roomy = torch.empty(len(blob) + 100, dtype=torch.uint8, device="cuda")
    data, off, crcs = P.encode_png_device(x, 8, out=roomy)
    assert data is roomy and files_of(data, off) == want
    host = P.encode_png_host(x, 8)
    assert [bytes(f) for f in host] == want and host.data.is_pinned() and host.nbytes == len(blob)
    assert host.crcs.tolist() == [zlib.crc32(w[41:-16]) for w in want]
    # noise needs more than the default room, the frames' raw size: the wrapper's second call gave these bytes
    (f,) = check(FIX["noise"], None)
    assert len(f) > FIX["noise"].size


def test_two_calls_give_equal_bytes():
    x = torch.from_numpy(np.stack([FIX["noise"], FIX["patch"], FIX["smooth_noise"]])).cuda()
    a, oa, ca = P.encode_png_device(x, 3)
    b, ob, cb = P.encode_png_device(x, 3)
    n = int(oa[-1])
    assert torch.equal(oa, ob) and torch.equal(a[:n], b[:n]) and torch.equal(ca, cb)


def test_frames_at_an_odd_address():
    batch = np.stack([FIX["patch"][:33, :17], FIX["smooth_noise"][:33, :17]])
    buf = torch.zeros(batch.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(batch.reshape(-1)).cuda()
    dev = buf[1:].view(2, 33, 17, 3)
    assert dev.data_ptr() % 2 == 1
    check(batch, None, dev)
    check(batch, 4, dev)


def test_invalid_arguments_are_refused_without_a_launch():
    L = pkg.native.lib()
    x = torch.zeros(1, 33, 17, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(int(L.float_png_work_bytes(1, 33, 17, 8)), dtype=torch.uint8, device="cuda")
    assert work.numel() > 0
    st = pkg.native.stream_ptr("cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(h=33, w=17, band=8, xs=p(x), o=p(out), of=p(off), wk=p(work), wb=work.numel()):
        return L.float_png_encode(xs, 1, h, w, band, o, out.numel(), of, None, wk, wb, st), L.float_last_error()

    for kw, word in ((dict(h=0), b"sides h x w"), (dict(w=16385), b"sides h x w"), (dict(band=34), b"band"), (dict(xs=None), b"null"),
                     (dict(o=None), b"null"), (dict(of=None), b"null"), (dict(wk=None), b"null"), (dict(wb=work.numel() - 1), b"work_bytes")):
        rc, msg = call(**kw)
        assert rc == 1 and word in msg and b"float_png_encode" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all() and (off.cpu() == -1).all()  # nothing ran
    with pytest.raises(ValueError):
        P.encode_png_device(x, band=34)
    with pytest.raises(ValueError):
        P.encode_png_device(x.float())
    with pytest.raises(ValueError):
        P.encode_png_device(x.cpu())


def test_decoder_decode_png():
    g = golden("dec_64")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(64, seed=g["seed"]), 64, 512, "cuda:0", max_frames=2)  # 3 frames in batches of 2
    try:
        dec.set_feats(W.synth_feats(64, seed=g["seed"]))
        s_r, r_d = g["s_r"], g["r_d"]
        u8 = dec.decode_u8(s_r, r_d).cpu()
        assert u8.shape[0] == 3
        for band in (None, 5):
            data, off, crcs = dec.decode_png(s_r, r_d, band)
            assert files_of(data, off) == HM.png_encode_rgb8(u8, band)
    finally:
        dec.close()
