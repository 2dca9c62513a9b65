"""float_jpg_encode and the layers above it on the GPU.  Every comparison is bytes equality with the host definition
host_models.jpeg_encode_rgb8: there is no tolerance."""
import ctypes as C
import importlib
import io

import numpy as np
import pytest
import torch

from tests.jpeg_util import avi_parts, fixtures
from tests.util import golden, load_pkg

pkg = load_pkg()
W = pkg.weights
HM = pkg.host_models
J = pkg.jpeg
pytestmark = pytest.mark.gpu
FIX = fixtures()
_state = {}


def files_of(data, offsets):
    data, off = data.cpu().numpy(), offsets.cpu().tolist()
    assert off[0] == 0 and all(b > a for a, b in zip(off, off[1:]))
    return [data[a:b].tobytes() for a, b in zip(off, off[1:])]


def check(frames, q, r):
    """Device bytes of `frames` ((T, H, W, 3) or (H, W, 3) uint8 array) against the definition."""
    want = HM.jpeg_encode_rgb8(frames, q, r)
    data, offsets = J.encode_jpeg_device(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), q, r)
    got = files_of(data, offsets)
    assert [len(g) for g in got] == [len(w) for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            first = next(k for k in range(len(w)) if g[k] != w[k])
            raise AssertionError("frame %d differs from byte %d of %d on" % (i, first, len(w)))
    return got


@pytest.mark.parametrize("q", [50, 90, 100])
@pytest.mark.parametrize("name", sorted(FIX))
def test_fixtures_are_the_definitions_bytes(name, q):
    img = FIX[name]
    for r in (0, 1, 3, None):
        check(img, q, r)


def test_batch_of_three_frames():
    batch = np.stack([FIX["noise"], FIX["extremes"], FIX["smooth_noise"]])
    for q, r in ((90, None), (100, 1), (50, 0), (90, 5)):
        check(batch, q, r)


def test_more_frames_than_one_group():
    """19 frames: two groups of the operator (16 + 3) sharing its scratch; the second group's offsets continue the first's."""
    rng = np.random.RandomState(7)
    base = [FIX[n] for n in ("noise", "extremes", "smooth_noise", "patch", "smooth")]
    batch = np.stack([np.roll(base[i % 5], rng.randint(0, 64), axis=1) for i in range(19)])
    check(batch, 90, None)


def test_512_noise_quality_100():
    """192 blocks per interval: two passes of 16 MCUs per workgroup, the bits carried between them, and the largest slots."""
    img = np.random.RandomState(11).randint(0, 256, (512, 512, 3)).astype(np.uint8)
    (f,) = check(img, 100, None)
    assert len(f) > 512 * 512  # beyond the default room too: the wrapper's second call gave these bytes


def test_256_smooth_noise_quality_90():
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float64)
    img = np.stack([127.5 + 100 * np.sin(xx / 31.0) * np.cos(yy / 23.0), xx, 127.5 + 110 * np.sin((xx + yy) / 41.0)], -1)
    img = np.clip(np.rint(img) + np.random.RandomState(12).randint(-6, 7, img.shape), 0, 255).astype(np.uint8)
    check(img, 90, None)
    check(img, 90, 20)  # intervals that wrap around the ends of MCU rows, two passes each


def _raw_encode(x, q, r, out, cap, offsets):
    L = pkg.native.lib()
    T, H, Wd, _ = x.shape
    work = torch.empty(int(L.float_jpg_work_bytes(T, H, Wd, r)), dtype=torch.uint8, device="cuda")
    return L.float_jpg_encode(C.c_void_p(x.data_ptr()), T, H, Wd, q, r, C.c_void_p(out.data_ptr()), cap, C.c_void_p(offsets.data_ptr()),
                              C.c_void_p(work.data_ptr()), work.numel(), pkg.native.stream_ptr("cuda:0"))


def test_capacity_rule():
    batch = np.stack([FIX["noise"], FIX["patch"], FIX["extremes"]])
    want = HM.jpeg_encode_rgb8(batch, 90, None)
    blob = b"".join(want)
    x = torch.from_numpy(batch).cuda()
    cap = len(blob) // 2
    out = torch.full((len(blob) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert _raw_encode(x, 90, 4, out, cap, offsets) == 0
    torch.cuda.synchronize()
    assert offsets.cpu().tolist() == [0] + np.cumsum([len(w) for w in want]).tolist()  # exact although nothing fits
    got = out.cpu().numpy()
    assert (got[cap:] == 0xA5).all()            # nothing at or beyond out + out_cap
    assert got[:cap].tobytes() == blob[:cap]    # what lies below is the files' prefix
    # the wrapper: one read of the offsets, then once more with room
    small = torch.empty(cap, dtype=torch.uint8, device="cuda")
    data, off = J.encode_jpeg_device(x, 90, None, out=small)
    assert data is not small and data.numel() == len(blob) and files_of(data, off) == want
    roomy = torch.empty(len(blob) + 100, dtype=torch.uint8, device="cuda")
    data, off = J.encode_jpeg_device(x, 90, None, out=roomy)
    assert data is roomy and files_of(data, off) == want


def test_two_calls_give_equal_bytes():
    x = torch.from_numpy(np.stack([FIX["noise"], FIX["patch"]])).cuda()
    a, oa = J.encode_jpeg_device(x, 100, 1)
    b, ob = J.encode_jpeg_device(x, 100, 1)
    n = int(oa[-1])
    assert torch.equal(oa, ob) and torch.equal(a[:n], b[:n])


def test_invalid_arguments_are_refused_without_a_launch():
    L = pkg.native.lib()
    x = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(int(L.float_jpg_work_bytes(1, 32, 32, 2)), dtype=torch.uint8, device="cuda")
    st = pkg.native.stream_ptr("cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(h=32, w=32, q=90, r=2, xs=p(x), o=p(out), of=p(off), wk=p(work), wb=work.numel()):
        return L.float_jpg_encode(xs, 1, h, w, q, r, o, out.numel(), of, wk, wb, st), L.float_last_error()

    for kw, word in ((dict(h=24), b"multiples of 16"), (dict(w=40), b"multiples of 16"), (dict(q=0), b"quality"), (dict(q=101), b"quality"),
                     (dict(xs=None), b"null"), (dict(o=None), b"null"), (dict(of=None), b"null"), (dict(wk=None), b"null"),
                     (dict(wb=work.numel() - 1), b"work_bytes"), (dict(r=-1), b"restart"), (dict(r=70000), b"restart")):
        rc, msg = call(**kw)
        assert rc == 1 and word in msg, (kw, msg)
    assert L.float_jpg_work_bytes(1, 24, 32, 2) == 0 and L.float_jpg_work_bytes(0, 32, 32, 2) == 0
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all() and (off.cpu() == -1).all()  # nothing ran
    with pytest.raises(ValueError):
        J.encode_jpeg_device(torch.zeros(24, 32, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        J.encode_jpeg_device(x, quality=0)
    with pytest.raises(ValueError):
        J.encode_jpeg_device(x.float())
    with pytest.raises(ValueError):
        J.encode_jpeg_device(x.cpu())


def test_decoder_decode_jpeg():
    g = golden("dec_64")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(64, seed=g["seed"]), 64, 512, "cuda:0", max_frames=2)  # 3 frames in batches of 2
    try:
        dec.set_feats(W.synth_feats(64, seed=g["seed"]))
        s_r, r_d = g["s_r"], g["r_d"]
        u8 = dec.decode_u8(s_r, r_d).cpu()
        assert u8.shape[0] == 3
        for q, r in ((90, None), (100, 1)):
            data, off = dec.decode_jpeg(s_r, r_d, q, r)
            assert files_of(data, off) == HM.jpeg_encode_rgb8(u8, q, r)
    finally:
        dec.close()


# ---------------------------------------------------------------------------------------------------------------------------
# through the product: the synthetic 64-px agent of tests/test_dec_u8_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------
SEED = 7


def _agent():
    if "agent" not in _state:
        gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
        opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
        opt.input_size, opt.nfe = 64, 6
        cfg = pkg.config.FmtConfig.from_options(opt)
        acfg = pkg.config.small_audio_config()
        acfg.dim_w = opt.dim_w
        parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
                     audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
        _state["agent"] = gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8)
        _state["img"] = torch.from_numpy(np.random.RandomState(5).rand(1, 3, 64, 64).astype(np.float32)).cuda() * 2 - 1
        _state["wav35"] = W.synth_waveform(1.4, seed=9).cuda()   # 35 frames: one window
        _state["wav60"] = W.synth_waveform(2.4, seed=10).cuda()  # 60 frames: two windows, the second short
        _state["wav185"] = W.synth_waveform(7.4, seed=10).cuda()  # 185 frames: four windows, the last short
    return _state["agent"]


def _whole(wav):
    """infer_device_jpeg of a clip as a list of bytes, computed once and left unchanged."""
    if ("jpeg", wav) not in _state:
        agent = _agent()
        fr = agent.infer_device_jpeg(_state["img"], _state[wav], 2.0, 1.0, 1.0, emo="happy", seed=SEED)
        assert fr.data.is_pinned() and fr.data.dtype == torch.uint8 and fr.offsets.dtype == torch.int64 and not fr.offsets.is_cuda
        assert fr.nbytes == int(fr.offsets[-1]) == sum(len(f) for f in fr)
        _state[("jpeg", wav)] = [bytes(f) for f in fr]
    return _state[("jpeg", wav)]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for v in ("FLOAT_AMD_VERIFY", "FLOAT_AMD_VERIFY_ACTION", "FLOAT_AMD_VERIFY_FRAMES", "FLOAT_AMD_VERIFY_PSNR", "FLOAT_AMD_OVERLAP"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FLOAT_AMD_NOISE", "cpu")


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    agent = _state.pop("agent", None)
    if agent is not None:
        agent.offload()
    _state.clear()


def test_agent_jpeg_is_the_definition_of_the_u8_frames():
    agent = _agent()
    got = _whole("wav35")
    u8 = agent.infer_device(_state["img"], _state["wav35"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, out_dtype=torch.uint8)
    assert tuple(u8.shape) == (35, 64, 64, 3) and got == HM.jpeg_encode_rgb8(u8, 90, None)
    q50 = agent.infer_device_jpeg(_state["img"], _state["wav35"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, quality=50, restart=1)
    assert [bytes(f) for f in q50] == HM.jpeg_encode_rgb8(u8, 50, 1)


@pytest.mark.parametrize("slots", [2, 3])
def test_stream_blocks_are_the_whole_clip(slots):
    agent = _agent()
    want = _whole("wav60")
    assert len(want) == 60
    got, spans = [], []
    for blk in agent.stream_device_jpeg(_state["img"], _state["wav60"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, slots=slots):
        assert blk.frames.data.is_pinned() and len(blk.frames) == blk.last - blk.first
        spans.append((blk.first, blk.last))
        got += [bytes(f) for f in blk.frames]
    assert spans == [(0, 50), (50, 60)] and got == want


@pytest.mark.parametrize("slots", [2, 3])
def test_jpeg_ring_is_bounded_and_no_slot_is_written_before_it_is_given_back(slots):
    """The ring contract of tests/test_stream_gpu.py for the JPEG sink: 7.4 s = 185 frames = 4 windows (last block 35) through
    `slots` slots - the smallest clip with more windows than slots and a short tail.  On receiving a block the whole device is
    synchronised, so that everything the generator has enqueued ahead has landed, and only then are its files compared with the
    same rows of infer_device_jpeg; exactly `slots` distinct pinned addresses, blocks k and k + slots share one."""
    agent = _agent()
    want = _whole("wav185")
    assert len(want) == 185
    ptrs, spans = [], []
    for blk in agent.stream_device_jpeg(_state["img"], _state["wav185"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, slots=slots):
        torch.cuda.synchronize()
        assert [bytes(f) for f in blk.frames] == want[blk.first:blk.last], (slots, blk.first)
        ptrs.append(blk.frames.data.data_ptr())
        spans.append((blk.first, blk.last))
    assert spans == [(0, 50), (50, 100), (100, 150), (150, 185)]
    assert len(set(ptrs)) == slots
    assert all(ptrs[k] == ptrs[k + slots] for k in range(4 - slots))


def test_stream_overflow_is_encoded_once_more(monkeypatch):
    """Room for 1024 bytes per slot and per whole-clip call: every block of the stream takes "the files did not fit: once more,
    with room", behind the windows already enqueued, and the whole-clip call takes its own second encode.  float_jpg_encode
    reports exact offsets when nothing fits (test_capacity_rule), so both give the files of the roomy run - and so does a plain
    call after the patch has gone."""
    agent = _agent()
    want = _whole("wav60")
    args = (_state["img"], _state["wav60"], 2.0, 1.0, 1.0)
    with monkeypatch.context() as m:
        m.setattr(pkg.jpeg, "default_capacity", lambda *a: 1024)
        got = []
        for blk in agent.stream_device_jpeg(*args, emo="happy", seed=SEED, slots=2):
            assert blk.frames.nbytes > 1024
            got += [bytes(f) for f in blk.frames]
        assert got == want
        assert [bytes(f) for f in agent.infer_device_jpeg(*args, emo="happy", seed=SEED)] == want
    assert [bytes(f) for f in agent.infer_device_jpeg(*args, emo="happy", seed=SEED)] == want


def test_stream_left_early_and_one_stream_at_a_time():
    agent = _agent()
    want = _whole("wav60")
    args = (_state["img"], _state["wav60"], 2.0, 1.0, 1.0)
    it = agent.stream_device_jpeg(*args, emo="happy", seed=SEED)
    first = next(it)
    assert [bytes(f) for f in first.frames] == want[:50]
    with pytest.raises(RuntimeError, match="still open"):
        agent.infer_device_jpeg(*args, emo="happy", seed=SEED)
    with pytest.raises(RuntimeError, match="still open"):
        agent.infer_device(*args, emo="happy", seed=SEED)
    with pytest.raises(RuntimeError, match="still open"):
        agent.stream_device_jpeg(*args, emo="happy", seed=SEED)
    it.close()  # left early: the agent is usable
    again = agent.infer_device_jpeg(*args, emo="happy", seed=SEED)
    assert [bytes(f) for f in again] == want
    with pytest.raises(ValueError):
        agent.stream_device_jpeg(*args, emo="happy", seed=SEED, slots=1)
    with pytest.raises(ValueError):
        agent.stream_device_jpeg(*args, emo="happy", seed=SEED, quality=0)


def test_write_video(tmp_path):
    agent = _agent()
    g = torch.Generator().manual_seed(0)
    img = torch.rand(1, 64, 64, 3, generator=g)
    audio = {"waveform": W.synth_waveform(1.4, seed=11).reshape(1, 1, -1).cpu(), "sample_rate": 16000}
    s, a = agent.host_inputs(img, audio, no_crop=True)
    want = [bytes(f) for f in agent.infer_device_jpeg(s, a, emo="happy", seed=SEED)]
    path = str(tmp_path / "clip.avi")
    assert agent.write_video(path, img, audio, emo="happy", no_crop=True, seed=SEED) == 35 == len(want)
    p = avi_parts(open(path, "rb").read())
    assert p["video"] == want and p["avih"][4] == 35 and (p["strh"][0][6], p["strh"][0][7]) == (1, 25)
    mono = audio["waveform"].reshape(-1)
    assert b"".join(p["audio"]) == HM.pcm16(mono) and p["strh"][1][9] == mono.numel() == 22400 and p["strh"][1][7] == 32000
    f = io.BytesIO()  # a seekable file object, another quality and rate
    assert agent.write_video(f, img, audio, emo="happy", no_crop=True, seed=SEED, quality=50, fps=30) == 35
    p = avi_parts(f.getvalue())
    assert len(p["video"]) == 35 and p["video"] != want and (p["strh"][0][6], p["strh"][0][7]) == (1, 30)
