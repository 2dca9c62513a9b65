"""A clip streamed window by window through a bounded ring of pinned frame buffers (FloatHotPath.stream_to_host,
InferenceAgent.stream_device / stream_inference): the blocks are, bit for bit, the rows of the whole-clip call - the stream runs
the same window launches and the same decoder launches, only per window - so every comparison here is torch.equal.

Clips: 2.6 s of audio = 65 frames = 2 windows with a short last block (15 frames), and 7.4 s = 185 frames = 4 windows (last block
35 frames): the smallest lengths with a short tail and with more windows than ring slots (2 and 3)."""
import importlib

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
pytestmark = pytest.mark.gpu
C, W = pkg.config, pkg.weights
SEED = 7
CLIPS = {"short": (2.6, 65, [(0, 50), (50, 65)]), "long": (7.4, 185, [(0, 50), (50, 100), (100, 150), (150, 185)])}
FORMATS = {"fp32": dict(), "u8": dict(out_dtype=torch.uint8), "i420": dict(out_format="i420")}
_state = {}


def _agent():
    """The synthetic 64-px agent of tests/test_fmt_ragged_gpu.py::_agent (max_frames = 8, nfe = 6), built once per module."""
    if "agent" not in _state:
        gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
        opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
        opt.input_size, opt.nfe = 64, 6
        cfg = C.FmtConfig.from_options(opt)
        acfg = C.small_audio_config()
        acfg.dim_w = opt.dim_w
        parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
                     audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
        _state["agent"] = gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8)
        _state["img"] = torch.from_numpy(np.random.RandomState(5).rand(1, 3, 64, 64).astype(np.float32)).cuda() * 2 - 1
        _state["wav"] = {name: W.synth_waveform(sec, seed=10).cuda() for name, (sec, _, _) in CLIPS.items()}
    return _state["agent"]


def _whole(clip, fmt, noise_mode):
    """infer_device of the clip, computed once per (clip, format, noise mode) under the caller's environment and left unchanged."""
    key = ("ref", clip, fmt, noise_mode)
    if key not in _state:
        agent = _agent()
        _state[key] = agent.infer_device(_state["img"], _state["wav"][clip], 2.0, 1.0, 1.0, emo="happy", seed=SEED,
                                         **FORMATS[fmt]).clone()
    return _state[key]


def _stream(clip, fmt, **kw):
    agent = _agent()
    return agent.stream_device(_state["img"], _state["wav"][clip], 2.0, 1.0, 1.0, emo="happy", seed=SEED, **FORMATS[fmt], **kw)


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


@pytest.mark.parametrize("noise_mode", ["cpu", "device"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_stream_is_bitwise_the_whole_clip(fmt, noise_mode, monkeypatch):
    """Both clips, the three frame formats, both FLOAT_AMD_NOISE modes: the concatenated blocks equal infer_device with the same
    seed; block bounds are the FMT windows, the last one short; every block is a pinned tensor of the format's shape."""
    monkeypatch.setenv("FLOAT_AMD_NOISE", noise_mode)
    for clip, (_, T, bounds) in CLIPS.items():
        want = _whole(clip, fmt, noise_mode)
        assert want.shape[0] == T
        blocks = [(b.first, b.last, b.frames.is_pinned(), b.frames.clone()) for b in _stream(clip, fmt)]
        assert [(f, l) for f, l, _, _ in blocks] == bounds
        assert all(p for _, _, p, _ in blocks)
        assert all(tuple(x.shape) == (l - f,) + tuple(want.shape[1:]) and x.dtype == want.dtype for f, l, _, x in blocks)
        assert torch.equal(torch.cat([x for _, _, _, x in blocks]), want), (clip, fmt, noise_mode)


@pytest.mark.parametrize("slots", [2, 3])
def test_ring_is_bounded_and_no_slot_is_written_before_it_is_given_back(slots):
    """The 4-window clip through `slots` buffers: exactly `slots` distinct addresses, block k and block k + slots share one.
    On receiving block k the whole device is synchronised, so that everything the generator has enqueued ahead has landed,
    and only then is the block compared with its rows of the whole-clip result: a generator that enqueues into the slot the
    consumer still holds (or into one it has not got back) fails here."""
    want = _whole("long", "fp32", "cpu")
    ptrs = []
    for blk in _stream("long", "fp32", slots=slots):
        torch.cuda.synchronize()
        assert torch.equal(blk.frames, want[blk.first:blk.last]), (slots, blk.first)
        ptrs.append(blk.frames.data_ptr())
    assert len(ptrs) == 4 and len(set(ptrs)) == slots
    assert all(ptrs[k] == ptrs[k + slots] for k in range(4 - slots))


def test_early_exit_leaves_the_agent_usable():
    """One block, close(): the work enqueued ahead is waited for, the FMT handle's unfinished job is overwritten by the next begin.
    The whole-clip call and a second stream on the same agent then give the reference's bytes."""
    agent = _agent()
    want = _whole("long", "fp32", "cpu")
    gen = _stream("long", "fp32")
    blk = next(gen)
    assert (blk.first, blk.last) == (0, 50) and torch.equal(blk.frames, want[:50])
    gen.close()
    assert agent.G.__dict__.get("_open_stream") is None
    assert not any(agent.range_counts(reset=False).values())  # read and reset on the way out
    again = agent.infer_device(_state["img"], _state["wav"]["long"], 2.0, 1.0, 1.0, emo="happy", seed=SEED)
    assert torch.equal(again, want)
    assert torch.equal(torch.cat([b.frames.clone() for b in _stream("long", "fp32")]), want)
    # a consumer that raises: the generator is dropped with the exception's frames
    with pytest.raises(KeyError):
        for blk in _stream("short", "fp32"):
            raise KeyError(blk.first)
    assert torch.equal(torch.cat([b.frames.clone() for b in _stream("short", "fp32")]), _whole("short", "fp32", "cpu"))


def test_one_stream_at_a_time():
    agent = _agent()
    want = _whole("short", "fp32", "cpu")
    img, wav = _state["img"], _state["wav"]["short"]
    gen = _stream("short", "fp32")
    first = next(gen)
    held = first.frames.clone()
    with pytest.raises(RuntimeError, match="still open"):
        agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=SEED)
    with pytest.raises(RuntimeError, match="still open"):
        agent.infer_device_batch([(img, wav)], emo="happy", seeds=[SEED])
    with pytest.raises(RuntimeError, match="still open"):
        _stream("short", "fp32")
    cond = pkg.pipeline.synth_conditions(agent.cfg, 20, seed=1)
    with pytest.raises(RuntimeError, match="still open"):
        agent.G.sample(cond["r_s"], cond["wa"], cond["we"], 6)
    with pytest.raises(RuntimeError, match="still open"):
        agent.G.generate_to_host(cond["r_s"], cond["wa"], cond["we"], cond["s_r"], None, 6)
    with pytest.raises(RuntimeError, match="still open"):
        agent.G.decode_to_host(cond["s_r"], torch.zeros(4, 512))
    # the refused calls disturbed nothing: the open stream goes on to the reference's bytes
    rest = [b.frames.clone() for b in gen]
    assert torch.equal(torch.cat([held] + rest), want)
    assert torch.equal(agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=SEED), want)  # exhausted: open again


def test_argument_errors_are_raised_at_the_call():
    agent = _agent()
    img, wav = _state["img"], _state["wav"]["short"]
    with pytest.raises(ValueError, match="slots"):
        agent.stream_device(img, wav, emo="happy", slots=1)
    with pytest.raises(ValueError, match="I420"):
        agent.stream_device(img, wav, emo="happy", out_format="i420", out_dtype=torch.float32)
    with pytest.raises(ValueError, match="slots"):
        agent.G.stream_to_host(None, None, None, None, None, 6, slots=1)
    with pytest.raises(ValueError, match="I420"):
        agent.G.stream_to_host(None, None, None, None, None, 6, out_format="i420", out_dtype=torch.float32)
    with pytest.raises(ValueError, match="slots"):
        agent.stream_inference(None, None, slots=0)
    two = pkg.pipeline.synth_conditions(agent.cfg, 20, seed=1)["wa"].repeat(2, 1, 1)
    with pytest.raises(ValueError, match="B = 1"):
        agent.G.stream_to_host(None, two, None, None, None, 6)
    assert agent.G.__dict__.get("_open_stream") is None


def test_range_policy_on_a_clean_clip(monkeypatch):
    """FLOAT_AMD_RANGE=raise: the counters are read once after the last block, and a clean clip ends without raising; `auto`
    acts as warn (nothing to warn about here) and `off` skips the read."""
    for mode in ("raise", "auto", "off"):
        monkeypatch.setenv("FLOAT_AMD_RANGE", mode)
        assert [(b.first, b.last) for b in _stream("short", "u8")] == CLIPS["short"][2]
    counts = _agent().range_counts(reset=False)
    assert {"fmt", "decoder"} <= set(counts) and not any(counts.values())


def test_stream_inference_from_host_inputs():
    """Host portrait and audio: the blocks of stream_inference are the rows of run_inference."""
    agent = _agent()
    g = torch.Generator().manual_seed(0)
    img = torch.rand(1, 64, 64, 3, generator=g)
    audio = {"waveform": W.synth_waveform(2.6, seed=11).reshape(1, 1, -1).cpu(), "sample_rate": 16000}
    want = agent.run_inference(None, img, audio, emo="happy", no_crop=True, seed=SEED, out_format="i420").clone()
    got = [b.frames.clone() for b in agent.stream_inference(img, audio, emo="happy", no_crop=True, seed=SEED, out_format="i420", slots=2)]
    assert [tuple(x.shape) for x in got] == [(50, 96, 64), (15, 96, 64)]
    assert torch.equal(torch.cat(got), want)
