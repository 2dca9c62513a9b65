"""The PNG routes of the product on the GPU, through the synthetic 64-px agent of tests/test_jpeg_gpu.py: the files, decoded by
Pillow, are the 8-bit frames of the uint8 routes bit for bit - lossless means no tolerance."""
import importlib
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests.test_img_front_gpu import image
from tests.util import load_pkg

pkg = load_pkg()
W = pkg.weights
HM = pkg.host_models
pytestmark = pytest.mark.gpu
SEED = 7
_state = {}


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
        _state["wav60"] = W.synth_waveform(2.4, seed=10).cuda()  # 60 frames: two windows, the second short
    return _state["agent"]


def _audio():
    return {"waveform": W.synth_waveform(1.4, seed=9).reshape(1, 1, -1), "sample_rate": 16000}


def _u8():
    """infer_device(out_dtype=torch.uint8) of the 60-frame clip, computed once and left unchanged."""
    if "u8" not in _state:
        agent = _agent()
        _state["u8"] = agent.infer_device(_state["img"], _state["wav60"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, out_dtype=torch.uint8).cpu().numpy()
    return _state["u8"]


def decoded(f):
    return np.array(Image.open(io.BytesIO(bytes(f))).convert("RGB"))


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for v in ("FLOAT_AMD_VERIFY", "FLOAT_AMD_VERIFY_ACTION", "FLOAT_AMD_VERIFY_FRAMES", "FLOAT_AMD_VERIFY_PSNR", "FLOAT_AMD_OVERLAP",
              "FLOAT_AMD_IMAGE_FRONT"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FLOAT_AMD_NOISE", "cpu")


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    agent = _state.pop("agent", None)
    if agent is not None:
        agent.offload()
    _state.clear()


def test_infer_device_png_decodes_to_the_u8_frames():
    agent = _agent()
    u8 = _u8()
    assert u8.shape == (60, 64, 64, 3)
    fr = agent.infer_device_png(_state["img"], _state["wav60"], 2.0, 1.0, 1.0, emo="happy", seed=SEED)
    assert fr.data.is_pinned() and len(fr) == 60 and fr.nbytes == int(fr.offsets[-1]) == sum(len(f) for f in fr)
    for i, f in enumerate(fr):
        assert np.array_equal(decoded(f), u8[i]), i
    files = [bytes(f) for f in fr]
    assert files == HM.png_encode_rgb8(u8)  # and they are the definition's bytes
    assert fr.crcs.tolist() == [zlib.crc32(f[41:-16]) for f in files]
    _state["files"] = files
    b3 = agent.infer_device_png(_state["img"], _state["wav60"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, band=3)
    assert [bytes(f) for f in b3] == HM.png_encode_rgb8(u8, 3)
    with pytest.raises(ValueError):
        agent.infer_device_png(_state["img"], _state["wav60"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, band=65)


@pytest.mark.parametrize("slots", [2, 3])
def test_stream_blocks_are_the_whole_clip(slots):
    agent = _agent()
    u8 = _u8()
    got, spans = [], []
    for blk in agent.stream_device_png(_state["img"], _state["wav60"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, slots=slots):
        assert blk.frames.data.is_pinned() and len(blk.frames) == blk.last - blk.first == len(blk.frames.crcs)
        spans.append((blk.first, blk.last))
        got += [bytes(f) for f in blk.frames]
    assert spans == [(0, 50), (50, 60)]
    assert got == (_state.get("files") or HM.png_encode_rgb8(u8))
    with pytest.raises(ValueError):
        agent.stream_device_png(_state["img"], _state["wav60"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, slots=1)
    with pytest.raises(ValueError):
        agent.stream_device_png(_state["img"], _state["wav60"], 2.0, 1.0, 1.0, emo="happy", seed=SEED, band=65)


def test_stream_overflow_is_encoded_once_more(monkeypatch):
    """Room for 1024 bytes per slot and per whole-clip call: every block and the whole-clip call take their second encode."""
    agent = _agent()
    want = _state.get("files") or HM.png_encode_rgb8(_u8())
    args = (_state["img"], _state["wav60"], 2.0, 1.0, 1.0)
    monkeypatch.setattr(pkg.png, "default_capacity", lambda *a: 1024)
    got = [bytes(f) for blk in agent.stream_device_png(*args, emo="happy", seed=SEED, slots=2) for f in blk.frames]
    assert got == want
    assert [bytes(f) for f in agent.infer_device_png(*args, emo="happy", seed=SEED)] == want


def test_pasted_png_of_a_90_x_67_portrait():
    agent = _agent()
    img = image(23, 90, 67, 3)
    kw = dict(emo="happy", no_crop=True, seed=SEED)
    pasted = agent.infer_pasted(img[None], _audio(), **kw).numpy()
    assert pasted.shape == (35, 90, 67, 3)
    fr = agent.infer_pasted_png(img[None], _audio(), **kw)
    assert len(fr) == 35
    for i, f in enumerate(fr):
        assert np.array_equal(decoded(f), pasted[i]), i
    files = [bytes(f) for f in fr]
    assert files == HM.png_encode_rgb8(pasted)
    streamed = [bytes(f) for b in agent.stream_pasted_png(img[None], _audio(), **kw) for f in b.frames]
    assert streamed == files


def test_write_apng(tmp_path):
    agent = _agent()
    g = torch.Generator().manual_seed(0)
    img = torch.rand(1, 64, 64, 3, generator=g)
    audio = _audio()
    s, a = agent.host_inputs(img, audio, no_crop=True)
    u8 = agent.infer_device(s, a, emo="happy", seed=SEED, out_dtype=torch.uint8).cpu().numpy()
    f = io.BytesIO()
    assert agent.write_apng(f, img, audio, emo="happy", no_crop=True, seed=SEED) == 35 == len(u8)
    im = Image.open(io.BytesIO(f.getvalue()))
    assert im.n_frames == 35 and im.is_animated
    for t in range(35):
        im.seek(t)
        assert np.array_equal(np.array(im.convert("RGB")), u8[t]), t
        assert im.info["duration"] == 40.0  # opt.fps = 25
    path = str(tmp_path / "clip.png")
    assert agent.write_apng(path, img, audio, emo="happy", no_crop=True, seed=SEED, fps=12.5, band=3) == 35
    im = Image.open(path)
    im.seek(34)
    assert im.n_frames == 35 and np.array_equal(np.array(im.convert("RGB")), u8[34]) and im.info["duration"] == 80.0
    pasted = agent.infer_pasted(image(23, 90, 67, 3)[None], audio, emo="happy", no_crop=True, seed=SEED).numpy()
    f = io.BytesIO()
    assert agent.write_apng(f, image(23, 90, 67, 3)[None], audio, emo="happy", no_crop=True, seed=SEED, paste_back=True) == 35
    im = Image.open(io.BytesIO(f.getvalue()))
    assert im.size == (67, 90) and im.n_frames == 35
    for t in (0, 17, 34):
        im.seek(t)
        assert np.array_equal(np.array(im.convert("RGB")), pasted[t]), t
