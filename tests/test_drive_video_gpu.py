"""InferenceAgent.align_driving / drive_video on the synthetic 64-px model of tests/test_enc_motion_gpu.py: a raw 97 x 131 host
video against drive_device on crops made by the host definition.  Rects are given or crop=None: no detector weights needed."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm, W = pkg.host_models, pkg.weights
pytestmark = pytest.mark.gpu
T = 12
RECTS = [(10 + 3 * t, 5 + 2 * t, 70 + t, 70 + t) for t in range(T)]  # the last ones reach past the bottom edge


@functools.lru_cache(None)
def _agent():
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.input_size, opt.nfe = 64, 6
    acfg = pkg.config.small_audio_config()
    acfg.dim_w = opt.dim_w
    parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31),
                 fmt=W.synth_fmt_state(pkg.config.FmtConfig.from_options(opt), seed=31), audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
    return gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8)


@functools.lru_cache(None)
def _video():
    return torch.from_numpy(np.random.RandomState(7).uniform(-0.1, 1.1, size=(T, 97, 131, 3)).astype(np.float32))


def _crops(rects):
    return torch.stack([hm.resize_rgb8(hm.image_to_rgb8(_video()[t]), rects[t], 64, 64) for t in range(T)])


@pytest.mark.parametrize("crop", ["rects", None])
def test_drive_video_is_drive_device_on_the_definitions_crops(crop):
    agent = _agent()
    portrait = torch.from_numpy(np.random.RandomState(5).rand(1, 64, 64, 3).astype(np.float32))
    rects = RECTS if crop == "rects" else [(17, 0, 96, 96)] * T  # the centre square of 97 x 131
    got = agent.drive_video(portrait, _video(), rects=RECTS if crop == "rects" else None, crop=None, chunk=5, out_dtype=torch.uint8).clone()
    s = agent.host_inputs(portrait, {"waveform": torch.zeros(1, 1, 16), "sample_rate": 16000})[0]
    want = agent.drive_device(s, _crops(rects).cuda(), out_dtype=torch.uint8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (T, 64, 64, 3) and torch.equal(got, want)


def test_align_driving_device_video_equals_host_video():
    agent = _agent()
    on_host, r_host = agent.align_driving(_video(), rects=RECTS, chunk=5)
    on_dev, r_dev = agent.align_driving(_video().cuda(), rects=RECTS, chunk=7)
    assert r_host == r_dev == RECTS and torch.equal(on_host, on_dev) and torch.equal(on_host.cpu(), _crops(RECTS))


def test_align_driving_detects_on_the_sampled_views(monkeypatch):
    """crop="fixed" with the package's detector stubbed: it sees the definition's 360-px views of frames 0, 5, 10 and 11, and
    the clip gets process_img's rect for the box it returns."""
    monkeypatch.delenv("FLOAT_AMD_FACE_DETECTOR", raising=False)
    seen = []

    class FA:
        class face_detector:
            @staticmethod
            def detect_from_image(arr):
                seen.append(torch.from_numpy(arr.copy()))
                return [(100.0, 40.0, 250.0, 200.0, 0.99)]

    monkeypatch.setattr(hm, "_FA", FA())
    video = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (T, 400, 300, 3)).astype(np.uint8))
    frames, rects = _agent().align_driving(video, crop="fixed")
    assert len(seen) == 4 and torch.equal(seen[3], hm.resize_rgb8(video[11], None, 360, 270, scale=(10, 9)))
    want = hm.process_img(video[0].float() / 255, 64, 1.6)[1]
    assert rects == [want] * T and torch.equal(frames[11].cpu(), hm.resize_rgb8(video[11], want, 64, 64))
