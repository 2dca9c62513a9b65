"""InferenceAgent.align_driving / drive_video on a .y4m file, on the synthetic 64-px model of tests/test_drive_video_gpu.py: 5 frames
of 98 x 98 (write_y4m takes square frames; chroma rows of 49 bytes) written by write_y4m, read chunk by chunk, against the definition's crops.  Rects are given: no detector weights."""
import functools
import importlib

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm, W = pkg.host_models, pkg.weights
pytestmark = pytest.mark.gpu
T, SH, SW = 5, 98, 98
RECTS = [(11 + 3 * t, 5 + 9 * t, 70 + t, 70 + t) for t in range(T)]  # the last ones reach past the right and bottom edges


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
def _planes():
    return torch.from_numpy(np.random.RandomState(11).randint(0, 256, (T, 3 * SH // 2, SW)).astype(np.uint8))


def _crops(matrix, chroma):
    rgb = hm.yuv420_to_rgb8(_planes(), "i420", matrix, chroma)
    return torch.stack([hm.resize_rgb8(rgb[t], RECTS[t], 64, 64) for t in range(T)])


@pytest.mark.parametrize("full,src_matrix,src_chroma,matrix,chroma", [(False, None, None, 0, "nearest"), (True, "bt709-full", "centre", 6, "centre")])
def test_y4m_path_gives_the_definitions_crops_and_drives_like_them(tmp_path, full, src_matrix, src_chroma, matrix, chroma):
    agent = _agent()
    path = str(tmp_path / "drive.y4m")
    hm.write_y4m(path, _planes(), 25, 4 if full else 0)
    crops = _crops(matrix if src_matrix else (4 if full else 0), chroma)
    frames, rects = agent.align_driving(path, rects=RECTS, chunk=2, src_matrix=src_matrix, src_chroma=src_chroma)
    assert rects == RECTS and torch.equal(frames.cpu(), crops)
    portrait = torch.from_numpy(np.random.RandomState(5).rand(1, 64, 64, 3).astype(np.float32))
    got = agent.drive_video(portrait, path, rects=RECTS, chunk=2, out_dtype=torch.uint8, src_matrix=src_matrix, src_chroma=src_chroma).clone()
    s = agent.host_inputs(portrait, {"waveform": torch.zeros(1, 1, 16), "sample_rate": 16000})[0]
    assert torch.equal(got, agent.drive_device(s, crops.cuda(), out_dtype=torch.uint8))
