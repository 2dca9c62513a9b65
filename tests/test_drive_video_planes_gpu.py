"""InferenceAgent.align_driving on a pitched yuv422p10le clip (an image.PlanarYuv), on the synthetic 64-px model of
tests/test_drive_video_gpu.py: 6 frames of 97 x 99, on the host (chunks of 4 through one device buffer) and resident on the device,
against the same call on the definition's RGB frames.  Rects are given: no detector weights."""
import functools
import importlib

import pytest
import torch

from tests.util import load_pkg
from tests.yuv_planes_fill import fill_planes

pkg = load_pkg()
hm, image, W = pkg.host_models, pkg.image, pkg.weights
pytestmark = pytest.mark.gpu
T, SH, SW = 6, 97, 99
RECTS = [(11 + 3 * t, 5 + 7 * t, 70 + t, 70 + t) for t in range(T)]  # the last ones reach past the right and bottom edges


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


@pytest.mark.parametrize("resident", [False, True])
def test_a_pitched_422_10_bit_clip_aligns_like_its_rgb_frames(resident):
    kw = dict(y_pitch=2 * SW + 6, c_pitch=2 * ((SW + 1) // 2) + 2, frame_stride=40000, matrix="bt709", chroma="centre")
    data = fill_planes(hm.yuv_planes_format(SH, SW, "422", 10, **kw), T, 17)[0]
    clip = image.PlanarYuv.of("yuv422p10le", data, SH, SW, **kw)
    agent = _agent()
    want, _ = agent.align_driving(clip.to_rgb8(), rects=RECTS)
    got, rects = agent.align_driving(clip.like(data.cuda()) if resident else clip, rects=RECTS, chunk=4)
    assert rects == RECTS and torch.equal(got, want)
    full, _ = agent.align_driving(clip, rects=RECTS, src_matrix="bt601-full", src_chroma="nearest")  # the overrides reach the kernel
    assert torch.equal(full, agent.align_driving(clip.like(data, "bt601-full", "nearest").to_rgb8(), rects=RECTS)[0]) and not torch.equal(full, want)
