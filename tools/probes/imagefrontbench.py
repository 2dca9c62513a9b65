"""The image front end on the device (float_img_front) against the host route it replaces, interleaved in one process, on the
benchmark's shapes (bench.py config 1: a 10-s clip at 512 px, 51 grid points, decode batches of 32, seeded weights of the
checkpoint's shapes).  The input is what a node hands over: a pageable fp32 IMAGE tensor in host memory.
Two forms take turns:
  device  InferenceAgent.host_inputs with the front end (the default);
  host    the same call with FLOAT_AMD_IMAGE_FRONT=0 (read at the call): alpha discarded, round / adaptive_avg_pool2d in torch.
Portraits: a 1024 x 1024 RGB image and a 3840 x 2160 RGBA image (133 MB), both without a face crop (no detector is needed).
Cases, per portrait:
  host_inputs    the call alone (portrait + waveform -> s, a on the device);
  run_inference  the whole step, host inputs -> frames in pinned host memory.
Each call is timed with a host clock between two device synchronisations (the host form's cost is CPU time), REPS (default
20) repetitions per form after WARMUP (default 3).  Prints one JSON line: median, min, max and spread (max - min) per form and
case, ms, `device_minus_host_ms`, and, for the device form, whether s is bitwise the definition (host_models.resize_rgb8 of
host_models.image_to_rgb8; skipped with CHECK=0: the definition of the 4K portrait takes a while on the CPU).  Run from the
repository root.  Environment: REPS, WARMUP, CHECK, PORTRAITS (default "rgb1024,rgba4k")."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from tests.util import load_pkg  # noqa: E402

pkg = load_pkg()
hm = pkg.host_models
REPS, WARMUP, CHECK = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3")), os.environ.get("CHECK", "1") != "0"
PORTRAITS = os.environ.get("PORTRAITS", "rgb1024,rgba4k").split(",")
SHAPES = {"rgb1024": (1024, 1024, 3), "rgba4k": (2160, 3840, 4)}
SIZE, SECONDS, NFE, MAX_FRAMES = 512, 10.0, 51, 32
dev = "cuda:0"

cfg = pkg.config.FmtConfig()
gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
opt.nfe, opt.input_size, opt.fps, opt.rank = NFE, SIZE, 25.0, dev
acfg = pkg.config.AudioConfig()
parts = dict(enc=pkg.weights.synth_encoder_state(SIZE, seed=1), dec=pkg.weights.synth_decoder_state(SIZE, seed=1),
             fmt=pkg.weights.synth_fmt_state(cfg, seed=1), audio_encoder=(pkg.weights.synth_audio_state(acfg, seed=1), acfg))
agent = gen.InferenceAgent(opt, parts, dev, max_frames=MAX_FRAMES, use_graph=2)
n = int(round(SECONDS * 16000))
wave = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 16000) + 0.1 * np.random.RandomState(1).standard_normal(n)).astype("float32")
audio = {"waveform": torch.from_numpy(wave)[None, None], "sample_rate": 16000}


def portrait(name):
    """a ComfyUI IMAGE item in pageable host memory: smooth colour ramps plus noise, alpha a soft disc"""
    h, w, ch = SHAPES[name]
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[0:h, 0:w].astype("float32")
    x = np.stack([xx / w, yy / h, 0.5 + 0.5 * np.sin(xx / 37.0)], axis=-1) * 0.8 + 0.2 * rs.rand(h, w, 3).astype("float32")
    if ch == 4:
        r = np.sqrt((xx / w - 0.5) ** 2 + (yy / h - 0.5) ** 2)
        x = np.concatenate([x, np.clip((0.45 - r) * 8.0, 0.0, 1.0)[..., None]], axis=-1)
    return torch.from_numpy(np.ascontiguousarray(x.astype("float32")))[None]


def set_form(form):
    if form == "host":
        os.environ["FLOAT_AMD_IMAGE_FRONT"] = "0"
    else:
        os.environ.pop("FLOAT_AMD_IMAGE_FRONT", None)


def timed(f, form):
    set_form(form)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    agent.G.release_host_inflight()
    return ms, out


def case(f):
    for _ in range(WARMUP):
        for form in ("device", "host"):
            timed(f, form)
    ms = {"device": [], "host": []}
    for _ in range(REPS):
        for form in ("device", "host"):  # taking turns: drift of the box lands on both
            ms[form].append(timed(f, form)[0])
    out = {form: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), spread=round(max(v) - min(v), 3))
           for form, v in ms.items()}
    out["device_minus_host_ms"] = round(out["device"]["median"] - out["host"]["median"], 3)
    return out


res = dict(probe="imagefrontbench", size=SIZE, seconds=SECONDS, nfe=NFE, max_frames=MAX_FRAMES, reps=REPS, warmup=WARMUP,
           torch_threads=torch.get_num_threads())
for name in PORTRAITS:
    img = portrait(name)
    assert not img.is_pinned()
    r = {"shape": list(img.shape[1:]), "mbytes": round(img.numel() * 4 / 1e6, 1)}
    r["host_inputs"] = case(lambda: agent.host_inputs(img, audio))
    r["run_inference"] = case(lambda: agent.run_inference(None, img, audio, 2.0, 1.0, 1.0, emo="neutral", no_crop=True, seed=15))
    if CHECK:
        s_dev = timed(lambda: agent.host_inputs(img, audio)[0], "device")[1].cpu()
        want = hm.rgb8_to_model_input(hm.resize_rgb8(hm.image_to_rgb8(img[0], opt.rgba_conversion, hm.hex_to_rgb8(opt.bkg_color_hex)),
                                                     None, SIZE, SIZE))
        r["device_equals_definition"] = bool(torch.equal(s_dev, want))
        s_host = timed(lambda: agent.host_inputs(img, audio)[0], "host")[1].cpu()
        r["max_abs_device_minus_host"] = float((s_dev - s_host).abs().max())
    res[name] = r
set_form("device")
print(json.dumps(res))
