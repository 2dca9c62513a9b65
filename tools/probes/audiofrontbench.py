"""The audio front end on the device (float_aud_front) against the host resampler it replaces, interleaved in one process, on
the benchmark's shapes (bench.py config 1: a 10-s clip at 512 px, 51 grid points, decode batches of 32, seeded weights of the
checkpoint's shapes).  The input is what a node hands over: a pageable stereo waveform in host memory at 48 or 44.1 kHz.
Two forms take turns:
  device  InferenceAgent.host_inputs with the front end (the default);
  host    the same call with FLOAT_AMD_AUDIO_FRONT=0 (read at the call): mono mix and resample_sinc on the CPU, then the copy.
Cases, per source rate:
  host_inputs    the call alone (portrait + waveform -> s, a on the device);
  run_inference  the whole step, host inputs -> frames in pinned host memory.
Each call is timed with a host clock between two device synchronisations (the host form's cost is CPU time), REPS (default
20) repetitions per form after WARMUP (default 3).  Prints one JSON line: median, min, max and spread (max - min) per form and
case, ms, `device_minus_host_ms`, and the largest |a_device - a_host| of the two waveforms.  Run from the repository root.
Environment: REPS, WARMUP, RATES (default "48000,44100")."""
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
REPS, WARMUP = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3"))
RATES = [int(r) for r in os.environ.get("RATES", "48000,44100").split(",")]
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
img = torch.from_numpy(np.random.RandomState(0).rand(1, SIZE, SIZE, 3).astype("float32"))  # a ComfyUI IMAGE item, host memory


def audio_item(rate):
    """10 s of stereo at `rate`: a 220 Hz tone + noise per channel, (1, 2, N) pageable fp32"""
    n = int(round(SECONDS * rate))
    tone = 0.3 * np.sin(2 * np.pi * 220.0 * np.arange(n) / rate)
    w = np.stack([tone + 0.1 * np.random.RandomState(s).standard_normal(n) for s in (1, 2)]).astype("float32")
    return {"waveform": torch.from_numpy(w)[None], "sample_rate": rate}


def set_form(form):
    if form == "host":
        os.environ["FLOAT_AMD_AUDIO_FRONT"] = "0"
    else:
        os.environ.pop("FLOAT_AMD_AUDIO_FRONT", None)


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


res = dict(probe="audiofrontbench", size=SIZE, seconds=SECONDS, nfe=NFE, max_frames=MAX_FRAMES, reps=REPS, warmup=WARMUP,
           torch_threads=torch.get_num_threads())
for rate in RATES:
    audio = audio_item(rate)
    r = {}
    r["host_inputs"] = case(lambda: agent.host_inputs(img, audio))
    r["run_inference"] = case(lambda: agent.run_inference(None, img, audio, 2.0, 1.0, 1.0, emo="neutral", no_crop=True, seed=15))
    a_dev, a_host = timed(lambda: agent.host_inputs(img, audio)[1], "device")[1], timed(lambda: agent.host_inputs(img, audio)[1], "host")[1]
    r["samples"] = int(a_dev.shape[-1])
    r["max_abs_device_minus_host"] = float((a_dev - a_host).abs().max())
    res[str(rate)] = r
set_form("device")
print(json.dumps(res))
