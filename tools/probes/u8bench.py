"""fp32 against 8-bit frames, interleaved in one process, on the benchmark's shapes (bench.py config 1: a 10-s clip at 512 px,
51 grid points, decode batches of 32, seeded weights of the checkpoint's shapes):
  decode      FloatHotPath.decode_to_host for 250 frames (decode + hand-over into pinned host memory);
  clip        InferenceAgent.infer_device for one clip;
  batch16     InferenceAgent.infer_device_batch for B = 16 clips, reported per clip.
Each is timed with device events around the call, REPS (default 20) repetitions per format after WARMUP (default 3), fp32 and
uint8 taking turns.  Prints one JSON line: median, min and max per format and case, ms.  `ok` = the u8 median does not exceed the
fp32 median by more than the fp32 repetitions' own spread (max - min).  Run from the repository root.
Environment: REPS, WARMUP, B (default 16; 0 skips the batch case)."""
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from tests.util import load_pkg  # noqa: E402

pkg = load_pkg()
REPS, WARMUP, B = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("B", "16"))
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
hp = agent.G


def portrait(seed):
    return (torch.from_numpy(np.random.RandomState(seed).rand(1, 3, SIZE, SIZE).astype("float32")) * 2 - 1).to(dev)


img, wav = portrait(0), pkg.weights.synth_waveform(SECONDS, seed=1).to(dev)
items = [(portrait(i), pkg.weights.synth_waveform(SECONDS, seed=1 + i).to(dev)) for i in range(B)]
T = 250
g = torch.Generator().manual_seed(0)
s_r, r_d = torch.randn(1, 512, generator=g).to(dev), (torch.randn(T, 512, generator=g) * 0.5).to(dev)
agent.enc.encode_image_into_latent(img, want_feats=False)
agent.enc.hand_feats_to(hp.dec)
keep = {}


def decode(dt):
    keep["d"] = None  # the previous result is released first, as a caller that consumed it would have
    keep["d"] = hp.decode_to_host(s_r, r_d, out_dtype=dt)


def clip(dt):
    keep["c"] = None
    keep["c"] = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15, out_dtype=dt)


def batch(dt):
    keep["b"] = None
    keep["b"] = agent.infer_device_batch(items, 2.0, 1.0, 1.0, "neutral", [15 + i for i in range(B)], out_dtype=dt)


def ev_ms(f, dt):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f(dt)
    e1.record()
    e1.synchronize()
    hp.release_host_inflight()
    return e0.elapsed_time(e1)


def case(f, per=1):
    formats = (("fp32", torch.float32), ("u8", torch.uint8))
    for _ in range(WARMUP):
        for _, dt in formats:
            ev_ms(f, dt)
    ms = {name: [] for name, _ in formats}
    for _ in range(REPS):
        for name, dt in formats:  # taking turns: drift of the box lands on both
            ms[name].append(ev_ms(f, dt) / per)
    out = {name: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for name, v in ms.items()}
    spread = out["fp32"]["max"] - out["fp32"]["min"]
    out["fp32_spread"] = round(spread, 3)
    out["gain_ms"] = round(out["fp32"]["median"] - out["u8"]["median"], 3)
    out["ok"] = out["u8"]["median"] <= out["fp32"]["median"] + spread
    return out


res = dict(probe="u8bench", size=SIZE, frames=T, nfe=NFE, max_frames=MAX_FRAMES, reps=REPS, warmup=WARMUP,
           staging_mb=dict(fp32=round(T * SIZE * SIZE * 3 * 4 / 1e6, 1), u8=round(T * SIZE * SIZE * 3 / 1e6, 1)))
res["decode_250"] = case(decode)
res["clip"] = case(clip)
if B > 0:
    keep.clear()
    res["batch%d_per_clip" % B] = case(batch, per=B)
# the two formats of the last repetition agree bitwise on the single clip
a = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15)
b = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15, out_dtype=torch.uint8)
res["u8_equals_rounded_fp32"] = bool(torch.equal(b, torch.round(a * 255).to(torch.uint8)))
print(json.dumps(res))
