"""8-bit RGB against planar YUV 4:2:0 (I420) frames, interleaved in one process, on the benchmark's shapes (bench.py config 1: a
10-s clip at 512 px, 51 grid points, decode batches of 32, seeded weights of the checkpoint's shapes).  Three forms take turns:
  u8          uint8 RGB (float_dec_frames_host_u8): the yardstick;
  i420_fused  I420 formed by dec_flowlast_kernel's I420 instantiation (float_dec_frames_host_i420, the default);
  i420_conv   I420 through 8-bit RGB scratch + dec_rgb8_to_i420_kernel: a second agent built with FLOAT_DEC_YUV_FUSED=0.
Cases:
  decode      FloatHotPath.decode_to_host for 250 frames (decode + hand-over into pinned host memory);
  clip        InferenceAgent.infer_device for one clip;
  batch16     InferenceAgent.infer_device_batch for B = 16 clips, reported per clip.
Every destination of the decode and clip cases is allocated (pinned) before the first repetition; the batch case returns the
product's own tensors.  Each call is timed with device events around it, REPS (default 20) repetitions per form after WARMUP
(default 3).  Prints one JSON line: median, min, max and spread (max - min) per form and case, ms.  `ok` = an I420 median does
not exceed the u8 median by more than the u8 repetitions' own spread.  Run from the repository root.
--matrix M (2 | 4 | 6 or a name host_models.yuv_matrix_id knows): two more forms, i420_fused_m and i420_conv_m, the same calls with
matrix=M, take turns with the others; each reports `minus_id0_ms` against its id-0 sibling and `ok_vs_id0` = its median does not
exceed the sibling's by more than the sibling's own spread, and the clip of the last repetition is compared with
rgb8_to_i420(u8, M).
Environment: REPS, WARMUP, B (default 16; 0 skips the batch case)."""
import argparse
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
ap = argparse.ArgumentParser()
ap.add_argument("--matrix", default=None, help="a second colour matrix to interleave with id 0 (2, 4, 6 or a name)")
MATRIX = ap.parse_args().matrix
MATRIX = None if MATRIX is None else pkg.host_models.yuv_matrix_id(int(MATRIX) if MATRIX.lstrip("-").isdigit() else MATRIX)
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


def build(fused):
    old = os.environ.get("FLOAT_DEC_YUV_FUSED")
    os.environ["FLOAT_DEC_YUV_FUSED"] = "1" if fused else "0"  # read when the decoder handle is created
    try:
        return gen.InferenceAgent(opt, parts, dev, max_frames=MAX_FRAMES, use_graph=2)
    finally:
        if old is None:
            del os.environ["FLOAT_DEC_YUV_FUSED"]
        else:
            os.environ["FLOAT_DEC_YUV_FUSED"] = old


agents = dict(fused=build(True), conv=build(False))
# form -> (agent, out_dtype, out_format, matrix)
FORMS = dict(u8=(agents["fused"], torch.uint8, None, None), i420_fused=(agents["fused"], None, "i420", None),
             i420_conv=(agents["conv"], None, "i420", None))
if MATRIX is not None:
    FORMS.update(i420_fused_m=(agents["fused"], None, "i420", MATRIX), i420_conv_m=(agents["conv"], None, "i420", MATRIX))


def portrait(seed):
    return (torch.from_numpy(np.random.RandomState(seed).rand(1, 3, SIZE, SIZE).astype("float32")) * 2 - 1).to(dev)


img, wav = portrait(0), pkg.weights.synth_waveform(SECONDS, seed=1).to(dev)
items = [(portrait(i), pkg.weights.synth_waveform(SECONDS, seed=1 + i).to(dev)) for i in range(B)]
T = 250
g = torch.Generator().manual_seed(0)
s_r, r_d = torch.randn(1, 512, generator=g).to(dev), (torch.randn(T, 512, generator=g) * 0.5).to(dev)
for a in agents.values():
    a.enc.encode_image_into_latent(img, want_feats=False)
    a.enc.hand_feats_to(a.G.dec)
SHAPES = {f: (T, SIZE, SIZE, 3) if f == "u8" else (T, 3 * SIZE // 2, SIZE) for f in FORMS}
dst = {(c, f): torch.empty(SHAPES[f], dtype=torch.uint8).pin_memory() for c in ("decode", "clip") for f in FORMS}
keep = {}


def mkw(m):
    return {} if m is None else dict(matrix=m)


def decode(form):
    agent, dt, fmt, m = FORMS[form]
    agent.G.decode_to_host(s_r, r_d, out=dst["decode", form], out_dtype=dt, out_format=fmt, **mkw(m))


def clip(form):
    agent, dt, fmt, m = FORMS[form]
    agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15, out=dst["clip", form], out_dtype=dt, out_format=fmt, **mkw(m))


def batch(form):
    agent, dt, fmt, m = FORMS[form]
    keep["b"] = None  # the previous result is released first, as a caller that consumed it would have
    keep["b"] = agent.infer_device_batch(items, 2.0, 1.0, 1.0, "neutral", [15 + i for i in range(B)], out_dtype=dt, out_format=fmt, **mkw(m))


def ev_ms(f, form):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f(form)
    e1.record()
    e1.synchronize()
    FORMS[form][0].G.release_host_inflight()
    return e0.elapsed_time(e1)


def case(f, per=1):
    for _ in range(WARMUP):
        for form in FORMS:
            ev_ms(f, form)
    ms = {form: [] for form in FORMS}
    for _ in range(REPS):
        for form in FORMS:  # taking turns: drift of the box lands on all three
            ms[form].append(ev_ms(f, form) / per)
    out = {form: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), spread=round(max(v) - min(v), 3))
           for form, v in ms.items()}
    for form in ("i420_fused", "i420_conv"):
        out[form]["minus_u8_ms"] = round(out[form]["median"] - out["u8"]["median"], 3)
        out[form]["ok"] = out[form]["median"] <= out["u8"]["median"] + out["u8"]["spread"]
        if MATRIX is not None:
            a, b = out[form + "_m"], out[form]
            a["minus_id0_ms"] = round(a["median"] - b["median"], 3)
            a["ok_vs_id0"] = a["median"] <= b["median"] + b["spread"]
    return out


res = dict(probe="yuvbench", matrix=MATRIX, size=SIZE, frames=T, nfe=NFE, max_frames=MAX_FRAMES, reps=REPS, warmup=WARMUP,
           staging_mb=dict(u8=round(T * SIZE * SIZE * 3 / 1e6, 1), i420=round(T * SIZE * SIZE * 3 / 2 / 1e6, 1)))
res["decode_250"] = case(decode)
res["clip"] = case(clip)
if B > 0:
    res["batch%d_per_clip" % B] = case(batch, per=B)
    keep.clear()
# the three forms of the last repetition agree bitwise on the single clip
want = pkg.host_models.rgb8_to_i420(dst["clip", "u8"])
res["i420_equals_converted_u8"] = dict(fused=bool(torch.equal(dst["clip", "i420_fused"], want)),
                                       conv=bool(torch.equal(dst["clip", "i420_conv"], want)))
if MATRIX is not None:
    want_m = pkg.host_models.rgb8_to_i420(dst["clip", "u8"], MATRIX)
    res["i420_m_equals_converted_u8"] = dict(fused=bool(torch.equal(dst["clip", "i420_fused_m"], want_m)),
                                             conv=bool(torch.equal(dst["clip", "i420_conv_m"], want_m)))
res["pinned_bytes_per_250_frames"] = dict(u8=dst["clip", "u8"].numel(), i420=dst["clip", "i420_fused"].numel())
print(json.dumps(res))
