"""uint8 RGB, I420, JPEG (quality 90, one MCU row per restart interval) and PNG (lossless, the default band) frames through the
product's calls, interleaved in one process, on the benchmark's shapes (bench.py config 1: a 10-s clip at 512 px, 51 grid
points, decode batches of 32, seeded weights of the checkpoint's shapes).  Four forms take turns:
  u8     InferenceAgent.infer_device(out_dtype=torch.uint8): the yardstick (the parent commit's figure, from the same run);
  i420   InferenceAgent.infer_device(out_format="i420") (likewise);
  jpeg   InferenceAgent.infer_device_jpeg(quality=QUALITY) (likewise);
  png    InferenceAgent.infer_device_png().
Cases:
  decode  250 frames from fixed latents: FloatHotPath.decode_to_host for u8 / i420, decode_u8 + jpeg.encode_jpeg_host /
          png.encode_png_host for jpeg / png (decode + hand-over into pinned host memory);
  clip    the whole call for one clip;
  encode  the launches of float_jpg_encode / float_png_encode alone on 250 decoded frames in HBM, into buffers made once (device
          events around the call, nothing read back).
Each call is timed on the host clock between device synchronisations (the file forms read their offsets on the host inside the
call), REPS (default 20) repetitions per form after WARMUP (default 3).  Prints one JSON line: bytes that cross PCIe per clip and
median, min, max and spread (max - min) per form and case, ms.  The synthetic model's frames are not a face: the file bytes per
clip are this model's, not a checkpoint's.  Run from the repository root.  Environment: REPS, WARMUP, QUALITY."""
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
REPS, WARMUP, QUALITY = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("QUALITY", "90"))
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
FORMS = ("u8", "i420", "jpeg", "png")
KW = dict(u8=dict(out_dtype=torch.uint8), i420=dict(out_format="i420"))

img = (torch.from_numpy(np.random.RandomState(0).rand(1, 3, SIZE, SIZE).astype("float32")) * 2 - 1).to(dev)
wav = pkg.weights.synth_waveform(SECONDS, seed=1).to(dev)
T = 250
g = torch.Generator().manual_seed(0)
s_r, r_d = torch.randn(1, 512, generator=g).to(dev), (torch.randn(T, 512, generator=g) * 0.5).to(dev)
agent.enc.encode_image_into_latent(img, want_feats=False)
agent.enc.hand_feats_to(agent.G.dec)
dst = {(c, f): torch.empty((T, SIZE, SIZE, 3) if f == "u8" else (T, 3 * SIZE // 2, SIZE), dtype=torch.uint8).pin_memory()
       for c in ("decode", "clip") for f in ("u8", "i420")}
last = {}


def decode(form):
    if form == "jpeg":
        last["decode"] = pkg.jpeg.encode_jpeg_host(agent.G.dec.decode_u8(s_r, r_d), QUALITY)
    elif form == "png":
        last["decode_png"] = pkg.png.encode_png_host(agent.G.dec.decode_u8(s_r, r_d))
    else:
        agent.G.decode_to_host(s_r, r_d, out=dst["decode", form], **KW[form])


def clip(form):
    if form == "jpeg":
        last["clip"] = agent.infer_device_jpeg(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15, quality=QUALITY)
    elif form == "png":
        last["clip_png"] = agent.infer_device_png(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15)
    else:
        agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15, out=dst["clip", form], **KW[form])


def wall_ms(f, form):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f(form)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    agent.G.release_host_inflight()
    return ms


def case(f):
    for _ in range(WARMUP):
        for form in FORMS:
            wall_ms(f, form)
    ms = {form: [] for form in FORMS}
    for _ in range(REPS):
        for form in FORMS:  # taking turns: drift of the box lands on all three
            ms[form].append(wall_ms(f, form))
    out = {form: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), spread=round(max(v) - min(v), 3))
           for form, v in ms.items()}
    for form in ("jpeg", "png"):
        out[form]["minus_u8_ms"] = round(out[form]["median"] - out["u8"]["median"], 3)
        out[form]["minus_i420_ms"] = round(out[form]["median"] - out["i420"]["median"], 3)
    return out


def encode_alone():
    """the encoders' launches on 250 decoded frames in HBM, by device events, taking turns"""
    u8 = agent.G.dec.decode_u8(s_r, r_d)
    off = torch.empty(T + 1, dtype=torch.int64, device=dev)
    crc = torch.empty(T, dtype=torch.int32, device=dev)
    room = torch.empty(u8.numel() * 9 // 8 + (1 << 20), dtype=torch.uint8, device=dev)
    band = pkg.png.default_band(SIZE, SIZE)
    work = {"jpeg": None, "png": None}

    def run(form):
        if form == "jpeg":
            work[form] = pkg.jpeg.enqueue_encode(u8, QUALITY, pkg.jpeg.default_restart(SIZE), room, off, work[form])
        else:
            work[form] = pkg.png.enqueue_encode(u8, band, room, off, crc, work[form])

    ms = {"jpeg": [], "png": []}
    for i in range(WARMUP + REPS):
        for form in ms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(form)
            b.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                ms[form].append(a.elapsed_time(b))
    return {form: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for form, v in ms.items()}


res = dict(probe="pngbench", size=SIZE, frames=T, nfe=NFE, max_frames=MAX_FRAMES, reps=REPS, warmup=WARMUP, quality=QUALITY)
res["decode_250"] = case(decode)
res["clip"] = case(clip)
res["encode_launches_250"] = encode_alone()
res["bytes_per_clip"] = dict(u8=dst["clip", "u8"].numel(), i420=dst["clip", "i420"].numel(), jpeg=last["clip"].nbytes,
                             jpeg_fixed_latents=last["decode"].nbytes, png=last["clip_png"].nbytes,
                             png_fixed_latents=last["decode_png"].nbytes)
# the files of the last repetition are the definition's for the first and the last frame of the clip
u8 = dst["clip", "u8"]
want = pkg.host_models.jpeg_encode_rgb8(u8[[0, T - 1]], QUALITY)
res["jpeg_equals_definition"] = bool(bytes(last["clip"][0]) == want[0] and bytes(last["clip"][T - 1]) == want[1])
want = pkg.host_models.png_encode_rgb8(u8[[0, T - 1]])
res["png_equals_definition"] = bool(bytes(last["clip_png"][0]) == want[0] and bytes(last["clip_png"][T - 1]) == want[1])
print(json.dumps(res))
