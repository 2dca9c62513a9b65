"""The streamed clip against the whole-clip call, interleaved in one process, on the benchmark's shapes (bench.py config 1: a 10-s
clip at 512 px = 250 frames = 5 FMT windows, 51 grid points, decode batches of 32, seeded weights of the checkpoint's shapes).
Per output format (fp32, u8, i420) two forms take turns:
  whole    InferenceAgent.infer_device into a pinned destination allocated before the first repetition;
  stream   InferenceAgent.stream_device (SLOTS ring buffers, default 3) with a consumer that reads one sample of each block.
Times are host-clock milliseconds from a synchronised device to the moment the host holds the frames (infer_device returns after
its stream synchronise; a block is timed when it is yielded, i.e. after its event):
  whole_ms        infer_device wall time;
  first_block_ms  start -> the first yielded block (50 frames);
  last_block_ms   start -> the last yielded block;
  end_ms          start -> the generator exhausted (adds the range check's counter reads).
REPS (default 20) repetitions per form after WARMUP (default 3).  Prints one JSON line: median, min, max and spread (max - min),
`stream_minus_whole_ms` = median last_block_ms - median whole_ms (what the per-window decode calls leave exposed: five
hand-over flushes per clip instead of one, five short decode tails), the pinned bytes each form holds (slots x block against T x
frame), and whether the blocks of the last repetition equal the whole-clip frames bitwise.  Run from the repository root.
The ring is allocated inside the first next() of every stream; after WARMUP the host allocator hands cached pinned blocks back, so
first_block_ms is the steady-state figure, not the latency of a cold first call (which adds the pinned allocation).
Environment: REPS, WARMUP, SLOTS."""
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
REPS, WARMUP, SLOTS = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3")), int(os.environ.get("SLOTS", "3"))
SIZE, SECONDS, NFE, MAX_FRAMES, T = 512, 10.0, 51, 32, 250
dev = "cuda:0"
if not torch.cuda.is_available():
    sys.exit("streambench measures on the GPU: no device visible")
for v in ("FLOAT_AMD_VERIFY", "FLOAT_AMD_OVERLAP"):
    os.environ.pop(v, None)

cfg = pkg.config.FmtConfig()
gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
opt.nfe, opt.input_size, opt.fps, opt.rank = NFE, SIZE, 25.0, dev
acfg = pkg.config.AudioConfig()
parts = dict(enc=pkg.weights.synth_encoder_state(SIZE, seed=1), dec=pkg.weights.synth_decoder_state(SIZE, seed=1),
             fmt=pkg.weights.synth_fmt_state(cfg, seed=1), audio_encoder=(pkg.weights.synth_audio_state(acfg, seed=1), acfg))
agent = gen.InferenceAgent(opt, parts, dev, max_frames=MAX_FRAMES, use_graph=2)
img = (torch.from_numpy(np.random.RandomState(0).rand(1, 3, SIZE, SIZE).astype("float32")) * 2 - 1).to(dev)
wav = pkg.weights.synth_waveform(SECONDS, seed=1).to(dev)

FORMATS = dict(fp32=dict(out_dtype=torch.float32), u8=dict(out_dtype=torch.uint8), i420=dict(out_format="i420"))
SHAPES = dict(fp32=(SIZE, SIZE, 3), u8=(SIZE, SIZE, 3), i420=(3 * SIZE // 2, SIZE))
DTYPES = dict(fp32=torch.float32, u8=torch.uint8, i420=torch.uint8)
dst = {f: torch.empty((T,) + SHAPES[f], dtype=DTYPES[f]).pin_memory() for f in FORMATS}
L = cfg.num_frames_for_clip


def whole(fmt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15, out=dst[fmt], **FORMATS[fmt])
    return dict(whole_ms=(time.perf_counter() - t0) * 1e3)


def stream(fmt, keep=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stamps, touched = [], 0
    for blk in agent.stream_device(img, wav, 2.0, 1.0, 1.0, emo="neutral", seed=15, slots=SLOTS, **FORMATS[fmt]):
        stamps.append((time.perf_counter() - t0) * 1e3)
        touched += int(blk.frames.reshape(-1)[0] > 0)  # the consumer only touches the block
        if keep is not None:
            keep.append(blk.frames.clone())
    end = (time.perf_counter() - t0) * 1e3
    assert len(stamps) == (T + L - 1) // L
    return dict(first_block_ms=stamps[0], last_block_ms=stamps[-1], end_ms=end)


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), spread=round(max(v) - min(v), 3))


res = dict(probe="streambench", size=SIZE, frames=T, windows=(T + L - 1) // L, nfe=NFE, max_frames=MAX_FRAMES, slots=SLOTS,
           reps=REPS, warmup=WARMUP)
for _ in range(WARMUP):
    for fmt in FORMATS:
        whole(fmt)
        stream(fmt)
ms = {fmt: {} for fmt in FORMATS}
for _ in range(REPS):
    for fmt in FORMATS:  # taking turns: drift of the box lands on both forms and all formats
        for k, v in list(whole(fmt).items()) + list(stream(fmt).items()):
            ms[fmt].setdefault(k, []).append(v)
for fmt in FORMATS:
    out = {k: stats(v) for k, v in ms[fmt].items()}
    out["stream_minus_whole_ms"] = round(out["last_block_ms"]["median"] - out["whole_ms"]["median"], 3)
    frame = int(np.prod(SHAPES[fmt])) * dst[fmt].element_size()
    out["pinned_bytes"] = dict(whole=T * frame, stream=SLOTS * L * frame)
    out["device_staging_bytes"] = dict(whole=T * frame, stream=L * frame)
    blocks = []
    whole(fmt)
    stream(fmt, keep=blocks)
    out["stream_equals_whole"] = bool(torch.equal(torch.cat(blocks), dst[fmt]))
    res[fmt] = out
print(json.dumps(res))
