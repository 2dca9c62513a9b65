"""Clips of DIFFERENT lengths: three ways to run a batch of 16 clips between 2 s and 20 s (a fixed list, 89 windows in all), in one
process, on the benchmark's shapes (512 px, 51 grid points, decode batches of 32, seeded weights of the checkpoint's shapes):
  loop     the per-clip loop: InferenceAgent.infer_device / the one-clip FMT handle, clip after clip;
  padded   every clip padded to the longest (audio with silence) through the equal-length stacked chain
           (InferenceAgent.infer_device_batch / float_fmt_sample_batch): windows nobody wants are sampled and decoded;
  ragged   the ragged stacked chain (float_fmt_sample_batch_ragged): a clip leaves the stack after its last window.
Two timings per strategy, device events around the call: `fmt` = the FMT stage alone on conditions computed beforehand, `call` =
the whole product call (encoders, FMT, decode, frames in pinned host memory as uint8 - fp32 frames of the padded form would
pin 25 GB).  WARMUP (default 2) rounds first, so every stack height's graph exists, then REPS (default 10) rounds with the three
strategies taking turns.  Before the warm-up, on the fresh 16-clip handle: the one-off cost of the first window at each new
stack height (capture + instantiate of its graph) = first call - second call of a one-window job, host clock around a
synchronised call, and the device memory the 15 graphs hold (drop of the device's free memory across those calls, every tensor
allocated beforehand; the growth of torch's allocator in between is reported beside it).
Prints one JSON line, ms per batch: median, min, max.  Run from the repository root.  Environment: REPS, WARMUP, NFE, SIZE."""
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from tests.util import load_pkg  # noqa: E402

pkg = load_pkg()
REPS, WARMUP = int(os.environ.get("REPS", "10")), int(os.environ.get("WARMUP", "2"))
NFE, SIZE, MAX_FRAMES = int(os.environ.get("NFE", "51")), int(os.environ.get("SIZE", "512")), 32
SECONDS = [9.4, 2.0, 17.0, 5.0, 12.9, 3.2, 20.0, 7.3, 10.0, 4.4, 15.5, 8.0, 18.6, 6.1, 14.2, 11.7]  # caller order, not sorted
B = len(SECONDS)
dev = "cuda:0"

cfg = pkg.config.FmtConfig()
L = cfg.num_frames_for_clip
gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
opt.nfe, opt.input_size, opt.fps, opt.rank = NFE, SIZE, 25.0, dev
acfg = pkg.config.AudioConfig()
parts = dict(enc=pkg.weights.synth_encoder_state(SIZE, seed=1), dec=pkg.weights.synth_decoder_state(SIZE, seed=1),
             fmt=pkg.weights.synth_fmt_state(cfg, seed=1), audio_encoder=(pkg.weights.synth_audio_state(acfg, seed=1), acfg))
agent = gen.InferenceAgent(opt, parts, dev, max_frames=MAX_FRAMES, use_graph=2)
hp = agent.G
seeds = [15 + i for i in range(B)]


def portrait(seed):
    return (torch.from_numpy(np.random.RandomState(seed).rand(1, 3, SIZE, SIZE).astype("float32")) * 2 - 1).to(dev)


items = [(portrait(i), pkg.weights.synth_waveform(s, seed=1 + i).to(dev)) for i, s in enumerate(SECONDS)]
n_max = max(a.shape[-1] for _, a in items)
padded_items = [(s, torch.nn.functional.pad(a, (0, n_max - a.shape[-1]))) for s, a in items]
conds = [agent.conditions_device(s, a, "neutral") for s, a in items]
Ts = [c["T"] for c in conds]
wins = [int(math.ceil(T / L)) for T in Ts]
T_max, w_max = max(Ts), max(wins)
noise = [pkg.fmt.draw_noise(w, 1, cfg, seeds[i]).to(dev) for i, w in enumerate(wins)]
noise_pad = torch.cat([pkg.fmt.draw_noise(w_max, 1, cfg, seeds[i]) for i in range(B)], dim=1).to(dev)
r_s = torch.cat([c["r_s"].reshape(1, -1) for c in conds])
wa_list = [c["wa"].reshape(c["T"], -1) for c in conds]
we_list = [c["we"].reshape(1, -1) for c in conds]
wa_pad = torch.stack([torch.cat([w, w[-1:].expand(T_max - w.shape[0], -1)]) for w in wa_list])
we_cat = torch.cat([c["we"].reshape(1, 1, -1) for c in conds])
many = hp.batched_fmt(B)
assert many.max_batch == B, "the stacked handle holds %d clips, not %d" % (many.max_batch, B)
scales = (2.0, 1.0, 1.0)


# ---- one-off cost of a new stack height, on the fresh handle
wa_one, nz_one = [w[:L].contiguous() for w in wa_list], [z[:1].reshape(1, L, -1).contiguous() for z in noise]
out_one = [torch.empty(L, cfg.dim_w, device=dev) for _ in range(B)]  # every tensor of the call exists beforehand: what
# mem_get_info loses below is held by the HIP runtime for the graphs, not by torch's allocator


def one_window(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    many.sample_ragged(r_s[:n], wa_one[:n], we_list[:n], nz_one[:n], NFE, *scales, out=out_one[:n])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


one_window(B)  # module load, first-launch costs and the graph of the full stack: not part of the figure below
reserved0, free0 = torch.cuda.memory_reserved(dev), torch.cuda.mem_get_info(dev)[0]
capture = {}
for n in range(B - 1, 0, -1):
    first, second = one_window(n), one_window(n)
    capture[n] = dict(first=round(first, 2), replay=round(second, 2), capture=round(first - second, 2))
graph_mb = (free0 - torch.cuda.mem_get_info(dev)[0]) / 2**20
torch_mb = (torch.cuda.memory_reserved(dev) - reserved0) / 2**20  # 0 unless torch's allocator grew in between
keep = {}


def fmt_loop():
    keep["f"] = [hp.fmt.sample(r_s[i:i + 1], wa_list[i][None], we_cat[i:i + 1], noise[i], NFE, *scales) for i in range(B)]


def fmt_padded():
    keep["f"] = many.sample(r_s, wa_pad, we_cat, noise_pad, NFE, *scales)


def fmt_ragged():
    keep["f"] = many.sample_ragged(r_s, wa_list, we_list, noise, NFE, *scales)


def call_loop():
    keep["c"] = None
    keep["c"] = [agent.infer_device(s, a, *scales, emo="neutral", seed=seeds[i], out_dtype=torch.uint8) for i, (s, a) in enumerate(items)]


def call_padded():
    keep["c"] = None
    keep["c"] = agent.infer_device_batch(padded_items, *scales, "neutral", seeds, out_dtype=torch.uint8)


def call_ragged():
    keep["c"] = None
    keep["c"] = agent.infer_device_batch(items, *scales, "neutral", seeds, out_dtype=torch.uint8)


def ev_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    hp.release_host_inflight()
    return e0.elapsed_time(e1)


def case(fs):
    for _ in range(WARMUP):
        for f in fs.values():
            ev_ms(f)
    ms = {k: [] for k in fs}
    for _ in range(REPS):
        for k, f in fs.items():  # taking turns: drift of the box lands on all three
            ms[k].append(ev_ms(f))
    return {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in ms.items()}


res = dict(probe="raggedbench", size=SIZE, nfe=NFE, clips=B, seconds=SECONDS, frames=Ts, windows=sum(wins),
           windows_padded=B * w_max, reps=REPS, warmup=WARMUP)
res["fmt_ms"] = case(dict(loop=fmt_loop, padded=fmt_padded, ragged=fmt_ragged))
res["call_ms"] = case(dict(loop=call_loop, padded=call_padded, ragged=call_ragged))
for k in ("fmt_ms", "call_ms"):
    res[k]["ragged_beats_loop"] = res[k]["ragged"]["median"] < res[k]["loop"]["median"]
    res[k]["ragged_beats_padded"] = res[k]["ragged"]["median"] < res[k]["padded"]["median"]
res["frames_per_s_call"] = {k: round(sum(Ts) / res["call_ms"][k]["median"] * 1e3, 1) for k in ("loop", "padded", "ragged")}
cap = [v["capture"] for v in capture.values()]
res["new_stack_height"] = dict(capture_ms_median=round(statistics.median(cap), 2), capture_ms_min=min(cap), capture_ms_max=max(cap),
                               graphs=len(cap), graphs_device_mb=round(graph_mb, 1), of_which_torch_allocator_mb=round(torch_mb, 1),
                               per_height=capture)
print(json.dumps(res))
