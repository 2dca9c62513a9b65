"""Dynamic-emotion timing probe: the xlsr speech-emotion shape (emotion_audio_config, seeded weights, fp16) on clips of 10 s
and 60 s in 2-s chunks (5 and 30 chunks), three forms interleaved in one process, wall-clock ms per clip (the host waits for
the result at the end of every repetition), medians of 20 after warm-up and the spread max - min:
  (a) the per-chunk loop the node ran before: normalise the chunk in torch, predict_emotion, then .cpu() of the list and
      F.interpolate(mode="nearest") on the host;
  (b) the same loop without the final .cpu() (the scores stay on the device, no expansion);
  (c) Audio2EmotionHIP.predict_emotion_chunks: one stacked pass, normalisation and expansion as kernels.
Launches of (c) are counted from its launch sequence with one kernel per Linear layer (what the GEMM service runs at these
shapes unless its tuning says otherwise).
DYNEMO_AGENT=1 (default): also infer_device(emo="dynamic") against emo="none" on the 512-px synthetic model, 10-s clip."""
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from tests.util import load_pkg  # noqa: E402

pkg = load_pkg()
REPS, WARM, RATE, CHUNK, FPS = 20, 3, 16000, 32000, 25.0
ecfg = pkg.config.emotion_audio_config()
ser = pkg.audio.Audio2EmotionHIP(pkg.weights.synth_audio_state(ecfg, seed=2), ecfg, "cuda:0", "fp16")


def loop(w, to_host):
    n = math.ceil(w.shape[0] / CHUNK)
    seq = []
    for i in range(n):
        p = w[i * CHUNK:(i + 1) * CHUNK]
        p = ((p - p.mean()) / torch.sqrt(p.var(unbiased=False) + 1e-7))[None]
        seq.append(ser.predict_emotion(p))
    seq = torch.cat(seq)[None]
    if not to_host:
        return seq
    seq = seq.cpu()
    T = math.ceil(w.shape[0] / RATE * FPS)
    return F.interpolate(seq.transpose(1, 2), size=T, mode="nearest").transpose(1, 2) if n > 1 else seq.repeat(1, T, 1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(forms):
    ts = {k: [] for k in forms}
    for r in range(WARM + REPS):
        for k, fn in forms.items():
            t = timed(fn)
            if r >= WARM:
                ts[k].append(t)
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in ts.items()}


for seconds in (10.0, 60.0):
    w = (pkg.weights.synth_waveform(seconds, seed=3)[0] * 0.2 + 0.05).cuda()
    T = math.ceil(w.shape[0] / RATE * FPS)
    res = interleaved({"a": lambda: loop(w, True), "b": lambda: loop(w, False), "c": lambda: ser.predict_emotion_chunks(w, CHUNK, T)})
    d = float((ser.predict_emotion_chunks(w, CHUNK, T)[0] - loop(w, False)[0]).abs().max())
    launches = 1 + 1 + 2 * (len(ecfg.conv_dim) - 1) + 2 + 2 + 7 * ecfg.num_hidden_layers + 4 + 1
    print("%2.0f s, %2d chunks: (a) loop + .cpu() %.3f ms (spread %.3f) | (b) loop %.3f ms (spread %.3f) | (c) stacked %.3f ms (spread %.3f), "
          "%d launches | max |c - b| %.2e" % (seconds, math.ceil(w.shape[0] / CHUNK), *res["a"], *res["b"], *res["c"], launches, d))

if os.environ.get("DYNEMO_AGENT", "1") != "0":
    import importlib
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    agent = gen.InferenceAgent(opt, gen.InferenceAgent.synthetic_parts(opt), "cuda:0")
    s = (torch.rand(1, 3, opt.input_size, opt.input_size, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    a = pkg.weights.synth_waveform(10.0, seed=3)[0].cuda()
    res = interleaved({"none": lambda: agent.infer_device(s, a, 1.0, 1.0, 3.0, emo="none", seed=7),
                       "dynamic": lambda: agent.infer_device(s, a, 1.0, 1.0, 3.0, emo="dynamic", seed=7)})
    print("infer_device, %d px, 10-s clip: emo='none' %.2f ms (spread %.2f) | emo='dynamic' %.2f ms (spread %.2f)" % (
        opt.input_size, *res["none"], *res["dynamic"]))
