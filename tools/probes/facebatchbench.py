"""The face detector on n stacked views (float_sfd_detect_batch) against the loop of single calls, in time; seeded weights of the
real shapes (weights.synth_sfd_state, the bias of every head's face logit lowered by 3.5 as in facedetbench.py), fp16.
Part 1, the detector's launches: for N = 1 / 4 / 16 views of 360 x 270 and of 360 x 640, device events around ONE
float_sfd_detect_batch on the N views and around N float_sfd_detect calls on the same views (the raw calls: forward, decode,
selection; no read-back), taking turns.
Part 2, the wrapper with its read-back, N = 16: FaceDetectorHIP.detect_batch (one device-to-host copy) against 16 detect calls
(two copies and a synchronisation each), host clock between two device synchronisations.
Part 3, the product call: InferenceAgent.host_inputs_batch against B x host_inputs with face_align on B = 4 pageable
1920 x 1080 portraits under FLOAT_AMD_FACE_DETECTOR=device, taking turns, host clock between two device synchronisations.
REPS (default 20) rounds after WARMUP (default 3) in one process; prints one JSON line with median, min, max and spread
(max - min) per form, ms.  Run from the repository root."""
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from tests.util import load_pkg  # noqa: E402

pkg = load_pkg()
native = pkg.native
REPS, WARMUP = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3"))
PRODUCT = os.environ.get("PRODUCT", "1") != "0"
dev = "cuda:0"
state = pkg.weights.synth_sfd_state(seed=5)
for k in state:
    if k.endswith("_mbox_conf.bias"):
        state[k] = state[k].clone()
        state[k][-1] -= 3.5


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), spread=round(max(v) - min(v), 3))


def event_ms(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rounds(forms, clock):
    """forms: {name: callable}; every round runs each form once, in turn"""
    for _ in range(WARMUP):
        for f in forms.values():
            clock(f)
    ms = {k: [] for k in forms}
    for _ in range(REPS):
        for k, f in forms.items():
            ms[k].append(clock(f))
    out = {k: stats(v) for k, v in ms.items()}
    a, b = out["single_loop"], out["stacked"]
    out["loop_over_stacked"] = round(a["median"] / b["median"], 3)
    out["gain_exceeds_spread"] = bool(a["median"] - b["median"] > max(a["spread"], b["spread"]))
    return out


res = dict(probe="facebatchbench", reps=REPS, warmup=WARMUP, dtype="fp16")
L, st = native.lib(), native.stream_ptr(torch.device(dev))
det = pkg.face.FaceDetectorHIP(state, dev, dtype="fp16", max_hw=(360, 640))
for hw in ((360, 270), (360, 640)):
    for n in (1, 4, 16):
        views = torch.from_numpy(np.random.RandomState(hw[1] + n).randint(0, 256, size=(n,) + hw + (3,)).astype(np.uint8)).to(dev)
        det.reserve_batch(n, *hw)

        def stacked():
            native.check(L.float_sfd_detect_batch(det._h, C.c_void_p(views.data_ptr()), n, hw[0], hw[1], 0.5, 0.3,
                                                  C.c_void_p(det._bboxes.data_ptr()), C.c_void_p(det._bcounts.data_ptr()), st))

        def single_loop():
            for i in range(n):
                native.check(L.float_sfd_detect(det._h, C.c_void_p(views[i].data_ptr()), hw[0], hw[1], 0.5, 0.3,
                                                C.c_void_p(det._boxes.data_ptr()), C.c_void_p(det._counts.data_ptr()), st))
        r = rounds({"single_loop": single_loop, "stacked": stacked}, event_ms)
        r["counts_view0"] = det._bcounts[0].tolist()
        res["launches_%dx%d_n%d" % (hw[0], hw[1], n)] = r
        if n == 16:
            before = det.fallbacks
            r = rounds({"single_loop": lambda: [det.detect(views[i]) for i in range(n)], "stacked": lambda: det.detect_batch(views)}, host_ms)
            r["fallbacks"] = det.fallbacks - before
            res["wrapper_%dx%d_n16" % hw] = r
res["saturation"] = det.saturation()
det.close()

if PRODUCT:
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.nfe, opt.input_size, opt.fps, opt.rank = 10, 512, 25.0, dev
    cfg, acfg = pkg.config.FmtConfig(), pkg.config.AudioConfig()
    parts = dict(enc=pkg.weights.synth_encoder_state(512, seed=1), dec=pkg.weights.synth_decoder_state(512, seed=1),
                 fmt=pkg.weights.synth_fmt_state(cfg, seed=1), audio_encoder=(pkg.weights.synth_audio_state(acfg, seed=1), acfg))
    agent = gen.InferenceAgent(opt, parts, dev, max_frames=32, use_graph=2)
    wave = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(16000) / 16000)).astype("float32")
    B = 4
    auds = [{"waveform": torch.from_numpy(wave)[None, None], "sample_rate": 16000} for _ in range(B)]
    yy, xx = np.mgrid[0:1080, 0:1920].astype("float32")
    imgs = [torch.from_numpy(np.ascontiguousarray((np.stack([xx / 1920, yy / 1080, 0.5 + 0.5 * np.sin(xx / (31.0 + 3 * i))], axis=-1) * 0.8 +
                                                   0.2 * np.random.RandomState(i).rand(1080, 1920, 3)).astype("float32")))[None] for i in range(B)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s3fd.pth")
        torch.save(state, path)
        os.environ["FLOAT_AMD_SFD_WEIGHTS"] = path
        os.environ["FLOAT_AMD_FACE_DETECTOR"] = "device"
        r = rounds({"single_loop": lambda: [agent.host_inputs(im, au, no_crop=False) for im, au in zip(imgs, auds)],
                    "stacked": lambda: agent.host_inputs_batch(imgs, auds, no_crop=False)}, host_ms)
        r["fallbacks"], r["portraits"] = agent.face.fallbacks, B
        res["host_inputs_1920x1080_b4"] = r
        os.environ.pop("FLOAT_AMD_FACE_DETECTOR", None)
        os.environ.pop("FLOAT_AMD_SFD_WEIGHTS", None)
print(json.dumps(res))
