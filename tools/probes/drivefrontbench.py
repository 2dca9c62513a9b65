"""Driving-video front-end timing probe: a 10-s clip (250 frames of 1920 x 1080, fp32 RGB, already in HBM), two forms interleaved
in one process, device-event ms per clip, medians of 20 after warm-up and the spread max - min:
  (a) crops: a 1000-px window -> 512 px.  `loop`: 250 float_img_front calls through ctypes, each writing its 8-bit frame
      straight into the stack, one scratch made beforehand and shared - what a caller could do before; `frames`: one
      float_img_front_frames call.
  (b) views: the whole frame -> 360 x 640, the same two forms.
  (c) InferenceAgent.drive_video on a pageable uint8 host video against drive_device on crops made beforehand (512-px synthetic
      model, wall clock, DRIVEFRONT_C_REPS = 5 repetitions: the host copy dominates).
  (d) the fraction of float_probe_peaks' streaming read that (a) `frames` reaches on the windows' bytes (12 per pixel).
Also: the bytes of the two forms are compared.  DRIVEFRONT_FRAMES / DRIVEFRONT_REPS shrink the run for a rehearsal."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from tests.util import load_pkg  # noqa: E402

pkg = load_pkg()
N, I = pkg.native, pkg.image
T, REPS, WARM = int(os.environ.get("DRIVEFRONT_FRAMES", 250)), int(os.environ.get("DRIVEFRONT_REPS", 20)), 3
C_REPS = int(os.environ.get("DRIVEFRONT_C_REPS", 5))
H, W = 1080, 1920
video8 = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))  # pageable
frames = video8.cuda().float().div_(255.0)
RECT = (460, 40, 1000, 1000)
out = {}


L, st = N.lib(), N.stream_ptr("cuda:0")
work = torch.empty(max(int(L.float_img_front_work_bytes(H, W, 512, 512)), int(L.float_img_front_work_bytes(H, W, 360, 640))) // 4,
                   dtype=torch.int32, device="cuda")


def loop(dst_h, dst_w, rect, scale, key):
    o = out.setdefault(key, torch.empty(T, dst_h, dst_w, 3, dtype=torch.uint8, device="cuda"))
    x0, y0, w, h = rect
    src, dst, step_in, step_out = frames.data_ptr(), o.data_ptr(), H * W * 3 * 4, dst_h * dst_w * 3
    for t in range(T):
        N.check(L.float_img_front(C.c_void_p(src + t * step_in), H, W, 3, x0, y0, w, h, scale[0], scale[1], 0, 0, 0, 0, N.IMG_OUT_HWC_U8,
                                  C.c_void_p(dst + t * step_out), dst_h, dst_w, C.c_void_p(work.data_ptr()), work.numel() * 4, st))


def fused(dst_h, dst_w, rect, scale, key):
    out[key] = I.front_frames_device(frames, rect, dst_h, dst_w, scale=scale, out=out.get(key))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


forms = {"a loop": lambda: loop(512, 512, RECT, (0, 0), "al"), "a frames": lambda: fused(512, 512, RECT, None, "af"),
         "b loop": lambda: loop(360, 640, (0, 0, W, H), (3, 1), "bl"), "b frames": lambda: fused(360, 640, (0, 0, W, H), (3, 1), "bf")}
ts = {k: [] for k in forms}
for r in range(WARM + REPS):
    for k, fn in forms.items():
        t = timed(fn)
        if r >= WARM:
            ts[k].append(t)
print("%d fp32 RGB frames of %d x %d in HBM" % (T, W, H))
for k, v in ts.items():
    print("(%s) %-7s %9.3f ms per clip (spread %.3f) | %.2f us per frame" % (k[0], k[2:], statistics.median(v), max(v) - min(v),
                                                                           statistics.median(v) / T * 1e3))
print("bytes equal: crops %s, views %s" % (torch.equal(out["al"], out["af"]), torch.equal(out["bl"], out["bf"])))
peak = N.probe_peaks("cuda:0")["hbm_read_GBps"]
gbps = T * RECT[2] * RECT[3] * 12 / statistics.median(ts["a frames"]) / 1e6
print("(d) the windows' bytes at %.0f GB/s = %.3f of the streaming read of this box (%.0f GB/s)" % (gbps, gbps / peak, peak))

# (c) through the agent
del frames
gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
opt.input_size = 512
acfg = pkg.config.small_audio_config()
acfg.dim_w = opt.dim_w
Wt = pkg.weights
parts = dict(enc=Wt.synth_encoder_state(512, seed=31), dec=Wt.synth_decoder_state(512, seed=31),
             fmt=Wt.synth_fmt_state(pkg.config.FmtConfig.from_options(opt), seed=31), audio_encoder=(Wt.synth_audio_state(acfg, seed=31), acfg))
agent = gen.InferenceAgent(opt, parts, "cuda:0")
portrait = torch.rand(1, 512, 512, 3, generator=torch.Generator().manual_seed(3))
s = agent.host_inputs(portrait, {"waveform": torch.zeros(1, 1, 16), "sample_rate": opt.sampling_rate})[0]
crops = agent.align_driving(video8, rects=RECT)[0]
tc = {"drive_video": [], "drive_device": []}
for r in range(1 + C_REPS):
    for k, fn in (("drive_video", lambda: agent.drive_video(portrait, video8, rects=RECT, out_dtype=torch.uint8)),
                  ("drive_device", lambda: agent.drive_device(s, crops, out_dtype=torch.uint8))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= 1:
            tc[k].append((time.perf_counter() - t0) * 1e3)
for k, v in tc.items():
    print("(c) %-12s %9.1f ms per clip (spread %.1f), pageable uint8 host video" % (k, statistics.median(v), max(v) - min(v)))
