"""JPEG decode timing probe: a 10-s driving clip (250 frames of 1920 x 1080) as Motion-JPEG files (quality 90, 4:2:0, made by
float_jpg_encode_padded from a smooth moving pattern with noise), with one restart interval per MCU row and without restart
markers.  All routes interleaved in one process, medians of JPEGDEC_REPS (10) repetitions after warm-up, spread max - min:
  (a) float_jpg_decode alone, files already in HBM: device-event ms per clip and GB/s of output pixels, both clips.
  (b) InferenceAgent.drive_video (512-px synthetic model, rects given, wall clock) from: the MJPEG files with restart markers;
      the files without; the raw pageable uint8 host video (the route before this decoder); a Pillow decode loop on the host
      feeding that raw route (the Pillow loop is also reported alone).
Bytes across PCIe: the files against T x 1080 x 1920 x 3.  JPEGDEC_FRAMES / JPEGDEC_REPS shrink the run for a rehearsal.
--entropy sync|auto adds, interleaved with the others: to (a) the clip without restart markers through that entropy route, once per
value of --sync-bytes (a comma list, default: the library's), with the relaxation's rounds over the last group's frames; to (b)
drive_video from that clip with entropy= set.
--entropy split adds a third clip with one restart marker every 17 MCU rows (4 intervals a frame, a capture card's shape) and,
interleaved with the others: to (a) that clip without it, both clips WITH markers through the split route once per value of
--sync-bytes, and the clip without markers under "auto" for comparison; to (b) drive_video from the three."""
import argparse
import importlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, ".")
from tests.util import load_pkg  # noqa: E402

pkg = load_pkg()
J, Wt = pkg.jpeg, pkg.weights
ap = argparse.ArgumentParser()
ap.add_argument("--entropy", choices=("sync", "auto", "split"), default=None)
ap.add_argument("--sync-bytes", default="")
args = ap.parse_args()
SYNC = [int(v) for v in args.sync_bytes.split(",") if v] or [None]
T, REPS, WARM = int(os.environ.get("JPEGDEC_FRAMES", 250)), int(os.environ.get("JPEGDEC_REPS", 10)), 2
H, W = 1080, 1920
RECT = (460, 40, 1000, 1000)

g = torch.Generator(device="cuda").manual_seed(2)
yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
frames = torch.empty(T, H, W, 3, dtype=torch.uint8, device="cuda")
for t in range(T):
    base = torch.stack([128 + 100 * torch.sin((xx + 3 * t) / 70.0 + c) * torch.cos(yy / 50.0 - c) for c in range(3)], -1)
    frames[t] = (base + 6 * torch.randn(H, W, 3, device="cuda", generator=g)).clamp_(0, 255).to(torch.uint8)
clips = {}
COARSE = "restart every 17 MCU rows"
for name, restart in (("restart per MCU row", None), ("no restart markers", 0)) + (((COARSE, 17 * -(-W // 16)),) if args.entropy == "split" else ()):
    data, offsets = J.encode_jpeg_device(frames, 90, restart, pad="edge")
    clips[name] = J.to_host(data, offsets.cpu())
del frames
video8 = J.decode_jpeg_device(clips["restart per MCU row"]).cpu()  # pageable: what the raw route is handed
print("%d frames of %d x %d: %.1f MB of files (%.1f MB without restart markers) against %.1f MB raw" % (
    T, W, H, clips["restart per MCU row"].nbytes / 1e6, clips["no restart markers"].nbytes / 1e6, video8.numel() / 1e6))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# (a) the decode launches alone
resident = {}
variants = [(name, name, None, None) for name in clips]
if args.entropy == "split":
    variants += [("%s, split%s" % (c, "" if S is None else " S=%d" % S), c, "split", S) for c in ("restart per MCU row", COARSE) for S in SYNC]
    variants += [("no restart markers, auto", "no restart markers", "auto", None)]
elif args.entropy:
    variants += [("no restart markers, %s%s" % (args.entropy, "" if S is None else " S=%d" % S), "no restart markers", args.entropy, S) for S in SYNC]
for name, clip, entropy, S in variants:
    data, edges = J.host_files(clips[clip])
    plan = J.JpegPlan(data, edges, entropy, S)
    resident[name] = (data.cuda(), edges.cuda(), plan, torch.empty(plan.n, H, W, 3, dtype=torch.uint8, device="cuda"),
                      torch.empty(plan.n, dtype=torch.int32, device="cuda"), torch.empty(plan.work_bytes, dtype=torch.uint8, device="cuda"))
ta = {k: [] for k in resident}
for r in range(WARM + REPS):
    for k, (d, e, plan, out, st, work) in resident.items():
        ms = event_ms(lambda: J.enqueue_decode(d, e, plan, out, st, work))
        if r >= WARM:
            ta[k].append(ms)
for k, v in ta.items():
    m = statistics.median(v)
    print("(a) decode, %-34s %9.2f ms per clip (spread %.2f) | %.1f GB/s of pixels | equal to the other clip's frames: %s" % (
        k, m, max(v) - min(v), T * H * W * 3 / m / 1e6, torch.equal(resident[k][3], next(iter(resident.values()))[3])))
    plan, work = resident[k][2], resident[k][5]
    route = plan.ints[16:16 + 8 * plan.n].view(-1, 8)[:, 5]
    if int(route.abs().max()):  # frames on the sync or the split route: the lane table ends a frame's share of `work`
        per, table = plan.work_bytes // min(plan.n, plan.group), 40992 if int(route.min()) < 0 else 24608
        rounds = work[:plan.work_bytes].view(-1, per)[:(plan.n - 1) % plan.group + 1, per - table:][:, 8:20].contiguous().view(torch.int32).cpu()
        print("    relaxation: %s lanes, rounds min %d median %d max %d (the last group's frames)" % (
            sorted(set(rounds[:, 0].tolist())), rounds[:, 2].min(), rounds[:, 2].median(), rounds[:, 2].max()))
del resident

# (b) through the agent
gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
opt.input_size = 512
acfg = pkg.config.small_audio_config()
acfg.dim_w = opt.dim_w
parts = dict(enc=Wt.synth_encoder_state(512, seed=31), dec=Wt.synth_decoder_state(512, seed=31),
             fmt=Wt.synth_fmt_state(pkg.config.FmtConfig.from_options(opt), seed=31), audio_encoder=(Wt.synth_audio_state(acfg, seed=31), acfg))
agent = gen.InferenceAgent(opt, parts, "cuda:0")
portrait = torch.rand(1, 512, 512, 3, generator=torch.Generator().manual_seed(3))
pil_files = [bytes(f) for f in clips["restart per MCU row"]]


def pillow_loop():
    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in pil_files]))


drive = lambda v: agent.drive_video(portrait, v, rects=RECT, out_dtype=torch.uint8)  # noqa: E731
routes = {"mjpeg, restart per MCU row": lambda: drive(clips["restart per MCU row"]),
          "mjpeg, no restart markers": lambda: drive(clips["no restart markers"]),
          "raw pageable uint8 video": lambda: drive(video8),
          **({"mjpeg, no restart markers, " + args.entropy: lambda: agent.drive_video(portrait, clips["no restart markers"], rects=RECT, out_dtype=torch.uint8,
                                                                                      entropy=args.entropy)} if args.entropy in ("sync", "auto") else {}),
          **({"mjpeg, restart per MCU row, split": lambda: agent.drive_video(portrait, clips["restart per MCU row"], rects=RECT, out_dtype=torch.uint8, entropy="split"),
              "mjpeg, " + COARSE: lambda: drive(clips[COARSE]),
              "mjpeg, " + COARSE + ", split": lambda: agent.drive_video(portrait, clips[COARSE], rects=RECT, out_dtype=torch.uint8, entropy="split"),
              "mjpeg, no restart markers, auto": lambda: agent.drive_video(portrait, clips["no restart markers"], rects=RECT, out_dtype=torch.uint8, entropy="auto")}
             if args.entropy == "split" else {}),
          "pillow loop + raw route": lambda: drive(pillow_loop()),
          "pillow loop alone": pillow_loop}
tb = {k: [] for k in routes}
for r in range(1 + REPS):
    for k, fn in routes.items():
        ms = wall_ms(fn)
        if r >= 1:
            tb[k].append(ms)
for k, v in tb.items():
    print("(b) %-42s %9.1f ms per clip (spread %.1f)" % (k, statistics.median(v), max(v) - min(v)))
