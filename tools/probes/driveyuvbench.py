"""Driving video as YUV 4:2:0 against uint8 RGB: a 10-s clip (250 frames of 1920 x 1080, the same content in both forms), the forms
interleaved in one process, medians of DRIVEYUV_REPS = 20 after 3 warm-up rounds and the spread max - min.
  (a) the launches alone, frames in HBM, a 1000-px window -> 512 px, device events: `rgb8` float_img_front_frames on uint8 RGB,
      `yuv nearest` / `yuv centre` float_img_front_frames_yuv on --src i420 | nv12.
  (b) the bytes the windows hold (3 or 1.5 per pixel) over those times, against float_probe_peaks' streaming read of this box.
  (c) InferenceAgent.drive_video from a pageable host clip, uint8 RGB against the YUV form (512-px synthetic model, wall clock
      around a synchronise, DRIVEYUV_C_REPS = 5 repetitions).
Also: the YUV crops are compared with the definition on frame 0.  DRIVEYUV_FRAMES shrinks the run for a rehearsal.
--format NAME [--pitch BYTES] measures image.PlanarYuv (any planar YUV) instead of the above: planar() below says what."""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from tests.util import load_pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--src", choices=("i420", "nv12"), default="i420")
ap.add_argument("--format", default=None, help="an image.PLANAR_YUV_NAMES name: measure image.PlanarYuv instead (see planar())")
ap.add_argument("--pitch", type=int, default=None, help="with --format: bytes from one luma row to the next (chroma rows get the same padding)")
ARGS = ap.parse_args()
SRC = ARGS.src
pkg = load_pkg()
N, I, hm = pkg.native, pkg.image, pkg.host_models
T, REPS, WARM = int(os.environ.get("DRIVEYUV_FRAMES", 250)), int(os.environ.get("DRIVEYUV_REPS", 20)), 3
C_REPS = int(os.environ.get("DRIVEYUV_C_REPS", 5))
H, W = 1080, 1920
RECT = (460, 40, 1000, 1000)
if not torch.cuda.is_available():
    sys.exit("driveyuvbench: no GPU: nothing is measured")

# smooth content (a decoded video is not noise, though no kernel here depends on the values), made on the device
g = torch.Generator(device="cuda").manual_seed(2)
small = torch.rand(T, 3, H // 8, W // 8, device="cuda", generator=g)
rgb_d = torch.empty(T, H, W, 3, dtype=torch.uint8, device="cuda")
yuv_d = torch.empty(T, 3 * H // 2, W, dtype=torch.uint8, device="cuda")
for t in range(0, T, 10):
    up = torch.nn.functional.interpolate(small[t:t + 10], size=(H, W), mode="bilinear", align_corners=False)
    rgb_d[t:t + 10] = (up.permute(0, 2, 3, 1) * 255).round().to(torch.uint8)
    yuv_d[t:t + 10] = hm.rgb8_to_i420(rgb_d[t:t + 10], "bt709")
if SRC == "nv12":
    c = yuv_d[:, H:].reshape(T, 2, H // 2, W // 2)
    yuv_d[:, H:] = c.permute(0, 2, 3, 1).reshape(T, H // 2, W)
del small, up
rgb_h, yuv_h = rgb_d.cpu(), yuv_d.cpu()  # pageable
out = {}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def front(key, frames):
    out[key] = I.front_frames_device(frames, RECT, 512, 512, out=out.get(key))


def planar_clip(name, pitch):
    """The I420 content as a PlanarYuv `name` on the device: samples << (depth - 8), chroma rows / columns repeated for 4:2:2 / 4:4:4,
    luma rows `pitch` bytes apart (None: packed) and chroma rows with the same padding."""
    kw = I.PLANAR_YUV_NAMES[name]
    hs, vs = hm.YUV_SUBSAMPLING[kw["sub"]]
    depth, semi = kw.get("depth", 8), kw.get("semi", False)
    b = 1 if depth == 8 else 2
    pad = 0 if pitch is None else pitch - W * b
    pitches = dict(y_pitch=W * b + pad, c_pitch=W // hs * b * (2 if semi else 1) + pad)
    f = hm.yuv_planes_format(H, W, matrix="bt709", **dict(kw, **pitches))
    buf = torch.zeros((T - 1) * f.frame_stride + f.last_end, dtype=torch.uint8, device="cuda")
    words = buf.view(torch.int16) if b == 2 else buf
    c = yuv_d[:, H:].reshape(T, 2, H // 2, W // 2)
    for off, plane, pitch_, step in ((f.y_off, yuv_d[:, :H], f.y_pitch, b), (f.u_off, c[:, 0], f.c_pitch, f.c_step), (f.v_off, c[:, 1], f.c_pitch, f.c_step)):
        if plane.shape[1] != H:
            plane = plane.repeat_interleave(2 // vs, dim=1).repeat_interleave(2 // hs, dim=2)
        dst = torch.as_strided(words, tuple(plane.shape), (f.frame_stride // b, pitch_ // b, step // b), off // b)
        dst.copy_(plane.to(words.dtype) << (depth - 8 + kw.get("shift", 0)))
    return I.PlanarYuv.of(name, buf, H, W, matrix="bt709", **pitches)


def planar():
    """--format NAME [--pitch BYTES]: (a) the launches alone, frames in HBM, interleaved: `yuv420p` through the EXISTING
    float_img_front_frames_yuv (the yardstick), `yuv422p10le` and `p010` through float_img_front_frames_planes, both chroma rules;
    (c) drive_video from a pageable pitched NAME clip as an image.PlanarYuv, against the route without it: pack the rows, shift to
    8 bits and drop every second chroma row on the host with torch, then image.YuvFrames."""
    clips = {n: planar_clip(n, None) for n in ("yuv422p10le", "p010")}
    forms = {}
    for chroma in ("nearest", "centre"):
        forms["yuv420p %s (yuv call)" % chroma] = lambda c=chroma: front("y" + c, I.YuvFrames(yuv_d, H, W, "i420", "bt709", c))
        for n, clip in clips.items():
            forms["%s %s" % (n, chroma)] = lambda n=n, clip=clip, c=chroma: front(n + c, clip.like(clip.data, chroma=c))
    ts = {k: [] for k in forms}
    for r in range(WARM + REPS):
        for k, fn in forms.items():
            t = timed(fn)
            if r >= WARM:
                ts[k].append(t)
    print("%d frames of %d x %d in HBM, window %s -> 512 px" % (T, W, H, RECT))
    for k, v in ts.items():
        print("(a) %-30s %8.3f ms per clip (spread %.3f)" % (k, statistics.median(v), max(v) - min(v)))
    for n, clip in clips.items():
        one = clip[0:1]
        want = hm.resize_rgb8(one.like(one.data.cpu(), chroma="centre").to_rgb8()[0], RECT, 512, 512)
        print("frame 0, %s centre: equal to the definition: %s" % (n, torch.equal(out[n + "centre"][0].cpu(), want)))
    clips.clear()
    out.clear()
    dev = planar_clip(ARGS.format, ARGS.pitch)
    f = dev.fmt
    host = dev.like(dev.data.cpu())  # pageable
    del dev

    def todays_route():
        if f.depth == 8 or f.c_step != 2:
            raise SystemExit("driveyuvbench: the host route is written for planar 16-bit formats (got %s)" % ARGS.format)
        w16 = host.data.view(torch.int16)
        cw, ch = -(-W // f.hs), -(-H // f.vs)
        pl = lambda off, rows, cols, pitch: (torch.as_strided(w16, (T, rows, cols), (f.frame_stride // 2, pitch // 2, 1), off // 2)  # noqa: E731
                                             >> (f.shift + f.depth - 8)).to(torch.uint8)
        y, u, v = pl(f.y_off, H, W, f.y_pitch), pl(f.u_off, ch, cw, f.c_pitch), pl(f.v_off, ch, cw, f.c_pitch)
        u, v = (c[:, ::2 // f.vs, ::2 // f.hs].reshape(T, H // 4, W) for c in (u, v))
        return I.YuvFrames(torch.cat([y, u, v], dim=1), H, W, "i420", "bt709", "nearest")

    agent, portrait = make_agent()
    tc = {"PlanarYuv %s" % ARGS.format: [], "host pack + shift + drop rows, YuvFrames": []}
    for r in range(1 + C_REPS):
        for k, video in zip(tc, (lambda: host, todays_route)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.drive_video(portrait, video(), rects=RECT, out_dtype=torch.uint8)
            torch.cuda.synchronize()
            if r >= 1:
                tc[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in tc.items():
        print("(c) drive_video %-42s %8.1f ms per clip (spread %.1f), pageable host clip of %.0f MB, luma pitch %d"
              % (k, statistics.median(v), max(v) - min(v), host.data.numel() / 1e6, f.y_pitch))


def make_agent():
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.input_size = 512
    acfg = pkg.config.small_audio_config()
    acfg.dim_w = opt.dim_w
    Wt = pkg.weights
    parts = dict(enc=Wt.synth_encoder_state(512, seed=31), dec=Wt.synth_decoder_state(512, seed=31),
                 fmt=Wt.synth_fmt_state(pkg.config.FmtConfig.from_options(opt), seed=31), audio_encoder=(Wt.synth_audio_state(acfg, seed=31), acfg))
    return gen.InferenceAgent(opt, parts, "cuda:0"), torch.rand(1, 512, 512, 3, generator=torch.Generator().manual_seed(3))


if ARGS.format:
    if ARGS.format not in I.PLANAR_YUV_NAMES:
        sys.exit("driveyuvbench: --format must be one of %s" % sorted(I.PLANAR_YUV_NAMES))
    del rgb_d, rgb_h, yuv_h
    planar()
    sys.exit(0)

forms = {"rgb8": lambda: front("rgb8", rgb_d),
         "yuv nearest": lambda: front("yn", I.YuvFrames(yuv_d, H, W, SRC, "bt709", "nearest")),
         "yuv centre": lambda: front("yc", I.YuvFrames(yuv_d, H, W, SRC, "bt709", "centre"))}
ts = {k: [] for k in forms}
for r in range(WARM + REPS):
    for k, fn in forms.items():
        t = timed(fn)
        if r >= WARM:
            ts[k].append(t)
peak = N.probe_peaks("cuda:0")["hbm_read_GBps"]
print("%d frames of %d x %d in HBM, window %s -> 512 px, --src %s" % (T, W, H, RECT, SRC))
for k, v in ts.items():
    med, bpp = statistics.median(v), 3.0 if k == "rgb8" else 1.5
    gbps = T * RECT[2] * RECT[3] * bpp / med / 1e6
    print("(a) %-11s %8.3f ms per clip (spread %.3f) | (b) %.1f bytes per pixel: %.0f GB/s = %.3f of the streaming read (%.0f GB/s)"
          % (k, med, max(v) - min(v), bpp, gbps, gbps / peak, peak))
for key, chroma in (("yn", "nearest"), ("yc", "centre")):
    want = hm.resize_rgb8(hm.yuv420_to_rgb8(yuv_h[0], SRC, "bt709", chroma), RECT, 512, 512)
    print("frame 0, %s: equal to the definition: %s" % (chroma, torch.equal(out[key][0].cpu(), want)))

# (c) through the agent
del rgb_d, yuv_d
out.clear()
agent, portrait = make_agent()
yuv_clip = I.YuvFrames(yuv_h, H, W, SRC, "bt709", "nearest")
tc = {"rgb8": [], SRC: []}
for r in range(1 + C_REPS):
    for k, video in (("rgb8", rgb_h), (SRC, yuv_clip)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.drive_video(portrait, video, rects=RECT, out_dtype=torch.uint8)
        torch.cuda.synchronize()
        if r >= 1:
            tc[k].append((time.perf_counter() - t0) * 1e3)
for k, v in tc.items():
    print("(c) drive_video %-5s %8.1f ms per clip (spread %.1f), pageable host clip of %.0f MB"
          % (k, statistics.median(v), max(v) - min(v), (rgb_h if k == "rgb8" else yuv_h).numel() / 1e6))
