"""What pasting the generated frames back into the portrait costs, on the 512-px synthetic model (bench.py config 1: a 10-s clip,
51 grid points, decode batches of 32, seeded weights of the checkpoint's shapes) with a 1024 x 1024 and a 1920 x 1088 portrait,
face_align on and a stub detector whose box gives a crop of about 0.6 of the portrait's height.  Per portrait four forms take
turns in one process:
  u8      host_inputs + InferenceAgent.infer_device(out_dtype=torch.uint8): the crop clip, the yardstick of the same process;
  pasted  InferenceAgent.infer_pasted;
  i420    InferenceAgent.infer_pasted(out_format="i420"): paste and colour conversion in one kernel, 1.5 bytes per pixel;
  jpeg    InferenceAgent.infer_pasted_jpeg(quality=QUALITY).
Then the pasted JPEG clip at 1920 x 1080 under pad="edge" (1080 lines are 67.5 MCUs: float_jpg_encode_padded, the first 1080 lines
of the 1920 x 1088 portrait) takes turns with the one at 1920 x 1088 (float_jpg_encode), REPS times after WARMUP: key
"jpeg_1080_edge_vs_1088"; the 1088 clip of that loop is the yardstick, the first file of the 1080 clip is compared with the
definition's.
Each call is timed on the host clock between device synchronisations, REPS (default 10) repetitions per form after WARMUP
(default 2), taking turns.  The paste launch alone (image.paste_frames_device on 50 crops in HBM, the product's group) is timed by
device events, LAUNCH_REPS (default 30) times after 3, the RGB and the I420 launch taking turns, and held to the bytes it moves -
50 H W 3 (I420: 50 H W 3 / 2) written, 50 H W 3 of the source and 50 x 512 x 512 x 3 of the frames read - over the copy bandwidth
float_probe_peaks measures in this process (bytes read + bytes written per second).  Prints one JSON line: median, min, max and
spread (max - min) per form, ms; per launch its median, its GB/s and its fraction of the copy peak.  Run from the repository root.
--matrix M (2 | 4 | 6 or a name host_models.yuv_matrix_id knows): one more form, i420_m = infer_pasted(out_format="i420", matrix=M),
takes turns with the others, and one more launch, i420_m, with the paste launches; each reports `minus_id0_ms` against i420 and
`ok_vs_id0` = its median does not exceed i420's by more than i420's own spread.
--resample NAME ("bicubic" | "lanczos"): three more forms take turns with the others - pasted_r, i420_r, jpeg_r: the pasted clip
in RGB, I420 and JPEG form with resample=NAME, each reporting `minus_default_ms` against its default form of the same process - and
two more launches with the paste launches: `resample`, the two kernels of float_img_resample alone on the 50 crops (the window of
the box that lies in the image; held to the bytes they move - the crops read, the 8-bit intermediate written and read, the window
written - over the same copy peak), and `rgb_r`, the paste with resample=NAME whole (three kernels), compared with the definition.
The 1080-line JPEG loop is left out of such a run.
Environment: REPS, WARMUP, LAUNCH_REPS, QUALITY."""
import argparse
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
hm = pkg.host_models
ap = argparse.ArgumentParser()
ap.add_argument("--matrix", default=None, help="a second colour matrix to interleave with id 0 (2, 4, 6 or a name)")
ap.add_argument("--resample", default=None, help="a resampling filter of the paste to interleave with the default route (bicubic, lanczos)")
MATRIX, RESAMPLE = ap.parse_args().matrix, ap.parse_args().resample
if RESAMPLE is not None:
    hm.resample_filter_id("pastebench", RESAMPLE)
MATRIX = None if MATRIX is None else hm.yuv_matrix_id(int(MATRIX) if MATRIX.lstrip("-").isdigit() else MATRIX)
REPS, WARMUP, QUALITY = int(os.environ.get("REPS", "10")), int(os.environ.get("WARMUP", "2")), int(os.environ.get("QUALITY", "90"))
LAUNCH_REPS = int(os.environ.get("LAUNCH_REPS", "30"))
SIZE, SECONDS, NFE, MAX_FRAMES = 512, 10.0, 51, 32
dev = "cuda:0"


class _Detector:
    """a box in the middle of the 360-px view, half side 0.19 of its height: at margin 1.6 a crop of 0.6 of the portrait's height"""
    def detect_from_image(self, arr):
        h, w = arr.shape[0], arr.shape[1]
        r = 0.19 * h
        return [(w / 2 - r, h / 2 - r, w / 2 + r, h / 2 + r, 0.99)]


class _FA:
    face_detector = _Detector()


hm._FA = _FA()

cfg = pkg.config.FmtConfig()
gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
opt.nfe, opt.input_size, opt.fps, opt.rank = NFE, SIZE, 25.0, dev
acfg = pkg.config.AudioConfig()
parts = dict(enc=pkg.weights.synth_encoder_state(SIZE, seed=1), dec=pkg.weights.synth_decoder_state(SIZE, seed=1),
             fmt=pkg.weights.synth_fmt_state(cfg, seed=1), audio_encoder=(pkg.weights.synth_audio_state(acfg, seed=1), acfg))
agent = gen.InferenceAgent(opt, parts, dev, max_frames=MAX_FRAMES, use_graph=2)
audio = {"waveform": pkg.weights.synth_waveform(SECONDS, seed=1).reshape(1, 1, -1).cpu(), "sample_rate": 16000}
FORMS = ("u8", "pasted", "i420", "jpeg") + (("i420_m",) if MATRIX is not None else ()) + \
    (("pasted_r", "i420_r", "jpeg_r") if RESAMPLE is not None else ())
KW = dict(emo="neutral", seed=15)
last = {}


def run(form, img, pad=None):
    if form == "u8":
        s, a = agent.host_inputs(img, audio, no_crop=False)
        last[form] = agent.infer_device(s, a, 2.0, 1.0, 1.0, out_dtype=torch.uint8, **KW)
    elif form == "pasted":
        last[form] = agent.infer_pasted(img, audio, 2.0, 1.0, 1.0, no_crop=False, **KW)
    elif form == "i420":
        last[form] = agent.infer_pasted(img, audio, 2.0, 1.0, 1.0, no_crop=False, out_format="i420", **KW)
    elif form == "i420_m":
        last[form] = agent.infer_pasted(img, audio, 2.0, 1.0, 1.0, no_crop=False, out_format="i420", matrix=MATRIX, **KW)
    elif form == "pasted_r":
        last[form] = agent.infer_pasted(img, audio, 2.0, 1.0, 1.0, no_crop=False, resample=RESAMPLE, **KW)
    elif form == "i420_r":
        last[form] = agent.infer_pasted(img, audio, 2.0, 1.0, 1.0, no_crop=False, out_format="i420", resample=RESAMPLE, **KW)
    elif form == "jpeg_r":
        last[form] = agent.infer_pasted_jpeg(img, audio, 2.0, 1.0, 1.0, no_crop=False, quality=QUALITY, pad=pad, resample=RESAMPLE, **KW)
    else:
        last[form] = agent.infer_pasted_jpeg(img, audio, 2.0, 1.0, 1.0, no_crop=False, quality=QUALITY, pad=pad, **KW)


def wall_ms(form, img, pad=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(form, img, pad)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    agent.G.release_host_inflight()
    return ms


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), spread=round(max(v) - min(v), 3))


def vs_id0(out):
    out["i420_m"]["minus_id0_ms"] = round(out["i420_m"]["median"] - out["i420"]["median"], 3)
    out["i420_m"]["ok_vs_id0"] = out["i420_m"]["median"] <= out["i420"]["median"] + out["i420"]["spread"]


def launch_alone(place, peaks):
    """{"rgb": ..., "i420": ...}: float_img_paste and float_img_paste_i420 on the same 50 crops, taking turns"""
    n, (H, W) = 50, place.size
    crops = torch.randint(0, 256, (n, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    feather = hm.default_feather(place.rect)
    outs = {"rgb": torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev), "i420": torch.empty(n, 3 * H // 2, W, dtype=torch.uint8, device=dev)}
    if MATRIX is not None:
        outs["i420_m"] = torch.empty(n, 3 * H // 2, W, dtype=torch.uint8, device=dev)
    if RESAMPLE is not None:
        xa, ya, xb, yb = pkg.image.paste_window(H, W, place.rect)
        win = (xa - place.rect[0], ya - place.rect[1], xb - xa, yb - ya)
        scratch = pkg.image.paste_scratch((H, W), (SIZE, SIZE), place.rect, n, RESAMPLE, torch.device(dev))
        outs["rgb_r"] = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        outs["resample"] = scratch.face
    ms = {fmt: [] for fmt in outs}
    for i in range(3 + LAUNCH_REPS):
        for fmt, out in outs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if fmt == "resample":
                pkg.image.resample_frames_device(crops, place.rect[3], place.rect[2], RESAMPLE, win, out=out, work=scratch.work)
            elif fmt == "rgb_r":
                pkg.image.paste_frames_device(place.src8, crops, place.rect, feather, out=out, resample=RESAMPLE, scratch=scratch)
            else:
                kw = dict(out_format="i420", matrix=MATRIX) if fmt == "i420_m" else dict(out_format=fmt)
                pkg.image.paste_frames_device(place.src8, crops, place.rect, feather, out=out, **kw)
            e1.record()
            e1.synchronize()
            if i >= 3:
                ms[fmt].append(e0.elapsed_time(e1))
    want = hm.paste_rgb8(place.src8.cpu(), crops[:1].cpu(), place.rect, feather)
    res = {}
    for fmt, out in outs.items():
        if fmt == "resample":  # the rows of the crops the window references, the intermediate written and read, the window written
            ymin, yn, _ = hm.resample_coeffs(SIZE, place.rect[3], RESAMPLE, win[1], win[3])
            rows = int((ymin + yn).max()) - int(ymin.min())
            mid = rows * 3 * ((win[2] + 3) // 4 * 4)
            moved = n * (rows * SIZE * 3 + 2 * mid + win[2] * win[3] * 3)
            r = stats(ms[fmt])
            r.update(frames=n, window=list(win), bytes_moved=moved, GBps=round(moved / 1e9 / (r["median"] * 1e-3), 1),
                     fraction_of_copy_peak=round(moved / 1e9 / (r["median"] * 1e-3) / peaks["hbm_copy_GBps"], 3),
                     equals_definition=bool(torch.equal(out[:1].cpu(), hm.resample_rgb8(crops[:1].cpu(), place.rect[3], place.rect[2], RESAMPLE, win))))
            res[fmt] = r
            continue
        if fmt == "rgb_r":
            r = stats(ms[fmt])
            r.update(frames=n, minus_rgb_ms=round(r["median"] - statistics.median(ms["rgb"]), 3),
                     equals_definition=bool(torch.equal(out[:1].cpu(), hm.paste_rgb8(place.src8.cpu(), crops[:1].cpu(), place.rect, feather,
                                                                                    resample=RESAMPLE))))
            res[fmt] = r
            continue
        moved = n * out[0].numel() + n * H * W * 3 + n * SIZE * SIZE * 3
        r = stats(ms[fmt])
        r.update(frames=n, bytes_moved=moved, GBps=round(moved / 1e9 / (r["median"] * 1e-3), 1),
                 fraction_of_copy_peak=round(moved / 1e9 / (r["median"] * 1e-3) / peaks["hbm_copy_GBps"], 3),
                 equals_definition=bool(torch.equal(out[:1].cpu(), want if fmt == "rgb" else
                                                    hm.rgb8_to_i420(want, MATRIX if fmt == "i420_m" else None))))
        res[fmt] = r
    res["i420_minus_rgb_ms"] = round(res["i420"]["median"] - res["rgb"]["median"], 3)
    if MATRIX is not None:
        vs_id0(res)
    return res


peaks = pkg.native.probe_peaks(dev)
res = dict(probe="pastebench", matrix=MATRIX, resample=RESAMPLE, size=SIZE, frames=250, nfe=NFE, max_frames=MAX_FRAMES, reps=REPS, warmup=WARMUP, quality=QUALITY, peaks=peaks)
for H, W in ((1024, 1024), (1088, 1920)):
    img = torch.from_numpy(np.random.RandomState(H).rand(1, H, W, 3).astype("float32"))
    for _ in range(WARMUP):
        for form in FORMS:
            wall_ms(form, img)
    ms = {form: [] for form in FORMS}
    for _ in range(REPS):
        for form in FORMS:  # taking turns: drift of the box lands on all three
            ms[form].append(wall_ms(form, img))
    out = {form: stats(v) for form, v in ms.items()}
    out["pasted"]["minus_u8_ms"] = round(out["pasted"]["median"] - out["u8"]["median"], 3)
    out["i420"]["minus_u8_ms"] = round(out["i420"]["median"] - out["u8"]["median"], 3)
    out["i420"]["minus_pasted_ms"] = round(out["i420"]["median"] - out["pasted"]["median"], 3)
    out["jpeg"]["minus_u8_ms"] = round(out["jpeg"]["median"] - out["u8"]["median"], 3)
    if MATRIX is not None:
        vs_id0(out)
    if RESAMPLE is not None:
        for form, base in (("pasted_r", "pasted"), ("i420_r", "i420"), ("jpeg_r", "jpeg")):
            out[form]["minus_default_ms"] = round(out[form]["median"] - out[base]["median"], 3)
            out[form]["fraction_of_default"] = round(out[form]["median"] / out[base]["median"] - 1.0, 4)
    _, _, place = agent.host_inputs_placed(img, audio, no_crop=False)
    out["rect"] = list(place.rect)
    out["bytes_to_host"] = dict(u8=last["u8"].numel(), pasted=last["pasted"].numel(), i420=last["i420"].numel(), jpeg=last["jpeg"].nbytes)
    out["paste_launch_50_frames"] = launch_alone(place, peaks)
    res["%dx%d" % (W, H)] = out
if RESAMPLE is not None:
    print(json.dumps(res))
    sys.exit(0)
img1088 = torch.from_numpy(np.random.RandomState(1088).rand(1, 1088, 1920, 3).astype("float32"))
turns = (("1920x1088", img1088, None), ("1920x1080_edge", img1088[:, :1080].contiguous(), "edge"))
ms = {name: [] for name, _, _ in turns}
for i in range(WARMUP + REPS):
    for name, img, pad in turns:
        t = wall_ms("jpeg", img, pad)
        if i >= WARMUP:
            ms[name].append(t)
    if i == 0:  # `last` holds the 1080 clip: its first file against the definition of the first pasted frame
        edge_file, edge_bytes = bytes(last["jpeg"][0]), last["jpeg"].nbytes
        first = agent.infer_pasted(turns[1][1], audio, 2.0, 1.0, 1.0, no_crop=False, **KW)[:1].clone()
        agent.G.release_host_inflight()
        edge_ok = edge_file == hm.jpeg_encode_rgb8(first, QUALITY, None, pad="edge")[0]
out = {name: stats(v) for name, v in ms.items()}
out["edge_minus_1088_ms"] = round(out["1920x1080_edge"]["median"] - out["1920x1088"]["median"], 3)
out["bytes_to_host_1080_edge"] = edge_bytes
out["first_file_equals_definition"] = bool(edge_ok)
res["jpeg_1080_edge_vs_1088"] = out
print(json.dumps(res))
