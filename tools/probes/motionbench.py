"""Motion-pass timing probe: lambda rows of a 10-s driving clip (250 frames of 512 px, fp16, seeded weights, frames already in
HBM), two forms interleaved in one process, wall-clock ms per clip (the host waits at the end of every repetition), medians
of 20 after warm-up and the spread max - min:
  (loop)   250 float_enc_forward calls with feats = NULL on the frames as fp32 NCHW images: the only way the once-per-clip
           operator produces the same rows;
  (motion) float_enc_motion on the 8-bit frames with block = 1, 4, 8, 16.
Also: ms per frame, the achieved FLOP/s (operations counted from the layer shapes below) against the box's MFMA peak
(float_probe_peaks), the scratch per block, and the largest rel-L2 between the two forms' rows.
MOTION_FRAMES / MOTION_SIZE / MOTION_REPS shrink the run for a rehearsal."""
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from tests.util import load_pkg, rel_l2  # noqa: E402

pkg = load_pkg()
N = pkg.native
T, S = int(os.environ.get("MOTION_FRAMES", 250)), int(os.environ.get("MOTION_SIZE", 512))
REPS, WARM = int(os.environ.get("MOTION_REPS", 20)), 3
esd = pkg.weights.synth_encoder_state(S, seed=1)
enc = pkg.encoder.EncoderHIP(esd, S, 512, 20, "cuda:0", "fp16")
frames = torch.randint(0, 256, (T, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
imgs = (frames.permute(0, 3, 1, 2).float() / 127.5 - 1).contiguous()
lam_loop, lam_m = torch.empty(T, 20, device="cuda"), None
L, st = N.lib(), N.stream_ptr("cuda:0")


def flops():
    ch = pkg.weights.ENC_CHANNELS
    n, R = 2.0 * S * S * 3 * ch[S], S
    while R > 4:
        c, co = ch[R], ch[R // 2]
        n += 2.0 * R * R * c * c * 9 + 2.0 * (R // 2) ** 2 * c * co * 10
        R //= 2
    return n + 2.0 * 16 * ch[4] * 512 + 2.0 * (4 * 512 * 512 + 512 * 20)


def loop():
    for t in range(T):
        N.check(L.float_enc_forward(enc._h, N.dev_ptr(imgs[t]), None, C.c_void_p(lam_loop[t].data_ptr()), None, None, 0, st))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


encs = {}  # one handle per block size: changing a handle's block replaces its scratch (a device synchronise and six allocations)
for blk in (1, 4, 8, 16):
    encs[blk] = enc if blk == 8 else pkg.encoder.EncoderHIP(esd, S, 512, 20, "cuda:0", "fp16")
    encs[blk].encode_motion(frames[:1], block=blk)


def motion(block):
    global lam_m
    lam_m = encs[block].encode_motion(frames)


forms = {"loop": loop}
ts = {"loop": []}
for blk in (1, 4, 8, 16):
    forms["block %d" % blk] = (lambda b=blk: motion(b))
    ts["block %d" % blk] = []
for r in range(WARM + REPS):
    for k, fn in forms.items():
        t = timed(fn)
        if r >= WARM:
            ts[k].append(t)
peak = N.probe_peaks("cuda:0")["mfma_f16_16x16x32_TFLOPs"]
gf = flops()
print("%d frames of %d px, fp16, %.1f GFLOP per frame; MFMA peak of this box %.0f TFLOP/s" % (T, S, gf / 1e9, peak))
for k, v in ts.items():
    med, spread = statistics.median(v), max(v) - min(v)
    print("%-9s %9.2f ms per clip (spread %.2f) | %.3f ms per frame | %.1f TFLOP/s = %.3f of peak" % (
        k, med, spread, med / T, gf * T / med / 1e9, gf * T / med / 1e9 / peak))
print("largest rel-L2 of a row, motion (block 16) against the loop: %.2e; saturation counter %d" % (
    max(rel_l2(lam_m[t].cpu(), lam_loop[t].cpu()) for t in range(T)), sum(e.saturation() for e in encs.values())))
