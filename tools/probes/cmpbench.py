"""Achieved read bandwidth of float_cmp_segments beside the device's own streaming-read peak (float_probe_peaks): the figure
quoted in DESIGN.md section 2.  Default: 250 frames of 512 px (2 x 786 MB read per call), device events around each call.
  python tools/probes/cmpbench.py [--frames 250] [--size 512] [--reps 10]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.util import load_pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    N = load_pkg().native
    seg = a.size * a.size * 3
    g = torch.Generator("cuda").manual_seed(0)
    x = torch.rand(a.frames * seg, device="cuda", generator=g)
    y = x + torch.randn(a.frames * seg, device="cuda", generator=g) * 0.01
    for _ in range(2):
        N.cmp_segments(x, y, seg)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        N.cmp_segments(x, y, seg)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    gb = 2 * x.numel() * 4 / 1e9
    peaks = N.probe_peaks()
    print(json.dumps(dict(frames=a.frames, size=a.size, read_GB=round(gb, 3), ms_min=round(min(ms), 4), ms_median=round(sorted(ms)[len(ms) // 2], 4),
                          GBps_best=round(gb / (min(ms) * 1e-3), 1), GBps_median=round(gb / (sorted(ms)[len(ms) // 2] * 1e-3), 1),
                          probe_hbm_read_GBps=peaks["hbm_read_GBps"])))


if __name__ == "__main__":
    main()
