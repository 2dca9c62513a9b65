"""The decoder's launch geometry against references it does not share code with.

A. 128 / 256 px against the fp64 oracle (oracle/float_oracle.py, itself held to the reference by tests/test_oracle_golden.py and
   tests/test_oracle_vs_reference_live.py).  tests/test_dec_sizes_gpu.py compares two element types of the SAME kernels there,
   so an indexing mistake both share - the partial 28-px tiles of dec_zblur_kernel (256 = 9 x 28 + 4, 128 = 4 x 28 + 16), a
   border, a channel block - was invisible.  Inputs are that file's; limits are the project's own: fp32 verification mode
   frames max-abs <= 1e-4, raw <= 2e-4 (tests/test_dec_fp32_gpu.py); fp16 PSNR >= 52 dB, mean abs <= 0.5/255
   (LIMITS of tests/test_dec_gpu.py).  That the fp32 limits mean something on these inputs is pinned without a GPU by
   tests/test_oracle_golden.py::test_dec_geometry_inputs_are_well_conditioned (fp32 oracle within a quarter of them).
B. The 64-channel last level of a 256-px decoder: ToFlow in conv2's epilogue (dec_conv16_kernel<T, 4, 3, 3, 1> +
   dec_flowfrag_kernel + dec_flowlast_kernel) is taken by both element types (float_dec_create: `flow_epi &&
   conv_takes_flow_epi(..)`), so part A at 256 px holds it to the oracle; the other side of the switch (FLOAT_DEC_FLOW_EPI=0,
   dec_flow_kernel<.., Last = true> on the stored V, read once per process: child processes) is held here, and so is the
   same route taken because FLOAT_DEC_CONV_BN=32 splits conv2's 64 channels over two workgroups.
C. A frame's pixels do not depend on the batch it was decoded in, bit for bit, at the frame counts where the geometry changes:
   launch_conv `g.tpw = total >= 16384 ? 4 : (total >= 4096 ? 2 : 1)` (total = 16 x 16 tiles x frames), the frame blocks of the
   generic low-resolution kernel (`g.lnf = 8 - 2 * g.lth`: 16 frames per workgroup at 4 px, 4 at 8 px), launch_flow's band
   count (`bx = (2048 + n - 1) / n`, multiples of 8), the low batch (`lo_frames = min(128, 8 * max_frames)`).
D. Unit ops at the shapes the product runs (tests/util.py UNIT_CONV_CASES / UNIT_FLOW_CASES) against the fp64 oracle, limits
   `LIM` of tests/test_dec_units_gpu.py."""
import math
import os
import subprocess
import sys
from functools import lru_cache

import pytest
import torch

from oracle import float_oracle as O
from tests import util as U
from tests.test_dec_units_gpu import LIM
from tests.util import ROOT, golden, load_pkg, max_abs, rel_l2

pkg = load_pkg()
W, D = pkg.weights, pkg.decoder
pytestmark = pytest.mark.gpu
LIMITS = {"fp16": dict(psnr=52.0, mean=0.5 / 255)}  # tests/test_dec_gpu.py


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


@lru_cache(maxsize=None)
def oracle64(size):
    """(frames (7,S,S,3), un-clamped frame 0 (1,3,S,S)) of the fp64 oracle on the inputs of tests/test_dec_sizes_gpu.py."""
    sd, feats, s_r, r_d = U.dec_size_inputs(size)
    return (O.decode_frames(sd, s_r, r_d, feats, dtype=torch.float64),
            O.synthesis(sd, s_r + r_d[:, 0], feats, torch.float64))


def check_against_oracle(size, dtype, frames, raw, sat, tag):
    """The limits of part A for one decode (frames (7,S,S,3), raw (1,3,S,S) or None); returns the PSNR."""
    want, want_raw = oracle64(size)
    assert frames.shape == want.shape and sat == 0
    d = (frames.double() - want.double()).abs()
    m, mean, p = float(d.max()), float(d.mean()), psnr(frames, want)
    mr = max_abs(raw, want_raw) if raw is not None else float("nan")
    print("%s %d px %s vs fp64 oracle: frames max|d| %.2e mean %.2e psnr %.1f dB, raw max|d| %.2e" % (tag, size, dtype, m, mean, p, mr))
    if dtype == "fp32":
        if m > 1e-4:
            where(frames.permute(0, 3, 1, 2), want.permute(0, 3, 1, 2), "frames")
        assert m <= 1e-4 and mr <= 2e-4
    else:
        assert p >= LIMITS[dtype]["psnr"] and mean <= LIMITS[dtype]["mean"]
        assert frames.min() >= 0 and frames.max() <= 1
    return p


def where(got, want, tag):
    """Prints the worst element of (F,C,H,W) tensors: frame / channel / y / x and its place in the 16- and 28-px tiles."""
    d = (got.double().cpu() - want.double().cpu()).abs()
    i = int(d.flatten().argmax())
    f, c, y, x = [int(v) for v in torch.unravel_index(torch.tensor(i), d.shape)]
    print("  worst %s element: frame %d channel %d y %d x %d (in the 16-px tile %d,%d; in the 28-px tile %d,%d; tile %d,%d of 28): "
          "got %.6g want %.6g" % (tag, f, c, y, x, y % 16, x % 16, y % 28, x % 28, y // 28, x // 28,
                                  float(got[f, c, y, x]), float(want[f, c, y, x])))


# ---- A: 128 / 256 px against the fp64 oracle ----

@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("size", [128, 256])
def test_size_matches_fp64_oracle(size, dtype):
    """7 frames in batches of 3 + 4.  Measured on MI355X against the limits of the module docstring:
      128 px fp32 frames max 7.6e-6 (<= 1e-4), raw 7.5e-6 (<= 2e-4); fp16 79.2 dB (>= 52), mean 5.9e-5 (<= 2.0e-3), max 2.9e-3
      256 px fp32 frames max 2.6e-5,           raw 5.3e-5;           fp16 70.3 dB,         mean 1.5e-4,             max 2.9e-2
    (the fp32 oracle itself: 3.8e-6 / 7.6e-6 and 1.1e-5 / 1.9e-5).  At 256 px both modes run the last level's ToFlow in conv2's
    epilogue (part B): `rocprofv3 --kernel-trace --stats` of the fp32 case lists dec_conv16_kernel<FP32, 4, 3, 3, 0, 1>,
    dec_flowfrag_kernel<FP32> and dec_flowlast_kernel<FP32> three times each (batches of 3 + 4 frames and the raw frame), twelve
    dec_flow_kernel<FP32, 2, false> for the levels below and no dec_flow_kernel<.., true>: this is that route's first comparison
    with anything independent."""
    sd, feats, s_r, r_d = U.dec_size_inputs(size)
    dec = D.SynthesisHIP(sd, size, 512, "cuda:0", dtype, max_frames=4)
    dec.set_feats(feats)
    frames = dec.decode_latent_into_processed_images(s_r, r_d).float().cpu()
    raw = dec.synthesis_raw(s_r, r_d[:, :1]).cpu()
    check_against_oracle(size, dtype, frames, raw, dec.saturation(), "A")


# ---- B: the other side of the ToFlow switch at 256 px ----

CHILD = r'''
import sys, torch
sys.path.insert(0, %(root)r)
from tests import util as U
pkg = U.load_pkg()
size, dtype, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
sd, feats, s_r, r_d = U.dec_size_inputs(size)
dec = pkg.decoder.SynthesisHIP(sd, size, 512, "cuda:0", dtype, max_frames=4)
dec.set_feats(feats)
frames = dec.decode_latent_into_processed_images(s_r, r_d).float().cpu()
raw = dec.synthesis_raw(s_r, r_d[:, :1]).cpu()
torch.save({"frames": frames, "raw": raw, "sat": dec.saturation()}, out)
'''


def run_child(tmp_path, size, dtype, flow_epi, **switches):
    script = tmp_path / "child.py"
    script.write_text(CHILD % {"root": ROOT})
    out = tmp_path / ("dec_%d_%s_epi%s.pt" % (size, dtype, flow_epi))
    env = dict(os.environ, FLOAT_DEC_FLOW_EPI=flow_epi, **switches)
    subprocess.run([sys.executable, str(script), str(size), dtype, str(out)], check=True, env=env, cwd=ROOT, timeout=600)
    return torch.load(out)


def test_stored_v_flow_route_256_fp32_matches_oracle(tmp_path):
    """FLOAT_DEC_FLOW_EPI=0 in the fp32 mode: conv2 stores V and dec_flow_kernel<FP32, 4, true> reads it - the first
    independent check of that kernel at 64 channels.  Same limits as part A; measured frames max 2.6e-5, raw 5.3e-5
    (to the digits printed, the values of the epilogue route: the two differ by fp32 summation order only)."""
    r = run_child(tmp_path, 256, "fp32", "0")
    check_against_oracle(256, "fp32", r["frames"], r["raw"], r["sat"], "B stored-V")


def test_flow_routes_agree_256_fp16(tmp_path):
    """Both routes in fp16, each in its own process.  They sum the same exact products in fp32 in different orders, so they must
    agree with each other at least 20 dB better than either agrees with the fp64 oracle (the 512-px pair of
    tests/test_variants_gpu.py has about 25 dB of headroom over its 56 dB of parity; its 80 dB was measured for 32 channels).
    Measured: the routes agree to 143.5 dB (max 9.8e-6, mean 1.0e-8, not bitwise); each is 70.3 dB from the oracle: 73 dB of
    headroom, so at 64 channels and 256 px no 16-bit rounding flipped between the routes on these frames."""
    epi = run_child(tmp_path, 256, "fp16", "1")
    old = run_child(tmp_path, 256, "fp16", "0")
    p_epi = check_against_oracle(256, "fp16", epi["frames"], epi["raw"], epi["sat"], "B epilogue")
    p_old = check_against_oracle(256, "fp16", old["frames"], old["raw"], old["sat"], "B stored-V")
    d = (epi["frames"] - old["frames"]).abs()
    p = psnr(epi["frames"], old["frames"])
    print("B 256 px fp16: ToFlow in the epilogue vs flow kernel %.1f dB (max %.2e, mean %.2e); oracle %.1f / %.1f dB" % (
        p, float(d.max()), float(d.mean()), p_epi, p_old))
    assert p >= max(p_epi, p_old) + 20.0


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_conv_bn32_takes_the_flow_kernel_256(tmp_path, dtype):
    """FLOAT_DEC_CONV_BN=32 (read once per handle: a child process) on the 64-channel last level: conv2 runs in two 32-channel
    blocks, so ToFlow cannot ride in its epilogue (it needs the whole channel range in one workgroup) and the level goes through
    dec_flow_kernel on the stored V.  One function (conv_bn, dec_launch.hpp) now answers both launch_conv and run_level's `epi`;
    before, `epi` did not know the block size and the decode failed with "ToFlow epilogue needs the layer's 64 output channels
    in one block of 32".  Limits: part A's at 256 px."""
    r = run_child(tmp_path, 256, dtype, "1", FLOAT_DEC_CONV_BN="32")
    check_against_oracle(256, dtype, r["frames"], r["raw"], r["sat"], "B 32-channel blocks")


# ---- C: frame-count geometry, bit for bit ----

def clip(size, seed, n):
    gen = torch.Generator().manual_seed(1)
    s_r, r_d = torch.randn(1, 512, generator=gen), torch.randn(1, n, 512, generator=gen) * 0.5
    return W.synth_decoder_state(size, seed=seed), W.synth_feats(size, seed=seed), s_r, r_d


def decode(sd, feats, size, dtype, max_frames, s_r, r_d):
    dec = D.SynthesisHIP(sd, size, 512, "cuda:0", dtype, max_frames=max_frames)
    dec.set_feats(feats)
    out = dec.decode_latent_into_processed_images(s_r, r_d)
    assert dec.saturation() == 0
    dec.close()
    return out


def assert_same_bits(a, b, tag):
    if torch.equal(a, b):
        print("C %s: bitwise equal (%d frames)" % (tag, a.shape[0]))
        return
    ne = (a != b).flatten(1).sum(1).cpu()
    first = int(ne.nonzero()[0])
    where(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), tag)
    raise AssertionError("%s: %d of %d frames differ, the first is frame %d (%d elements), max |d| %.3e" % (
        tag, int((ne > 0).sum()), a.shape[0], first, int(ne[first]), float((a - b).abs().max())))


def test_frames_independent_of_batching_512_fp16():
    """33 frames at 512 px, max_frames 33 / 16 / 3.  16 x 16 tiles x frames per high batch:
      33 frames: 33 792 at 512 px (tpw 4), 8 448 at 256 px (tpw 2), 2 112 / 528 below (tpw 1); the low batch is 33 frames: three
                 frame blocks in the 4-px conv, nine at 8 px; flow bands sized for n = 33;
      16 frames: 16 384 at 512 px - tpw 4 exactly at the threshold - and 4 096 at 256 px (tpw 2 at its threshold), high batches
                 1 + 16 + 16 (the short piece first) under one low batch of 33;
      3 frames:  tpw 1 everywhere, low batches 9 + 24.
    Also through decode_into_host into pinned memory with the 33-frame batch: once alone, and once as the first of two batches
    (66 frames), where the ride-along copy workgroups of batch 1 are appended to every grid of batch 2 (the last batch of a call
    has no successor to carry its copy).  Measured: every comparison bitwise equal."""
    sd, feats, s_r, r_d = clip(512, 9, 33)
    f33 = decode(sd, feats, 512, "fp16", 33, s_r, r_d)
    assert f33.shape == (33, 512, 512, 3) and bool(torch.isfinite(f33).all())
    assert_same_bits(f33, decode(sd, feats, 512, "fp16", 3, s_r, r_d), "512 px fp16 max_frames 33 vs 3")
    assert_same_bits(f33, decode(sd, feats, 512, "fp16", 16, s_r, r_d), "512 px fp16 max_frames 33 vs 16")
    dec = D.SynthesisHIP(sd, 512, 512, "cuda:0", "fp16", max_frames=33)
    dec.set_feats(feats)
    host = torch.full((33, 512, 512, 3), -1.0).pin_memory()
    staging = dec.decode_into_host(s_r, r_d, host)
    torch.cuda.current_stream().synchronize()
    assert_same_bits(host, f33.cpu(), "512 px fp16 decode_into_host (pinned) vs decode")
    assert_same_bits(staging, f33, "512 px fp16 decode_into_host staging vs decode")
    # twice 33 frames with max_frames 33: the second batch's launches carry the first batch's copy
    r2 = torch.cat([r_d, r_d.flip(1)], dim=1)
    host2 = torch.full((66, 512, 512, 3), -1.0).pin_memory()
    dec.decode_into_host(s_r, r2, host2)
    torch.cuda.current_stream().synchronize()
    assert_same_bits(host2[:33], f33.cpu(), "512 px fp16 decode_into_host, batch 1 of 2")
    assert_same_bits(host2[33:], f33.cpu().flip(0), "512 px fp16 decode_into_host, batch 2 of 2 (carries the copy of batch 1)")
    dec.close()


def test_frames_independent_of_batching_256_fp16():
    """70 frames at 256 px: max_frames 70 (17 920 tiles x frames at the top level: tpw 4; 4 480 at 128 px: tpw 2), 16 (4 096: tpw 2
    at its threshold; batches 6 + 16 x 4) and 5 (1 280: tpw 1; low batches 30 + 40).  Here the 64-channel ToFlow epilogue is the
    kernel whose tiles per workgroup change.  Measured: bitwise equal."""
    sd, feats, s_r, r_d = clip(256, 9, 70)
    f70 = decode(sd, feats, 256, "fp16", 70, s_r, r_d)
    assert f70.shape == (70, 256, 256, 3) and bool(torch.isfinite(f70).all())
    assert_same_bits(f70, decode(sd, feats, 256, "fp16", 16, s_r, r_d), "256 px fp16 max_frames 70 vs 16")
    assert_same_bits(f70, decode(sd, feats, 256, "fp16", 5, s_r, r_d), "256 px fp16 max_frames 70 vs 5")


def test_frames_independent_of_batching_512_fp32():
    """The fp32 verification mode with 17 frames at 512 px, max_frames 17 (17 408 tiles x frames: tpw 4 and a second frame block of
    the 4-px conv through the 4-byte kernels) against max_frames 2 (tpw 1).  The clip starts with the two latents of
    tests/golden/dec_512.npz: frames 0-1 must equal, bit for bit, the max_frames = 2 decode of those two alone, which
    tests/test_dec_fp32_gpu.py::test_dec_512_fp32_golden holds to the reference at 1e-4 - asserted here on the 17-frame run too.
    Measured: bitwise equal; frames 0-1 against the golden max 9.8e-5."""
    g = golden("dec_512")
    sd, feats = W.synth_decoder_state(512, seed=g["seed"]), W.synth_feats(512, seed=g["seed"])
    gen = torch.Generator().manual_seed(1)
    r_d = torch.cat([g["r_d"], torch.randn(1, 15, 512, generator=gen) * 0.5], dim=1)
    f17 = decode(sd, feats, 512, "fp32", 17, g["s_r"], r_d)
    assert f17.shape == (17, 512, 512, 3)
    assert_same_bits(f17, decode(sd, feats, 512, "fp32", 2, g["s_r"], r_d), "512 px fp32 max_frames 17 vs 2")
    assert_same_bits(f17[:2], decode(sd, feats, 512, "fp32", 2, g["s_r"], g["r_d"]), "512 px fp32 frames 0-1 vs the golden's decode")
    two = f17[:2].cpu()
    m = max(max_abs(two[:, ::7, ::5], g["lattice"]), max_abs(two[:, 250:258], g["band"]))
    print("C 512 px fp32 frames 0-1 of the 17-frame batch vs the reference golden: max|d| %.2e" % m)
    assert m <= 1e-4


# ---- D: unit ops at product shapes ----

@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("case", range(len(U.UNIT_CONV_CASES)), ids=["%dto%d_r%d_up%d" % c for c in U.UNIT_CONV_CASES])
def test_styled_conv_product_shapes(case, dtype):
    """StyledConv through the production kernels against O.styled_conv in fp64, two frames.  Measured max |d| / rel-L2
    (limits fp32 2e-5 / 2e-6, fp16 3e-2 / 2e-3; the fp32 oracle's own distance in brackets):
      32 -> 32 at 64 px        fp32 4.8e-6 / 4.5e-7 (2.6e-6 / 2.4e-7)   fp16 3.0e-3 / 3.6e-4     dec_conv16_kernel NT = 2
      128 -> 128 at 32 px      fp32 9.5e-6 / 6.8e-7 (2.5e-6 / 2.5e-7)   fp16 2.8e-3 / 3.6e-4     two 64-channel blocks
      256 -> 128, 64 -> 128 px fp32 3.4e-6 / 4.3e-7 (3.0e-6 / 3.3e-7)   fp16 2.8e-3 / 3.4e-4     dec_zblur_kernel, partial tile of 16
      128 -> 64, 128 -> 256 px fp32 3.5e-6 / 3.6e-7 (2.5e-6 / 2.5e-7)   fp16 3.0e-3 / 3.4e-4     dec_zblur_kernel, partial tile of 4
      512 -> 512, 8 -> 16 px   fp32 5.2e-6 / 5.6e-7 (3.6e-6 / 4.4e-7)   fp16 2.5e-3 / 3.4e-4     dec_zconv4_kernel + dec_blur_kernel
    The plain 3x3 convs sit at 2-4 x the fp32 oracle: v_mfma_f32_16x16x4_f32 runs one accumulation chain over K = 9 * cin in
    steps of 4 (1 152 terms at 128 channels; tests/test_dec_units_gpu.py's 64-channel case: 6.2e-6 / 5.6e-7)."""
    cin, cout, R, up = U.UNIT_CONV_CASES[case]
    sd, x = U.unit_conv_case(case)
    out, sat = D.debug_styled_conv(sd, x, U.unit_style(), upsample=bool(up), dtype=dtype)
    want = U.unit_conv_oracle(case)
    m, r = max_abs(out.cpu(), want), rel_l2(out.cpu(), want)
    print("D %s styled_conv %d -> %d at %d px up %d: max|d| %.2e rel %.2e" % (dtype, cin, cout, R, up, m, r))
    assert out.shape == want.shape and sat == 0
    if m > LIM[dtype]["max"] or r > LIM[dtype]["rel"]:
        where(out, want, "styled_conv")
    assert m <= LIM[dtype]["max"] and r <= LIM[dtype]["rel"]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("case", range(len(U.UNIT_FLOW_CASES)), ids=["c%d_r%d_prev%d" % c for c in U.UNIT_FLOW_CASES])
def test_flow_level_product_shapes(case, dtype):
    """ToFlow + ToRGB of one level through dec_flow_kernel against O.to_flow / O.to_rgb in fp64, two frames; limits as in
    tests/test_dec_units_gpu.py::test_flow_level (x5 for `blend` / `rgb`, which sit behind the warp).  Measured max |d| of
    out / blend / rgb:
      64 ch at 64 px (PIX = 4, 8 lanes per pixel, 32 bands)   fp32 5.6e-7 / 1.5e-5 / 9.4e-6    fp16 4.4e-4 / 1.1e-2 / 5.6e-3
      256 ch at 64 px                                         fp32 4.9e-7 / 1.6e-5 / 2.1e-5    fp16 3.6e-4 / 1.0e-2 / 1.3e-2
      512 ch at 8 px                                          fp32 4.1e-7 / 2.7e-6 / 6.5e-7    fp16 3.0e-4 / 1.6e-3 / 5.2e-4
      64 ch at 128 px, no pyramid below                       fp32 2.3e-7 / 1.8e-5 / 2.0e-5    fp16 2.0e-4 / 9.3e-3 / 9.8e-3
    (limits: out 2e-5, blend / rgb 1e-4 in fp32; 3e-2 and 0.15 in fp16; rel-L2 at most 1.2e-6 / 6.0e-4)."""
    C, R, prev = U.UNIT_FLOW_CASES[case]
    sd, x, feat, pflow, prgb = U.unit_flow_case(case)
    got = dict(zip(("out", "blend", "rgb"), D.debug_flow_level(sd, x, feat, U.unit_style(), pflow, prgb, dtype=dtype)))
    want = U.unit_flow_oracle(case)
    bad = []
    for what in ("out", "blend", "rgb"):
        m, r = max_abs(got[what].cpu(), want[what]), rel_l2(got[what].cpu(), want[what])
        k = 5 if what != "out" else 1
        print("D %s flow level %d ch at %d px prev %d %-5s max|d| %.2e rel %.2e" % (dtype, C, R, prev, what, m, r))
        assert got[what].shape == want[what].shape
        if m > LIM[dtype]["max"] * k or r > LIM[dtype]["rel"] * k:
            where(got[what], want[what], what)
            bad.append(what)
    assert not bad, bad
