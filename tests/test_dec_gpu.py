"""GPU parity of the decoder operator against the CPU oracle / goldens, through the C ABI.
16-bit activations with fp32 accumulation.  Stated tolerances (calibrated on MI355X):
frames in [0,1]: PSNR >= 52 dB and mean |d| <= 0.5/255 with fp16 operands (the only operand type of the decoder: bf16 sat at
40.7 dB against the 40 dB of SURVEY 8d and was dropped)."""
import math

import pytest
import torch

from oracle import float_oracle as O
from tests.util import golden, load_pkg

pkg = load_pkg()
W = pkg.weights
pytestmark = pytest.mark.gpu


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


LIMITS = {"fp16": dict(psnr=52.0, mean=0.5 / 255)}


@pytest.mark.parametrize("dtype", ["fp16"])
def test_dec_64_golden(dtype):
    g = golden("dec_64")
    sd = W.synth_decoder_state(64, seed=g["seed"])
    feats = W.synth_feats(64, seed=g["seed"])
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", dtype=dtype, max_frames=2)  # 3 frames -> 2 batches
    frames = dec.decode_latent_into_processed_images(g["s_r"], g["r_d"], feats).cpu()
    assert frames.shape == g["frames"].shape
    p, m = psnr(frames, g["frames"]), float((frames - g["frames"]).abs().mean())
    raw = dec.synthesis_raw(g["s_r"], g["r_d"][:, :1]).cpu()
    print(dtype, "64px: PSNR %.1f dB mean|d| %.2e max|d| %.2e raw max|d| %.2e" % (
        p, m, float((frames - g["frames"]).abs().max()), float((raw - g["raw0"]).abs().max())))
    assert p >= LIMITS[dtype]["psnr"] and m <= LIMITS[dtype]["mean"]
    assert frames.min() >= 0 and frames.max() <= 1
    assert float((frames - g["frames"]).abs().max()) <= 2.0 / 255  # 64 px: the per-pixel bound of SURVEY 8d holds outright
    assert dec.saturation() == 0  # nothing had to be clamped at fp16's range


@pytest.mark.parametrize("dtype", ["fp16"])
def test_dec_512_golden_lattice(dtype):
    g = golden("dec_512")
    sd = W.synth_decoder_state(512, seed=g["seed"])
    feats = W.synth_feats(512, seed=g["seed"])
    dec = pkg.decoder.SynthesisHIP(sd, 512, 512, "cuda:0", dtype=dtype, max_frames=4)
    frames = dec.decode_latent_into_processed_images(g["s_r"], g["r_d"], feats).cpu()
    assert frames.shape == (2, 512, 512, 3)
    lat, band = frames[:, ::7, ::5], frames[:, 250:258]
    p = min(psnr(lat, g["lattice"]), psnr(band, g["band"]))
    m = float((lat - g["lattice"]).abs().mean())
    print(dtype, "512px: PSNR %.1f dB mean|d| %.2e max|d| %.2e mean err of means %.2e" % (
        p, m, float((lat - g["lattice"]).abs().max()), float((frames.mean(dim=(1, 2, 3)) - g["mean"]).abs().max())))
    assert p >= LIMITS[dtype]["psnr"] and m <= LIMITS[dtype]["mean"]
    # per-pixel bound ("max-abs <= 2/255"): measured max 2.6e-2 at isolated pixels (a flow value that rounds the
    # other way moves a bilinear tap across a feature edge); held: <= 0.5 % of the pixels beyond 2/255 (measured 0.23 %), none
    # beyond 0.05
    d = (lat - g["lattice"]).abs()
    frac = float((d > 2.0 / 255).float().mean())
    print("  pixels off by > 2/255: %.4f %%, max %.3e" % (100 * frac, float(d.max())))
    assert frac <= 5e-3 and float(d.max()) <= 0.05
    assert dec.saturation() == 0


def test_dec_512_vs_oracle_levels():
    """Full size against the live oracle (one frame, un-clamped output).  The per-op checks against the reference modules are
    tests/test_dec_units_gpu.py; the per-level logic is held at 1e-4 by the fp32 mode (tests/test_dec_fp32_gpu.py)."""
    sd = W.synth_decoder_state(512, seed=3)
    feats = W.synth_feats(512, seed=3)
    gen = torch.Generator().manual_seed(5)
    s_r, r_d = torch.randn(1, 512, generator=gen), torch.randn(1, 1, 512, generator=gen) * 0.5
    want = O.synthesis(sd, s_r + r_d[:, 0], feats)
    dec = pkg.decoder.SynthesisHIP(sd, 512, 512, "cuda:0", dtype="fp16", max_frames=1)
    dec.set_feats(feats)
    raw = dec.synthesis_raw(s_r, r_d).cpu()
    d = (raw - want).abs()
    print("512 raw: mean|d| %.2e p99.9 %.2e max %.2e (raw std %.2f)" % (
        float(d.mean()), float(d.flatten().kthvalue(int(d.numel() * 0.999))[0]), float(d.max()), float(want.std())))
    assert float(d.mean()) < 1e-2


def test_frames_independent_of_batching():
    """Size-independent property: a frame's pixels do not depend on which batch it was decoded in."""
    sd = W.synth_decoder_state(64, seed=9)
    feats = W.synth_feats(64, seed=9)
    gen = torch.Generator().manual_seed(1)
    s_r, r_d = torch.randn(1, 512, generator=gen), torch.randn(1, 7, 512, generator=gen) * 0.5
    a = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=7)
    b = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=3)
    fa = a.decode_latent_into_processed_images(s_r, r_d, feats).cpu()
    fb = b.decode_latent_into_processed_images(s_r, r_d, feats).cpu()
    assert torch.equal(fa, fb)


def test_dec_errors():
    sd = W.synth_decoder_state(64, seed=9)
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0")
    with pytest.raises(ValueError, match="set_feats"):
        dec.decode_latent_into_processed_images(torch.zeros(1, 512), torch.zeros(1, 1, 512))
    bad = dict(sd)
    del bad["to_flows.0.conv.weight"]
    with pytest.raises(KeyError):
        pkg.decoder.SynthesisHIP(bad, 64, 512, "cuda:0")


def test_decoder_refuses_bf16():
    with pytest.raises(ValueError, match="fp16"):
        pkg.decoder.SynthesisHIP(W.synth_decoder_state(64, seed=1), 64, 512, "cuda:0", dtype="bf16")


@pytest.mark.parametrize("side_stream", [False, True])
def test_decode_into_host_equals_decode(side_stream):
    """float_dec_frames_host: the frames that land in (pinned) host memory batch by batch - behind each batch on the same
    stream, or on a second stream while the next batch renders - are bitwise the frames of float_dec_frames."""
    sd = W.synth_decoder_state(64, seed=4)
    feats = W.synth_feats(64, seed=4)
    gen = torch.Generator().manual_seed(1)
    s_r, r_d = torch.randn(1, 512, generator=gen), torch.randn(1, 11, 512, generator=gen) * 0.5
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=4)  # 11 frames -> 3 batches
    want = dec.decode_latent_into_processed_images(s_r, r_d, feats).cpu()
    host = torch.full((11, 64, 64, 3), -1.0).pin_memory()
    staging = dec.decode_into_host(s_r, r_d, host, copy_stream=torch.cuda.Stream("cuda:0") if side_stream else None)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(host, want) and torch.equal(staging.cpu(), want)
    with pytest.raises(ValueError):
        dec.decode_into_host(s_r, r_d, torch.empty(10, 64, 64, 3))


def test_decode_into_host_ragged_equals_single_batches():
    """A clip that is no multiple of max_frames runs its short piece first (6 frames at max_frames = 4: pieces 2 + 4, the
    full batch carries the short one's copy).  The frames in pinned host memory are bitwise those of calls that decode one
    batch each."""
    sd = W.synth_decoder_state(64, seed=4)
    feats = W.synth_feats(64, seed=4)
    gen = torch.Generator().manual_seed(2)
    s_r, r_d = torch.randn(1, 512, generator=gen), torch.randn(1, 6, 512, generator=gen) * 0.5
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", dtype="fp16", max_frames=4)
    want = torch.cat([dec.decode_latent_into_processed_images(s_r, r_d[:, i:i + 4].contiguous(), feats).cpu() for i in (0, 4)])
    assert want.shape == (6, 64, 64, 3)
    host = torch.full((6, 64, 64, 3), -1.0).pin_memory()
    dec.decode_into_host(s_r, r_d, host)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(host, want)


def test_decode_into_pageable_host():
    """a destination that is NOT pinned must not be written by the copy workgroups (a kernel storing to an
    unmapped host address is a GPU fault).  float_dec_frames_host asks hipPointerGetAttributes and sends pageable memory through
    hipMemcpyAsync behind each batch: same frames, several batches."""
    sd = W.synth_decoder_state(64, seed=4)
    feats = W.synth_feats(64, seed=4)
    gen = torch.Generator().manual_seed(1)
    s_r, r_d = torch.randn(1, 512, generator=gen), torch.randn(1, 11, 512, generator=gen) * 0.5
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=4)  # 11 frames -> 3 batches
    want = dec.decode_latent_into_processed_images(s_r, r_d, feats).cpu()
    host = torch.full((11, 64, 64, 3), -1.0)
    assert not host.is_pinned()
    dec.decode_into_host(s_r, r_d, host)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(host, want)
    # a pinned tensor viewed at an offset that is not 16-byte aligned takes the same path
    big = torch.full((11 * 64 * 64 * 3 + 1,), -1.0).pin_memory()
    off = big[1:].view(11, 64, 64, 3)
    dec.decode_into_host(s_r, r_d, off)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(off, want)


def test_set_feats_validates_every_map():
    """A feature list from a differently sized encoder must be refused before the repack kernel reads it."""
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(64, seed=1), 64, 512, "cuda:0")
    assert dec.feat_shapes() == [(512, 8), (512, 16), (512, 32), (256, 64)]
    good = W.synth_feats(64, seed=1)
    dec.set_feats(good)
    bad = list(good)
    bad[2] = bad[2][:, :, :16, :16]
    with pytest.raises(ValueError, match=r"feats\[2\]"):
        dec.set_feats(bad)
    with pytest.raises(ValueError):
        dec.set_feats(good[:3])


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_dec_channel_multiplier_2(dtype):
    """Synthesis(channel_multiplier=2) of the reference (styledecoder.py:447-467; the widget of Load FLOAT Synthesis,
    nodes_vadv_loader.py:567-611): the operator reads every level's channel count off the checkpoint (512 / 256 channels at
    64 / 128 px here).  Un-clamped output vs the reference: fp32 mode max-abs <= 1e-4, fp16 rel-L2 <= 5e-3."""
    g = golden("dec_cm2_128")
    sd = W.synth_decoder_state(128, seed=g["seed"], channel_multiplier=2)
    feats = W.synth_feats(128, seed=g["seed"], channel_multiplier=2)
    dec = pkg.decoder.SynthesisHIP(sd, 128, 512, "cuda:0", dtype=dtype, max_frames=2)
    assert dec.feat_shapes()[-2:] == [(512, 64), (256, 128)]
    dec.set_feats(feats)
    raw = dec.synthesis_raw(g["s_r"], g["r_d"]).cpu()
    m = float((raw - g["raw"]).abs().max())
    r = float((raw - g["raw"]).norm() / g["raw"].norm())
    print("channel_multiplier 2, %s: max|d| %.2e rel-L2 %.2e" % (dtype, m, r))
    assert (m <= 1e-4) if dtype == "fp32" else (r <= 5e-3)
    assert dec.saturation() == 0


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_blur_kernel_from_checkpoint_and_widget(dtype):
    """A Synthesis trained with another 4-tap blur kernel (tests/golden/dec_blur.npz: reference Synthesis(blur_kernel=[1,2,4,1])
    with that kernel's `conv.blur.kernel` buffers loaded strictly, nodes_vadv_loader.py:567-632).  The operator takes the FIR of
    every up-sampling StyledConv from the checkpoint's buffer; a state without the buffers takes the loader's widget value;
    ToRGB / ToFlow up-sampling kernels of rank > 1 or of another size are refused (rank-1 ones: test_upsample_kernels_from_checkpoint).  fp32 mode max-abs <= 1e-4, fp16 rel-L2 <= 5e-3."""
    g = golden("dec_blur")
    bk = g["kernels"].tolist()[1]
    sd = W.synth_decoder_state(128, seed=g["seed"], blur_kernel=bk)
    feats = W.synth_feats(128, seed=g["seed"])

    def run(state, **kw):
        dec = pkg.decoder.SynthesisHIP(state, 128, 512, "cuda:0", dtype=dtype, max_frames=2, **kw)
        dec.set_feats(feats)
        raw = dec.synthesis_raw(g["s_r"], g["r_d"]).cpu()
        assert dec.saturation() == 0
        return raw

    raw = run(sd)
    m, r = float((raw - g["raw"]).abs().max()), float((raw - g["raw"]).norm() / g["raw"].norm())
    print("blur kernel %s from the checkpoint, %s: max|d| %.2e rel-L2 %.2e" % (bk, dtype, m, r))
    assert (m <= 1e-4) if dtype == "fp32" else (r <= 5e-3)
    bare = {k: v for k, v in sd.items() if not k.endswith("blur.kernel")}
    assert torch.equal(run(bare, blur_kernel=bk), raw)  # the widget value where the state has no buffers
    dflt = run(bare)
    assert float((dflt - g["raw"]).norm() / g["raw"].norm()) > 0.05  # [1,3,3,1] is a different decoder
    assert torch.equal(run(sd, blur_kernel=[1, 3, 3, 1]), raw)  # a contradicting widget loses to the checkpoint (strict load)
    odd = dict(sd)
    odd["to_rgbs.1.upsample.kernel"] = torch.eye(4)  # rank 4: not ky (x) kx
    with pytest.raises(ValueError, match="rank-1"):
        pkg.decoder.SynthesisHIP(odd, 128, 512, "cuda:0", dtype=dtype, max_frames=2)
    odd["to_rgbs.1.upsample.kernel"] = torch.ones(3, 3) / 9 * 4  # the Upsample's padding belongs to 4 taps
    with pytest.raises(ValueError, match="4 x 4"):
        pkg.decoder.SynthesisHIP(odd, 128, 512, "cuda:0", dtype=dtype, max_frames=2)
    with pytest.raises(ValueError, match="4-tap"):
        pkg.decoder.SynthesisHIP(sd, 128, 512, "cuda:0", dtype=dtype, max_frames=2, blur_kernel=[1, 2, 1])


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_upsample_kernels_from_checkpoint(dtype):
    """ToRGB / ToFlow `upsample.kernel` buffers that are not make_kernel([1,3,3,1]) * 4 (tests/golden/fir_buffers.npz: the reference
    Synthesis after a strict load of weights.fir_buffer_states - ToRGB make_kernel([1,2,4,1]) * 4, ToFlow 4 outer([1,3,3,1],
    [1,2,4,1]) / 64: asymmetric, different per axis and per module).  dec_flow_kernel takes the per-axis taps of both Upsamples
    from the checkpoint.  fp32 mode max-abs <= 1e-4, fp16 rel-L2 <= 5e-3; the default kernels are a 41 % different decoder, and a
    state without the buffers decodes bitwise like one that holds the default buffers."""
    g = golden("fir_buffers")
    size, seed = int(g["size"]), int(g["seed"])
    _, sd = W.fir_buffer_states(size, seed)
    feats = W.synth_feats(size, seed=seed)

    def run(state):
        dec = pkg.decoder.SynthesisHIP(state, size, 512, "cuda:0", dtype=dtype, max_frames=2)
        dec.set_feats(feats)
        raw = dec.synthesis_raw(g["dec_s_r"], g["dec_r_d"]).cpu()
        assert dec.saturation() == 0
        return raw

    raw = run(sd)
    m, r = float((raw - g["dec_raw"]).abs().max()), float((raw - g["dec_raw"]).norm() / g["dec_raw"].norm())
    print("upsample kernels from the checkpoint, %s: max|d| %.2e rel-L2 %.2e" % (dtype, m, r))
    assert (m <= 1e-4) if dtype == "fp32" else (r <= 5e-3)
    sd0 = W.synth_decoder_state(size, seed=seed)
    dflt = run(sd0)
    assert float((dflt - g["dec_raw"]).norm() / g["dec_raw"].norm()) > 0.1
    assert torch.equal(run({k: v for k, v in sd0.items() if not k.endswith("upsample.kernel")}), dflt)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_upsample_kernels_at_512(dtype):
    """The same non-default ToRGB / ToFlow up-sampling buffers at 512 px (the 256- and 512-px levels run dec_flow_kernel with 4
    pixels per lane group, the golden's 64-px decoder only the 2-pixel form), one frame against the oracle - which equals the
    reference to the last bit on tests/golden/fir_buffers.npz."""
    from oracle import float_oracle as O
    _, sd = W.fir_buffer_states(512, 2100)
    feats = W.synth_feats(512, seed=2100)
    g = torch.Generator().manual_seed(2100)
    s_r, r_d = torch.randn(1, 512, generator=g), torch.randn(1, 1, 512, generator=g) * 0.5
    want = O.synthesis(sd, s_r + r_d[:, 0], feats)
    dec = pkg.decoder.SynthesisHIP(sd, 512, 512, "cuda:0", dtype=dtype, max_frames=2)
    dec.set_feats(feats)
    raw = dec.synthesis_raw(s_r, r_d).cpu()
    m, r = float((raw - want).abs().max()), float((raw - want).norm() / want.norm())
    print("512 px, upsample kernels from the checkpoint, %s: max|d| %.2e rel-L2 %.2e" % (dtype, m, r))
    assert dec.saturation() == 0
    # fp32 mode: rel-L2 5e-6, single pixels 2.6e-4 (the warp turns a 1e-7 difference in a flow into a sampling difference)
    assert (m <= 5e-4 and r <= 2e-5) if dtype == "fp32" else (r <= 5e-3)
