"""8-bit frames (float_dec_frames_u8 / float_dec_frames_host_u8): HWC uint8, quantised on the device by the kernel that forms the
frame.  Definition: with y the value the fp32 mode stores (clamp(v, -1, 1) * 0.5 + 0.5), q = (uint8) rintf(y * 255.0f) - one
multiply, one round-half-to-even, nothing to contract - so q is BITWISE torch.round(frames_fp32 * 255).to(torch.uint8) of the same
handle.  Every comparison with the fp32 output below is therefore torch.equal, with no tolerance.

Against the reference's frames (tests/golden) the bounds are derived, not measured:
  fp32 handle: the fp32 mode is held to 1e-4 max-abs against these goldens (tests/test_dec_fp32_gpu.py); 1e-4 * 255 < 0.5, so a
    value can cross at most one rounding boundary: |u8 - round(255 golden)| <= 1 at every pixel.
  fp16 handle: the limits of tests/test_dec_gpu.py applied to u8 / 255 with one quantisation step added to the per-pixel bounds:
    PSNR >= 52 dB, <= 0.5 % of the pixels beyond 3/255, max <= 0.05 + 1/255 (64 px: max <= 3/255 outright)."""
import importlib
import math
import warnings

import numpy as np
import pytest
import torch

from tests.util import golden, load_pkg

pkg = load_pkg()
W = pkg.weights
pytestmark = pytest.mark.gpu


def q8(frames):
    return torch.round(frames * 255).to(torch.uint8)


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


def _inputs(seed, n):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(1, 512, generator=gen), torch.randn(1, n, 512, generator=gen) * 0.5


def _exact(dec, s_r, r_d, feats):
    dec.set_feats(feats)
    want = q8(dec.decode_latent_into_processed_images(s_r, r_d)).cpu()
    got = dec.decode_u8(s_r, r_d)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == tuple(want.shape)
    got = got.cpu()
    print("  u8 levels used: %d, pixels that differ from round(255 fp32): %d of %d" % (
        int(got.unique().numel()), int((got != want).sum()), got.numel()))
    assert torch.equal(got, want)
    assert int(got.unique().numel()) > 16  # a real image, not a constant
    return got


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exactness against the fp32 output of the same handle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_u8_equals_rounded_fp32_64(dtype):
    """64 px, 3 frames in batches of 2: the last level runs dec_flow_kernel (256 channels)."""
    g = golden("dec_64")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(64, seed=g["seed"]), 64, 512, "cuda:0", dtype=dtype, max_frames=2)
    _exact(dec, g["s_r"], g["r_d"], W.synth_feats(64, seed=g["seed"]))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_u8_equals_rounded_fp32_512(dtype):
    """512 px: the product's path - ToFlow in conv2's epilogue, dec_flowlast_kernel packs a quad's 12 bytes into three dwords."""
    g = golden("dec_512")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(512, seed=g["seed"]), 512, 512, "cuda:0", dtype=dtype, max_frames=4)
    _exact(dec, g["s_r"], g["r_d"], W.synth_feats(512, seed=g["seed"]))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_u8_equals_rounded_fp32_256_flow_kernel(dtype):
    """A 256-px model whose last level goes through dec_flow_kernel: channel_multiplier 2 gives it 128 channels there (the ToFlow
    epilogue takes 32 or 64).  3 frames in batches of 2."""
    sd = W.synth_decoder_state(256, seed=77, channel_multiplier=2)
    dec = pkg.decoder.SynthesisHIP(sd, 256, 512, "cuda:0", dtype=dtype, max_frames=2)
    assert dec.feat_shapes()[-1] == (128, 256)
    s_r, r_d = _inputs(77, 3)
    _exact(dec, s_r, r_d, W.synth_feats(256, seed=77, channel_multiplier=2))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_u8_equals_rounded_fp32_256_epilogue(dtype):
    """The default 256-px model (64 channels on the last level): dec_flowlast_kernel at another size."""
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(256, seed=78), 256, 512, "cuda:0", dtype=dtype, max_frames=2)
    assert dec.feat_shapes()[-1] == (64, 256)
    s_r, r_d = _inputs(78, 3)
    _exact(dec, s_r, r_d, W.synth_feats(256, seed=78))


def test_u8_equals_rounded_fp32_512_without_the_epilogue(monkeypatch):
    """FLOAT_DEC_FLOW_EPI=0 (read when the handle is created): the 512-px last level falls back to dec_flow_kernel with 4 lanes per
    pixel - the byte-store form of the 8-bit mode."""
    monkeypatch.setenv("FLOAT_DEC_FLOW_EPI", "0")
    g = golden("dec_512")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(512, seed=g["seed"]), 512, 512, "cuda:0", dtype="fp16", max_frames=2)
    _exact(dec, g["s_r"], g["r_d"], W.synth_feats(512, seed=g["seed"]))


def test_u8_and_i420_into_a_callers_buffer():
    """decode_u8 / decode_i420 with out=: 3 frames at 64 px in batches of 2 land in the caller's tensor, which is returned, bitwise
    the call without it; a buffer of another shape, dtype or device, or a strided one, is refused before anything runs."""
    g = golden("dec_64")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(64, seed=g["seed"]), 64, 512, "cuda:0", max_frames=2)
    try:
        dec.set_feats(W.synth_feats(64, seed=g["seed"]))
        s_r, r_d = g["s_r"], g["r_d"]
        for fn, shape in ((dec.decode_u8, (3, 64, 64, 3)), (dec.decode_i420, (3, 96, 64))):
            want = fn(s_r, r_d)
            assert tuple(want.shape) == shape
            buf = torch.full(shape, 7, dtype=torch.uint8, device="cuda:0")
            assert fn(s_r, r_d, out=buf) is buf and torch.equal(buf, want)
            part = torch.full((5,) + shape[1:], 7, dtype=torch.uint8, device="cuda:0")  # a prefix view, as the stream ring passes
            assert torch.equal(fn(s_r, r_d, out=part[:3]), want) and int(part[3:].min()) == int(part[3:].max()) == 7
            for bad in (torch.empty((2,) + shape[1:], dtype=torch.uint8, device="cuda:0"), torch.empty(shape, device="cuda:0"),
                        torch.empty(shape, dtype=torch.uint8), torch.empty((6,) + shape[1:], dtype=torch.uint8, device="cuda:0")[::2]):
                with pytest.raises(ValueError):
                    fn(s_r, r_d, out=bad)
    finally:
        dec.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against the reference's frames
# ---------------------------------------------------------------------------------------------------------------------------
def _golden_pairs(size, dtype):
    """[(name, u8 of the operator, the reference's fp32 frames)] on the golden's sample of the frames."""
    g = golden("dec_%d" % size)
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(size, seed=g["seed"]), size, 512, "cuda:0", dtype=dtype,
                                   max_frames=2 if size == 64 else 4)
    got = dec.decode_u8(g["s_r"], g["r_d"], W.synth_feats(size, seed=g["seed"])).cpu()
    assert dec.saturation() == 0
    if size == 64:
        assert got.shape == g["frames"].shape
        return [("frames", got, g["frames"])]
    assert got.shape == (2, 512, 512, 3)
    return [("lattice", got[:, ::7, ::5], g["lattice"]), ("band", got[:, 250:258], g["band"])]


@pytest.mark.parametrize("size", [64, 512])
def test_u8_fp32_handle_within_one_level_of_the_reference(size):
    for name, got, ref in _golden_pairs(size, "fp32"):
        d = (got.int() - q8(ref).int()).abs()
        print("fp32 handle, %d px %s: %.4f %% of the pixels differ from round(255 golden), max %d level(s)" % (
            size, name, 100.0 * float((d > 0).float().mean()), int(d.max())))
        assert int(d.max()) <= 1


@pytest.mark.parametrize("size", [64, 512])
def test_u8_fp16_handle_holds_the_fp16_limits_plus_one_level(size):
    for name, got, ref in _golden_pairs(size, "fp16"):
        f = got.float() / 255
        d = (f - ref).abs()
        p, frac, mx = psnr(f, ref), float((d > 3.0 / 255).float().mean()), float(d.max())
        print("fp16 handle, %d px %s: PSNR %.1f dB, mean|d| %.2e, %.4f %% beyond 3/255, max %.3e" % (
            size, name, p, float(d.mean()), 100 * frac, mx))
        assert p >= 52.0
        assert frac <= 5e-3
        assert mx <= (3.0 / 255 if size == 64 else 0.05 + 1.0 / 255)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. hand-over
# ---------------------------------------------------------------------------------------------------------------------------
def _handover_case():
    sd, feats = W.synth_decoder_state(64, seed=4), W.synth_feats(64, seed=4)
    s_r, r_d = _inputs(1, 11)
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=4)  # 11 frames -> 3 batches
    dec.set_feats(feats)
    return dec, s_r, r_d, dec.decode_u8(s_r, r_d).cpu()


@pytest.mark.parametrize("form", ["pinned", "pinned_side_stream", "pageable", "pinned_misaligned"])
def test_u8_hand_over(form):
    """float_dec_frames_host_u8 under float_dec_frames_host's contract: copy workgroups through pinned 16-byte-aligned memory,
    hipMemcpyAsync for everything else (pageable memory, a pinned tensor viewed at a 1-byte offset), the side-stream form; after
    synchronising the current stream the host tensor and the staging tensor are bitwise decode_u8."""
    dec, s_r, r_d, want = _handover_case()
    n = 11 * 64 * 64 * 3
    if form == "pageable":
        host = torch.full((11, 64, 64, 3), 7, dtype=torch.uint8)
        assert not host.is_pinned()
    elif form == "pinned_misaligned":
        big = torch.full((n + 1,), 7, dtype=torch.uint8).pin_memory()
        host = big[1:].view(11, 64, 64, 3)
        assert host.data_ptr() % 16 == 1
    else:
        host = torch.full((11, 64, 64, 3), 7, dtype=torch.uint8).pin_memory()
    cs = torch.cuda.Stream("cuda:0") if form == "pinned_side_stream" else None
    staging = dec.decode_into_host(s_r, r_d, host, copy_stream=cs)
    torch.cuda.current_stream().synchronize()
    assert staging.dtype == torch.uint8 and staging.is_cuda
    assert torch.equal(host, want) and torch.equal(staging.cpu(), want)


def test_u8_hand_over_argument_rules():
    dec, s_r, r_d, want = _handover_case()
    with pytest.raises(ValueError):
        dec.decode_into_host(s_r, r_d, torch.empty(10, 64, 64, 3, dtype=torch.uint8))  # wrong length
    with pytest.raises(ValueError):
        dec.decode_into_host(s_r, r_d, torch.empty(11, 64, 64, 3, dtype=torch.float16))  # neither fp32 nor uint8
    # a staging tensor of the other dtype is replaced, not reinterpreted
    host = torch.full((11, 64, 64, 3), 7, dtype=torch.uint8).pin_memory()
    wrong = torch.zeros(11, 64, 64, 3, device="cuda:0", dtype=torch.float32)
    staging = dec.decode_into_host(s_r, r_d, host, wrong)
    torch.cuda.current_stream().synchronize()
    assert staging is not wrong and staging.dtype == torch.uint8
    assert torch.equal(host, want) and float(wrong.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. no leakage between formats, 5. batch independence
# ---------------------------------------------------------------------------------------------------------------------------
def test_formats_alternate_on_one_handle():
    """fp32 hand-over, u8 hand-over, fp32 hand-over on one handle: the ride-along state of one call does not reach the next."""
    dec, s_r, r_d, want8 = _handover_case()
    want = dec.decode_latent_into_processed_images(s_r, r_d).cpu()
    a = torch.full((11, 64, 64, 3), -1.0).pin_memory()
    b = torch.full((11, 64, 64, 3), 7, dtype=torch.uint8).pin_memory()
    c = torch.full((11, 64, 64, 3), -1.0).pin_memory()
    dec.decode_into_host(s_r, r_d, a)
    dec.decode_into_host(s_r, r_d, b)
    dec.decode_into_host(s_r, r_d, c)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(a, c) and torch.equal(a, want)
    assert torch.equal(b, want8) and torch.equal(b, q8(want))


def test_u8_frames_independent_of_batching():
    sd, feats = W.synth_decoder_state(64, seed=9), W.synth_feats(64, seed=9)
    s_r, r_d = _inputs(1, 7)
    a = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=7)
    b = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=3)
    assert torch.equal(a.decode_u8(s_r, r_d, feats).cpu(), b.decode_u8(s_r, r_d, feats).cpu())


# ---------------------------------------------------------------------------------------------------------------------------
# 6. through the product
# ---------------------------------------------------------------------------------------------------------------------------
def _agent(**kw):
    """The synthetic 64-px agent of tests/test_precision_guard_gpu.py."""
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.input_size, opt.nfe = 64, 6
    C = pkg.config
    cfg = C.FmtConfig.from_options(opt)
    acfg = C.small_audio_config()
    acfg.dim_w = opt.dim_w
    parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
                 audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
    img = torch.from_numpy(np.random.RandomState(5).rand(1, 3, 64, 64).astype(np.float32)) * 2 - 1
    wav = W.synth_waveform(1.4, seed=9)  # 35 frames: one window, replicate-padded
    return gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8, **kw), img.cuda(), wav.cuda()


GUARD_ENV = ("FLOAT_AMD_VERIFY", "FLOAT_AMD_VERIFY_ACTION", "FLOAT_AMD_VERIFY_FRAMES", "FLOAT_AMD_VERIFY_PSNR")


def test_agent_u8_frames(monkeypatch):
    for v in GUARD_ENV:
        monkeypatch.delenv(v, raising=False)
    agent, img, wav = _agent()
    f32 = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7).clone()
    u8 = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7, out_dtype=torch.uint8)
    assert u8.dtype == torch.uint8 and u8.is_pinned() and tuple(u8.shape) == (35, 64, 64, 3)
    assert torch.equal(u8, q8(f32))
    again = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7)  # and back: the staging cache is keyed by dtype
    assert again.dtype == torch.float32 and torch.equal(again, f32)
    # a caller-supplied destination fixes the format; contradicting it is refused
    mine = torch.full((35, 64, 64, 3), 7, dtype=torch.uint8).pin_memory()
    got = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7, out=mine)
    assert got is mine and torch.equal(mine, u8)
    with pytest.raises(ValueError):
        agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7, out=mine, out_dtype=torch.float32)
    with pytest.raises(ValueError):
        agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7, out_dtype=torch.float16)


def test_agent_u8_batch(monkeypatch):
    for v in GUARD_ENV:
        monkeypatch.delenv(v, raising=False)
    agent, img, wav = _agent()
    img2 = torch.from_numpy(np.random.RandomState(6).rand(1, 3, 64, 64).astype(np.float32)).cuda() * 2 - 1
    items = [(img, wav), (img2, wav)]
    f32 = [t.clone() for t in agent.infer_device_batch(items, 2.0, 1.0, 1.0, emo="happy", seeds=[7, 8])]
    u8 = agent.infer_device_batch(items, 2.0, 1.0, 1.0, emo="happy", seeds=[7, 8], out_dtype=torch.uint8)
    assert len(u8) == 2
    for a, b in zip(u8, f32):
        assert a.dtype == torch.uint8 and a.is_pinned() and tuple(a.shape) == (35, 64, 64, 3)
        assert torch.equal(a, q8(b))
    assert not torch.equal(u8[0], u8[1])


def test_guard_reports_the_same_numbers_for_both_formats(monkeypatch):
    """FLOAT_AMD_VERIFY=first: with 8-bit output the guard decodes its k frames once more in the fp32 form, so every figure of the
    report is the one an fp32 clip gives."""
    for v in GUARD_ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FLOAT_AMD_VERIFY", "first")
    reps = {}
    for dt in (torch.float32, torch.uint8):
        agent, img, wav = _agent()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # which side of 40 dB the synthetic model lands on is not the point
            out = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7, out_dtype=dt)
        assert out.dtype == dt
        reps[dt] = agent.last_precision_report
        assert reps[dt] is not None
        agent.offload()
    a, b = reps[torch.float32], reps[torch.uint8]
    for name in ("fmt", "decoder", "end_to_end"):
        print("guard %s: fp32 output %s | u8 output %s" % (name, a[name], b[name]))
        assert a[name] == b[name]
    assert a["k"] == b["k"] == 8 and a["n"] == b["n"] == 35
