"""Planar YUV 4:2:0 frames (float_dec_frames_i420 / float_dec_frames_host_i420): I420, BT.601 limited range, converted on the
device.  The format is defined in integers FROM the 8-bit RGB samples the u8 mode stores (host_models.rgb8_to_i420), so whichever
kernel forms the planes - dec_flowlast_kernel's I420 instantiation on the product path, or dec_rgb8_to_i420_kernel behind a last
level that runs in dec_flow_kernel - the bytes are rgb8_to_i420(decode_u8(...)) of the same handle: every comparison below is
torch.equal, there is no tolerance anywhere."""
import importlib
import warnings

import numpy as np
import pytest
import torch

from tests.util import golden, load_pkg

pkg = load_pkg()
W = pkg.weights
pytestmark = pytest.mark.gpu
to_i420 = pkg.host_models.rgb8_to_i420


def _inputs(seed, n):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(1, 512, generator=gen), torch.randn(1, n, 512, generator=gen) * 0.5


def _exact(dec, s_r, r_d, feats):
    dec.set_feats(feats)
    R = dec.size
    rgb = dec.decode_u8(s_r, r_d)
    want = to_i420(rgb).cpu()
    got = dec.decode_i420(s_r, r_d)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (rgb.shape[0], 3 * R // 2, R)
    got = got.cpu()
    y, c = got[:, :R], got[:, R:]
    print("  %d px: Y levels %d, chroma levels %d, bytes that differ from rgb8_to_i420(decode_u8): Y %d, chroma %d of %d" % (
        R, int(y.unique().numel()), int(c.unique().numel()), int((y != want[:, :R]).sum()), int((c != want[:, R:]).sum()), got.numel()))
    assert torch.equal(got, want)
    # a real image, not a constant: more than 16 distinct Y values, and U and V not all 128
    assert int(y.unique().numel()) > 16
    u, v = c.reshape(c.shape[0], 2, -1)[:, 0], c.reshape(c.shape[0], 2, -1)[:, 1]
    assert bool((u != 128).any()) and bool((v != 128).any())
    assert 16 <= int(y.min()) and int(y.max()) <= 235 and 16 <= int(c.min()) and int(c.max()) <= 240
    return got


# ---------------------------------------------------------------------------------------------------------------------------
# 1. - 5. exactness against the u8 output of the same handle, on every route
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_i420_64(dtype):
    """64 px, 3 frames in batches of 2: the last level runs dec_flow_kernel (256 channels), the converter follows it."""
    g = golden("dec_64")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(64, seed=g["seed"]), 64, 512, "cuda:0", dtype=dtype, max_frames=2)
    _exact(dec, g["s_r"], g["r_d"], W.synth_feats(64, seed=g["seed"]))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_i420_256_fused(dtype):
    """The default 256-px model (64 channels on the last level), 3 frames in batches of 2: the fused form with two workgroups
    per row pair - the smallest size with a workgroup seam inside a row."""
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(256, seed=78), 256, 512, "cuda:0", dtype=dtype, max_frames=2)
    assert dec.feat_shapes()[-1] == (64, 256)
    s_r, r_d = _inputs(78, 3)
    _exact(dec, s_r, r_d, W.synth_feats(256, seed=78))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_i420_512_fused_and_converter(dtype, monkeypatch):
    """512 px, batches of 4: the fused form, then FLOAT_DEC_YUV_FUSED=0 (read when the handle is created) for the converter on the
    same inputs; the two forms give the same bytes."""
    g = golden("dec_512")
    sd, feats = W.synth_decoder_state(512, seed=g["seed"]), W.synth_feats(512, seed=g["seed"])
    monkeypatch.delenv("FLOAT_DEC_YUV_FUSED", raising=False)
    fused = pkg.decoder.SynthesisHIP(sd, 512, 512, "cuda:0", dtype=dtype, max_frames=4)
    a = _exact(fused, g["s_r"], g["r_d"], feats)
    fused.close()
    monkeypatch.setenv("FLOAT_DEC_YUV_FUSED", "0")
    conv = pkg.decoder.SynthesisHIP(sd, 512, 512, "cuda:0", dtype=dtype, max_frames=4)
    b = _exact(conv, g["s_r"], g["r_d"], feats)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_i420_256_flow_kernel(dtype):
    """channel_multiplier 2 gives the 256-px last level 128 channels: dec_flow_kernel + converter.  3 frames in batches of 2."""
    sd = W.synth_decoder_state(256, seed=77, channel_multiplier=2)
    dec = pkg.decoder.SynthesisHIP(sd, 256, 512, "cuda:0", dtype=dtype, max_frames=2)
    assert dec.feat_shapes()[-1] == (128, 256)
    s_r, r_d = _inputs(77, 3)
    _exact(dec, s_r, r_d, W.synth_feats(256, seed=77, channel_multiplier=2))


def test_i420_512_without_the_epilogue(monkeypatch):
    """FLOAT_DEC_FLOW_EPI=0: the 512-px last level falls back to dec_flow_kernel, and I420 to the converter with it."""
    monkeypatch.setenv("FLOAT_DEC_FLOW_EPI", "0")
    g = golden("dec_512")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(512, seed=g["seed"]), 512, 512, "cuda:0", dtype="fp16", max_frames=2)
    _exact(dec, g["s_r"], g["r_d"], W.synth_feats(512, seed=g["seed"]))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. hand-over
# ---------------------------------------------------------------------------------------------------------------------------
def _handover_case():
    sd, feats = W.synth_decoder_state(64, seed=4), W.synth_feats(64, seed=4)
    s_r, r_d = _inputs(1, 11)
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=4)  # 11 frames -> 3 batches
    dec.set_feats(feats)
    return dec, s_r, r_d, to_i420(dec.decode_u8(s_r, r_d)).cpu()


@pytest.mark.parametrize("form", ["pinned", "pinned_side_stream", "pageable", "pinned_misaligned"])
def test_i420_hand_over(form):
    """float_dec_frames_host_i420 under float_dec_frames_host_u8's contract: copy workgroups through pinned 16-byte-aligned memory,
    hipMemcpyAsync for everything else (pageable memory, a pinned tensor viewed at a 1-byte offset), the side-stream form; after
    synchronising the current stream the host tensor and the staging tensor are bitwise the reference."""
    dec, s_r, r_d, want = _handover_case()
    n = 11 * 96 * 64
    if form == "pageable":
        host = torch.full((11, 96, 64), 7, dtype=torch.uint8)
        assert not host.is_pinned()
    elif form == "pinned_misaligned":
        big = torch.full((n + 1,), 7, dtype=torch.uint8).pin_memory()
        host = big[1:].view(11, 96, 64)
        assert host.data_ptr() % 16 == 1
    else:
        host = torch.full((11, 96, 64), 7, dtype=torch.uint8).pin_memory()
    cs = torch.cuda.Stream("cuda:0") if form == "pinned_side_stream" else None
    staging = dec.decode_into_host(s_r, r_d, host, copy_stream=cs, out_format="i420")
    torch.cuda.current_stream().synchronize()
    assert staging.dtype == torch.uint8 and staging.is_cuda and tuple(staging.shape) == (11, 96, 64)
    assert torch.equal(host, want) and torch.equal(staging.cpu(), want)


def test_i420_hand_over_argument_rules():
    dec, s_r, r_d, want = _handover_case()
    with pytest.raises(ValueError):
        dec.decode_into_host(s_r, r_d, torch.empty(10, 96, 64, dtype=torch.uint8), out_format="i420")  # wrong length
    with pytest.raises(ValueError):
        dec.decode_into_host(s_r, r_d, torch.empty(11, 64, 64, 3, dtype=torch.uint8), out_format="i420")  # RGB-shaped
    with pytest.raises(ValueError):
        dec.decode_into_host(s_r, r_d, torch.empty(11, 96, 64, dtype=torch.uint8), out_format="rgb")  # I420-shaped
    with pytest.raises(ValueError):
        dec.decode_into_host(s_r, r_d, torch.empty(11, 96, 64, dtype=torch.float32), out_format="i420")  # I420 is uint8
    with pytest.raises(ValueError):
        dec.decode_into_host(s_r, r_d, torch.empty(11, 96, 64, dtype=torch.uint8), out_format="nv12")
    # a staging tensor of another format is replaced and left untouched, even one with as many bytes or more
    host = torch.full((11, 96, 64), 7, dtype=torch.uint8).pin_memory()
    wrong = torch.zeros(11, 64, 64, 3, device="cuda:0", dtype=torch.uint8)
    staging = dec.decode_into_host(s_r, r_d, host, wrong, out_format="i420")
    torch.cuda.current_stream().synchronize()
    assert staging is not wrong and tuple(staging.shape) == (11, 96, 64)
    assert torch.equal(host, want) and int(wrong.max()) == 0
    # and the format follows the destination's shape where it is not stated
    host2 = torch.full((11, 96, 64), 7, dtype=torch.uint8).pin_memory()
    kept = dec.decode_into_host(s_r, r_d, host2, staging)
    torch.cuda.current_stream().synchronize()
    assert kept is staging and torch.equal(host2, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. no leakage between formats, 8. batch independence
# ---------------------------------------------------------------------------------------------------------------------------
def test_three_formats_alternate_on_one_handle():
    """fp32, u8, I420, fp32 hand-overs on one handle: the ride-along state of one call does not reach the next."""
    dec, s_r, r_d, want420 = _handover_case()
    want = dec.decode_latent_into_processed_images(s_r, r_d).cpu()
    want8 = dec.decode_u8(s_r, r_d).cpu()
    a = torch.full((11, 64, 64, 3), -1.0).pin_memory()
    b = torch.full((11, 64, 64, 3), 7, dtype=torch.uint8).pin_memory()
    c = torch.full((11, 96, 64), 7, dtype=torch.uint8).pin_memory()
    d = torch.full((11, 64, 64, 3), -1.0).pin_memory()
    dec.decode_into_host(s_r, r_d, a)
    dec.decode_into_host(s_r, r_d, b)
    dec.decode_into_host(s_r, r_d, c, out_format="i420")
    dec.decode_into_host(s_r, r_d, d)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(a, d) and torch.equal(a, want)
    assert torch.equal(b, want8) and torch.equal(c, want420) and torch.equal(c, to_i420(b))


def test_i420_frames_independent_of_batching():
    sd, feats = W.synth_decoder_state(64, seed=9), W.synth_feats(64, seed=9)
    s_r, r_d = _inputs(1, 7)
    a = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=7)
    b = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=3)
    assert torch.equal(a.decode_i420(s_r, r_d, feats).cpu(), b.decode_i420(s_r, r_d, feats).cpu())


# ---------------------------------------------------------------------------------------------------------------------------
# 9. through the product, 10. the precision guard
# ---------------------------------------------------------------------------------------------------------------------------
def _agent(**kw):
    """The synthetic 64-px agent of tests/test_dec_u8_gpu.py."""
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


def test_agent_i420_frames(monkeypatch):
    for v in GUARD_ENV:
        monkeypatch.delenv(v, raising=False)
    agent, img, wav = _agent()
    run = lambda **kw: agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7, **kw)  # noqa: E731
    f32 = run().clone()
    u8 = run(out_dtype=torch.uint8).clone()
    yuv = run(out_format="i420")
    assert yuv.dtype == torch.uint8 and yuv.is_pinned() and tuple(yuv.shape) == (35, 96, 64)
    assert torch.equal(yuv, to_i420(u8))
    again = run()  # and back: the staging cache is keyed by format
    assert again.dtype == torch.float32 and torch.equal(again, f32)
    assert torch.equal(run(out_dtype=torch.uint8, out_format="i420"), yuv)
    # a caller-supplied destination fixes the format; contradicting it is refused
    mine = torch.full((35, 96, 64), 7, dtype=torch.uint8).pin_memory()
    got = run(out=mine)
    assert got is mine and torch.equal(mine, yuv)
    assert run(out=mine, out_format="i420") is mine
    rgb = torch.full((35, 64, 64, 3), 7, dtype=torch.uint8).pin_memory()
    for kw in (dict(out=mine, out_format="rgb"), dict(out=rgb, out_format="i420"), dict(out_format="i420", out_dtype=torch.float32),
               dict(out=torch.empty(35, 64, 64, 3).pin_memory(), out_format="i420"), dict(out_format="nv12")):
        with pytest.raises(ValueError):
            run(**kw)
    assert int(rgb.min()) == 7  # a refused call wrote nothing


def test_agent_i420_batch_of_ragged_lengths(monkeypatch):
    for v in GUARD_ENV:
        monkeypatch.delenv(v, raising=False)
    agent, img, wav = _agent()
    img2 = torch.from_numpy(np.random.RandomState(6).rand(1, 3, 64, 64).astype(np.float32)).cuda() * 2 - 1
    items = [(img, wav), (img2, W.synth_waveform(0.6, seed=10).cuda())]  # 35 and 15 frames
    u8 = [t.clone() for t in agent.infer_device_batch(items, 2.0, 1.0, 1.0, emo="happy", seeds=[7, 8], out_dtype=torch.uint8)]
    yuv = agent.infer_device_batch(items, 2.0, 1.0, 1.0, emo="happy", seeds=[7, 8], out_format="i420")
    assert [tuple(t.shape) for t in yuv] == [(35, 96, 64), (15, 96, 64)]
    for a, b in zip(yuv, u8):
        assert a.dtype == torch.uint8 and a.is_pinned()
        assert torch.equal(a, to_i420(b))
    with pytest.raises(ValueError):
        agent.infer_device_batch(items, 2.0, 1.0, 1.0, emo="happy", seeds=[7, 8], out_format="i420", out_dtype=torch.float32)


def test_guard_reports_the_same_numbers_for_i420(monkeypatch):
    """FLOAT_AMD_VERIFY=first: with I420 output the guard decodes its k frames once more in the fp32 form, as for 8-bit RGB, so
    every figure of the report is the one an fp32 clip gives."""
    for v in GUARD_ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FLOAT_AMD_VERIFY", "first")
    reps = {}
    for fmt in (None, "i420"):
        agent, img, wav = _agent()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # which side of 40 dB the synthetic model lands on is not the point
            out = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=7, out_format=fmt)
        assert tuple(out.shape) == ((35, 96, 64) if fmt else (35, 64, 64, 3))
        reps[fmt] = agent.last_precision_report
        assert reps[fmt] is not None
        agent.offload()
    a, b = reps[None], reps["i420"]
    for name in ("fmt", "decoder", "end_to_end"):
        print("guard %s: fp32 output %s | I420 output %s" % (name, a[name], b[name]))
        assert a[name] == b[name]
    assert a["k"] == b["k"] == 8 and a["n"] == b["n"] == 35
