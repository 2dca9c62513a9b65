"""float_aud_front on the GPU: mono mix, band-limited resampling and normalisation of a waveform in HBM, against
host_models.resample_sinc_direct (the closed form in fp64) with the host resampler's own fp32 error as the yardstick.

Yardstick.  Per case, from one seeded input (noise of sigma 0.3 clamped to +-1): ref = resample_sinc_direct in fp64,
e_host = max |resample_sinc(fp32 input) - ref|, e_dev = max |device - ref| with flags = 0; required: e_dev <= 4 * e_host.  For
44099 -> 16000 and 44100 -> 16001 the host function is an approximation: e_host comes from the 44100 -> 16000 run on an input
of the same length.

Tile.  A workgroup of audf_resample_kernel owns TILE = 256 consecutive outputs (kAudfTile, csrc/audf_kernels.hpp); the lengths
below are derived from it: n_in = 1, 7 (the whole clip inside one tap window), exactly one tile of outputs, one tile + 1 (one more
input sample where up-sampling skips it), three tiles + 37 with n_in no multiple of `down` (the last window runs past the end).

Measured e_dev / e_host, one MI355X, 2026-10-18 (lengths in the order above; e_host 1.3e-7 ... 2.8e-7 from one tile up, e_dev
6e-9 ... 9.6e-8; with 1 ... 14 outputs both are a few roundings, 1.00 = the same rounding of the same value):
  48000 -> 16000     1.00 2.43 0.24 0.14 0.17        44099 -> 16000     1.93 1.20 0.34 0.21 0.30
  32000 -> 16000     1.00 0.92 0.13 0.14 0.16        44100 -> 16001     0.62 1.92 0.26 0.19 0.21
  44100 -> 16000     1.00 1.17 0.36 0.27 0.22        192000 -> 16000    1.00 1.00 0.07 0.07 0.07
  22050 -> 16000     1.00 0.88 0.74 1.04 0.57        1024000 -> 16000   1.00 0.37 0.04 0.03 0.04
  11025 -> 16000     1.00 0.54 0.98 0.56 0.47        250 -> 16000       2.34 0.85 0.94 0.80 0.75
  8000 -> 16000      1.00 1.41 0.22 0.19 0.19        320 s of 44.1 kHz  0.27 (1112 indices)
  host_inputs at 48 kHz stereo after un-normalising 0.11; run_inference front end on against off 73.0 dB.
"""
import ctypes as C
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm, W = pkg.host_models, pkg.weights
pytestmark = pytest.mark.gpu

TILE = 256  # kAudfTile
RATIOS = [(48000, 16000), (32000, 16000), (44100, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (44099, 16000),
          (44100, 16001), (192000, 16000)]
# every ratio from 1/64 to 64 must work: the two ends (64 : 1 stages 78 KB of LDS per tile, past the 64 KiB a launch gets
# without asking, and walks 3254 taps per output)
ENDS = [(1024000, 16000), (250, 16000)]


def noise(seed, *shape, dc=0.0):
    x = np.clip(np.random.RandomState(seed).standard_normal(shape) * 0.3, -1, 1) + dc
    return torch.from_numpy(x.astype(np.float32))


def up_down(ri, ro):
    g = math.gcd(ri, ro)
    return ro // g, ri // g


def n_out_of(n, ri, ro):
    up, down = up_down(ri, ro)
    return -((-n * up) // down)


def n_in_for(outputs, ri, ro, odd=False):
    """smallest n_in with at least `outputs` outputs; odd: and no multiple of `down`"""
    up, down = up_down(ri, ro)
    n = (outputs - 1) * down // up + 1
    assert n_out_of(n, ri, ro) >= outputs > n_out_of(n - 1, ri, ro)
    if odd and down > 1 and n % down == 0:
        n += 1
    return n


def lengths(ri, ro):
    return [1, 7, n_in_for(TILE, ri, ro), n_in_for(TILE + 1, ri, ro), n_in_for(3 * TILE + 37, ri, ro, odd=True)]


def front(w, ri, ro, flags=0, zeros=24, rolloff=0.945):
    """float_aud_front on a (C, N) device tensor whose rows are contiguous (a view is passed as it is) -> (n_out,) on the host"""
    assert w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and (w.shape[1] == 1 or w.stride(1) == 1)
    L = pkg.native.lib()
    n_in = int(w.shape[1])
    n_out = int(L.float_aud_front_len(n_in, ri, ro))
    need = int(L.float_aud_front_work_bytes(n_in, ri, ro))
    a = torch.full((n_out,), float("nan"), device=w.device)
    work = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=w.device)  # no zeroing needed
    pkg.native.check(L.float_aud_front(C.c_void_p(w.data_ptr()), int(w.shape[0]), int(w.stride(0)) if w.shape[0] > 1 else n_in, n_in, ri, ro,
                                       zeros, rolloff, flags, C.c_void_p(a.data_ptr()), n_out, C.c_void_p(work.data_ptr()),
                                       need, pkg.native.stream_ptr(w.device)))
    return a.cpu()


@functools.lru_cache(maxsize=None)
def yard(ri, ro, n, seed):
    """(input (n,), ref fp64, e_host) of one case; computed once, shared, never modified"""
    x = noise(seed, n)
    ref = hm.resample_sinc_direct(x.double(), ri, ro)
    hr = (44100, 16000) if (ri, ro) in ((44099, 16000), (44100, 16001)) else (ri, ro)
    href = ref if hr == (ri, ro) else hm.resample_sinc_direct(x.double(), *hr)
    e_host = float((hm.resample_sinc(x, *hr).double() - href).abs().max())
    return x, ref, e_host


def held(tag, got, ref, e_host):
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), tag
    e_dev = float((got.double() - ref).abs().max())
    print("%s: e_host %.3g e_dev %.3g e_dev/e_host %.2f" % (tag, e_host, e_dev, e_dev / max(e_host, 1e-300)))
    assert e_dev <= 4 * e_host, tag
    return e_dev


@pytest.mark.parametrize("ri,ro", RATIOS + ENDS)
def test_resample_against_the_closed_form(ri, ro):
    for i, n in enumerate(lengths(ri, ro)):
        x, ref, e_host = yard(ri, ro, n, 1000 + i)
        assert ref.shape[0] == n_out_of(n, ri, ro)
        held("%d -> %d n_in %d n_out %d" % (ri, ro, n, ref.shape[0]), front(x[None].cuda(), ri, ro), ref, e_host)


def test_tile_lengths_are_what_they_claim():
    """no GPU work: the derived lengths hit one tile exactly, pass it, and leave a remainder"""
    for ri, ro in RATIOS + ENDS:
        up, down = up_down(ri, ro)
        one, plus, three = lengths(ri, ro)[2:]
        assert n_out_of(one, ri, ro) == TILE and TILE < n_out_of(plus, ri, ro) <= TILE + max(1, -(-up // down))
        assert n_out_of(three, ri, ro) // TILE == 3 and n_out_of(three, ri, ro) % TILE and (down == 1 or three % down)


def seq_mean(w):
    """the operator's mono mix: the channels added in order, divided by their number, in fp32"""
    m = w[0].clone()
    for c in range(1, w.shape[0]):
        m = m + w[c]
    return m / float(w.shape[0])


@pytest.mark.parametrize("channels", [2, 6])
def test_channels_match_the_mono_call_on_the_host_side_mean(channels):
    ri, ro = 44100, 16000
    n = lengths(ri, ro)[-1]
    w = noise(77 + channels, channels, n)
    mono = front(seq_mean(w)[None].cuda(), ri, ro)
    assert torch.equal(front(w.cuda(), ri, ro), mono)
    if channels == 2:
        assert torch.equal(seq_mean(w), w.mean(dim=0))  # what preprocess_audio mixes on the host


def test_a_time_slice_needs_no_copy():
    ri, ro = 44100, 16000
    n = lengths(ri, ro)[-1]
    big = noise(81, 2, n + 11).cuda()
    view = big[:, 3:3 + n]  # ch_stride n + 11 > n_in, an odd element offset
    assert view.data_ptr() == big.data_ptr() + 12 and view.stride(0) == n + 11
    assert torch.equal(front(view, ri, ro), front(view.contiguous(), ri, ro))
    # and through the Python entry point, which passes the view as it is
    got = pkg.audio.preprocess_audio_device(view, ri, ro, device="cuda:0", normalize=False)
    assert tuple(got.shape) == (1, n_out_of(n, ri, ro)) and torch.equal(got[0].cpu(), front(view, ri, ro))


def test_long_clip_crosses_2_to_the_31():
    """320 s of 44.1 kHz: m * down passes 2^31 at output 4 869 624 of 5 120 000.  1000 seeded indices and the last 100 against
    the closed form evaluated per index; the yardstick is the 44100 -> 16000 case above (same filter, same input statistics)."""
    ri, ro, n = 44100, 16000, 14112000
    up, down = up_down(ri, ro)
    x = torch.from_numpy(np.clip(np.random.RandomState(320).standard_normal(n).astype(np.float32) * np.float32(0.3), -1, 1))
    got = front(x[None].cuda(), ri, ro)
    n_out = n_out_of(n, ri, ro)
    assert got.shape[0] == n_out == 5120000 and (n_out - 1) * down > 2 ** 31
    idx = np.unique(np.concatenate([np.random.RandomState(321).randint(0, n_out, 1000), np.arange(n_out - 100, n_out),
                                    np.arange(4869618, 4869630)])).astype(np.int64)
    c = 0.945 * min(1.0, up / down)
    Wt = int(math.ceil(24 / c))
    k = np.arange(-Wt, Wt + 2, dtype=np.int64)
    q, r = (idx * down) // up, (idx * down) % up
    j = q[:, None] + k[None, :]
    t = np.clip((k[None, :] * up - r[:, None]).astype(np.float64) / up * c, -24, 24)
    ker = np.sinc(t) * np.cos(np.pi * t / 48) ** 2 * c
    xs = np.where((j >= 0) & (j < n), x.numpy().astype(np.float64)[np.clip(j, 0, n - 1)], 0.0)
    ref = torch.from_numpy((xs * ker).sum(axis=1))
    _, _, e_host = yard(ri, ro, lengths(ri, ro)[-1], 1004)
    held("long clip, %d indices" % len(idx), got[torch.from_numpy(idx)], ref, e_host)


@pytest.mark.parametrize("channels,n", [(1, 1), (1, 3 * TILE + 37), (2, 3 * TILE + 37), (6, TILE + 1)])
def test_equal_rates_give_the_mono_mix_bitwise(channels, n):
    w = noise(90 + channels, channels, n)
    assert torch.equal(front(w.cuda(), 16000, 16000), seq_mean(w))


def norm_bound(tag, got, y):
    """got against (y - mean) / sqrt(var + 1e-7) in fp64: |err| <= 2^-22 ((|y| + |mu|) / sigma + |out|), two fp32 roundings
    with fp64 statistics"""
    yd = y.double()
    mu, var = yd.mean(), yd.var(unbiased=False)
    sd = torch.sqrt(var + 1e-7)
    want = (yd - mu) / sd
    err = (got.double() - want).abs()
    bound = 2.0 ** -22 * ((yd.abs() + mu.abs()) / sd + want.abs())
    print("%s: max |err| %.3g, max err / bound %.3g" % (tag, float(err.max()), float((err / bound).max())))
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), tag


@pytest.mark.parametrize("channels,n", [(1, 100), (1, 40 * TILE + 13), (2, 40 * TILE + 13)])
def test_normalisation_at_equal_rates(channels, n):
    w = noise(95 + channels, channels, n, dc=0.5)
    norm_bound("%d ch, n %d" % (channels, n), front(w.cuda(), 16000, 16000, flags=1), seq_mean(w))


@pytest.mark.parametrize("value,n", [(0.25, 1000), (0.3, 5 * TILE + 1), (-1.0, 1), (0.0, 77)])
def test_a_constant_input_gives_zeros(value, n):
    got = front(torch.full((1, n), value).cuda(), 16000, 16000, flags=1)
    assert bool(torch.isfinite(got).all()) and int(torch.count_nonzero(got)) == 0


def test_normalisation_after_a_resample_and_repeatability():
    ri, ro = 44100, 16000
    w = noise(99, 2, 44100, dc=0.1).cuda()  # 63 tiles
    y = front(w, ri, ro)
    a1, a2 = front(w, ri, ro, flags=1), front(w, ri, ro, flags=1)
    assert torch.equal(a1, a2)  # partials folded in a fixed order: bitwise repeatable
    norm_bound("44100 -> 16000 stereo", a1, y)
    got = pkg.audio.preprocess_audio_device(w.cpu(), ri, ro, device="cuda:0")  # from the host, normalised by default
    assert got.is_cuda and tuple(got.shape) == (1, 16000) and torch.equal(got[0].cpu(), a1)


# ---------------------------------------------------------------------------------------------------------------------------
# through the agent
# ---------------------------------------------------------------------------------------------------------------------------
def _agent():
    """The synthetic 64-px agent of tests/test_dec_u8_gpu.py; 2 s of 48 kHz stereo (tone + noise, the two channels differ)."""
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.input_size, opt.nfe = 64, 6
    cfg = pkg.config.FmtConfig.from_options(opt)
    acfg = pkg.config.small_audio_config()
    acfg.dim_w = opt.dim_w
    parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
                 audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
    img = torch.from_numpy(np.random.RandomState(5).rand(1, 64, 64, 3).astype(np.float32))
    n = 96000
    tone = 0.3 * np.sin(2 * np.pi * 220.0 * np.arange(n) / 48000.0)
    wav = np.stack([tone + 0.1 * np.random.RandomState(s).standard_normal(n) for s in (9, 10)]).astype(np.float32)
    return gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8), img, torch.from_numpy(wav)[None]


def test_through_the_agent(monkeypatch):
    for v in ("FLOAT_AMD_VERIFY", "FLOAT_AMD_VERIFY_ACTION", "FLOAT_AMD_OVERLAP", "FLOAT_AMD_AUDIO_FRONT"):
        monkeypatch.delenv(v, raising=False)
    agent, img, wav = _agent()
    audio = {"waveform": wav, "sample_rate": 48000}
    parent = hm.preprocess_audio(wav[0], 48000, 16000, device=agent.rank).cpu()  # the parent's host route
    s, a = agent.host_inputs(img, audio)
    assert a.is_cuda and a.shape == parent.shape == (1, 32000)
    # the yardstick after un-normalising both with the statistics of the fp64 closed form
    ref = hm.resample_sinc_direct(wav[0].mean(dim=0).double(), 48000, 16000)
    mu, sd = ref.mean(), torch.sqrt(ref.var(unbiased=False) + 1e-7)
    e_host = float((parent[0].double() * sd + mu - ref).abs().max())
    held("host_inputs, 48 kHz stereo", (a[0].cpu().double() * sd + mu), ref, e_host)
    frames_on = agent.run_inference(None, img, audio, emo="happy", no_crop=True, seed=7).clone()
    monkeypatch.setenv("FLOAT_AMD_AUDIO_FRONT", "0")  # read at the call
    s0, a0 = agent.host_inputs(img, audio)
    assert torch.equal(a0.cpu(), parent) and torch.equal(s0, s)
    frames_off = agent.run_inference(None, img, audio, emo="happy", no_crop=True, seed=7).clone()
    monkeypatch.delenv("FLOAT_AMD_AUDIO_FRONT")
    assert frames_on.shape == frames_off.shape == (50, 64, 64, 3)
    mse = float(((frames_on.double() - frames_off.double()) ** 2).mean())
    psnr = 10 * math.log10(1.0 / max(mse, 1e-30))
    print("run_inference, device front end against the host resampler: %.1f dB" % psnr)
    assert psnr >= 45.0  # two routes to the same clip
    # at the model's rate nothing changes
    wav16 = wav[:, :, :32000]
    _, a16 = agent.host_inputs(img, {"waveform": wav16, "sample_rate": 16000})
    assert torch.equal(a16.cpu(), hm.preprocess_audio(wav16[0], 16000, 16000, device=agent.rank).cpu())
