"""The audio operator's two attention kernels (csrc/aud_kernels.hpp) on their own, through the test hook float_aud_debug
(AudioEncoderHIP.attention_probe), against a float64 softmax of the same rounded inputs - at the tile edges.  The launch is the
one inference_impl makes for the handle (one helper): aud_attn_mfma_kernel for fp16 / bf16, aud_attn_kernel (one wave per query,
2048-key tiles) for fp32 handles and under FLOAT_AUD_ATTN_MFMA=0.

Inputs are peaked (tests/util.py::peaked_qkv): one key of logit 24 planted on a query for every edge of a 16-key sub-tile, a
64-key tile and the 2048-key tile, and for the last keys of the clip - so a lost key, a wrong scale or a missing rescale of the
online softmax costs whole value rows, not a ten-thousandth of an average (tests/test_aud_attn.py shows that on a model).

Limits (tests/util.py::ATTN_LIMITS, derived from the number formats, not measured): 16-bit routes max|d| <= 2^-10 max|v| (fp16),
2^-7 max|v| (bf16), rel-L2 <= 2^-11 / 2^-8; the one-wave route keeps P in fp32 and meets the same.  fp32: max(4 * e32, 1e-6 max|v|)
with e32 = the error of the same formula evaluated by torch in fp32 (the factor 4: __expf and another summation order)."""
import pytest
import torch

from tests.util import ATTN_LIMITS, AUD_ATTN_CASES, aud_attn_case, load_pkg, max_abs, qkv_rows, rel_l2

pkg = load_pkg()
W, C = pkg.weights, pkg.config
pytestmark = pytest.mark.gpu

ROUTES = [("fp16", "mfma"), ("bf16", "mfma"), ("fp16", "wave"), ("bf16", "wave"), ("fp32", "wave")]
_STATE, _HANDLES = {}, {}


def _cfg(heads):
    # 4 heads: the small test shape; 12 heads: hidden 768 of wav2vec2-base (pack stride D / 32 = 24) with one layer
    return C.small_audio_config() if heads == 4 else C.AudioConfig(num_hidden_layers=1)


def _new_handle(heads, dtype, route, monkeypatch):
    """The switch is read when the handle is created (csrc/tuning.hpp): set it first."""
    if route == "wave" and dtype != "fp32":
        monkeypatch.setenv("FLOAT_AUD_ATTN_MFMA", "0")
    else:
        monkeypatch.delenv("FLOAT_AUD_ATTN_MFMA", raising=False)
    if heads not in _STATE:
        _STATE[heads] = W.synth_audio_state(_cfg(heads), seed=60 + heads)
    return pkg.audio.AudioEncoderHIP(_STATE[heads], _cfg(heads), "cuda:0", dtype)


def _handle(heads, dtype, route, monkeypatch):
    """One handle per (config, dtype, route), shared by the cases."""
    key = (heads, dtype, route)
    if key not in _HANDLES:
        _HANDLES[key] = _new_handle(heads, dtype, route, monkeypatch)
    return _HANDLES[key]


def _rows(c):
    return qkv_rows(c["q"], c["k"], c["v"])


@pytest.mark.parametrize("dtype,route", ROUTES, ids=["%s-%s" % r for r in ROUTES])
@pytest.mark.parametrize("Tn,heads", AUD_ATTN_CASES)
def test_attention_kernels_against_fp64(Tn, heads, dtype, route, monkeypatch):
    """Measured on one MI355X, the kernel's max|d| as a fraction of its limit over the shapes from 17 frames up (one frame is exact
    on every route): matrix pipe 0.22-0.28 (fp16) and 0.21-0.33 (bf16), rel-L2 0.38-0.44 of its limit; one wave per query 0.20-0.28
    and 0.20-0.33, rel-L2 0.36-0.42.  fp32: the kernel's max|d| is 2.5e-6 ... 7.6e-6 beside e32 = 2.7e-6 ... 8.0e-6 (0.22-0.26 of
    the limit), rel-L2 2.6e-7 ... 9.9e-7; every case prints its own figures."""
    c = aud_attn_case(Tn, heads, dtype)
    enc = _handle(heads, dtype, route, monkeypatch)
    got = enc.attention_probe(_rows(c))
    again = enc.attention_probe(_rows(c))
    out = got.cpu()
    d, r = max_abs(out, c["ref"]), rel_l2(out, c["ref"])
    if dtype == "fp32":
        lim = max(4 * c["e32"], 1e-6 * c["vmax"])
        print("Tn %d fp32 one-wave: kernel max|d| %.3e, e32 %.3e, limit %.3e (%.2f of it), rel-L2 %.3e" % (Tn, d, c["e32"], lim, d / lim, r))
        assert d <= lim
    else:
        lim_abs, lim_rel = ATTN_LIMITS[dtype][0] * c["vmax"], ATTN_LIMITS[dtype][1]
        print("Tn %d %s %s: max|d| %.3e = %.2f of the limit, rel-L2 %.3e = %.2f of the limit" % (Tn, dtype, route, d, d / lim_abs, r, r / lim_rel))
        assert d <= lim_abs and r <= lim_rel
    assert out.shape == (Tn, heads * 64) and bool(torch.isfinite(out).all())
    assert enc.saturation() == 0
    assert torch.equal(got, again)


@pytest.mark.parametrize("dtype,route", ROUTES, ids=["%s-%s" % r for r in ROUTES])
def test_rows_left_by_a_longer_call_are_not_read(dtype, route, monkeypatch):
    """2120 frames and then 65 on one handle = 65 frames on a new handle, bit for bit: the clamped loads of the last tile and
    the key bound stop at Tn, not at what the workspace holds."""
    long_c, short_c = aud_attn_case(2120, 4, dtype), aud_attn_case(65, 4, dtype)
    used = _new_handle(4, dtype, route, monkeypatch)
    used.attention_probe(_rows(long_c))
    after = used.attention_probe(_rows(short_c))
    fresh = _new_handle(4, dtype, route, monkeypatch).attention_probe(_rows(short_c))
    assert torch.equal(after, fresh)


def test_argument_errors_and_the_emotion_handle(monkeypatch):
    N, L = pkg.native, pkg.native.lib()
    enc = _new_handle(4, "fp16", "mfma", monkeypatch)
    with pytest.raises(ValueError):
        enc.attention_probe(torch.zeros(5, 3 * 256 + 1))
    with pytest.raises(ValueError):
        enc.attention_probe(torch.zeros(0, 3 * 256))
    with pytest.raises(ValueError):
        enc.attention_probe(torch.zeros(3 * 256))
    x, out, st = torch.zeros(96, 3 * 256, device="cuda:0"), torch.zeros(96, 256, device="cuda:0"), N.stream_ptr("cuda:0")
    # the hook itself does not allocate: nothing reserved yet, then 65 frames reserved and 96 asked for
    assert L.float_aud_debug(enc._h, 1, N.dev_ptr(x), 65, N.dev_ptr(out), st) == 1 and b"float_aud_reserve" in L.float_last_error()
    enc.reserve(400, 65)
    rc = L.float_aud_debug(enc._h, 1, N.dev_ptr(x), 96, N.dev_ptr(out), st)
    assert rc == 1 and b"float_aud_reserve" in L.float_last_error()
    with pytest.raises(ValueError, match="float_aud_reserve"):
        N.check(rc)
    assert L.float_aud_debug(enc._h, 1, N.dev_ptr(x), 0, N.dev_ptr(out), st) == 1 and b"Tn" in L.float_last_error()
    assert L.float_aud_debug(enc._h, 7, N.dev_ptr(x), 65, N.dev_ptr(out), st) == 1 and b"unknown request" in L.float_last_error()
    assert L.float_aud_debug(enc._h, 1, None, 65, N.dev_ptr(out), st) == 1 and L.float_aud_debug(enc._h, 1, N.dev_ptr(x), 65, None, st) == 1
    N.check(L.float_aud_debug(enc._h, 1, N.dev_ptr(x), 65, N.dev_ptr(out), st))
    # Audio2EmotionHIP inherits the probe: the same kernel on the same shape, the same bits
    c = aud_attn_case(65, 4, "fp16")
    ecfg = C.small_emotion_config()
    ser = pkg.audio.Audio2EmotionHIP(W.synth_audio_state(ecfg, seed=61), ecfg, "cuda:0", "fp16")
    assert torch.equal(ser.attention_probe(_rows(c)), enc.attention_probe(_rows(c)))
