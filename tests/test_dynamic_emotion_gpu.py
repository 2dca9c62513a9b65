"""Dynamic emotion on the GPU: float_aud_classify_segments (all equal chunks of a clip through one stacked speech-emotion pass),
float_aud_expand_rows, Audio2EmotionHIP.predict_emotion_chunks, the agent's emo="dynamic" and the dynamic-emotion node.

Reference: the CPU oracle (O.audio2emotion_predict) on every piece normalised in fp64 on the host.  A segment is a clip, so the
limits are the operator's own from tests/test_aud_gpu.py: max |d| < 2e-3 fp16 (test_speech_emotion_live_oracle_ragged), 1e-2
bf16, 2e-6 fp32 (test_speech_emotion_golden).  Segment lengths: 24 000 samples = 74 frames (more than one 64-query / 64-key tile
of the matrix-pipe attention, no multiple of 4 or 16: LayerNorm and positional-conv workgroups straddle two segments), 32 000 =
99 frames (the product's chunk; 4 x 99 rows = more than three 128-row GEMM tiles, seams inside tiles), 4 000 = 12 frames (both
edges of a segment inside the 16-tap positional kernel of the small config)."""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import float_oracle as O
from tests.util import load_pkg

pkg = load_pkg()
W, CFG, HM, N = pkg.weights, pkg.config, pkg.host_models, pkg.native
pytestmark = pytest.mark.gpu

LIMIT = {"fp16": 2e-3, "bf16": 1e-2, "fp32": 2e-6}
SEED = 51
_state = {}


def _cfg():
    return CFG.small_emotion_config()


@functools.lru_cache(None)
def _sd():
    return W.synth_audio_state(_cfg(), seed=SEED)


@functools.lru_cache(None)
def _ser(dtype):
    return pkg.audio.Audio2EmotionHIP(_sd(), _cfg(), "cuda:0", dtype)


@functools.lru_cache(None)
def _piece(seg_len, k):
    """Piece k of seg_len samples: a synthetic waveform of its own seed, scaled and offset so that normalisation matters."""
    w = W.synth_waveform(seg_len / 16000.0, seed=60 + k)[0, :seg_len]
    assert w.shape[0] == seg_len
    return w * (0.05 + 0.4 * k) + (0.3 * k - 0.5)


def _norm64(x):
    xd = x.double()
    return ((xd - xd.mean()) / torch.sqrt(xd.var(unbiased=False) + 1e-7)).float()


@functools.lru_cache(None)
def _oracle_piece(seg_len, k):
    """The reference scores of piece k, computed once and left unchanged."""
    return O.audio2emotion_predict(_sd(), _cfg(), _norm64(_piece(seg_len, k))[None])[0]


def _oracle_of(x):
    return O.audio2emotion_predict(_sd(), _cfg(), _norm64(x)[None])[0]


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("seg_len", [4000, 24000, 32000])
@pytest.mark.parametrize("n_seg", [1, 3, 4])
def test_segments_match_the_oracle_per_segment(n_seg, seg_len, dtype):
    ser = _ser(dtype)
    a = torch.cat([_piece(seg_len, k) for k in range(n_seg)]).cuda()
    scores, _ = ser.classify_segments(a, n_seg, seg_len)
    scores = scores.cpu()
    ref = torch.stack([_oracle_piece(seg_len, k) for k in range(n_seg)])
    d = float((scores - ref).abs().max())
    print("n_seg %d seg_len %d %s: stacked max|d| %.3e" % (n_seg, seg_len, dtype, d))
    if dtype == "fp32" and not d < LIMIT[dtype]:
        # the live oracle is no golden: the single-clip call on the same pieces against the same oracle, and twice its figure
        # for the summation order of another tiling
        one = torch.cat([ser.predict_emotion(_norm64(_piece(seg_len, k))[None]) for k in range(n_seg)]).cpu()
        d1 = float((one - ref).abs().max())
        print("   fp32 single-clip max|d| %.3e -> limit %.3e" % (d1, 2 * d1))
        assert d <= 2 * d1
    else:
        assert d < LIMIT[dtype]
    assert scores.shape == (n_seg, 7) and float((scores.sum(-1) - 1).abs().max()) < 1e-5
    assert ser.saturation() == 0
    assert torch.equal(ser.classify_segments(a, n_seg, seg_len)[0].cpu(), scores)  # bitwise repeatable


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("seg_len", [24000, 4000])
def test_no_leak_across_segment_seams(seg_len, dtype):
    """[A, B, C] against [A, X, C], X loud and different: rows 0 and 2 do not move by a bit."""
    ser = _ser(dtype)
    A, B, Cc = (_piece(seg_len, k) for k in range(3))
    X = W.synth_waveform(seg_len / 16000.0, seed=99)[0, :seg_len] * 30.0
    for normalize in (True, False):
        s1 = ser.classify_segments(torch.cat([A, B, Cc]).cuda(), 3, seg_len, normalize=normalize)[0].cpu()
        s2 = ser.classify_segments(torch.cat([A, X, Cc]).cuda(), 3, seg_len, normalize=normalize)[0].cpu()
        assert torch.equal(s1[0], s2[0]) and torch.equal(s1[2], s2[2]), (normalize, s1, s2)
        assert not torch.equal(s1[1], s2[1])


@pytest.mark.parametrize("seg_len", [4000, 24000])
def test_segment_normalisation(seg_len):
    """The workspace copy (float_aud_debug, what = 2) against the fp64 closed form by the bound tests/test_aud_front_gpu.py
    derives for float_aud_front's normalisation, |err| <= 2^-22 ((|y| + |mu|) / sigma + |out|); the caller's samples are not
    written; a strided layout with poison in the gaps gives the packed layout's scores."""
    ser, n_seg = _ser("fp16"), 4
    pieces = [_piece(seg_len, k) for k in range(n_seg)]
    a = torch.cat(pieces).cuda()
    keep = a.clone()
    scores = ser.classify_segments(a, n_seg, seg_len)[0]
    got = ser.segment_normalised(n_seg * seg_len).cpu().reshape(n_seg, seg_len)
    assert torch.equal(a, keep)
    for k, y in enumerate(pieces):
        yd = y.double()
        mu, sd = yd.mean(), torch.sqrt(yd.var(unbiased=False) + 1e-7)
        want = (yd - mu) / sd
        err = (got[k].double() - want).abs()
        bound = 2.0 ** -22 * ((yd.abs() + mu.abs()) / sd + want.abs())
        print("seg_len %d piece %d: max |err| %.3g, max err / bound %.3g" % (seg_len, k, float(err.max()), float((err / bound).max())))
        assert bool(torch.isfinite(got[k]).all()) and bool((err <= bound).all()), k
    stride = seg_len + 37
    gap = torch.full((n_seg, stride), 1e30)
    gap[:, :seg_len] = torch.stack(pieces)
    b = gap.reshape(-1).cuda()
    keep_b = b.clone()
    strided = ser.classify_segments(b, n_seg, seg_len, seg_stride=stride)[0]
    assert torch.equal(strided, scores) and torch.equal(b, keep_b)
    assert ser.saturation() == 0


def test_chunks_tail_and_expansion():
    """predict_emotion_chunks: two stacked chunks + a 0.61-s tail, and a clip whose tail is 250 samples (replicate pad); the
    rows against the oracle, the frames bitwise host_models.nearest_rows(seq, T); a second call is bitwise the first."""
    ser, chunk = _ser("fp16"), 32000
    for tail in (9760, 250):
        w = torch.cat([_piece(chunk, 0), _piece(chunk, 1), _piece(tail, 2)])
        for T in (66, 82, 116):
            seq, frames = ser.predict_emotion_chunks(w, chunk, T)
            assert seq.is_cuda and frames.is_cuda and seq.shape == (3, 7) and frames.shape == (T, 7)
            assert torch.equal(frames.cpu(), HM.nearest_rows(seq.cpu(), T)), (tail, T)
            seq2, frames2 = ser.predict_emotion_chunks(w[None].cuda(), chunk, T)
            assert torch.equal(seq, seq2) and torch.equal(frames, frames2)
        last = _norm64(_piece(tail, 2))
        if tail < 400:
            last = torch.nn.functional.pad(last[None, None], (0, 400 - tail), mode="replicate")[0, 0]
        ref = torch.stack([_oracle_piece(chunk, 0), _oracle_piece(chunk, 1), O.audio2emotion_predict(_sd(), _cfg(), last[None])[0]])
        d = float((seq.cpu() - ref).abs().max())
        print("tail %d: seq max|d| %.3e" % (tail, d))
        assert d < LIMIT["fp16"]
    # no tail: the stacked call expands its own rows; a clip shorter than one chunk: one row, repeated
    seq, frames = ser.predict_emotion_chunks(torch.cat([_piece(chunk, 0), _piece(chunk, 1)]), chunk, 82)
    assert torch.equal(frames.cpu(), HM.nearest_rows(seq.cpu(), 82)) and torch.equal(seq.cpu(), ser.classify_segments(
        torch.cat([_piece(chunk, 0), _piece(chunk, 1)]).cuda(), 2, chunk)[0].cpu())
    seq, frames = ser.predict_emotion_chunks(_piece(4000, 1), chunk, 7)
    assert seq.shape == (1, 7) and torch.equal(frames, seq.repeat(7, 1))
    assert float((seq.cpu()[0] - _oracle_piece(4000, 1)).abs().max()) < LIMIT["fp16"]
    assert ser.predict_emotion_chunks(_piece(4000, 1), chunk)[1] is None
    assert ser.saturation() == 0


def test_segment_calls_do_not_allocate_and_refuse():
    """Beyond the reservation: FLOAT_E_INVALID naming float_aud_reserve_segments; and the refusals that need a handle."""
    L = N.lib()
    ser = pkg.audio.Audio2EmotionHIP(_sd(), _cfg(), "cuda:0", "fp16")
    a = torch.cat([_piece(24000, k) for k in range(3)]).cuda()
    out = torch.empty(3, 7, device="cuda:0")
    st = N.stream_ptr("cuda:0")
    call = lambda n: L.float_aud_classify_segments(ser._h, N.dev_ptr(a), n, 24000, 24000, 1, N.dev_ptr(out), None, 0, 0.0, st)  # noqa: E731
    assert call(3) == 1 and b"float_aud_reserve_segments" in L.float_last_error()
    N.check(L.float_aud_reserve_segments(ser._h, 2, 24000, st))
    assert call(2) == 0
    assert call(3) == 1 and b"float_aud_reserve_segments" in L.float_last_error()
    N.check(L.float_aud_reserve_segments(ser._h, 3, 24000, st))
    assert call(3) == 0
    assert torch.equal(out, ser.classify_segments(a, 3, 24000)[0])
    assert torch.equal(ser.predict_emotion(_norm64(_piece(24000, 0))[None].cuda()), ser.predict_emotion(_norm64(_piece(24000, 0))[None].cuda()))
    # a segment below the receptive field; more frames than one call takes (refused before anything is allocated)
    assert L.float_aud_reserve_segments(ser._h, 2, 399, st) == 1 and b"too short" in L.float_last_error()
    assert L.float_aud_classify_segments(ser._h, N.dev_ptr(a), 2, 399, 399, 1, N.dev_ptr(out), None, 0, 0.0, st) == 1
    assert L.float_aud_reserve_segments(ser._h, 201, 320080, st) == 1 and b"200000" in L.float_last_error()
    # a handle with the audio projection head (and a GroupNorm extractor)
    acfg = CFG.small_audio_config()
    enc = pkg.audio.AudioEncoderHIP(W.synth_audio_state(acfg, seed=3), acfg, "cuda:0", "fp16")
    assert L.float_aud_reserve_segments(enc._h, 2, 24000, st) == 1 and b"num_labels" in L.float_last_error()
    assert L.float_aud_classify_segments(enc._h, N.dev_ptr(a), 2, 24000, 24000, 1, N.dev_ptr(out), None, 0, 0.0, st) == 1
    # a classification handle with the GroupNorm extractor
    gcfg = _cfg()
    gcfg.feat_extract_norm, gcfg.conv_bias = "group", False
    grp = pkg.audio.Audio2EmotionHIP(W.synth_audio_state(gcfg, seed=4), gcfg, "cuda:0", "fp16")
    assert L.float_aud_reserve_segments(grp._h, 2, 24000, st) == 1 and b"group" in L.float_last_error()


def test_group_norm_handle_goes_chunk_by_chunk():
    """A GroupNorm speech-emotion checkpoint (feat_extract_norm = "group", what a wav2vec2-base-derived folder gives): the
    stacked call refuses it, predict_emotion_chunks and the node score it chunk by chunk on the device - every row the
    single-clip call's bytes for that chunk, within the operator's limit of the oracle, frames bitwise nearest_rows."""
    gcfg = _cfg()
    gcfg.feat_extract_norm, gcfg.conv_bias = "group", False
    gsd = W.synth_audio_state(gcfg, seed=4)
    grp = pkg.audio.Audio2EmotionHIP(gsd, gcfg, "cuda:0", "fp16")
    with pytest.raises(ValueError, match="group"):
        grp.classify_segments(_piece(24000, 0).cuda(), 1, 24000)
    chunk = 8000
    w = torch.cat([_piece(chunk, 0), _piece(chunk, 1), _piece(chunk, 2), _piece(250, 3)])  # three chunks and a 250-sample tail
    seq, frames = grp.predict_emotion_chunks(w, chunk, 41)
    assert seq.is_cuda and seq.shape == (4, 7) and torch.equal(frames.cpu(), HM.nearest_rows(seq.cpu(), 41))
    for i in range(4):
        piece = w[i * chunk:(i + 1) * chunk]
        dev = pkg.audio.preprocess_audio_device(piece, 16000, 16000, "cuda:0", True)
        ref = _norm64(piece)
        if piece.shape[0] < 400:
            dev = torch.nn.functional.pad(dev[None], (0, 400 - piece.shape[0]), mode="replicate")[0]
            ref = torch.nn.functional.pad(ref[None, None], (0, 400 - piece.shape[0]), mode="replicate")[0, 0]
        assert torch.equal(seq[i], grp.predict_emotion(dev)[0]), i
        d = float((seq[i].cpu() - O.audio2emotion_predict(gsd, gcfg, ref[None])[0]).abs().max())
        assert d < LIMIT["fp16"], (i, d)
    assert torch.equal(seq, grp.predict_emotion_chunks(w, chunk)[0]) and grp.saturation() == 0
    nodes = importlib.import_module(pkg.__name__ + ".src.nodes.nodes_vadv")
    pipe = (grp, None, {"num_labels": 7, "sampling_rate": 16000})
    we, _, nseq = nodes.FloatExtractEmotionWithCustomModelDyn().extract_dynamic_emotion({"waveform": w[None, None], "sample_rate": 16000}, pipe, 25.0, 0.5)
    assert torch.equal(nseq[0], seq.cpu()) and we.shape == (1, math.ceil(24250 / 16000 * 25.0), 7)


def test_chunks_below_the_receptive_field_are_padded():
    """Chunks under 400 samples: every one replicate-padded to 400 after its normalisation, as the reference's loop does."""
    ser, chunk = _ser("fp16"), 300
    w = _piece(1000, 1)  # 300 + 300 + 300 + 100
    seq, frames = ser.predict_emotion_chunks(w, chunk, 9)
    assert seq.shape == (4, 7) and torch.equal(frames.cpu(), HM.nearest_rows(seq.cpu(), 9))
    for i in range(4):
        piece = w[i * chunk:(i + 1) * chunk]
        ref = torch.nn.functional.pad(_norm64(piece)[None, None], (0, 400 - piece.shape[0]), mode="replicate")[0, 0]
        d = float((seq[i].cpu() - O.audio2emotion_predict(_sd(), _cfg(), ref[None])[0]).abs().max())
        assert d < LIMIT["fp16"], (i, d)


# ------------------------------------------------------------------------------------------ product route
def _agent():
    if "agent" not in _state:
        gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
        opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
        opt.input_size, opt.nfe = 64, 6
        cfg = CFG.FmtConfig.from_options(opt)
        acfg = CFG.small_audio_config()
        acfg.dim_w = opt.dim_w
        parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
                     audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
        _state["plain_parts"] = dict(parts)
        parts["emotion_encoder"] = (_sd(), _cfg())
        _state["gen"], _state["opt"] = gen, opt
        _state["agent"] = gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8)
        _state["img"] = torch.from_numpy(np.random.RandomState(5).rand(1, 3, 64, 64).astype(np.float32)).cuda() * 2 - 1
        _state["wav"] = W.synth_waveform(4.4, seed=10)[0].cuda()  # 110 frames: three windows; chunks of 2 s, 2 s and 0.4 s
    return _state["agent"]


def test_product_route_dynamic_emotion():
    agent = _agent()
    s, a = _state["img"], _state["wav"]
    T = math.ceil(a.shape[0] * 25 / 16000)
    c = agent.conditions_device(s, a, "dynamic")
    seq, frames = agent.emotion_encoder.predict_emotion_chunks(a, 32000, T)
    assert c["T"] == T == 110 and c["we"].shape == (1, T, 7) and seq.shape == (3, 7)
    assert torch.equal(c["we"][0], frames)
    ref = torch.stack([_oracle_of(a[:32000].cpu()), _oracle_of(a[32000:64000].cpu()), _oracle_of(a[64000:].cpu())])
    assert float((seq.cpu() - ref).abs().max()) < LIMIT["fp16"]
    c1 = agent.conditions_device(s, a, ("dynamic", 1.0))
    assert c1["we"].shape == (1, T, 7) and torch.equal(c1["we"][0], agent.emotion_encoder.predict_emotion_chunks(a, 16000, T)[1])
    assert len(torch.unique(c1["we"][0], dim=0)) == 5 and len(torch.unique(c["we"][0], dim=0)) == 3  # twice the chunks: 5 against 3
    got = agent.infer_device(s, a, a_cfg_scale=1.0, e_cfg_scale=3.0, emo="dynamic", seed=7).clone()
    assert got.shape == (T, 64, 64, 3) and bool(torch.isfinite(got).all())
    none = agent.infer_device(s, a, a_cfg_scale=1.0, e_cfg_scale=3.0, emo="none", seed=7).clone()
    assert not torch.equal(got, none)
    # by hand: the hot path with that `we` and the same noise
    c = agent.conditions_device(s, a, "dynamic")
    noise = agent._noise_to_device(agent.G.n_chunks(T), 7)
    hand = agent.G.generate_to_host(c["r_s"], c["wa"], c["we"], c["s_r"], None, agent.opt.nfe, 1.0, 1.0, 3.0, noise=noise)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(hand, got)
    agent.G.release_host_inflight()
    blocks = [(b.first, b.last, b.frames.clone()) for b in agent.stream_device(s, a, a_cfg_scale=1.0, e_cfg_scale=3.0, emo="dynamic", seed=7)]
    assert torch.equal(torch.cat([b[2] for b in blocks]), got)
    with pytest.raises(ValueError, match="dynamic"):
        agent.infer_device_batch([(s, a), (s, a)], emo=["dynamic", "happy"])
    both = agent.infer_device_batch([(s, a), (s, a[:40000])], a_cfg_scale=1.0, e_cfg_scale=3.0, emo="dynamic", seeds=[7, 8])
    assert both[0].shape == got.shape and both[1].shape[0] == 63 and all(bool(torch.isfinite(b).all()) for b in both)


def test_dynamic_emotion_needs_the_speech_emotion_weights():
    _agent()
    plain = _state["gen"].InferenceAgent(_state["opt"], _state["plain_parts"], "cuda:0", max_frames=8)
    with pytest.raises(NotImplementedError):
        plain.conditions_device(_state["img"], _state["wav"], "dynamic")
    with pytest.raises(NotImplementedError):
        plain.conditions_device(_state["img"], _state["wav"], "none")
    plain.offload()


def test_dynamic_emotion_node():
    """extract_dynamic_emotion on a 2-item batch of 4.4 s: CPU outputs, (2, T, 7) and (2, 3, 7), every chunk within the limit."""
    nodes = importlib.import_module(pkg.__name__ + ".src.nodes.nodes_vadv")
    ser = _ser("fp16")
    wav = torch.stack([W.synth_waveform(4.4, seed=20), W.synth_waveform(4.4, seed=21) * 0.2 + 0.1])  # (2, 1, 70400)
    pipe = (ser, None, {"num_labels": 7, "sampling_rate": 16000})
    we, pipe_out, seq = nodes.FloatExtractEmotionWithCustomModelDyn().extract_dynamic_emotion({"waveform": wav, "sample_rate": 16000}, pipe, 25.0, 2.0)
    assert pipe_out is pipe and not we.is_cuda and not seq.is_cuda
    T = math.ceil(70400 / 16000 * 25.0)  # the node's arithmetic (111: the quotient is not exact in binary)
    assert we.shape == (2, T, 7) and seq.shape == (2, 3, 7)
    assert torch.equal(we, HM.nearest_rows(seq, T))
    for b in range(2):
        for i in range(3):
            d = float((seq[b, i] - _oracle_of(wav[b, 0, i * 32000:(i + 1) * 32000])).abs().max())
            assert d < LIMIT["fp16"], (b, i, d)
