"""Ragged FMT jobs on the GPU (float_fmt_sample_batch_ragged, FlowMatchingTransformerHIP.sample_ragged): B clips of their own
lengths in one stacked chain, a clip leaving the stack after its last window.  Each clip is held to what the one-clip handle
gives for it alone at the bound tests/test_edge_cases_gpu.py::test_batched_sampling_equals_per_clip sets for stacked chains
(rel-L2 < 0.25 x the operand type's tolerance); where the launches are those of an existing path the comparison is bitwise."""
import importlib

import numpy as np
import pytest
import torch

from oracle import float_oracle as O
from tests.util import load_pkg, rel_l2

pkg = load_pkg()
pytestmark = pytest.mark.gpu
C, W = pkg.config, pkg.weights
CFG = C.FmtConfig()
TOL = {"fp16": 4e-3, "bf16": 2e-2}
NFE = 5
LADDER = [70, 20, 130, 70]  # caller order; windows 2 / 1 / 3 / 2, so the stack is 4 -> 3 -> 1 clips (720 -> 540 -> 180 rows)


def _clips(lengths, seed, dynamic=False, cfg=CFG):
    cs = [pkg.pipeline.synth_conditions(cfg, T, seed=seed + q, dynamic_we=dynamic) for q, T in enumerate(lengths)]
    noise = [pkg.fmt.draw_noise((T + cfg.num_frames_for_clip - 1) // cfg.num_frames_for_clip, 1, cfg, seed=15 + q)
             for q, T in enumerate(lengths)]
    return cs, noise


def _ragged(m, cs, noise, *scales, **kw):
    return m.sample_ragged(torch.cat([c["r_s"] for c in cs]), [c["wa"][0] for c in cs], [c["we"][0] for c in cs], noise, NFE,
                           *scales, **kw)


def _alone(one, c, nz, *scales, **kw):
    return one.sample(c["r_s"], c["wa"], c["we"], nz, NFE, *scales, **kw)[0]


_handles = {}


def _handle(dtype, max_batch=1, use_graph=2, seed=41):
    key = (dtype, max_batch, use_graph, seed)
    if key not in _handles:
        sd = W.synth_fmt_state(CFG, seed=seed)
        _handles[key] = pkg.fmt.FlowMatchingTransformerHIP(sd, CFG, "cuda:0", dtype, use_graph=use_graph, max_batch=max_batch)
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()
    _ladder_cache.clear()


_ladder_cache = {}


def _ladder(dtype, use_graph=2):
    """The ladder job on the 4-clip handle, written into slices of one NaN-filled buffer: (results, buffer, slices)."""
    key = (dtype, use_graph)
    if key not in _ladder_cache:
        many = _handle(dtype, 4, use_graph)
        cs, noise = _clips(LADDER, 50)
        pad = 3
        buf = torch.full((sum(LADDER) + pad * (len(LADDER) + 1), CFG.dim_w), float("nan"), device="cuda:0")
        spans, off = [], pad
        for T in LADDER:
            spans.append((off, off + T))
            off += T + pad
        out = [buf[a:b] for a, b in spans]
        got = _ragged(many, cs, noise, 2.0, 1.0, 1.0, out=out)
        torch.cuda.synchronize()
        _ladder_cache[key] = (got, buf, spans, cs, noise, many)
    return _ladder_cache[key]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_ladder_across_the_row_blocked_boundary(dtype):
    """Lengths 130 / 70 / 70 / 20 in shuffled caller order: 4 -> 3 -> 1 active clips, i.e. 720 and 540 rows on the row-blocked
    tile (fmt_gemm_rbs_kernel, from 300 rows) and 180 rows on fmt_gemm_kernel.  Every clip against the one-clip handle; the
    padded rows of a clip's last window (n_cur x windows - T) never reach r_d: the rows around each r_d[i] stay NaN."""
    got, buf, spans, cs, noise, many = _ladder(dtype)
    one = _handle(dtype)
    assert [tuple(g.shape) for g in got] == [(T, 512) for T in LADDER]
    inside = torch.zeros(buf.shape[0], dtype=torch.bool, device=buf.device)
    for a, b in spans:
        inside[a:b] = True
    assert torch.isfinite(buf[inside]).all() and torch.isnan(buf[~inside]).all()
    for q, T in enumerate(LADDER):
        alone = _alone(one, cs[q], noise[q], 2.0, 1.0, 1.0)
        err = rel_l2(got[q], alone)
        print("%s clip %d (T = %d): rel-L2 %.3e vs the one-clip chain" % (dtype, q, T, err))
        assert err < 0.25 * TOL[dtype], (q, err)
    again = _ragged(many, cs, noise, 2.0, 1.0, 1.0)  # fixed summation order: bitwise run to run
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    assert many.saturation() == 0


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_equal_lengths_are_the_uniform_call(dtype):
    """B = 3, T = 70: the slot order is the caller's and the chain launches are those of float_fmt_sample_batch - bitwise."""
    many = _handle(dtype, 4)
    cs, noise = _clips([70] * 3, 70)
    cat = lambda k: torch.cat([c[k] for c in cs])  # noqa: E731
    want = many.sample(cat("r_s"), cat("wa"), cat("we"), torch.cat(noise, dim=1), NFE, 2.0, 1.0, 1.0)
    got = _ragged(many, cs, noise, 2.0, 1.0, 1.0)
    assert all(torch.equal(got[q], want[q]) for q in range(3))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("mode", ["dynamic_we", "four_way_cfg"])
def test_dynamic_emotion_and_four_way_cfg(mode, dtype):
    """Lengths 120 / 60: in window 2 the longer clip runs alone, with the prev_we / prev_x / prev_wa it kept while its partner
    left the stack.  we of (T_i, 7), and the 4-row CFG batch with r = 1.5."""
    dynamic = mode == "dynamic_we"
    scales, kw = ((1.0, 1.0, 3.0), {}) if dynamic else ((2.0, 1.5, 1.2), {"include_r_cfg": True})
    one, many = _handle(dtype), _handle(dtype, 4)
    lengths = [60, 120]
    cs, noise = _clips(lengths, 90, dynamic=dynamic)
    assert cs[1]["we"].shape[1] == (120 if dynamic else 1)
    got = _ragged(many, cs, noise, *scales, **kw)
    for q, T in enumerate(lengths):
        assert got[q].shape == (T, 512)
        err = rel_l2(got[q], _alone(one, cs[q], noise[q], *scales, **kw))
        print("%s %s clip %d: rel-L2 %.3e" % (dtype, mode, q, err))
        assert err < 0.25 * TOL[dtype], (q, err)
    assert many.saturation() == 0


def test_tier3_entry_and_exit():
    """14 clips, 13 of T = 70 and one of T = 20: 2 520 rows in window 0 and 2 340 in window 1, both tier 3 of `pick_rb` with a
    different clip count.  Clips 0, 6 and the short one against the one-clip handle."""
    dtype, short = "fp16", 3
    lengths = [70] * 14
    lengths[short] = 20
    one, many = _handle(dtype), _handle(dtype, 14)
    cs, noise = _clips(lengths, 120)
    got = _ragged(many, cs, noise, 2.0, 1.0, 1.0)
    assert [tuple(g.shape) for g in got] == [(T, 512) for T in lengths]
    for q in (0, 6, short):
        err = rel_l2(got[q], _alone(one, cs[q], noise[q], 2.0, 1.0, 1.0))
        print("tier 3 clip %d (T = %d): rel-L2 %.3e" % (q, lengths[q], err))
        assert err < 0.25 * TOL[dtype], (q, err)
    assert many.saturation() == 0


def test_fp32_verification_mode():
    """fp32 operands, lengths 70 / 120, every clip against the oracle at the limit of
    tests/test_fmt_fp32_gpu.py::test_batched_and_runge_kutta_fp32 (1e-4)."""
    cfg = C.FmtConfig()
    sd = W.synth_fmt_state(cfg, seed=91)
    fmt = pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", "fp32", max_batch=2)
    try:
        lengths = [70, 120]
        cs, noise = _clips(lengths, 80, cfg=cfg)
        got = _ragged(fmt, cs, noise, 2.0, 1.0, 1.0)
        for q in range(2):
            ref = O.sample_rd(sd, cfg, cs[q]["r_s"], cs[q]["wa"], cs[q]["we"], noise[q], NFE, 2.0, 1.0, 1.0)
            err = rel_l2(got[q].cpu()[None], ref)
            print("fp32 clip %d: rel-L2 %.3e vs the oracle" % (q, err))
            assert err < 1e-4, (q, err)
    finally:
        fmt.close()


def test_runge_kutta_ragged():
    """heun3, lengths 60 / 110, held to the one-clip handle like test_batched_sampling_runge_kutta (1e-3)."""
    sd = W.synth_fmt_state(CFG, seed=42)
    one = pkg.fmt.FlowMatchingTransformerHIP(sd, CFG, "cuda:0", "fp16")
    many = pkg.fmt.FlowMatchingTransformerHIP(sd, CFG, "cuda:0", "fp16", max_batch=2)
    try:
        one.set_method("heun3")
        many.set_method("heun3")
        lengths = [60, 110]
        cs, noise = _clips(lengths, 60)
        got = many.sample_ragged(torch.cat([c["r_s"] for c in cs]), [c["wa"][0] for c in cs], [c["we"][0] for c in cs], noise, 3)
        for q in range(2):
            alone = one.sample(cs[q]["r_s"], cs[q]["wa"], cs[q]["we"], noise[q], 3)[0]
            assert rel_l2(got[q], alone) < 1e-3, (q, rel_l2(got[q], alone))
    finally:
        one.close()
        many.close()


def test_graph_cache_evicts_settings_not_stack_heights():
    """The graph cache holds 8 chain SETTINGS (nfe, CFG shape, scales, ...), each with one executable per stack height it has met.
    Small model, lengths 130 / 70 / 20 (heights 3 -> 2 -> 1): ten audio scales present 30 (setting, height) pairs and ten
    settings, so the first setting is evicted with all three of its graphs (device synchronised, executables destroyed) and
    captured again when it comes back - to the same bits, which are also those of an eager handle; and a setting still in the
    cache replays to its earlier bits after the evictions around it."""
    cfg = C.small_fmt_config()
    sd = W.synth_fmt_state(cfg, seed=10)
    graph = pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", "fp16", max_batch=3)
    eager = pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", "fp16", use_graph=0, max_batch=3)
    try:
        cs, noise = _clips([130, 70, 20], 30, cfg=cfg)
        scales = [1.5] + [2.0 + 0.1 * i for i in range(9)]
        run = lambda m, a: [t.clone() for t in _ragged(m, cs, noise, a, 1.0, 1.0)]  # noqa: E731
        same = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))  # noqa: E731
        seen = [run(graph, a) for a in scales]                     # settings 0 and 1 are evicted by the ninth and tenth
        assert all(torch.isfinite(t).all() for r in seen for t in r)
        assert not same(seen[0], seen[1])
        assert same(run(graph, scales[-1]), seen[-1])              # still cached
        assert same(run(graph, scales[0]), seen[0])                # evicted, captured again (evicts setting 2)
        assert same(run(graph, scales[1]), seen[1])
        assert same(seen[0], run(eager, scales[0])) and same(seen[-1], run(eager, scales[-1]))
        assert graph.saturation() == 0
    finally:
        graph.close()
        eager.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_eager_equals_graph(dtype):
    """The ladder on a use_graph = 0 handle against the default handle (one cached graph per stack height): bitwise."""
    graph, eager = _ladder(dtype)[0], _ladder(dtype, use_graph=0)[0]
    assert all(torch.equal(a, b) for a, b in zip(eager, graph))


def test_argument_rules():
    one, many = _handle("fp16"), _handle("fp16", 4)
    cs, noise = _clips([70, 20], 50)
    r_s = torch.cat([c["r_s"] for c in cs]).cuda()
    wa, we = [c["wa"][0].cuda() for c in cs], [c["we"][0].cuda() for c in cs]
    noise = [n.reshape(-1, 50, 512).cuda() for n in noise]
    with pytest.raises(ValueError, match="Dynamic emotion latent"):
        many.sample_ragged(r_s, wa, [torch.rand(70, 7), we[1]], noise, NFE)      # one dynamic, one static
    with pytest.raises(ValueError, match="Dynamic emotion latent"):
        many.sample_ragged(r_s, wa, [torch.rand(70, 7), torch.rand(21, 7)], noise, NFE)
    with pytest.raises(ValueError, match="noise"):
        many.sample_ragged(r_s, wa, we, [noise[0], noise[0]], NFE)               # two windows of noise for a one-window clip
    with pytest.raises(ValueError):
        many.sample_ragged(r_s, wa, we, noise[:1], NFE)
    good = [torch.empty(70, 512, device="cuda:0"), torch.empty(20, 512, device="cuda:0")]
    for bad in (torch.empty(20, 1024, device="cuda:0")[:, ::2], torch.empty(20, 512, device="cuda:0", dtype=torch.float16),
                torch.empty(20, 512), torch.empty(21, 512, device="cuda:0")):
        with pytest.raises(ValueError, match=r"out\[1\] must be a contiguous float32"):
            many.sample_ragged(r_s, wa, we, noise, NFE, out=[good[0], bad])
    # the native checks, before any HIP call
    N, L = pkg.native, pkg.native.lib()
    ptrs = lambda ts: N.dev_ptr_array(list(ts))  # noqa: E731
    Ts = (N.C.c_int32 * 2)(70, 20)
    out = [torch.empty(70, 512, device="cuda:0"), torch.empty(20, 512, device="cuda:0")]
    args = lambda h, n, T, nfe=NFE, wa_=None: (h._h, n, T, ptrs(r_s), wa_ or ptrs(wa), ptrs(we), 0, ptrs(noise), nfe,  # noqa: E731
                                               2.0, 1.0, 1.0, 0, ptrs(out))
    with pytest.raises(ValueError, match="max_batch"):
        N.check(L.float_fmt_sample_begin_ragged(*args(one, 2, Ts)))
    with pytest.raises(ValueError, match="max_batch"):
        N.check(L.float_fmt_sample_begin_ragged(*args(many, 0, Ts)))
    with pytest.raises(ValueError, match="T must be >= 1"):
        N.check(L.float_fmt_sample_begin_ragged(*args(many, 2, (N.C.c_int32 * 2)(70, 0))))
    with pytest.raises(ValueError, match="too many evaluations"):
        N.check(L.float_fmt_sample_begin_ragged(*args(many, 2, Ts, nfe=5000)))
    with pytest.raises(ValueError, match="null"):
        N.check(L.float_fmt_sample_begin_ragged(*args(many, 2, Ts, wa_=(N.C.c_void_p * 2)(wa[0].data_ptr(), None))))
    with pytest.raises(ValueError, match="null"):
        N.check(L.float_fmt_sample_begin_ragged(many._h, 2, Ts, None, None, None, 0, None, NFE, 2.0, 1.0, 1.0, 0, None))


def test_window_by_window_and_under_capture():
    """float_fmt_sample_begin_ragged + float_fmt_sample_next: windows_left counts down from the longest clip's window count;
    and the whole job captured by the caller (pointers and lengths are kernel arguments) replays to the same result."""
    many = _handle("fp16", 4)
    got, _, _, cs, noise, _ = _ladder("fp16")
    N, L = pkg.native, pkg.native.lib()
    r_s = torch.cat([c["r_s"] for c in cs]).cuda()
    wa, we = [c["wa"][0].cuda() for c in cs], [c["we"][0].cuda() for c in cs]
    nz = [n.reshape(-1, 50, 512).cuda() for n in noise]
    out = [torch.zeros(T, 512, device="cuda:0") for T in LADDER]
    Ts = (N.C.c_int32 * 4)(*LADDER)
    begin = lambda: N.check(L.float_fmt_sample_begin_ragged(  # noqa: E731
        many._h, 4, Ts, N.dev_ptr_array(list(r_s)), N.dev_ptr_array(wa), N.dev_ptr_array(we), 0, N.dev_ptr_array(nz), NFE, 2.0,
        1.0, 1.0, 0, N.dev_ptr_array(out)))
    begin()
    k, left, seen = N.C.c_int32(-1), N.C.c_int32(-1), []
    for _ in range(3):
        N.check(L.float_fmt_sample_next(many._h, N.stream_ptr("cuda:0"), N.C.byref(k), N.C.byref(left)))
        seen.append((k.value, left.value))
    assert seen == [(0, 2), (1, 1), (2, 0)]
    assert L.float_fmt_sample_next(many._h, N.stream_ptr("cuda:0"), None, None) == 1  # the job is over
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, got))
    for o in out:
        o.zero_()
    run = lambda: many.sample_ragged(r_s, wa, we, nz, NFE, 2.0, 1.0, 1.0, out=out)  # noqa: E731  (device inputs: no copies inside)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # warm-up on the capture stream
        torch.cuda.current_stream().synchronize()
        for o in out:
            o.zero_()
        with torch.cuda.graph(graph, stream=side):
            run()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, got))
    wa[LADDER.index(130)].mul_(0.5)  # same buffers, new contents: the replay must follow
    want = [t.clone() for t in many.sample_ragged(r_s, wa, we, nz, NFE, 2.0, 1.0, 1.0)]
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(want[2], got[2]) and all(torch.equal(a, b) for a, b in zip(out, want))


# ------------------------------------------------------------------------------------------------------------ product call
def _agent():
    """The synthetic 64-px agent of tests/test_dec_u8_gpu.py, and two items whose audio differs in length."""
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.input_size, opt.nfe = 64, 6
    cfg = C.FmtConfig.from_options(opt)
    acfg = C.small_audio_config()
    acfg.dim_w = opt.dim_w
    parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
                 audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
    imgs = [torch.from_numpy(np.random.RandomState(s).rand(1, 3, 64, 64).astype(np.float32)).cuda() * 2 - 1 for s in (5, 6)]
    wavs = [W.synth_waveform(1.4, seed=9).cuda(), W.synth_waveform(2.6, seed=10).cuda()]  # 35 and 65 frames: 1 and 2 windows
    return gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8), list(zip(imgs, wavs))


def _psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 99.0 if mse == 0 else -10 * float(np.log10(mse))


@pytest.mark.parametrize("noise_mode", ["cpu", "device"])
def test_product_call_with_two_lengths(noise_mode, monkeypatch):
    """InferenceAgent.infer_device_batch with items of different audio length: each item >= 45 dB from infer_device of that
    item alone with its seed (the limit tests/test_nodes_gpu.py holds stacked items to), in both FLOAT_AMD_NOISE modes; 8-bit
    output is round(255 frame) of the fp32 call, bitwise (tests/test_dec_u8_gpu.py)."""
    for v in ("FLOAT_AMD_VERIFY", "FLOAT_AMD_VERIFY_ACTION", "FLOAT_AMD_VERIFY_FRAMES", "FLOAT_AMD_VERIFY_PSNR", "FLOAT_AMD_OVERLAP"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("FLOAT_AMD_NOISE", noise_mode)
    agent, items = _agent()
    seeds = [7, 8]
    got = agent.infer_device_batch(items, 2.0, 1.0, 1.0, emo="happy", seeds=seeds)
    assert [tuple(t.shape) for t in got] == [(35, 64, 64, 3), (65, 64, 64, 3)] and all(t.is_pinned() for t in got)
    f32 = [t.clone() for t in got]
    for i, (s, a) in enumerate(items):
        alone = agent.infer_device(s, a, 2.0, 1.0, 1.0, emo="happy", seed=seeds[i])
        db = _psnr(f32[i], alone)
        print("%s noise, item %d: ragged batch vs per-item %.1f dB" % (noise_mode, i, db))
        assert db >= 45.0, (i, db)
    if noise_mode == "cpu":
        u8 = agent.infer_device_batch(items, 2.0, 1.0, 1.0, emo="happy", seeds=seeds, out_dtype=torch.uint8)
        for a, b in zip(u8, f32):
            assert a.dtype == torch.uint8 and torch.equal(a, torch.round(b * 255).to(torch.uint8))
