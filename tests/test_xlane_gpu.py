"""The kernels' cross-lane reductions (csrc/common.hpp: wave_sum, wave_max, group_sum) as DPP operands and lane swaps
instead of the __shfl_xor butterfly, which is an LDS round trip per step.  Both forms run in one probe kernel
(float_fmt_debug request 5, FlowMatchingTransformerHIP.xlane_probe) and must agree on every lane bit for bit; then the two
kernels of the step chain that use them - LayerNorm and the banded attention - at the row counts of
tests/test_fmt_launch_head_gpu.py (1 / 3 / 4, 17 / 51 / 68 and 60 / 180 / 240 rows: partial waves and partial 8-row groups), for
a band of 2 (every load in front of the first use) and of 3 (the loop), against the references and limits of the tests that
already hold them (tests/test_fmt_tables.py, tests/test_fmt_launch_head_gpu.py), with a second call and a graph replay
bitwise equal to the first call."""
import functools

import pytest
import torch

from oracle import float_oracle as O
from tests.util import ATTN_LIMITS, attention_fp64, load_pkg, max_abs, peaked_qkv, qkv_rows, rel_l2

pkg = load_pkg()
W, C, N = pkg.weights, pkg.config, pkg.native
pytestmark = pytest.mark.gpu

SUMS = ("wave sum", "wave max", "16-lane sum", "8-lane sum", "4-lane sum")
GROUP = (64, 64, 16, 8, 4)
TOL = {"fp16": 4e-3, "bf16": 2e-2, "fp32": 2e-5}  # per evaluation, as tests/test_fmt_launch_head_gpu.py
SCALES = {1: (1.0, 1.0, 1.0, False), 3: (2.0, 1.0, 1.0, False), 4: (2.0, 1.5, 1.2, True)}  # a, r, e, include_r_cfg
SIZES = [(0, 1), (2, 15), (10, 50)]  # (n_prev, n_cur): 1, 17 and 60 tokens
T_EVAL = 0.3


def _probe_inputs():
    g = torch.Generator().manual_seed(41)
    rnd = torch.randn(64, 64, generator=g)
    # magnitudes 2^-20 .. 2^20 with mixed signs: (a + b) + c and a + (b + c) differ in their last bits almost everywhere
    wide = torch.randn(64, 64, generator=g).sign() * torch.exp2(torch.rand(64, 64, generator=g) * 40 - 20)
    one_hot = torch.eye(64) * 3.0  # a term that a wrong partner drops (or counts twice) changes the sum by 3
    neg_hot = -torch.eye(64) - 1.0  # the max's counterpart: -2 in one lane and -1 elsewhere (a lane counted for its partner shows) ...
    pos_hot = torch.eye(64) - 2.0  # ... and -1 in one lane, -2 elsewhere (a lane that is left out shows)
    return {"random": rnd, "wide": wide, "one_hot": one_hot, "neg_hot": neg_hot, "pos_hot": pos_hot}


@functools.lru_cache(maxsize=None)
def _handle(dtype="fp16"):
    cfg = C.small_fmt_config()
    return pkg.fmt.FlowMatchingTransformerHIP(W.synth_fmt_state(cfg, seed=71), cfg, "cuda:0", dtype)


@pytest.mark.parametrize("name", list(_probe_inputs()))
def test_new_form_is_the_shfl_xor_butterfly_on_every_lane(name):
    v = _probe_inputs()[name]
    out = _handle().xlane_probe(v).cpu()
    assert out.shape == (v.shape[0], 5, 2, 64)
    for k, what in enumerate(SUMS):
        assert torch.equal(out[:, k, 0], out[:, k, 1]), "%s of %s vectors: new form != __shfl_xor form" % (what, name)
    # and the butterfly itself is the sum / max it is meant to be: exact where every partial sum is (small integers), else
    # within the rounding of 63 fp32 additions of terms of one vector (64 * 2^-24 * sum |v|)
    grp = lambda t, n: t.double().reshape(t.shape[0], 64 // n, n)  # noqa: E731
    exact = name not in ("random", "wide")
    for k, n in enumerate(GROUP):
        want = (grp(v, n).amax(-1) if k == 1 else grp(v, n).sum(-1)).repeat_interleave(n, dim=1)
        lim = (grp(v, n).abs().sum(-1) * (0.0 if exact or k == 1 else 64 * 2.0 ** -24)).repeat_interleave(n, dim=1)
        d = (out[:, k, 0].double() - want).abs()
        print("%s, %s: max|d| to fp64 %.3e" % (name, SUMS[k], float(d.max())))
        assert bool((d <= lim).all())


def test_probe_takes_any_number_of_vectors():
    v = _probe_inputs()["wide"]
    f = _handle()
    whole = f.xlane_probe(v)
    assert torch.equal(f.xlane_probe(v[:5]), whole[:5])
    assert torch.equal(f.xlane_probe(torch.cat([v, v[:7]]))[64:], whole[:7])
    with pytest.raises(ValueError):
        f.xlane_probe(torch.zeros(3, 32))


def _cfg(n_prev, n_cur, window):
    cfg = C.small_fmt_config()
    cfg.num_prev_frames, cfg.num_frames_for_clip, cfg.attention_window = n_prev, n_cur, window
    return cfg


@functools.lru_cache(maxsize=None)
def _attn_case(ntok, window, dtype):
    q, k, v, _ = peaked_qkv(ntok, 2, 128, 9000 + ntok, dtype)
    blocked = W.band_mask(ntok, window)
    ref = attention_fp64(q, k, v, blocked)
    return {"rows": qkv_rows(q, k, v), "ref": ref, "vmax": float(v.abs().max()),
            "e32": max_abs(attention_fp64(q, k, v, blocked, dtype=torch.float32), ref)}


def _replay(call, new):
    """`call(out)` captured into a graph on a side stream and replayed once into a zeroed buffer."""
    out_g, graph, side = new(), torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(out_g)  # warm-up on the capture stream
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(graph, stream=side):
            call(out_g)
    torch.cuda.current_stream().wait_stream(side)
    out_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    return out_g


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("window", [2, 3])
@pytest.mark.parametrize("n_prev,n_cur", SIZES)
def test_attention_call(n_prev, n_cur, window, dtype):
    """One launch of the chain's attention kernel on 1, 17 and 60 rows (2 heads): against attention_fp64 of the rounded inputs
    under the band, at the limits of tests/test_fmt_tables.py (ATTN_LIMITS; fp32: max(4 * e32, 1e-6 max|v|))."""
    cfg = _cfg(n_prev, n_cur, window)
    c = _attn_case(cfg.n_tokens, window, dtype)
    fmt = pkg.fmt.FlowMatchingTransformerHIP(W.synth_fmt_state(cfg, seed=71), cfg, "cuda:0", dtype)
    try:
        rows = c["rows"].to("cuda:0")
        first = fmt.attention_probe(rows)
        out = first.cpu()
        d, r = max_abs(out, c["ref"]), rel_l2(out, c["ref"])
        if dtype == "fp32":
            lim = max(4 * c["e32"], 1e-6 * c["vmax"])
            print("ntok %d window %d fp32: max|d| %.3e, e32 %.3e, limit %.3e" % (cfg.n_tokens, window, d, c["e32"], lim))
            assert d <= lim
        else:
            lim_abs, lim_rel = ATTN_LIMITS[dtype][0] * c["vmax"], ATTN_LIMITS[dtype][1]
            print("ntok %d window %d %s: max|d| %.3e (limit %.3e), rel-L2 %.3e (limit %.3e)" % (cfg.n_tokens, window, dtype, d, lim_abs, r, lim_rel))
            assert d <= lim_abs and r <= lim_rel
        assert torch.equal(fmt.attention_probe(rows), first), "second call on the handle"

        def call(o):
            N.check(N.lib().float_fmt_debug(fmt._h, 1, N.dev_ptr(rows), N.dev_ptr(o), N.stream_ptr(fmt.device)))

        assert torch.equal(_replay(call, lambda: torch.zeros_like(first)), first), "graph replay against the eager launch"
        assert fmt.saturation() == 0
    finally:
        fmt.close()


@functools.lru_cache(maxsize=None)
def _eval_case(n_prev, n_cur, way, window):
    """Weights, inputs (on the GPU) and the oracle's velocity of one case: made once, shared by the dtypes, read-only."""
    cfg = _cfg(n_prev, n_cur, window)
    sd = W.synth_fmt_state(cfg, seed=71)
    g = torch.Generator().manual_seed(100 * n_cur + way)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = dict(x=r(1, n_cur, cfg.dim_w), wa=r(1, n_cur, cfg.dim_a), wr=r(1, cfg.dim_w), we=torch.softmax(r(1, 1, cfg.dim_e), -1),
               prev_x=r(1, n_prev, cfg.dim_w), prev_wa=r(1, n_prev, cfg.dim_a))
    a, rs, e, inc = SCALES[way]
    ref = O.fmt_forward_cfv(sd, cfg, torch.tensor([T_EVAL]), inp["x"], inp["wa"], inp["wr"], inp["we"], inp["prev_x"], inp["prev_wa"],
                            None, a, rs, e, inc)
    dev = {k: v.to("cuda:0").contiguous() for k, v in inp.items()}
    for k in ("prev_x", "prev_wa"):  # an empty tensor has no address: n_prev = 0 hands over a pointer 0 elements are copied from
        if dev[k].numel() == 0:
            dev[k] = torch.zeros(1, device="cuda:0")
    return cfg, sd, dev, ref


# every CFG width under the band of 2; the loop path of the band of 3 does not depend on the width beyond the row count
EVALS = [(p, c, way, 2) for p, c in SIZES for way in (1, 3, 4)] + [(p, c, 3, 3) for p, c in SIZES]


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("n_prev,n_cur,way,window", EVALS)
def test_evaluation(n_prev, n_cur, way, window, dtype):
    """One float_fmt_eval (17 LayerNorm and 8 attention launches among its 59) against the oracle's fmt_forward_cfv."""
    cfg, sd, dev, ref = _eval_case(n_prev, n_cur, way, window)
    fmt = pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", dtype)
    a, r, e, inc = SCALES[way]
    p = N.dev_ptr

    def call(out):
        N.check(N.lib().float_fmt_eval(fmt._h, T_EVAL, p(dev["x"]), p(dev["wa"]), p(dev["wr"]), p(dev["we"]), 1, p(dev["prev_x"]),
                                       p(dev["prev_wa"]), None, a, r, e, 1 if inc else 0, p(out), N.stream_ptr(fmt.device)))
        return out

    new = lambda: torch.zeros(1, cfg.n_tokens, cfg.dim_w, device="cuda:0")  # noqa: E731
    try:
        first = call(new())
        torch.cuda.synchronize()
        err = rel_l2(first.cpu(), ref)
        print("n_prev %d n_cur %d %d-way window %d %s: rel-L2 %.3e (limit %.0e)" % (n_prev, n_cur, way, window, dtype, err, TOL[dtype]))
        assert err < TOL[dtype], err
        assert torch.equal(call(new()), first), "second call on the handle"
        assert torch.equal(_replay(call, new), first), "graph replay against the eager launches"
        assert fmt.saturation() == 0
    finally:
        fmt.close()
