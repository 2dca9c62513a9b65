"""The step chain's kernels behind their preloaded heads (csrc/fmt_pack.hpp GemmHead, csrc/fmt_decode.hpp): one float_fmt_eval
per case against the oracle's fmt_forward_cfv at the per-evaluation limits of tests/test_fmt_gpu.py and test_fmt_fp32_gpu.py.
The small config (dim_h 256) gives qkv 12 column blocks of 64 - not a multiple of 8, the generic walk of the block decode that
the full model never takes - and its row counts 1 / 3 / 4, 17 / 51 / 68 and 60 / 180 / 240 cross the 16- and 48-row tile edges
with 1-, 3- and 4-way CFG.  Every case also: a second call on the same handle and a replay of the evaluation captured into a
graph, both bitwise equal to the first eager call."""
import functools

import pytest
import torch

from oracle import float_oracle as O
from tests.util import load_pkg, rel_l2

pkg = load_pkg()
W, C, N = pkg.weights, pkg.config, pkg.native
pytestmark = pytest.mark.gpu

TOL = {"fp16": 4e-3, "bf16": 2e-2, "fp32": 2e-5}
SCALES = {1: (1.0, 1.0, 1.0, False), 3: (2.0, 1.0, 1.0, False), 4: (2.0, 1.5, 1.2, True)}  # a, r, e, include_r_cfg
T_EVAL = 0.3


@functools.lru_cache(maxsize=None)
def _case(n_prev, n_cur, way, full=False):
    """Config, weights, inputs (on the GPU) and the oracle's velocity of one case: made once, shared by the dtypes, read-only."""
    cfg = C.FmtConfig() if full else C.small_fmt_config()
    if not full:
        cfg.num_prev_frames, cfg.num_frames_for_clip = n_prev, n_cur
    sd = W.synth_fmt_state(cfg, seed=71)
    g = torch.Generator().manual_seed(100 * n_cur + way)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = dict(x=r(1, n_cur, cfg.dim_w), wa=r(1, n_cur, cfg.dim_a), wr=r(1, cfg.dim_w), we=torch.softmax(r(1, 1, cfg.dim_e), -1),
               prev_x=r(1, n_prev, cfg.dim_w), prev_wa=r(1, n_prev, cfg.dim_a))
    a, rs, e, inc = SCALES[way]
    ref = O.fmt_forward_cfv(sd, cfg, torch.tensor([T_EVAL]), inp["x"], inp["wa"], inp["wr"], inp["we"], inp["prev_x"], inp["prev_wa"],
                            None, a, rs, e, inc)
    dev = {k: v.to("cuda:0").contiguous() for k, v in inp.items()}
    # an empty tensor has no address: n_prev = 0 hands the library a pointer it copies 0 elements from
    for k in ("prev_x", "prev_wa"):
        if dev[k].numel() == 0:
            dev[k] = torch.zeros(1, device="cuda:0")
    return cfg, sd, dev, ref


def _eval(fmt, dev, way, out):
    a, r, e, inc = SCALES[way]
    p = N.dev_ptr
    N.check(N.lib().float_fmt_eval(fmt._h, T_EVAL, p(dev["x"]), p(dev["wa"]), p(dev["wr"]), p(dev["we"]), 1, p(dev["prev_x"]),
                                   p(dev["prev_wa"]), None, a, r, e, 1 if inc else 0, p(out), N.stream_ptr(fmt.device)))
    return out


def _check(n_prev, n_cur, way, dtype, full=False):
    cfg, sd, dev, ref = _case(n_prev, n_cur, way, full)
    fmt = pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", dtype)
    new = lambda: torch.zeros(1, cfg.n_tokens, cfg.dim_w, device="cuda:0")  # noqa: E731
    try:
        first = _eval(fmt, dev, way, new())
        torch.cuda.synchronize()
        err = rel_l2(first.cpu(), ref)
        print("n_prev %d n_cur %d %d-way %s%s: rel-L2 %.3e (limit %.0e)" % (n_prev, n_cur, way, dtype, " full" if full else "", err, TOL[dtype]))
        assert err < TOL[dtype], err
        assert torch.equal(_eval(fmt, dev, way, new()), first), "second call on the handle"
        out_g, graph, side = new(), torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _eval(fmt, dev, way, out_g)  # warm-up on the capture stream
            torch.cuda.current_stream().synchronize()
            with torch.cuda.graph(graph, stream=side):
                _eval(fmt, dev, way, out_g)
        torch.cuda.current_stream().wait_stream(side)
        out_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g, first), "graph replay against the eager launches"
        assert fmt.saturation() == 0
    finally:
        fmt.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("way", [1, 3, 4])
@pytest.mark.parametrize("n_prev,n_cur", [(0, 1), (2, 15), (10, 50)])
def test_eval_small_config(n_prev, n_cur, way, dtype):
    _check(n_prev, n_cur, way, dtype)


def test_eval_full_config():
    _check(10, 50, 3, "fp16", full=True)
