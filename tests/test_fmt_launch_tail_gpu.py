"""The step chain's GEMM behind its last MFMA (csrc/fmt_kernels.hpp fmt_gemm_body): the straight-line form of the body for the
one-clip shapes - every load of the prologue issued by every lane, the touch without a branch, its retire behind the last store.
None of it may move a bit.

The cases are those of tests/test_fmt_launch_head_gpu.py - its inputs and its call - because they are the shapes at which the
tail can go wrong: row counts 1 / 3 / 4, 17 / 51 / 68 and 60 / 180 / 240 cross the 16- and 48-row tile edges (the row guard
of the reducing threads, partial tiles), the small config's K = 256 takes the general form of the body and the full config's
K = 1024 the straight-line one.  One float_fmt_eval per case, checked
  1. against the oracle at the per-evaluation limits of that file,
  2. bitwise against the velocity the commit before this change produced (tests/golden/fmt_tail_parent.npz, recorded on an
     MI355X by tools/make_tail_golden.py),
  3. a second call on the handle and a graph replay bitwise equal to the first call, saturation() == 0,
  4. the same on a handle whose tuning record has the weight touch switched off, bitwise equal to touch on.

test_ksplit_exchange runs ONE workgroup's K-split exchange through LDS (straight-line form, K = 1024) on operands that make
wave w's partial sum at (row, column) the power of two 2^(3w - 12 + d), d = digit w of a base-3 code that is unique per (row, column): the eight waves own disjoint 3-bit fields of
the fp32 sum, so the sum is exact in any order and its bits name each (wave, row, column) that was dropped (field empty),
duplicated (carry into the next bit) or taken from another place (another digit)."""
import os

import numpy as np
import pytest
import torch

from tests import test_fmt_launch_head_gpu as H
from tests.util import GOLDEN, rel_l2

pkg, C, W = H.pkg, H.C, H.W
pytestmark = pytest.mark.gpu

_golden = None


def _parent(key):
    global _golden
    if _golden is None:
        _golden = np.load(os.path.join(GOLDEN, "fmt_tail_parent.npz"))
    return torch.from_numpy(_golden[key])


def _handle_checks(fmt, cfg, dev, way):
    """First call, second call and graph replay on one handle; returns the first call's velocity."""
    new = lambda: torch.zeros(1, cfg.n_tokens, cfg.dim_w, device="cuda:0")  # noqa: E731
    first = H._eval(fmt, dev, way, new())
    torch.cuda.synchronize()
    assert torch.equal(H._eval(fmt, dev, way, new()), first), "second call on the handle"
    out_g, graph, side = new(), torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H._eval(fmt, dev, way, out_g)  # warm-up on the capture stream
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(graph, stream=side):
            H._eval(fmt, dev, way, out_g)
    torch.cuda.current_stream().wait_stream(side)
    out_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g, first), "graph replay against the eager launches"
    assert fmt.saturation() == 0
    return first


def _check(monkeypatch, n_prev, n_cur, way, dtype, full=False):
    cfg, sd, dev, ref = H._case(n_prev, n_cur, way, full)
    key = "%d_%d_%d_%s%s" % (n_prev, n_cur, way, dtype, "_full" if full else "")
    fmt = pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", dtype)
    try:
        first = _handle_checks(fmt, cfg, dev, way)
    finally:
        fmt.close()
    err = rel_l2(first.cpu(), ref)
    print("%s: rel-L2 %.3e (limit %.0e)" % (key, err, H.TOL[dtype]))
    assert err < H.TOL[dtype], err
    want = _parent(key)
    nbad = int((first.cpu() != want).sum())
    print("%s: %d of %d elements differ from the parent commit's velocity" % (key, nbad, want.numel()))
    assert torch.equal(first.cpu(), want), "velocity differs from the parent commit's (%d elements)" % nbad
    monkeypatch.setenv("FLOAT_FMT_TOUCH", "0")  # read into the handle's tuning record when it is created
    plain = pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", dtype)
    try:
        assert torch.equal(_handle_checks(plain, cfg, dev, way), first), "weight touch off against touch on"
    finally:
        plain.close()


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("way", [1, 3, 4])
@pytest.mark.parametrize("n_prev,n_cur", [(0, 1), (2, 15), (10, 50)])
def test_eval_small_config(monkeypatch, n_prev, n_cur, way, dtype):
    _check(monkeypatch, n_prev, n_cur, way, dtype)


def test_eval_full_config(monkeypatch):
    _check(monkeypatch, 10, 50, 3, "fp16", full=True)


def _exchange_operands(N, waves=8, K=1024):
    """a (48, K), w (N, K), want (48, N) float64: wave i multiplies columns i * K / waves .. of both; a picks column `row` of the
    wave's slice, where w holds the wave's power of two for (row, column)."""
    ks = K // waves
    assert ks >= 48 and 48 * N <= 3 ** waves
    row, col = torch.meshgrid(torch.arange(48), torch.arange(N), indexing="ij")
    code = ((row * N + col) * 1117) % (3 ** waves)  # 1117 is prime to 3: one code per (row, column)
    a, w, want = torch.zeros(48, K), torch.zeros(N, K), torch.zeros(48, N, dtype=torch.float64)
    for i in range(waves):
        e = 3 * i - 12 + (code // 3 ** i) % 3
        p = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())  # (48, N)
        a[torch.arange(48), i * ks + torch.arange(48)] = 1.0
        w[:, i * ks:i * ks + 48] = p.t().float()
        want += p
    return a, w, want, code


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("N", [64, 16])
def test_ksplit_exchange(N, dtype):
    cfg = C.small_fmt_config()
    fmt = pkg.fmt.FlowMatchingTransformerHIP(W.synth_fmt_state(cfg, seed=71), cfg, "cuda:0", dtype)
    try:
        a, w, want, code = _exchange_operands(N)
        got = fmt.gemm_tile_probe(a, w).cpu().double()
    finally:
        fmt.close()
    bad = (got != want).nonzero()
    for r, c in bad[:8].tolist():
        digits = [int(code[r, c] // 3 ** i) % 3 for i in range(8)]
        print("(row %d, column %d): got %r, expected %r = sum_w 2^(3w - 12 + d_w), d = %s" % (r, c, float(got[r, c]), float(want[r, c]), digits))
    assert len(bad) == 0, "%d of %d sums of the 48 x %d tile are not the eight waves' partial sums" % (len(bad), want.numel(), N)
