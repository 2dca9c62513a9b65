"""Every arm of the FMT host layer's kernel dispatch that a tuning switch selects: the GEMM tilings of each epilogue list, the
LayerNorm reduction arms, the LayerNorm / attention workgroup shapes, the full-height CFG-epilogue tilings and the wide-N
kernels of the fused adaLN projection.  The switches are read when a handle is created (csrc/tuning.hpp), so each case sets
its environment first and then creates its own handle, runs ONE 3-way-CFG evaluation (180 rows, 12 row tiles: the smallest
shape on which the CFG-batched tilings are what production picks) and holds it to the reference golden at the fp16 limit of
tests/test_fmt_gpu.py.  Whether an arm is bitwise the default chain is printed, not asserted (not measured for every arm)."""
import functools

import pytest
import torch

from tests.test_fmt_gpu import TOL
from tests.util import golden, load_pkg, rel_l2

pkg = load_pkg()
W, C = pkg.weights, pkg.config
pytestmark = pytest.mark.gpu

# (row tiles, column tiles) per workgroup of the split GEMM tilings; each exists with 4, 8 and 16 K-splitting waves, and 16
# waves need K % 512 == 0, which no layer of the small model with K = 256 has
SPLIT_SHAPES = [(3, 1), (3, 2), (3, 4), (5, 1), (5, 2), (5, 4), (4, 1), (4, 2), (6, 2), (2, 1), (1, 1)]


def _plan(layers, mtw, nt, nw):
    return {"FLOAT_FMT_PLAN_" + layer: "%d,%d,%d" % (mtw, nt, nw) for layer in layers}


SMALL_CASES = (
    [_plan(("QKV", "FC1"), mtw, nt, nw) for mtw, nt in SPLIT_SHAPES for nw in (4, 8)]  # EPI_T16, EPI_GELU_P16
    + [_plan(("PROJ", "FC2"), 3, 1, 4), _plan(("PROJ", "FC2"), 5, 2, 8)]  # EPI_GATE_RES, EPI_PARTIAL
    + [{"FLOAT_FMT_PROJ_SPLIT": v} for v in ("1", "2")]  # LayerNorm reduction arms KS = 1, 2
    + [{"FLOAT_FMT_FC2_SPLIT": v} for v in ("0", "1", "2")]
    + [{"FLOAT_FMT_LN_ROWS": v} for v in ("2", "4")]
    + [{"FLOAT_FMT_ATTN": v} for v in ("8,8", "4,16")]
    + [{"FLOAT_FMT_NO_TOKBLK": "1", "FLOAT_FMT_FULL_NW": v} for v in ("4", "8")]  # the full-height EPI_CFG tilings
)
# the register-staged wide kernels and the lock-step LDS-DMA tile: the fused projection's N is a multiple of 320 on the full
# model only
FULL_CASES = [{"FLOAT_FMT_WIDE_VARIANT": v} for v in ("0", "1", "3", "4", "5", "6")]


def _case_id(env):
    return "-".join("%s=%s" % (k.replace("FLOAT_FMT_", ""), v) for k, v in env.items())


@functools.lru_cache(maxsize=None)
def _model(tag):
    g = golden("fmt_eval_" + tag)
    cfg = C.small_fmt_config() if tag == "small" else C.FmtConfig()
    return g, cfg, W.synth_fmt_state(cfg, g["seed"])


def _eval_cfg3(tag):
    """(velocity of the golden's cfg3 case on a new fp16 handle, its saturation count)"""
    g, cfg, sd = _model(tag)
    fmt = pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", dtype="fp16")
    a, r, e, rc = [float(v) for v in g["cfg3_scales"]]
    out = fmt.forward_with_cfv(g["t"], g["cfg3_x"], g["cfg3_wa"], g["cfg3_wr"], g["cfg3_we"], g["cfg3_prev_x"], g["cfg3_prev_wa"],
                               g.get("cfg3_prev_we"), a_cfg_scale=a, r_cfg_scale=r, e_cfg_scale=e, include_r_cfg=bool(rc)).cpu()
    return out, fmt.saturation()


@pytest.fixture(scope="module")
def default_out():
    """The default handle's result per model, computed once and before any case sets its switches."""
    return {tag: _eval_cfg3(tag)[0] for tag in ("small", "full")}


def _check(tag, env, default_out, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out, sat = _eval_cfg3(tag)
    err = rel_l2(out, _model(tag)[0]["cfg3_out"])
    print(tag, _case_id(env), "rel-L2 %.3e" % err, "bitwise the default handle's:", torch.equal(out, default_out[tag]))
    assert err < TOL["fp16"], err
    assert sat == 0


@pytest.mark.parametrize("env", SMALL_CASES, ids=_case_id)
def test_small_model_dispatch(env, default_out, monkeypatch):
    _check("small", env, default_out, monkeypatch)


@pytest.mark.parametrize("env", FULL_CASES, ids=_case_id)
def test_wide_projection_variants(env, default_out, monkeypatch):
    _check("full", env, default_out, monkeypatch)
