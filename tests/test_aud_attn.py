"""CPU side of the audio attention unit tests (tests/test_aud_attn_gpu.py runs the kernels): the test hook float_aud_debug is
declared, bound and exported alike and refuses a null handle before any HIP call; and the inputs and limits of the GPU cases
are checked WITHOUT the kernel - every planted (query, key) pair really is a peak of the fp64 softmax, a torch model of the
matrix-pipe kernel's rounding (tests/util.py::attention_16bit_model) stays within half of the 16-bit limits, and the same model
with an edge key lost or without the online-softmax rescale misses them by more than 100 times (fp16; 50 times for bf16, whose
limit is 1 / 128 of max|v|).  So the limits belong to the arithmetic, and a kernel with one of those defects cannot pass."""
import ctypes as C
import os
import re

import pytest

from tests.util import ATTN_LIMITS, AUD_ATTN_CASES, ROOT, attention_16bit_model, aud_attn_case, load_pkg, max_abs, rel_l2

pkg = load_pkg()
N = pkg.native


def test_hook_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    m = re.search(r"\bint\s+float_aud_debug\s*\(([^)]*)\)\s*;", hdr)
    assert m, "float_aud_debug is not declared in include/float_hip.h"
    ctype = {"float_aud_t*": C.c_void_p, "int32_t": C.c_int32, "const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p}
    declared = [ctype[a.strip().rsplit(" ", 1)[0].strip()] for a in m.group(1).split(",")]
    res, args = N._SIGNATURES["float_aud_debug"]
    assert res is C.c_int and args == declared
    assert "float_aud_debug" in N.EXPORTS and hasattr(N.lib(), "float_aud_debug")
    assert N.lib().float_hip_abi_version() == 6 == N.ABI_VERSION  # additive: the version does not move


def test_null_arguments_are_refused_without_a_gpu():
    L = N.lib()
    assert L.float_aud_debug(None, 1, None, 1, None, None) == 1
    assert b"null argument to float_aud_debug" in L.float_last_error()
    with pytest.raises(ValueError):
        N.check(1)


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("Tn,heads", AUD_ATTN_CASES)
def test_planted_pairs_are_peaks(Tn, heads, dtype):
    """Weight of every planted pair in the fp64 softmax of the rounded inputs, in every head: >= 0.9 (measured >= 0.992)."""
    c = aud_attn_case(Tn, heads, dtype)
    print("Tn %d %s: %d pairs, smallest weight %.5f" % (Tn, dtype, len(c["pairs"]), c["pair_weight"]))
    assert len(c["pairs"]) >= 1 and c["pair_weight"] >= 0.9


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("Tn,heads", AUD_ATTN_CASES)
def test_limits_belong_to_the_arithmetic(Tn, heads, dtype):
    """The rounding model stays within HALF of the 16-bit limits (measured: 0.21 to 0.33 of the max-abs limit; rel-L2 at most 2.2e-4
    fp16 and 1.7e-3 bf16, 0.44 of the limit - on an MI355X the matrix-pipe kernel gives the model's max|d| to three digits), and misses them by more than 100 times when the last key is never seen, when the first key of the last 64-key
    tile is never seen, or when the tiles are not rescaled as the max rises.  A defect is tried where the shape can express it: a
    lost key needs a second key, the rescale a second tile.  Measured: max|d| 2.1 to 5.2 in both types, against limits of 3.5e-3
    to 5.2e-3 (fp16: 526 to 1076 times) and 2.8e-2 to 4.1e-2 (bf16: 66 to 134 times).
    The factor is 100 for fp16.  For bf16 it is 50, and that is arithmetic, not tuning: a defect replaces one value row by a mix
    of others, so its max|d| cannot exceed about max|v|, which IS 128 bf16 limits (2^-7 max|v|); without the rescale a one-key
    second tile (Tn = 65) moves the result at most half way, 64 limits.  100 bf16 limits = 0.78 max|v| is not reachable by
    every defect at every shape, whatever the seed."""
    c = aud_attn_case(Tn, heads, dtype)
    q, k, v, ref = c["q"], c["k"], c["v"], c["ref"]
    lim_abs, lim_rel = ATTN_LIMITS[dtype][0] * c["vmax"], ATTN_LIMITS[dtype][1]
    got = attention_16bit_model(q, k, v, dtype)
    d, r = max_abs(got, ref), rel_l2(got, ref)
    print("Tn %d %s model: max|d| %.3e = %.2f of the limit, rel-L2 %.3e = %.2f of the limit" % (Tn, dtype, d, d / lim_abs, r, r / lim_rel))
    assert d <= 0.5 * lim_abs and r <= 0.5 * lim_rel
    defects = {}
    if Tn >= 2:
        defects["last key never seen"] = dict(drop=(Tn - 1,))
        defects["first key of the last tile never seen"] = dict(drop=(64 * ((Tn - 1) // 64),))
    if Tn > 64:
        defects["no rescale"] = dict(rescale=False)
    for name, kw in defects.items():
        bad = max_abs(attention_16bit_model(q, k, v, dtype, **kw), ref)
        print("Tn %d %s %s: max|d| %.3e = %.0f times the limit" % (Tn, dtype, name, bad, bad / lim_abs))
        assert bad > {"fp16": 100, "bf16": 50}[dtype] * lim_abs, name
