"""CPU-side checks of the fp16 precision guard: the comparison call is part of the C ABI (additive, version still 6) and refuses
bad arguments before any HIP call; report_precision decides from a report who is at fault and warns / raises / returns; the
policy is off unless FLOAT_AMD_VERIFY asks.  No GPU here: the kernel itself is tests/test_cmp_gpu.py, the guard on the recorded
regimes tests/test_precision_guard_gpu.py."""
import ctypes as C
import math
import warnings

import pytest

from tests.util import load_pkg

pkg = load_pkg()
N, P = pkg.native, pkg.pipeline


def test_cmp_calls_are_exported_and_abi_is_still_6():
    assert "float_cmp_segments" in N.EXPORTS and "float_cmp_work_bytes" in N.EXPORTS
    L = N.lib()
    assert hasattr(L, "float_cmp_segments") and hasattr(L, "float_cmp_work_bytes")
    assert L.float_hip_abi_version() == 6 and N.ABI_VERSION == 6


def test_cmp_work_bytes_is_a_function_of_the_shape():
    L = N.lib()
    assert L.float_cmp_work_bytes(0, 10) == 0 and L.float_cmp_work_bytes(3, 0) == 0 and L.float_cmp_work_bytes(-1, -1) == 0
    for n_seg, seg_len in [(1, 1), (8, 786432), (250, 786432), (250, 3), (1, 25600), (5000, 1023)]:
        w = L.float_cmp_work_bytes(n_seg, seg_len)
        assert w >= n_seg * 5 * 8 and w % (n_seg * 5 * 8) == 0, (n_seg, seg_len, w)
        slices = w // (n_seg * 5 * 8)
        assert slices <= 512 and (slices == 1 or slices * 2048 <= seg_len), (n_seg, seg_len, slices)
    # few segments are cut into enough workgroups for 256 CUs, many are not cut into a silly number
    assert L.float_cmp_work_bytes(8, 786432) // (8 * 40) * 8 >= 1024
    assert L.float_cmp_work_bytes(250, 786432) // (250 * 40) * 250 <= 4096


def test_cmp_argument_errors_need_no_gpu():
    """FLOAT_E_INVALID (1) + a message, before any HIP call: the pointers below are host addresses that are never read."""
    L = N.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    p4 = C.c_void_p(C.addressof(buf) + 4)
    big = 1 << 20
    assert L.float_cmp_segments(None, p, 1, 8, 0.0, p, p, big, None) == 1 and b"null" in L.float_last_error()
    assert L.float_cmp_segments(p, None, 1, 8, 0.0, p, p, big, None) == 1
    assert L.float_cmp_segments(p, p, 1, 8, 0.0, None, p, big, None) == 1
    assert L.float_cmp_segments(p, p, 1, 8, 0.0, p, None, big, None) == 1
    assert L.float_cmp_segments(p, p, 0, 8, 0.0, p, p, big, None) == 1 and b"positive" in L.float_last_error()
    assert L.float_cmp_segments(p, p, -3, 8, 0.0, p, p, big, None) == 1
    assert L.float_cmp_segments(p, p, 1, 0, 0.0, p, p, big, None) == 1 and b"positive" in L.float_last_error()
    assert L.float_cmp_segments(p, p, 1, -8, 0.0, p, p, big, None) == 1
    need = L.float_cmp_work_bytes(8, 786432)
    assert L.float_cmp_segments(p, p, 8, 786432, 0.0, p, p, need - 1, None) == 1 and b"work_bytes" in L.float_last_error()
    assert L.float_cmp_segments(p, p, 1, 8, float("nan"), p, p, big, None) == 1 and b"NaN" in L.float_last_error()
    assert L.float_cmp_segments(p, p, 1, 8, 0.0, p4, p, big, None) == 1 and b"aligned" in L.float_last_error()
    with pytest.raises(ValueError):
        N.check(1)


def _cmp(psnr, non_finite=0, segments=8):
    return dict(psnr=psnr, psnr_min=psnr - 1, rel_l2=10 ** (-psnr / 20), pct_beyond=1.5, max=0.05, non_finite=non_finite,
                segments=segments)


def test_cmp_summary_pools_the_segments():
    seg = 1000
    rows = [[0.1, 250.0, 0.02, 3, 0], [0.3, 250.0, 0.05, 7, 10]]
    c = P.cmp_summary(rows, seg)
    assert c["segments"] == 2 and c["non_finite"] == 10 and c["max"] == 0.05
    assert math.isclose(c["psnr"], -10 * math.log10(0.4 / 1990), rel_tol=1e-12)
    assert math.isclose(c["psnr_min"], -10 * math.log10(0.3 / 990), rel_tol=1e-12)
    assert math.isclose(c["rel_l2"], math.sqrt(0.4 / 500), rel_tol=1e-12)
    assert math.isclose(c["pct_beyond"], 100 * 10 / 1990, rel_tol=1e-12)
    same = P.cmp_summary([[0.0, 5.0, 0.0, 0, 0]], seg)
    assert same["psnr"] == float("inf") and same["rel_l2"] == 0.0 and same["pct_beyond"] == 0.0


def test_report_precision_passes_above_the_threshold():
    rep = dict(fmt=_cmp(60, segments=1), decoder=_cmp(56.0), end_to_end=_cmp(48.6))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for action in ("warn", "raise", "auto"):
            assert P.report_precision(rep, "t", action=action) is None
        assert P.report_precision(dict(decoder=_cmp(56.0)), "t", action="raise") is None  # the decoder comparison on its own


def test_report_precision_warns_raises_and_attributes():
    dec_bad = dict(fmt=_cmp(70, segments=1), decoder=_cmp(26.6), end_to_end=_cmp(26.0))
    fmt_bad = dict(fmt=_cmp(50, segments=1), decoder=_cmp(56.0), end_to_end=_cmp(34.0))
    with pytest.warns(RuntimeWarning, match="fp16 precision check failed.*At fault: decoder"):
        assert P.report_precision(dec_bad, "t", action="warn") == "decoder"
    with pytest.warns(RuntimeWarning, match="At fault: fmt"):
        assert P.report_precision(fmt_bad, "t", action="warn") == "fmt"
    with pytest.warns(RuntimeWarning):
        assert P.report_precision(fmt_bad, "t", action="auto") == "fmt"  # auto: warn, the caller rebuilds
    with pytest.raises(P.Fp16PrecisionError, match="26.0 dB"):
        P.report_precision(dec_bad, "t", action="raise")
    assert issubclass(P.Fp16PrecisionError, ArithmeticError) and not issubclass(P.Fp16PrecisionError, P.Fp16RangeError)
    with pytest.raises(P.Fp16PrecisionError, match="At fault: decoder"):
        P.report_precision(dict(decoder=_cmp(26.6, segments=2)), "t", action="raise")  # decoder-only report
    # the threshold is an argument / FLOAT_AMD_VERIFY_PSNR, 40 dB by default
    assert P.report_precision(fmt_bad, "t", action="raise", min_psnr=30.0) is None
    with pytest.raises(P.Fp16PrecisionError):
        P.report_precision(dict(decoder=_cmp(56.0), end_to_end=_cmp(48.6)), "t", action="raise", min_psnr=50.0)
    with pytest.raises(ValueError):
        P.report_precision(fmt_bad, "t", action="ignore")
    with pytest.raises(ValueError):
        P.report_precision({}, "t", action="raise")


def test_report_precision_env(monkeypatch):
    fmt_bad = dict(fmt=_cmp(50, segments=1), decoder=_cmp(56.0), end_to_end=_cmp(34.0))
    monkeypatch.delenv("FLOAT_AMD_VERIFY_ACTION", raising=False)
    monkeypatch.delenv("FLOAT_AMD_VERIFY_PSNR", raising=False)
    with pytest.warns(RuntimeWarning):
        assert P.report_precision(fmt_bad, "t") == "fmt"  # default: warn at 40 dB
    monkeypatch.setenv("FLOAT_AMD_VERIFY_ACTION", "raise")
    with pytest.raises(P.Fp16PrecisionError):
        P.report_precision(fmt_bad, "t")
    monkeypatch.setenv("FLOAT_AMD_VERIFY_PSNR", "33.5")
    assert P.report_precision(fmt_bad, "t") is None


def test_a_non_finite_sample_always_fails():
    for rep, fault in [(dict(fmt=_cmp(60, segments=1), decoder=_cmp(56.0, non_finite=1), end_to_end=_cmp(48.6, non_finite=1)), "decoder"),
                       (dict(fmt=_cmp(60, non_finite=2, segments=1), decoder=_cmp(56.0), end_to_end=_cmp(48.6)), "fmt"),
                       (dict(fmt=_cmp(60, segments=1), decoder=_cmp(56.0), end_to_end=_cmp(float("inf"), non_finite=5)), "fmt")]:
        with pytest.raises(P.Fp16PrecisionError, match="non-finite"):
            P.report_precision(rep, "t", action="raise")
        with pytest.warns(RuntimeWarning):
            assert P.report_precision(rep, "t", action="warn") == fault


def test_policy_is_off_unless_asked(monkeypatch):
    monkeypatch.delenv("FLOAT_AMD_VERIFY", raising=False)
    assert P.precision_policy() == "skip" and P.precision_policy(checked=True) == "skip"
    monkeypatch.setenv("FLOAT_AMD_VERIFY", "off")
    assert P.precision_policy() == "skip"
    monkeypatch.setenv("FLOAT_AMD_VERIFY", "first")
    assert P.precision_policy(checked=False) == "check" and P.precision_policy(checked=True) == "skip"
    monkeypatch.setenv("FLOAT_AMD_VERIFY", "always")
    assert P.precision_policy(checked=True) == "check"
    monkeypatch.setenv("FLOAT_AMD_VERIFY", "sometimes")
    with pytest.raises(ValueError):
        P.precision_policy()
    monkeypatch.delenv("FLOAT_AMD_VERIFY_FRAMES", raising=False)
    assert P.verify_frames_default() == 8
