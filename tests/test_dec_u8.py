"""8-bit frames, the part that needs no GPU: the two entry points exist on both sides of the boundary and refuse null arguments
before any HIP call."""
import ctypes as C
import os
import re

from tests.util import ROOT, load_pkg

pkg = load_pkg()
NEW = ("float_dec_frames_u8", "float_dec_frames_host_u8")


def test_u8_entry_points_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    declared = set(re.findall(r"\b(float_[a-z_0-9]+)\s*\(", hdr))
    L = pkg.native.lib()
    for name in NEW:
        assert name in pkg.native.EXPORTS and name in declared
        assert hasattr(L, name)
    assert L.float_hip_abi_version() == pkg.native.ABI_VERSION == 6  # new symbols only: the version does not move


def test_u8_entry_points_refuse_null_arguments_without_a_gpu():
    L = pkg.native.lib()
    assert L.float_dec_frames_u8(None, None, None, 1, None, None) == 1
    assert b"null argument" in L.float_last_error() and b"float_dec_frames_u8" in L.float_last_error()
    assert L.float_dec_frames_host_u8(None, None, None, 1, None, None, None, None) == 1
    assert b"null argument" in L.float_last_error() and b"float_dec_frames_host_u8" in L.float_last_error()
    # a handle-less call with every pointer set but the handle is still a null argument (nothing is dereferenced)
    buf = (C.c_float * 4)()
    assert L.float_dec_frames_u8(None, buf, buf, 1, buf, None) == 1 and b"null argument" in L.float_last_error()


def test_frame_format_rules_need_no_gpu():
    """The Python side's dtype rules (pipeline._resolve_out_dtype): fp32 by default, uint8 on request, `out` fixes the format, a
    contradiction or any other dtype is a ValueError."""
    import pytest
    import torch
    P = pkg.pipeline
    assert P._resolve_out_dtype(None, None) == torch.float32
    assert P._resolve_out_dtype(None, torch.uint8) == torch.uint8
    assert P._resolve_out_dtype(torch.empty(1, dtype=torch.uint8), None) == torch.uint8
    assert P._resolve_out_dtype(torch.empty(1, dtype=torch.float32), torch.float32) == torch.float32
    with pytest.raises(ValueError):
        P._resolve_out_dtype(torch.empty(1, dtype=torch.uint8), torch.float32)
    with pytest.raises(ValueError):
        P._resolve_out_dtype(None, torch.float16)
    with pytest.raises(ValueError):
        P._resolve_out_dtype(torch.empty(1, dtype=torch.int8), None)
