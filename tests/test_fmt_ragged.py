"""Ragged FMT jobs (float_fmt_sample_begin_ragged / float_fmt_sample_batch_ragged, FlowMatchingTransformerHIP.sample_ragged),
the parts that need no GPU: how clips are grouped into chains, and the C boundary of the two new entry points."""
import ctypes
import os
import re

import pytest

from tests.util import ROOT, load_pkg

pkg = load_pkg()
groups = pkg.fmt.ragged_groups
N_CUR = 50


def windows(T):
    return (T + N_CUR - 1) // N_CUR


LENGTH_SETS = [[130, 70, 70, 20], [20, 70, 130, 70], [1], [50, 51, 100, 101, 49], [70] * 5,
               [500, 55, 120, 300, 60, 250, 90, 410, 50, 175, 230, 140, 365, 75, 105, 480, 20, 333, 260]]


@pytest.mark.parametrize("lengths", LENGTH_SETS)
@pytest.mark.parametrize("max_batch", [1, 3, 4, 16])
def test_groups_partition_the_batch(lengths, max_batch):
    gs = groups(lengths, N_CUR, max_batch)
    assert sorted(i for g in gs for i in g) == list(range(len(lengths)))          # every index exactly once
    assert all(1 <= len(g) <= max_batch for g in gs) and all(len(g) == max_batch for g in gs[:-1])
    for g in gs:
        w = [windows(lengths[i]) for i in g]
        assert w == sorted(w, reverse=True)                                       # non-increasing inside a group
        # the clips active in window k are the first active(k) slots, and the chain evaluates exactly the windows asked for
        active = [sum(1 for x in w if x > k) for k in range(w[0])]
        assert all(w[q] > k for k in range(w[0]) for q in range(active[k]))
        assert sum(active) == sum(w)
    flat = [windows(lengths[i]) for g in gs for i in g]
    assert flat == sorted(flat, reverse=True)                                     # B > max_batch is cut by sorted length


def test_equal_lengths_keep_the_caller_order():
    assert groups([70] * 7, N_CUR, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert groups([70, 60, 99, 51], N_CUR, 16) == [[0, 1, 2, 3]]                  # all two windows: stable
    assert groups([], N_CUR, 4) == []


def test_longer_clips_share_a_chain():
    assert groups([20, 130, 70, 70], N_CUR, 16) == [[1, 2, 3, 0]]
    assert groups([20, 130, 70, 70, 260], N_CUR, 2) == [[4, 1], [2, 3], [0]]


NEW = ("float_fmt_sample_begin_ragged", "float_fmt_sample_batch_ragged")


def _declared_args(name):
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, "%s is not declared in float_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _kind(decl):
    """C parameter declaration -> the ctypes type the binding must use for it."""
    if re.match(r"^(const )?float\* ?const\* \w+$", decl):
        return ctypes.POINTER(ctypes.c_void_p)      # host array of device pointers
    if re.match(r"^const int32_t\* \w+$", decl):
        return ctypes.POINTER(ctypes.c_int32)
    if re.match(r"^int32_t \w+$", decl):
        return ctypes.c_int32
    if re.match(r"^float \w+$", decl):
        return ctypes.c_float
    if re.match(r"^(float_fmt_t|void)\* \w+$", decl):
        return ctypes.c_void_p
    raise AssertionError("unexpected parameter %r" % decl)


@pytest.mark.parametrize("name", NEW)
def test_binding_matches_the_header(name):
    args = _declared_args(name)
    res, argtypes = pkg.native._SIGNATURES[name]
    assert res is ctypes.c_int
    assert [_kind(a) for a in args] == list(argtypes), (args, argtypes)
    assert hasattr(pkg.native.lib(), name)


def test_batch_form_is_begin_plus_a_stream():
    begin, batch = (_declared_args(n) for n in NEW)
    assert batch[:-1] == begin and batch[-1] == "void* stream"
    names = [a.split()[-1] for a in begin]
    assert names == ["h", "n_clips", "T", "wr", "wa", "we", "we_dynamic", "noise", "nfe", "a_cfg", "r_cfg", "e_cfg",
                     "include_r_cfg", "r_d"]


def test_abi_version_stays_6():
    assert pkg.native.ABI_VERSION == 6 and pkg.native.lib().float_hip_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    assert re.search(r"#define FLOAT_HIP_ABI_VERSION 6\b", hdr)


def test_null_handle_is_invalid_with_a_message():
    L = pkg.native.lib()
    one = (ctypes.c_void_p * 1)(None)
    T = (ctypes.c_int32 * 1)(70)
    assert L.float_fmt_sample_begin_ragged(None, 1, T, one, one, one, 0, one, 5, 2.0, 1.0, 1.0, 0, one) == 1
    assert b"null FMT handle" in L.float_last_error()
    assert L.float_fmt_sample_batch_ragged(None, 1, T, one, one, one, 0, one, 5, 2.0, 1.0, 1.0, 0, one, None) == 1
    assert b"null FMT handle" in L.float_last_error()
    with pytest.raises(ValueError, match="null FMT handle"):
        pkg.native.check(L.float_fmt_sample_begin_ragged(None, 0, None, None, None, None, 0, None, 5, 2.0, 1.0, 1.0, 0, None))
