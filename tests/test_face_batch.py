"""The face detector on n stacked views, without a GPU: the five float_sfd_*_batch symbols, the refusals that need no handle
(null pointers, n outside 1 ... 64; those against a reservation need a handle and are in test_face_batch_gpu.py), and
FaceDetectorHIP.detect_batch's grouping on a stub library."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.util import ROOT, load_pkg

pkg = load_pkg()

BATCH_SYMBOLS = ("float_sfd_reserve_batch", "float_sfd_maps_batch", "float_sfd_post_batch", "float_sfd_detect_batch", "float_sfd_dense_batch")


def test_batch_symbols_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    declared = set(re.findall(r"\b(float_[a-z_0-9]+)\s*\(", hdr))
    L = pkg.native.lib()
    for name in BATCH_SYMBOLS:
        assert name in declared and name in pkg.native.EXPORTS and hasattr(L, name), name
    assert L.float_hip_abi_version() == 6 and pkg.native.ABI_VERSION == 6  # new symbols only


def test_batch_argument_checks_need_no_gpu():
    """Every batched call refuses before any HIP call, and the message names the function and the argument."""
    L = pkg.native.lib()
    buf = (C.c_float * 16)()
    calls = {
        "float_sfd_reserve_batch": lambda n, H, W: L.float_sfd_reserve_batch(None, n, H, W),
        "float_sfd_maps_batch": lambda n, H, W: L.float_sfd_maps_batch(None, buf, n, H, W, buf, None),
        "float_sfd_post_batch": lambda n, H, W: L.float_sfd_post_batch(None, buf, n, H, W, 0.5, 0.3, buf, buf, None),
        "float_sfd_detect_batch": lambda n, H, W: L.float_sfd_detect_batch(None, buf, n, H, W, 0.5, 0.3, buf, buf, None),
    }
    for name, call in calls.items():
        for n in (0, 65, -1):
            assert call(n, 64, 64) == 1
            msg = L.float_last_error()
            assert name.encode() in msg and b"n = %d" % n in msg and b"1 ... 64" in msg, msg
        assert call(2, 15, 64) == 1 and name.encode() in L.float_last_error() and b"15 x 64" in L.float_last_error()
        assert call(2, 64, 4097) == 1 and b"4097" in L.float_last_error()
        assert call(2, 64, 64) == 1 and name.encode() in L.float_last_error() and b"null handle" in L.float_last_error()
    assert L.float_sfd_dense_batch(None, buf, None) == 1 and b"float_sfd_dense_batch" in L.float_last_error()
    assert b"null argument" in L.float_last_error()


class _StubLib:
    """float_sfd_reserve_batch / float_sfd_detect_batch that record their n and do nothing."""

    def __init__(self):
        self.reserved, self.detected = [], []

    def float_sfd_reserve_batch(self, h, n, H, W):
        self.reserved.append((n, H, W))
        return 0

    def float_sfd_detect_batch(self, h, rgb8, n, H, W, score_thr, iou_thr, boxes, counts, stream):
        self.detected.append((n, H, W, rgb8.value))
        return 0


def test_detect_batch_groups_views_by_max_batch(monkeypatch):
    """5 views with max_batch=2 go through 2 / 2 / 1, each group starting where the last ended, with one reservation (the
    largest group) and one read-back per group.  The detector object is built without a handle; buffers live on the CPU."""
    face = pkg.face
    stub = _StubLib()
    monkeypatch.setattr(face.native, "lib", lambda: stub)
    monkeypatch.setattr(face.native, "stream_ptr", lambda device: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    det = object.__new__(face.FaceDetectorHIP)
    det.device, det.max_boxes, det.max_candidates, det.fallbacks = torch.device("cpu"), 4, 16, 0
    det._h, det._reserved, det._bboxes, det._bcounts, det._last_counts = None, (0, 0, 0), None, None, []
    views = torch.zeros(5, 16, 20, 3, dtype=torch.uint8)
    out = det.detect_batch(views, max_batch=2)
    assert out == [[], [], [], [], []] and det.counts_batch() == [(0, 0)] * 5
    assert [d[:3] for d in stub.detected] == [(2, 16, 20), (2, 16, 20), (1, 16, 20)]
    step = 2 * 16 * 20 * 3
    base = stub.detected[0][3]
    assert [d[3] - base for d in stub.detected] == [0, step, 2 * step]
    assert stub.reserved == [(2, 16, 20)]
    with pytest.raises(ValueError):
        det.detect_batch(torch.zeros(16, 20, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        det.detect_batch(torch.zeros(2, 16, 20, 3))
    det._h = None  # nothing for __del__ to release
