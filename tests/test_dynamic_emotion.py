"""Dynamic emotion, the host definitions and the C ABI's refusals (no GPU): host_models.nearest_rows is torch's
F.interpolate(mode="nearest") bitwise, host_models.dynamic_emotion_plan is the arithmetic of the reference's
FloatExtractEmotionWithCustomModelDyn node, and float_aud_reserve_segments / float_aud_classify_segments / float_aud_expand_rows
refuse bad arguments before any HIP call.  The refusals that need a handle (no classification head, a GroupNorm extractor, a
segment below the receptive field, too many frames) are in tests/test_dynamic_emotion_gpu.py: a handle cannot exist without a
device."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import load_pkg

pkg = load_pkg()
HM = pkg.host_models

T_VALUES = list(range(1, 400)) + [749, 750, 751, 1499, 1500, 1501, 2999, 3000, 4501]


def test_nearest_rows_is_torch_nearest_bitwise():
    g = torch.Generator().manual_seed(3)
    for n in range(2, 65):
        seq = torch.randn(2, n, 7, generator=g)
        for T in T_VALUES:
            want = F.interpolate(seq.transpose(1, 2), size=T, mode="nearest").transpose(1, 2)
            got = HM.nearest_rows(seq, T)
            assert got.shape == (2, T, 7) and torch.equal(got, want), (n, T)
    # the exact integer form is NOT torch's rule, e.g. at (2, 82): why the fp32 form is the definition
    seq = torch.randn(1, 2, 7, generator=g)
    assert not torch.equal(seq[:, [t * 2 // 82 for t in range(82)]], HM.nearest_rows(seq, 82))


def test_nearest_rows_single_row_repeats():
    seq = torch.randn(3, 1, 7, generator=torch.Generator().manual_seed(4))
    for T in (1, 2, 113):
        assert torch.equal(HM.nearest_rows(seq, T), seq.repeat(1, T, 1))
    assert torch.equal(HM.nearest_rows(seq[0], 5), seq[0].repeat(5, 1))  # (n, C) without a batch axis


@pytest.mark.parametrize("n_samples,chunk_sec,fps", [(160000, 2.0, 25), (161234, 2.0, 25), (47999, 0.7, 29.97), (300, 2.0, 25)])
def test_dynamic_emotion_plan_is_the_nodes_arithmetic(n_samples, chunk_sec, fps):
    sr = 16000
    chunk = int(chunk_sec * sr)  # the node: nodes_vadv.py, extract_dynamic_emotion
    n_chunks = math.ceil(n_samples / chunk)
    T = math.ceil(n_samples / sr * fps)
    got = HM.dynamic_emotion_plan(n_samples, sr, chunk_sec, fps)
    assert got == (chunk, n_chunks, n_samples - (n_chunks - 1) * chunk, T)
    assert 1 <= got[2] <= chunk and (n_chunks - 1) * chunk + got[2] == n_samples


def test_dynamic_emotion_plan_refuses_an_empty_chunk():
    with pytest.raises(ValueError):
        HM.dynamic_emotion_plan(16000, 16000, 1e-5, 25)


def test_dynamic_emotion_request_parsing():
    f = HM.dynamic_emotion_chunk_sec
    assert f("dynamic", 2.0) == 2.0 and f("Dynamic", 1.5) == 1.5 and f(("dynamic", 1), 2.0) == 1.0
    for emo in (None, "none", "S2E", "happy", ("happy", 1.0), ("dynamic",), 3, ["dynamic", 0.5]):  # a list: one emo per item
        assert f(emo) is None, emo
    assert HM.emotion_index("dynamic") is None


def test_segment_calls_refuse_without_a_gpu():
    """The refusals that do not need a handle come first, so they can be seen with a NULL handle; then the NULL handle itself."""
    L = pkg.native.lib()
    h, p = None, C.c_void_p(16)  # p: never dereferenced, every call below returns before any HIP call
    assert L.float_aud_reserve_segments(h, 0, 32000, None) == 1 and b"n_seg" in L.float_last_error()
    assert L.float_aud_reserve_segments(h, 2, 32000, None) == 1 and b"null audio handle" in L.float_last_error()
    assert b"float_aud_reserve_segments" in L.float_last_error()
    assert L.float_aud_classify_segments(h, p, 0, 32000, 32000, 1, p, None, 0, 0.0, None) == 1 and b"n_seg" in L.float_last_error()
    assert L.float_aud_classify_segments(h, p, 2, 32000, 31999, 1, p, None, 0, 0.0, None) == 1 and b"seg_stride" in L.float_last_error()
    assert L.float_aud_classify_segments(h, p, 2, 32000, 32000, 1, p, p, 0, 0.0, None) == 1 and b"T must be" in L.float_last_error()
    assert L.float_aud_classify_segments(h, p, 2, 32000, 32000, 4, p, None, 0, 0.0, None) == 1 and b"flags" in L.float_last_error()
    assert L.float_aud_classify_segments(h, p, 2, 32000, 32000, 1, p, None, 0, 0.0, None) == 1 and b"null audio handle" in L.float_last_error()
    assert L.float_aud_expand_rows(p, 0, 7, p, 10, 0.0, None) == 1 and b"float_aud_expand_rows" in L.float_last_error()
    assert L.float_aud_expand_rows(p, 2, 7, p, 0, 0.0, None) == 1
    assert L.float_aud_expand_rows(None, 2, 7, p, 10, 0.2, None) == 1 and b"null argument" in L.float_last_error()
    assert L.float_aud_debug(None, 2, None, 4, None, None) == 1
    with pytest.raises(ValueError):
        pkg.native.check(L.float_aud_reserve_segments(h, 0, 32000, None))
