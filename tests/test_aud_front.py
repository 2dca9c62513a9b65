"""The audio front end on the device (float_aud_front), the part that needs no GPU: the three entry points on both sides of
the boundary, the argument rules (refused before the device is touched), the output length in exact integers, and the
definition the kernels are held to - host_models.resample_sinc_direct, the closed form of what resample_sinc computes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.util import ROOT, load_pkg

pkg = load_pkg()
hm = pkg.host_models
NEW = ("float_aud_front", "float_aud_front_len", "float_aud_front_work_bytes")


def test_front_entry_points_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    declared = set(re.findall(r"\b(float_[a-z_0-9]+)\s*\(", hdr))
    L = pkg.native.lib()
    for name in NEW:
        assert name in pkg.native.EXPORTS and name in declared
        assert hasattr(L, name)
    assert "FLOAT_AUD_FRONT_NORMALIZE = 1" in hdr and pkg.native.AUD_FRONT_NORMALIZE == 1
    assert L.float_hip_abi_version() == pkg.native.ABI_VERSION == 6  # new symbols only: the version does not move


def _call(L, buf, **kw):
    """float_aud_front with valid host-side arguments for 441 samples of 44.1 kHz stereo, `kw` overriding some: every case
    below must be refused before the device is touched (the buffers are host memory)."""
    n_in, ri, ro = kw.get("n_in", 441), kw.get("rate_in", 44100), kw.get("rate_out", 16000)
    a = dict(w=buf, channels=2, ch_stride=n_in, n_in=n_in, rate_in=ri, rate_out=ro, zeros=24, rolloff=0.945, flags=1, a=buf,
             n_out=int(L.float_aud_front_len(n_in, ri, ro)), work=buf, work_bytes=int(L.float_aud_front_work_bytes(n_in, ri, ro)),
             stream=None)
    a.update(kw)
    p = lambda v: None if v is None else C.cast(v, C.c_void_p)  # noqa: E731
    rc = L.float_aud_front(p(a["w"]), a["channels"], a["ch_stride"], a["n_in"], a["rate_in"], a["rate_out"], a["zeros"],
                           a["rolloff"], a["flags"], p(a["a"]), a["n_out"], p(a["work"]), a["work_bytes"], a["stream"])
    return rc, L.float_last_error()


def test_front_refuses_bad_arguments_without_a_gpu():
    L = pkg.native.lib()
    buf = (C.c_double * 1024)()
    assert L.float_aud_front_len(441, 44100, 16000) == 160 and L.float_aud_front_work_bytes(441, 44100, 16000) > 0
    for kw, word in (({"w": None}, b"null argument"), ({"a": None}, b"null argument"), ({"work": None}, b"null argument"),
                     ({"channels": 0}, b"channels"), ({"channels": 9}, b"channels"),
                     ({"zeros": 0}, b"zeros"), ({"zeros": 33}, b"zeros"),
                     ({"rolloff": 0.0}, b"rolloff"), ({"rolloff": 1.5}, b"rolloff"),
                     ({"rate_in": 0, "n_out": 160, "work_bytes": 64}, b"rate_in"),
                     ({"rate_out": 0, "n_out": 160, "work_bytes": 64}, b"rate_out"),
                     ({"rate_in": (1 << 20) + 1, "n_out": 160, "work_bytes": 64}, b"rate_in"),
                     ({"n_in": 0, "n_out": 160, "work_bytes": 64}, b"n_in"),
                     ({"n_out": 161}, b"n_out"), ({"n_out": 159}, b"n_out"),
                     ({"ch_stride": 440}, b"ch_stride"),
                     ({"flags": 2}, b"flags"),
                     ({"work_bytes": int(L.float_aud_front_work_bytes(441, 44100, 16000)) - 1}, b"work_bytes"),
                     ({"work_bytes": 0}, b"work_bytes"),
                     # a tile the LDS cannot hold: 256 outputs of a 64 : 1 decimation with a cut-off at a tenth of Nyquist
                     ({"rate_in": 1024000, "rolloff": 0.1, "n_in": 64000, "ch_stride": 64000}, b"LDS")):
        rc, msg = _call(L, buf, **kw)
        assert rc == 1, (kw, rc)  # FLOAT_E_INVALID
        assert b"float_aud_front" in msg and word in msg, (kw, msg)
    with pytest.raises(ValueError, match="float_aud_front"):
        pkg.native.check(1)


RATES = [(48000, 16000), (44100, 16000), (44099, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (16000, 16000), (44100, 16001)]


def test_front_len_is_the_exact_ceiling():
    L = pkg.native.lib()
    for ri, ro in RATES:
        g = math.gcd(ri, ro)
        up, down = ro // g, ri // g
        for n in (1, 7, 441, 442, 160001, 14112000):
            assert L.float_aud_front_len(n, ri, ro) == -((-n * up) // down), (n, ri, ro)
            tiles = -(-L.float_aud_front_len(n, ri, ro) // 256)
            assert L.float_aud_front_work_bytes(n, ri, ro) == 8 * (2 + 2 * tiles)
    for args in ((441, 0, 16000), (441, 44100, 0), (0, 44100, 16000), (-1, 44100, 16000), (441, (1 << 20) + 1, 16000)):
        assert L.float_aud_front_len(*args) == 0 and L.float_aud_front_work_bytes(*args) == 0


@pytest.mark.parametrize("src", [48000, 44100, 32000, 22050, 8000])
def test_resample_sinc_direct_is_the_closed_form_of_resample_sinc(src):
    w = torch.from_numpy(np.random.RandomState(src).standard_normal(src // 5)).double()  # 0.2 s of noise
    want = hm.resample_sinc(w, src, 16000)
    got = hm.resample_sinc_direct(w, src, 16000)
    assert got.dtype == torch.float64 and got.shape == want.shape
    err = float((got - want).abs().max())
    print("%d -> 16000: max |direct - polyphase| %.3g" % (src, err))
    assert err <= 1e-12


def test_resample_sinc_direct_edges():
    w = torch.from_numpy(np.random.RandomState(1).standard_normal(100))
    assert hm.resample_sinc_direct(w, 16000, 16000) is w  # equal rates: the input itself
    # near-coprime rates are served as they are (resample_sinc snaps them): the lengths follow the exact ceiling
    assert hm.resample_sinc_direct(w, 44099, 16000).shape[0] == -((-100 * 16000) // 44099)
    assert hm.resample_sinc_direct(w, 44100, 16001).shape[0] == -((-100 * 16001) // 44100)
    # a band-limited tone keeps its amplitude and phase through 44099 -> 16000 (what the snapped route only approximates)
    n = 8820
    tone = torch.sin(2 * math.pi * 440.0 * torch.arange(n, dtype=torch.float64) / 44099.0)
    y = hm.resample_sinc_direct(tone, 44099, 16000)
    m = torch.arange(y.shape[0], dtype=torch.float64)
    mid = slice(200, y.shape[0] - 200)
    assert float((y - torch.sin(2 * math.pi * 440.0 * m / 16000.0))[mid].abs().max()) < 1e-3
