"""Pasted frames as planar YUV 4:2:0 (float_img_paste_i420), the part that needs no GPU: the definition host_models.paste_i420 =
rgb8_to_i420(paste_rgb8(...)), the entry point's argument rules on both sides of the boundary, and the Y4M writer at a size that
is not square.  Everything is integers: comparisons are torch.equal, there is no tolerance in this file."""
import ctypes as C
import inspect
import io
import os
import re

import numpy as np
import pytest
import torch

from tests.util import ROOT, load_pkg

pkg = load_pkg()
hm = pkg.host_models
NAME = "float_img_paste_i420"


def noise(seed, *shape):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------
CASES = (((34, 50), 3, (7, 5, 21, 19), 4), ((36, 40), 2, (5, 3, 16, 12), 2), ((90, 68), 2, (-13, 21, 37, 37), 7),
         ((12, 18), 2, (40, 40, 4, 4), 3), ((2, 2), 3, (-1, -1, 4, 4), 0))


@pytest.mark.parametrize("src_hw,T,rect,feather", CASES)
def test_paste_i420_is_the_composition(src_hw, T, rect, feather):
    src, frames = noise(1, *src_hw, 3), noise(2, T, 16, 16, 3)
    got = hm.paste_i420(src, frames, rect, feather)
    H, W = src_hw
    assert got.dtype == torch.uint8 and tuple(got.shape) == (T, 3 * H // 2, W)
    assert torch.equal(got, hm.rgb8_to_i420(hm.paste_rgb8(src, frames, rect, feather)))


def test_chroma_is_the_mean_of_pasted_pixels_not_a_blend_of_chroma():
    """Written out per sample in Python integers for the case whose 2 x 2 blocks straddle all four box edges and the feather."""
    (H, W), T, rect, feather = CASES[0]
    src, frames = noise(1, H, W, 3), noise(2, T, 16, 16, 3)
    rgb = hm.paste_rgb8(src, frames, rect, feather).numpy().astype(np.int64)
    got = hm.paste_i420(src, frames, rect, feather).reshape(T, -1).numpy()
    assert rect[0] % 2 == 1 and rect[1] % 2 == 1 and (rect[0] + rect[2]) % 2 == 0 and (rect[1] + rect[3]) % 2 == 0  # odd offsets: blocks straddle
    for t in range(T):
        for y in range(H):
            for x in range(W):
                r, g, b = (int(v) for v in rgb[t, y, x])
                assert got[t, y * W + x] == ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
        for by in range(H // 2):
            for bx in range(W // 2):
                m = [(int(rgb[t, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2, c].sum()) + 2) >> 2 for c in range(3)]
                at = by * (W // 2) + bx
                assert got[t, H * W + at] == ((-38 * m[0] - 74 * m[1] + 112 * m[2] + 128) >> 8) + 128
                assert got[t, H * W + (H // 2) * (W // 2) + at] == ((112 * m[0] - 94 * m[1] - 18 * m[2] + 128) >> 8) + 128


@pytest.mark.parametrize("src_hw", [(33, 50), (34, 51), (1, 1), (35, 35)])
def test_paste_i420_refuses_odd_sides(src_hw):
    with pytest.raises(ValueError) as e:
        hm.paste_i420(noise(1, *src_hw, 3), noise(2, 1, 16, 16, 3), (0, 0, 4, 4), 0)
    assert "even" in str(e.value) and "%d x %d" % src_hw in str(e.value)
    assert tuple(hm.paste_rgb8(noise(1, *src_hw, 3), noise(2, 1, 16, 16, 3), (0, 0, 4, 4), 0).shape) == (1,) + src_hw + (3,)  # RGB takes it


# ---------------------------------------------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_declared_and_does_not_move_the_version():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % NAME, hdr)
    assert m, "float_img_paste_i420 is not declared in float_hip.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    res, args = pkg.native._SIGNATURES[NAME]
    assert NAME in pkg.native.EXPORTS and res is C.c_int and len(args) == n_args == 15
    assert "FLOAT_IMG_MATRIX_BT601_LIMITED = 0" in hdr and pkg.native.IMG_MATRIX_BT601_LIMITED == 0
    assert "FLOAT_DEC_MATRIX_BT601_LIMITED = 0" in hdr and pkg.native.MATRIX_BT601_LIMITED == 0  # the decoder's enum is its own
    L = pkg.native.lib()
    assert hasattr(L, NAME) and L.float_hip_abi_version() == pkg.native.ABI_VERSION == 6


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    """Every rule is checked before any HIP call: status 1 and a message naming the function and the argument."""
    L = pkg.native.lib()
    buf = (C.c_uint8 * 64)()
    p = C.c_void_p(C.addressof(buf))  # never dereferenced: every call below fails validation

    def call(src_hw=(34, 50), T=2, fr=(64, 64), rect=(7, 5, 21, 19), feather=4, matrix=0, src=p, frames=p, out=p):
        rc = L.float_img_paste_i420(src, src_hw[0], src_hw[1], frames, T, fr[0], fr[1], *rect, feather, matrix, out, None)
        return rc, L.float_last_error().decode("utf-8", "replace")

    for kw, word in ((dict(src=None), "null"), (dict(frames=None), "null"), (dict(out=None), "null"),
                     (dict(src_hw=(33, 50)), "src_h"), (dict(src_hw=(34, 51)), "src_w"), (dict(src_hw=(0, 50)), "src_h"),
                     (dict(src_hw=(34, 0)), "src_w"), (dict(src_hw=(1, 1)), "src_h"), (dict(matrix=1), "matrix"), (dict(matrix=-1), "matrix"),
                     # the limits shared with float_img_paste
                     (dict(src_hw=(16386, 50)), "src_h"), (dict(src_hw=(34, 16386)), "src_w"), (dict(T=0), "n_frames"),
                     (dict(fr=(1025, 64)), "fr_h"), (dict(fr=(64, 0)), "fr_w"), (dict(rect=(7, 5, 0, 19)), "rect_w"),
                     (dict(rect=(7, 5, 21, 16385)), "rect_h"), (dict(rect=((1 << 30) + 1, 5, 21, 19)), "rect_x"),
                     (dict(rect=(7, -(1 << 30) - 1, 21, 19)), "rect_y"), (dict(feather=-1), "feather"), (dict(feather=16385), "feather")):
        rc, msg = call(**kw)
        assert rc == 1 and NAME in msg and word in msg, (kw, rc, msg)
    for kw in (dict(src_hw=(33, 50)), dict(src_hw=(34, 51))):
        assert "even" in call(**kw)[1]
    with pytest.raises(ValueError) as e:
        pkg.native.check(call(matrix=709)[0])
    assert "matrix" in str(e.value)


def test_python_layers_take_out_format_and_keep_their_defaults():
    gen = __import__("importlib").import_module(pkg.__name__ + ".src.nodes.generate")
    for fn in (pkg.image.paste_frames_device, pkg.pipeline.FloatHotPath.generate_pasted, pkg.pipeline.FloatHotPath.stream_to_host_pasted,
               gen.InferenceAgent.infer_pasted, gen.InferenceAgent.stream_pasted):
        assert inspect.signature(fn).parameters["out_format"].default is None, fn
    sig = inspect.signature(gen.InferenceAgent.write_y4m)
    assert list(sig.parameters)[1:] == ["path_or_file", "ref_img", "ref_audio", "a_cfg_scale", "r_cfg_scale", "e_cfg_scale", "emo", "no_crop",
                                        "seed", "fps", "paste_back", "feather", "slots"]
    assert "audio" in gen.InferenceAgent.write_y4m.__doc__.lower()
    assert pkg.image.paste_format("x", None) == pkg.image.paste_format("x", "rgb") == "rgb" and pkg.image.paste_format("x", "i420") == "i420"
    with pytest.raises(ValueError):
        pkg.image.paste_format("x", "nv12")
    with pytest.raises(ValueError) as e:
        pkg.image.require_even_sides("x", 90, 67)
    assert "even" in str(e.value) and "90 x 67" in str(e.value)
    pkg.image.require_even_sides("x", 1080, 1920)


# ---------------------------------------------------------------------------------------------------------------------------
# the Y4M writer at a size that is not square
# ---------------------------------------------------------------------------------------------------------------------------
def test_y4m_writer_at_50_by_34():
    src, frames = noise(1, 34, 50, 3), noise(2, 3, 16, 16, 3)
    i420 = hm.paste_i420(src, frames, (7, 5, 21, 19), 4)
    f = io.BytesIO()
    with hm.Y4MWriter(f, 50, 34, 25) as w:
        assert w.write(i420[:2]) == 2 and w.write(i420[2:]) == 3
    data = f.getvalue()
    header, _, rest = data.partition(b"\n")
    assert header.split()[:4] == [b"YUV4MPEG2", b"W50", b"H34", b"F25:1"] and b"C420jpeg" in header
    assert 50 * 34 * 3 // 2 == 2550 and len(rest) == 3 * (len(b"FRAME\n") + 2550)
    for t in range(3):
        chunk = rest[t * 2556:(t + 1) * 2556]
        assert chunk[:6] == b"FRAME\n" and chunk[6:] == i420[t].numpy().tobytes()
    with pytest.raises(ValueError):
        hm.Y4MWriter(io.BytesIO(), 67, 90, 25)
