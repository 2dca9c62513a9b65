"""The format rules of a hand-over call, as a table: pipeline.resolve_out_format and the one function that infers "rgb" / "i420"
from the destination tensor (decoder.infer_out_format, which resolve_out_format and SynthesisHIP.decode_into_host both call).
Every combination of `out` (None, fp32 4-d, uint8 4-d, uint8 3-d), `out_dtype` (None, fp32, uint8) and `out_format` (None, "rgb",
"i420").  The expected column was recorded from resolve_out_format as it stood before the rule moved into decoder.py: a
(dtype, format) pair, or the words of the ValueError."""
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
OUTS = {None: None, "f32_4d": torch.empty(2, 4, 4, 3), "u8_4d": torch.empty(2, 4, 4, 3, dtype=torch.uint8),
        "u8_3d": torch.empty(2, 6, 4, dtype=torch.uint8)}
F32, U8 = torch.float32, torch.uint8
E_I420 = "I420 frames are uint8: out_format='i420' contradicts torch.float32"
E_F32_U8 = "out is torch.float32 but out_dtype asks for torch.uint8"
E_U8_F32 = "out is torch.uint8 but out_dtype asks for torch.float32"
E_4D = "out has 4 dimensions, out_format 'i420' takes (T, 3R/2, R)"
E_3D = "out has 3 dimensions, out_format 'rgb' takes (T, R, R, 3)"
TABLE = [
    (None, None, None, (F32, "rgb")), (None, None, "rgb", (F32, "rgb")), (None, None, "i420", (U8, "i420")),
    (None, F32, None, (F32, "rgb")), (None, F32, "rgb", (F32, "rgb")), (None, F32, "i420", E_I420),
    (None, U8, None, (U8, "rgb")), (None, U8, "rgb", (U8, "rgb")), (None, U8, "i420", (U8, "i420")),
    ("f32_4d", None, None, (F32, "rgb")), ("f32_4d", None, "rgb", (F32, "rgb")), ("f32_4d", None, "i420", E_I420),
    ("f32_4d", F32, None, (F32, "rgb")), ("f32_4d", F32, "rgb", (F32, "rgb")), ("f32_4d", F32, "i420", E_I420),
    ("f32_4d", U8, None, E_F32_U8), ("f32_4d", U8, "rgb", E_F32_U8), ("f32_4d", U8, "i420", E_F32_U8),
    ("u8_4d", None, None, (U8, "rgb")), ("u8_4d", None, "rgb", (U8, "rgb")), ("u8_4d", None, "i420", E_4D),
    ("u8_4d", F32, None, E_U8_F32), ("u8_4d", F32, "rgb", E_U8_F32), ("u8_4d", F32, "i420", E_U8_F32),
    ("u8_4d", U8, None, (U8, "rgb")), ("u8_4d", U8, "rgb", (U8, "rgb")), ("u8_4d", U8, "i420", E_4D),
    ("u8_3d", None, None, (U8, "i420")), ("u8_3d", None, "rgb", E_3D), ("u8_3d", None, "i420", (U8, "i420")),
    ("u8_3d", F32, None, E_U8_F32), ("u8_3d", F32, "rgb", E_U8_F32), ("u8_3d", F32, "i420", E_U8_F32),
    ("u8_3d", U8, None, (U8, "i420")), ("u8_3d", U8, "rgb", E_3D), ("u8_3d", U8, "i420", (U8, "i420")),
]


def test_the_table_is_complete():
    assert len(TABLE) == len({row[:3] for row in TABLE}) == 4 * 3 * 3


@pytest.mark.parametrize("out,out_dtype,out_format,want", TABLE)
def test_resolve_out_format(out, out_dtype, out_format, want):
    if isinstance(want, str):
        with pytest.raises(ValueError) as e:
            pkg.pipeline.resolve_out_format(OUTS[out], out_dtype, out_format)
        assert str(e.value) == want
    else:
        assert pkg.pipeline.resolve_out_format(OUTS[out], out_dtype, out_format) == want


@pytest.mark.parametrize("out,out_dtype,out_format,want", [row for row in TABLE if row[3] not in (E_F32_U8, E_U8_F32)])
def test_infer_out_format(out, out_dtype, out_format, want):
    """The inference alone, on the rows where `out` and `out_dtype` agree (that contradiction is resolve_out_format's own check),
    with the dtype the hand-over has: the tensor's, or (no tensor) the one resolve_out_format settles on.  It gives the table's
    format and the table's I420 refusal; whether a tensor has the number of dimensions of a STATED format is the callers' shape
    check, so there the stated format comes back."""
    t = OUTS[out]
    dtype = out_dtype if out_dtype is not None else (U8 if out_format == "i420" else F32)
    if want == E_I420:
        with pytest.raises(ValueError, match="I420") as e:
            pkg.decoder.infer_out_format(t, out_format, dtype)
        assert str(e.value) == want
    else:
        assert pkg.decoder.infer_out_format(t, out_format, dtype) == (out_format if want in (E_4D, E_3D) else want[1])


def test_an_unknown_format_is_refused():
    for fn in (lambda: pkg.pipeline.resolve_out_format(None, None, "nv12"), lambda: pkg.decoder.infer_out_format(None, "nv12", U8)):
        with pytest.raises(ValueError, match="out_format must be None, 'rgb' or 'i420'"):
            fn()
