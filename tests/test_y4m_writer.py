"""host_models.Y4MWriter: a Y4M stream written block by block is, byte for byte, write_y4m of the whole clip."""
import io

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
H = pkg.host_models
R, T = 8, 65
HEADER = b"YUV4MPEG2 W8 H8 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"


def _clip():
    rgb = torch.from_numpy(np.random.RandomState(11).randint(0, 256, size=(T, R, R, 3)).astype(np.uint8))
    return H.rgb8_to_i420(rgb)


def _whole(frames, fps=25):
    f = io.BytesIO()
    H.write_y4m(f, frames, fps)
    return f.getvalue()


def test_blocks_of_50_and_15_frames_are_the_whole_clip_file_object():
    frames = _clip()
    want = _whole(frames)
    f = io.BytesIO()
    with H.Y4MWriter(f, R, R, 25) as w:
        assert f.getvalue() == HEADER  # the header goes out when the writer is made
        assert w.write(frames[:50]) == 50
        assert w.write(frames[50:]) == T and w.frames == T
    assert not f.closed  # a file the caller opened stays open
    got = f.getvalue()
    assert got == want
    assert got.count(b"YUV4MPEG2") == 1 and got.startswith(HEADER)
    assert len(got) == len(HEADER) + T * (6 + 3 * R * R // 2)
    with pytest.raises(ValueError, match="after close"):
        w.write(frames[:1])


def test_blocks_of_50_and_15_frames_are_the_whole_clip_path(tmp_path):
    frames = _clip()
    p, q = tmp_path / "blocks.y4m", tmp_path / "whole.y4m"
    w = H.Y4MWriter(str(p), R, R, 25)
    w.write(frames[:50])
    w.write(frames[50:])
    w.close()  # a file the writer opened is closed by it: everything is on disk and the path can be opened again
    assert p.read_bytes() == _whole(frames)
    w.close()  # twice is harmless
    with pytest.raises(ValueError, match="after close"):
        w.write(frames[:1])
    with open(str(p), "ab") as again:
        again.write(b"")
    H.write_y4m(str(q), frames, 25)
    assert p.read_bytes() == q.read_bytes() == _whole(frames)


def test_a_view_of_a_larger_buffer_and_an_empty_block():
    """What a stream's short last block is: a prefix view of a ring slot."""
    frames = _clip()
    slot = torch.zeros(50, 3 * R // 2, R, dtype=torch.uint8)
    slot[:15] = frames[50:]
    f = io.BytesIO()
    with H.Y4MWriter(f, R, R, 25) as w:
        w.write(frames[:50])
        w.write(slot[:0])
        w.write(slot[:15])
    assert f.getvalue() == _whole(frames)


def test_mis_shaped_frames_are_refused():
    f = io.BytesIO()
    with H.Y4MWriter(f, R, R, 25) as w:
        for bad in (torch.zeros(2, R, R, 3, dtype=torch.uint8),            # RGB
                    torch.zeros(2, 3 * R // 2, R),                          # fp32
                    torch.zeros(3 * R // 2, R, dtype=torch.uint8),          # one frame without the leading axis
                    torch.zeros(2, 3 * R // 2, R + 2, dtype=torch.uint8),   # another width
                    torch.zeros(2, 3 * (R + 2) // 2, R, dtype=torch.uint8)):
            with pytest.raises(ValueError, match="I420"):
                w.write(bad)
    assert f.getvalue() == HEADER  # nothing of a refused block was written
    for w_, h_ in ((7, 8), (8, 7), (0, 8)):
        with pytest.raises(ValueError, match="even"):
            H.Y4MWriter(io.BytesIO(), w_, h_, 25)


def test_ntsc_rate_and_non_square_frames():
    f = io.BytesIO()
    with H.Y4MWriter(f, 16, 8, 29.97) as w:
        w.write(torch.full((1, 12, 16), 128, dtype=torch.uint8))
    assert f.getvalue().startswith(b"YUV4MPEG2 W16 H8 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\nFRAME\n")
    assert _whole(_clip()[:2], 29.97).startswith(b"YUV4MPEG2 W8 H8 F30000:1001 ")
