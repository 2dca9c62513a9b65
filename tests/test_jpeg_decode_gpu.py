"""float_jpg_decode against its definition, host_models.jpeg_decode_rgb8: bitwise, on the files of tests/test_jpeg_decode.py."""
import io

import numpy as np
import pytest
import torch

from tests.test_jpeg_decode import SIZES, case_files, image, pil_file
from tests.test_drive_video_gpu import _agent
from tests.util import load_pkg

pkg = load_pkg()
hm, J = pkg.host_models, pkg.jpeg
pytestmark = pytest.mark.gpu


def definition(files):
    return torch.from_numpy(np.stack([hm.jpeg_decode_rgb8(f) for f in files]))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("sub", ["4:4:4", "4:2:2", "4:2:0", "grey"])
def test_decode_is_the_definition(sub, size):
    files = case_files(sub, size)  # one call: eight frames whose table sets and restart intervals differ
    got, status = J.decode_jpeg_device(files, return_status=True)
    assert status.tolist() == [0] * len(files) and torch.equal(got.cpu(), definition(files))


def test_more_frames_than_a_group_and_two_calls_agree():
    files = [pil_file(33, 47, "4:2:0", 25 + 3 * i, ("row", None, "mcu")[i % 3]) for i in range(19)]  # frames 1, 4, ... have no restart markers
    a, b = J.decode_jpeg_device(files), J.decode_jpeg_device(files)
    assert torch.equal(a, b) and torch.equal(a.cpu(), definition(files))


@pytest.mark.parametrize("restart", [None, 0])
def test_device_round_trip(restart):
    x = torch.from_numpy(np.stack([image(48, 64), image(48, 64)[::-1].copy()])).cuda()
    data, offsets = J.encode_jpeg_device(x, 90, restart)
    files = hm.jpeg_encode_rgb8(x, 90, restart)
    assert torch.equal(J.decode_jpeg_device(data, offsets).cpu(), definition(files))


@pytest.mark.parametrize("restart", [None, "row"])
def test_truncated_scan_gets_the_definitions_pixels_and_a_status(restart):
    f = pil_file(48, 64, "4:2:0", 90, restart)
    hdr = hm.jpeg_parse_header(f)
    cut = f[:hdr["scan_start"] + (hdr["scan_end"] - hdr["scan_start"]) // 2]
    want, st = hm.jpeg_decode_rgb8(cut, status=True)
    got, status = J.decode_jpeg_device([f, cut], strict=False, return_status=True)
    assert st != 0 and status.tolist() == [0, st] and torch.equal(got[1].cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError, match="frame 1 is damaged"):
        J.decode_jpeg_device([f, cut])


def test_align_driving_from_an_mjpeg_avi():
    T, rects = 20, [(5 + t, 2 + t, 40, 40) for t in range(20)]
    video = torch.from_numpy(np.stack([np.roll(image(48, 64), 2 * t, axis=1) for t in range(T)]))
    files = hm.jpeg_encode_rgb8(video, 90)
    buf = io.BytesIO()
    with hm.AviMjpegWriter(buf, 64, 48, 25) as w:
        w.write(files)
    agent = _agent()
    got, r = agent.align_driving(hm.AviMjpegReader(io.BytesIO(buf.getvalue())), rects=rects, chunk=7)
    want, _ = agent.align_driving(definition(files), rects=rects, chunk=7)
    assert r == rects and torch.equal(got, want)
