"""The split entropy route of float_jpg_decode against the definition, host_models.jpeg_decode_rgb8: bitwise, pixels and status."""
import numpy as np
import pytest
import torch

from tests.test_jpeg_decode import J, hm, image, pil_file
from tests.test_jpeg_split import CASES, SUBS, case_files, damaged

pytestmark = pytest.mark.gpu


def definition(files):
    both = [hm.jpeg_decode_rgb8(f, status=True) for f in files]
    return torch.from_numpy(np.stack([rgb for rgb, _ in both])), [st for _, st in both]


@pytest.mark.parametrize("S", [1, 8, None])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sub", SUBS)
def test_split_route_is_the_definition(sub, case, S):
    files = case_files(sub, case)
    got, status = J.decode_jpeg_device(files, entropy="split", sync_bytes=S, return_status=True)
    want, st = definition(files)
    assert status.tolist() == st == [0, 0] and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("h,w,sub", [(33, 47, "4:2:0"), (200, 200, "4:4:4")])  # a marker per MCU: 9 intervals, split; 625, a lane each
def test_mixed_files_in_one_call_of_more_than_a_group(h, w, sub):
    kws = ({"restart_marker_rows": 2}, {}, {"restart_marker_blocks": 1})
    files = [pil_file(h, w, sub, 25 + 3 * i, None, **kws[i % 3]) for i in range(19)]
    got, status = J.decode_jpeg_device(files, entropy="split", return_status=True)
    want, st = definition(files)
    assert status.tolist() == st and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("S", [8, None])
def test_damaged_scans(S):
    files = damaged()
    got, status = J.decode_jpeg_device(files, strict=False, entropy="split", sync_bytes=S, return_status=True)
    want, st = definition(files)
    assert st[0] and st[2] and st[3] == hm.JPEG_DEC_BAD_CODE and status.tolist() == st and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("restart", [0, 1])
def test_device_files_of_the_own_encoder(restart):
    x = torch.from_numpy(np.stack([image(48, 64), image(48, 64)[::-1].copy()])).cuda()
    data, offsets = J.encode_jpeg_device(x, 90, restart)
    assert torch.equal(J.decode_jpeg_device(data, offsets, entropy="split").cpu(), definition(hm.jpeg_encode_rgb8(x, 90, restart))[0])
