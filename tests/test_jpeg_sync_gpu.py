"""The sync entropy route of float_jpg_decode against the definition, host_models.jpeg_decode_rgb8: bitwise, pixels and status."""
import numpy as np
import pytest
import torch

from tests.test_jpeg_decode import J, hm, image, pil_file
from tests.test_jpeg_sync import SIZES, SUBS

pytestmark = pytest.mark.gpu


def definition(files):
    both = [hm.jpeg_decode_rgb8(f, status=True) for f in files]
    return torch.from_numpy(np.stack([rgb for rgb, _ in both])), [st for _, st in both]


@pytest.mark.parametrize("S", [1, 8, 64, None])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("sub", SUBS)
def test_sync_route_is_the_definition(sub, size, S):
    files = [pil_file(*size, sub, q, None) for q in (25, 100)]
    got, status = J.decode_jpeg_device(files, entropy="sync", sync_bytes=S, return_status=True)
    want, st = definition(files)
    assert status.tolist() == st == [0, 0] and torch.equal(got.cpu(), want)


def test_both_routes_in_one_call_of_more_than_a_group():
    files = [pil_file(33, 47, "4:2:0", 25 + 3 * i, ("row", None, "mcu")[i % 3]) for i in range(19)]  # frames 1, 4, ... have no restart markers
    got, status = J.decode_jpeg_device(files, entropy="sync", return_status=True)
    want, st = definition(files)
    assert status.tolist() == st and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("S", [8, 64])
def test_damaged_scans(S):
    f = pil_file(48, 64, "4:2:0", 90, None)
    hdr = hm.jpeg_parse_header(f)
    flipped = bytearray(f)
    flipped[hdr["scan_start"] + 40] ^= 0x10
    files = [f, f[:hdr["scan_start"] + (hdr["scan_end"] - hdr["scan_start"]) // 2], bytes(flipped)]
    got, status = J.decode_jpeg_device(files, strict=False, entropy="sync", sync_bytes=S, return_status=True)
    want, st = definition(files)
    assert st[1] != 0 and status.tolist() == st and torch.equal(got.cpu(), want)


def test_device_files_of_the_own_encoder():
    x = torch.from_numpy(np.stack([image(48, 64), image(48, 64)[::-1].copy()])).cuda()
    data, offsets = J.encode_jpeg_device(x, 90, 0)
    assert torch.equal(J.decode_jpeg_device(data, offsets, entropy="sync").cpu(), definition(hm.jpeg_encode_rgb8(x, 90, 0))[0])
