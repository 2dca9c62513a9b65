"""The sync entropy route of the JPEG decoder on the host path (float_jpg_decode_host following the plan's route): a scan without
restart markers cut into subsequences must give Pillow's pixels bit for bit, whatever the subsequence length."""
import numpy as np
import pytest

from tests.test_jpeg_decode import J, hm, pil_file, pillow

SUBS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
SIZES = [(1, 1), (17, 13), (48, 64), (96, 128)]  # one lane; partial MCUs; 12-13 stuffed bytes at q 100; above 1024 lanes of 8 bytes


@pytest.mark.parametrize("S", [1, 8, 64, None])  # 1 and 8: shorter than a block, lanes that own nothing, several rounds
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("sub", SUBS)
def test_sync_route_is_pillow(sub, size, S):
    files = [pil_file(*size, sub, q, None) for q in (25, 100)]
    got, status = J.decode_jpeg_host(files, entropy="sync", sync_bytes=S)
    assert status.tolist() == [0, 0]
    for i, f in enumerate(files):
        assert np.array_equal(got[i].numpy(), pillow(f)), i


@pytest.mark.parametrize("S", [8, 64])
def test_damaged_scans_get_the_definitions_pixels_and_status(S):
    f = pil_file(48, 64, "4:2:0", 90, None)
    hdr = hm.jpeg_parse_header(f)
    flipped = bytearray(f)
    flipped[hdr["scan_start"] + 40] ^= 0x10
    files = [f[:hdr["scan_start"] + (hdr["scan_end"] - hdr["scan_start"]) // 2], bytes(flipped)]
    got, status = J.decode_jpeg_host(files, entropy="sync", sync_bytes=S)
    for i, d in enumerate(files):
        rgb, st = hm.jpeg_decode_rgb8(d, status=True)
        assert int(status[i]) == st and np.array_equal(got[i].numpy(), rgb), i
    assert int(status[0]) == hm.JPEG_DEC_PAST_END


def test_plan_words_and_refusals():
    plain = [pil_file(48, 64, "4:2:0", 90, r) for r in (None, "row")]
    marked = [pil_file(48, 64, "4:2:0", 90, r) for r in ("row", "mcu")]
    a, b = J.host_files(plain), J.host_files(marked)
    assert J.JpegPlan(*a).ints.equal(J.JpegPlan(*a, entropy="interval").ints)
    assert J.JpegPlan(*b).ints.equal(J.JpegPlan(*b, entropy="sync").ints) and J.JpegPlan(*b).work_bytes == J.JpegPlan(*b, entropy="sync").work_bytes
    assert J.JpegPlan(*a).ints.equal(J.JpegPlan(*a, entropy="auto").ints)  # a scan far below 64 KB
    assert not J.JpegPlan(*a).ints.equal(J.JpegPlan(*a, entropy="sync").ints)
    for kw in ({"entropy": "parallel"}, {"entropy": 1}, {"entropy": "sync", "sync_bytes": 0}, {"entropy": "sync", "sync_bytes": 65537},
               {"entropy": "sync", "sync_bytes": 8.0}):
        with pytest.raises(ValueError, match="entropy|sync_bytes"):
            J.JpegPlan(*a, **kw)
