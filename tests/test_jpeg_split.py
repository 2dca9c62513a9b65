"""The split entropy route of the JPEG decoder on the host path (float_jpg_decode_host following the plan's route): the restart
intervals of a scan cut into subsequences must give Pillow's pixels bit for bit, whatever the subsequence length."""
import numpy as np
import pytest

from tests.test_jpeg_decode import J, hm, image, pil_file, pillow

SUBS = ["4:4:4", "4:2:2", "4:2:0", "grey"]
# partial MCUs, intervals that are not rows, a short last one; 3 intervals of several lanes at S = 8; intervals of 4 + 2 MCU rows
# at 4:2:0, and at q 100 and S = 1 more bytes than lanes, so S_eff > S; one interval: the sync route
CASES = {"17x13 3 mcus": (17, 13, {"restart_marker_blocks": 3}), "48x64 row": (48, 64, {"restart_marker_rows": 1}),
         "96x128 4 rows": (96, 128, {"restart_marker_rows": 4}), "48x64 none": (48, 64, {})}


def case_files(sub, case):
    h, w, kw = CASES[case]
    return [pil_file(h, w, sub, q, None, **kw) for q in (25, 100)]


def damaged():
    """The 48 x 64 file with a marker per MCU row: cut inside the scan, with a wrong bit in the first interval, with its first
    marker removed - an interval of double length in front of one without a segment -, and with 48 one-bits inside the second
    interval: no code is 16 ones, so that chain dies there."""
    f = pil_file(48, 64, "4:2:0", 90, "row")
    hdr = hm.jpeg_parse_header(f)
    flipped = bytearray(f)
    flipped[hdr["scan_start"] + 40] ^= 0x10
    at = f.index(b"\xff\xd0", hdr["scan_start"])
    return [f[:hdr["scan_start"] + (hdr["scan_end"] - hdr["scan_start"]) // 2], bytes(flipped), f[:at] + f[at + 2:],
            f[:at + 12] + b"\xff\x00" * 6 + f[at + 24:]]


@pytest.mark.parametrize("S", [1, 8, None])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sub", SUBS)
def test_split_route_is_pillow(sub, case, S):
    files = case_files(sub, case)
    got, status = J.decode_jpeg_host(files, entropy="split", sync_bytes=S)
    assert status.tolist() == [0, 0]
    for i, f in enumerate(files):
        assert np.array_equal(got[i].numpy(), pillow(f)), i
    if not CASES[case][2]:
        assert got.equal(J.decode_jpeg_host(files, entropy="sync", sync_bytes=S)[0])


def test_plan_words():
    for case in list(CASES)[:3]:
        a = J.host_files(case_files("4:4:4", case))  # 4:2:0 leaves 17 x 13 two MCUs: one interval
        assert not J.JpegPlan(*a).ints.equal(J.JpegPlan(*a, entropy="split").ints), case
        assert J.JpegPlan(*a).ints.equal(J.JpegPlan(*a, entropy="sync").ints), case
    b = J.host_files([pil_file(200, 200, "4:4:4", 90, "mcu")])  # 625 intervals: a lane each already
    plain, split = J.JpegPlan(*b), J.JpegPlan(*b, entropy="split")
    assert plain.ints.equal(split.ints) and plain.work_bytes == split.work_bytes


@pytest.mark.parametrize("S", [8, None])
def test_damaged_scans_get_the_definitions_pixels_and_status(S):
    files = damaged()
    got, status = J.decode_jpeg_host(files, entropy="split", sync_bytes=S)
    for i, d in enumerate(files):
        rgb, st = hm.jpeg_decode_rgb8(d, status=True)
        assert int(status[i]) == st and np.array_equal(got[i].numpy(), rgb), i
    assert int(status[2]) & hm.JPEG_DEC_RESTARTS and int(status[3]) == hm.JPEG_DEC_BAD_CODE


@pytest.mark.parametrize("restart", [None, 1])
def test_own_encoder_is_pillow(restart):
    files = hm.jpeg_encode_rgb8(np.stack([image(48, 64), image(48, 64)[::-1]]), 90, restart)
    got, status = J.decode_jpeg_host(files, entropy="split")
    assert status.tolist() == [0, 0]
    for i, f in enumerate(files):
        assert np.array_equal(got[i].numpy(), pillow(f)), i
