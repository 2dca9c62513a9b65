"""Inputs for tools/probes/jpgd_host.cpp: the files of tests/test_jpeg_decode.py (every subsampling x size, each with its eight
quality / restart / table variants), this project's own encoder's files, and the two truncated scans of
tests/test_jpeg_decode_gpu.py, and the files of tests/test_jpeg_split.py (restart intervals of several MCU rows), each as NAME.jpg with NAME.rgb = host_models.jpeg_decode_rgb8's bytes beside it.
  python tools/probes/jpgd_inputs.py OUT_DIR
  clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/probes/jpgd_host.cpp -o jpgd_host
  ./jpgd_host --selftest --mangle OUT_DIR/*.jpg"""
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from tests import test_jpeg_split as split  # noqa: E402
from tests.test_jpeg_decode import SIZES, case_files, hm, image, pil_file  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
files = [f for sub in ("4:4:4", "4:2:2", "4:2:0", "grey") for size in SIZES for f in case_files(sub, size)]
files += [f for restart in (0, None, 1) for f in hm.jpeg_encode_rgb8(np.stack([image(48, 64), image(16, 16).repeat(3, 0).repeat(4, 1)]), 90, restart)]
files += [pil_file(96, 128, sub, 100, None) for sub in ("4:4:4", "4:2:2", "4:2:0", "grey")]  # long scans without markers: --sync 8 needs all 1024 lanes
for restart in (None, "row"):
    f = pil_file(48, 64, "4:2:0", 90, restart)
    hdr = hm.jpeg_parse_header(f)
    files.append(f[:hdr["scan_start"] + (hdr["scan_end"] - hdr["scan_start"]) // 2])
files += [f for sub in split.SUBS for case in split.CASES for f in split.case_files(sub, case)] + split.damaged()  # --split: coarse intervals
for i, f in enumerate(files):
    open(os.path.join(out, "f%04d.jpg" % i), "wb").write(f)
    hm.jpeg_decode_rgb8(f).tofile(os.path.join(out, "f%04d.rgb" % i))
print("%d files in %s" % (len(files), out))
