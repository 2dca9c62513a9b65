"""Writes tests/golden/jpeg_def.npz: two of the JPEG test fixtures and the bytes host_models.jpeg_encode_rgb8 gives for them (quality
90 with one MCU row per restart interval, quality 100 with a restart marker after every MCU).  Refuses to write unless Pillow
decodes every stream to the right size.      python tools/make_jpeg_golden.py"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.jpeg_util import fixtures  # noqa: E402
from tests.util import GOLDEN, load_pkg  # noqa: E402


def main():
    from PIL import Image  # required: the fixture is only as good as the check that it is a JPEG
    HM = load_pkg().host_models
    fix = fixtures()
    out = {}
    for name in ("extremes", "smooth_noise"):
        img = fix[name]
        out[name] = img
        for key, q, r in (("q90_row", 90, None), ("q100_r1", 100, 1)):
            data = HM.jpeg_encode_rgb8(img, q, r)[0]
            im = Image.open(io.BytesIO(data))
            im.load()
            if im.size != (img.shape[1], img.shape[0]) or im.mode != "RGB":
                raise SystemExit("Pillow reads %s %s as %s %s: nothing written" % (name, key, im.size, im.mode))
            out["%s_%s" % (name, key)] = np.frombuffer(data, np.uint8)
    path = os.path.join(GOLDEN, "jpeg_def.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
