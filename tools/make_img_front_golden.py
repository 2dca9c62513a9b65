"""Writes tests/golden/img_front.npz: small RGBA / RGB float images and what the reference's own img_tensor_2_np_array +
convert_rgba_to_rgb_numpy (utils/image.py:38-131) make of them, for the three RGBA strategies and two background colours.
host_models.image_to_rgb8 is held to these bytes (tests/test_img_front.py).

BUILD-CONTAINER ONLY, like tools/ref_import.py: the reference module is loaded by path, with empty stand-ins for `cv2` and
`face_alignment` in sys.modules while it imports (it uses neither in the two functions run here); the stand-ins leave
sys.modules again.  The fixture holds data only.  Run from the repository root: python tools/make_img_front_golden.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
import ref_import  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "img_front.npz")
STRATEGIES = ("discard_alpha", "blend_with_color", "replace_with_color")
BKGS = ("#000000", "#3fa07c")


def load_reference_image_module():
    added = []
    for name in ("cv2", "face_alignment"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
            added.append(name)
    try:
        spec = importlib.util.spec_from_file_location("floatref_utils_image", os.path.join(ref_import.REF_ROOT, "src", "nodes", "utils", "image.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name in added:
            del sys.modules[name]
    return mod


def images():
    """name -> (H, W, 3|4) fp32: values below 0, above 1, exact multiples of 1 / 255, alpha 0, 1 / 255 and 1 among them"""
    rs = np.random.RandomState(20261019)
    out = {}
    a = rs.uniform(-0.2, 1.3, size=(12, 10, 4)).astype(np.float32)
    a[:, :2, 3] = 0.0                                      # fully transparent columns
    a[:, 2:4, 3] = np.float32(1.0) / np.float32(255.0)     # the smallest alpha that is not 0
    a[:, 4:6, 3] = 1.0
    a[:3, :, :3] = (rs.randint(0, 256, size=(3, 10, 3)).astype(np.float32) / np.float32(255.0))  # exact multiples of 1 / 255
    a[3:5, :, :3] = rs.randint(0, 256, size=(2, 10, 3)).astype(np.float32) * np.float32(1.0 / 255.0)  # and their other spelling
    out["rgba_noise"] = a
    k = np.arange(256, dtype=np.float32)
    lv = np.zeros((16, 16, 4), np.float32)  # every alpha level once, over a colour ramp
    lv[..., 3] = (k / np.float32(255.0)).reshape(16, 16)
    lv[..., 0] = (k[::-1] / np.float32(255.0)).reshape(16, 16)
    lv[..., 1] = ((k * 7) % 256 / np.float32(255.0)).reshape(16, 16)
    lv[..., 2] = 1.0
    out["rgba_levels"] = lv
    white = np.ones((5, 7, 4), np.float32)  # white under transparency on the left, opaque mid-grey on the right
    white[:, :3, 3] = 0.0
    white[:, 3:, :3] = 0.5
    out["rgba_white_under"] = white
    c = rs.uniform(-0.5, 1.5, size=(12, 10, 3)).astype(np.float32)
    c[:2] = rs.randint(0, 256, size=(2, 10, 3)).astype(np.float32) / np.float32(255.0)
    c[2, :4, 0] = [0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), np.nextafter(np.float32(0.0), np.float32(1.0))]
    out["rgb_noise"] = c
    out["rgb_tiny"] = rs.uniform(0.0, 1.0, size=(3, 4, 3)).astype(np.float32)
    return out


def main():
    ref = load_reference_image_module()
    data = {}
    names = []
    for name, img in images().items():
        names.append(name)
        data["img_" + name] = img
        t = torch.from_numpy(img)
        if img.shape[-1] == 3:
            data["out_%s" % name] = np.ascontiguousarray(ref.img_tensor_2_np_array(t[None], "blend_with_color", "#3fa07c"))
            continue
        outs = np.zeros((len(STRATEGIES), len(BKGS)) + img.shape[:2] + (3,), np.uint8)  # one array per image: [strategy, background]
        for i, st in enumerate(STRATEGIES):
            for j, bk in enumerate(BKGS):
                got = ref.img_tensor_2_np_array(t, st, bk)
                assert got.dtype == np.uint8 and got.shape == img.shape[:2] + (3,)
                outs[i, j] = got
        data["out_%s" % name] = outs
    data["names"] = np.array(names)
    data["strategies"] = np.array(STRATEGIES)
    data["bkgs"] = np.array(BKGS)
    np.savez_compressed(OUT, **data)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
