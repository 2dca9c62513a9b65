"""The S3FD face detector without a GPU: the C boundary (symbols, argument checks), the definition in host_models (map shapes,
decoding, NMS and the commutation of the score filter with it), the FLOAT_AMD_FACE_DETECTOR switch of process_img and the
weight-file search of face.py."""
import ctypes as C
import functools
import logging
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.util import ROOT, load_pkg

pkg = load_pkg()
hm = pkg.host_models

SFD_SYMBOLS = ("float_sfd_create", "float_sfd_destroy", "float_sfd_detect", "float_sfd_maps", "float_sfd_post", "float_sfd_dense",
               "float_sfd_saturation")


@functools.lru_cache(maxsize=None)
def sfd_state():
    return pkg.weights.synth_sfd_state(seed=5)


def test_sfd_symbols_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "float_hip.h")).read()
    declared = set(re.findall(r"\b(float_[a-z_0-9]+)\s*\(", hdr))
    L = pkg.native.lib()
    for name in SFD_SYMBOLS:
        assert name in declared and name in pkg.native.EXPORTS and hasattr(L, name), name
    assert L.float_hip_abi_version() == 6 and pkg.native.ABI_VERSION == 6  # new symbols only


def test_sfd_state_has_the_package_keys():
    shapes = hm.sfd_state_shapes()
    assert len(shapes) == 2 * 19 + 3 + 4 * 6  # 19 trunk convs, 3 L2Norms, 6 x (conf, loc)
    assert shapes["conv1_1.weight"] == (64, 3, 3, 3) and shapes["fc6.weight"] == (1024, 512, 3, 3) and shapes["fc7.weight"] == (1024, 1024, 1, 1)
    assert shapes["conv3_3_norm.weight"] == (256,) and shapes["conv3_3_norm_mbox_conf.weight"] == (4, 256, 3, 3)
    assert shapes["conv4_3_norm_mbox_conf.bias"] == (2,) and shapes["fc7_mbox_loc.weight"] == (4, 1024, 3, 3)
    assert shapes["conv7_2_mbox_conf.weight"] == (2, 256, 3, 3) and shapes["conv6_2.weight"] == (512, 256, 3, 3)
    sd = sfd_state()
    assert {k: tuple(v.shape) for k, v in sd.items()} == shapes
    assert float(sd["conv3_3_norm.weight"][0]) == 10 and float(sd["conv4_3_norm.weight"][0]) == 8 and float(sd["conv5_3_norm.weight"][0]) == 5


@pytest.mark.parametrize("hw,want", [((45, 61), [(11, 15), (5, 7), (2, 3), (5, 5), (3, 3), (2, 2)]),
                                     ((72, 100), [(18, 25), (9, 12), (4, 6), (6, 7), (3, 4), (2, 2)])])
def test_sfd_forward_shapes(hw, want):
    """Floor pooling at every pool, fc6's growth by 4, the stride-2 convs on odd inputs."""
    view = torch.from_numpy(np.random.RandomState(hw[0]).randint(0, 256, size=hw + (3,)).astype(np.uint8))
    with torch.no_grad():
        maps = hm.sfd_forward(sfd_state(), view)
    assert len(maps) == 12 and hm.sfd_map_sizes(*hw) == want
    for i, (h, w) in enumerate(want):
        assert tuple(maps[2 * i].shape) == (1, 2, h, w) and tuple(maps[2 * i + 1].shape) == (1, 4, h, w), i
        assert maps[2 * i].dtype == torch.float32 and bool(torch.isfinite(maps[2 * i]).all())


def test_sfd_forward_refuses_a_15_px_side():
    with pytest.raises(ValueError):
        hm.sfd_forward(sfd_state(), torch.zeros(15, 64, 3, dtype=torch.uint8))


def _zero_maps(H, W, bg=-20.0):
    maps = []
    for h, w in hm.sfd_map_sizes(H, W):
        conf = torch.zeros(1, 2, h, w)
        conf[:, 1] = bg
        maps += [conf, torch.zeros(1, 4, h, w)]
    return maps


def test_sfd_decode_planted_positions():
    """One planted position per level of a 72 x 100 view, boxes computed by hand: conf (0, ln 3) -> score 3 / 4; loc (1, -1, 0, 5 ln 2)
    -> centre (s / 2 + x s + 0.4 s, s / 2 + y s - 0.4 s), width 4 s, height 8 s.  Level 3's position (5, 6) lies in the border fc6
    grew: its prior centre x = 16 + 6 * 32 = 208 is beyond the 100-px view, and it is kept with stride 32."""
    maps = _zero_maps(72, 100)
    planted = [(0, 2, 3), (1, 8, 11), (2, 3, 0), (3, 5, 6), (4, 1, 2), (5, 1, 1)]
    for lvl, y, x in planted:
        maps[2 * lvl][0, 1, y, x] = math.log(3.0)
        maps[2 * lvl + 1][0, :, y, x] = torch.tensor([1.0, -1.0, 0.0, 5 * math.log(2.0)])
    got = hm.sfd_decode(maps, 0.5)
    assert got.shape == (6, 5)
    for row, (lvl, y, x) in zip(got, planted):  # position order = level order here
        s = 2.0 ** (lvl + 2)
        want = [s * (x + 0.9) - 2 * s, s * (y + 0.1) - 4 * s, s * (x + 0.9) + 2 * s, s * (y + 0.1) + 4 * s, 0.75]
        assert np.allclose(row, want, rtol=0, atol=2e-4), (lvl, row, want)  # the planted logits are fp32
    assert np.allclose(got[0], [7.6, -7.6, 23.6, 24.4, 0.75], atol=1e-5)       # level 0, stride 4, (y, x) = (2, 3)
    assert np.allclose(got[3], [156.8, 35.2, 284.8, 291.2, 0.75], atol=1e-4)  # level 3, stride 32, (5, 6): beyond the image
    dense = hm.sfd_decode_dense(maps)
    assert dense.shape == (sum(h * w for h, w in hm.sfd_map_sizes(72, 100)), 5) and int((dense[:, 4] > 0.5).sum()) == 6
    assert hm.sfd_decode(maps, 0.75 + 1e-6).shape == (0, 5) and hm.sfd_decode(maps, 0.75 - 1e-6).shape == (6, 5)


def test_sfd_nms_plus_one_areas():
    """A = (0, 0, 9, 9) and B = (5, 0, 14, 9): with the `+1` convention both areas are 100 and the overlap is 5 x 10, IoU 1 / 3 > 0.3,
    so B goes; without it the IoU would be 36 / 126 < 0.3 and B would stay."""
    boxes = np.array([[0, 0, 9, 9, 0.9], [5, 0, 14, 9, 0.8]], dtype=np.float64)
    assert hm.sfd_nms(boxes, 0.3) == [0]
    assert hm.sfd_nms(boxes, 0.34) == [0, 1]


def test_sfd_nms_keeps_iou_exactly_at_the_threshold():
    """B = (7, 0, 9, 9) lies inside A = (0, 0, 9, 9): overlap 30, union 100, IoU = 30 / 100 == 0.3 in float64: kept (dropped only above)."""
    boxes = np.array([[0, 0, 9, 9, 0.9], [7, 0, 9, 9, 0.8]], dtype=np.float64)
    assert 30.0 / 100.0 == 0.3
    assert hm.sfd_nms(boxes, 0.3) == [0, 1]
    assert hm.sfd_nms(boxes, 0.3 - 1e-12) == [0]


def test_sfd_nms_orders_ties_by_position():
    boxes = np.array([[0, 0, 9, 9, 0.7], [1, 0, 10, 9, 0.7], [100, 0, 109, 9, 0.7], [2, 0, 11, 9, 0.9], [50, 0, 59, 9, 0.7]], dtype=np.float64)
    # 3 (highest) drops 0 and 1; the equal scores that are left keep their position order
    assert hm.sfd_nms(boxes, 0.3) == [3, 2, 4]
    assert hm.sfd_nms(boxes[:3], 0.3) == [0, 2]  # of two overlapping boxes of equal score the earlier position wins


@pytest.mark.parametrize("thr", [0.5, 0.95])
def test_score_filter_commutes_with_nms(thr):
    """The package's order - candidates above 0.05, NMS, then score > thr - against the definition's: filter first."""
    r = np.random.RandomState(31)
    n = 1000
    x1, y1 = r.uniform(0, 300, n), r.uniform(0, 300, n)
    boxes = np.stack([x1, y1, x1 + r.uniform(5, 120, n), y1 + r.uniform(5, 120, n), r.uniform(0, 1, n)], axis=1)
    boxes[::50, 4] = boxes[7, 4]  # some ties
    cand = boxes[boxes[:, 4] > 0.05]
    literal = [list(cand[i]) for i in hm.sfd_nms(cand, 0.3) if cand[i, 4] > thr]
    assert literal == hm.sfd_select(boxes, thr, 0.3) and 0 < len(literal) < len(cand)


def test_sfd_argument_checks_need_no_gpu():
    L = pkg.native.lib()
    buf = (C.c_float * 16)()
    assert L.float_sfd_detect(None, buf, 64, 64, 0.5, 0.3, buf, buf, None) == 1 and b"null handle" in L.float_last_error()
    assert L.float_sfd_detect(None, buf, 15, 64, 0.5, 0.3, buf, buf, None) == 1 and b"15 x 64" in L.float_last_error()
    assert L.float_sfd_maps(None, buf, 64, 4097, buf, None) == 1 and b"4097" in L.float_last_error()
    assert L.float_sfd_post(None, buf, 64, 64, 0.5, 0.3, buf, buf, None) == 1
    assert L.float_sfd_dense(None, buf, None) == 1 and L.float_sfd_saturation(None, None, 0, None) == 1
    h = C.c_void_p()
    arr = (pkg.native.FloatTensor * 1)()
    for cfg in (pkg.native.SfdCfg(1, 15, 64, 1024, 64), pkg.native.SfdCfg(1, 360, 4097, 1024, 64), pkg.native.SfdCfg(1, 360, 640, 4096, 64),
                pkg.native.SfdCfg(1, 360, 640, 16, 64), pkg.native.SfdCfg(7, 360, 640, 1024, 64)):
        assert L.float_sfd_create(C.byref(cfg), arr, 0, C.byref(h)) == 1
    L.float_sfd_destroy(None)


# ---------------------------------------------------------------------------------------------- the switch of process_img
class _Log(logging.Handler):
    def __init__(self):
        super().__init__()
        self.seen = []

    def emit(self, rec):
        self.seen.append(rec.getMessage())


def _logger(name):
    log, h = logging.getLogger(name), _Log()
    log.handlers[:] = [h]
    log.propagate = False
    return log, h.seen


def _package_stub(monkeypatch, box):
    calls = []

    def detect_from_image(img):
        calls.append(img.shape)
        return [box]
    fa = types.SimpleNamespace(face_detector=types.SimpleNamespace(detect_from_image=detect_from_image))
    monkeypatch.setattr(hm, "_face_detector", lambda: fa)
    return calls


def _no_package(monkeypatch):
    def fail():
        raise ImportError("No module named 'face_alignment'")
    monkeypatch.setattr(hm, "_face_detector", fail)


IMG = torch.rand(720, 800, 3, generator=torch.Generator().manual_seed(2))
PKG_BOX, DEV_BOX = [100.0, 50.0, 200.0, 170.0, 0.99], [150.0, 100.0, 250.0, 260.0, 0.97]
CENTRE = (40, 0, 720, 720)


def _bbox_of(box):  # process_img's rule for a 720-px-high image (mult = 0.5)
    x1, y1, x2, y2 = (int(v / 0.5) for v in box[:4])
    bs = int(max(int((y2 - y1) / 2), int((x2 - x1) / 2)) * 1.6)
    mx, my = int((x1 + x2) / 2), int((y1 + y2) / 2)
    return (mx - bs, my - bs, 2 * bs, 2 * bs)


def test_switch_all_four_values(monkeypatch):
    dev_calls = []

    def device(view):
        dev_calls.append(tuple(view.shape))
        return [DEV_BOX]
    pk_calls = _package_stub(monkeypatch, PKG_BOX)
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "off")
    assert hm.process_img(IMG, 360, detector=device)[1] == CENTRE and not dev_calls and not pk_calls
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "package")
    assert hm.process_img(IMG, 360, detector=device)[1] == _bbox_of(PKG_BOX) and not dev_calls and pk_calls == [(360, 400, 3)]
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "device")
    assert hm.process_img(IMG, 360, detector=device)[1] == _bbox_of(DEV_BOX) and dev_calls == [(360, 400, 3)] and len(pk_calls) == 1
    with pytest.raises(ValueError):
        hm.process_img(IMG, 360)
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "auto")  # an installed package goes first
    assert hm.process_img(IMG, 360, detector=device)[1] == _bbox_of(PKG_BOX) and len(dev_calls) == 1 and len(pk_calls) == 2
    _no_package(monkeypatch)
    assert hm.process_img(IMG, 360, detector=device)[1] == _bbox_of(DEV_BOX) and len(dev_calls) == 2
    monkeypatch.delenv("FLOAT_AMD_FACE_DETECTOR")  # unset = auto
    assert hm.process_img(IMG, 360, detector=device)[1] == _bbox_of(DEV_BOX) and len(dev_calls) == 3
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "package")  # the package alone: without it the centre square, never the device
    log, seen = _logger("test_face_switch_pkg")
    assert hm.process_img(IMG, 360, logger=log, detector=device)[1] == CENTRE and len(dev_calls) == 3 and "no face detector is available" in seen[0]
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "sometimes")
    with pytest.raises(ValueError):
        hm.process_img(IMG, 360, detector=device)


def test_switch_device_detector_on_the_front_route(monkeypatch):
    """With `front`, the view goes to the detector as the front end made it (no host copy), and the rect comes back."""
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "device")
    view = torch.zeros(360, 400, 3, dtype=torch.uint8)
    got = []

    def device(v):
        got.append(v)
        return [DEV_BOX]
    rect, bbox = hm.process_img(IMG, 360, front=lambda vh: view, detector=device)
    assert got[0] is view and rect == bbox == _bbox_of(DEV_BOX)
    assert hm.process_img(IMG, 360, front=lambda vh: view, detector=lambda v: [])[0] == CENTRE  # no face: the centre square


def test_switch_auto_with_neither_is_todays_centre_square(monkeypatch):
    _no_package(monkeypatch)
    monkeypatch.delenv("FLOAT_AMD_FACE_DETECTOR", raising=False)
    log, seen = _logger("test_face_switch_auto")
    crop, bbox = hm.process_img(IMG, 360, logger=log)
    want = torch.nn.functional.adaptive_avg_pool2d(IMG[:, 40:760].permute(2, 0, 1)[None], (360, 360))[0].permute(1, 2, 0)
    assert bbox == CENTRE and torch.equal(crop, want)
    assert len(seen) == 1 and seen[0].startswith("face_align=True, but no face detector is available (ImportError: No module named "
                                                 "'face_alignment'): no face detection, the centre square of the image is used "
                                                 "(install face_alignment for the reference's crop).")
    assert "FLOAT_AMD_SFD_WEIGHTS" in seen[0] and "face_alignment/s3fd.safetensors" in seen[0]  # where to put the file
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "off")
    crop2, bbox2 = hm.process_img(IMG, 360, logger=log)
    assert bbox2 == CENTRE and torch.equal(crop2, want) and len(seen) == 1


# ---------------------------------------------------------------------------------------------- the weight file
def test_find_sfd_weights_order(monkeypatch, tmp_path):
    F = pkg.face
    models, home = tmp_path / "models", tmp_path / "home"
    monkeypatch.setenv("FLOAT_MODELS_DIR", str(models))
    monkeypatch.setenv("HOME", str(home))
    monkeypatch.delenv("FLOAT_AMD_SFD_WEIGHTS", raising=False)
    monkeypatch.setitem(__import__("sys").modules, "folder_paths", None)  # outside ComfyUI
    assert F.find_sfd_weights() is None
    order = [home / ".cache" / "torch" / "hub" / "checkpoints" / "s3fd-619a316812.pth", models / "face_alignment" / "s3fd-619a316812.pth",
             models / "face_alignment" / "s3fd.pth", models / "face_alignment" / "s3fd.safetensors"]
    assert [str(p) for p in reversed(order)] == F.sfd_weight_candidates()
    for p in order:  # from the last place looked in to the first: each new file wins
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"x")
        assert F.find_sfd_weights() == str(p)
    env = tmp_path / "mine.pth"
    monkeypatch.setenv("FLOAT_AMD_SFD_WEIGHTS", str(env))
    with pytest.raises(FileNotFoundError):  # a named file that is not there is an error, not a reason to look further
        F.find_sfd_weights()
    env.write_bytes(b"x")
    assert F.find_sfd_weights() == str(env) and F.sfd_weight_candidates()[0] == str(env)


def test_load_sfd_state_is_strict(tmp_path):
    F = pkg.face
    sd = dict(sfd_state())
    good = tmp_path / "s3fd.pth"
    torch.save(sd, str(good))
    back = F.load_sfd_state(str(good))
    assert set(back) == set(sd) and torch.equal(back["fc7.bias"], sd["fc7.bias"])
    sd["conv4_3_norm_mbox_location.weight"] = sd.pop("conv4_3_norm_mbox_loc.weight")
    bad = tmp_path / "renamed.pth"
    torch.save(sd, str(bad))
    with pytest.raises(ValueError) as e:
        F.load_sfd_state(str(bad))
    assert "conv4_3_norm_mbox_loc.weight" in str(e.value) and "conv4_3_norm_mbox_location.weight" in str(e.value)
    sd = dict(sfd_state())
    sd["fc6.weight"] = sd["fc6.weight"][:, :, :1, :1]
    with pytest.raises(ValueError) as e:
        hm.sfd_check_state(sd)
    assert "fc6.weight" in str(e.value)
