"""The advanced (Ad) node family and the batched face alignment under it, on the GPU with the synthetic 64-px agent:
InferenceAgent.face_align_batch / host_inputs_batch against the per-image route (bitwise, one detect_batch for the batch),
FloatProcess with two portraits on and off the batched line, and the Ad graph stage by stage against the same operators driven
directly (bitwise) and against the CPU oracle (the limits of test_nodes_va_gpu.py::test_va_graph)."""
import functools
import importlib
import logging

import numpy as np
import pytest
import torch

from oracle import float_oracle as O
from tests.util import load_pkg, rel_l2

pytestmark = pytest.mark.gpu

pkg = load_pkg()
hm, W = pkg.host_models, pkg.weights
SIZE = 64
# 720 x 540 portraits, chosen on the CPU with the definition (sfd_detect on synth_sfd_state(seed=5)): seeds 4 and 6 give two
# boxes above process_img's 0.95, the RGBA one a single box; every margin asserted in _definition holds
PORTRAITS = ((4, 3), (6, 3), (0, 4))
RGBA, BKG = "blend_with_color", "#000000"


@functools.lru_cache(maxsize=None)
def sfd_state():
    return W.synth_sfd_state(seed=5)


@functools.lru_cache(maxsize=None)
def parts():
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.input_size, opt.nfe = SIZE, 4
    cfg = pkg.config.FmtConfig.from_options(opt)
    acfg = pkg.config.small_audio_config()
    acfg.dim_w = opt.dim_w
    sds = dict(enc=W.synth_encoder_state(SIZE, seed=31), dec=W.synth_decoder_state(SIZE, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
               audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
    return opt, cfg, acfg, sds


@functools.lru_cache(maxsize=None)
def agent():
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt, _, _, sds = parts()
    return gen.InferenceAgent(opt, sds, "cuda:0", max_frames=8)


@functools.lru_cache(maxsize=None)
def portraits():
    return tuple(torch.rand(720, 540, ch, generator=torch.Generator().manual_seed(seed)) for seed, ch in PORTRAITS)


def _audio(seed=9):
    return {"waveform": W.synth_waveform(1.4, seed=seed).reshape(1, 1, -1), "sample_rate": 16000}


@pytest.fixture
def device_detector(monkeypatch, tmp_path):
    weights = tmp_path / "s3fd.pth"
    torch.save(sfd_state(), str(weights))
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "device")
    monkeypatch.setenv("FLOAT_AMD_SFD_WEIGHTS", str(weights))
    monkeypatch.setenv("FLOAT_AMD_SFD_DTYPE", "fp32")
    monkeypatch.delenv("FLOAT_AMD_IMAGE_FRONT", raising=False)
    a = agent()
    a.opt.rgba_conversion, a.opt.bkg_color_hex = RGBA, BKG
    return a


@pytest.fixture
def calls(monkeypatch):
    """How often the two detector entry points of the wrapper were used."""
    n = {"detect": 0, "detect_batch": 0}
    cls = pkg.face.FaceDetectorHIP
    for name in n:
        def counted(self, *a, _f=getattr(cls, name), _name=name, **k):
            n[_name] += 1
            return _f(self, *a, **k)
        monkeypatch.setattr(cls, name, counted)
    return n


def _definition(img):
    """(view on the device, sfd_detect's rows on it), with process_img's decisions away from their edges: the margins of
    test_product_call_with_the_device_detector, for the first two boxes (index = 2 is used here)."""
    dimg = pkg.image.image_to_device(img, "cuda:0")
    view = pkg.image.detector_view_device(dimg, 360, RGBA, BKG)
    assert tuple(view.shape) == (360, 270, 3)
    det = hm.sfd_detect(sfd_state(), view.cpu())
    faces = [d for d in det if d[4] > 0.95]
    assert all(abs(d[4] - 0.95) > 1e-3 for d in det)
    assert all(det[i][4] - det[i + 1][4] > 1e-4 for i in range(min(2, len(det) - 1)))
    assert all(abs(2 * v - round(2 * v)) > 2e-2 for f in faces[:2] for v in f[:4])  # int(v / mult), mult = 1 / 2
    return dimg, view, det, len(faces)


def test_face_align_batch_is_the_single_image_route(device_detector, calls, caplog):
    a = device_detector
    imgs = portraits()
    batch = torch.zeros(3, 720, 540, 4)
    for i, im in enumerate(imgs):
        batch[i, ..., :im.shape[-1]] = im
        if im.shape[-1] == 3:
            batch[i, ..., 3] = 1.0  # opaque: blending leaves the colours as they are
    defs = [_definition(batch[i]) for i in range(3)]
    assert [d[3] for d in defs] == [2, 2, 1]
    for index in (1, 2):
        caplog.clear()
        calls["detect"] = calls["detect_batch"] = 0
        with caplog.at_level(logging.WARNING):
            crops, rects = a.face_align_batch(batch, index=index)
        assert calls == {"detect": 0, "detect_batch": 1}
        assert crops.dtype == torch.uint8 and tuple(crops.shape) == (3, SIZE, SIZE, 3) and crops.is_cuda and len(rects) == 3
        assert ("Only 1 detected, using the first one" in caplog.text) == (index == 2)
        for i, (dimg, view, det, n_faces) in enumerate(defs):
            # the definition's rect, and the per-image route on the device detector
            want_rect, _ = hm.process_img(dimg, SIZE, a.opt.face_margin, index=index, front=lambda vh: view, detector=lambda v: det)
            one_rect, _ = hm.process_img(dimg, SIZE, a.opt.face_margin, index=index,
                                         front=lambda vh: pkg.image.detector_view_device(dimg, vh, RGBA, BKG), detector=a._face_detector())
            assert tuple(rects[i]) == tuple(want_rect) == tuple(one_rect), (index, i)
            assert tuple(want_rect) != (0, 90, 540, 540)
            assert torch.equal(crops[i], pkg.image.image_front_device(dimg, SIZE, SIZE, one_rect, None, RGBA, BKG, True)), (index, i)
        if index == 2:
            first = a.face_align_batch(batch, index=1)[1]
            assert rects[0] != first[0] and rects[1] != first[1] and rects[2] == first[2]  # the second box where there is one
    assert a.face.fallbacks == 0 and a.face.saturation() == 0


def test_face_align_batch_with_the_detector_off(device_detector, calls, monkeypatch):
    monkeypatch.setenv("FLOAT_AMD_FACE_DETECTOR", "off")
    batch = torch.stack([p[..., :3] for p in portraits()])
    crops, rects = device_detector.face_align_batch(batch)
    assert rects == [(0, 90, 540, 540)] * 3 and calls == {"detect": 0, "detect_batch": 0}
    for i in range(3):
        assert torch.equal(crops[i], pkg.image.image_front_device(batch[i], SIZE, SIZE, rects[i], None, RGBA, BKG, True))


def test_host_inputs_batch_is_host_inputs(device_detector, calls):
    a = device_detector
    imgs = [p[None] for p in portraits()]
    auds = [_audio(9), _audio(10), _audio(11)]
    want = [a.host_inputs(im, au, False) for im, au in zip(imgs, auds)]
    assert calls == {"detect": 3, "detect_batch": 0}
    got = a.host_inputs_batch(imgs, auds, False)
    assert calls == {"detect": 3, "detect_batch": 1}
    plain = a.host_inputs_batch(torch.stack([p[..., :3] for p in portraits()]), auds, True)  # a tensor of images, no crop
    assert calls == {"detect": 3, "detect_batch": 1}
    for i in range(3):
        assert torch.equal(got[i][0], want[i][0]) and torch.equal(got[i][1], want[i][1]), i
        s, au = a.host_inputs(imgs[i][..., :3], auds[i], True)
        assert torch.equal(plain[i][0], s) and torch.equal(plain[i][1], au), i
    assert not torch.equal(got[0][0], plain[0][0])  # the crop is not the whole image


class _PerItemPipe:
    """The agent without host_inputs_batch: FloatProcess' hasattr guard takes the per-item line."""

    def __init__(self, pipe):
        object.__setattr__(self, "_pipe", pipe)

    def __getattr__(self, name):
        if name == "host_inputs_batch":
            raise AttributeError(name)
        return getattr(self._pipe, name)


def test_floatprocess_batched_line_equals_the_per_item_line(device_detector, calls):
    a = device_detector
    node = pkg.NODE_CLASS_MAPPINGS["FloatProcessOpt"]()
    imgs = torch.stack([p[..., :3] for p in portraits()[:2]])
    wav = torch.cat([_audio(9)["waveform"], _audio(10)["waveform"]])
    args = ({"waveform": wav, "sample_rate": 16000},)
    frames, _, fps = node.floatprocess(imgs, *args, a, 2.0, 1.0, 25.0, "happy", True, 7)
    assert calls == {"detect": 0, "detect_batch": 1}
    frames = frames.clone()
    per_item, _, _ = node.floatprocess(imgs, *args, _PerItemPipe(a), 2.0, 1.0, 25.0, "happy", True, 7)
    assert calls == {"detect": 2, "detect_batch": 1}
    assert tuple(frames.shape) == (2 * 35, SIZE, SIZE, 3) and fps == 25.0 and torch.equal(frames, per_item)


def test_ad_graph():
    n = pkg.NODE_CLASS_MAPPINGS
    a = agent()
    opt, cfg, acfg, sds = parts()
    img = torch.from_numpy(np.random.RandomState(5).rand(2, SIZE, SIZE, 3).astype(np.float32))
    app, lam, p = n["FloatEncodeImageToLatents"]().encode_image_batch(img, a)
    assert p is a and app["h_source"].shape == (2, 512) and lam.shape == (2, 20) and len(app["feats"]) == 4
    s = img.permute(0, 3, 1, 2).contiguous() * 2 - 1
    for b in range(2):
        sb, lb, fb, _ = a.enc.encode_image_into_latent(s[b])
        assert torch.equal(app["h_source"][b:b + 1], sb.cpu()) and torch.equal(lam[b:b + 1], lb.cpu())
        assert all(torch.equal(f[b:b + 1], g.cpu()) for f, g in zip(app["feats"], fb))
    o_s, _, o_l = O.encode_appearance(sds["enc"], s)
    e_enc = max(rel_l2(app["h_source"], o_s), rel_l2(lam, o_l))
    r_s, _ = n["FloatGetIdentityReference"]().get_identity_reference_batch(lam, a)
    assert torch.equal(r_s, a.G.dec.direction(lam).cpu())
    e_dir = rel_l2(r_s, O.direction(sds["dec"], lam))

    wav = torch.cat([W.synth_waveform(1.0, seed=8), W.synth_waveform(1.0, seed=9)])[:, None]
    wa, T, a_norm, _ = n["FloatEncodeAudioToLatentWA"]().encode_audio_to_wa(a, {"waveform": wav, "sample_rate": 16000}, 25.0)
    assert T == 25 and wa.shape == (2, 25, 512) and a_norm.shape == (2, 16000) and not a_norm.is_cuda and opt.fps == 25.0
    assert torch.equal(wa, a.audio_encoder.inference(a_norm.cuda(), seq_len=25).cpu())
    for b in range(2):
        assert torch.equal(a_norm[b:b + 1], a._host_audio({"waveform": wav[b:b + 1], "sample_rate": 16000}).cpu())
    e_wa = rel_l2(wa, O.audio_encoder_inference(sds["audio_encoder"][0], acfg, a_norm, 25))

    E = n["FloatEncodeEmotionToLatentWE"]()
    we_label, _ = E.encode_emotion_to_we(a_norm, a, "happy")
    assert torch.equal(we_label, torch.nn.functional.one_hot(torch.tensor(3), 7).float()[None, None].repeat(2, 1, 1))
    with pytest.raises(NotImplementedError, match="speech-emotion"):  # this agent has no speech-emotion model
        E.encode_emotion_to_we(a_norm, a, "none")
    a.emotion_predictor = lambda x: torch.softmax(x[:, :7], -1)  # a stand-in predictor: (1, N) -> (1, 7)
    try:
        we_pred, _ = E.encode_emotion_to_we(a_norm, a, "none")
    finally:
        a.emotion_predictor = None
    assert we_pred.shape == (2, 1, 7) and torch.allclose(we_pred[:, 0], torch.softmax(a_norm[:, :7], -1), atol=1e-6)

    we = torch.softmax(torch.randn(2, 1, 7, generator=torch.Generator().manual_seed(1)), -1)
    S = n["FloatSampleMotionSequenceRD"]()
    r_d, _ = S.sample_rd_sequence(r_s, wa, T, we, a, 2.0, 1.0, 15)
    assert r_d.shape == (2, 25, 512) and torch.equal(r_d, S.sample_rd_sequence(r_s, wa, T, we, a, 2.0, 1.0, 15)[0])
    assert not torch.equal(r_d, S.sample_rd_sequence(r_s, wa, T, we, a, 2.0, 1.0, 16)[0])
    noise = pkg.fmt.draw_noise(1, 2, cfg, 15, device="cuda:0")
    assert torch.equal(r_d, a.G.batched_fmt(2).sample(r_s, wa, we, noise, 4, 2.0, opt.r_cfg_scale, 1.0).cpu())
    want = O.sample_rd(sds["fmt"], cfg, r_s[:1], wa[:1], we[:1], noise[:, :1].cpu(), 4, 2.0, 1.0, 1.0)
    e_rd = rel_l2(r_d[:1], want)
    we_dyn = torch.softmax(torch.randn(2, T, 7, generator=torch.Generator().manual_seed(2)), -1)
    r_dyn, _ = S.sample_rd_sequence(r_s, wa, T, we_dyn, a, 2.0, 1.0, 15)
    assert r_dyn.shape == (2, 25, 512) and bool(torch.isfinite(r_dyn).all()) and not torch.equal(r_dyn, r_d)
    print("Ad graph against the oracle: encoder %.2e  direction %.2e  wa %.2e  r_d[0] %.2e" % (e_enc, e_dir, e_wa, e_rd))
    assert e_enc < 2e-3 and e_dir < 1e-5 and e_wa < 3e-3 and e_rd < 5e-3

    r_d = r_d * 0.3
    D = n["FloatDecodeLatentsToImages"]()
    frames, fps, _ = D.decode_latents_to_images(app, r_d[:, :3], a)
    assert frames.shape == (6, SIZE, SIZE, 3) and frames.is_pinned() and frames.min() >= 0 and frames.max() <= 1 and fps == opt.fps == 25.0
    direct = a.G.dec.decode_latent_into_processed_images(app["h_source"][1:2], r_d[1, :3], [f[1:2] for f in app["feats"]]).cpu()
    assert torch.equal(frames[3:], direct)
    empty, fps0, _ = D.decode_latents_to_images(app, r_d[:, :0], a)
    assert empty.shape == (0, SIZE, SIZE, 3) and fps0 == 25.0
