"""The encoder's motion pass over stacked driving frames (float_enc_motion / float_enc_drive_rows) against the fp64 oracle,
its bitwise frame independence, the untouched source state, the composition of driving rows and the driven route."""
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle import float_oracle as O
from tests.test_enc_gpu import TOL
from tests.util import load_pkg, rel_l2

pkg = load_pkg()
W = pkg.weights
pytestmark = pytest.mark.gpu
SEED = 11
CASES = [(1, 8), (2, 8), (5, 4), (9, 8)]  # (T, block); (5, 4) and (9, 8) leave a remainder block of one frame


@functools.lru_cache(None)
def _frames(size):
    """9 seeded uint8 frames; an all-0 and an all-255 frame side by side (a halo read across a frame border would show)."""
    f = torch.from_numpy(np.random.RandomState(size).randint(0, 256, (9, size, size, 3)).astype(np.uint8))
    f[1], f[2] = 0, 255
    return f


@functools.lru_cache(None)
def _oracle_lam(size):
    x = _frames(size).permute(0, 3, 1, 2).double() / 127.5 - 1
    return O.encode_appearance(W.synth_encoder_state(size, seed=SEED), x, dtype=torch.float64)[2]


@functools.lru_cache(None)
def _enc(size, dtype):
    dsd = W.synth_decoder_state(size, seed=SEED)
    return pkg.encoder.EncoderHIP(W.synth_encoder_state(size, seed=SEED), size, 512, 20, "cuda:0", dtype, direction_weight=dsd["direction.weight"])


@pytest.mark.parametrize("T,block", CASES)
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("size", [64, 128])
def test_lambda_against_oracle(size, dtype, T, block):
    enc = _enc(size, dtype)
    lam = enc.encode_motion(_frames(size)[:T].cuda(), block=block).cpu()
    errs = [rel_l2(lam[t], _oracle_lam(size)[t]) for t in range(T)]
    print(size, dtype, T, block, " ".join("%.2e" % e for e in errs))
    assert lam.shape == (T, 20) and max(errs) < TOL[dtype], errs
    assert enc.saturation() == 0


@pytest.mark.parametrize("T,block", CASES[2:])
@pytest.mark.parametrize("size", [64, 128])
def test_frame_independence_bitwise(size, T, block):
    enc, fr = _enc(size, "fp16"), _frames(size)[:T].cuda()
    lam = enc.encode_motion(fr, block=block)
    for t in range(T):
        assert torch.equal(enc.encode_motion(fr[t:t + 1])[0], lam[t]), t
    assert torch.equal(enc.encode_motion(fr, block=1), lam)


def test_source_state_survives():
    enc = _enc(64, "fp16")
    img = torch.from_numpy(np.random.RandomState(3).rand(1, 3, 64, 64).astype(np.float32)) * 2 - 1
    s_r = enc.encode_image_into_latent(img, want_feats=False)[0]
    before, s_r0 = [b.clone() for b in enc.export_feats16()], s_r.clone()
    enc.encode_motion(_frames(64).cuda(), block=4)
    assert all(torch.equal(a, b) for a, b in zip(before, enc.export_feats16())) and torch.equal(s_r, s_r0)


@pytest.mark.parametrize("mode", ["absolute", "relative"])
def test_drive_rows(mode):
    enc = _enc(64, "fp16")
    lam = enc.encode_motion(_frames(64).cuda())
    src = torch.from_numpy(np.random.RandomState(5).randn(1, 20).astype(np.float32)).cuda()
    dw = W.synth_decoder_state(64, seed=SEED)["direction.weight"]
    q, _ = torch.linalg.qr((dw.float() + 1e-8).double())
    got = enc.drive_rows(lam, mode, lam_source=src)
    want = pkg.host_models.drive_rows(lam.cpu().double(), q, mode, src.cpu().double())
    d = (got.cpu().double() - want).abs().amax(dim=1)
    bound = 20 * 2.0 ** -23 * want.abs().amax(dim=1)
    print(mode, "max|d| / bound %.3f" % float((d / bound).max()))
    assert got.shape == (9, 512) and bool((d <= bound).all()), (d / bound)
    if mode == "relative":
        assert torch.equal(enc.drive_rows(lam, mode, lam_source=src, lam_start=lam[0:1]), got)


def test_driven_route():
    gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
    opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
    opt.input_size, opt.nfe = 64, 6
    acfg = pkg.config.small_audio_config()
    acfg.dim_w = opt.dim_w
    parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31),
                 fmt=W.synth_fmt_state(pkg.config.FmtConfig.from_options(opt), seed=31), audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
    agent = gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8)
    img = (torch.from_numpy(np.random.RandomState(5).rand(1, 3, 64, 64).astype(np.float32)) * 2 - 1).cuda()
    fr = _frames(64).cuda()
    host = agent.drive_device(img, fr, mode="absolute", out_dtype=torch.uint8)
    enc, dec = agent.enc, agent.G.dec
    s_r = enc.encode_image_into_latent(img, want_feats=False)[0]
    enc.hand_feats_to(dec)
    want = dec.decode_u8(s_r, enc.drive_rows(enc.encode_motion(fr), "absolute"))
    assert host.dtype == torch.uint8 and tuple(host.shape) == (9, 64, 64, 3) and torch.equal(host, want.cpu())
    # the reference-shaped call: Encoder.forward(source, target) -> h_motion[0] = lambda of the quantised target frames
    tgt = fr.permute(0, 3, 1, 2).float() / 127.5 - 1
    h_source, h_motion, feats = enc(img, tgt)
    assert len(h_motion) == 1 and torch.equal(h_motion[0], enc.encode_motion(fr)) and torch.equal(h_source, s_r)
    assert len(enc(img, tgt, h_motion[0][0:1])[1]) == 3
