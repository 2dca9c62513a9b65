"""The colour matrices of the I420 outputs on the GPU (ids 2 / 4 / 6 beside today's 0): the three kernels that form YUV -
dec_flowlast_kernel's I420 instantiation, dec_rgb8_to_i420_kernel and imgp_paste_i420_kernel - share one device function and one
table, and are held bit for bit to host_models.rgb8_to_i420 / paste_i420 with the same matrix.  Every comparison is torch.equal;
there is no tolerance in this file.

The decoder's own frames cannot be steered to the ends of the range, so the paste kernel's inputs carry flat, even-aligned patches
of black, white and the pure primaries and secondaries: there the no-clamp property of the table (full range reaches exactly 0 and
255 on every plane, limited range 16 / 235 and 16 / 240) meets a kernel, and the test first checks on the definition's output
that those values are really there.

InferenceAgent.write_y4m keeps its parameter list (tests/test_img_paste_i420.py holds it); the call with a matrix to choose is
InferenceAgent.write_y4m_matrix."""
import ctypes as C
import functools
import importlib
import io

import numpy as np
import pytest
import torch

from tests.test_img_paste_i420_gpu import held, paste_raw
from tests.util import golden, load_pkg

pkg = load_pkg()
W = pkg.weights
hm = pkg.host_models
to_i420 = hm.rgb8_to_i420
pytestmark = pytest.mark.gpu
NEW = (2, 4, 6)


def _inputs(seed, n):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(1, 512, generator=gen), torch.randn(1, n, 512, generator=gen) * 0.5


def _all_matrices(dec, s_r, r_d):
    """{m: decode_i420(matrix=m)} for 0, 2, 4, 6, each held to rgb8_to_i420(decode_u8(...), m); id 0 and no keyword agree"""
    R = dec.size
    rgb = dec.decode_u8(s_r, r_d).cpu()
    plain = dec.decode_i420(s_r, r_d).cpu()
    assert tuple(plain.shape) == (rgb.shape[0], 3 * R // 2, R)
    out = {0: dec.decode_i420(s_r, r_d, matrix=0).cpu()}
    assert torch.equal(out[0], plain) and torch.equal(plain, to_i420(rgb))
    assert torch.equal(dec.decode_i420(s_r, r_d, matrix=None).cpu(), plain)
    for m in NEW:
        got = dec.decode_i420(s_r, r_d, matrix=m)
        assert got.is_cuda and got.dtype == torch.uint8
        held("%d px, matrix %d" % (R, m), got.cpu(), to_i420(rgb, m))
        assert not torch.equal(got.cpu(), plain)  # a real image: another matrix gives other bytes
        out[m] = got.cpu()
    assert torch.equal(dec.decode_i420(s_r, r_d, matrix="bt709-full").cpu(), out[6])
    assert torch.equal(dec.decode_i420(s_r, r_d).cpu(), plain)  # and back: nothing of the last call's matrix stays on the handle
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the decoder
# ---------------------------------------------------------------------------------------------------------------------------
def test_decoder_converter_route():
    """64 px, 3 frames in batches of 2: the last level runs dec_flow_kernel, dec_rgb8_to_i420_kernel follows it."""
    g = golden("dec_64")
    dec = pkg.decoder.SynthesisHIP(W.synth_decoder_state(64, seed=g["seed"]), 64, 512, "cuda:0", dtype="fp16", max_frames=2)
    dec.set_feats(W.synth_feats(64, seed=g["seed"]))
    _all_matrices(dec, g["s_r"], g["r_d"])


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_decoder_fused_route(dtype, monkeypatch):
    """The default 256-px model (64 channels on the last level, so ToFlow rides in conv2's epilogue and dec_flowlast_kernel's I420
    instantiation forms the planes: what float_dec_create tests), 3 frames in batches of 2 - the smallest size with a workgroup
    seam inside a row.  fp16 once more with FLOAT_DEC_YUV_FUSED=0 (read when the handle is created): the converter on the same
    inputs gives the same bytes."""
    monkeypatch.delenv("FLOAT_DEC_YUV_FUSED", raising=False)
    monkeypatch.delenv("FLOAT_DEC_FLOW_EPI", raising=False)
    sd, feats = W.synth_decoder_state(256, seed=78), W.synth_feats(256, seed=78)
    dec = pkg.decoder.SynthesisHIP(sd, 256, 512, "cuda:0", dtype=dtype, max_frames=2)
    assert dec.feat_shapes()[-1] == (64, 256)  # the fused form's condition, with 256 % 128 == 0 and the two switches unset
    s_r, r_d = _inputs(78, 3)
    dec.set_feats(feats)
    fused = _all_matrices(dec, s_r, r_d)
    if dtype == "fp16":
        dec.close()
        monkeypatch.setenv("FLOAT_DEC_YUV_FUSED", "0")
        conv = pkg.decoder.SynthesisHIP(sd, 256, 512, "cuda:0", dtype=dtype, max_frames=2)
        conv.set_feats(feats)
        for m in NEW:
            held("256 px through the converter, matrix %d" % m, conv.decode_i420(s_r, r_d, matrix=m).cpu(), fused[m])


def test_decoder_hand_over_with_a_matrix():
    """float_dec_frames_host_i420 with matrix 6 into pinned memory, 11 frames in batches of 4 (copy workgroups)."""
    sd, feats = W.synth_decoder_state(64, seed=4), W.synth_feats(64, seed=4)
    s_r, r_d = _inputs(1, 11)
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=4)
    dec.set_feats(feats)
    want = to_i420(dec.decode_u8(s_r, r_d).cpu(), 6)
    host = torch.full((11, 96, 64), 7, dtype=torch.uint8).pin_memory()
    staging = dec.decode_into_host(s_r, r_d, host, out_format="i420", matrix=6)
    torch.cuda.current_stream().synchronize()
    held("hand-over, matrix 6", host, want)
    assert torch.equal(staging.cpu(), want)
    # the format follows the destination where it is unstated, and the next call without a matrix is BT.601 limited range again
    host2 = torch.full((11, 96, 64), 7, dtype=torch.uint8).pin_memory()
    dec.decode_into_host(s_r, r_d, host2, staging)
    torch.cuda.current_stream().synchronize()
    assert torch.equal(host2, to_i420(dec.decode_u8(s_r, r_d).cpu()))
    rgb = torch.full((11, 64, 64, 3), 7, dtype=torch.uint8).pin_memory()
    with pytest.raises(ValueError, match="matrix"):
        dec.decode_into_host(s_r, r_d, rgb, matrix=6)
    with pytest.raises(ValueError, match="matrix"):
        dec.decode_into_host(s_r, r_d, torch.empty(11, 64, 64, 3).pin_memory(), matrix="bt709")
    torch.cuda.synchronize()
    assert int(rgb.min()) == 7  # a refused call wrote nothing


# ---------------------------------------------------------------------------------------------------------------------------
# the paste kernel, at the ends of the range
# ---------------------------------------------------------------------------------------------------------------------------
PATCHES = ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255))


@functools.lru_cache(maxsize=None)
def _patched(seed, *shape):
    """seeded uint8 noise (..., H, W, 3) whose rows H/2 - 2 ... H/2 + 1 - an even start, four rows - hold the eight flat colours in
    even-aligned runs of W // 16 * 2 columns; computed once, shared, never modified"""
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    H, Wd = shape[-3], shape[-2]
    y0, run = (H // 2 - 2) & ~1, Wd // 16 * 2
    for i, c in enumerate(PATCHES):
        x[..., y0:y0 + 4, i * run:(i + 1) * run, :] = torch.tensor(c, dtype=torch.uint8)
    return x


# name -> (source (H, W), T, rect, feather, byte offset of `out`): the boxes lie beside the source's patches (rows H/2 - 2 ...)
PASTE_CASES = {
    "fast_36x48": ((36, 48), 1, (26, 2, 20, 12), 2, 0),            # W % 4 == 0, out 4-byte aligned: the FAST instantiation
    "bytes_34x50_out_plus_1": ((34, 50), 1, (3, 21, 21, 11), 4, 1),  # W % 4 == 2: byte stores, a last cell of two columns
    "two_frames_box_partly_outside_40x44": ((40, 44), 2, (-9, -30, 48, 48), 4, 0),
}


@pytest.mark.parametrize("m", NEW)
@pytest.mark.parametrize("case", sorted(PASTE_CASES))
def test_paste_kernel_reaches_the_ends_of_the_range(case, m):
    src_hw, T, rect, feather, shift = PASTE_CASES[case]
    src, frames = _patched(1, *src_hw, 3), _patched(2, T, 64, 64, 3)
    want = hm.paste_i420(src, frames, rect, feather, matrix=m)
    H = src_hw[0]
    y, c = want[:, :H], want[:, H:]
    cc = c.reshape(T, -1)  # the U plane, then the V plane, H W / 4 bytes each
    u, v = cc[:, :cc.shape[1] // 2], cc[:, cc.shape[1] // 2:]
    ends = {"Y": (0, 255), "U": (0, 255), "V": (0, 255)} if m & 4 else {"Y": (16, 235), "U": (16, 240), "V": (16, 240)}
    for name, plane in (("Y", y), ("U", u), ("V", v)):
        lo, hi = int(plane.min()), int(plane.max())
        print("  %s, matrix %d: %s in [%d, %d]" % (case, m, name, lo, hi))
        # the condition of the test, on the definition's output: without these values it shows nothing about the no-clamp property
        assert (lo, hi) == ends[name], "vacuous: %s of the expected frames does not reach %s" % (name, ends[name])
    assert not torch.equal(want, hm.paste_i420(src, frames, rect, feather))
    _, _, got = paste_raw(src.cuda(), frames.cuda(), rect, feather, shift=shift, matrix=m)
    held("%s, matrix %d" % (case, m), got, want)


def test_paste_wrapper_takes_the_matrix():
    src, frames, rect = _patched(1, 36, 48, 3), _patched(2, 1, 64, 64, 3), (26, 2, 20, 12)
    P = pkg.image.paste_frames_device
    plain = P(src, frames, rect, 2, out_format="i420").cpu()
    assert torch.equal(plain, hm.paste_i420(src, frames, rect, 2)) and torch.equal(P(src, frames, rect, 2, out_format="i420", matrix=0).cpu(), plain)
    for m, name in ((2, "bt709"), (4, "bt601-full"), (6, "bt709-full")):
        want = hm.paste_i420(src, frames, rect, 2, matrix=m)
        assert torch.equal(P(src, frames, rect, 2, out_format="i420", matrix=m).cpu(), want)
        assert torch.equal(P(src, frames, rect, 2, out_format="i420", matrix=name).cpu(), want)
    assert torch.equal(P(src, frames, rect, 2, out_format="i420", matrix="auto").cpu(), plain)  # 48 x 36: BT.601
    for kw in (dict(out_format="rgb", matrix="bt709"), dict(matrix=2), dict(out_format="i420", matrix=1), dict(out_format="i420", matrix="bt2020")):
        with pytest.raises(ValueError, match="matrix"):
            P(src, frames, rect, 2, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# argument rules with a device present
# ---------------------------------------------------------------------------------------------------------------------------
def test_unknown_ids_are_refused_by_all_three_entry_points():
    L = pkg.native.lib()
    sd, feats = W.synth_decoder_state(64, seed=4), W.synth_feats(64, seed=4)
    s_r, r_d = _inputs(1, 2)
    dec = pkg.decoder.SynthesisHIP(sd, 64, 512, "cuda:0", max_frames=2)
    dec.set_feats(feats)
    s, r = s_r.cuda().reshape(-1).contiguous(), r_d.cuda().reshape(-1, 512).contiguous()
    out = torch.full((2, 96, 64), 77, dtype=torch.uint8, device="cuda:0")
    host = torch.full((2, 96, 64), 77, dtype=torch.uint8).pin_memory()
    st = pkg.native.stream_ptr(out.device)
    src, frames = _patched(1, 36, 48, 3).cuda(), _patched(2, 1, 64, 64, 3).cuda()
    pout = torch.full((54, 48), 77, dtype=torch.uint8, device="cuda:0")
    for m in (1, 8):
        rc = L.float_dec_frames_i420(dec._h, pkg.native.dev_ptr(s), pkg.native.dev_ptr(r), 2, m, C.c_void_p(out.data_ptr()), st)
        assert rc == 1 and b"matrix" in L.float_last_error() and b"float_dec_frames_i420" in L.float_last_error()
        rc = L.float_dec_frames_host_i420(dec._h, pkg.native.dev_ptr(s), pkg.native.dev_ptr(r), 2, m, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(host.data_ptr()), st, None)
        assert rc == 1 and b"matrix" in L.float_last_error() and b"float_dec_frames_host_i420" in L.float_last_error()
        rc = L.float_img_paste_i420(C.c_void_p(src.data_ptr()), 36, 48, C.c_void_p(frames.data_ptr()), 1, 64, 64, 26, 2, 20, 12, 2, m,
                                    C.c_void_p(pout.data_ptr()), st)
        assert rc == 1 and b"matrix" in L.float_last_error() and b"float_img_paste_i420" in L.float_last_error()
        with pytest.raises(ValueError, match="matrix"):
            dec.decode_i420(s_r, r_d, matrix=m)
    torch.cuda.synchronize()
    assert int(out.min()) == 77 and int(host.min()) == 77 and int(pout.min()) == 77 and int(pout.max()) == 77  # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------------
# through the product: the synthetic 64-px agent
# ---------------------------------------------------------------------------------------------------------------------------
SEED = 7
_cache = {}


def _agent():
    if "agent" not in _cache:
        gen = importlib.import_module(pkg.__name__ + ".src.nodes.generate")
        opt = importlib.import_module(pkg.__name__ + ".src.nodes.options.base_options").BaseOptions()
        opt.input_size, opt.nfe = 64, 6
        cfg = pkg.config.FmtConfig.from_options(opt)
        acfg = pkg.config.small_audio_config()
        acfg.dim_w = opt.dim_w
        parts = dict(enc=W.synth_encoder_state(64, seed=31), dec=W.synth_decoder_state(64, seed=31), fmt=W.synth_fmt_state(cfg, seed=31),
                     audio_encoder=(W.synth_audio_state(acfg, seed=31), acfg))
        _cache["agent"] = gen.InferenceAgent(opt, parts, "cuda:0", max_frames=8)
    return _cache["agent"]


def _clean_env(monkeypatch):
    for v in ("FLOAT_AMD_VERIFY", "FLOAT_AMD_VERIFY_ACTION", "FLOAT_AMD_VERIFY_FRAMES", "FLOAT_AMD_VERIFY_PSNR", "FLOAT_AMD_OVERLAP",
              "FLOAT_AMD_IMAGE_FRONT"):
        monkeypatch.delenv(v, raising=False)


def _crop_inputs():
    img = torch.from_numpy(np.random.RandomState(5).rand(1, 3, 64, 64).astype(np.float32)) * 2 - 1
    return img.cuda(), W.synth_waveform(2.4, seed=9).cuda()  # 60 frames: two windows


def _crop_u8():
    if "u8" not in _cache:
        img, wav = _crop_inputs()
        _cache["u8"] = _agent().infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=SEED, out_dtype=torch.uint8).clone()
    return _cache["u8"]


def test_agent_infer_device_with_a_matrix(monkeypatch):
    _clean_env(monkeypatch)
    agent = _agent()
    img, wav = _crop_inputs()
    run = lambda **kw: agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=SEED, **kw)  # noqa: E731
    u8 = _crop_u8()
    assert tuple(u8.shape) == (60, 64, 64, 3)
    got = run(out_format="i420", matrix="bt709")
    assert got.is_pinned() and tuple(got.shape) == (60, 96, 64)
    held("infer_device(matrix='bt709')", got, to_i420(u8, 2))
    assert torch.equal(run(out_format="i420", matrix="auto"), to_i420(u8))  # 64 x 64: BT.601 limited range, today's bytes
    assert torch.equal(run(out_format="i420"), to_i420(u8))
    mine = torch.full((60, 96, 64), 7, dtype=torch.uint8).pin_memory()
    assert run(out=mine, matrix=6) is mine and torch.equal(mine, to_i420(u8, 6))  # a 3-d uint8 destination is I420
    # a matrix with RGB frames is refused before any launch
    rgb = torch.full((60, 64, 64, 3), 7, dtype=torch.uint8).pin_memory()
    for kw in (dict(out_format="rgb", matrix="bt709"), dict(matrix="bt709"), dict(out_dtype=torch.uint8, matrix=2), dict(out=rgb, matrix="auto"),
               dict(out_format="i420", matrix="bt2020"), dict(out_format="i420", matrix=1)):
        with pytest.raises(ValueError, match="matrix"):
            run(**kw)
    torch.cuda.synchronize()
    assert int(rgb.min()) == 7
    with pytest.raises(ValueError, match="matrix"):
        agent.infer_device_batch([(img, wav)], 2.0, 1.0, 1.0, emo="happy", seeds=[SEED], out_dtype=torch.uint8, matrix="bt709")


def test_agent_stream_device_with_a_matrix(monkeypatch):
    _clean_env(monkeypatch)
    agent = _agent()
    img, wav = _crop_inputs()
    u8 = _crop_u8()
    blocks = [(b.first, b.last, b.frames.clone())
              for b in agent.stream_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=SEED, out_format="i420", matrix="bt601-full")]
    assert [(f, l) for f, l, _ in blocks] == [(0, 50), (50, 60)]
    whole = agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=SEED, out_format="i420", matrix="bt601-full")
    held("stream_device(matrix='bt601-full') against the whole clip", torch.cat([fr for _, _, fr in blocks]), whole)
    held("and against the definition", whole, to_i420(u8, 4))
    with pytest.raises(ValueError, match="matrix"):
        agent.stream_device(img, wav, out_dtype=torch.uint8, matrix="bt709")  # at the call: no generator exists
    with pytest.raises(ValueError, match="matrix"):
        agent.stream_device(img, wav, matrix="bt709")
    assert tuple(agent.infer_device(img, wav, 2.0, 1.0, 1.0, emo="happy", seed=SEED, out_dtype=torch.uint8).shape) == (60, 64, 64, 3)  # no stream left open


def _portrait(seed, H, Wd):
    return torch.from_numpy(np.random.RandomState(seed).uniform(-0.1, 1.1, size=(1, H, Wd, 3)).astype(np.float32))


def _audio5():
    return {"waveform": W.synth_waveform(0.2, seed=9).reshape(1, 1, -1), "sample_rate": 16000}  # 5 frames


def _stub_detector(monkeypatch):
    class Detector:
        def detect_from_image(self, arr):
            h, w = arr.shape[0], arr.shape[1]
            return [(0.31 * w, 0.27 * h, 0.55 * w, 0.66 * h, 0.99)]

    class FA:
        face_detector = Detector()

    monkeypatch.setattr(hm, "_FA", FA())


def _pasted_definition(agent, img, matrix, no_crop):
    """paste_i420 of the clip's own 8-bit crops at the agent's own box"""
    s, a, place = agent.host_inputs_placed(img, _audio5(), no_crop=no_crop)
    crops = agent.infer_device(s, a, emo="happy", seed=SEED, out_dtype=torch.uint8)
    rect = tuple(place.rect)
    return hm.paste_i420(hm.image_to_rgb8(img[0]), crops, rect, hm.default_feather(rect), matrix=matrix), rect


def test_agent_infer_pasted_auto_goes_by_the_portraits_size(monkeypatch):
    _clean_env(monkeypatch)
    _stub_detector(monkeypatch)
    agent = _agent()
    kw = dict(emo="happy", no_crop=False, seed=SEED)
    hd = _portrait(21, 720, 1280)
    want709, rect = _pasted_definition(agent, hd, 2, False)
    got = agent.infer_pasted(hd, _audio5(), out_format="i420", matrix="auto", **kw)
    assert tuple(got.shape) == (5, 1080, 1280) and 0 < rect[0] and rect[0] + rect[2] < 1280  # a box inside the portrait
    held("infer_pasted(matrix='auto') at 1280 x 720 is BT.709 limited range", got, want709)
    assert not torch.equal(got, agent.infer_pasted(hd, _audio5(), out_format="i420", **kw))  # the default did not move to "auto"
    sd = _portrait(22, 64, 64)
    want601, _ = _pasted_definition(agent, sd, 0, True)
    kw["no_crop"] = True
    held("infer_pasted(matrix='auto') at 64 x 64 is BT.601 limited range",
         agent.infer_pasted(sd, _audio5(), out_format="i420", matrix="auto", **kw), want601)
    for call in (lambda: agent.infer_pasted(sd, _audio5(), matrix="bt709", **kw),
                 lambda: agent.infer_pasted(sd, _audio5(), out_format="rgb", matrix="auto", **kw),
                 lambda: agent.stream_pasted(sd, _audio5(), matrix=6, **kw),
                 lambda: agent.infer_pasted(sd, _audio5(), out_format="i420", matrix="bt2020", **kw)):
        with pytest.raises(ValueError, match="matrix"):
            call()


def test_agent_write_y4m_matrix_pasted_full_range(monkeypatch, tmp_path):
    _clean_env(monkeypatch)
    _stub_detector(monkeypatch)
    agent = _agent()
    kw = dict(emo="happy", no_crop=False, seed=SEED)
    img = _portrait(23, 90, 120)
    want, _ = _pasted_definition(agent, img, 6, False)
    buf = io.BytesIO()
    assert agent.write_y4m_matrix(buf, img, _audio5(), paste_back=True, matrix="bt709-full", **kw) == 5
    data = buf.getvalue()
    header, _, rest = data.partition(b"\n")
    assert header == b"YUV4MPEG2 W120 H90 F%d:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL" % int(agent.opt.fps)
    n = 90 * 120 * 3 // 2
    assert len(rest) == 5 * (6 + n)
    for t in range(5):
        chunk = rest[t * (6 + n):(t + 1) * (6 + n)]
        assert chunk[:6] == b"FRAME\n" and chunk[6:] == want[t].numpy().tobytes(), t
    # no matrix: write_y4m's bytes; at the model's size the tag follows the id as well
    a, b = io.BytesIO(), io.BytesIO()
    agent.write_y4m(a, img, _audio5(), paste_back=True, **kw)
    agent.write_y4m_matrix(b, img, _audio5(), paste_back=True, **kw)
    assert a.getvalue() == b.getvalue() and b"XCOLORRANGE=LIMITED" in a.getvalue()[:80]
    c = io.BytesIO()
    agent.write_y4m_matrix(c, img, _audio5(), matrix=4, **kw)
    s, au = agent.host_inputs(img, _audio5(), no_crop=False)
    ref = io.BytesIO()
    hm.write_y4m(ref, agent.infer_device(s, au, emo="happy", seed=SEED, out_format="i420", matrix=4), agent.opt.fps, matrix=4)
    assert c.getvalue() == ref.getvalue() and b"W64 H64" in c.getvalue()[:32] and b"XCOLORRANGE=FULL" in c.getvalue()[:80]
    path = tmp_path / "never.y4m"
    with pytest.raises(ValueError, match="matrix"):
        agent.write_y4m_matrix(str(path), img, _audio5(), paste_back=True, matrix="bt2020", **kw)
    with pytest.raises(ValueError, match="matrix"):
        agent.write_y4m_matrix(str(path), img, _audio5(), matrix=3, **kw)
    assert not path.exists()  # refused before a file is opened
