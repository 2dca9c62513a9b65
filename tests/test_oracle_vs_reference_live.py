"""The oracle next to the reference itself on fresh seeds (not the seeds of the other fixtures), so the oracle is pinned
beyond them: tests/golden/oracle_live_*.npz hold the inputs and what the reference computed from them
(tools/make_goldens.py::gen_oracle_live); the weights come from their seeds."""
import pytest
import torch

from oracle import float_oracle as O
from tests.util import golden_parts, load_pkg, rel_l2

pkg = load_pkg()


@pytest.fixture(scope="module")
def ref():
    return golden_parts("oracle_live")


def test_fmt_eval_and_window_live(ref):
    cfg = pkg.config.small_fmt_config()
    sd = pkg.weights.synth_fmt_state(cfg, seed=77)
    x, wa, wr, we, px, pwa, t = (ref["fmt_" + k] for k in ("x", "wa", "wr", "we", "px", "pwa", "t"))
    want = ref["fmt_out"]
    got = O.fmt_forward_cfv(sd, cfg, t, x, wa, wr, we, px, pwa, None, 1.7, 1.0, 2.2)
    assert rel_l2(got, want) < 1e-5


def test_synthesis_live(ref):
    sd = pkg.weights.synth_decoder_state(64, seed=78)
    feats = pkg.weights.synth_feats(64, seed=78)
    lat, want, flow = ref["dec_lat"], ref["dec_img"], ref["dec_flow"]
    got, gflow, _ = O.synthesis(sd, lat, feats, return_all=True)
    assert float((got - want).abs().max()) < 1e-4 and float((gflow - flow).abs().max()) < 1e-5


def test_encoder_oracle_live(ref):
    sd = pkg.weights.synth_encoder_state(64, seed=79)
    img, s_r, lam = ref["enc_img"], ref["enc_s_r"], ref["enc_lam"]
    feats = [ref["enc_feat%d" % i] for i in range(4)]
    s2, f2, l2 = O.encode_appearance(sd, img)
    assert float((s_r - s2).abs().max()) < 1e-5 and float((lam - l2).abs().max()) < 1e-5
    assert len(f2) == len(feats) and all(float((a - b).abs().max()) < 1e-5 for a, b in zip(feats, f2))
