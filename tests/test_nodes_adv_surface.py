"""The advanced (Ad) node family against the contract captured from the reference's nodes_adv classes
(tests/golden/node_surface_adv.json, written by tools/make_adv_surface_golden.py): widgets, return tuples, names, the display
mapping, the node types of the reference's float_adv*.json example graphs, and each node's input validation on a fake pipe."""
import contextlib
import json
import logging
import os

import pytest
import torch

from tests.util import GOLDEN, load_pkg

pkg = load_pkg()
nodes = pkg.NODE_CLASS_MAPPINGS
FIX = json.load(open(os.path.join(GOLDEN, "node_surface_adv.json")))
AD_BUILT = ("FloatImageFaceAlign", "FloatAdvancedParameters", "FloatEncodeImageToLatents", "FloatGetIdentityReference",
            "FloatEncodeAudioToLatentWA", "FloatEncodeEmotionToLatentWE", "FloatSampleMotionSequenceRD", "FloatDecodeLatentsToImages")


def _norm(x):
    if isinstance(x, dict):
        return {k: _norm(v) for k, v in x.items() if k != "tooltip"}  # tooltips are prose
    if isinstance(x, (list, tuple)):
        return [_norm(v) for v in x]
    return json.loads(json.dumps(x, default=str))


def test_ad_node_contracts():
    """Same widgets (name, order, type, default, range; `size` min / max / step included), return tuples and names as the
    reference classes, and the display name with the module's suffix."""
    for name, ref in FIX["classes"].items():
        cls = nodes[name]
        for attr in ("RETURN_TYPES", "RETURN_NAMES"):
            assert list(getattr(cls, attr)) == ref[attr], (name, attr)
        for attr in ("FUNCTION", "CATEGORY", "UNIQUE_NAME", "DISPLAY_NAME"):
            assert getattr(cls, attr) == ref[attr], (name, attr)
        it, rit = _norm(cls.INPUT_TYPES()), ref["INPUT_TYPES"]
        assert list(it) == list(rit), name
        for sect in rit:
            assert list(it[sect].keys()) == list(rit[sect].keys()), (name, sect)
        assert it == rit, name
        assert callable(getattr(cls, cls.FUNCTION))
        assert ref["SUFFIX"] == "(Ad)" and pkg.NODE_DISPLAY_NAME_MAPPINGS[name] == ref["DISPLAY_NAME"] + " (Ad)"
    assert set(FIX["classes"]) == set(AD_BUILT)  # every class of the reference's module is there


def test_ad_example_graph_node_types_are_registered():
    assert len(FIX["workflow_node_types"]) >= 8
    for t in FIX["workflow_node_types"]:
        assert t in nodes, t


def test_fixture_holds_contracts_only():
    """Names, types, defaults, ranges and return tuples - no prose, nothing executable."""
    text = open(os.path.join(GOLDEN, "node_surface_adv.json")).read()
    assert "tooltip" not in text and "def " not in text and "import " not in text and len(text) < 20000


# ---------------------------------------------------------------------------------------------- validation on a fake pipe
class FakePipe:
    rank = "cpu"

    class opt:
        input_size, input_nc, dim_m, dim_w, fps, sampling_rate = 64, 3, 20, 512, 25.0, 16000

    def __init__(self):
        self.calls = []

    @contextlib.contextmanager
    def model_to_target(self):
        yield self

    def face_align_batch(self, images, **kw):
        self.calls.append((tuple(images.shape), kw))
        B, size = images.shape[0], kw["size"]
        crops = torch.arange(B * size * size * 3, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(B, size, size, 3)
        return crops, [(1 + i, 2, 30, 30) for i in range(B)]

    def _host_audio(self, audio):
        w = audio["waveform"][0].mean(0)
        return w[None][:, :int(w[0].item())] if w[0] > 0 else w[None]


def test_face_align_passes_its_widgets_through(caplog):
    pipe = FakePipe()
    node = nodes["FloatImageFaceAlign"]()
    img = torch.rand(2, 40, 30, 4)
    out, boxes = node.process(img, 1.8, "replace_with_color", "#102030", size=64, index=3, float_pipe=pipe)
    assert pipe.calls == [((2, 40, 30, 4), dict(size=64, margin=1.8, index=3, rgba_conversion="replace_with_color", bkg_color_hex="#102030"))]
    want, _ = FakePipe().face_align_batch(img, size=64)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 64, 64, 3) and torch.equal(out, want.float() / 255.0)
    assert boxes == [(1, 2, 30, 30), (2, 2, 30, 30)]
    with caplog.at_level(logging.WARNING):
        out1, boxes1 = node.process(img[0], 1.6, "blend_with_color", "#000000", size=96, float_pipe=pipe)  # 3-D: unsqueezed, with a warning
    assert tuple(out1.shape) == (1, 96, 96, 3) and len(boxes1) == 1 and pipe.calls[-1][1]["index"] == 1
    assert "Missing batch size" in caplog.text and "96" in caplog.text  # ... and 96 is no model size
    with pytest.raises(ValueError):
        node.process(torch.rand(1, 2, 40, 30, 3), 1.6, "blend_with_color", "#000000", float_pipe=pipe)
    with pytest.raises(ValueError):
        node.process(torch.rand(40, 30), 1.6, "blend_with_color", "#000000", float_pipe=pipe)


def test_ad_validation_errors():
    pipe = FakePipe()
    enc = nodes["FloatEncodeImageToLatents"]()
    with pytest.raises(TypeError):
        enc.encode_image_batch([[0.0]], pipe)
    with pytest.raises(ValueError, match="4D"):
        enc.encode_image_batch(torch.zeros(64, 64, 3), pipe)
    with pytest.raises(ValueError, match="64x64"):
        enc.encode_image_batch(torch.zeros(1, 32, 64, 3), pipe)
    with pytest.raises(ValueError, match="channels"):
        enc.encode_image_batch(torch.zeros(1, 64, 64, 4), pipe)
    ident = nodes["FloatGetIdentityReference"]()
    with pytest.raises(TypeError):
        ident.get_identity_reference_batch(None, pipe)
    with pytest.raises(ValueError, match="2D"):
        ident.get_identity_reference_batch(torch.zeros(20), pipe)
    with pytest.raises(ValueError, match="dim_m"):
        ident.get_identity_reference_batch(torch.zeros(2, 19), pipe)
    aud = nodes["FloatEncodeAudioToLatentWA"]()
    with pytest.raises(TypeError):
        aud.encode_audio_to_wa(pipe, {"waveform": torch.zeros(1, 1, 8)}, 25.0)
    with pytest.raises(TypeError):
        aud.encode_audio_to_wa(pipe, {"waveform": [0.0], "sample_rate": 16000}, 25.0)
    with pytest.raises(ValueError, match="2D or 3D"):
        aud.encode_audio_to_wa(pipe, {"waveform": torch.zeros(8), "sample_rate": 16000}, 25.0)
    wav = torch.zeros(2, 1, 8)
    wav[0, 0, 0], wav[1, 0, 0] = 5, 7  # the fake preparation returns 5 and 7 samples: unequal lengths
    with pytest.raises(RuntimeError, match="uniform"):
        aud.encode_audio_to_wa(pipe, {"waveform": wav, "sample_rate": 16000}, 25.0)
    emo = nodes["FloatEncodeEmotionToLatentWE"]()
    with pytest.raises(TypeError):
        emo.encode_emotion_to_we([0.0], pipe, "none")
    with pytest.raises(ValueError, match="2D"):
        emo.encode_emotion_to_we(torch.zeros(8), pipe, "none")
    we, p = emo.encode_emotion_to_we(torch.zeros(3, 8), pipe, "happy")  # a label needs no model
    assert p is pipe and torch.equal(we, torch.nn.functional.one_hot(torch.tensor(3), 7).float()[None, None].repeat(3, 1, 1))
    smp = nodes["FloatSampleMotionSequenceRD"]()
    with pytest.raises(TypeError):
        smp.sample_rd_sequence(torch.zeros(2, 512), None, 5, torch.zeros(2, 1, 7), pipe, 2.0, 1.0, 1)
    with pytest.raises(ValueError, match="Batch size mismatch"):
        smp.sample_rd_sequence(torch.zeros(1, 512), torch.zeros(2, 5, 512), 5, torch.zeros(2, 1, 7), pipe, 2.0, 1.0, 1)
    with pytest.raises(ValueError, match="Batch size mismatch"):
        smp.sample_rd_sequence(torch.zeros(2, 512), torch.zeros(2, 5, 512), 5, torch.zeros(3, 1, 7), pipe, 2.0, 1.0, 1)
    dec = nodes["FloatDecodeLatentsToImages"]()
    app = {"h_source": torch.zeros(2, 512), "feats": [torch.zeros(2, 4, 8, 8)]}
    with pytest.raises(KeyError, match="feats"):
        dec.decode_latents_to_images({"h_source": app["h_source"]}, torch.zeros(2, 3, 512), pipe)
    with pytest.raises(TypeError):
        dec.decode_latents_to_images(app, [0.0], pipe)
    with pytest.raises(TypeError, match="list"):
        dec.decode_latents_to_images({"h_source": app["h_source"], "feats": app["feats"][0]}, torch.zeros(2, 3, 512), pipe)
    with pytest.raises(ValueError, match="Batch size mismatch"):
        dec.decode_latents_to_images(app, torch.zeros(3, 3, 512), pipe)
    with pytest.raises(ValueError, match="Batch size mismatch"):
        dec.decode_latents_to_images({"h_source": app["h_source"], "feats": [torch.zeros(1, 4, 8, 8)]}, torch.zeros(2, 3, 512), pipe)
    empty, fps, p = dec.decode_latents_to_images(app, torch.zeros(2, 0, 512), pipe)  # T = 0 needs no operator
    assert tuple(empty.shape) == (0, 64, 64, 3) and fps == 25.0 and p is pipe
