"""Advanced (Ad) nodes (reference nodes_adv.py): FLOAT Advanced Options, and the seven stage nodes the reference's
`float_adv*.json` example graphs are made of - Face Align, Encode Image to Latents, Get Identity Reference, Encode Audio to
latent wa, Encode Emotion to latent we, Sample Motion Sequence rd, Decode Latents to Images.  Same class attributes, widget
names / defaults / ranges and return tuples as the reference; the bodies drive the operators of the `float_pipe`
(InferenceAgent) one stage at a time, inside float_pipe.model_to_target(), and hand CPU tensors to the next node like there.
The tier is batched throughout: Face Align aligns every item of an IMAGE batch with one detector pass
(InferenceAgent.face_align_batch)."""
import math

import torch

from ... import host_models
from ...fmt import draw_noise
from ...pipeline import report_range
from ...weights import ENC_CHANNELS
from . import EMOTIONS, RGBA_CONVERSION_STRATEGIES, TORCHDIFFEQ_FIXED_STEP_SOLVERS
from . import main_logger as logger
from .options.base_options import BaseOptions

BASE_CATEGORY = "FLOAT/Advanced"
SUFFIX = "(Ad)"


def _num(kind, default, **kw):
    d = {"default": default}
    d.update(kw)
    return (kind, d)


class FloatImageFaceAlign:
    @classmethod
    def INPUT_TYPES(cls):
        practical = [s for s in sorted(ENC_CHANNELS) if s >= 64]  # the model sizes a widget can sensibly offer
        return {
            "required": {
                "image": ("IMAGE", {"tooltip": "A batch of portraits, each with at least one face"}),
                "face_margin": _num("FLOAT", 1.6, min=1.2, max=2.0, step=0.1,
                                    tooltip="Half side of the crop in units of the face box's larger half side"),
                "rgba_conversion": (RGBA_CONVERSION_STRATEGIES, {"default": "blend_with_color",
                                                                 "tooltip": "What becomes of an alpha channel"}),
                "bkg_color_hex": ("STRING", {"default": "#000000", "tooltip": "The colour the two colour strategies use"}),
            },
            "optional": {
                "size": _num("INT", BaseOptions.input_size, min=min(practical), max=max(practical), step=64,
                             tooltip="Side of the square crop; the encoder wants its model size"),
                "index": _num("INT", 1, min=1, max=14, tooltip="Which of the detected faces, best score first"),
            },
        }

    RETURN_TYPES = ("IMAGE", "BBOX")
    RETURN_NAMES = ("image", "bboxes")
    FUNCTION = "process"
    CATEGORY = BASE_CATEGORY
    DESCRIPTION = "Crops every image of the batch to its face, resizes to the model size and converts RGBA to RGB; one detector pass."
    UNIQUE_NAME = "FloatImageFaceAlign"
    DISPLAY_NAME = "Face Align for FLOAT"

    def process(self, image, face_margin, rgba_conversion, bkg_color_hex, size=None, index=1, float_pipe=None):
        """float_pipe: the reference's node has no pipe input (its detector is a process-wide singleton); without one the
        agent loaded last in this process is used (InferenceAgent.latest)."""
        sz = size if size is not None else BaseOptions.input_size
        if sz not in ENC_CHANNELS:
            logger.warning("Provided size %s is not a model size; downstream nodes such as the encoder may refuse it.  Valid sizes: %s",
                           sz, sorted(ENC_CHANNELS))
        if image.ndim == 3:
            logger.warning("Missing batch size")
            image = image.unsqueeze(0)
        if image.ndim != 4:
            raise ValueError("Image shape is incorrect %s" % (tuple(image.shape),))
        pipe = float_pipe if float_pipe is not None else _latest_pipe()
        with pipe.model_to_target():
            crops8, rects = pipe.face_align_batch(image, size=sz, margin=face_margin, index=index, rgba_conversion=rgba_conversion,
                                                  bkg_color_hex=bkg_color_hex)
            out = (crops8.float() / 255.0).to(image.device)
        return (out, [tuple(r) for r in rects])


def _latest_pipe():
    from .generate import InferenceAgent
    pipe = getattr(InferenceAgent, "latest", None)
    pipe = pipe() if pipe is not None else None
    if pipe is None:
        raise RuntimeError("Face Align for FLOAT needs a loaded FLOAT pipe (Load FLOAT Models) in this process: its detector and "
                           "image front end run on that pipe's device")
    return pipe


class FloatAdvancedParameters:
    @classmethod
    def INPUT_TYPES(cls):
        prob = dict(min=0.0, max=1.0, step=0.01, display="number")
        tol = dict(min=1e-9, max=1e-1, step=1e-6, display="number", precision=9)
        return {
            "required": {
                "r_cfg_scale": _num("FLOAT", 1.0, min=1.0, step=0.1),
                "attention_window": _num("INT", 2, min=1, max=10, step=1, display="number"),
                "audio_dropout_prob": _num("FLOAT", 0.1, **prob),
                "ref_dropout_prob": _num("FLOAT", 0.1, **prob),
                "emotion_dropout_prob": _num("FLOAT", 0.1, **prob),
                "ode_atol": _num("FLOAT", 1e-5, **tol),
                "ode_rtol": _num("FLOAT", 1e-5, **tol),
                "nfe": _num("INT", 10, min=1, max=1000, step=1, display="number"),
                "torchdiffeq_ode_method": (TORCHDIFFEQ_FIXED_STEP_SOLVERS, {"default": "euler"}),
                "face_margin": _num("FLOAT", 1.6, min=1.2, max=2.0, step=0.1, display="number"),
                "rgba_conversion": (RGBA_CONVERSION_STRATEGIES, {"default": "blend_with_color"}),
                "bkg_color_hex": ("STRING", {"default": "#000000"}),
            }
        }

    RETURN_TYPES = ("ADV_FLOAT_DICT",)
    RETURN_NAMES = ("advanced_options",)
    FUNCTION = "get_options"
    CATEGORY = BASE_CATEGORY
    DESCRIPTION = "FLOAT Advanced Options"
    UNIQUE_NAME = "FloatAdvancedParameters"
    DISPLAY_NAME = "FLOAT Advanced Options"

    def get_options(self, r_cfg_scale, attention_window, audio_dropout_prob, ref_dropout_prob, emotion_dropout_prob,
                    ode_atol, ode_rtol, nfe, torchdiffeq_ode_method, face_margin, rgba_conversion, bkg_color_hex):
        return (dict(r_cfg_scale=r_cfg_scale, attention_window=attention_window, audio_dropout_prob=audio_dropout_prob,
                     ref_dropout_prob=ref_dropout_prob, emotion_dropout_prob=emotion_dropout_prob, ode_atol=ode_atol,
                     ode_rtol=ode_rtol, nfe=nfe, torchdiffeq_ode_method=torchdiffeq_ode_method, face_margin=face_margin,
                     rgba_conversion=rgba_conversion, bkg_color_hex=bkg_color_hex),)


class FloatEncodeImageToLatents:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"ref_image": ("IMAGE",), "float_pipe": ("FLOAT_PIPE",)}}

    RETURN_TYPES = ("FLOAT_APPEARANCE_PIPE", "TORCH_TENSOR", "FLOAT_PIPE")
    RETURN_NAMES = ("appearance_pipe (Ws→r)", "r_s_lambda_latent", "float_pipe")
    FUNCTION = "encode_image_batch"
    CATEGORY = BASE_CATEGORY
    DESCRIPTION = "Encodes a batch of reference images: appearance pipe {h_source, feats} and the motion coefficients r_s_lambda."
    UNIQUE_NAME = "FloatEncodeImageToLatents"
    DISPLAY_NAME = "FLOAT Encode Image to Latents"

    def encode_image_batch(self, ref_image, float_pipe):
        opt = float_pipe.opt
        if not isinstance(ref_image, torch.Tensor):
            raise TypeError("Input 'ref_image' must be a torch.Tensor, got %s" % type(ref_image))
        if ref_image.ndim != 4:
            raise ValueError("Input 'ref_image' must be a 4D tensor (B, H, W, C), got %dD." % ref_image.ndim)
        _, hh, ww, ch = ref_image.shape
        if hh != opt.input_size or ww != opt.input_size:
            raise ValueError("Input images must be %dx%d. Got %dx%d." % (opt.input_size, opt.input_size, hh, ww))
        if ch != opt.input_nc:
            raise ValueError("Input images must be RGB (channels=%d). Got %d channels." % (opt.input_nc, ch))
        s = ref_image.permute(0, 3, 1, 2).contiguous() * 2.0 - 1.0  # nodes_adv.py:297-299
        s_r, lam, feats = [], [], None
        with float_pipe.model_to_target():
            enc = float_pipe.enc
            for b in range(s.shape[0]):  # the operator's batch is 1 (include/float_hip.h)
                sb, lb, fb, _ = enc.encode_image_into_latent(s[b])
                s_r.append(sb)
                lam.append(lb)
                feats = [[f] for f in fb] if feats is None else [acc + [f] for acc, f in zip(feats, fb)]
            pipe = {"h_source": torch.cat(s_r).cpu(), "feats": [torch.cat(f).cpu() for f in feats]}  # .cpu() synchronises
            lam = torch.cat(lam).cpu()
            if enc.dtype == "fp16":
                report_range({"encoder": enc.saturation(reset=True)}, "FloatEncodeImageToLatents")
        return (pipe, lam, float_pipe)


class FloatGetIdentityReference:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"r_s_lambda_latent": ("TORCH_TENSOR",), "float_pipe": ("FLOAT_PIPE",)}}

    RETURN_TYPES = ("TORCH_TENSOR", "FLOAT_PIPE")
    RETURN_NAMES = ("r_s_latent (Wr→s)", "float_pipe")
    FUNCTION = "get_identity_reference_batch"
    CATEGORY = BASE_CATEGORY
    DESCRIPTION = "r_s = Direction(r_s_lambda): the identity-specific motion reference latent of every item."
    UNIQUE_NAME = "FloatGetIdentityReference"
    DISPLAY_NAME = "FLOAT Get Identity Reference"

    def get_identity_reference_batch(self, r_s_lambda_latent, float_pipe):
        opt = float_pipe.opt
        if not isinstance(r_s_lambda_latent, torch.Tensor):
            raise TypeError("Input 'r_s_lambda_latent' must be a torch.Tensor, got %s" % type(r_s_lambda_latent))
        if r_s_lambda_latent.ndim != 2:
            raise ValueError("Input 'r_s_lambda_latent' must be a 2D tensor (Batch, DimM), got %dD." % r_s_lambda_latent.ndim)
        if r_s_lambda_latent.shape[1] != opt.dim_m:
            raise ValueError("Dimension 1 of 'r_s_lambda_latent' should be opt.dim_m (%d), got %d." % (opt.dim_m, r_s_lambda_latent.shape[1]))
        with float_pipe.model_to_target():
            r_s = float_pipe.G.dec.direction(r_s_lambda_latent).cpu()
        return (r_s, float_pipe)


class FloatEncodeAudioToLatentWA:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"float_pipe": ("FLOAT_PIPE",), "audio": ("AUDIO",), "fps": _num("FLOAT", 25.0, min=1.0, step=0.1)}}

    RETURN_TYPES = ("TORCH_TENSOR", "INT", "TORCH_TENSOR", "FLOAT_PIPE")
    RETURN_NAMES = ("wa_latent", "audio_num_frames", "processed_audio_features", "float_pipe")
    FUNCTION = "encode_audio_to_wa"
    CATEGORY = BASE_CATEGORY
    DESCRIPTION = "Resamples and normalises a batch of audio clips of one length and encodes it into wa (B, T, dim_w)."
    UNIQUE_NAME = "FloatEncodeAudioToLatentWA"
    DISPLAY_NAME = "FLOAT Encode Audio to latent wa"

    def encode_audio_to_wa(self, float_pipe, audio, fps):
        opt = float_pipe.opt
        if not isinstance(audio, dict) or "waveform" not in audio or "sample_rate" not in audio:
            raise TypeError("Input 'audio' must be a ComfyUI AUDIO dictionary.")
        if not isinstance(audio["waveform"], torch.Tensor):
            raise TypeError("audio['waveform'] must be a torch.Tensor.")
        w, rate = audio["waveform"], audio["sample_rate"]
        if w.ndim == 2:
            w = w.unsqueeze(0)
        elif w.ndim != 3:
            raise ValueError("audio['waveform'] must be 2D or 3D, got %dD." % w.ndim)
        with float_pipe.model_to_target():
            # item by item the agent's own preparation (generate.py:69-73): mono mix, resampling to the model's rate - the
            # device front end off 16 kHz, FLOAT_AMD_AUDIO_FRONT honoured - and normalisation, each (1, N) on the device
            items = [float_pipe._host_audio({"waveform": w[i:i + 1], "sample_rate": rate}) for i in range(w.shape[0])]
            if any(a.shape != items[0].shape for a in items):
                raise RuntimeError("Failed to stack the preprocessed audio clips: their lengths differ (%s samples).  The input AUDIO "
                                   "batch must result in uniform processed lengths." % sorted({int(a.shape[-1]) for a in items}))
            a = torch.cat(items)
            opt.fps = fps
            float_pipe.audio_encoder.fps = fps  # the operator's frame arithmetic (its interpolation to T frames) follows the widget
            T = math.ceil(a.shape[1] * opt.fps / opt.sampling_rate)
            wa = float_pipe.audio_encoder.inference(a, seq_len=T).cpu()
            a_cpu = a.cpu()
        return (wa, T, a_cpu, float_pipe)


class FloatEncodeEmotionToLatentWE:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"processed_audio_features": ("TORCH_TENSOR",), "float_pipe": ("FLOAT_PIPE",),
                             "emotion": (EMOTIONS, {"default": "none"})}}

    RETURN_TYPES = ("TORCH_TENSOR", "FLOAT_PIPE")
    RETURN_NAMES = ("we_latent", "float_pipe")
    FUNCTION = "encode_emotion_to_we"
    CATEGORY = BASE_CATEGORY
    DESCRIPTION = "Emotion conditioning we (B, 1, 7): predicted from the normalised audio, or one-hot for a named emotion."
    UNIQUE_NAME = "FloatEncodeEmotionToLatentWE"
    DISPLAY_NAME = "FLOAT Encode Emotion to latent we"

    def encode_emotion_to_we(self, processed_audio_features, float_pipe, emotion):
        if not isinstance(processed_audio_features, torch.Tensor):
            raise TypeError("Input 'processed_audio_features' must be a torch.Tensor, got %s" % type(processed_audio_features))
        if processed_audio_features.ndim != 2:
            raise ValueError("Input 'processed_audio_features' must be a 2D tensor (Batch, NumSamples), got %dD with shape %s."
                             % (processed_audio_features.ndim, tuple(processed_audio_features.shape)))
        B = processed_audio_features.shape[0]
        if host_models.emotion_index(emotion) is not None:
            return (host_models.emotion_one_hot(emotion, "cpu").repeat(B, 1, 1), float_pipe)
        # 'none', or a label the model does not know: the scores of every item from its audio (nodes_adv.py:522-529)
        with float_pipe.model_to_target():
            predict = float_pipe.require_emotion_predictor()
            a = processed_audio_features.to(float_pipe.rank)
            we = torch.stack([predict(a[b:b + 1]).reshape(1, -1) for b in range(B)]).cpu()
        return (we, float_pipe)


class FloatSampleMotionSequenceRD:
    @classmethod
    def INPUT_TYPES(cls):
        f01 = dict(min=0.0, max=10.0, step=0.1)
        return {"required": {
            "r_s_latent": ("TORCH_TENSOR",),
            "wa_latent": ("TORCH_TENSOR",),
            "audio_num_frames": ("INT", {"forceInput": True}),
            "we_latent": ("TORCH_TENSOR",),
            "float_pipe": ("FLOAT_PIPE",),
            "a_cfg_scale": _num("FLOAT", 2.0, **f01),
            "e_cfg_scale": _num("FLOAT", 1.0, **f01),
            "seed": _num("INT", 62064758300528, min=0, max=0xffffffffffffffff),
        }}

    RETURN_TYPES = ("TORCH_TENSOR", "FLOAT_PIPE")
    RETURN_NAMES = ("r_d_latents", "float_pipe")
    FUNCTION = "sample_rd_sequence"
    CATEGORY = BASE_CATEGORY
    DESCRIPTION = "Runs the FMT ODE sampling loop -> r_d latents; evaluations, solver and r_cfg_scale come from the pipe's options."
    UNIQUE_NAME = "FloatSampleMotionSequenceRD"
    DISPLAY_NAME = "FLOAT Sample Motion Sequence rd"

    def sample_rd_sequence(self, r_s_latent, wa_latent, audio_num_frames, we_latent, float_pipe, a_cfg_scale, e_cfg_scale, seed):
        opt = float_pipe.opt
        if not all(isinstance(t, torch.Tensor) for t in (r_s_latent, wa_latent, we_latent)):
            raise TypeError("All latent inputs (r_s, wa, we) must be torch.Tensors.")
        B = wa_latent.shape[0]
        if not (r_s_latent.shape[0] == B and we_latent.shape[0] == B):
            raise ValueError("Batch size mismatch: wa_latent has %d, r_s_latent has %d, we_latent has %d. All must match."
                             % (B, r_s_latent.shape[0], we_latent.shape[0]))
        if wa_latent.shape[1] != audio_num_frames:
            logger.warning("wa_latent time dimension (%d) differs from audio_num_frames (%d); the sequence follows wa_latent.",
                           wa_latent.shape[1], audio_num_frames)
        with float_pipe.model_to_target():
            cfg = float_pipe.cfg
            fmt = float_pipe.G.batched_fmt(B)  # B > 1: the stacked chain (float_fmt_sample_batch)
            n_chunks = int(math.ceil(wa_latent.shape[1] / cfg.num_frames_for_clip))
            # ONE generator for the whole batch, seeded once and drawn chunk by chunk on the target device (nodes_adv.py:578-612);
            # seed == -1 means opt.seed, and without opt.fix_noise_seed and without a seed the global RNG draws (nodes_adv.py:762-787)
            if opt.fix_noise_seed or seed != -1:
                noise = draw_noise(n_chunks, B, cfg, opt.seed if seed == -1 else seed, device=fmt.device)
            else:
                noise = torch.stack([torch.randn(B, cfg.num_frames_for_clip, cfg.dim_w, device=fmt.device) for _ in range(n_chunks)])
            fmt.set_method(getattr(opt, "torchdiffeq_ode_method", "euler"))
            r_d = fmt.sample(r_s_latent, wa_latent, we_latent, noise, opt.nfe, a_cfg_scale, opt.r_cfg_scale, e_cfg_scale, False)
            r_d_cpu = r_d.cpu()  # synchronises
            if fmt.dtype == "fp16":
                report_range({"fmt": fmt.saturation(reset=True)}, "FloatSampleMotionSequenceRD")
        return (r_d_cpu, float_pipe)


class FloatDecodeLatentsToImages:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "appearance_pipe": ("FLOAT_APPEARANCE_PIPE", {"tooltip": "{h_source, feats} of FLOAT Encode Image to Latents (Ws→r)"}),
            "r_d_latents": ("TORCH_TENSOR",),
            "float_pipe": ("FLOAT_PIPE",),
        }}

    RETURN_TYPES = ("IMAGE", "FLOAT", "FLOAT_PIPE")
    RETURN_NAMES = ("images", "fps", "float_pipe")
    FUNCTION = "decode_latents_to_images"
    CATEGORY = BASE_CATEGORY
    DESCRIPTION = "Decodes r_d latents into frames with the appearance pipe of FLOAT Encode Image to Latents: (B*T, H, W, 3)."
    UNIQUE_NAME = "FloatDecodeLatentsToImages"
    DISPLAY_NAME = "FLOAT Decode Latents to Images"

    def decode_latents_to_images(self, appearance_pipe, r_d_latents, float_pipe):
        opt = float_pipe.opt
        try:
            s_r, feats = appearance_pipe["h_source"], appearance_pipe["feats"]
        except KeyError as e:
            raise KeyError("Input 'appearance_pipe' is missing an expected key: %s. It must be the output of a "
                           "FloatEncodeImageToLatents node." % e)
        if not all(isinstance(t, torch.Tensor) for t in (s_r, r_d_latents)):
            raise TypeError("Inputs s_r_latent and r_d_latents must be torch.Tensors.")
        if not (isinstance(feats, list) and all(isinstance(t, torch.Tensor) for t in feats)):
            raise TypeError("appearance_pipe['feats'] must be a list of Tensors.")
        B = s_r.shape[0]
        if not (r_d_latents.shape[0] == B and all(f.shape[0] == B for f in feats)):
            raise ValueError("Batch size mismatch: s_r_latent %d, r_d_latents %d, s_r_feats batch sizes %s. All must match."
                             % (B, r_d_latents.shape[0], [f.shape[0] for f in feats]))
        T = r_d_latents.shape[1]
        if T == 0:
            logger.warning("r_d_latents has 0 frames. Returning empty image batch.")
            return (torch.empty((0, opt.input_size, opt.input_size, opt.input_nc), dtype=torch.float32), opt.fps, float_pipe)
        # frame t of item b decodes s_r[b] + r_d[b, t]; the frames of every item land in ONE pinned host tensor, item b at rows b*T..
        host = torch.empty((B * T, opt.input_size, opt.input_size, opt.input_nc), dtype=torch.float32, pin_memory=True)
        staging = None
        with float_pipe.model_to_target():
            dec = float_pipe.G.dec
            for b in range(B):
                dec.set_feats([f[b:b + 1] for f in feats])
                staging = dec.decode_into_host(s_r[b:b + 1], r_d_latents[b], host[b * T:(b + 1) * T], staging)
            torch.cuda.current_stream(dec.device).synchronize()
            if dec.dtype == "fp16":  # an fp16 decoder that left its range must not hand over black regions silently
                report_range({"decoder": dec.saturation(reset=True)}, "FloatDecodeLatentsToImages")
        del staging
        return (host, opt.fps, float_pipe)
