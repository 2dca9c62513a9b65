"""InferenceAgent of the MI355X build (reference generate.py:84-173): owns the weights, the host-side
conditioning encoders and the HIP hot path, and exposes run_inference with the reference signature."""
import contextlib
import math
import os
import weakref

import torch

from ... import host_models, weights
from ...audio import Audio2EmotionHIP, AudioEncoderHIP, preprocess_audio_device
from ...config import AudioConfig, FmtConfig, emotion_audio_config, small_audio_config, small_emotion_config
from ...encoder import EncoderHIP
from ...face import FaceDetectorHIP, find_sfd_weights, load_sfd_state
from ...image import (detector_view_device, front_takes, image_front_device, image_to_device, paste_format, preprocess_image_device, require_even_sides,
                      require_jpeg_sides, source_rgb8_device)
from ...pipeline import FloatHotPath, Placement, resolve_out_format, precision_policy, report_precision, report_range, verify_frames_default
from . import SYNTHETIC_MODEL, main_logger

# key prefixes of the unified checkpoint (utils/downloader.py:35-42)
PREFIXES = {
    "enc": "motion_autoencoder.enc.",
    "dec": "motion_autoencoder.dec.",
    "proj": "audio_encoder.audio_projection.",
    "fmt": "fmt.",
    "wav2vec": "audio_encoder.wav2vec2.",
    "ser": "emotion_encoder.wav2vec2_for_emotion.",
}


def split_unified(state):
    """FLOAT.state_dict() -> per-part dicts with the prefixes stripped."""
    parts = {k: {} for k in PREFIXES}
    for key, v in state.items():
        for part, pre in PREFIXES.items():
            if key.startswith(pre):
                parts[part][key[len(pre):]] = v
                break
    return parts


class InferenceAgent:
    latest = None  # weakref to the agent built last in this process: the pipe of the one Ad node that has no pipe input (Face Align)

    def __init__(self, opt, parts=None, device=None, max_frames=32, use_graph=2, fmt_dtype=None, dec_dtype=None, aud_dtype=None):
        InferenceAgent.latest = weakref.ref(self)
        self.opt = opt
        self.rank = torch.device(device if device is not None else getattr(opt, "rank", "cuda:0"))
        self.cfg = FmtConfig.from_options(opt)
        if parts is None:
            parts = self._load_parts(opt)
        self.dec_sd = parts["dec"]
        # the host copy of the weights stays with the agent (the reference's offload device, nodes.py:139): offload() frees
        # every device allocation, to_target() rebuilds the operators from here
        self._parts = parts
        from ... import native as _native
        canon = _native.canon_dtype  # 'float16' and 'fp16' are one type to every later `== "fp16"` test
        self._build = dict(max_frames=max_frames, use_graph=use_graph,
                           fmt_dtype=canon(fmt_dtype or os.environ.get("FLOAT_AMD_FMT_DTYPE", "fp16")),
                           dec_dtype=canon(dec_dtype or os.environ.get("FLOAT_AMD_DEC_DTYPE", "fp16")),
                           aud_dtype=canon(aud_dtype or os.environ.get("FLOAT_AMD_AUD_DTYPE", "fp16")))
        self.G = None
        self._drop_caches()
        self.last_precision_report = None  # check_precision (FLOAT_AMD_VERIFY) keeps its last report here
        self.to_target()

    # ------------------------------------------------------------------ residency (reference: model_to_target, nodes.py:173-175)
    def to_target(self):
        """Build the HIP operators on self.rank from the host weights if they are not resident (no-op otherwise)."""
        if self.G is not None:
            return self
        opt, parts, b = self.opt, self._parts, self._build
        self._precision_checked = False  # FLOAT_AMD_VERIFY=first: the first clip after the operators were (re)built
        # 16-bit MFMA operand types (fp32 accumulation): fp16 in both operators gives ~8x lower rounding error than
        # bf16 at the same rate (end-to-end 48.7 vs 34.1 dB on BASELINE configs[0]); FLOAT_AMD_FMT_DTYPE=bf16
        # selects the type BASELINE configs[1] names.
        self.G = FloatHotPath(parts["fmt"], parts["dec"], self.cfg, self.rank, opt.input_size, fmt_dtype=b["fmt_dtype"],
                              dec_dtype=b["dec_dtype"], max_frames=b["max_frames"], use_graph=b["use_graph"])
        self.G.fmt.set_method(getattr(opt, "torchdiffeq_ode_method", "euler"))
        # appearance encoder + Encoder.fc + Direction as one HIP operator (float_enc_*); same 16-bit type as the
        # decoder so the skip features go to it without an fp32 round trip
        self.enc = EncoderHIP(parts["enc"], opt.input_size, opt.dim_w, getattr(opt, "dim_m", 20), self.rank,
                              dtype=self.G.dec.dtype, direction_weight=parts["dec"]["direction.weight"])
        # wav2vec2 + audio projection as one HIP operator (float_aud_*)
        aud_sd, aud_cfg = parts["audio_encoder"]
        self.audio_encoder = AudioEncoderHIP(aud_sd, aud_cfg, self.rank, dtype=b["aud_dtype"], sampling_rate=opt.sampling_rate, fps=opt.fps)
        # speech-to-emotion (emotion="none"): the wav2vec2-large variant of the same operator with its classification head
        ser = parts.get("emotion_encoder")
        self.emotion_encoder = Audio2EmotionHIP(ser[0], ser[1], self.rank, dtype=b["aud_dtype"]) if ser is not None else None
        # callable(a) -> (1,7) softmax scores; None disables emotion="none"
        self.emotion_predictor = self.emotion_encoder.predict_emotion if ser is not None else parts.get("emotion_predictor")
        return self

    def offload(self):
        """Free every device allocation of the agent (packed weights, workspaces, hipGraphs, staging and cached tensors:
        ~6.5 GB at the default shapes) - the counterpart of the reference moving G back to the offload device after a node
        call.  The next call rebuilds the operators from the host weights (to_target); results are bitwise the same."""
        if self.G is None:
            return
        torch.cuda.current_stream(self.rank).synchronize()
        for op in [self.G.fmt, self.G.dec, self.enc, self.audio_encoder, self.emotion_encoder, self.face] + list(self.G._fmt_batched.values()):
            if op is not None:
                op.close()
        if self.emotion_encoder is not None:
            self.emotion_predictor = None
        self.G = self.enc = self.audio_encoder = self.emotion_encoder = None
        self._drop_caches()
        with torch.cuda.device(self.rank):
            torch.cuda.empty_cache()

    def _drop_caches(self):
        """Everything the agent caches between clips besides the operators, empty: what __init__ declares and offload() frees."""
        self._we_cache = {}        # {emotion index: (1,1,7) one-hot on the device} (_one_hot)
        self._noise_pin = self._noise_pin_b = self._noise_pin_r = None  # pinned noise of one clip / a batch / a ragged batch (_draw_noise)
        self._feat_slots = []      # per batch item, the encoder's skip maps copied aside (infer_device_batch)
        self._side_stream = None   # the speech-emotion model's stream (_cond_stream)
        self.face = None           # the face detector (float_sfd_*), built on first use (_face_detector)
        self._face_key = None      # (weight file, dtype) it was built from

    @property
    def resident(self):
        return self.G is not None

    @contextlib.contextmanager
    def model_to_target(self, offload_after=None):
        """The reference wraps every node call in `with model_to_target(logger, float_pipe.G)` (nodes.py:173-175): operators
        on the target device inside, back on the offload device after.  Here staying resident is the default (288 GB of
        HBM; a rebuild costs seconds of host packing): offload_after=True, or FLOAT_AMD_OFFLOAD=always, gives the reference's
        behaviour; FLOAT_AMD_OFFLOAD=never (default) keeps the operators."""
        self.to_target()
        try:
            yield self
        finally:
            if offload_after if offload_after is not None else os.environ.get("FLOAT_AMD_OFFLOAD", "never").lower() == "always":
                self.offload()

    # ------------------------------------------------------------------ weights
    @staticmethod
    def _load_parts(opt):
        path = getattr(opt, "ckpt_path", None)
        if path is None or os.path.basename(path) == SYNTHETIC_MODEL or os.environ.get("FLOAT_AMD_SYNTHETIC") == "1":
            return InferenceAgent.synthetic_parts(opt)
        if not os.path.exists(path):
            raise FileNotFoundError("Checkpoint file not found: %s" % path)
        from safetensors.torch import load_file
        parts = split_unified(load_file(path, device="cpu"))
        aud_sd = {"wav2vec2." + k: v for k, v in parts["wav2vec"].items()}
        aud_sd.update({"audio_projection." + k: v for k, v in parts["proj"].items()})
        parts["audio_encoder"] = (aud_sd, AudioConfig(dim_w=opt.dim_w, only_last_features=opt.only_last_features))
        if parts["ser"]:
            parts["emotion_encoder"] = (parts["ser"], emotion_audio_config())
        return parts

    @staticmethod
    def synthetic_parts(opt, seed=0):
        """Seeded random weights in the checkpoint layout (no network / no checkpoint available)."""
        cfg = FmtConfig.from_options(opt)
        acfg = small_audio_config()
        acfg.dim_w = opt.dim_w
        return dict(enc=weights.synth_encoder_state(opt.input_size, seed=seed), dec=weights.synth_decoder_state(opt.input_size, seed=seed),
                    fmt=weights.synth_fmt_state(cfg, seed=seed),
                    audio_encoder=(weights.synth_audio_state(acfg, seed=seed), acfg),
                    emotion_encoder=(weights.synth_audio_state(small_emotion_config(), seed=seed), small_emotion_config()))

    # ------------------------------------------------------------------ inference
    def _one_hot(self, emo):
        """(1,1,7) one-hot of a label on the device, made once per label (a fresh one costs a blocking scalar upload per clip)."""
        cache = self._we_cache
        idx = host_models.emotion_index(emo)
        if idx not in cache:
            cache[idx] = host_models.emotion_one_hot(emo, "cpu").to(self.rank)
        return cache[idx]

    def _draw_noise(self, pin, shape, clips, at):
        """The noise of `clips` = [(seed, n_windows)] as ONE fp32 device tensor of `shape`; at(buf, i, k) is the (1, L, W) view
        of it that window k of clip i goes to.  Every clip draws what it would draw alone: a generator seeded once per clip and
        drawn window after window in (1, L, W) pieces - the reference's sequential draws (fmt.draw_noise; FLOAT.py:203-215).
        Default: the CPU generator's stream (the reference run on the CPU, what the goldens and the oracle use), written
        straight into the pinned buffer kept under the attribute `pin` and sent by ONE non-blocking copy: the host neither waits
        for the encoder kernels queued in front of the copy nor leaves the GPU idle behind them.  The buffer is kept until the
        next draw of that layout (which starts after this clip was synchronised).  FLOAT_AMD_NOISE=device: "the reference on
        this device", torch.Generator(rank) + randn on the device per window - the stream a user of the reference on ROCm
        gets.  The two streams differ, the sampler does not."""
        c = self.cfg
        on_device = os.environ.get("FLOAT_AMD_NOISE", "cpu").lower() == "device"
        if on_device:
            buf = torch.empty(shape, dtype=torch.float32, device=self.rank)
        else:
            buf = getattr(self, pin)
            if buf is None or tuple(buf.shape) != shape:
                buf = torch.empty(shape, dtype=torch.float32, pin_memory=True)
                setattr(self, pin, buf)
        for i, (seed, n) in enumerate(clips):
            g = torch.Generator(self.rank if on_device else "cpu")
            g.manual_seed(int(seed))
            for k in range(n):
                torch.randn(1, c.num_frames_for_clip, c.dim_w, generator=g, out=at(buf, i, k))
        return buf if on_device else buf.to(self.rank, non_blocking=True)

    def _noise_to_device(self, n_chunks, seed):
        """(n_chunks, 1, L, W): the noise of one clip (_draw_noise)."""
        c = self.cfg
        return self._draw_noise("_noise_pin", (n_chunks, 1, c.num_frames_for_clip, c.dim_w), [(seed, n_chunks)], lambda buf, i, k: buf[k])

    def _noise_batch_to_device(self, n_chunks, seeds):
        """(n_chunks, B, L, W): item i draws what _noise_to_device draws for it alone from seeds[i]."""
        c = self.cfg
        return self._draw_noise("_noise_pin_b", (n_chunks, len(seeds), c.num_frames_for_clip, c.dim_w), [(sd, n_chunks) for sd in seeds],
                                lambda buf, i, k: buf[k, i:i + 1])

    def _noise_ragged_to_device(self, n_chunks, seeds):
        """[(n_chunks[i], L, W)]: item i draws what _noise_to_device draws for it alone (seeds[i], n_chunks[i] sequential draws)."""
        c, first = self.cfg, [sum(n_chunks[:i]) for i in range(len(n_chunks))]
        noise = self._draw_noise("_noise_pin_r", (sum(n_chunks), c.num_frames_for_clip, c.dim_w), list(zip(seeds, n_chunks)),
                                 lambda buf, i, k: buf[first[i] + k:first[i] + k + 1])
        return list(noise.split(list(n_chunks)))

    NO_EMOTION_MODEL = ("emotion='none' asks the speech-emotion model for scores (FLOAT.py:196-198) but the checkpoint has "
                        "no `emotion_encoder.wav2vec2_for_emotion.` weights - pick an emotion or attach agent.emotion_predictor")

    def require_emotion_predictor(self):
        """The callable (1, N) normalised audio -> (1, 7) scores, or the error conditions_device raises without one."""
        if self.emotion_predictor is None:
            raise NotImplementedError(self.NO_EMOTION_MODEL)
        return self.emotion_predictor

    @torch.no_grad()
    def conditions_device(self, s, a, emo=None):
        """Once-per-clip stage on HIP operators, inputs already in HBM: s (1,3,H,W) in [-1,1] -> (s_r, feats handed to the
        decoder, r_s); a (N,) the normalised 16 kHz waveform -> (wa, T); and for any `emo` that is not one of the seven labels
        (None, 'none', 'S2E', ...) the speech-emotion scores (FLOAT.py:196-198).
        emo = "dynamic" or ("dynamic", chunk_sec): one emotion vector per frame, `we` (1, T, 7) - the scores of every chunk of
        chunk_sec seconds (default opt.wav2vec_sec), each normalised on its own, nearest-expanded to the T frames
        (Audio2EmotionHIP.predict_emotion_chunks: one stacked pass on the device, the reference's dynamic-emotion node).  `a`
        is the clip-normalised waveform; a chunk's own normalisation is invariant under that positive affine map."""
        o = self.opt
        if self.G is not None:
            self.G.require_no_stream("conditions_device")  # it hands this clip's skip features to the decoder an open stream reads
        dyn_sec = host_models.dynamic_emotion_chunk_sec(emo, getattr(o, "wav2vec_sec", 2.0))
        if dyn_sec is not None:
            emo = None  # scores from the audio
        if host_models.emotion_index(emo) is None and (self.emotion_predictor is None or (dyn_sec is not None and self.emotion_encoder is None)):
            raise NotImplementedError(self.NO_EMOTION_MODEL)
        T = math.ceil(a.shape[-1] * o.fps / o.sampling_rate)  # FLOAT.py:192
        need_ser = host_models.emotion_index(emo) is None
        # The speech-emotion model (emotion = "none", the reference's default widget) is independent of the other two producers
        # and the longest of the three (2.6 ms of ~200 small launches against 0.9 + 1.2): it runs on a side stream beside them
        # and joins before the FMT starts (111.8 -> 111.1 ms per clip, same box).  Only here: a second ACTIVE queue during the FMT chain
        # costs it 12 ms; and not for the label case - encoder || audio encoder on two streams measured
        # 0.45 ms SLOWER than one after the other (the stream hand-offs cost more than the 0.9 ms they hide).
        cur = torch.cuda.current_stream(self.rank)
        side = self._cond_stream() if (need_ser and os.environ.get("FLOAT_AMD_COND_STREAMS", "1") != "0") else None
        we = None
        if need_ser:
            if side is not None:
                side.wait_stream(cur)  # `a` was produced on the caller's stream
            with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                if dyn_sec is not None:
                    chunk = host_models.dynamic_emotion_plan(a.shape[-1], o.sampling_rate, dyn_sec, o.fps)[0]
                    we = self.emotion_encoder.predict_emotion_chunks(a.reshape(-1), chunk, T)[1][None]
                else:
                    we = self.emotion_predictor(a).reshape(1, 1, -1).to(self.rank)
        wa = self.audio_encoder.inference(a, seq_len=T)
        s_r, _, _, r_s = self.enc.encode_image_into_latent(s, want_feats=False)  # FLOAT.py:283-291
        self.enc.hand_feats_to(self.G.dec)
        if side is not None:
            cur.wait_stream(side)
            we.record_stream(cur)  # allocated on the side stream, consumed on the caller's
        if we is None:
            we = self._one_hot(emo)
        return dict(s_r=s_r, feats=None, r_s=r_s, wa=wa, we=we, T=T)  # feats: already in the decoder (NHWC 16-bit)

    def _cond_stream(self):
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(self.rank)
        return self._side_stream

    def host_inputs(self, ref_img, ref_audio, no_crop=True):
        """Host plumbing of the reference's DataProcessor (generate.py:34-81): optional face crop, area resize to the model
        size, [-1,1]; mono, resample to 16 kHz, normalise.  Returns (s (1,3,H,W), a (N,)) on the device."""
        return self._host_inputs(ref_img, ref_audio, no_crop, False)[:2]

    def host_inputs_placed(self, ref_img, ref_audio, no_crop=True):
        """host_inputs that keeps what it learns about the crop: (s, a, place).  s and a are host_inputs' own, on every route;
        place is a pipeline.Placement - `src8` the (H, W, 3) uint8 portrait on the device as the model's input was cut from it
        (image.source_rgb8_device: opt.rgba_conversion and opt.bkg_color_hex honoured; with FLOAT_AMD_IMAGE_FRONT=0 the alpha is
        discarded, as on that route), `rect` = (x0, y0, w, h) the crop window in its coordinates: the one process_img(...,
        front=...) gives on the device-front route, the bbox process_img returns on the host routes (H <= 360 with face_align,
        beyond the size limits, FLOAT_AMD_IMAGE_FRONT=0), (0, 0, W, H) with no_crop.  It may reach outside the image.  What
        infer_pasted, stream_pasted and their JPEG forms paste the generated frames back with."""
        return self._host_inputs(ref_img, ref_audio, no_crop, True)

    def _source_rgb8(self, img, front_on):
        """The portrait of a Placement: the definition's 8-bit RGB of the IMAGE item, on the device."""
        o = self.opt
        if front_on:
            return source_rgb8_device(img, getattr(o, "rgba_conversion", "blend_with_color"), getattr(o, "bkg_color_hex", "#000000"), self.rank)
        return host_models.image_to_rgb8(img, "discard_alpha").to(self.rank, non_blocking=True).contiguous()

    def _face_detector(self):
        """The `detector=` of host_models.process_img for this call: the device detector where FLOAT_AMD_FACE_DETECTOR allows it
        and its weight file is found (face.find_sfd_weights; never downloaded), else None.  device: a missing file is an error.
        The handle is built when the callable is first used - in auto mode an installed `face_alignment` package goes first and
        nothing is built - and is freed with the other operators in offload()."""
        path = self._sfd_path()
        return None if path is None else (lambda view: self._detect_faces(path, view))

    def _sfd_path(self):
        """The weight file of _face_detector's callable, or None where there is no such callable."""
        mode = host_models.face_detector_mode()
        if mode in ("package", "off"):
            return None
        path = find_sfd_weights()
        if path is None:
            if mode == "device":
                raise FileNotFoundError("FLOAT_AMD_FACE_DETECTOR=device, but no s3fd weight file was found.  " + host_models.SFD_WEIGHTS_HINT)
            return None
        return path

    def _face_handle(self, path):
        """The detector built from `path`, on first use or when the file or FLOAT_AMD_SFD_DTYPE changed."""
        from ... import native as _native
        key = (path, _native.canon_dtype(os.environ.get("FLOAT_AMD_SFD_DTYPE", "fp16")))
        if self.face is None or self._face_key != key:
            if self.face is not None:
                self.face.close()
            self.face = FaceDetectorHIP(load_sfd_state(path), self.rank, dtype=key[1])
            self._face_key = key
        return self.face

    def _view_fits(self, face, view):
        h, w = int(view.shape[0]), int(view.shape[1])
        if min(h, w) < host_models.SFD_MIN_SIDE or h > face.max_hw[0] or w > face.max_hw[1]:
            main_logger.warning("face_align=True: a %d x %d detector view is outside the device detector's sizes (%d ... %d x %d): "
                                "no face detection", h, w, host_models.SFD_MIN_SIDE, face.max_hw[0], face.max_hw[1])
            return False
        return True

    def _detect_faces(self, path, view):
        """S3FD on the (h, w, 3) uint8 view - on the device already (image.detector_view_device) or host-made (the H <= 360
        route: uploaded) - with the handle built on first use.  Only the box rows and the two counts come back.
        FLOAT_AMD_SFD_DTYPE = fp16 (default) | bf16 | fp32: fp32 is the remedy where check_range reports the detector."""
        face = self._face_handle(path)
        return face.detect(view) if self._view_fits(face, view) else []

    # ------------------------------------------------------------------ a batch of portraits: one detector pass
    def _align_source(self, img, size, rgba, bkg):
        """How _host_inputs treats an image with face_align: (True, the image on the device) on the device-front route, (False,
        the (H, W, 3) float host image process_img gets) on the host routes (H <= 360, beyond the front end's size limits,
        FLOAT_AMD_IMAGE_FRONT=0)."""
        front_on = os.environ.get("FLOAT_AMD_IMAGE_FRONT", "1") != "0"
        H, Wd, ch = int(img.shape[0]), int(img.shape[1]), int(img.shape[2])
        if front_on and H > 360 and front_takes(H, Wd, size, crop=True):
            return True, image_to_device(img, self.rank)
        if front_on and ch == 4:
            img = host_models.image_to_rgb8(img, rgba, host_models.hex_to_rgb8(bkg)).float() / 255.0
        return False, img[..., :3].float()

    def _found_faces(self, sources, rgba, bkg):
        """For each (on_device, image) of _align_source: (view, rows) - the detector's view of the image and the rows of the
        device detector on it - or None where the device detector is not the one process_img would use (FLOAT_AMD_FACE_DETECTOR
        = off | package, auto with the `face_alignment` package at hand or without a weight file): those images take the
        per-image route.  The views are made one by one (the front end on the device, process_img_view on the host routes),
        stacked, and go through ONE FaceDetectorHIP.detect_batch per view size: one S3FD pass and one synchronisation for the
        batch instead of one each per portrait."""
        path = self._sfd_path()
        if path is not None and host_models.face_detector_mode() == "auto":
            try:
                host_models._face_detector()  # the package goes first in auto mode, per image as before
                path = None
            except Exception:  # noqa: BLE001
                pass
        if path is None:
            return [None] * len(sources)
        face = self._face_handle(path)
        views = [host_models.process_img_view(x, (lambda vh, x=x: detector_view_device(x, vh, rgba, bkg)) if on_dev else None)
                 for on_dev, x in sources]
        rows = [[] for _ in views]
        groups = {}
        for i, v in enumerate(views):
            if self._view_fits(face, v):
                groups.setdefault(tuple(v.shape), []).append(i)
        for idx in groups.values():
            stacked = torch.stack([views[i].to(self.rank, non_blocking=True) for i in idx])
            for i, r in zip(idx, face.detect_batch(stacked)):
                rows[i] = r
        return list(zip(views, rows))

    @torch.no_grad()
    def face_align_batch(self, images, size=None, margin=None, index=1, rgba_conversion=None, bkg_color_hex=None):
        """The face-aligned crops of a batch of portraits (the Ad tier's Face Align node): images (B, H, W, 3|4) float in
        [0, 1] -> (crops8 (B, size, size, 3) uint8 on the device, rects = B tuples (x, y, w, h) as process_img returns them).
        Item i is what the single-image route gives: process_img(..., index=index, front=..., detector=...) and the image
        front end in its 8-bit output mode (on the host routes: process_img's crop, rounded to 8 bits).  The B detector views
        go through one detect_batch (_found_faces); the crop rule is process_img's own, on the rows that came back.  Defaults
        come from opt."""
        o = self.opt
        size = int(size if size is not None else o.input_size)
        margin = float(margin if margin is not None else getattr(o, "face_margin", 1.6))
        rgba = rgba_conversion if rgba_conversion is not None else getattr(o, "rgba_conversion", "blend_with_color")
        bkg = bkg_color_hex if bkg_color_hex is not None else getattr(o, "bkg_color_hex", "#000000")
        if images.dim() != 4 or images.shape[-1] not in (3, 4):
            raise ValueError("face_align_batch: images must be (B, H, W, 3|4), got %s" % (tuple(images.shape),))
        self.to_target()
        sources = [self._align_source(images[i], size, rgba, bkg) for i in range(images.shape[0])]
        found = self._found_faces(sources, rgba, bkg)
        crops, rects = [], []
        for (on_dev, x), f in zip(sources, found):
            front = None
            if on_dev:
                front = (lambda vh, v=f[0]: v) if f is not None else (lambda vh, x=x: detector_view_device(x, vh, rgba, bkg))
            detector = (lambda view, r=f[1]: r) if f is not None else self._face_detector()
            crop, rect = host_models.process_img(x, size, margin, index=index, logger=main_logger, front=front, detector=detector)
            if on_dev:
                crop8 = image_front_device(x, size, size, rect, None, rgba, bkg, True)
            else:
                crop8 = (crop.clamp(0, 1) * 255).round().to(torch.uint8).to(self.rank, non_blocking=True)
            crops.append(crop8)
            rects.append(tuple(int(v) for v in rect))
        return torch.stack(crops), rects

    def host_inputs_batch(self, ref_images, audios, no_crop=True):
        """host_inputs for a batch: ref_images (B, H, W, C) or a list of B images, audios a list of B AUDIO items -> a list of
        (s, a); item i is bitwise host_inputs(ref_images[i:i+1], audios[i], no_crop).  With face_align the B detector views
        go through one detect_batch (_found_faces) instead of B detector passes and B synchronisations."""
        o = self.opt
        imgs = [x[0] if x.dim() == 4 else x for x in (ref_images if isinstance(ref_images, (list, tuple)) else
                                                       [ref_images[i] for i in range(ref_images.shape[0])])]
        if len(imgs) != len(audios):
            raise ValueError("host_inputs_batch: %d images, %d audio items" % (len(imgs), len(audios)))
        found = [None] * len(imgs)
        if not no_crop:
            rgba, bkg = getattr(o, "rgba_conversion", "blend_with_color"), getattr(o, "bkg_color_hex", "#000000")
            sources = [self._align_source(x, o.input_size, rgba, bkg) for x in imgs]
            found = self._found_faces(sources, rgba, bkg)
            imgs = [src if on_dev else x for x, (on_dev, src) in zip(imgs, sources)]  # on the device already: not uploaded twice
        return [self._host_inputs(x, a, no_crop, False, f)[:2] for x, a, f in zip(imgs, audios, found)]

    def _host_inputs(self, ref_img, ref_audio, no_crop, placed, found=None):
        """The one body of host_inputs and host_inputs_placed: (s, a, place), place None unless `placed`.  found: (view, rows)
        of _found_faces for this image - the detector's view and what the device detector found on it - where a batch has them
        already."""
        o = self.opt
        detector = (lambda view: found[1]) if found is not None else None
        img = ref_img[0] if ref_img.dim() == 4 else ref_img
        # The image front end on the device (float_img_front): the raw IMAGE tensor crosses PCIe once, and RGBA conversion
        # (opt.rgba_conversion, opt.bkg_color_hex), the zero-bordered crop, the exact area resize, the 8-bit rounding and the
        # normalisation are HIP kernels; with face_align only the detector's 360-px copy comes back to the host.  Taken when
        # there is something to convert, crop or resize; a 3-channel image at the model's size without a crop takes the
        # lines below, as do images of 360 px height or less with face_align (the reference's INTER_CUBIC route) and images
        # outside the kernels' size limits (a side above 16384; with face_align a detector copy wider than 4096 columns).
        # FLOAT_AMD_IMAGE_FRONT=0 (read here, per call): the host route for everything, alpha discarded.
        front_on = os.environ.get("FLOAT_AMD_IMAGE_FRONT", "1") != "0"
        H, Wd, ch = int(img.shape[0]), int(img.shape[1]), int(img.shape[2])
        cubic = not no_crop and H <= 360
        rgba, bkg = getattr(o, "rgba_conversion", "blend_with_color"), getattr(o, "bkg_color_hex", "#000000")
        if (front_on and not cubic and (ch == 4 or H != o.input_size or Wd != o.input_size or not no_crop)
                and front_takes(H, Wd, o.input_size, crop=not no_crop)):
            dimg = image_to_device(img, self.rank)
            rect = None
            if not no_crop:  # generate.py:77-78
                rect, _ = host_models.process_img(dimg, o.input_size, getattr(o, "face_margin", 1.6), logger=main_logger,
                                                  front=(lambda view_h: found[0]) if found is not None else
                                                  (lambda view_h: detector_view_device(dimg, view_h, rgba, bkg)),
                                                  detector=detector or self._face_detector())
            if ch == 3 and (H, Wd) == (o.input_size, o.input_size) and rect is not None and tuple(rect) == (0, 0, Wd, H):
                # the crop turned out to be the whole image (a square portrait without a detected face): nothing to convert,
                # crop or resize after all, so this is the case of the lines below, bitwise
                s = host_models.preprocess_image(dimg, o.input_size)
            else:
                s = preprocess_image_device(dimg, o.input_size, rect, rgba, bkg)
            place = Placement(self._source_rgb8(dimg, True), tuple(int(v) for v in rect) if rect is not None else (0, 0, Wd, H)) if placed else None
            return s, self._host_audio(ref_audio), place
        src = img
        if front_on and ch == 4:  # the cubic route, an image beyond the size limits: the widgets are honoured there too
            img = host_models.image_to_rgb8(img, rgba, host_models.hex_to_rgb8(bkg)).float() / 255.0
        bbox = (0, 0, Wd, H)
        if not no_crop:  # generate.py:77-78
            img, bbox = host_models.process_img(img[..., :3].float(), o.input_size, getattr(o, "face_margin", 1.6), logger=main_logger,
                                                detector=detector or self._face_detector())
        # The raw tensors cross PCIe first (3 MB + 0.6 MB for a 10-s clip) and the elementwise / reduction plumbing runs on the
        # device: on the host the same ops cost 1-29 ms per clip (torch's 128-thread intra-op pool on sub-megabyte tensors),
        # as much as a quarter of the whole clip.  The reference moves its slices to the device first too (nodes.py:193-201).
        s = host_models.preprocess_image(img[..., :3].to(self.rank, non_blocking=True), o.input_size)
        place = Placement(self._source_rgb8(src, front_on), tuple(int(v) for v in bbox)) if placed else None
        return s, self._host_audio(ref_audio), place

    def _host_audio(self, ref_audio):
        o = self.opt
        # Audio at another rate than the model's (a ComfyUI AUDIO item: 44.1 / 48 kHz stereo) takes the same route: the raw planar
        # samples cross PCIe and the mono mix, the band-limited resampler and the normalisation are HIP kernels
        # (float_aud_front) instead of a polyphase conv1d on the host.  At the model's rate nothing changes.
        # FLOAT_AMD_AUDIO_FRONT=0 (read here, per call): the host resampler.
        wav, rate = ref_audio["waveform"][0], ref_audio["sample_rate"]
        if int(rate) != o.sampling_rate and os.environ.get("FLOAT_AMD_AUDIO_FRONT", "1") != "0":
            a = preprocess_audio_device(wav, int(rate), o.sampling_rate, device=self.rank)
        else:
            a = host_models.preprocess_audio(wav, rate, o.sampling_rate, device=self.rank)
        return a

    @torch.no_grad()
    def conditions(self, ref_img, ref_audio, emo=None, no_crop=True):
        s, a = self.host_inputs(ref_img, ref_audio, no_crop)
        return self.conditions_device(s, a, emo)

    @torch.no_grad()
    def _clip_inputs(self, s, a, emo, seed):
        """(conditions, noise) of one clip: operators resident, encoder kernels enqueued (nothing waits for them on the host)
        and the clip's noise on its way to the device."""
        self.to_target()  # no-op while resident
        c = self.conditions_device(s, a, emo)
        return c, self._noise_to_device(self.G.n_chunks(c["T"]), seed if seed is not None else self.opt.seed)

    @torch.no_grad()
    def infer_device(self, s, a, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", seed=25, out=None,
                     out_dtype=None, out_format=None, matrix=None):
        """Portrait and waveform in HBM -> (T,H,W,3) fp32 frames in [0,1] in pinned host memory: every operator of the path and
        the hand-over (frames of decode batch i leave inside the launches of batch i+1, float_dec_frames_host).  bench.py
        times exactly this call.  Like the reference, the grid size comes from opt.nfe (FLOAT.py:188).
        out_dtype=torch.uint8: 8-bit frames, quantised by the decoder's last kernel (round(255 * frame), bitwise what rounding the
        fp32 frames gives) - a quarter of the staging, pinned and PCIe bytes; default (None) fp32.  A caller-supplied `out`
        fixes the dtype; contradicting it is a ValueError.
        out_format="i420": (T, 3H/2, W) uint8 planar YUV 4:2:0 (BT.601 limited range, host_models.rgb8_to_i420 of the 8-bit
        frames, converted by the decoder's last kernel) - what a video encoder reads, half the bytes of uint8 RGB
        (host_models.write_y4m pipes it).  It implies uint8; with out_dtype=torch.float32 or an fp32 `out` it is a ValueError.
        matrix: the colour matrix of I420 frames, as host_models.yuv_matrix_id reads it - None = BT.601 limited range, "bt709",
        "bt601-full", "bt709-full", their ids 2 / 4 / 6, or "auto" (by the crop's size: BT.709 from 1280 x 720 up).  The bytes
        are host_models.rgb8_to_i420(the 8-bit frames, matrix).  With fp32 or uint8 RGB frames anything but None is a ValueError."""
        matrix = self._crop_matrix("infer_device", out, out_dtype, out_format, matrix)  # a contradiction is refused before anything runs
        c, noise = self._clip_inputs(s, a, emo, seed)
        ov = os.environ.get("FLOAT_AMD_OVERLAP", "")  # "prio" | "cu:N": decode window k beside the chain of window k + 1 (pipeline.py)
        verify = precision_policy(self._precision_checked) == "check"  # FLOAT_AMD_VERIFY, default off: nothing below changes
        if ov and ov != "0":
            host = self.G.generate_to_host_overlap(c["r_s"], c["wa"], c["we"], c["s_r"], self.opt.nfe, a_cfg_scale, r_cfg_scale,
                                                   e_cfg_scale, noise=noise, out=out, mode=ov, return_rd=verify,
                                                   out_dtype=out_dtype, out_format=out_format, matrix=matrix)
        else:
            host = self.G.generate_to_host(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale,
                                           e_cfg_scale, noise=noise, out=out, return_rd=verify, out_dtype=out_dtype,
                                           out_format=out_format, matrix=matrix)
        host, r_d = host if verify else (host, None)
        torch.cuda.current_stream(self.rank).synchronize()  # the frames are in host memory
        self.G.release_host_inflight()
        bad = self.check_range("InferenceAgent.infer_device", allow_rebuild=True)
        if bad == "rebuilt":
            return self.infer_device(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, out, out_dtype, out_format, matrix)  # once more, in the wider types
        if verify and not bad:  # a range failure has been reported already: the frames are wrong for a reason that is known
            # 8-bit output (RGB or I420): the staging buffer holds quantised frames, so the first k frames are decoded once more in the fp32
            # form by the same handle (a frame does not depend on its batch: bitwise what the fp32 staging buffer would hold)
            frames_dev = None
            if host.dtype == torch.uint8:
                k = min(verify_frames_default(), c["T"], self.cfg.num_frames_for_clip)
                frames_dev = self.G.dec.decode_latent_into_processed_images(c["s_r"], r_d[0, :k])
            if self.check_precision("InferenceAgent.infer_device", s, c, noise, r_d, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                    allow_rebuild=True, frames_dev=frames_dev) == "rebuilt":
                return self.infer_device(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, out, out_dtype, out_format, matrix)  # once more, in fp32
        return host

    def stream_device(self, s, a, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", seed=25, out_dtype=None,
                      out_format=None, slots=3, matrix=None):
        """The streaming sibling of infer_device: a generator of FrameBlock(first, last, frames), one per 50-frame FMT window, in
        frame order - concatenated, bit for bit the frames infer_device returns for the same inputs and seed, in both
        FLOAT_AMD_NOISE modes and all three formats (out_dtype / out_format / matrix as there).  `frames` is a view of one of `slots`
        pinned buffers (FloatHotPath.stream_to_host has the contract): complete when yielded, OVERWRITTEN once the generator has
        been advanced again - copy what is to be kept.  Pinned memory is slots x 50 frames whatever the clip's length, and the
        first block arrives after one window instead of after the clip.  slots < 2 or contradicting formats raise ValueError here,
        at the call; nothing runs before the first next().  While the stream is open every other call that produces frames on
        this agent raises RuntimeError; close() (or dropping) the generator early leaves the agent usable.
        After the last block FLOAT_AMD_RANGE is applied once: warn, raise (Fp16RangeError from the next() that ends the stream)
        and off as in infer_device; auto cannot run frames again that were consumed already and acts as warn.  A stream left
        early (close(), dropped, an exception in the consumer) is not reported, and its range counters are read and reset so
        that they are not held against the next clip.  FLOAT_AMD_VERIFY is NOT applied in a stream, and FLOAT_AMD_OVERLAP is ignored (the stream is
        windowed already, on one queue)."""
        matrix = self._check_stream_call("stream_device", slots, out_dtype, out_format, matrix)

        def _stream_device(c, noise):
            return self.G.stream_to_host(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                         noise=noise, out_dtype=out_dtype, out_format=out_format, slots=int(slots), matrix=matrix)
        return self._stream_clip("InferenceAgent.stream_device", s, a, emo, seed, _stream_device)

    def _crop_matrix(self, what, out, out_dtype, out_format, matrix):
        """resolve_out_format's refusals, and the id of `matrix` for frames of the crop's size (None stays None: BT.601 limited range)"""
        _, fmt = resolve_out_format(out, out_dtype, out_format, matrix)
        size = self.opt.input_size
        return None if matrix is None else host_models.yuv_matrix_for(what, matrix, fmt, size, size)

    def _check_stream_call(self, what, slots, out_dtype=None, out_format=None, matrix=None):
        """What a stream refuses at the call, before its generator exists (a generator's body runs at the first next()).  Returns
        the id of `matrix` (None for None)."""
        if int(slots) < 2:
            raise ValueError("%s needs slots >= 2 (one block with the consumer, one in flight), got %r" % (what, slots))
        matrix = self._crop_matrix(what, None, out_dtype, out_format, matrix)
        if self.G is not None:
            self.G.require_no_stream(what)
        return matrix

    def _stream_clip(self, where, s, a, emo, seed, start):
        """The generator behind every stream of the agent: the clip's inputs, the blocks of start(conditions, noise) - a
        FloatHotPath stream - and FLOAT_AMD_RANGE once after the last of them."""
        c, noise = self._clip_inputs(s, a, emo, seed)
        done = False
        try:
            yield from start(c, noise)
            done = True
        finally:
            # left early: the inner generator has waited for its work; what the abandoned windows counted is not the next clip's
            if not done and self.G is not None and not self.G._open_stream and os.environ.get("FLOAT_AMD_RANGE", "warn").lower() != "off":
                self.range_counts(reset=True)
        if os.environ.get("FLOAT_AMD_RANGE", "warn").lower() == "auto":
            where += " (FLOAT_AMD_RANGE=auto acts as warn in a stream: the frames have been consumed and are not run again)"
        self.check_range(where)

    def stream_inference(self, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False,
                         seed=25, out_dtype=None, out_format=None, slots=3, matrix=None):
        """The streaming sibling of run_inference: host inputs as there, blocks as stream_device yields them.  There is no
        `nfe` argument: the grid size comes from opt.nfe (run_inference keeps the reference's argument and ignores it)."""
        matrix = self._check_stream_call("stream_inference", slots, out_dtype, out_format, matrix)
        return self._stream_inference(ref_img, ref_audio, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, no_crop, seed, out_dtype,
                                      out_format, int(slots), matrix)

    def _stream_inference(self, ref_img, ref_audio, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, no_crop, seed, out_dtype,
                          out_format, slots, matrix=None):
        with torch.no_grad():
            s, a = self.host_inputs(ref_img, ref_audio, no_crop)
        yield from self.stream_device(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, out_dtype, out_format, slots, matrix)

    @torch.no_grad()
    def infer_device_jpeg(self, s, a, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", seed=25, quality=90, restart=None):
        """infer_device with the frames leaving as baseline JPEG files: a jpeg.JpegFrames in pinned host memory, file i bitwise
        host_models.jpeg_encode_rgb8(infer_device(out_dtype=torch.uint8)[i], quality, restart) (FloatHotPath.generate_to_jpeg: the
        encoder runs on the 8-bit frames in HBM and only the files cross PCIe).  FLOAT_AMD_RANGE applies as in infer_device (auto
        rebuilds and runs the clip again); FLOAT_AMD_VERIFY is NOT applied and FLOAT_AMD_OVERLAP is ignored."""
        c, noise = self._clip_inputs(s, a, emo, seed)
        frames = self.G.generate_to_jpeg(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                         noise=noise, quality=quality, restart=restart)
        if self.check_range("InferenceAgent.infer_device_jpeg", allow_rebuild=True) == "rebuilt":
            return self.infer_device_jpeg(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, quality, restart)  # once more, in the wider types
        return frames

    def stream_device_jpeg(self, s, a, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", seed=25, quality=90, restart=None,
                           slots=3):
        """The streaming sibling of infer_device_jpeg: a generator of JpegBlock(first, last, frames), one per 50-frame FMT window, in
        frame order - concatenated, the files infer_device_jpeg returns for the same inputs and seed.  `frames` lives in one of
        `slots` pinned ring buffers (FloatHotPath.stream_to_jpeg has the contract): complete when yielded, OVERWRITTEN once the
        generator has been advanced again.  slots < 2 or a quality outside 1 ... 100 raise ValueError here, at the call; nothing
        runs before the first next().  While the stream is open every other call that produces frames on this agent raises
        RuntimeError; close() (or dropping) the generator early leaves the agent usable.  After the last block FLOAT_AMD_RANGE is
        applied once, as in stream_device: warn, raise and off, and auto acts as warn.  FLOAT_AMD_VERIFY is NOT applied."""
        self._check_stream_call("stream_device_jpeg", slots)
        if not 1 <= int(quality) <= 100:
            raise ValueError("stream_device_jpeg: quality (%r) must be 1 ... 100" % (quality,))

        def _stream_device_jpeg(c, noise):
            return self.G.stream_to_jpeg(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                         noise=noise, quality=int(quality), restart=restart, slots=int(slots))
        return self._stream_clip("InferenceAgent.stream_device_jpeg", s, a, emo, seed, _stream_device_jpeg)

    def write_video(self, path, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False, seed=25,
                    quality=90, fps=None, paste_back=False, feather=None, pad=None, resample=None):
        """A playable file: host_inputs, stream_device_jpeg, and host_models.AviMjpegWriter on `path` (a path or a seekable binary
        file object) - Motion JPEG in an AVI container with the clip's audio as a 16-bit PCM track: the AUDIO item's own samples
        at its own rate, channels mixed to mono (not the normalised 16 kHz waveform the model hears), one `01wb` chunk behind the
        frames of every window.  fps defaults to opt.fps.  Returns the number of frames written.
        paste_back=True: the frames are the user's portrait with the generated face pasted back (stream_pasted_jpeg, `feather` as
        in infer_pasted) and the file is written at the portrait's size, whose sides must be multiples of 16 (ValueError
        otherwise, before the file is opened) unless pad="edge" (as in infer_pasted_jpeg) opts in to any size: a 1920 x 1080
        portrait then gives a 1920 x 1080 file.  pad has no say without paste_back: the crops are model-size frames.
        resample: as in infer_pasted; with paste_back=False anything but None is a ValueError, before the file is opened."""
        o = self.opt
        fps = o.fps if fps is None else fps
        self._paste_call("write_video", ref_img, resample=resample, paste_back=paste_back)
        if paste_back:
            img = ref_img[0] if ref_img.dim() == 4 else ref_img
            height, width = int(img.shape[0]), int(img.shape[1])
            blocks = self.stream_pasted_jpeg(ref_img, ref_audio, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, no_crop, seed, feather, quality,
                                             pad=pad, resample=resample)
        else:
            height = width = o.input_size
            with torch.no_grad():
                s, a = self.host_inputs(ref_img, ref_audio, no_crop)
            blocks = self.stream_device_jpeg(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, quality)
        audio = ref_audio["waveform"][0].detach().float().cpu()
        audio = (audio.mean(dim=0) if audio.dim() == 2 else audio).reshape(-1)
        rate = int(ref_audio["sample_rate"])
        with host_models.AviMjpegWriter(path, width, height, fps, audio_rate=rate) as w:
            sent = 0
            for blk in blocks:
                w.write(blk.frames)
                upto = min(audio.numel(), int(round(blk.last * rate / float(fps))))
                w.write_audio(audio[sent:upto])
                sent = max(sent, upto)
            w.write_audio(audio[sent:])
            return w.frames

    # ------------------------------------------------------------------ paste back: the frames in the user's portrait
    def _paste_call(self, what, ref_img, jpeg_out=False, out_format=None, pad=None, matrix=None, resample=None, paste_back=True):
        """What a pasted producer refuses at the call: with JPEG output, a portrait whose sides float_jpg_encode does not take
        (pad="edge": none) or a pad that is neither None nor "edge"; with
        out_format="i420", a portrait with an odd side; an out_format that is none of None, "rgb", "i420"; a `matrix` with RGB
        frames or one host_models.yuv_matrix_id does not know; a `resample` that is no filter of host_models.RESAMPLE_FILTERS, or any
        without paste_back (only a pasted crop is resized).  Returns the id of `matrix` ("auto": by the portrait's size), None for None."""
        if resample is not None:
            host_models.resample_filter_id(what, resample)
            if not paste_back:
                raise ValueError("%s: resample=%r needs paste_back=True (the crops leave at the model's size, nothing is resized)" % (what, resample))
        if not paste_back:
            return None
        img = ref_img[0] if ref_img.dim() == 4 else ref_img
        if jpeg_out:
            require_jpeg_sides(what, int(img.shape[0]), int(img.shape[1]), pad)
        fmt = paste_format(what, out_format)
        if fmt == "i420":
            require_even_sides(what, int(img.shape[0]), int(img.shape[1]))
        return None if matrix is None else host_models.yuv_matrix_for(what, matrix, fmt, int(img.shape[1]), int(img.shape[0]))

    @torch.no_grad()
    def infer_pasted(self, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False, seed=25,
                     feather=None, out=None, out_format=None, matrix=None, resample=None):
        """run_inference whose frames are the user's portrait with the generated face pasted back: (T, H, W, 3) uint8 in pinned host
        memory at the portrait's own size, bitwise host_models.paste_rgb8(place.src8, infer_device(s, a, out_dtype=torch.uint8),
        place.rect, feather) with (s, a, place) = host_inputs_placed(ref_img, ref_audio, no_crop).  The 8-bit crops never leave
        the device (FloatHotPath.generate_pasted: decode_u8, float_img_paste, one copy per 50 frames).  feather: the width in
        source pixels over which the box fades into the portrait where its edge lies inside the image; None = rect_w // 16, a
        visual choice, not a measurement.  With no_crop the box is the whole image: the frames resized to the portrait's size.
        FLOAT_AMD_RANGE applies as in infer_device (auto rebuilds and runs the clip again); FLOAT_AMD_VERIFY is NOT applied and
        FLOAT_AMD_OVERLAP is ignored.
        out_format="i420" (default None = "rgb": the above): (T, 3H/2, W) uint8 planar YUV 4:2:0 in pinned host memory (BT.601
        limited range), bitwise host_models.rgb8_to_i420 of the RGB result = host_models.paste_i420(...): paste and conversion are
        one kernel and half the bytes cross PCIe.  Any even size is taken (1920 x 1080); a portrait with an odd side is a
        ValueError at this call, before anything runs - nothing is padded or cropped.  FLOAT_AMD_RANGE applies as above.
        matrix: the colour matrix of I420 frames, as in infer_device; "auto" goes by the portrait's size (BT.709 limited range
        when W >= 1280 or H > 576 - what players assume for untagged video of that size).  A ValueError with RGB frames.
        resample (default None: the above, byte for byte): "bicubic" | "lanczos" - the crop is brought to the box's size by Pillow's
        Image.resize rule with that filter (float_img_resample, two more launches per 50 frames) instead of the front end's rule,
        which enlarges linearly: bitwise host_models.paste_rgb8 / paste_i420(..., resample=resample).  For a box larger than the
        model's frame - a face in an HD portrait, no_crop - the pasted face is as sharp as an image tool would make it.  Another
        name is a ValueError at this call."""
        matrix = self._paste_call("infer_pasted", ref_img, out_format=out_format, matrix=matrix, resample=resample)
        s, a, place = self.host_inputs_placed(ref_img, ref_audio, no_crop)
        while True:
            c, noise = self._clip_inputs(s, a, emo, seed)
            host = self.G.generate_pasted(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                          noise=noise, place=place, feather=feather, out=out, out_format=out_format,
                                          matrix=matrix, resample=resample)
            torch.cuda.current_stream(self.rank).synchronize()  # the frames are in host memory
            if self.check_range("InferenceAgent.infer_pasted", allow_rebuild=True) != "rebuilt":
                return host  # otherwise once more, in the wider types

    def stream_pasted(self, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False, seed=25,
                      feather=None, slots=3, out_format=None, matrix=None, resample=None):
        """The streaming sibling of infer_pasted: a generator of FrameBlock(first, last, frames), one per 50-frame FMT window, in
        frame order - concatenated, the frames infer_pasted returns for the same inputs and seed.  The ring rules are
        stream_device's: `frames` is a (last - first, H, W, 3) uint8 view of one of `slots` pinned buffers, complete when yielded,
        OVERWRITTEN once the generator has been advanced again; slots < 2 raises ValueError at the call; while the stream is open
        every other producer on this agent raises RuntimeError.  FLOAT_AMD_RANGE is applied once after the last block (auto acts
        as warn); FLOAT_AMD_VERIFY is NOT applied and FLOAT_AMD_OVERLAP is ignored.
        out_format="i420": `frames` is a (last - first, 3H/2, W) uint8 view, the frames of infer_pasted(out_format="i420"); the
        pinned slots are half the size.  A portrait with an odd side raises ValueError here, at the call.  matrix, resample: as in
        infer_pasted."""
        self._check_stream_call("stream_pasted", slots)
        matrix = self._paste_call("stream_pasted", ref_img, out_format=out_format, matrix=matrix, resample=resample)

        def _stream_pasted(c, noise, place):
            return self.G.stream_to_host_pasted(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale,
                                                e_cfg_scale, noise=noise, place=place, feather=feather, slots=int(slots),
                                                out_format=out_format, matrix=matrix, resample=resample)
        return self._stream_placed("InferenceAgent.stream_pasted", ref_img, ref_audio, no_crop, emo, seed, _stream_pasted)

    def write_y4m(self, path_or_file, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False,
                  seed=25, fps=None, paste_back=False, feather=None, slots=3):
        """A clip for an encoder: host_inputs, a stream of I420 blocks, and host_models.Y4MWriter on `path_or_file` - a path, or an
        object with write(), which may be a non-seekable pipe to ffmpeg's or x264's stdin (the header goes out first and nothing
        is patched afterwards).  The frames are yuv420p, BT.601 limited range (write_y4m_matrix is this call with a colour matrix
        to choose): the consumer converts no colours.  Y4M carries
        NO AUDIO: the clip's sound has to be given to the encoder separately (write_video writes a file with an audio track).
        fps defaults to opt.fps.  Returns the number of frames written.
        paste_back=False: stream_device(out_format="i420") at the model's size.
        paste_back=True: stream_pasted(out_format="i420", feather=feather) - the user's portrait with the generated face pasted
        back, at the portrait's size, which must have even sides (ValueError otherwise, before anything runs or a file is opened).
        Pinned memory is `slots` x 50 frames of 1.5 bytes per pixel whatever the clip's length."""
        return self.write_y4m_matrix(path_or_file, ref_img, ref_audio, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, no_crop, seed, fps,
                                     paste_back, feather, slots)

    def write_y4m_matrix(self, path_or_file, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E",
                         no_crop=False, seed=25, fps=None, paste_back=False, feather=None, slots=3, matrix=None, resample=None):
        """write_y4m with the colour matrix of the frames to choose.  matrix: as in infer_device / infer_pasted - None = BT.601
        limited range (then this is write_y4m, byte for byte), "bt709", "bt601-full", "bt709-full", their ids, or "auto": by the
        size of the frames that leave, the model's with paste_back=False and the portrait's with paste_back=True (BT.709 limited
        range when W >= 1280 or H > 576, what players assume for untagged video).  It is resolved once, before anything runs or a
        file is opened, and the one id goes to the producer and to the writer, so the tag cannot disagree with the samples: full
        range is written as XCOLORRANGE=FULL.  Y4M has no tag for the matrix itself: host_models.yuv_ffmpeg_args(matrix) are the
        arguments that state it to ffmpeg.  (A method of its own because write_y4m's parameter list is held as it is.)
        resample: as in infer_pasted (write_y4m's held parameter list has no room for it: this is the Y4M call that takes it); with
        paste_back=False anything but None is a ValueError, before anything runs or a file is opened."""
        o = self.opt
        fps = o.fps if fps is None else fps
        self._paste_call("write_y4m", ref_img, resample=resample, paste_back=paste_back)
        if paste_back:
            img = ref_img[0] if ref_img.dim() == 4 else ref_img
            height, width = int(img.shape[0]), int(img.shape[1])
            matrix = self._paste_call("write_y4m", ref_img, out_format="i420", matrix=matrix, resample=resample)
            blocks = self.stream_pasted(ref_img, ref_audio, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, no_crop, seed, feather, slots,
                                        out_format="i420", matrix=matrix, resample=resample)
        else:
            height = width = o.input_size
            matrix = self._check_stream_call("write_y4m", slots, out_format="i420", matrix=matrix)
            with torch.no_grad():
                s, a = self.host_inputs(ref_img, ref_audio, no_crop)
            blocks = self.stream_device(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, out_format="i420", slots=slots,
                                        matrix=matrix)
        try:
            with host_models.Y4MWriter(path_or_file, width, height, fps, matrix) as w:
                for blk in blocks:
                    w.write(blk.frames)
                return w.frames
        finally:
            blocks.close()  # a writer that failed leaves no stream open on the agent

    def _stream_placed(self, where, ref_img, ref_audio, no_crop, emo, seed, start):
        with torch.no_grad():
            s, a, place = self.host_inputs_placed(ref_img, ref_audio, no_crop)
        yield from self._stream_clip(where, s, a, emo, seed, lambda c, noise: start(c, noise, place))

    @torch.no_grad()
    def infer_pasted_jpeg(self, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False, seed=25,
                          feather=None, quality=90, restart=None, pad=None, resample=None):
        """infer_pasted with the frames leaving as baseline JPEG files: a jpeg.JpegFrames in pinned host memory, file i bitwise
        host_models.jpeg_encode_rgb8(infer_pasted(...)[i], quality, restart).  Paste and encoder run on the device and only the
        files cross PCIe.  float_jpg_encode takes sides that are multiples of 16: a portrait of another size is a ValueError at
        this call, before anything runs - nothing is padded.  pad="edge" (default None) opts in to any portrait size:
        float_jpg_encode_padded replicates the last row and column into the partial 16 x 16 MCUs, the files carry the true size, file
        i is bitwise jpeg_encode_rgb8(infer_pasted(...)[i], quality, restart, pad="edge"), and restart=None is ceil(W / 16) MCUs.
        FLOAT_AMD_RANGE applies as in infer_device_jpeg; FLOAT_AMD_VERIFY is NOT applied and FLOAT_AMD_OVERLAP is ignored.
        resample: as in infer_pasted - the files are those of infer_pasted(..., resample=resample)."""
        self._paste_call("infer_pasted_jpeg", ref_img, jpeg_out=True, pad=pad, resample=resample)
        s, a, place = self.host_inputs_placed(ref_img, ref_audio, no_crop)
        while True:
            c, noise = self._clip_inputs(s, a, emo, seed)
            frames = self.G.generate_to_jpeg(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                             noise=noise, quality=quality, restart=restart, place=place, feather=feather, pad=pad,
                                             resample=resample)
            if self.check_range("InferenceAgent.infer_pasted_jpeg", allow_rebuild=True) != "rebuilt":
                return frames  # otherwise once more, in the wider types

    def stream_pasted_jpeg(self, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False, seed=25,
                           feather=None, quality=90, restart=None, slots=3, pad=None, resample=None):
        """The streaming sibling of infer_pasted_jpeg: a generator of JpegBlock(first, last, frames) under the ring rules of
        stream_device_jpeg - concatenated, the files infer_pasted_jpeg returns.  slots < 2, a quality outside 1 ... 100 or a portrait
        whose sides are no multiples of 16 (without pad="edge", which is infer_pasted_jpeg's) raise ValueError here, at the call.
        FLOAT_AMD_RANGE is applied once after the last block (auto acts as warn); FLOAT_AMD_VERIFY is NOT applied and
        FLOAT_AMD_OVERLAP is ignored.  resample: as in infer_pasted, refused at the call too."""
        self._check_stream_call("stream_pasted_jpeg", slots)
        if not 1 <= int(quality) <= 100:
            raise ValueError("stream_pasted_jpeg: quality (%r) must be 1 ... 100" % (quality,))
        self._paste_call("stream_pasted_jpeg", ref_img, jpeg_out=True, pad=pad, resample=resample)

        def _stream_pasted_jpeg(c, noise, place):
            return self.G.stream_to_jpeg(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                         noise=noise, quality=int(quality), restart=restart, slots=int(slots), place=place, feather=feather,
                                         pad=pad, resample=resample)
        return self._stream_placed("InferenceAgent.stream_pasted_jpeg", ref_img, ref_audio, no_crop, emo, seed, _stream_pasted_jpeg)

    # ------------------------------------------------------------------ lossless frames: PNG files and APNG clips
    def _png_call(self, what, band, ref_img=None):
        """What a PNG producer refuses at the call: a band host_models.png_check_band does not take for the frames that leave -
        the model's size, or with ref_img the portrait's (any size up to 16384 is taken).  Returns the band in rows."""
        if ref_img is None:
            return host_models.png_check_band(self.opt.input_size, self.opt.input_size, band)
        img = ref_img[0] if ref_img.dim() == 4 else ref_img
        try:
            return host_models.png_check_band(int(img.shape[0]), int(img.shape[1]), band)
        except ValueError as e:
            raise ValueError("%s: %s" % (what, e)) from None

    @torch.no_grad()
    def infer_device_png(self, s, a, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", seed=25, band=None):
        """infer_device with the frames leaving as LOSSLESS PNG files: a png.PngFrames in pinned host memory; file i decodes to
        infer_device(out_dtype=torch.uint8)[i] bit for bit and is bitwise host_models.png_encode_rgb8 of it
        (FloatHotPath.generate_to_png: the encoder runs on the 8-bit frames in HBM and only the files cross PCIe).  band: rows
        per band, None = png.default_band.  FLOAT_AMD_RANGE applies as in infer_device (auto rebuilds and runs the clip again);
        FLOAT_AMD_VERIFY is NOT applied and FLOAT_AMD_OVERLAP is ignored."""
        band = self._png_call("infer_device_png", band)
        c, noise = self._clip_inputs(s, a, emo, seed)
        frames = self.G.generate_to_png(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                        noise=noise, band=band)
        if self.check_range("InferenceAgent.infer_device_png", allow_rebuild=True) == "rebuilt":
            return self.infer_device_png(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, band)  # once more, in the wider types
        return frames

    def stream_device_png(self, s, a, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", seed=25, band=None, slots=3):
        """The streaming sibling of infer_device_png: a generator of PngBlock(first, last, frames), one per 50-frame FMT window, in
        frame order - concatenated, the files infer_device_png returns for the same inputs and seed.  The ring rules are
        stream_device_jpeg's: `frames` lives in one of `slots` pinned buffers, complete when yielded, OVERWRITTEN once the generator
        has been advanced again; slots < 2 or a band outside its rule raise ValueError here, at the call; while the stream is open
        every other producer on this agent raises RuntimeError.  FLOAT_AMD_RANGE is applied once after the last block (auto acts
        as warn); FLOAT_AMD_VERIFY is NOT applied."""
        self._check_stream_call("stream_device_png", slots)
        band = self._png_call("stream_device_png", band)

        def _stream_device_png(c, noise):
            return self.G.stream_to_png(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                        noise=noise, band=band, slots=int(slots))
        return self._stream_clip("InferenceAgent.stream_device_png", s, a, emo, seed, _stream_device_png)

    @torch.no_grad()
    def infer_pasted_png(self, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False, seed=25,
                         feather=None, band=None, resample=None):
        """infer_pasted with the frames leaving as LOSSLESS PNG files: a png.PngFrames in pinned host memory; file i decodes to
        infer_pasted(...)[i] bit for bit and is bitwise host_models.png_encode_rgb8 of it.  Paste and encoder run on the device and
        only the files cross PCIe.  A portrait of any size up to 16384 x 16384 is taken.  FLOAT_AMD_RANGE applies as in
        infer_device_png; FLOAT_AMD_VERIFY is NOT applied and FLOAT_AMD_OVERLAP is ignored.  resample: as in infer_pasted - the
        files decode to infer_pasted(..., resample=resample)."""
        self._paste_call("infer_pasted_png", ref_img, resample=resample)
        band = self._png_call("infer_pasted_png", band, ref_img)
        s, a, place = self.host_inputs_placed(ref_img, ref_audio, no_crop)
        while True:
            c, noise = self._clip_inputs(s, a, emo, seed)
            frames = self.G.generate_to_png(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                            noise=noise, band=band, place=place, feather=feather, resample=resample)
            if self.check_range("InferenceAgent.infer_pasted_png", allow_rebuild=True) != "rebuilt":
                return frames  # otherwise once more, in the wider types

    def stream_pasted_png(self, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False, seed=25,
                          feather=None, band=None, slots=3, resample=None):
        """The streaming sibling of infer_pasted_png: a generator of PngBlock(first, last, frames) under the ring rules of
        stream_device_png - concatenated, the files infer_pasted_png returns.  slots < 2 or a band outside its rule raise
        ValueError here, at the call.  FLOAT_AMD_RANGE is applied once after the last block (auto acts as warn); FLOAT_AMD_VERIFY
        is NOT applied and FLOAT_AMD_OVERLAP is ignored.  resample: as in infer_pasted, refused at the call too."""
        self._check_stream_call("stream_pasted_png", slots)
        self._paste_call("stream_pasted_png", ref_img, resample=resample)
        band = self._png_call("stream_pasted_png", band, ref_img)

        def _stream_pasted_png(c, noise, place):
            return self.G.stream_to_png(c["r_s"], c["wa"], c["we"], c["s_r"], None, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale,
                                        noise=noise, band=band, slots=int(slots), place=place, feather=feather,
                                        resample=resample)
        return self._stream_placed("InferenceAgent.stream_pasted_png", ref_img, ref_audio, no_crop, emo, seed, _stream_pasted_png)

    def write_apng(self, path, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", no_crop=False, seed=25,
                   fps=None, paste_back=False, feather=None, band=None, resample=None):
        """A lossless clip in one file: host_inputs, stream_device_png, and host_models.ApngWriter on `path` (a path or a seekable
        binary file object) - an animated PNG that browsers and ffmpeg open, every frame bit for bit the 8-bit frame.  The
        zlib streams are copied as the device wrote them and every chunk CRC comes from the device's per-frame CRCs.  APNG carries
        NO AUDIO: the clip's sound has to be kept separately (write_video writes a file with an audio track).  fps defaults to
        opt.fps.  Returns the number of frames written.
        paste_back=True: the frames are the user's portrait with the generated face pasted back (stream_pasted_png, `feather` as
        in infer_pasted) and the file is written at the portrait's size, any size up to 16384.  resample: as in infer_pasted; with
        paste_back=False anything but None is a ValueError, before the file is opened."""
        o = self.opt
        fps = o.fps if fps is None else fps
        self._paste_call("write_apng", ref_img, resample=resample, paste_back=paste_back)
        if paste_back:
            img = ref_img[0] if ref_img.dim() == 4 else ref_img
            height, width = int(img.shape[0]), int(img.shape[1])
            blocks = self.stream_pasted_png(ref_img, ref_audio, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, no_crop, seed, feather, band,
                                            resample=resample)
        else:
            height = width = o.input_size
            band = self._png_call("write_apng", band)
            with torch.no_grad():
                s, a = self.host_inputs(ref_img, ref_audio, no_crop)
            blocks = self.stream_device_png(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, band)
        try:
            with host_models.ApngWriter(path, width, height, fps) as w:
                for blk in blocks:
                    w.write(blk.frames)
                return w.frames
        finally:
            blocks.close()  # a writer that failed leaves no stream open on the agent

    def range_counts(self, reset=True):
        """{operator: clamped / non-finite 16-bit stores since the last call} over every fp16 handle of the agent."""
        if self.G is None:
            return {}
        counts = self.G.range_counts(reset)
        for name, op in (("encoder", self.enc), ("audio", self.audio_encoder), ("speech_emotion", self.emotion_encoder),
                         ("face_detector", self.face)):
            if op is not None and op.dtype == "fp16":
                counts[name] = op.saturation(reset)
        return counts

    def check_range(self, where, allow_rebuild=False):
        """Once per clip, after the frames have arrived: an fp16 operator that left its range does not go unnoticed.
        FLOAT_AMD_RANGE = warn (default: RuntimeWarning + log line) | raise (Fp16RangeError) | off (skip the 8-byte reads) |
        auto: warn, then REBUILD the operators that overflowed in a type with the range - decoder + encoder in fp32 (the
        verification mode: same kernels, 1/16 of the MFMA rate), FMT / audio / speech-emotion in bf16 - and tell the caller to
        run the clip again ("rebuilt"); the agent keeps those types from then on."""
        mode = os.environ.get("FLOAT_AMD_RANGE", "warn").lower()
        if mode == "off":
            return {}
        bad = report_range(self.range_counts(), where, mode="warn" if mode == "auto" else mode)
        if mode == "auto" and bad and allow_rebuild:
            b, changes = self._build, {}
            if ("decoder" in bad or "encoder" in bad) and b["dec_dtype"] != "fp32":
                changes["dec_dtype"] = "fp32"
            if "fmt" in bad and b["fmt_dtype"] == "fp16":
                changes["fmt_dtype"] = "bf16"
            if ("audio" in bad or "speech_emotion" in bad) and b["aud_dtype"] == "fp16":
                changes["aud_dtype"] = "bf16"
            return self._rebuild(where, changes, "fmt=%(fmt_dtype)s, decoder/encoder=%(dec_dtype)s, audio=%(aud_dtype)s") or bad
        return bad

    def _rebuild(self, where, changes, types):
        """Apply `changes` ({key of _build: dtype}) and rebuild the operators in the new types (`types`: how the caller's log
        line names them).  Returns "rebuilt" - the caller runs the clip again - or None where nothing changes."""
        if not changes:
            return None
        self._build.update(changes)
        main_logger.warning("%s: rebuilding the operators as %s and running the clip again", where, types % self._build)
        self.offload()
        self.to_target()
        return "rebuilt"

    @torch.no_grad()
    def check_precision(self, where, s, c, noise, r_d, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, allow_rebuild=False,
                        frames_dev=None):
        """The fp16 PRECISION guard, the sibling of check_range (which sees only values beyond fp16's range): after a clip has
        arrived, run the fp32 verification mode of the FMT and the decoder on a small sample of it and compare on the device
        (FloatHotPath.verify_precision).  s: the portrait (1,3,H,W) of the clip, c: its conditions_device result, noise / r_d:
        the noise it was sampled from and the latents it gave; the device-side frames are the hot path's fp32 staging buffer, or
        `frames_dev` (fp32, at least the first k frames) where the clip left as 8-bit frames.
          FLOAT_AMD_VERIFY         off (default: infer_device never calls this) | first (the first clip after the operators
                                   were built or rebuilt) | always
          FLOAT_AMD_VERIFY_ACTION  warn (default) | raise (Fp16PrecisionError) | auto: warn, REBUILD the operator at fault in
                                   fp32 - decoder + encoder when the decoder comparison is below the threshold, otherwise the
                                   FMT - and tell the caller to run the clip again ("rebuilt"); the agent keeps those types
          FLOAT_AMD_VERIFY_FRAMES  frames compared (default 8, clipped to min(T, n_cur))
          FLOAT_AMD_VERIFY_PSNR    the end-to-end limit in dB (default 40.0, the project's stated tolerance)
        Covered: window 0 of the sampler and the first k frames.  The skip features of the fp32 side come from an fp32 twin of
        the appearance encoder on the same image; s_r and r_s are the product's.  NOT covered: the audio and speech-emotion
        operators - wa and we are taken from the product for both sides.  The twins are built for the check and closed after
        it.  Returns the operator at fault, "rebuilt", or None; the report stays in self.last_precision_report."""
        import time
        t0 = time.perf_counter()
        o, T = self.opt, c["T"]
        k = min(verify_frames_default(), T, self.cfg.num_frames_for_clip)
        enc32 = EncoderHIP(self._parts["enc"], o.input_size, o.dim_w, getattr(o, "dim_m", 20), self.rank, dtype="fp32",
                           direction_weight=self._parts["dec"]["direction.weight"])
        try:
            feats = enc32.encode_image_into_latent(s, want_feats=True)[2]
            rep = self.G.verify_precision(c["r_s"], c["wa"], c["we"], c["s_r"], feats, o.nfe, a_cfg_scale, r_cfg_scale,
                                          e_cfg_scale, noise, r_d, frames_dev if frames_dev is not None else self.G.staging(T), k)
        finally:
            enc32.close()
        del feats
        self._precision_checked = True
        rep["ms"] = (time.perf_counter() - t0) * 1e3
        rep["dtypes"] = dict(fmt=self.G.fmt.dtype, decoder=self.G.dec.dtype, encoder=self.enc.dtype)
        self.last_precision_report = rep
        main_logger.info(
            "%s: precision check (fmt %s, decoder %s) on window 0 / %d frames: FMT latents rel-L2 %.2e | decoder %.1f dB | "
            "end to end %.1f dB, %.2f %% beyond 2/255, max %.3f, %d non-finite | one-off cost %.0f ms (twins %.0f ms, %.2f GB)",
            where, rep["dtypes"]["fmt"], rep["dtypes"]["decoder"], rep["k"], rep["fmt"]["rel_l2"], rep["decoder"]["psnr"],
            rep["end_to_end"]["psnr"], rep["end_to_end"]["pct_beyond"], rep["end_to_end"]["max"],
            rep["end_to_end"]["non_finite"], rep["ms"], rep["build_ms"], rep["hbm_bytes"] / 2**30)
        fault = report_precision(rep, where)
        if fault and allow_rebuild and os.environ.get("FLOAT_AMD_VERIFY_ACTION", "warn").lower() == "auto":
            key = {"decoder": "dec_dtype", "fmt": "fmt_dtype"}[fault]
            changes = {key: "fp32"} if self._build[key] != "fp32" else {}
            return self._rebuild(where, changes, "fmt=%(fmt_dtype)s, decoder/encoder=%(dec_dtype)s") or fault
        return fault

    @torch.no_grad()
    def infer_device_batch(self, items, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, emo="S2E", seeds=None,
                           out_dtype=None, out_format=None, matrix=None):
        """B clips through one stacked FMT chain (every weight is read once per evaluation for all of them), then decoded one
        after the other.  Clips of equal length run float_fmt_sample_batch; clips of different lengths run its ragged sibling
        (FlowMatchingTransformerHIP.sample_ragged: a clip leaves the stack after its last window).  items: [(s (1,3,H,W), a (N,))] in HBM; seeds: one per
        item (FloatProcess uses seed + i, nodes.py:189-209) - each item keeps its own noise stream, so item i is what
        infer_device gives for it alone (bit for bit where the GEMM tilings coincide, within the fp16 tolerance otherwise).
        emo: one value for all items, or a list with one per item (a list ALWAYS means per item: the chunk length goes in a tuple); dynamic emotion ("dynamic", ("dynamic", sec)) for all or none.
        Returns a list of (T,H,W,3) pinned host tensors, fp32 or - out_dtype=torch.uint8 - 8-bit frames as in infer_device; out_format="i420":
        (T,3H/2,W) uint8 planar YUV 4:2:0 as there, with `matrix` as there."""
        matrix = self._crop_matrix("infer_device_batch", None, out_dtype, out_format, matrix)  # a contradiction is refused before anything runs
        B = len(items)
        emos = list(emo) if isinstance(emo, list) else [emo] * B  # a list: one `emo` per item
        if len(emos) != B:
            raise ValueError("infer_device_batch: %d emo entries for %d items" % (len(emos), B))
        dyn = [host_models.dynamic_emotion_chunk_sec(e) is not None for e in emos]
        if any(dyn) and not all(dyn):
            raise ValueError("infer_device_batch: dynamic emotion for every item of a batch or for none (one stacked chain takes `we` "
                             "per frame for all clips or one row per clip); got %s" % (emos,))
        dyn = all(dyn)
        self.to_target()
        seeds = list(seeds) if seeds is not None else [self.opt.seed] * B
        # once-per-clip producers of every item; the encoder's skip maps of item i are copied aside (33 MB, a D2D copy) so
        # that no item needs a second encoder pass when its turn to decode comes
        conds, feats = [], []
        slots = self._feat_slots
        for i, (s, a) in enumerate(items):
            conds.append(self.conditions_device(s, a, emos[i]))
            if i >= len(slots):
                slots.append(None)
            slots[i] = self.enc.export_feats16(slots[i])
            feats.append(slots[i])
        T = conds[0]["T"]
        r_s = torch.cat([c["r_s"].reshape(1, -1) for c in conds])
        if any(c["T"] != T for c in conds):
            # clips of different lengths: one chain whose stack shrinks as clips end (float_fmt_sample_batch_ragged)
            noise = self._noise_ragged_to_device([self.G.n_chunks(c["T"]) for c in conds], seeds)
            r_d = self.G.batched_fmt(B).sample_ragged(r_s, [c["wa"].reshape(c["T"], -1) for c in conds],
                                                      [c["we"].reshape(c["T"] if dyn else 1, -1) for c in conds], noise, self.opt.nfe,
                                                      a_cfg_scale, r_cfg_scale, e_cfg_scale)
        else:
            noise = self._noise_batch_to_device(self.G.n_chunks(T), seeds)
            wa = torch.cat([c["wa"].reshape(1, T, -1) for c in conds])
            we = torch.cat([c["we"].reshape(1, T if dyn else 1, -1) for c in conds])
            r_d = self.G.batched_fmt(B).sample(r_s, wa, we, noise, self.opt.nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale)
        out = []
        for i in range(B):
            # decodes queue back to back: the last frames of item i cross PCIe inside the launches of item i + 1
            self.G.dec.set_feats16(feats[i], self.enc.dtype)
            out.append(self.G.decode_to_host(conds[i]["s_r"], r_d[i], out_dtype=out_dtype, out_format=out_format, matrix=matrix))
        torch.cuda.current_stream(self.rank).synchronize()
        self.G.release_host_inflight()
        self.check_range("InferenceAgent.infer_device_batch")
        return out

    @torch.no_grad()
    def run_inference(self, res_video_path, ref_img, ref_audio, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0,
                      emo="S2E", nfe=10, no_crop=False, seed=25, out_format=None, matrix=None):
        """Reference signature (generate.py:154-173).  Returns (T,H,W,3) fp32 in [0,1] on the CPU (pinned); out_format="i420":
        (T,3H/2,W) uint8 planar YUV 4:2:0 as in infer_device, `matrix` its colour matrix as there.
        Like the reference, the grid size comes from opt.nfe, not from the `nfe` argument (FLOAT.py:188)."""
        self._crop_matrix("run_inference", None, None, out_format, matrix)  # refused before the inputs are prepared
        s, a = self.host_inputs(ref_img, ref_audio, no_crop)
        return self.infer_device(s, a, a_cfg_scale, r_cfg_scale, e_cfg_scale, emo, seed, out_format=out_format, matrix=matrix)
