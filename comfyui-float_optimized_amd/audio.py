"""Host mirror of the audio conditioning encoder (reference FLOAT.AudioEncoder, FLOAT.py:304-375; its wav2vec2
backbone src/nodes/models/wav2vec2.py), running on the HIP operator (`float_aud_*`, include/float_hip.h)."""
import ctypes as C

import torch
import torch.nn.functional as F

from . import native
from .config import AudioConfig


@torch.no_grad()
def preprocess_audio_device(waveform, sample_rate, target_rate=16000, device="cuda:0", normalize=True, zeros=24, rolloff=0.945):
    """host_models.preprocess_audio on the device (`float_aud_front`): a (C,N) or (N,) waveform on any device -> the
    (1, n_out) fp32 mono waveform at target_rate, zero-mean / unit-variance when `normalize`.  The raw samples cross PCIe
    (non_blocking) and the channel mean, the band-limited resampler (host_models.resample_sinc_direct is its definition: any
    pair of rates, nothing snapped) and the statistics run as HIP kernels on the current stream; the output and the scratch
    come from torch's allocator, nothing synchronises."""
    device = torch.device(device)
    w = waveform.detach().to(device, non_blocking=True)
    if w.dim() == 1:
        w = w[None]
    if w.dim() != 2:
        raise ValueError("preprocess_audio_device: waveform must be (C, N) or (N,), got %s" % (tuple(waveform.shape),))
    if w.dtype != torch.float32:
        w = w.float()
    if w.shape[1] > 1 and w.stride(1) != 1:
        w = w.contiguous()
    C_, n_in = int(w.shape[0]), int(w.shape[1])
    if n_in == 0:
        raise ValueError("preprocess_audio_device: the waveform is empty")
    L = native.lib()
    n_out = int(L.float_aud_front_len(n_in, int(sample_rate), int(target_rate)))
    need = int(L.float_aud_front_work_bytes(n_in, int(sample_rate), int(target_rate)))
    with torch.cuda.device(device):
        a = torch.empty(1, n_out, dtype=torch.float32, device=device)
        work = torch.empty(max(1, (need + 7) // 8), dtype=torch.float64, device=device)
        native.check(L.float_aud_front(C.c_void_p(w.data_ptr()), C_, int(w.stride(0)) if C_ > 1 else n_in, n_in, int(sample_rate),
                                       int(target_rate), int(zeros), float(rolloff), native.AUD_FRONT_NORMALIZE if normalize else 0,
                                       C.c_void_p(a.data_ptr()), n_out, C.c_void_p(work.data_ptr()), work.numel() * 8,
                                       native.stream_ptr(device)))
    return a


@native.rebuildable
class AudioEncoderHIP:
    """state_dict keys: `wav2vec2.*`, `audio_projection.{0,1}.*` (an `audio_encoder.` prefix is stripped) - the
    reference's AudioEncoder.state_dict()."""

    def __init__(self, state_dict, cfg: AudioConfig = None, device="cuda:0", dtype="fp16", sampling_rate=16000, fps=25.0):
        self.cfg = cfg or AudioConfig()
        self.device = torch.device(device)
        self.dtype = dtype = native.canon_dtype(dtype)
        self.sampling_rate, self.fps = sampling_rate, fps
        sd = {}
        for k, v in state_dict.items():
            for pref in ("audio_encoder.", "emotion_encoder.wav2vec2_for_emotion."):
                if k.startswith(pref):
                    k = k[len(pref):]
            if not k.endswith("masked_spec_embed"):  # only used when mask_time_indices is given (never at inference)
                sd[k] = v
        c = self.cfg
        n = len(c.conv_dim)
        if n > 8 or len(c.conv_kernel) != n or len(c.conv_stride) != n:
            raise ValueError("feature extractor must have <= 8 layers with matching kernel/stride lists")
        ncfg = native.AudCfg()
        ncfg.n_conv = n
        for i in range(n):
            ncfg.conv_dim[i], ncfg.conv_kernel[i], ncfg.conv_stride[i] = c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i]
        ncfg.hidden, ncfg.layers, ncfg.heads, ncfg.intermediate = c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size
        ncfg.pos_k, ncfg.pos_groups = c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups
        ncfg.dim_w, ncfg.only_last, ncfg.dtype, ncfg.ln_eps = c.dim_w, int(c.only_last_features), native.DTYPES[dtype], c.layer_norm_eps
        if c.feat_extract_norm not in ("group", "layer"):
            raise ValueError("feat_extract_norm must be 'group' or 'layer', got %r" % (c.feat_extract_norm,))
        ncfg.feat_norm_layer, ncfg.stable_ln = int(c.feat_extract_norm == "layer"), int(c.do_stable_layer_norm)
        ncfg.conv_bias, ncfg.num_labels = int(c.conv_bias), int(c.num_labels)
        arr, keep = native.tensor_table(sd)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            native.check(native.lib().float_aud_create(C.byref(ncfg), arr, len(sd), C.byref(h)))
        self._h = h
        self._reserved = (0, 0)  # a new handle has no workspace yet (also after a rebuild: native.rebuildable)
        del keep

    def saturation(self, reset=False):
        """Threads with a clamped (+-65504) or non-finite 16-bit activation store since create / the last reset
        (float_aud_saturation): 0 unless the checkpoint leaves fp16's range - then the result is not the reference's within the
        stated tolerance; run it with dtype="fp32" (or "bf16").  Always 0 for bf16 / fp32 handles.  Synchronises the current stream."""
        with torch.cuda.device(self.device):
            return native.saturation("float_aud_saturation", self._h, self.device, reset)

    def close(self):
        if getattr(self, "_h", None) and native is not None:
            native.lib().float_aud_destroy(self._h)
            self._h = None

    __del__ = close

    def reserve(self, n_samples, seq_len=0):
        """Workspace for clips of up to n_samples samples / seq_len frames (float_aud_reserve): the operator's run-time calls
        never allocate, so this mirror grows the reservation (a stream synchronise + hipMalloc) before a longer clip."""
        cap = getattr(self, "_reserved", (0, 0))
        frames = int(seq_len) if seq_len > 0 else int(n_samples) // 320 + 1
        if n_samples <= cap[0] and frames <= cap[1]:
            return
        with torch.cuda.device(self.device):
            native.check(native.lib().float_aud_reserve(self._h, int(n_samples), int(seq_len), native.stream_ptr(self.device)))
        self._reserved = (max(cap[0], int(n_samples)), max(cap[1], frames))

    @torch.no_grad()
    def attention_probe(self, qkv):
        """Test hook (float_aud_debug): qkv (Tn, 3*hidden) = [q | k | v] -> (Tn, hidden), the attention launch of this handle
        (operand type, FLOAT_AUD_ATTN_MFMA as read at create) on caller data: softmax(q k^T / 8) v per head of 64, no mask."""
        D = self.cfg.hidden_size
        if qkv.dim() != 2 or qkv.shape[0] < 1 or qkv.shape[1] != 3 * D:
            raise ValueError("qkv must be (Tn >= 1, %d), got %s" % (3 * D, tuple(qkv.shape)))
        qkv = qkv.to(self.device, torch.float32).contiguous()
        Tn = int(qkv.shape[0])
        self.reserve(400, Tn)  # 400 samples: the shortest clip the feature extractor takes; the hook only uses the frame buffers
        out = torch.empty(Tn, D, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            native.check(native.lib().float_aud_debug(self._h, 1, native.dev_ptr(qkv), Tn, native.dev_ptr(out),
                                                      native.stream_ptr(self.device)))
        return out

    @torch.no_grad()
    def inference(self, a, seq_len):
        """AudioEncoder.inference (FLOAT.py:370-375): a (B,N) normalised 16 kHz waveform -> wa (B,seq_len,dim_w)."""
        a = a.to(self.device, torch.float32)
        if a.dim() == 1:
            a = a[None]
        need = int(seq_len * self.sampling_rate / self.fps)
        if a.shape[1] % need != 0:  # FLOAT.py:371-373
            a = F.pad(a[:, None], (0, need - a.shape[1]), mode="replicate")[:, 0]
        a = a.contiguous()
        self.reserve(a.shape[1], seq_len)
        out = torch.empty(a.shape[0], seq_len, self.cfg.dim_w, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            for b in range(a.shape[0]):
                native.check(native.lib().float_aud_inference(self._h, native.dev_ptr(a[b]), a.shape[1], int(seq_len),
                                                              native.dev_ptr(out[b]), native.stream_ptr(self.device)))
        return out


@native.rebuildable
class Audio2EmotionHIP(AudioEncoderHIP):
    """Speech-to-emotion (reference Audio2Emotion, FLOAT.py:378-401, on Wav2Vec2ForSpeechClassification,
    wav2vec2_ser.py:41-118): the wav2vec2-large variant of the same operator with the classification head.
    state_dict keys: `wav2vec2.*`, `classifier.{dense,out_proj}.*` (prefix `emotion_encoder.wav2vec2_for_emotion.` stripped)."""

    id2label = {0: "angry", 1: "disgust", 2: "fear", 3: "happy", 4: "neutral", 5: "sad", 6: "surprise"}  # FLOAT.py:390

    def __init__(self, state_dict, cfg: AudioConfig = None, device="cuda:0", dtype="fp16"):
        from .config import emotion_audio_config
        cfg = cfg or emotion_audio_config()
        if not cfg.num_labels:
            raise ValueError("Audio2EmotionHIP needs a config with num_labels > 0")
        super().__init__(state_dict, cfg, device, dtype)

    def inference(self, a, seq_len):
        raise TypeError("the speech-emotion model has no audio projection; use predict_emotion")

    @torch.no_grad()
    def predict_emotion(self, a, prev_a=None):
        """FLOAT.py:396-401: a (B,N) normalised waveform -> softmax scores (B, num_labels)."""
        if prev_a is not None:
            a = torch.cat([prev_a, a], dim=1)
        a = a.to(self.device, torch.float32)
        if a.dim() == 1:
            a = a[None]
        a = a.contiguous()
        self.reserve(a.shape[1], 0)
        out = torch.empty(a.shape[0], self.cfg.num_labels, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            for b in range(a.shape[0]):
                native.check(native.lib().float_aud_classify(self._h, native.dev_ptr(a[b]), a.shape[1], native.dev_ptr(out[b]),
                                                             native.stream_ptr(self.device)))
        return out

    def segment_normalised(self, n_floats):
        """Test hook (float_aud_debug, what = 2): the first n_floats of the normalised (n_seg, seg_len) copy that the last
        float_aud_classify_segments(FLOAT_AUD_SEG_NORMALIZE) of this handle left in its workspace."""
        out = torch.empty(int(n_floats), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            native.check(native.lib().float_aud_debug(self._h, 2, None, int(n_floats), native.dev_ptr(out), native.stream_ptr(self.device)))
        return out

    @torch.no_grad()
    def classify_segments(self, a, n_seg, seg_len, seg_stride=None, normalize=True, T=None):
        """float_aud_classify_segments on a device waveform: segment s = a[s * seg_stride : s * seg_stride + seg_len] ->
        (scores (n_seg, labels), frames (T, labels) or None).  Reserves first; `a` is not written."""
        a = a.to(self.device, torch.float32).reshape(-1).contiguous()
        n_seg, seg_len = int(n_seg), int(seg_len)
        seg_stride = seg_len if seg_stride is None else int(seg_stride)
        if n_seg >= 1 and seg_stride >= seg_len and a.numel() < (n_seg - 1) * seg_stride + seg_len:
            raise ValueError("classify_segments: %d samples do not hold %d segments of %d at stride %d" % (a.numel(), n_seg, seg_len, seg_stride))
        labels = self.cfg.num_labels
        scores = torch.empty(max(n_seg, 0), labels, device=self.device, dtype=torch.float32)
        frames = torch.empty(int(T), labels, device=self.device, dtype=torch.float32) if T is not None else None
        L = native.lib()
        with torch.cuda.device(self.device):
            st = native.stream_ptr(self.device)
            native.check(L.float_aud_reserve_segments(self._h, n_seg, seg_len, st))  # a no-op when it fits
            native.check(L.float_aud_classify_segments(self._h, native.dev_ptr(a), n_seg, seg_len, seg_stride,
                                                       native.AUD_SEG_NORMALIZE if normalize else 0, native.dev_ptr(scores),
                                                       native.dev_ptr(frames) if frames is not None else None, int(T or 0),
                                                       _nearest_scale(n_seg, T or 1), st))
        return scores, frames

    @torch.no_grad()
    def predict_emotion_chunks(self, w, chunk, T=None, normalize=True):
        """Dynamic emotion (reference FloatExtractEmotionWithCustomModelDyn, nodes_vadv.py:812-838) on the device: w, the (N,) or
        (1, N) mono waveform at the model's rate on any device, in chunks of `chunk` samples, each normalised on its own
        (`normalize`) and classified -> (seq (n_chunks, labels), frames (T, labels) or None), frames = host_models.nearest_rows(seq, T).
        Both on the device; nothing synchronises and nothing comes back to the host.
        The N // chunk equal chunks are ONE float_aud_classify_segments (one stacked launch sequence); a shorter last chunk is
        normalised on its own by the audio front end's kernels (float_aud_front at equal rates), replicate-padded to 400 samples
        when it is shorter than the feature extractor's receptive field (as the node does), and scored by float_aud_classify into
        the last row of seq.  The expansion then runs ONCE over all rows: float_aud_expand_rows is its own entry of the ABI, so a
        clip with a tail does not expand the stacked rows a second time; without a tail it is the `frames` argument of the
        stacked call (the same kernel).
        What the stacked call does not take goes chunk by chunk through the tail's route - normalised on the device, padded,
        float_aud_classify into row i, then the one expansion; still nothing on the host: handles with the GroupNorm extractor
        (feat_extract_norm = "group": its statistics run over time) and chunks below 400 samples (the reference's loop pads every
        such chunk, not only the last)."""
        w = w.detach()
        if w.dim() == 2 and w.shape[0] == 1:
            w = w[0]
        if w.dim() != 1:
            raise ValueError("predict_emotion_chunks: waveform must be (N,) or (1, N), got %s" % (tuple(w.shape),))
        w = w.to(self.device, torch.float32, non_blocking=True).contiguous()
        N, chunk = int(w.shape[0]), int(chunk)
        if chunk < 1 or N < 1:
            raise ValueError("predict_emotion_chunks: needs at least one sample and chunk >= 1 (N = %d, chunk = %d)" % (N, chunk))
        n_chunks = -(-N // chunk)
        stacked = N // chunk if (self.cfg.feat_extract_norm == "layer" and chunk >= 400) else 0  # rows of the stacked call
        labels = self.cfg.num_labels
        seq = torch.empty(n_chunks, labels, device=self.device, dtype=torch.float32)
        frames = torch.empty(int(T), labels, device=self.device, dtype=torch.float32) if T is not None else None
        L = native.lib()
        with torch.cuda.device(self.device):
            st = native.stream_ptr(self.device)
            inline = frames is not None and stacked == n_chunks  # every row from the stacked call: it expands its own rows
            if stacked:
                native.check(L.float_aud_reserve_segments(self._h, stacked, chunk, st))  # a no-op when it fits
                native.check(L.float_aud_classify_segments(self._h, native.dev_ptr(w), stacked, chunk, chunk,
                                                           native.AUD_SEG_NORMALIZE if normalize else 0, native.dev_ptr(seq),
                                                           native.dev_ptr(frames) if inline else None, int(T) if inline else 0,
                                                           _nearest_scale(stacked, T) if inline else 0.0, st))
            for i in range(stacked, n_chunks):
                piece = w[i * chunk:(i + 1) * chunk]
                n = int(piece.shape[0])
                if normalize:
                    piece = preprocess_audio_device(piece, self.sampling_rate, self.sampling_rate, self.device, True)[0]
                if n < 400:
                    piece = F.pad(piece[None, None], (0, 400 - n), mode="replicate")[0, 0].contiguous()
                self.reserve(piece.shape[0], 0)
                native.check(L.float_aud_classify(self._h, native.dev_ptr(piece), int(piece.shape[0]), native.dev_ptr(seq[i]), st))
            if frames is not None and not inline:
                native.check(L.float_aud_expand_rows(native.dev_ptr(seq), n_chunks, labels, native.dev_ptr(frames), int(T),
                                                     _nearest_scale(n_chunks, T), st))
        return seq, frames


def _nearest_scale(n, T):
    """(float)n / (float)T as fp32, the scale F.interpolate(mode="nearest") multiplies the output index by (host_models.nearest_rows)."""
    import numpy as np
    return float(np.float32(n) / np.float32(T))
