"""Host mirror of the motion-autoencoder encoder (reference encoder.py Encoder / EncoderApp and
FLOAT.encode_image_into_latent, FLOAT.py:283-291), running on the HIP operator (`float_enc_*`,
include/float_hip.h).  Once per clip: image -> s_r, skip features, motion coefficients, r_s."""
import ctypes as C
import math

import torch

from . import native


@native.rebuildable
class EncoderHIP:
    """Encoder(size, dim, dim_motion) (encoder.py:234-281).  `state_dict` uses the reference keys
    (`net_app.convs.*`, `fc.*`; a `motion_autoencoder.enc.` prefix is stripped); pass the decoder's
    `direction.weight` (styledecoder.py:431) as `direction_weight` to get r_s from the same launch chain."""

    def __init__(self, state_dict, size=512, dim=512, dim_motion=20, device="cuda:0", dtype="fp16", direction_weight=None):
        self.size, self.dim, self.dim_motion = size, dim, dim_motion
        self.device = torch.device(device)
        self.dtype = dtype = native.canon_dtype(dtype)
        self.n_feats = int(math.log2(size)) - 2
        pref = "motion_autoencoder.enc."
        # the Blur buffers (`*.kernel`, encoder.py:59-71) travel too: the operator has [1,3,3,1] in its code and refuses others
        sd = {(k[len(pref):] if k.startswith(pref) else k): v for k, v in state_dict.items()}
        if direction_weight is not None:
            sd["direction.weight"] = direction_weight
        self.has_direction = "direction.weight" in sd
        arr, keep = native.tensor_table(sd)
        cfg = native.EncCfg(size, dim, dim_motion, native.DTYPES[dtype])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            native.check(native.lib().float_enc_create(C.byref(cfg), arr, len(sd), C.byref(h)))
        self._h = h
        del keep

    def saturation(self, reset=False):
        """Threads with a clamped (+-65504) or non-finite 16-bit activation store since create / the last reset
        (float_enc_saturation): 0 unless the checkpoint leaves fp16's range - then the result is not the reference's within the
        stated tolerance; run it with dtype="fp32".  Always 0 for bf16 / fp32 handles.  Synchronises the current stream."""
        with torch.cuda.device(self.device):
            return native.saturation("float_enc_saturation", self._h, self.device, reset)

    def close(self):
        if getattr(self, "_h", None) and native is not None:
            native.lib().float_enc_destroy(self._h)
            self._h = None

    __del__ = close

    def feat_shapes(self):
        from .weights import ENC_CHANNELS
        return [(ENC_CHANNELS[8 << i], 8 << i, 8 << i) for i in range(self.n_feats)]

    @torch.no_grad()
    def encode_image_into_latent(self, x, want_feats=True):
        """FLOAT.py:283-291 for one image: x (1,3,S,S) or (3,S,S) in [-1,1].
        Returns s_r (1,dim), r_s_lambda (1,dim_motion), feats [(1,C,R,R)] (reference order), r_s (1,dim)|None."""
        if x.numel() != 3 * self.size * self.size:
            raise ValueError("encoder input must be one (3,%d,%d) image, got %s" % (self.size, self.size, tuple(x.shape)))
        x = x.to(self.device, torch.float32).reshape(3, self.size, self.size).contiguous()
        dev = self.device
        s_r = torch.empty(1, self.dim, device=dev)
        lam = torch.empty(1, self.dim_motion, device=dev)
        r_s = torch.empty(1, self.dim, device=dev) if self.has_direction else None
        feats = [torch.empty((1,) + shp, device=dev) for shp in self.feat_shapes()] if want_feats else []
        ptrs = (C.c_void_p * max(len(feats), 1))(*[f.data_ptr() for f in feats])
        with torch.cuda.device(dev):
            native.check(native.lib().float_enc_forward(
                self._h, native.dev_ptr(x), native.dev_ptr(s_r), native.dev_ptr(lam), native.dev_ptr(r_s), ptrs, len(feats),
                native.stream_ptr(dev)))
        return s_r, lam, feats, r_s

    @torch.no_grad()
    def encode_motion(self, frames_u8, block=None):
        """Motion coefficients of T driving frames (float_enc_motion): frames_u8 (T,S,S,3) uint8 NHWC on the device ->
        lambda (T, dim_motion) fp32, `fc(net_app(q / 127.5 - 1))` per frame (encoder.py:262-277).  The frames go through in
        blocks of `block` frames (None: the handle's current block, 8 on first use) over a scratch of their own: the source
        portrait's state in the handle (s_r, the skip maps) stays what the last encode_image_into_latent left.  Row t does not
        depend, by a bit, on T, on `block` or on the other frames."""
        S = self.size
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or tuple(frames_u8.shape[1:]) != (S, S, 3) or frames_u8.shape[0] < 1:
            raise ValueError("driving frames must be (T,%d,%d,3) uint8 with T >= 1, got %s %s" % (S, S, tuple(frames_u8.shape), frames_u8.dtype))
        frames_u8 = frames_u8.to(self.device).contiguous()
        lam = torch.empty(frames_u8.shape[0], self.dim_motion, device=self.device)
        L = native.lib()
        with torch.cuda.device(self.device):
            if block is not None:
                native.check(L.float_enc_motion_reserve(self._h, int(block)))
            native.check(L.float_enc_motion(self._h, C.c_void_p(frames_u8.data_ptr()), frames_u8.shape[0], native.dev_ptr(lam),
                                            native.stream_ptr(self.device)))
        return lam

    DRIVE_MODES = {"absolute": 0, "relative": 1}

    @torch.no_grad()
    def drive_rows(self, lam, mode="relative", lam_source=None, lam_start=None):
        """Driving rows r_d (T, dim) of the decoder from lambda rows (float_enc_drive_rows; host_models.drive_rows is the
        definition).  "absolute": Direction(lam[t]); "relative": Direction(lam[t] - lam_start + lam_source), lam_source the
        portrait's own lambda (encode_image_into_latent()[1]), lam_start the driving clip's reference row (None: lam[0])."""
        if mode not in self.DRIVE_MODES:
            raise ValueError("drive_rows: mode must be 'relative' or 'absolute', got %r" % (mode,))
        if mode == "relative" and lam_source is None:
            raise ValueError("drive_rows: the relative mode needs lam_source, the portrait's own lambda")
        dev = self.device
        row = lambda v: None if v is None else v.to(dev, torch.float32).reshape(self.dim_motion).contiguous()
        lam = lam.to(dev, torch.float32).reshape(-1, self.dim_motion).contiguous()
        src, start = row(lam_source), row(lam_start)
        r_d = torch.empty(lam.shape[0], self.dim, device=dev)
        with torch.cuda.device(dev):
            native.check(native.lib().float_enc_drive_rows(self._h, native.dev_ptr(lam), lam.shape[0], self.DRIVE_MODES[mode], native.dev_ptr(src),
                                                           native.dev_ptr(start), native.dev_ptr(r_d), native.stream_ptr(dev)))
        return r_d

    def quantise_frames(self, x):
        """(T,3,S,S) in [-1,1] -> (T,S,S,3) uint8, q = round((x + 1) * 127.5) clamped to 0..255: the 8-bit grid the motion pass
        reads (q / 127.5 - 1 gives back x for every x that came from 8-bit pixels)."""
        x = x.to(self.device, torch.float32).reshape(-1, 3, self.size, self.size)
        return ((x + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def forward(self, input_source, input_target=None, h_start=None):
        """Encoder.forward (encoder.py:262-281).  input_target=None: (h_source, None, feats).  With input_target (T,3,S,S) in
        [-1,1]: (h_source, [h_motion_target], feats), or with h_start (a lambda row) (h_source, [h_motion_target,
        h_motion_source, h_start], feats) - the lists Synthesis.forward takes as `alpha`.  The target frames are QUANTISED to
        the 8-bit grid on the way in (quantise_frames): the motion pass reads 8-bit frames, which is what a video holds."""
        if input_target is None:
            s_r, _, feats, _ = self.encode_image_into_latent(input_source)
            return s_r, None, feats
        s_r, lam_s, feats, _ = self.encode_image_into_latent(input_source)
        h_t = self.encode_motion(self.quantise_frames(input_target))
        return s_r, ([h_t] if h_start is None else [h_t, lam_s, h_start]), feats

    __call__ = forward

    def export_feats16(self, bufs=None):
        """Copies of the NHWC skip features of the last forward in the operator's element type (float_enc_export_feats16), one
        flat device tensor per map - what `SynthesisHIP.set_feats16` takes back.  A batch of portraits keeps one set per item,
        so that item i can be decoded after item j was encoded without a second encoder pass."""
        eb = 4 if self.dtype == "fp32" else 2
        if bufs is None:
            bufs = [torch.empty(c * r * r * eb, dtype=torch.uint8, device=self.device) for c, r, _ in self.feat_shapes()]
        ptrs = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
        with torch.cuda.device(self.device):
            native.check(native.lib().float_enc_export_feats16(self._h, ptrs, len(bufs), native.stream_ptr(self.device)))
        return bufs

    def hand_feats_to(self, dec):
        """Give the NHWC 16-bit skip features of the last forward to a SynthesisHIP of the same dtype
        without the fp32 NCHW round trip (float_enc_feats16 -> float_dec_set_feats16)."""
        n = self.n_feats
        ptrs = (C.c_void_p * n)()
        ch = (C.c_int32 * n)()
        got = C.c_int32(0)
        L = native.lib()
        native.check(L.float_enc_feats16(self._h, ptrs, ch, n, C.byref(got)))
        with torch.cuda.device(self.device):
            native.check(L.float_dec_set_feats16(dec._h, ptrs, got.value, native.DTYPES[self.dtype], native.stream_ptr(self.device)))
