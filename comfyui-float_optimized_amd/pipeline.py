"""The hot path as one object: (conditioning tensors in HBM) -> r_d -> frames.
Mirrors FLOAT.sample + decode_latent_into_processed_images (reference FLOAT.py:172-253, 113-169)
with the noise stream explicit."""
import collections
import logging
import math
import os
import warnings

import torch

from . import host_models, image, jpeg, native, png
from .config import FmtConfig
from .decoder import SynthesisHIP, infer_out_format
from .fmt import FlowMatchingTransformerHIP, WindowSampler, draw_noise


class Fp16RangeError(OverflowError):
    """A 16-bit operator clamped (or stored inf for) activations beyond fp16's range: the result is not the reference's."""


def report_range(counts, where, mode=None):
    """counts: {operator name: float_*_saturation total}.  Any non-zero entry means a checkpoint / input left fp16's range in
    that operator (the frames may hold wrong or black regions).  FLOAT_AMD_RANGE = warn (default: RuntimeWarning + log) |
    raise (Fp16RangeError) | off."""
    bad = {k: v for k, v in counts.items() if v}
    mode = (mode or os.environ.get("FLOAT_AMD_RANGE", "warn")).lower()
    if not bad or mode == "off":
        return bad
    msg = ("%s: fp16 range exceeded in %s - the frames are NOT the reference's within the stated tolerance (they may show wrong "
           "or black regions). Run this checkpoint with dtype fp32 (decoder / encoder) or bf16 / fp32 (FMT / audio)."
           % (where, ", ".join("%s (%d stores)" % kv for kv in sorted(bad.items()))))
    if mode == "raise":
        raise Fp16RangeError(msg)
    logging.getLogger("float_amd").error(msg)
    warnings.warn(msg, RuntimeWarning, stacklevel=3)
    return bad


class Fp16PrecisionError(ArithmeticError):
    """The 16-bit operators stayed inside fp16's range but their rounding moved the frames further from the fp32 verification mode
    of the same kernels than the stated tolerance: the result is not the reference's."""


VERIFY_THR = 2.0 / 255  # the per-sample figure the tolerance tables quote ("share of the samples beyond 2/255")


def precision_policy(checked=False, mode=None):
    """What FLOAT_AMD_VERIFY asks for this clip: "skip" or "check".  off (default): never; first: the first clip after the
    operators were built or rebuilt (`checked` = a clip has been checked since); always: every clip."""
    mode = (mode if mode is not None else os.environ.get("FLOAT_AMD_VERIFY", "off")).lower() or "off"
    if mode not in ("off", "first", "always"):
        raise ValueError("FLOAT_AMD_VERIFY must be off, first or always (got %r)" % (mode,))
    return "check" if mode == "always" or (mode == "first" and not checked) else "skip"


def verify_frames_default():
    return max(1, int(os.environ.get("FLOAT_AMD_VERIFY_FRAMES", "8")))


def cmp_summary(rows, seg_len):
    """rows: the (n_seg, 5) float_cmp_segments statistics on the host -> one comparison of a precision report, pooled over the
    segments: psnr (peak 1.0; inf for identical buffers), psnr_min (worst segment), rel_l2, pct_beyond (share of the finite
    pairs beyond the threshold, %), max, non_finite."""
    rows = [[float(v) for v in r] for r in rows]
    n_pairs = float(seg_len) * len(rows)
    finite = n_pairs - sum(r[4] for r in rows)
    d2, b2 = sum(r[0] for r in rows), sum(r[1] for r in rows)

    def psnr(sq, n):
        return float("inf") if sq <= 0 or n <= 0 else -10.0 * math.log10(sq / n)

    return dict(psnr=psnr(d2, finite), psnr_min=min(psnr(r[0], seg_len - r[4]) for r in rows),
                rel_l2=math.sqrt(d2 / b2) if b2 > 0 else (0.0 if d2 == 0 else float("inf")),
                pct_beyond=100.0 * sum(r[3] for r in rows) / max(finite, 1.0), max=max(r[2] for r in rows),
                non_finite=int(sum(r[4] for r in rows)), segments=len(rows))


def report_precision(report, where, action=None, min_psnr=None):
    """The sibling of report_range for the OTHER way 16-bit operands go wrong: nothing overflows, the rounding is too coarse for
    this checkpoint.  report: {"decoder": cmp, "end_to_end": cmp or absent, "fmt": cmp or absent}, each a cmp_summary of the
    product against the fp32 verification mode (FloatHotPath.verify_precision / verify_decoder).  The comparison held to
    min_psnr (FLOAT_AMD_VERIFY_PSNR, default 40 dB: the project's end-to-end tolerance) is `end_to_end`, or `decoder` where
    that is all the report has; a non-finite sample in any comparison fails whatever the PSNR.  Returns None when the report
    passes, else the operator at fault: "decoder" (decoder + skip features: the decoder comparison alone is below the
    threshold or non-finite) or "fmt".  FLOAT_AMD_VERIFY_ACTION = warn (default: RuntimeWarning + log) | raise
    (Fp16PrecisionError) | auto (warn; the caller rebuilds the operator at fault in fp32)."""
    action = (action or os.environ.get("FLOAT_AMD_VERIFY_ACTION", "warn")).lower()
    if action not in ("warn", "raise", "auto"):
        raise ValueError("FLOAT_AMD_VERIFY_ACTION must be warn, raise or auto (got %r)" % (action,))
    min_psnr = float(min_psnr if min_psnr is not None else os.environ.get("FLOAT_AMD_VERIFY_PSNR", "40.0"))
    dec, e2e, fmt = report.get("decoder"), report.get("end_to_end"), report.get("fmt")
    held = e2e if e2e is not None else dec
    if held is None:
        raise ValueError("report_precision: the report holds neither an end_to_end nor a decoder comparison")
    non_finite = sum(c["non_finite"] for c in (dec, e2e, fmt) if c is not None)
    if held["psnr"] >= min_psnr and not non_finite:
        return None
    dec_bad = dec is not None and (dec["psnr"] < min_psnr or dec["non_finite"] > 0)
    fault = "decoder" if dec_bad or e2e is None else "fmt"
    msg = ("%s: fp16 precision check failed - the first %d frames are %.1f dB from the fp32 verification mode of the same "
           "kernels (limit %.1f dB; %.2f %% of the samples beyond 2/255, max %.3f, %d non-finite) with nothing out of fp16's "
           "range. At fault: %s%s. The frames are NOT the reference's within the stated tolerance: run this checkpoint with %s."
           % (where, held["segments"], held["psnr"], min_psnr, held["pct_beyond"], held["max"], non_finite, fault,
              "" if dec is None or e2e is None else " (decoder alone %.1f dB%s)" % (
                  dec["psnr"], ", FMT latents rel-L2 %.2e" % fmt["rel_l2"] if fmt is not None else ""),
              "dtype fp32 for the decoder and encoder (FLOAT_AMD_DEC_DTYPE=fp32)" if fault == "decoder"
              else "dtype fp32 for the FMT (FLOAT_AMD_FMT_DTYPE=fp32)"))
    if action == "raise":
        raise Fp16PrecisionError(msg)
    logging.getLogger("float_amd").error(msg)
    warnings.warn(msg, RuntimeWarning, stacklevel=3)
    return fault


def _rows(r_d, frame_range=None):
    """The (T, dim_w) latent rows of one clip from r_d (1, T, dim_w) or (T, dim_w); frame_range=(t0, t1): that shard of them."""
    rd = r_d[0] if r_d.dim() == 3 else r_d
    return rd if frame_range is None else rd[frame_range[0]:frame_range[1]]


@torch.no_grad()
def verify_decoder(dec_state, size, s_r, feats, r_d, frames_dev, k, device="cuda:0", style_dim=512, twin=None):
    """The decoder half of the precision guard, callable on its own: decode the first k latents of `r_d` with an fp32 twin
    of the decoder (verification mode, max_frames = k, skip features `feats` = fp32 NCHW through float_dec_set_feats) and
    compare the product's frames `frames_dev[:k]` (device, (T, size, size, 3)) against them with float_cmp_segments.  Only the
    k statistics rows cross to the host.  twin: an fp32 SynthesisHIP that already holds `feats` (kept open); else one is built
    and closed.  Returns {"decoder": cmp_summary, "k", "build_ms", "hbm_bytes"}."""
    import time
    dev = torch.device(device)
    rd = _rows(r_d).to(dev, torch.float32)
    k = max(1, min(int(k), rd.shape[0], frames_dev.shape[0]))
    own = twin is None
    build_ms, hbm = 0.0, 0
    if own:
        torch.cuda.synchronize(dev)
        free0, t0 = torch.cuda.mem_get_info(dev)[0], time.perf_counter()
        twin = SynthesisHIP(dec_state, size, style_dim, dev, "fp32", k)
        twin.set_feats(feats)
        torch.cuda.synchronize(dev)
        build_ms, hbm = (time.perf_counter() - t0) * 1e3, free0 - torch.cuda.mem_get_info(dev)[0]
    try:
        want = twin.decode_latent_into_processed_images(s_r, rd[:k])
        seg = size * size * 3
        rows = native.cmp_segments(frames_dev[:k].reshape(-1), want.reshape(-1), seg, VERIFY_THR).cpu()
    finally:
        if own:
            twin.close()
    return dict(decoder=cmp_summary(rows.tolist(), seg), k=k, build_ms=build_ms, hbm_bytes=int(hbm))


def _frame_dtype(dtype):
    """The two frame formats the decoder hands over: fp32 in [0,1], or uint8 quantised on the device."""
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError("frames leave the decoder as torch.float32 or torch.uint8 (got %r)" % (dtype,))
    return dtype


def _resolve_out_dtype(out, out_dtype):
    """The frame format of a hand-over call: a caller-supplied `out` fixes it, `out_dtype` alone selects it (default fp32), and
    the two must not contradict each other."""
    if out is not None:
        if out_dtype is not None and out_dtype != out.dtype:
            raise ValueError("out is %s but out_dtype asks for %s" % (out.dtype, out_dtype))
        return _frame_dtype(out.dtype)
    return _frame_dtype(torch.float32 if out_dtype is None else out_dtype)


def resolve_out_format(out, out_dtype, out_format, matrix=None):
    """(dtype, format) of a hand-over call.  out_format: None | "rgb" ((T, R, R, 3) frames, fp32 or uint8 as _resolve_out_dtype
    decides) | "i420" ((T, 3R/2, R) uint8 planar YUV 4:2:0, host_models.rgb8_to_i420).  "i420" implies uint8: with
    out_dtype=torch.float32 or an fp32 `out` it is a ValueError.  A caller-supplied `out` fixes the format by its dimensions (a
    3-d uint8 tensor is I420), and a stated format that contradicts it is a ValueError.  matrix: the colour matrix of I420 frames
    (host_models.yuv_matrix_id); with RGB frames, fp32 or uint8, anything but None is a ValueError, as is an unknown name."""
    if out_format == "i420" and out is None and out_dtype is None:
        out_dtype = torch.uint8
    dtype = _resolve_out_dtype(out, out_dtype)
    fmt = infer_out_format(out, out_format, dtype)
    if out is not None and out.dim() != (3 if fmt == "i420" else 4):
        raise ValueError("out has %d dimensions, out_format %r takes %s" % (out.dim(), fmt, "(T, 3R/2, R)" if fmt == "i420" else "(T, R, R, 3)"))
    host_models.yuv_matrix_for("out_format", matrix, fmt if fmt == "i420" else "%s RGB" % (dtype,), 0, 0)
    return dtype, fmt


class FrameBlock(collections.namedtuple("FrameBlock", "first last frames")):
    """One FMT window of a streamed clip (FloatHotPath.stream_to_host): frames [first, last) of the clip, `frames` a view of
    a pinned ring slot - (last - first, H, W, 3), or (last - first, 3H/2, W) for I420 - complete when the block is yielded and
    OVERWRITTEN after the generator has been advanced again: copy it to keep it."""
    __slots__ = ()


class JpegBlock(collections.namedtuple("JpegBlock", "first last frames")):
    """One FMT window of a clip streamed as JPEG files (FloatHotPath.stream_to_jpeg): frames [first, last) of the clip, `frames` a
    jpeg.JpegFrames over a pinned ring slot - complete when the block is yielded and OVERWRITTEN after the generator has been
    advanced again: write it out or copy it (`bytes(blk.frames[i])`) to keep it."""
    __slots__ = ()


class PngBlock(collections.namedtuple("PngBlock", "first last frames")):
    """One FMT window of a clip streamed as PNG files (FloatHotPath.stream_to_png): frames [first, last) of the clip, `frames` a
    png.PngFrames over a pinned ring slot - complete when the block is yielded and OVERWRITTEN after the generator has been
    advanced again: write it out or copy it (`bytes(blk.frames[i])`) to keep it."""
    __slots__ = ()


class Placement(collections.namedtuple("Placement", "src8 rect")):
    """Where the generated frames belong in the user's portrait (InferenceAgent.host_inputs_placed): `src8` the (H, W, 3) uint8
    portrait on the device (image.source_rgb8_device), `rect` = (x0, y0, w, h) the box of the crop in its coordinates - it may
    reach outside the image.  What the *_pasted producers and the `place` argument of the JPEG producers take."""
    __slots__ = ()

    @property
    def size(self):
        """(H, W) of the pasted frames"""
        return int(self.src8.shape[0]), int(self.src8.shape[1])


def _check_place(what, place, device):
    s = getattr(place, "src8", None)
    if not isinstance(place, Placement) or not isinstance(s, torch.Tensor) or s.dtype != torch.uint8 or s.dim() != 3 or s.shape[-1] != 3 \
            or s.device != device or not s.is_contiguous() or len(place.rect) != 4:
        raise ValueError("%s: place must be a Placement of a contiguous (H, W, 3) uint8 portrait on %s and a rect (x0, y0, w, h)"
                         % (what, device))
    return place


def _check_resample(what, resample, place):
    """`resample` of a pasted producer: None or a filter of host_models.RESAMPLE_FILTERS, and only where something is pasted"""
    if resample is not None:
        host_models.resample_filter_id(what, resample)
        if place is None:
            raise ValueError("%s: resample=%r needs a place (the crops are not resized unless they are pasted back)" % (what, resample))
    return resample


def _paste_scratch(hot, place, n, resample):
    """the scratch of pasting up to n crops with `resample`, owned by the caller beside its crops (None: nothing to resample)"""
    return image.paste_scratch(place.size, (hot.size, hot.size), place.rect, n, resample, hot.device) if place is not None else None


class _FrameSink:
    """What FloatHotPath._ring does per slot for stream_to_host: a slot is a pinned (L,) + frame_shape buffer, and the one device
    staging buffer is shared by all of them (safe in stream order)."""
    name = "stream_to_host"

    def __init__(self, hot, out_dtype, out_format, matrix=None):
        self.hot, self.dtype, self.fmt = hot, out_dtype, out_format
        self.matrix = hot.yuv_matrix(self.name, matrix, out_format)  # None for RGB frames

    def open(self, slots):
        shape = (self.hot.cfg.num_frames_for_clip,) + self.hot.dec.frame_shape(self.fmt)
        ring = [torch.empty(shape, dtype=self.dtype, pin_memory=True) for _ in range(slots)]
        self.staging = torch.empty(shape, device=self.hot.device, dtype=self.dtype)
        return ring

    def enqueue(self, slot, s_r_d, rows):
        n = rows.shape[0]
        self.hot.dec.decode_into_host(s_r_d, rows, slot[:n], self.staging[:n], out_format=self.fmt, matrix=self.matrix)

    def block(self, slot, f0, f1, ev, st):
        return FrameBlock(f0, f1, slot[:f1 - f0])


class _PasteSink:
    """What FloatHotPath._ring does per slot for stream_to_host_pasted: a slot is a pinned (L,) + frame_shape uint8 buffer of pasted
    frames - (H, W, 3), or (3H/2, W) with out_format="i420" - and the device buffers of L 8-bit crops and of L pasted frames are
    shared by all of them (safe in stream order).  generate_pasted runs its groups through the same three steps (`paste`).  The
    format and, for I420, the portrait's even sides are checked when the sink is made: at the call."""
    name = "stream_to_host_pasted"

    def __init__(self, hot, place, feather, out_format=None, name=None, matrix=None, resample=None):
        self.hot, self.place, self.feather = hot, place, feather
        self.name = name or self.name
        self.resample = _check_resample(self.name, resample, place)
        self.fmt = image.paste_format(self.name, out_format)
        H, W = place.size  # "auto" goes by the size of the frames that leave: the portrait's
        self.matrix = host_models.yuv_matrix_for(self.name, matrix, self.fmt, W, H) if matrix is not None else None
        if self.fmt == "i420":
            image.require_even_sides(self.name, *place.size)
        self.frame_shape = image.pasted_frame_shape(*place.size, self.fmt)

    def device_buffers(self, n):
        """the shared device buffers of n 8-bit crops and of n pasted frames"""
        dev, R = self.hot.device, self.hot.size
        self.crops = torch.empty(n, R, R, 3, dtype=torch.uint8, device=dev)
        self.pasted = torch.empty((n,) + self.frame_shape, dtype=torch.uint8, device=dev)
        self.scratch = _paste_scratch(self.hot, self.place, n, self.resample)

    def open(self, slots):
        L = self.hot.cfg.num_frames_for_clip
        ring = [torch.empty((L,) + self.frame_shape, dtype=torch.uint8, pin_memory=True) for _ in range(slots)]
        self.device_buffers(L)
        return ring

    def paste(self, host, s_r_d, rows):
        """decode_u8, the paste (and, for I420, the colour conversion in the same kernel), one non-blocking copy into `host`"""
        n = rows.shape[0]
        self.hot.dec.decode_u8(s_r_d, rows, out=self.crops[:n])
        image.paste_frames_device(self.place.src8, self.crops[:n], self.place.rect, self.feather, out=self.pasted[:n], out_format=self.fmt,
                                  matrix=self.matrix, resample=self.resample, scratch=self.scratch)
        host.copy_(self.pasted[:n], non_blocking=True)

    def enqueue(self, slot, s_r_d, rows):
        self.paste(slot[:rows.shape[0]], s_r_d, rows)

    def block(self, slot, f0, f1, ev, st):
        return FrameBlock(f0, f1, slot[:f1 - f0])


class _JpegSink:
    """What FloatHotPath._ring does per slot for stream_to_jpeg: a slot holds the 8-bit frames of a window on the device, the
    files and their offsets on both sides; the copy stream and the encoder's scratch are shared.  With `place` the slot's frames
    are the pasted H x W ones, and the window's 8-bit crops go through one shared device buffer."""
    name = "stream_to_jpeg"

    def __init__(self, hot, quality, restart, place=None, feather=None, pad=None, resample=None):
        self.hot, self.quality, self.restart, self.place, self.feather, self.pad = hot, quality, restart, place, feather, pad
        self.resample = _check_resample(self.name, resample, place)

    def open(self, slots):
        dev, L, R = self.hot.device, self.hot.cfg.num_frames_for_clip, self.hot.size
        H, W = self.place.size if self.place is not None else (R, R)
        cap = jpeg.default_capacity(L, H, W)
        ring = [dict(u8=torch.empty(L, H, W, 3, dtype=torch.uint8, device=dev), data=torch.empty(cap, dtype=torch.uint8, device=dev),
                     off=torch.empty(L + 1, dtype=torch.int64, device=dev), host=torch.empty(cap, dtype=torch.uint8, pin_memory=True),
                     off_host=torch.empty(L + 1, dtype=torch.int64, pin_memory=True)) for _ in range(slots)]
        self.s_copy, self.work = torch.cuda.Stream(dev), None
        self.crops = torch.empty(L, R, R, 3, dtype=torch.uint8, device=dev) if self.place is not None else None
        self.scratch = _paste_scratch(self.hot, self.place, L, self.resample)
        return ring

    def _encode(self, slot, n):
        self.work = jpeg.enqueue_encode(slot["u8"][:n], self.quality, self.restart, slot["data"], slot["off"][:n + 1], self.work,
                                         self.pad)

    def enqueue(self, slot, s_r_d, rows):
        n = rows.shape[0]
        if self.place is None:
            self.hot.dec.decode_u8(s_r_d, rows, out=slot["u8"][:n])
        else:
            self.hot.dec.decode_u8(s_r_d, rows, out=self.crops[:n])
            image.paste_frames_device(self.place.src8, self.crops[:n], self.place.rect, self.feather, out=slot["u8"][:n],
                                      resample=self.resample, scratch=self.scratch)
        self._encode(slot, n)
        slot["off_host"][:n + 1].copy_(slot["off"][:n + 1], non_blocking=True)

    def block(self, slot, f0, f1, ev, st):
        n = f1 - f0
        edges = slot["off_host"][:n + 1]
        total = int(edges[-1])
        if total > slot["data"].numel():  # the files did not fit: once more, with room (behind the windows already enqueued)
            with torch.cuda.stream(st):
                slot["data"] = torch.empty(total, dtype=torch.uint8, device=self.hot.device)
                slot["host"] = torch.empty(total, dtype=torch.uint8, pin_memory=True)
                self._encode(slot, n)
            st.synchronize()
        self.s_copy.wait_event(ev)
        return JpegBlock(f0, f1, jpeg.to_host(slot["data"], edges.clone(), slot["host"], self.s_copy))


class _PngSink(_JpegSink):
    """What FloatHotPath._ring does per slot for stream_to_png: _JpegSink's slots with room for the frames' raw size, and the
    files' CRCs beside the offsets on both sides."""
    name = "stream_to_png"

    def __init__(self, hot, band, place=None, feather=None, resample=None):
        self.hot, self.band, self.place, self.feather = hot, band, place, feather
        self.resample = _check_resample(self.name, resample, place)

    def open(self, slots):
        dev, L, R = self.hot.device, self.hot.cfg.num_frames_for_clip, self.hot.size
        H, W = self.place.size if self.place is not None else (R, R)
        cap = png.default_capacity(L, H, W)
        ring = [dict(u8=torch.empty(L, H, W, 3, dtype=torch.uint8, device=dev), data=torch.empty(cap, dtype=torch.uint8, device=dev),
                     off=torch.empty(L + 1, dtype=torch.int64, device=dev), host=torch.empty(cap, dtype=torch.uint8, pin_memory=True),
                     off_host=torch.empty(L + 1, dtype=torch.int64, pin_memory=True), crc=torch.empty(L, dtype=torch.int32, device=dev),
                     crc_host=torch.empty(L, dtype=torch.int32, pin_memory=True)) for _ in range(slots)]
        self.s_copy, self.work = torch.cuda.Stream(dev), None
        self.crops = torch.empty(L, R, R, 3, dtype=torch.uint8, device=dev) if self.place is not None else None
        self.scratch = _paste_scratch(self.hot, self.place, L, self.resample)
        return ring

    def _encode(self, slot, n):
        self.work = png.enqueue_encode(slot["u8"][:n], self.band, slot["data"], slot["off"][:n + 1], slot["crc"][:n], self.work)
        slot["crc_host"][:n].copy_(slot["crc"][:n], non_blocking=True)

    def block(self, slot, f0, f1, ev, st):
        n = f1 - f0
        edges = slot["off_host"][:n + 1]
        total = int(edges[-1])
        if total > slot["data"].numel():  # the files did not fit: once more, with room (behind the windows already enqueued)
            with torch.cuda.stream(st):
                slot["data"] = torch.empty(total, dtype=torch.uint8, device=self.hot.device)
                slot["host"] = torch.empty(total, dtype=torch.uint8, pin_memory=True)
                self._encode(slot, n)
            st.synchronize()
        self.s_copy.wait_event(ev)
        return PngBlock(f0, f1, png.to_host(slot["data"], edges.clone(), slot["crc_host"][:n].clone(), slot["host"], self.s_copy))


class FloatHotPath:
    def __init__(self, fmt_state, dec_state, cfg: FmtConfig = None, device="cuda:0", size=512, fmt_dtype="fp16",
                 dec_dtype="fp16", max_frames=32, use_graph=2, max_batch=1):
        self.cfg = cfg or FmtConfig()
        self.device = torch.device(device)
        self.size = size
        self._fmt_state, self._dec_state, self._use_graph = fmt_state, dec_state, use_graph
        self.fmt = FlowMatchingTransformerHIP(fmt_state, self.cfg, device, fmt_dtype, use_graph, max_batch)
        self.dec = SynthesisHIP(dec_state, size, self.cfg.dim_w, device, dec_dtype, max_frames)
        self._fmt_batched = {}     # {max_batch: FMT handle for stacked clips} (batched_fmt; at most one)
        self._staging = {}         # {(shape, dtype, format): device frame buffer of the hand-over} (staging; at most one)
        self._host_inflight = []   # [(pinned host tensor, event)] of hand-overs that may still be storing (_hold_inflight)
        self._ov_streams = {}      # {mode: (chain stream, decoder stream)} (_overlap_streams)
        self._open_stream = None   # description of the stream_to_host generator open on this object (require_no_stream)
        self._last_job = None      # the WindowSampler of the last windowed job: keeps its tensors alive (_windows)

    def n_chunks(self, T):
        return int(math.ceil(T / self.cfg.num_frames_for_clip))

    def require_no_stream(self, what):
        """One FMT handle carries one job, and the decoder holds one clip's skip features: while a stream_to_host generator is
        open on this object every other producer is refused."""
        if self._open_stream:
            raise RuntimeError("%s: %s is still open on this FloatHotPath - exhaust it or close() it first" % (what, self._open_stream))

    def batched_fmt(self, n_clips):
        """An FMT handle whose workspace holds `n_clips` stacked clips (float_fmt_sample_batch), built on first use from the
        same weights and cached: the default handle is sized for ONE clip (3.1 GB of workspace per clip).  Up to
        FLOAT_AMD_FMT_MAX_BATCH (default 16, the operator's limit: 50 GB of workspace of the 288) clips per chain; larger
        batches run in chunks of that size.  Per clip the chain costs 79 / 52 / 36 / 28 / 24 ms at 1 / 2 / 4 / 8 / 16 clips."""
        cap = max(1, min(16, int(os.environ.get("FLOAT_AMD_FMT_MAX_BATCH", "16"))))
        mb = min(cap, max(1, int(n_clips)))
        if mb > self.fmt.max_batch and mb not in self._fmt_batched:
            # 3.1 GB of workspace per stacked clip + the weights once more: size the handle for what the device has free (another
            # model resident in ComfyUI, a smaller GPU) instead of failing with out-of-memory inside the create call
            free, _ = torch.cuda.mem_get_info(self.device)
            fit = int((free - (2 << 30)) // int(3.3 * 2**30))
            if fit < mb:
                logging.getLogger("float_amd").warning("batched FMT handle: %.1f GB of HBM free, stacking %d clips per chain instead of %d",
                                                       free / 2**30, max(1, fit), mb)
                mb = max(1, fit)
        if mb <= self.fmt.max_batch:
            return self.fmt
        cache = self._fmt_batched
        if mb not in cache:
            for k in list(cache):
                cache.pop(k).close()
            cache[mb] = FlowMatchingTransformerHIP(self._fmt_state, self.cfg, self.device, self.fmt.dtype, self._use_graph, mb)
            cache[mb].set_method(getattr(self.fmt, "method", "euler"))
        return cache[mb]

    def range_counts(self, reset=True):
        """{operator: float_*_saturation total} of this object's 16-bit handles (synchronises the current stream)."""
        out = {}
        if self.fmt.dtype == "fp16":
            out["fmt"] = self.fmt.saturation(reset) + sum(f.saturation(reset) for f in self._fmt_batched.values())
        if self.dec.dtype == "fp16":
            out["decoder"] = self.dec.saturation(reset)
        return out

    @torch.no_grad()
    def verify_precision(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale, noise, r_d, frames_dev, k,
                         keep_twins=False):
        """The fp16 precision guard for one clip (B = 1) that this object has just produced: `r_d` (1, T, dim_w) and
        `frames_dev` (T, size, size, 3), both on the device.  Builds fp32 twins (verification mode: the same kernels with
        4-byte operands, held to the reference at 1e-4) of the FMT (eager launches, max_batch 1) and of the decoder
        (max_frames = k), samples WINDOW 0 ONLY in fp32 from the same conditions and the same noise, decodes the first k frames
        twice with the fp32 decoder - from the product's latents and from the fp32 latents - and compares on the device
        (float_cmp_segments; only the statistics rows are pulled to the host):
          fmt         product r_d[:n] against fp32 r_d[:n], n = min(T, n_cur) (attribution and the log line);
          decoder     product frames [0, k) against fp32-decoder frames of the PRODUCT's latents (decoder + skip features);
          end_to_end  product frames [0, k) against the all-fp32 frames: the one report_precision holds to the threshold.
        feats: the fp32 NCHW skip features (from an fp32 encoder).  wa / we are the product's on both sides: the audio
        operators are not covered.  k is clipped to n.  The twins are closed before returning unless keep_twins (then they are
        returned under "twins" and the caller closes them).  Also in the result: k, n, build_ms and hbm_bytes of the twins, ms
        of the whole check."""
        import time
        dev, c = self.device, self.cfg
        t_all = time.perf_counter()
        rd16 = _rows(r_d).to(dev, torch.float32)
        T = rd16.shape[0]
        n = min(T, c.num_frames_for_clip)
        k = max(1, min(int(k), n, frames_dev.shape[0]))
        torch.cuda.synchronize(dev)
        free0, t0 = torch.cuda.mem_get_info(dev)[0], time.perf_counter()
        fmt32 = FlowMatchingTransformerHIP(self._fmt_state, c, dev, "fp32", 0, 1)
        dec32 = None
        try:
            fmt32.set_method(getattr(self.fmt, "method", "euler"))
            dec32 = SynthesisHIP(self._dec_state, self.size, c.dim_w, dev, "fp32", k)
            dec32.set_feats(feats)
            torch.cuda.synchronize(dev)
            build_ms, hbm = (time.perf_counter() - t0) * 1e3, free0 - torch.cuda.mem_get_info(dev)[0]
            wa0 = wa.to(dev, torch.float32)[:, :n]
            we0 = we.to(dev, torch.float32)
            we0 = we0[:, :n] if we0.shape[1] > 1 else we0
            rd32 = fmt32.sample(r_s, wa0, we0, noise.to(dev, torch.float32)[:1], nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale)[0]
            seg = self.size * self.size * 3
            got = frames_dev[:k].reshape(-1)
            rows = [native.cmp_segments(rd16[:n].reshape(-1), rd32.reshape(-1), n * c.dim_w, VERIFY_THR),
                    native.cmp_segments(got, dec32.decode_latent_into_processed_images(s_r, rd16[:k]).reshape(-1), seg, VERIFY_THR),
                    native.cmp_segments(got, dec32.decode_latent_into_processed_images(s_r, rd32[:k]).reshape(-1), seg, VERIFY_THR)]
            rows = torch.cat(rows).cpu().tolist()  # the one hand-over: (1 + 2 k) x 5 doubles
        except BaseException:
            keep_twins = False
            raise
        finally:
            if not keep_twins:
                fmt32.close()
                if dec32 is not None:
                    dec32.close()
        out = dict(fmt=cmp_summary(rows[:1], n * c.dim_w), decoder=cmp_summary(rows[1:1 + k], seg),
                   end_to_end=cmp_summary(rows[1 + k:], seg), k=k, n=n, build_ms=build_ms, hbm_bytes=int(hbm),
                   ms=(time.perf_counter() - t_all) * 1e3)
        if keep_twins:
            out["twins"] = (fmt32, dec32)
        return out

    @torch.no_grad()
    def sample(self, r_s, wa, we, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15, noise=None,
               include_r_cfg=False):
        """r_d (B,T,512).  `noise` (n_chunks,B,50,512) overrides the seeded CPU-generator draw."""
        self.require_no_stream("sample")
        if noise is None:
            noise = draw_noise(self.n_chunks(wa.shape[1]), wa.shape[0], self.cfg, seed)
        return self.fmt.sample(r_s, wa, we, noise, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale, include_r_cfg)

    @torch.no_grad()
    def decode(self, s_r, feats, r_d, frame_range=None):
        """(T,H,W,3) fp32 in [0,1] on the GPU for batch item 0; frame_range=(t0,t1) decodes a shard."""
        self.require_no_stream("decode")
        if feats is not None:
            self.dec.set_feats(feats)
        return self.dec.decode_latent_into_processed_images(s_r, _rows(r_d, frame_range))

    def yuv_matrix(self, what, matrix, out_format):
        """The id of a `matrix` keyword for frames of the model's size (host_models.yuv_matrix_for: "auto" goes by that size; a
        matrix with RGB frames is a ValueError); None stays None, which every layer below reads as BT.601 limited range."""
        return None if matrix is None else host_models.yuv_matrix_for(what, matrix, out_format, self.size, self.size)

    def staging(self, n_frames, dtype=torch.float32, out_format="rgb"):
        """Device-side frame buffer of float_dec_frames_host[_u8|_i420], cached per clip length, dtype and format (786 MB for 250
        fp32 frames at 512 px, 197 MB as uint8, 98 MB as I420; sized for 288 GB).  The host side is NOT cached: callers get a fresh pinned tensor (torch's caching host allocator
        hands the block of a released earlier result back without a new hipHostMalloc), because ComfyUI keeps node outputs
        alive across executions and a re-used buffer would silently overwrite them."""
        cache = self._staging
        shape = (n_frames,) + self.dec.frame_shape(out_format)
        if (shape, dtype, out_format) not in cache:
            cache.clear()  # one clip length and format at a time
            cache[(shape, dtype, out_format)] = torch.empty(shape, device=self.device, dtype=_frame_dtype(dtype))
        return cache[(shape, dtype, out_format)]

    @torch.no_grad()
    def decode_to_host(self, s_r, r_d, feats=None, frame_range=None, out=None, out_dtype=None, out_format=None, matrix=None):
        """Frames of one clip (r_d (T,512)) into pinned host memory through float_dec_frames_host: the frames of batch i cross
        PCIe inside the launches of batch i+1.  Returns the host tensor (T,H,W,3); it is complete once the current stream has
        been synchronised (the callers that hand it to the user do that).  out_dtype: torch.float32 (default) or torch.uint8
        (8-bit frames quantised on the device, a quarter of the bytes); a caller-supplied `out` fixes the dtype, and an
        out_dtype that contradicts it is a ValueError.  out_format="i420": (T, 3H/2, W) uint8 planar YUV 4:2:0, converted on the
        device (half the bytes of uint8 RGB; resolve_out_format has the rules).  matrix: the colour matrix of I420 frames, as
        host_models.yuv_matrix_id reads it (None = BT.601 limited range; "auto" by the model's size); a ValueError with RGB frames."""
        out_dtype, out_format = resolve_out_format(out, out_dtype, out_format, matrix)
        matrix = self.yuv_matrix("decode_to_host", matrix, out_format)
        self.require_no_stream("decode_to_host")
        if feats is not None:
            self.dec.set_feats(feats)
        rd = _rows(r_d, frame_range)
        n = rd.shape[0]
        self._prune_inflight()
        if out is None:
            out = torch.empty((n,) + self.dec.frame_shape(out_format), dtype=out_dtype, pin_memory=True)
        # (the frames by hipMemcpyAsync on a second stream instead of copy workgroups inside the next batch's launches: 121.4-122.1 vs
        # 105.7-106.8 ms per clip on the round-6 kernels, as in round 3 - decoder.decode_into_host(copy_stream=) keeps the form)
        self.dec.decode_into_host(s_r, rd, out, self.staging(n, out_dtype, out_format), out_format=out_format, matrix=matrix)
        self._hold_inflight(out, torch.cuda.current_stream(self.device))
        return out

    def _hold_inflight(self, host, stream):
        """The copy workgroups / hipMemcpyAsync of a hand-over may still be writing its host tensor when the call returns, and
        torch's caching host allocator knows nothing about writes it did not issue: this object keeps a reference to that tensor
        until an event recorded on `stream` behind them has completed, so the block cannot be handed out again (e.g. as the
        next call's `out`) while the GPU stores into it.  No host wait: a batch of clips queues its decodes back to back; the
        device-side staging buffer is shared, which is safe in stream order."""
        ev = torch.cuda.Event()
        ev.record(stream)
        self._host_inflight.append((host, ev))

    def _prune_inflight(self):
        """Entries leave the list once their event has completed (query, not synchronize)."""
        self._host_inflight[:] = [(t, e) for t, e in self._host_inflight if not e.query()]

    def release_host_inflight(self):
        """Drop the references decode_to_host keeps on host tensors whose copies have completed (call after the stream has been
        synchronised: a batch of 16 clips would otherwise pin 12.6 GB here until the next decode)."""
        self._prune_inflight()

    @torch.no_grad()
    def generate_to_host(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15,
                         noise=None, frame_range=None, out=None, return_rd=False, out_dtype=None, out_format=None, matrix=None):
        """The product's hot path for one clip (B = 1): conditioning tensors in HBM -> frames in pinned host memory, the
        reference's destination (FLOAT.py:139,157-167).  This is what InferenceAgent.run_inference, FloatProcess and bench.py run.
        out_dtype, out_format, matrix: as in decode_to_host (torch.uint8 = 8-bit frames, "i420" = planar YUV 4:2:0)."""
        out_dtype, out_format = resolve_out_format(out, out_dtype, out_format, matrix)
        self.require_no_stream("generate_to_host")
        if feats is not None:
            self.dec.set_feats(feats)
        r_d = self.sample(r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale, seed, noise)  # noise=None: drawn there from `seed`
        host = self.decode_to_host(s_r, r_d, None, frame_range, out, out_dtype, out_format, matrix)
        return (host, r_d) if return_rd else host

    def stream_to_host(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15,
                       noise=None, out_dtype=None, out_format=None, slots=3, matrix=None):
        """generate_to_host for one clip (B = 1) as a generator: one FrameBlock(first, last, frames) per FMT window, in frame
        order, the same bytes as the whole-clip call (same kernels on the same operands; decode batching does not change a
        frame).  `frames` is a view of one of `slots` pinned ring buffers and is complete when it is yielded: the generator has
        waited on that block's own event, never on the whole stream.

        Everything runs on the stream that is current at the first next(): sample(k), decode(k) into the slot of block k,
        event(k), sample(k + 1), ...  Window k + 1 (and further windows, as far as free slots allow) is enqueued BEFORE the wait
        for event(k), so the device works while the consumer holds block k.

        Lifetime: the slot of block k belongs to the consumer from the yield of block k until the generator is advanced
        again.  After that it is OVERWRITTEN by block k + slots - a consumer that wants to keep a block copies it
        (`blk.frames.clone()`).  Work that writes a slot is enqueued only after the consumer has given that slot back.

        Memory: `slots` pinned buffers and ONE device staging buffer of num_frames_for_clip frames each, allocated once and kept
        on the generator (the whole-clip staging() cache is not touched) - slots x 50 frames whatever T is, where
        generate_to_host holds T frames on both sides.  The latents, conditions and noise still grow with T (about 6 KB per
        frame against 786 KB for an fp32 frame at 512 px).  The last block may be short: it is a prefix view of its slot.
        The buffers are allocated inside the first next() of every stream: where the host allocator has no cached block of that
        size (the first stream of a process, or of a format) the pinned allocation - 472 MB for fp32 at 512 px and 3 slots - is
        part of the time to the first block; later streams get the cached blocks back.

        matrix: the colour matrix of I420 frames, as in decode_to_host.
        slots >= 2, B = 1 and the resolve_out_format rules are checked here, at the call (ValueError); nothing is enqueued before the
        first next().  While the generator is open (first next() until exhaustion, close(), garbage collection or an exception
        thrown into it) sample, decode*, generate* and a second stream on this object raise RuntimeError.  Leaving early waits
        for the work already enqueued, drops the slots and clears that flag.  The FMT handle's unfinished job needs no abort
        call: float_fmt_sample_begin overwrites every field of the handle's job record, the first window of a job re-stages the
        time table and the history rows of the workspace, and the only call that reads an unfinished job is
        float_fmt_sample_next, which is reachable only through the WindowSampler this generator drops - so the next sample /
        sample_begin starts clean."""
        sink = _FrameSink(self, *resolve_out_format(None, out_dtype, out_format, matrix), matrix=matrix)
        self._check_stream_call(sink.name, slots, wa)
        return self._ring(sink, (r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale), s_r, feats, seed, noise, int(slots))

    def stream_to_host_pasted(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15,
                              noise=None, place=None, feather=None, slots=3, out_format=None, matrix=None, resample=None):
        """stream_to_host(out_dtype=torch.uint8) with every frame pasted back into the portrait on the device: a generator of
        FrameBlock(first, last, frames), `frames` a (last - first, H, W, 3) uint8 view of a pinned ring slot, bitwise
        host_models.paste_rgb8(place.src8, the window's 8-bit crops, place.rect, feather).  place: a Placement (the portrait on
        this device and the box); feather: source pixels, None = rect_w // 16 (host_models.default_feather).  Per window:
        the chain, decode_u8 into a shared device buffer of 50 crops, float_img_paste into a shared device buffer of 50 pasted
        frames, one non-blocking copy into the slot.  The ring rules, lifetime and early exit are stream_to_host's; pinned memory
        is slots x 50 x H x W x 3 bytes (940 MB at 1920 x 1088 and 3 slots).
        out_format="i420" (default None = "rgb": the above): `frames` is a (last - first, 3H/2, W) uint8 view, bitwise
        host_models.paste_i420 of the same operands; float_img_paste_i420 pastes and converts in one kernel, and the device buffer
        of pasted frames, the pinned slots and the copy are 3HW/2 bytes per frame - half of the above.  H and W must be even:
        a ValueError here, at the call.  matrix: the colour matrix of I420 frames (host_models.yuv_matrix_id; "auto" goes by the
        portrait's size); with RGB frames anything but None is a ValueError, also at the call.
        resample (default None: the above): "bicubic" | "lanczos" - the face is Pillow's resize of the crop with that filter
        (float_img_resample in front of the paste: image.paste_frames_device), bitwise host_models.paste_rgb8 / paste_i420(...,
        resample=resample); its tables are uploaded once and its scratch sits beside the two shared buffers."""
        place = _check_place("stream_to_host_pasted", place, self.device)
        sink = _PasteSink(self, place, feather, out_format, matrix=matrix, resample=resample)
        self._check_stream_call(sink.name, slots, wa)
        return self._ring(sink, (r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale), s_r, feats, seed, noise, int(slots))

    @torch.no_grad()
    def generate_pasted(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15, noise=None,
                        place=None, feather=None, out=None, return_rd=False, out_format=None, matrix=None, resample=None):
        """generate_to_host(out_dtype=torch.uint8) with every frame pasted back into the portrait on the device: the chain of the
        whole clip, then per group of num_frames_for_clip frames decode_u8, float_img_paste and one non-blocking copy into the
        pinned (T, H, W, 3) uint8 result - device memory stays at 50 crops and 50 pasted frames whatever T is.  The result is
        complete once the current stream has been synchronised (the callers that hand it to the user do that).
        out_format="i420" (default None = "rgb": the above): the result is (T, 3H/2, W) uint8 planar YUV 4:2:0, bitwise
        host_models.paste_i420; float_img_paste_i420 pastes and converts in one kernel, and the device buffer of pasted frames, the
        result and the copies are 3HW/2 bytes per frame.  H and W must be even - a ValueError before anything is enqueued - and
        an `out` of another shape than the format's is a ValueError.  matrix, resample: as in stream_to_host_pasted."""
        place = _check_place("generate_pasted", place, self.device)
        sink = _PasteSink(self, place, feather, out_format, name="generate_pasted", matrix=matrix, resample=resample)
        self.require_no_stream("generate_pasted")
        if feats is not None:
            self.dec.set_feats(feats)
        r_d = self.sample(r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale, seed, noise)
        rd = _rows(r_d)
        T, L = rd.shape[0], self.cfg.num_frames_for_clip
        shape = (T,) + sink.frame_shape
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.is_cuda or not out.is_contiguous():
            raise ValueError("generate_pasted: out must be a contiguous CPU uint8 tensor of shape %s" % (shape,))
        s_r_d = s_r.to(self.device, torch.float32).reshape(-1).contiguous()
        with torch.cuda.device(self.device):
            sink.device_buffers(min(T, L))
            for f0 in range(0, T, L):
                sink.paste(out[f0:f0 + min(L, T - f0)], s_r_d, rd[f0:f0 + L])
        return (out, r_d) if return_rd else out

    def _check_stream_call(self, what, slots, wa):
        """What every stream refuses at the call, before its generator exists (a generator's body runs at the first next())."""
        if int(slots) < 2:
            raise ValueError("%s needs slots >= 2 (one block with the consumer, one in flight), got %r" % (what, slots))
        if wa.dim() != 3 or wa.shape[0] != 1:
            raise ValueError("%s streams one clip (B = 1): wa must be (1, T, dim_a), got %s" % (what, tuple(wa.shape)))
        self.require_no_stream(what)

    def _windows(self, job, s_fmt, s_dec, frame_range=None):
        """The window pipeline of every windowed producer.  job = (r_s, wa, we, noise, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale)
        goes to a WindowSampler built on the chain stream `s_fmt`; each next() enqueues one window there and, where the decoder
        stream `s_dec` is another one, an event behind it that `s_dec` waits on, then yields (ws, f0, f1): the caller decodes
        ws.r_d[0, f0:f1] on `s_dec` into its own destination.  It makes `s_dec` current itself: a `with` held across a yield
        would restore a stale stream when an abandoned generator is closed.  frame_range=(t0, t1) clips [f0, f1) to the shard;
        a window outside it is sampled and not yielded.  Keep-alive: the job's tensors are allocated on `s_fmt` and read on
        `s_dec`, so the object holds the job (_last_job) until the next one replaces it or a producer that has waited drops it."""
        two = s_dec != s_fmt
        with torch.cuda.stream(s_fmt):
            ws = self._last_job = WindowSampler(self.fmt, *job)
        while ws.left > 0:
            with torch.cuda.stream(s_fmt):
                _, (f0, f1) = ws.next()
                if two:
                    ev = torch.cuda.Event()
                    ev.record(s_fmt)
            if frame_range is not None:
                f0, f1 = max(f0, frame_range[0]), min(f1, frame_range[1])
                if f0 >= f1:
                    continue
            if two:
                s_dec.wait_event(ev)
            yield ws, f0, f1

    def _ring(self, sink, job, s_r, feats, seed, noise, slots):
        """The bounded ring of every stream.  job = (r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale).  `sink` is what the
        forms differ in (_FrameSink, _JpegSink): open(slots) makes the slots and the per-stream scratch, inside the first next();
        enqueue(slot, s_r_d, rows) enqueues the work of one window on the stream; block(slot, first, last, event, stream) turns a
        slot whose event has been waited on into the block that is yielded."""
        self.require_no_stream(sink.name)  # another stream may have been started since the call
        T = job[1].shape[1]
        self._open_stream = "%s (%d frames, %d slots)" % (sink.name, T, slots)
        pending = collections.deque()  # (first, last, slot, event) of the blocks enqueued and not yet yielded
        ring = wins = slot = None
        try:
            st = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(st):
                if feats is not None:
                    self.dec.set_feats(feats)
                if noise is None:
                    noise = draw_noise(self.n_chunks(T), 1, self.cfg, seed)
                ring = sink.open(slots)
                s_r_d = s_r.to(self.device, torch.float32).reshape(-1).contiguous()
            wins = self._windows(job[:3] + (noise,) + job[3:], st, st)  # one stream: no events between the stages
            n_win, enqueued = self.n_chunks(T), 0
            for j in range(n_win):
                # block j is about to go to the consumer, who holds nothing now: blocks j .. j + slots - 1 sit in `slots` different
                # slots, and every earlier block has been given back
                with torch.cuda.stream(st):
                    while enqueued < min(n_win, j + slots):
                        ws, f0, f1 = next(wins)
                        sink.enqueue(ring[enqueued % slots], s_r_d, ws.r_d[0, f0:f1])
                        ev = torch.cuda.Event()
                        ev.record(st)
                        pending.append((f0, f1, ring[enqueued % slots], ev))
                        enqueued += 1
                f0, f1, slot, ev = pending.popleft()
                ev.synchronize()
                yield sink.block(slot, f0, f1, ev, st)
        finally:
            # early exit (close(), garbage collection, an exception thrown in or raised above): the work of the blocks still in
            # flight stores into the ring, so it is dropped only after the last of it has run.  Events complete in stream order:
            # the last one covers the others, and the job's tensors with them.
            try:
                if pending:
                    pending[-1][3].synchronize()
            finally:
                pending.clear()
                del ring, wins, sink, slot
                self._last_job = self._open_stream = None

    @torch.no_grad()
    def generate_to_jpeg(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15, noise=None,
                         quality=90, restart=None, return_rd=False, place=None, feather=None, pad=None, resample=None):
        """generate_to_host for one clip (B = 1) with the frames leaving as baseline JPEG files (jpeg.JpegFrames in pinned host
        memory): the chain, decode_u8 of the whole clip, float_jpg_encode on the 8-bit frames in HBM, ONE host read of the
        offsets, then offsets[T] bytes across PCIe - the files, not the frames.  File i is bitwise
        host_models.jpeg_encode_rgb8(frame i of generate_to_host(out_dtype=torch.uint8), quality, restart).  Complete on return
        (the stream has been synchronised).  The 8-bit frames stay on the device: T * size * size * 3 bytes of HBM while it runs.
        place (a Placement; default None: nothing above changes): the 8-bit crops are pasted back into the portrait on the device
        (float_img_paste, `feather` as in generate_pasted) and the encoder codes the H x W frames - file i is jpeg_encode_rgb8 of
        frame i of generate_pasted, and T * H * W * 3 more bytes of HBM are held while it runs.  float_jpg_encode takes sides that
        are multiples of 16: another portrait size is a ValueError here, before anything runs; nothing is padded - unless
        pad="edge" (default None) opts in: float_jpg_encode_padded then takes any portrait size, replicating the last row and column
        into the partial MCUs, and file i is jpeg_encode_rgb8(..., pad="edge") of the same frame (restart=None: ceil(W / 16)).
        resample: as in generate_pasted (with place only)."""
        jpeg.check_pad(pad)
        _check_resample("generate_to_jpeg", resample, place)
        if place is not None:
            place = _check_place("generate_to_jpeg", place, self.device)
            image.require_jpeg_sides("generate_to_jpeg", *place.size, pad=pad)
        self.require_no_stream("generate_to_jpeg")
        if feats is not None:
            self.dec.set_feats(feats)
        r_d = self.sample(r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale, seed, noise)
        with torch.cuda.device(self.device):
            u8 = self.dec.decode_u8(s_r, _rows(r_d))
            if place is not None:
                u8 = image.paste_frames_device(place.src8, u8, place.rect, feather, resample=resample,
                                               scratch=_paste_scratch(self, place, u8.shape[0], resample))
            frames = jpeg.encode_jpeg_host(u8, quality, restart, pad=pad)
        return (frames, r_d) if return_rd else frames

    def stream_to_jpeg(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15, noise=None,
                       quality=90, restart=None, slots=3, place=None, feather=None, pad=None, resample=None):
        """generate_to_jpeg as a generator: one JpegBlock(first, last, frames) per FMT window, in frame order, the same files as the
        whole-clip call.  The contract is stream_to_host's: `frames` (a jpeg.JpegFrames) lives in one of `slots` pinned ring
        buffers, is complete when it is yielded and OVERWRITTEN after the generator has been advanced again (AviMjpegWriter.write
        has handed the bytes on when it returns); window k + 1 and further windows, as far as free slots allow, are enqueued
        before the wait for window k; slots >= 2 and B = 1 are checked at the call (ValueError), nothing is enqueued before the
        first next(); while the generator is open every other producer on this object raises RuntimeError, and leaving early
        waits for the enqueued work and clears that flag.
        Per slot: a device buffer of 50 8-bit frames, a device and a pinned buffer of their I420 size for the files, and the
        offsets on both sides.  Per window the chain, decode_u8, float_jpg_encode and the copy of the 51 offsets are enqueued on
        the current stream; when the block's turn comes the generator waits on that block's event, reads offsets[-1] from pinned
        memory and copies that many bytes on a second stream.  Files beyond the slot's room (noise at quality 100) are encoded
        once more into a larger buffer.
        place, feather: as in generate_to_jpeg - the files are those of the pasted H x W frames, a slot's device buffer holds 50 of
        them and one more buffer of 50 crops is shared; a portrait whose sides are no multiples of 16 is a ValueError at the call,
        unless pad="edge" (as in generate_to_jpeg; the overflow re-encode pads the same way).  resample: as in generate_pasted."""
        jpeg.check_pad(pad)
        _check_resample("stream_to_jpeg", resample, place)
        quality = int(quality)
        if not 1 <= quality <= 100:
            raise ValueError("stream_to_jpeg: quality (%d) must be 1 ... 100" % quality)
        width = self.size
        if place is not None:
            place = _check_place("stream_to_jpeg", place, self.device)
            image.require_jpeg_sides("stream_to_jpeg", *place.size, pad=pad)
            width = place.size[1]
        sink = _JpegSink(self, quality, jpeg.pad_restart(width, pad) if restart is None else int(restart), place, feather, pad, resample)
        self._check_stream_call(sink.name, slots, wa)
        return self._ring(sink, (r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale), s_r, feats, seed, noise, int(slots))

    @torch.no_grad()
    def generate_to_png(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15, noise=None,
                        band=None, return_rd=False, place=None, feather=None, resample=None):
        """generate_to_host for one clip (B = 1) with the frames leaving as LOSSLESS PNG files (png.PngFrames in pinned host memory):
        the chain, decode_u8 of the whole clip, float_png_encode on the 8-bit frames in HBM, ONE host read of the offsets, then
        offsets[T] bytes across PCIe - the files, not the frames.  File i decodes to frame i of
        generate_to_host(out_dtype=torch.uint8) bit for bit and is bitwise host_models.png_encode_rgb8 of it (band: rows per
        band, None = png.default_band).  Complete on return (the stream has been synchronised).  The 8-bit frames stay on the
        device: T * size * size * 3 bytes of HBM while it runs, and as much again for the files.
        place (a Placement; default None: nothing above changes): the 8-bit crops are pasted back into the portrait on the device
        (float_img_paste, `feather` as in generate_pasted) and the encoder codes the H x W frames, of any size up to 16384 - file i
        is png_encode_rgb8 of frame i of generate_pasted.  resample: as in generate_pasted (with place only)."""
        _check_resample("generate_to_png", resample, place)
        if place is not None:
            place = _check_place("generate_to_png", place, self.device)
        H, W = place.size if place is not None else (self.size, self.size)
        band = host_models.png_check_band(H, W, band)
        self.require_no_stream("generate_to_png")
        if feats is not None:
            self.dec.set_feats(feats)
        r_d = self.sample(r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale, seed, noise)
        with torch.cuda.device(self.device):
            u8 = self.dec.decode_u8(s_r, _rows(r_d))
            if place is not None:
                u8 = image.paste_frames_device(place.src8, u8, place.rect, feather, resample=resample,
                                               scratch=_paste_scratch(self, place, u8.shape[0], resample))
            frames = png.encode_png_host(u8, band)
        return (frames, r_d) if return_rd else frames

    def stream_to_png(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15, noise=None,
                      band=None, slots=3, place=None, feather=None, resample=None):
        """generate_to_png as a generator: one PngBlock(first, last, frames) per FMT window, in frame order, the same files as the
        whole-clip call.  The contract is stream_to_jpeg's: `frames` (a png.PngFrames) lives in one of `slots` pinned ring
        buffers, is complete when it is yielded and OVERWRITTEN after the generator has been advanced again (ApngWriter.write has
        handed the bytes on when it returns); slots >= 2, B = 1 and the band are checked at the call (ValueError), nothing is
        enqueued before the first next(); while the generator is open every other producer on this object raises RuntimeError.
        Per slot: a device buffer of 50 8-bit frames, a device and a pinned buffer of their raw size for the files, and the offsets
        and CRCs on both sides.  Files beyond the slot's room (noise: 9 / 8 of the raw size) are encoded once more into a larger
        buffer.  place, feather, resample: as in generate_to_png."""
        _check_resample("stream_to_png", resample, place)
        if place is not None:
            place = _check_place("stream_to_png", place, self.device)
        H, W = place.size if place is not None else (self.size, self.size)
        sink = _PngSink(self, host_models.png_check_band(H, W, band), place, feather, resample)
        self._check_stream_call(sink.name, slots, wa)
        return self._ring(sink, (r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale), s_r, feats, seed, noise, int(slots))

    def _overlap_streams(self, mode):
        """(chain stream, decoder stream) of the stage-overlapped forms.  mode "prio": two streams of one device queue set, the
        chain on the higher priority; "cu:N": disjoint CU sets (hipExtStreamCreateWithCUMask), the decoder on the last N CUs."""
        cache = self._ov_streams
        if mode not in cache:
            dev = self.device
            if mode.startswith("cu:"):
                n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
                n_dec = max(8, min(n_cu - 8, int(mode[3:])))
                with torch.cuda.device(dev):
                    cache[mode] = (native.cu_range_stream(0, n_cu - n_dec, dev), native.cu_range_stream(n_cu - n_dec, n_cu, dev))
            elif mode in ("prio", "plain", "hi", "lo"):
                # (least, greatest) priority: the greater priority is the SMALLER number; 0 is the default.  "hi" / "lo" raise the
                # chain / lower the decoder only (tools/probes/overlap_check.py; "hi" is what generate(overlap=True) runs on)
                lo, hi = torch.cuda.Stream.priority_range()
                pf = hi if mode in ("prio", "hi") else 0
                pd = lo if mode in ("prio", "lo") else 0
                cache[mode] = (torch.cuda.Stream(dev, priority=pf), torch.cuda.Stream(dev, priority=pd))
            else:
                raise ValueError("overlap mode must be 'prio', 'hi', 'lo', 'plain' or 'cu:N', got %r" % (mode,))
        return cache[mode]

    def _overlapped(self, mode, job, s_r, decode, frame_range=None):
        """The two-stream loop of the stage-overlapped forms: the chain of window k + 1 on one stream of _overlap_streams(mode)
        while decode(s_r_d, rows, f0, f1) runs for window k with the other one current.  The caller has produced everything
        `decode` touches (noise, destination, staging) on the current stream BEFORE this call: both streams wait for the current
        one only here, behind that work and behind s_r_d, and the current one waits for both at the end.  Returns r_d."""
        s_r_d = s_r.to(self.device, torch.float32).reshape(-1).contiguous()
        s_fmt, s_dec = self._overlap_streams(mode)
        cur = torch.cuda.current_stream(self.device)
        s_fmt.wait_stream(cur)
        s_dec.wait_stream(cur)
        for ws, f0, f1 in self._windows(job, s_fmt, s_dec, frame_range):
            with torch.cuda.stream(s_dec):
                decode(s_r_d, ws.r_d[0, f0:f1], f0, f1)
        cur.wait_stream(s_dec)
        cur.wait_stream(s_fmt)
        return self._last_job.r_d

    @torch.no_grad()
    def generate_to_host_overlap(self, r_s, wa, we, s_r, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, noise=None,
                                 out=None, mode="prio", return_rd=False, out_dtype=None, out_format=None, seed=15, matrix=None):
        """generate_to_host with the two stages pipelined (FLOAT.py runs 209-253 then 113-169; here window k is decoded and
        handed to the host on a second stream while the chain samples window k + 1).  Same kernels on the same operands as
        the sequential order, per-window decode batches (50 frames = 32 + 18 instead of 250 = 7 x 32 + 26): frames bitwise
        equal to generate_to_host (decode batching does not change a frame, tests/test_dec_gpu.py).  FLOAT_AMD_OVERLAP
        selects it in InferenceAgent.infer_device; what it measures against the sequential order: DESIGN.md section 7.
        out_dtype, out_format, matrix: as in decode_to_host (torch.uint8 = 8-bit frames, "i420" = planar YUV 4:2:0)."""
        out_dtype, out_format = resolve_out_format(out, out_dtype, out_format, matrix)
        matrix = self.yuv_matrix("generate_to_host_overlap", matrix, out_format)
        self.require_no_stream("generate_to_host_overlap")
        T = wa.shape[1]
        if noise is None:
            noise = draw_noise(self.n_chunks(T), 1, self.cfg, seed)
        self._prune_inflight()
        if out is None:
            out = torch.empty((T,) + self.dec.frame_shape(out_format), dtype=out_dtype, pin_memory=True)
        staging = self.staging(T, out_dtype, out_format)
        r_d = self._overlapped(mode, (r_s, wa, we, noise, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale), s_r,
                               lambda s_r_d, rows, f0, f1: self.dec.decode_into_host(s_r_d, rows, out[f0:f1], staging[f0:f1],
                                                                                     out_format=out_format, matrix=matrix))
        self._hold_inflight(out, torch.cuda.current_stream(self.device))
        return (out, r_d) if return_rd else out

    @torch.no_grad()
    def generate(self, r_s, wa, we, s_r, feats, nfe, a_cfg_scale=2.0, r_cfg_scale=1.0, e_cfg_scale=1.0, seed=15,
                 noise=None, overlap=False, frame_range=None, return_rd=False):
        """Whole hot path for one clip (B = 1): frames (T,H,W,3) on the GPU.

        overlap=True pipelines the two stages on two HIP streams (_overlap_streams("hi"): the chain on the greatest priority):
        the FMT chain of window k+1 runs while the decoder renders the 50 frames of window k.  Results are identical to the
        sequential order (same kernels, same operands).  Measured on MI355X it does NOT pay (r01: 183 vs 174 ms per 10 s
        clip): the decoder's grids own every CU, so each of the chain's ~3000 tiny dependent kernels per window queues behind
        running decoder workgroups; generate_to_host_overlap(mode="cu:N") is the form with disjoint CU sets.
        frame_range=(t0,t1) decodes only that shard of the clip (multi-GPU frame sharding)."""
        self.require_no_stream("generate")
        if feats is not None:
            self.dec.set_feats(feats)
        T = wa.shape[1]
        if noise is None:
            noise = draw_noise(self.n_chunks(T), 1, self.cfg, seed)
        if not overlap:
            r_d = self.sample(r_s, wa, we, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale, seed, noise)
            frames = self.decode(s_r, None, r_d, frame_range)
            return (frames, r_d) if return_rd else frames
        t0, t1 = frame_range if frame_range is not None else (0, T)
        out = torch.empty(t1 - t0, self.size, self.size, 3, device=self.device, dtype=torch.float32)
        r_d = self._overlapped("hi", (r_s, wa, we, noise, nfe, a_cfg_scale, r_cfg_scale, e_cfg_scale), s_r,
                               lambda s_r_d, rows, a, b: self.dec.decode_latent_into_processed_images(s_r_d, rows, out=out[a - t0:b - t0]),
                               (t0, t1))
        return (out, r_d) if return_rd else out


def synth_conditions(cfg: FmtConfig, T, seed=0, dynamic_we=False, device="cpu"):
    """Synthetic stand-ins for the off-path encoders' outputs (formats of SURVEY.md section 8a):
    wa ~ SiLU(LayerNorm-ed projection) (FLOAT.py:338-342), we softmax scores, r_s, s_r."""
    g = torch.Generator().manual_seed(1000 + seed)
    wa = torch.nn.functional.silu(torch.randn(1, T, cfg.dim_a, generator=g))
    if dynamic_we:
        nwin = int(math.ceil(T / cfg.num_frames_for_clip))
        w = torch.softmax(torch.randn(1, nwin, cfg.dim_e, generator=g), -1)
        idx = torch.clamp((torch.arange(T).float() * nwin / T).long(), max=nwin - 1)  # nearest upsample, nodes_vadv.py:835-838
        we = w[:, idx]
    else:
        we = torch.softmax(torch.randn(1, 1, cfg.dim_e, generator=g), -1)
    r_s = torch.randn(1, cfg.dim_w, generator=g) * 0.5
    s_r = torch.randn(1, cfg.dim_w, generator=g)
    return dict(wa=wa.to(device), we=we.to(device), r_s=r_s.to(device), s_r=s_r.to(device))
