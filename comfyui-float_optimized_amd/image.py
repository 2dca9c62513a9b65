"""The image front end on the device (`float_img_front`, include/float_hip.h): the reference's DataProcessor image half -
img_tensor_2_np_array, process_img's zero-bordered crop, cv2.resize(INTER_AREA), / 127.5 - 1 (utils/image.py, generate.py:29-39) -
as HIP kernels on the raw ComfyUI IMAGE tensor.  The definition is host_models.image_to_rgb8 + host_models.resize_rgb8; the
kernels work in integers from the quantiser on and give its bytes."""
import collections
import ctypes as C
import fractions
import logging
import math

import torch

from . import host_models, native

logger = logging.getLogger(__name__)


def image_to_device(img, device=None):
    """A ComfyUI IMAGE item - (H, W, 3|4) or (1, H, W, 3|4), any float dtype, host or device - as the contiguous fp32 device
    tensor `float_img_front` reads.  The one copy across PCIe (non_blocking); a tensor that is already in that form is returned
    as it is, so the functions below can be chained without moving anything twice."""
    if img.dim() == 4:
        if img.shape[0] != 1:
            raise ValueError("image front end: a batch of %d images (one image per call)" % img.shape[0])
        img = img[0]
    if img.dim() != 3 or img.shape[-1] not in (3, 4) or not img.is_floating_point():
        raise ValueError("image front end: expected an (H, W, 3) or (H, W, 4) float image, got %s %s" % (img.dtype, tuple(img.shape)))
    device = torch.device(device if device is not None else (img.device if img.is_cuda else "cuda:0"))
    x = img.detach().to(device, non_blocking=True)
    if x.dtype != torch.float32:
        x = x.float()
    return x.contiguous()


def _rgba_mode(rgba_conversion):
    mode = native.IMG_RGBA_MODES.get(rgba_conversion)
    if mode is None:  # utils/image.py:81-83
        logger.warning("Unknown RGBA conversion strategy: %r. Defaulting to 'discard_alpha'." % (rgba_conversion,))
        mode = native.IMG_RGBA_MODES["discard_alpha"]
    return mode


@torch.no_grad()
def image_front_device(img, dst_h, dst_w, rect=None, scale=None, rgba_conversion="blend_with_color", bkg_color_hex="#000000",
                       out_u8=False, device=None):
    """float_img_front on one image: the window `rect` = (x0, y0, w, h) of it (default: the whole image; it may reach outside,
    where the image is black) resized to dst_h x dst_w at w / dst_w by h / dst_h or at the shared `scale` = (P, Q) ->
    (dst_h, dst_w, 3) uint8 when out_u8, else (1, 3, dst_h, dst_w) fp32 in [-1, 1].  Runs on the current stream of the image's
    device; output and scratch come from torch's allocator, nothing synchronises."""
    x = image_to_device(img, device)
    H, W, ch = (int(v) for v in x.shape)
    x0, y0, w, h = (0, 0, W, H) if rect is None else (int(v) for v in rect)
    sn, sd = (0, 0) if scale is None else (int(scale[0]), int(scale[1]))
    bkg = host_models.hex_to_rgb8(bkg_color_hex)
    mode = _rgba_mode(rgba_conversion)
    L = native.lib()
    dst_h, dst_w = int(dst_h), int(dst_w)
    need = int(L.float_img_front_work_bytes(H, W, dst_h, dst_w))
    with torch.cuda.device(x.device):
        if out_u8:
            out = torch.empty(dst_h, dst_w, 3, dtype=torch.uint8, device=x.device)
        else:
            out = torch.empty(1, 3, dst_h, dst_w, dtype=torch.float32, device=x.device)
        work = torch.empty(max(1, need // 4), dtype=torch.int32, device=x.device)
        native.check(L.float_img_front(C.c_void_p(x.data_ptr()), H, W, ch, x0, y0, w, h, sn, sd, mode, bkg[0], bkg[1], bkg[2],
                                       native.IMG_OUT_HWC_U8 if out_u8 else native.IMG_OUT_NCHW_PM1, C.c_void_p(out.data_ptr()),
                                       dst_h, dst_w, C.c_void_p(work.data_ptr()), work.numel() * 4, native.stream_ptr(x.device)))
    return out


def preprocess_image_device(img, size, rect=None, rgba_conversion="blend_with_color", bkg_color_hex="#000000", device=None):
    """The model's source image from a ComfyUI IMAGE item: RGBA conversion, the optional crop `rect` (x0, y0, w, h - what
    host_models.process_img(..., front=...) returns), area resize to size x size, 8-bit rounding, / 127.5 - 1 -> (1, 3, size,
    size) fp32 on the device.  Bitwise host_models.rgb8_to_model_input(resize_rgb8(image_to_rgb8(img, ...), rect, size, size))."""
    return image_front_device(img, size, size, rect, None, rgba_conversion, bkg_color_hex, False, device)


def detector_view_size(H, W, view_h=360):
    """(rows, columns) of cv2.resize(img, (0, 0), fx=view_h / H, fy=view_h / H): both rounded half to even."""
    return int(view_h), max(1, round(fractions.Fraction(int(W) * int(view_h), int(H))))


def front_takes(H, W, size, crop=False, view_h=360):
    """Whether `float_img_front` takes an H x W source for a size x size model input - and, with `crop`, for the detector's
    view_h-row copy too.  Its limits (source sides 1 ... 16384, destination sides 1 ... 4096: float_hip.h) are asked of the
    library (`float_img_front_work_bytes` is 0 outside them), not repeated here.  A 4K or 8K portrait is far inside; a side
    above 16384 or, with `crop`, a panorama beyond about 11 : 1 is not, and InferenceAgent.host_inputs keeps the host route
    for those."""
    L = native.lib()
    if not L.float_img_front_work_bytes(int(H), int(W), int(size), int(size)):
        return False
    return not crop or bool(L.float_img_front_work_bytes(int(H), int(W), *detector_view_size(H, W, view_h)))


def detector_view_device(img, view_h=360, rgba_conversion="blend_with_color", bkg_color_hex="#000000", device=None):
    """The copy of the image the face detector looks at (utils/image.py:142-146): view_h rows, round(W view_h / H) columns, both
    axes at the one scale H / view_h -> (view_h, columns, 3) uint8 on the device.  Bitwise
    resize_rgb8(image_to_rgb8(img, ...), None, view_h, columns, scale=(H, view_h))."""
    x = image_to_device(img, device)
    H, W = int(x.shape[0]), int(x.shape[1])
    vh, vw = detector_view_size(H, W, view_h)
    g = math.gcd(H, vh)
    return image_front_device(x, vh, vw, None, (H // g, vh // g), rgba_conversion, bkg_color_hex, True, device)


# ---------------------------------------------------------------------------------------------------------------------------
# the step after the decoder: the generated frames back in the source portrait (`float_img_paste`, include/float_hip.h)
# ---------------------------------------------------------------------------------------------------------------------------
JPEG_SIDE_MULTIPLE = 16  # float_jpg_encode codes frames whose sides are multiples of 16


def source_rgb8_device(img, rgba_conversion="blend_with_color", bkg_color_hex="#000000", device=None):
    """A ComfyUI IMAGE item as the (H, W, 3) uint8 portrait on the device that the frames are pasted into: bitwise
    host_models.image_to_rgb8(img, rgba_conversion, hex_to_rgb8(bkg_color_hex)).  Inside float_img_front's limits it is the
    identity-scale call of image_front_device(out_u8=True) - the quantiser and the RGBA conversion alone; beyond them (a side
    above 4096, that operator's destination limit) it is the host definition and one upload."""
    x = img[0] if img.dim() == 4 and img.shape[0] == 1 else img
    if x.dim() != 3 or x.shape[-1] not in (3, 4) or not x.is_floating_point():
        raise ValueError("source_rgb8_device: expected an (H, W, 3) or (H, W, 4) float image, got %s %s" % (img.dtype, tuple(img.shape)))
    H, W = int(x.shape[0]), int(x.shape[1])
    if native.lib().float_img_front_work_bytes(H, W, H, W):
        return image_front_device(x, H, W, None, None, rgba_conversion, bkg_color_hex, True, device)
    device = torch.device(device if device is not None else (x.device if x.is_cuda else "cuda:0"))
    return host_models.image_to_rgb8(x, rgba_conversion, host_models.hex_to_rgb8(bkg_color_hex)).to(device, non_blocking=True)


def _u8_device(t, what, dims, device):
    if t.dtype != torch.uint8 or t.dim() != dims or t.shape[-1] != 3 or 0 in t.shape:
        raise ValueError("paste_frames_device: %s must be %s uint8, got %s %s"
                         % (what, "(H, W, 3)" if dims == 3 else "(T, h, w, 3)", t.dtype, tuple(t.shape)))
    return t.detach().to(device, non_blocking=True).contiguous()


def paste_format(what, out_format):
    """The frame format of a pasted producer: None | "rgb" -> "rgb" ((T, H, W, 3) uint8), "i420" -> "i420" ((T, 3H/2, W) uint8)."""
    if out_format in (None, "rgb"):
        return "rgb"
    if out_format != "i420":
        raise ValueError("%s: out_format must be None, 'rgb' or 'i420' (got %r)" % (what, out_format))
    return "i420"


def require_even_sides(what, H, W):
    """4:2:0 chroma halves both sides; a pasted clip has the portrait's size.  Nothing is padded or cropped."""
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError("%s: a %d x %d portrait cannot leave as I420 - 4:2:0 chroma needs even sides (crop or resize the portrait, "
                         "or take the RGB frames)" % (what, H, W))


def pasted_frame_shape(H, W, fmt):
    """The shape of one pasted frame: (H, W, 3), or (3H/2, W) as I420."""
    return (3 * H // 2, W) if fmt == "i420" else (H, W, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# bicubic / Lanczos resampling of 8-bit frames (`float_img_resample`, include/float_hip.h): what `resample=` selects on the paste
# ---------------------------------------------------------------------------------------------------------------------------
RESAMPLE_TABLES_KEPT = 8  # (sizes, window, filter, device) entries of the table cache: a clip uses one
_resample_tables = collections.OrderedDict()


def resample_table(n_in, n_out, filter, first=0, count=None):
    """float_img_resample_plan: one axis's table for output indices first ... first + count - 1 -> (count, 2 + ksize) int32 on the
    host, rows xmin, n, k[0 ... ksize - 1]: integer for integer host_models.resample_coeffs.  Host arithmetic in the library; no
    GPU is touched.  The library's refusals (an unknown filter, sizes below 1, more than 255 taps) are ValueErrors."""
    fid = host_models.resample_filter_id("resample_table", filter)
    n_in, n_out, first = int(n_in), int(n_out), int(first)
    count = n_out - first if count is None else int(count)
    L = native.lib()
    ints = int(L.float_img_resample_plan_ints(n_in, n_out, fid, count))
    table = torch.empty(max(ints, 1), dtype=torch.int32)
    native.check(L.float_img_resample_plan(n_in, n_out, fid, first, count, C.cast(table.data_ptr(), C.POINTER(C.c_int32)), ints))
    return table[:ints].reshape(count, ints // count)


def _resample_tables_device(device, fr_h, fr_w, h, w, filter, window):
    """(tab_x, tab_y) on the device for a call of float_img_resample, None for an axis that keeps its size; made and uploaded
    once per (sizes, window, filter, device) - once per clip on the paste routes - and kept for the next call."""
    key = (str(device), fr_h, fr_w, h, w, filter, window)
    tabs = _resample_tables.get(key)
    if tabs is None:
        xa, ya, wc, hc = window
        tabs = (resample_table(fr_w, w, filter, xa, wc).to(device) if fr_w != w else None,
                resample_table(fr_h, h, filter, ya, hc).to(device) if fr_h != h else None)  # blocking copies: complete on return
        _resample_tables[key] = tabs
        while len(_resample_tables) > RESAMPLE_TABLES_KEPT:
            _resample_tables.popitem(last=False)
    else:
        _resample_tables.move_to_end(key)
    return tabs


class ResampleScratch:
    """The device memory one resampled paste needs besides its output: `face`, the box-sized window of n frames, and `work`, the
    intermediate of float_img_resample.  Made once by paste_scratch for the largest group of frames and handed to every
    paste_frames_device(..., resample=, scratch=) of a clip."""

    def __init__(self, face, work):
        self.face, self.work = face, work


def paste_window(H, W, rect):
    """(xa, ya, xb, yb): the box rect = (x0, y0, w, h) clipped to an H x W image, as host_models.paste_rgb8 clips it; None when
    the box misses the image."""
    x0, y0, w, h = (int(v) for v in rect)
    ya, yb, xa, xb = max(0, y0), min(H, y0 + h), max(0, x0), min(W, x0 + w)
    return None if yb <= ya or xb <= xa else (xa, ya, xb, yb)


def _resample_work_bytes(n, fr_h, fr_w, h, w, fid, window):
    need = int(native.lib().float_img_resample_work_bytes(n, fr_h, fr_w, h, w, fid, *window))
    if not need:
        raise ValueError("resample: %d frames of %d x %d to %d x %d, window %r, are outside float_img_resample's limits (sides 1 ... 16384, "
                         "at most 255 taps per sample)" % (n, fr_h, fr_w, h, w, tuple(window)))
    return need


def paste_scratch(src_hw, frame_hw, rect, n, resample, device):
    """The ResampleScratch of pasting up to n frames of frame_hw at `rect` into a portrait of src_hw with resample=`resample`;
    None when there is nothing to resample (resample None, or a box that misses the image)."""
    if resample is None:
        return None
    fid = host_models.resample_filter_id("paste_scratch", resample)
    win = paste_window(int(src_hw[0]), int(src_hw[1]), rect)
    if win is None:
        return None
    xa, ya, xb, yb = win
    x0, y0, w, h = (int(v) for v in rect)
    need = _resample_work_bytes(int(n), int(frame_hw[0]), int(frame_hw[1]), h, w, fid, (xa - x0, ya - y0, xb - xa, yb - ya))
    return ResampleScratch(torch.empty(int(n), yb - ya, xb - xa, 3, dtype=torch.uint8, device=device),
                           torch.empty((need + 3) // 4, dtype=torch.int32, device=device))


@torch.no_grad()
def resample_frames_device(frames8, h, w, filter, window=None, out=None, work=None):
    """float_img_resample: frames8 (T, h_f, w_f, 3) uint8 resampled to h x w by Pillow's rule with filter "bicubic" | "lanczos" ->
    (T, h, w, 3) uint8 on the device, or with window = (xa, ya, wc, hc) only that part of it, (T, hc, wc, 3): bitwise
    host_models.resample_rgb8(frames8, h, w, filter, window).  Host tensors are uploaded (device: that of frames8, else cuda:0).
    out: a contiguous uint8 tensor of the result's shape on that device to write into; work: an int32 device tensor of at least
    float_img_resample_work_bytes (default: torch's allocator).  The two tables come from float_img_resample_plan and are kept
    on the device per (sizes, window, filter).  At most two launches on the current stream; nothing synchronises."""
    fid = host_models.resample_filter_id("resample_frames_device", filter)
    device = frames8.device if frames8.is_cuda else torch.device("cuda:0")
    f = _u8_device(frames8, "frames8", 4, device)
    T, fr_h, fr_w = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("resample_frames_device: the result %d x %d must be at least 1 x 1" % (h, w))
    window = host_models.resample_window("resample_frames_device", h, w, window)
    xa, ya, wc, hc = window
    need = _resample_work_bytes(T, fr_h, fr_w, h, w, fid, window)
    shape = (T, hc, wc, 3)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != device or not out.is_contiguous():
            raise ValueError("resample_frames_device: out must be a contiguous %s uint8 tensor on %s, got %s %s on %s"
                             % (shape, device, out.dtype, tuple(out.shape), out.device))
        if work is None:
            work = torch.empty((need + 3) // 4, dtype=torch.int32, device=device)
        elif work.dtype != torch.int32 or work.device != device or not work.is_contiguous() or work.numel() * 4 < need:
            raise ValueError("resample_frames_device: work must be a contiguous int32 tensor of at least %d bytes on %s" % (need, device))
        tab_x, tab_y = _resample_tables_device(device, fr_h, fr_w, h, w, filter, window)
        native.check(native.lib().float_img_resample(
            C.c_void_p(f.data_ptr()), T, fr_h, fr_w, h, w, fid, xa, ya, wc, hc, C.c_void_p(tab_x.data_ptr()) if tab_x is not None else None,
            C.c_void_p(tab_y.data_ptr()) if tab_y is not None else None, C.c_void_p(work.data_ptr()), work.numel() * 4,
            C.c_void_p(out.data_ptr()), native.stream_ptr(device)))
    return out


@torch.no_grad()
def paste_frames_device(src8, frames8, rect, feather=None, out=None, out_format=None, matrix=None, resample=None, scratch=None):
    """float_img_paste: frames8 (T, h, w, 3) uint8 - what the decoder's decode_u8 leaves in HBM - back in the portrait src8 (H, W,
    3) uint8 at the box rect = (x0, y0, w, h) in source coordinates (what InferenceAgent.host_inputs_placed returns; it may reach
    outside the image) -> (T, H, W, 3) uint8 on the device, bitwise host_models.paste_rgb8(src8, frames8, rect, feather).
    feather: the width in source pixels over which the box's open sides fade into the portrait; None = rect_w // 16
    (host_models.default_feather: a visual choice, not a measurement).  Host tensors are uploaded; the device is that of frames8,
    else of src8, else cuda:0.  out: a contiguous (T, H, W, 3) uint8 tensor on that device to write into.  One launch on the
    current stream; nothing is allocated besides `out`, nothing synchronises.
    out_format: None | "rgb" as above; "i420" is float_img_paste_i420, paste and colour conversion in one kernel -> (T, 3H/2, W)
    uint8 planar YUV 4:2:0, bitwise host_models.paste_i420(src8, frames8, rect, feather, matrix), half the bytes;
    H and W must be even (ValueError) and `out` is checked against that shape.  matrix: as host_models.yuv_matrix_id reads it
    (None = BT.601 limited range; "auto" goes by the portrait's size); with RGB frames anything but None is a ValueError.
    resample: None as above; "bicubic" | "lanczos": the face is Pillow's resize of the frame with that filter instead of the front
    end's rule - bitwise host_models.paste_rgb8 / paste_i420(..., resample=resample).  float_img_resample forms the window of the
    box that lies in the image (two more launches, tables uploaded once per sizes), and the paste kernel above gets that window
    as its frames, the clipped box as its rect and the feather of the unclipped one: its resize at equal sizes is the identity
    and clipping moves no open side, so the bytes are the definition's.  A box that misses the image launches nothing new.
    scratch: a ResampleScratch of paste_scratch for at least T frames (default: torch's allocator, per call)."""
    fmt = paste_format("paste_frames_device", out_format)
    if resample is not None:
        host_models.resample_filter_id("paste_frames_device", resample)  # refused before anything is uploaded
    if fmt != "i420":
        host_models.yuv_matrix_for("paste_frames_device", matrix, fmt)  # refused before anything is uploaded
    device = frames8.device if frames8.is_cuda else (src8.device if src8.is_cuda else torch.device("cuda:0"))
    s = _u8_device(src8, "src8", 3, device)
    f = _u8_device(frames8, "frames8", 4, device)
    m = host_models.yuv_matrix_for("paste_frames_device", matrix, fmt, int(s.shape[1]), int(s.shape[0]))
    if len(rect) != 4:
        raise ValueError("paste_frames_device: rect must be (x0, y0, w, h), got %r" % (rect,))
    x0, y0, w, h = (int(v) for v in rect)
    if max(abs(x0), abs(y0)) > 1 << 30 or not (0 < w <= 1 << 30 and 0 < h <= 1 << 30):
        raise ValueError("paste_frames_device: rect %r is outside float_img_paste's limits" % (tuple(rect),))
    feather = host_models.default_feather((x0, y0, w, h)) if feather is None else int(feather)
    if not 0 <= feather <= 1 << 30:
        raise ValueError("paste_frames_device: feather (%d) must be 0 ... 16384" % feather)
    T, H, W = int(f.shape[0]), int(s.shape[0]), int(s.shape[1])
    if fmt == "i420":
        require_even_sides("paste_frames_device", H, W)
    shape = (T,) + pasted_frame_shape(H, W, fmt)
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=device)
        elif (out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != device or not out.is_contiguous()):
            raise ValueError("paste_frames_device: out must be a contiguous %s uint8 tensor on %s, got %s %s on %s"
                             % (shape, device, out.dtype, tuple(out.shape), out.device))
        L = native.lib()
        win = paste_window(H, W, (x0, y0, w, h)) if resample is not None else None
        if win is not None:
            xa, ya, xb, yb = win
            if scratch is None:
                scratch = paste_scratch((H, W), f.shape[1:3], (x0, y0, w, h), T, resample, device)
            elif scratch.face.shape[0] < T or tuple(scratch.face.shape[1:]) != (yb - ya, xb - xa, 3) or scratch.face.device != device:
                raise ValueError("paste_frames_device: scratch was made for another paste (%s for %d frames of the window %r)"
                                 % (tuple(scratch.face.shape), T, win))
            f = resample_frames_device(f, h, w, resample, (xa - x0, ya - y0, xb - xa, yb - ya), out=scratch.face[:T], work=scratch.work)
            x0, y0, w, h = xa, ya, xb - xa, yb - ya  # `feather` stays the unclipped box's
        if fmt == "i420":
            native.check(L.float_img_paste_i420(C.c_void_p(s.data_ptr()), H, W, C.c_void_p(f.data_ptr()), T, int(f.shape[1]), int(f.shape[2]),
                                                x0, y0, w, h, feather, m, C.c_void_p(out.data_ptr()),
                                                native.stream_ptr(device)))
        else:
            native.check(L.float_img_paste(C.c_void_p(s.data_ptr()), H, W, C.c_void_p(f.data_ptr()), T, int(f.shape[1]), int(f.shape[2]),
                                           x0, y0, w, h, feather, C.c_void_p(out.data_ptr()), native.stream_ptr(device)))
    return out


def require_jpeg_sides(what, H, W, pad=None):
    """float_jpg_encode takes frames whose sides are multiples of 16; a pasted clip has the portrait's size.  Nothing is padded
    unless the caller opts in: pad="edge" (float_jpg_encode_padded) passes any size."""
    if pad is not None and pad != "edge":
        raise ValueError("%s: pad must be None or \"edge\" (got %r)" % (what, pad))
    if pad is None and (H % JPEG_SIDE_MULTIPLE or W % JPEG_SIDE_MULTIPLE):
        raise ValueError("%s: a %d x %d portrait cannot leave as JPEG - float_jpg_encode needs sides that are multiples of 16 "
                         "(crop or resize the portrait, or take the frames with infer_pasted)" % (what, H, W))
