"""The image front end on the device (`float_img_front`, include/float_hip.h): the reference's DataProcessor image half -
img_tensor_2_np_array, process_img's zero-bordered crop, cv2.resize(INTER_AREA), / 127.5 - 1 (utils/image.py, generate.py:29-39) -
as HIP kernels on the raw ComfyUI IMAGE tensor.  The definition is host_models.image_to_rgb8 + host_models.resize_rgb8; the
kernels work in integers from the quantiser on and give its bytes."""
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


@torch.no_grad()
def paste_frames_device(src8, frames8, rect, feather=None, out=None, out_format=None, matrix=None):
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
    (None = BT.601 limited range; "auto" goes by the portrait's size); with RGB frames anything but None is a ValueError."""
    fmt = paste_format("paste_frames_device", out_format)
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
