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
# a stack of frames, one window per frame (`float_img_front_frames`, include/float_hip.h): the driving video's front end
# ---------------------------------------------------------------------------------------------------------------------------
def frames_to_device(frames, device=None):
    """A video - (T, H, W, 3|4), uint8 or any float dtype, host or device - as the contiguous uint8 or fp32 device tensor
    `float_img_front_frames` reads; a tensor already in that form is returned as it is."""
    if frames.dim() != 4 or frames.shape[-1] not in (3, 4) or 0 in frames.shape or not (frames.dtype == torch.uint8 or frames.is_floating_point()):
        raise ValueError("frames front end: expected (T, H, W, 3|4) uint8 or float frames, got %s %s" % (frames.dtype, tuple(frames.shape)))
    device = torch.device(device if device is not None else (frames.device if frames.is_cuda else "cuda:0"))
    x = frames.detach().to(device, non_blocking=True)
    if x.dtype != torch.uint8 and x.dtype != torch.float32:
        x = x.float()
    return x.contiguous()


class YuvFrames:
    """A stack of 8-bit YUV 4:2:0 frames as front_frames_device and InferenceAgent.align_driving take them: data (T, 3h/2, w) - or
    (3h/2, w), one frame - uint8 on the host or the device, in `layout` "i420" (Y, then U and V at h/2 x w/2: ffmpeg's yuv420p,
    what the I420 outputs and host_models.Y4MReader give) or "nv12" (Y, then h/2 rows of interleaved U, V: most hardware
    decoders).  matrix: the matrix the frames were made with, as host_models.yuv_matrix_id reads it (None = BT.601 limited range;
    "auto" by w x h); chroma: "nearest" | "centre" (host_models.yuv420_to_rgb8).  h and w must be even; everything is checked
    here (ValueError).  len() is T and a slice frames[a:b] (step 1) is a YuvFrames over a view of those frames."""

    def __init__(self, data, h, w, layout="i420", matrix=None, chroma="nearest"):
        host_models.yuv420_check("YuvFrames", layout, chroma)
        h, w = int(h), int(w)
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError("YuvFrames: 4:2:0 frames have even sides (got %d x %d)" % (h, w))
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() not in (2, 3) or tuple(data.shape[-2:]) != (3 * h // 2, w):
            raise ValueError("YuvFrames: data must be (T, %d, %d) uint8 for %d x %d frames, got %s %s"
                             % (3 * h // 2, w, h, w, getattr(data, "dtype", type(data).__name__), tuple(getattr(data, "shape", ()))))
        self.data = data[None] if data.dim() == 2 else data
        self.h, self.w, self.layout, self.chroma = h, w, layout, chroma
        self.matrix = host_models.yuv_matrix_id(matrix, w, h)

    def __len__(self):
        return int(self.data.shape[0])

    def __getitem__(self, key):
        if not isinstance(key, slice) or key.step not in (None, 1):
            raise TypeError("YuvFrames: frames are taken by range, frames[a:b]")
        return YuvFrames(self.data[key], self.h, self.w, self.layout, self.matrix, self.chroma)

    def take(self, idx):
        """The frames `idx` (a list of indices) as a YuvFrames of their own."""
        return YuvFrames(self.data[torch.as_tensor(idx, dtype=torch.int64, device=self.data.device)], self.h, self.w, self.layout, self.matrix,
                         self.chroma)

    def to_rgb8(self):
        """The definition's frames: host_models.yuv420_to_rgb8 -> (T, h, w, 3) uint8 on the data's device."""
        return host_models.yuv420_to_rgb8(self.data, self.layout, self.matrix, self.chroma)


# ffmpeg's pixel-format names (and the FOURCCs YV12 and NV21's kin) -> PlanarYuv's keywords
PLANAR_YUV_NAMES = {
    "yuv420p": dict(sub="420"), "yuv422p": dict(sub="422"), "yuv444p": dict(sub="444"),
    "yuvj420p": dict(sub="420"), "yuvj422p": dict(sub="422"), "yuvj444p": dict(sub="444"),  # the same planes; the caller states the matrix
    "yv12": dict(sub="420", swap_uv=True),
    "nv12": dict(sub="420", semi=True), "nv21": dict(sub="420", semi=True, swap_uv=True),
    "nv16": dict(sub="422", semi=True), "nv24": dict(sub="444", semi=True), "nv42": dict(sub="444", semi=True, swap_uv=True),
    "yuv420p10le": dict(sub="420", depth=10), "yuv422p10le": dict(sub="422", depth=10), "yuv444p10le": dict(sub="444", depth=10),
    "yuv420p12le": dict(sub="420", depth=12), "yuv422p12le": dict(sub="422", depth=12), "yuv444p12le": dict(sub="444", depth=12),
    "p010": dict(sub="420", depth=10, shift=6, semi=True), "p010le": dict(sub="420", depth=10, shift=6, semi=True),
    "p012": dict(sub="420", depth=12, shift=4, semi=True), "p012le": dict(sub="420", depth=12, shift=4, semi=True),
    "p210": dict(sub="422", depth=10, shift=6, semi=True), "p210le": dict(sub="422", depth=10, shift=6, semi=True),
    "p410": dict(sub="444", depth=10, shift=6, semi=True), "p410le": dict(sub="444", depth=10, shift=6, semi=True),
}


class PlanarYuv:
    """A stack of planar or semi-planar YUV frames as a decoder hands them out, for front_frames_device and
    InferenceAgent.align_driving: data, a contiguous uint8 tensor on the host or the device, read as flat bytes exactly as it lies in
    memory, and where the h x w frames' planes are in it - host_models.yuv_planes_format has the keywords (sub "420" | "422" |
    "444", depth 8 | 10 | 12, shift, semi, swap_uv; pitches, frame_stride and offsets in bytes, None = packed in the order Y, U, V;
    matrix as host_models.yuv_matrix_id reads it, "auto" by w x h; chroma "nearest" | "centre").  Odd sides are allowed.  Everything
    is checked here (ValueError).  len() is the number of frames the buffer holds: (T - 1) frame_stride + the last plane's end <=
    data.numel().  frames[a:b] (step 1) and take(idx) are PlanarYuv objects of their own; to_rgb8() is the definition's frames.
    PlanarYuv.of(name, data, h, w, **more) builds one from an ffmpeg pixel-format name (PLANAR_YUV_NAMES)."""

    def __init__(self, data, h, w, *, sub="420", depth=8, shift=0, semi=False, swap_uv=False, y_pitch=None, c_pitch=None, frame_stride=None,
                 y_off=0, u_off=None, v_off=None, matrix=None, chroma="nearest"):
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or not data.is_contiguous():
            raise ValueError("PlanarYuv: data must be a contiguous uint8 tensor, got %s %s"
                             % (getattr(data, "dtype", type(data).__name__), tuple(getattr(data, "shape", ()))))
        self.fmt = host_models.yuv_planes_format(h, w, sub, depth, shift, semi, swap_uv, y_pitch, c_pitch, frame_stride, y_off, u_off, v_off,
                                                 matrix, chroma)
        self.data = data.reshape(-1)
        self._n = host_models.yuv_planes_frames(self.data.numel(), self.fmt)

    @classmethod
    def of(cls, name, data, h, w, **more):
        """A PlanarYuv from an ffmpeg pixel-format name: PlanarYuv.of("yuv422p10le", data, h, w, y_pitch=..., c_pitch=...)."""
        if name not in PLANAR_YUV_NAMES:
            raise ValueError("PlanarYuv.of: %r is not one of %s" % (name, sorted(PLANAR_YUV_NAMES)))
        return cls(data, h, w, **dict(PLANAR_YUV_NAMES[name], **more))

    def like(self, data, matrix=None, chroma=None):
        """The same layout over another buffer (a chunk of this one's frames, or its copy on the device); matrix and chroma
        replace this one's where given."""
        if chroma is not None and chroma not in host_models.YUV_CHROMA:
            raise ValueError("PlanarYuv: chroma must be one of %s (got %r)" % (host_models.YUV_CHROMA, chroma))
        new = object.__new__(PlanarYuv)
        new.fmt = self.fmt._replace(matrix=self.fmt.matrix if matrix is None else host_models.yuv_matrix_id(matrix, self.w, self.h),
                                    chroma=self.fmt.chroma if chroma is None else chroma)
        new.data = data.reshape(-1)
        new._n = host_models.yuv_planes_frames(new.data.numel(), new.fmt)
        return new

    h, w, matrix, chroma = (property(lambda self, k=k: getattr(self.fmt, k)) for k in ("h", "w", "matrix", "chroma"))

    def __len__(self):
        return self._n

    def frame_bytes(self, a, b):
        """The bytes of frames a ... b - 1, a view: from frame a's first byte to the end of frame b - 1's last plane."""
        if not 0 <= a < b <= self._n:
            raise ValueError("PlanarYuv: frames %d ... %d of %d" % (a, b - 1, self._n))
        return self.data[a * self.fmt.frame_stride:(b - 1) * self.fmt.frame_stride + self.fmt.last_end]

    def __getitem__(self, key):
        if not isinstance(key, slice) or key.step not in (None, 1):
            raise TypeError("PlanarYuv: frames are taken by range, frames[a:b]")
        a, b, _ = key.indices(self._n)
        return self.like(self.frame_bytes(a, b))

    def take(self, idx):
        """The frames `idx` (a list of indices) as a PlanarYuv of their own, each copied up to its last plane's end."""
        fmt = self.fmt
        stride = fmt.last_end + (fmt.last_end & 1)
        new = self.like(torch.stack([torch.nn.functional.pad(self.frame_bytes(int(i), int(i) + 1), (0, stride - fmt.last_end)) for i in idx]))
        new.fmt = new.fmt._replace(frame_stride=stride)
        new._n = len(idx)
        return new

    def to_rgb8(self):
        """The definition's frames: host_models.yuv_planes_to_rgb8 -> (T, h, w, 3) uint8 on the data's device."""
        return host_models.yuv_planes_to_rgb8(self.data, self.fmt)


def _front_frames_planes(frames, r, dst_h, dst_w, out, sn, sd, device):
    """front_frames_device for a PlanarYuv: float_img_front_frames_planes on the buffer as it is"""
    device = torch.device(device if device is not None else (frames.data.device if frames.data.is_cuda else "cuda:0"))
    x = frames.data.detach().to(device, non_blocking=True)
    T, f = len(frames), frames.fmt
    shape = (T, dst_h, dst_w, 3)
    planes = native.ImgPlanes(f.hs, f.vs, f.depth, f.shift, f.y_off, f.u_off, f.v_off, f.y_pitch, f.c_pitch, f.c_step, f.frame_stride)
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=x.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != x.device or not out.is_contiguous():
            raise ValueError("front_frames_device: out must be a contiguous %s uint8 tensor on %s, got %s %s on %s"
                             % (shape, x.device, out.dtype, tuple(out.shape), out.device))
        native.check(native.lib().float_img_front_frames_planes(
            C.c_void_p(x.data_ptr()), x.numel(), T, f.h, f.w, C.byref(planes), f.matrix, native.YUV_CHROMA[f.chroma],
            C.cast(r.data_ptr(), C.POINTER(C.c_int32)), sn, sd, C.c_void_p(out.data_ptr()), dst_h, dst_w, native.stream_ptr(x.device)))
    return out


def _front_frames_yuv(frames, r, dst_h, dst_w, out, sn, sd, device):
    """front_frames_device for a YuvFrames: float_img_front_frames_yuv"""
    device = torch.device(device if device is not None else (frames.data.device if frames.data.is_cuda else "cuda:0"))
    x = frames.data.detach().to(device, non_blocking=True).contiguous()
    T = len(frames)
    shape = (T, dst_h, dst_w, 3)
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=x.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != x.device or not out.is_contiguous():
            raise ValueError("front_frames_device: out must be a contiguous %s uint8 tensor on %s, got %s %s on %s"
                             % (shape, x.device, out.dtype, tuple(out.shape), out.device))
        native.check(native.lib().float_img_front_frames_yuv(
            C.c_void_p(x.data_ptr()), T, frames.h, frames.w, native.YUV_LAYOUTS[frames.layout], frames.matrix, native.YUV_CHROMA[frames.chroma],
            C.cast(r.data_ptr(), C.POINTER(C.c_int32)), sn, sd, C.c_void_p(out.data_ptr()), dst_h, dst_w, native.stream_ptr(x.device)))
    return out


@torch.no_grad()
def front_frames_device(frames, rects, dst_h, dst_w, rgba_conversion="blend_with_color", bkg_color_hex="#000000", out=None, scale=None,
                        device=None):
    """float_img_front_frames: frames (T, H, W, 3|4), fp32 in [0, 1] or uint8, and one window per frame - rects, T rows (x0, y0, w,
    h) in source coordinates (a single row serves every frame; a window may reach outside the image, where it is black) ->
    (T, dst_h, dst_w, 3) uint8 on the device.  Frame t is bitwise host_models.resize_rgb8(host_models.image_to_rgb8(frames[t],
    ...), rects[t], dst_h, dst_w, scale).  One fused kernel per 16 frames on the current stream of the frames' device; no scratch;
    nothing synchronises.  out: a contiguous (T, dst_h, dst_w, 3) uint8 tensor on that device to write into.
    frames may also be a YuvFrames (8-bit YUV 4:2:0, I420 or NV12): float_img_front_frames_yuv converts, crops and resizes in the
    same single pass, frame t bitwise host_models.resize_rgb8(host_models.yuv420_to_rgb8(frame t, layout, matrix, chroma),
    rects[t], dst_h, dst_w, scale); YUV has no alpha, so rgba_conversion and bkg_color_hex are not read.
    frames may also be a PlanarYuv (any planar YUV: 10 / 12 bits, 4:2:2, 4:4:4, odd sides, pitched): float_img_front_frames_planes
    reads the buffer as it lies, frame t bitwise host_models.resize_rgb8(frames.to_rgb8()[t], rects[t], dst_h, dst_w, scale)."""
    yuv = isinstance(frames, (YuvFrames, PlanarYuv))
    x = None if yuv else frames_to_device(frames, device)
    T, H, W, ch = (len(frames), frames.h, frames.w, 3) if yuv else (int(v) for v in x.shape)
    r = torch.as_tensor(rects, dtype=torch.int32, device="cpu").reshape(-1, 4)
    if r.shape[0] == 1 and T > 1:
        r = r.expand(T, 4)
    if r.shape[0] != T:
        raise ValueError("front_frames_device: %d rects for %d frames" % (r.shape[0], T))
    r = r.contiguous()
    sn, sd = (0, 0) if scale is None else (int(scale[0]), int(scale[1]))
    if yuv:
        return (_front_frames_planes if isinstance(frames, PlanarYuv) else _front_frames_yuv)(frames, r, int(dst_h), int(dst_w), out, sn, sd, device)
    bkg = host_models.hex_to_rgb8(bkg_color_hex)
    mode = _rgba_mode(rgba_conversion)
    dst_h, dst_w = int(dst_h), int(dst_w)
    shape = (T, dst_h, dst_w, 3)
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=x.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != x.device or not out.is_contiguous():
            raise ValueError("front_frames_device: out must be a contiguous %s uint8 tensor on %s, got %s %s on %s"
                             % (shape, x.device, out.dtype, tuple(out.shape), out.device))
        native.check(native.lib().float_img_front_frames(
            C.c_void_p(x.data_ptr()), T, H, W, ch, native.IMG_SRC_U8 if x.dtype == torch.uint8 else native.IMG_SRC_F32,
            C.cast(r.data_ptr(), C.POINTER(C.c_int32)), sn, sd, mode, bkg[0], bkg[1], bkg[2], C.c_void_p(out.data_ptr()), dst_h, dst_w,
            native.stream_ptr(x.device)))
    return out


def detector_views_device(frames, view_h=360, rgba_conversion="blend_with_color", bkg_color_hex="#000000", out=None, device=None):
    """The detector's view of every frame in one call: (T, view_h, round(W view_h / H), 3) uint8 on the device; view t is bitwise
    detector_view_device(frames[t], view_h, ...) - the whole image as every rect, both axes at the one scale H / view_h.  For a
    YuvFrames view t is bitwise resize_rgb8(yuv420_to_rgb8(frame t, ...), None, view_h, columns, scale=(H, view_h)), and for a
    PlanarYuv the same on its to_rgb8()."""
    H, W = (frames.h, frames.w) if isinstance(frames, (YuvFrames, PlanarYuv)) else (int(frames.shape[1]), int(frames.shape[2]))
    vh, vw = detector_view_size(H, W, view_h)
    g = math.gcd(H, vh)
    return front_frames_device(frames, (0, 0, W, H), vh, vw, rgba_conversion, bkg_color_hex, out, (H // g, vh // g), device)


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
    """The device memory one resampled or multi-band paste needs besides its output: `face`, the box-sized window of n frames,
    `work`, the intermediate of float_img_resample (None without resample=), and for blend="multiband" `crop`, the portrait's
    window that float_img_paste forms the face on, and `blend_work`, the pyramids of float_img_blend.  Made once by paste_scratch
    for the largest group of frames and handed to every paste_frames_device(..., scratch=) of a clip."""

    def __init__(self, face, work, crop=None, blend_work=None):
        self.face, self.work, self.crop, self.blend_work = face, work, crop, blend_work


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


def paste_scratch(src_hw, frame_hw, rect, n, resample, device, blend=None, inset=None, levels=None):
    """The ResampleScratch of pasting up to n frames of frame_hw at `rect` into a portrait of src_hw with resample=`resample` and
    blend=`blend`; None when neither needs one (both None, or a box that misses the image)."""
    spec = blend_spec("paste_scratch", blend, inset, levels, rect)
    if resample is None and spec is None:
        return None
    win = paste_window(int(src_hw[0]), int(src_hw[1]), rect)
    if win is None:
        return None
    xa, ya, xb, yb = win
    x0, y0, w, h = (int(v) for v in rect)
    work = crop = blend_work = None
    if resample is not None:
        fid = host_models.resample_filter_id("paste_scratch", resample)
        need = _resample_work_bytes(int(n), int(frame_hw[0]), int(frame_hw[1]), h, w, fid, (xa - x0, ya - y0, xb - xa, yb - ya))
        work = torch.empty((need + 3) // 4, dtype=torch.int32, device=device)
    if spec is not None:
        crop = torch.empty(yb - ya, xb - xa, 3, dtype=torch.uint8, device=device)
        blend_work = torch.empty((_blend_work_bytes(int(n), yb - ya, xb - xa, spec[1]) + 3) // 4, dtype=torch.int32, device=device)
    return ResampleScratch(torch.empty(int(n), yb - ya, xb - xa, 3, dtype=torch.uint8, device=device), work, crop, blend_work)


# ---------------------------------------------------------------------------------------------------------------------------
# multi-band blending of the face into the portrait (`float_img_blend`, include/float_hip.h): what `blend="multiband"` selects
# ---------------------------------------------------------------------------------------------------------------------------
BLEND_MODES = ("multiband",)
BLEND_PLANS_KEPT = 8  # (sizes, rect, inset, levels, device) entries of the mask cache: a clip uses one
_blend_plans = collections.OrderedDict()


def blend_spec(what, blend, inset=None, levels=None, rect=None, feather=None, out_format=None):
    """The checked form of a paste route's blend=, inset=, levels=: None (the feathered paste), or (inset, levels) with their
    defaults filled in from `rect` (host_models.default_feather, host_models.blend_levels; without a rect they stay as given).
    ValueError: an unknown blend; inset or levels without blend; with blend="multiband" a feather (the pyramid has no ramp), I420
    frames, an inset outside 0 ... 16384, levels outside 1 ... 8."""
    if blend is None:
        if inset is not None or levels is not None:
            raise ValueError("%s: inset and levels belong to blend=\"multiband\" (blend is None)" % what)
        return None
    if blend not in BLEND_MODES:
        raise ValueError("%s: blend must be None or \"multiband\" (got %r)" % (what, blend))
    if feather is not None:
        raise ValueError("%s: blend=\"multiband\" takes no feather (got %r): its width is inset=" % (what, feather))
    if out_format == "i420":
        raise ValueError("%s: blend=\"multiband\" leaves RGB frames in this version; convert them (host_models.rgb8_to_i420) or "
                         "paste with blend=None" % what)
    if inset is None and rect is not None:
        inset = host_models.default_feather(rect)
    if inset is not None:
        if isinstance(inset, bool) or int(inset) != inset or not 0 <= int(inset) <= 16384:
            raise ValueError("%s: inset must be 0 ... 16384 (got %r)" % (what, inset))
        inset = int(inset)
    if levels is not None or inset is not None:
        levels = host_models.blend_levels(what, inset if inset is not None else 0, levels)
    return inset, levels


def blend_plan(H, W, rect, inset, levels):
    """float_img_blend_plan: the mask pyramid of a multi-band paste of the box `rect` into an H x W portrait -> (flat int16 host
    tensor, [(h_l, w_l)]): levels + 1 levels over the window back to back, integer for integer host_models.blend_masks.  Host
    arithmetic in the library; no GPU is touched.  The library's refusals are ValueErrors."""
    x0, y0, w, h = (int(v) for v in rect)
    win = paste_window(int(H), int(W), (x0, y0, w, h))
    L = native.lib()
    ints = int(L.float_img_blend_plan_ints(win[3] - win[1], win[2] - win[0], int(levels))) if win is not None else 0
    table = torch.empty(max(ints, 1), dtype=torch.int16)
    native.check(L.float_img_blend_plan(int(H), int(W), x0, y0, w, h, int(inset), int(levels), C.cast(table.data_ptr(), C.POINTER(C.c_int16)),
                                        ints))
    sizes = list(zip(host_models.blend_sizes(win[3] - win[1], int(levels)), host_models.blend_sizes(win[2] - win[0], int(levels))))
    return table[:ints], sizes


def _blend_plan_device(device, H, W, rect, inset, levels):
    """the plan on the device: made and uploaded once per (sizes, rect, inset, levels, device) and kept for the next call"""
    key = (str(device), H, W, tuple(rect), inset, levels)
    plan = _blend_plans.get(key)
    if plan is None:
        plan = blend_plan(H, W, rect, inset, levels)[0].to(device)  # a blocking copy: complete on return
        _blend_plans[key] = plan
        while len(_blend_plans) > BLEND_PLANS_KEPT:
            _blend_plans.popitem(last=False)
    else:
        _blend_plans.move_to_end(key)
    return plan


def _blend_work_bytes(n, hc, wc, levels):
    need = int(native.lib().float_img_blend_work_bytes(n, hc, wc, levels))
    if not need:
        raise ValueError("blend: %d frames over a window of %d x %d with %d levels are outside float_img_blend's limits (sides 1 ... "
                         "16384, levels 1 ... 8)" % (n, hc, wc, levels))
    return need


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
def paste_frames_device(src8, frames8, rect, feather=None, out=None, out_format=None, matrix=None, resample=None, scratch=None, blend=None,
                        inset=None, levels=None):
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
    scratch: a ResampleScratch of paste_scratch for at least T frames (default: torch's allocator, per call).
    blend: None as above; "multiband": float_img_blend joins face and portrait by a Laplacian pyramid instead of the feathered
    ramp - bitwise host_models.paste_multiband_rgb8(src8, frames8, rect, inset, levels, resample).  inset: how far inside the box's
    open sides the hard mask starts (None = host_models.default_feather(rect)); levels: the pyramid's depth, 1 ... 8 (None =
    host_models.blend_levels).  feather must be None and the frames RGB (ValueError).  The face over the window (box & image) is
    formed as the definition forms it - float_img_paste with feather 0 on the window's crop of the portrait, or float_img_resample
    alone when resample= is given (that paste would copy its result) - then 2 levels launches; the mask pyramid is made by
    float_img_blend_plan and kept on the device per (sizes, rect, inset, levels).  A box that misses the image is the plain paste."""
    fmt = paste_format("paste_frames_device", out_format)
    spec = blend_spec("paste_frames_device", blend, inset, levels, rect if len(rect) == 4 else None, feather, fmt)
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
        win = paste_window(H, W, (x0, y0, w, h)) if resample is not None or spec is not None else None
        if win is not None:
            xa, ya, xb, yb = win
            if scratch is None:
                scratch = paste_scratch((H, W), f.shape[1:3], (x0, y0, w, h), T, resample, device, blend, *(spec or (None, None)))
            elif scratch.face.shape[0] < T or tuple(scratch.face.shape[1:]) != (yb - ya, xb - xa, 3) or scratch.face.device != device \
                    or (resample is not None and scratch.work is None):
                raise ValueError("paste_frames_device: scratch was made for another paste (%s for %d frames of the window %r)"
                                 % (tuple(scratch.face.shape), T, win))
            if resample is not None:
                f = resample_frames_device(f, h, w, resample, (xa - x0, ya - y0, xb - xa, yb - ya), out=scratch.face[:T], work=scratch.work)
        if win is not None and spec is not None:
            hc, wc = yb - ya, xb - xa
            need = _blend_work_bytes(T, hc, wc, spec[1])
            if scratch.crop is None or scratch.blend_work is None or scratch.blend_work.numel() * 4 < need:
                raise ValueError("paste_frames_device: scratch was made for another paste (blend=%r, %d levels, %d frames)" % (blend, spec[1], T))
            if resample is None:  # the face over the window: the plain paste at full weight on the window's crop of the portrait
                scratch.crop.copy_(s[ya:yb, xa:xb])
                native.check(L.float_img_paste(C.c_void_p(scratch.crop.data_ptr()), hc, wc, C.c_void_p(f.data_ptr()), T, int(f.shape[1]),
                                               int(f.shape[2]), x0 - xa, y0 - ya, w, h, 0, C.c_void_p(scratch.face.data_ptr()),
                                               native.stream_ptr(device)))
            mask = _blend_plan_device(device, H, W, (x0, y0, w, h), *spec)
            native.check(L.float_img_blend(C.c_void_p(s.data_ptr()), H, W, C.c_void_p(scratch.face.data_ptr()), T, xa, ya, hc, wc, spec[1],
                                           C.c_void_p(mask.data_ptr()), C.c_void_p(scratch.blend_work.data_ptr()),
                                           scratch.blend_work.numel() * 4, C.c_void_p(out.data_ptr()), native.stream_ptr(device)))
            return out
        if win is not None:
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
