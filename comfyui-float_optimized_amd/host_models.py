"""Host-side (PyTorch on ROCm or CPU) producers of the hot path's inputs.  These run ONCE per
clip and are plumbing, not part of the HIP hot path ("OUT OF SCOPE for HIP").
The appearance encoder + Direction, the audio encoder (wav2vec2-base + projection) and the speech-emotion classifier
(wav2vec2-large + head) are NOT here: they are the HIP operators `float_enc_*` / `float_aud_*` (encoder.py / audio.py in
this package).  What is left is tensor plumbing:

  * image / audio pre-processing of the simple node (generate.py:29-39, 69-73), the face-aligned crop (utils/image.py:135-180;
    detector optional) and the band-limited resampler in front of wav2vec2
  * the one-hot emotion vector of a named emotion (FLOAT.py:196-200)
  * the image front end in exact arithmetic (hex_to_rgb8, image_to_rgb8, resize_rgb8): the definition the kernels of
    `float_img_front` (image.py in this package) are held to bit for bit
  * the paste of the generated frames back into the source portrait (paste_alpha, paste_rgb8): the definition the kernel of
    `float_img_paste` is held to bit for bit
  * bicubic and Lanczos resampling of 8-bit frames in Pillow's fixed-point arithmetic (resample_coeffs, resample_rgb8): the
    definition the kernels of `float_img_resample` are held to bit for bit, and what `resample=` selects on the paste routes
  * the planar YUV 4:2:0 frame format in torch integer ops (the definition the decoder's I420 kernels are held to) and a Y4M
    writer for handing such frames to an encoder
  * baseline JPEG in integer arithmetic (jpeg_tables, jpeg_header, jpeg_encode_rgb8: the definition the kernels of
    `float_jpg_encode` are held to bit for bit; numpy, no imaging library) and a Motion-JPEG AVI writer (AviMjpegWriter)
  * lossless PNG in integer arithmetic (png_filter_rows, png_code_lengths, png_encode_rgb8, crc32_combine: the definition the
    kernels of `float_png_encode` are held to bit for bit) and an animated-PNG writer (ApngWriter)
  * the S3FD face detector written from the published network (sfd_forward, sfd_decode_dense, sfd_nms, sfd_detect): the
    definition the kernels of `float_sfd_*` (face.py in this package) are held to, and the FLOAT_AMD_FACE_DETECTOR switch of
    process_img
"""
import fractions
import logging
import math
import os

import torch
import torch.nn.functional as F

logger = logging.getLogger(__name__)


def preprocess_image(image_hwc, size=512):
    """(H,W,3) float in [0,1] (ComfyUI IMAGE item) -> (1,3,size,size) in [-1,1].  The reference resizes
    with cv2.INTER_AREA on uint8 (generate.py:34-39); cv2 is not a dependency here, so area-averaging
    is done with adaptive_avg_pool2d (identical for integer shrink factors) / bilinear when enlarging."""
    x = image_hwc[..., :3].permute(2, 0, 1)[None].float()
    x = (x * 255.0).round().clamp(0, 255)
    if x.shape[-1] != size or x.shape[-2] != size:
        if x.shape[-1] >= size and x.shape[-2] >= size:
            x = F.adaptive_avg_pool2d(x, (size, size))
        else:
            x = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)
    return x / 127.5 - 1.0


RGBA_CONVERSIONS = ("discard_alpha", "blend_with_color", "replace_with_color")


def hex_to_rgb8(hex_color):
    """'#RRGGBB' -> (R, G, B) in 0 ... 255 (the reference's hex_to_rgb_uint8, utils/image.py:25-35): a string that is not six
    hexadecimal digits after the leading '#'s gives (0, 0, 0) and a logged warning."""
    h = str(hex_color).lstrip("#")
    if len(h) != 6:
        logger.warning("Invalid hex color string: %r. Defaulting to black." % (h,))
        return (0, 0, 0)
    try:
        return tuple(int(h[i:i + 2], 16) for i in (0, 2, 4))
    except ValueError:
        logger.warning("Invalid characters in hex color string: %r. Defaulting to black." % (h,))
        return (0, 0, 0)


def _quant8(x):
    """clip(x * 255.0, 0, 255) in fp32, truncated towards zero (img_tensor_2_np_array, utils/image.py:123); NaN gives 0 - the
    reference leaves that cast undefined, 0 is this project's choice."""
    t = x.float() * 255.0
    return torch.where(torch.isnan(t), torch.zeros_like(t), t).clamp(0.0, 255.0).to(torch.uint8)


def image_to_rgb8(img, rgba_conversion="blend_with_color", bkg_rgb8=(0, 0, 0)):
    """(H, W, 3|4) float (a ComfyUI IMAGE item) -> (H, W, 3) uint8: the reference's img_tensor_2_np_array +
    convert_rgba_to_rgb_numpy (utils/image.py:38-131), bitwise (tests/golden/img_front.npz holds the reference's own outputs).
    Every channel, alpha included, is quantised first (_quant8).  With 4 channels:
      discard_alpha       the RGB as it is
      replace_with_color  the background colour where the quantised alpha is 0
      blend_with_color    rgb * (a / 255.0) + bkg * (1.0 - a / 255.0) in fp32, every operation rounded on its own (no fused
                          multiply-add), clipped to 0 ... 255 and truncated
      anything else       a logged warning, then discard_alpha - as in the reference.
    Torch on the CPU; this is the definition `float_img_front` is held to, as rgb8_to_i420 is for the I420 kernels."""
    if img.dim() != 3 or img.shape[-1] not in (3, 4) or not img.is_floating_point():
        raise ValueError("image_to_rgb8 takes an (H, W, 3) or (H, W, 4) float image, got %s %s" % (img.dtype, tuple(img.shape)))
    q = _quant8(img.detach().cpu())
    if q.shape[-1] == 3:
        return q
    rgb, a = q[..., :3], q[..., 3]
    if rgba_conversion == "discard_alpha":
        return rgb.contiguous()
    bkg = torch.tensor([int(c) for c in bkg_rgb8], dtype=torch.uint8)
    if rgba_conversion == "replace_with_color":
        return torch.where((a == 0)[..., None], bkg, rgb)
    if rgba_conversion == "blend_with_color":
        af = (a.float() / 255.0)[..., None]
        fg = rgb.float() * af
        bg = bkg.float() * (1.0 - af)
        return (fg + bg).clamp(0.0, 255.0).to(torch.uint8)
    logger.warning("Unknown RGBA conversion strategy: %r. Defaulting to 'discard_alpha'." % (rgba_conversion,))
    return rgb.contiguous()


def _axis_scale(n, dst, scale):
    num, den = (int(scale[0]), int(scale[1])) if scale is not None else (int(n), int(dst))
    if num < 1 or den < 1:
        raise ValueError("resize_rgb8: scale %d / %d must be positive" % (num, den))
    g = math.gcd(num, den)
    P, Q = num // g, den // g
    if (dst - 1) * P >= n * Q:
        raise ValueError("resize_rgb8: destination cell %d starts outside the window (extent %d at scale %d / %d)" % (dst - 1, n, P, Q))
    return P, Q


def _area_axis(x, axis, n, dst, P, Q):
    """sum over the samples of a cell of v * (integer length of the overlap), per destination cell; also the cell lengths"""
    x = x.movedim(axis, 0)
    out = torch.zeros((dst,) + tuple(x.shape[1:]), dtype=torch.int64)
    lens = torch.zeros(dst, dtype=torch.int64)
    for d in range(dst):
        c0, c1 = d * P, min((d + 1) * P, n * Q)
        lo, hi = c0 // Q, -((-c1) // Q)  # samples lo ... hi - 1 overlap the cell
        i = torch.arange(lo, hi, dtype=torch.int64)
        w = torch.minimum((i + 1) * Q, torch.tensor(c1)) - torch.maximum(i * Q, torch.tensor(c0))
        out[d] = (x[lo:hi] * w.reshape((-1,) + (1,) * (x.dim() - 1))).sum(dim=0)
        lens[d] = c1 - c0
    return out.movedim(0, axis), lens


def _linear_axis(x, axis, n, dst, P, Q):
    """v[sx] * (P - f) + v[min(sx + 1, n - 1)] * f per destination index (cv2's INTER_AREA magnification taps, in integers)"""
    d = torch.arange(dst, dtype=torch.int64)
    sx = (d * P) // Q
    num = (d + 1) * P - (sx + 1) * Q
    f = torch.where(num <= 0, torch.zeros_like(num), num % P)
    f = torch.where(sx >= n - 1, torch.zeros_like(f), f)
    sx = sx.clamp(max=n - 1)
    s1 = (sx + 1).clamp(max=n - 1)
    x = x.movedim(axis, 0)
    shape = (-1,) + (1,) * (x.dim() - 1)
    out = x[sx] * (P - f).reshape(shape) + x[s1] * f.reshape(shape)
    return out.movedim(0, axis)


def resize_rgb8(rgb8, rect=None, dst_h=None, dst_w=None, scale=None):
    """(H, W, 3) uint8 -> (dst_h, dst_w, 3) uint8: an exact area resize of a window of the image, in 64-bit integers - what
    cv2.resize(..., INTER_AREA) of the reference computes in fp32 / fixed point (generate.py:35, utils/image.py:144,178).
      rect = (x0, y0, w, h): the window in source coordinates (default: the whole image).  It may reach outside the image;
        samples there are 0 in all three channels (cv2.copyMakeBorder(value=0) of process_img).
      Scale per axis, a rational P / Q reduced by the gcd: w / dst_w and h / dst_h, or scale = (P, Q) on both axes (the
        fx = fy form of the detector's 360-px copy).  With n the window's extent, source sample i covers [i Q, (i + 1) Q).
      Area rule (P >= Q on both axes): destination cell d covers [d P, min((d + 1) P, n Q)), a sample's weight is the integer
        length of the overlap, out = sum(v wx wy) / (cell length x * cell length y), rounded half to even.
      Linear rule (P < Q on either axis, then on both - cv2's INTER_AREA magnification branch): sx = floor(d P / Q),
        num = (d + 1) P - (sx + 1) Q, f = 0 if num <= 0 else num mod P; if sx >= n - 1 then sx = n - 1, f = 0; taps (sx, P - f)
        and (min(sx + 1, n - 1), f); out = sum(v wx wy) / (Px Py), rounded half to even.
    Every destination cell must start inside the window.  Torch on the CPU; with image_to_rgb8 the definition
    `float_img_front` is held to bit for bit.  cv2 itself accumulates in fp32 (area) and 11-bit fixed point (linear) and can
    land one level away near a tie: parity with the package is not pinned."""
    if rgb8.dtype != torch.uint8 or rgb8.dim() != 3 or rgb8.shape[-1] != 3:
        raise ValueError("resize_rgb8 takes an (H, W, 3) uint8 image, got %s %s" % (rgb8.dtype, tuple(rgb8.shape)))
    H, W = int(rgb8.shape[0]), int(rgb8.shape[1])
    x0, y0, w, h = (0, 0, W, H) if rect is None else (int(v) for v in rect)
    dst_h, dst_w = int(dst_h), int(dst_w)
    if w < 1 or h < 1 or dst_h < 1 or dst_w < 1:
        raise ValueError("resize_rgb8: window %d x %d and destination %d x %d must be at least 1 x 1" % (h, w, dst_h, dst_w))
    Px, Qx = _axis_scale(w, dst_w, scale)
    Py, Qy = _axis_scale(h, dst_h, scale)
    win = torch.zeros(h, w, 3, dtype=torch.int64)  # the zero-bordered window
    ya, yb, xa, xb = max(0, y0), min(H, y0 + h), max(0, x0), min(W, x0 + w)
    if yb > ya and xb > xa:
        win[ya - y0:yb - y0, xa - x0:xb - x0] = rgb8[ya:yb, xa:xb].cpu().to(torch.int64)
    if Px < Qx or Py < Qy:
        S = _linear_axis(_linear_axis(win, 1, w, dst_w, Px, Qx), 0, h, dst_h, Py, Qy)
        D = torch.full((dst_h, dst_w, 1), Px * Py, dtype=torch.int64)
    else:
        rows, lx = _area_axis(win, 1, w, dst_w, Px, Qx)
        S, ly = _area_axis(rows, 0, h, dst_h, Py, Qy)
        D = (ly[:, None] * lx[None, :])[..., None]
    q = S // D
    r2 = 2 * (S - q * D)
    return (q + ((r2 > D) | ((r2 == D) & (q % 2 == 1))).to(torch.int64)).to(torch.uint8)


def rgb8_to_model_input(q):
    """(H, W, 3) uint8 -> (1, 3, H, W) fp32 in [-1, 1]: q / 127.5 - 1.0 in fp32 (CustomTransform, generate.py:36-38)."""
    return (q.float() / 127.5 - 1.0).permute(2, 0, 1)[None].contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# bicubic and Lanczos resampling: Pillow's Image.resize for 8-bit images, restated.  What `resample=` puts in the place of
# resize_rgb8 on the paste routes; the front end keeps its own rule.
# ---------------------------------------------------------------------------------------------------------------------------
RESAMPLE_FILTERS = {"bicubic": 0, "lanczos": 1}  # name -> FLOAT_IMG_FILTER_*
RESAMPLE_PRECISION_BITS = 22                     # coefficients are integers in units of 2^-22
RESAMPLE_MAX_KSIZE = 255                         # the most taps of one output sample (shrinking by about 42 x with Lanczos)
_RESAMPLE_SUPPORT = (2.0, 3.0)


def resample_filter_id(what, filter):
    """"bicubic" | "lanczos" -> 0 | 1; anything else is a ValueError that names the caller."""
    if not isinstance(filter, str) or filter not in RESAMPLE_FILTERS:
        raise ValueError("%s: resample filter must be one of %s (got %r)" % (what, ", ".join(sorted(RESAMPLE_FILTERS)), filter))
    return RESAMPLE_FILTERS[filter]


def _bicubic_filter(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos_filter(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def resample_ksize(n_in, n_out, filter):
    """The slots a table row holds for its coefficients: int(ceil(support)) * 2 + 1, support = S * max(n_in / n_out, 1)."""
    fid = resample_filter_id("resample_ksize", filter)
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("resample_ksize: sizes %d -> %d must be at least 1" % (n_in, n_out))
    ksize = int(math.ceil(_RESAMPLE_SUPPORT[fid] * max(n_in / n_out, 1.0))) * 2 + 1
    if ksize > RESAMPLE_MAX_KSIZE:
        raise ValueError("resample: %d -> %d with the %s filter needs %d taps per sample, more than %d" % (n_in, n_out, filter, ksize,
                                                                                                          RESAMPLE_MAX_KSIZE))
    return ksize


def resample_coeffs(n_in, n_out, filter, first=0, count=None):
    """One axis of Pillow's Image.resize (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc) for output indices
    first ... first + count - 1 of n_out (default: all) -> (xmin, n, k): int64 tensors of shape (count,), (count,), (count, ksize).
        scale = n_in / n_out;  fs = max(scale, 1.0);  support = S * fs  (S = 2 bicubic, 3 lanczos);  ss = 1.0 / fs
        ksize = int(ceil(support)) * 2 + 1
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5));  xmax = min(n_in, int(center + support + 0.5));  n = xmax - xmin
        w[x] = f((x + xmin - center + 0.5) * ss), x = 0 ... n - 1;  ww = their sum in that order;  w[x] /= ww if ww != 0
        k[x] = int(-0.5 + w[x] * 2^22) if w[x] < 0 else int(0.5 + w[x] * 2^22)   (int truncates toward zero);  k[x] = 0 for x >= n
        bicubic (a = -0.5): |x| < 1: ((a + 2) x - (a + 3)) x x + 1;  |x| < 2: (((x - 5) x + 8) x - 4) a;  else 0
        lanczos: -3 <= x < 3: sinc(x) sinc(x / 3) with sinc(0) = 1, sinc(x) = sin(pi x) / (pi x);  else 0
    in Python floats (IEEE double) with math.sin and math.pi: the libm Pillow and float_img_resample_plan call.  An output
    sample of the axis is clamp((2^21 + sum_x k[x] in[xmin + x]) >> 22, 0, 255); 255 sum|k| + 2^21 < 2^31 is asserted for every
    row, so 32-bit accumulators hold it.  ValueError: an unknown filter, a size below 1, a range outside 0 ... n_out, or more than
    255 taps (shrinking by more than about 42 x)."""
    fid = resample_filter_id("resample_coeffs", filter)
    resample_ksize(n_in, n_out, filter)  # the refusals
    n_out, first = int(n_out), int(first)
    count = n_out - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > n_out:
        raise ValueError("resample_coeffs: indices %d ... %d lie outside 0 ... %d" % (first, first + count, n_out))
    return _resample_table(int(n_in), n_out, fid, first, count)


def _resample_table(n_in, n_out, fid, first, count):
    """the rule of resample_coeffs itself, at any number of taps"""
    f = (_bicubic_filter, _lanczos_filter)[fid]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = _RESAMPLE_SUPPORT[fid] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    one = float(1 << RESAMPLE_PRECISION_BITS)
    xmins, ns, ks = [], [], []
    for xx in range(first, first + count):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        n = min(n_in, int(center + support + 0.5)) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        assert 255 * sum(abs(v) for v in k) + (1 << (RESAMPLE_PRECISION_BITS - 1)) < 1 << 31, (n_in, n_out, fid, xx)
        xmins.append(xmin), ns.append(n), ks.append(k + [0] * (ksize - n))
    return (torch.tensor(xmins, dtype=torch.int64), torch.tensor(ns, dtype=torch.int64),
            torch.tensor(ks, dtype=torch.int64).reshape(count, ksize))


def _resample_axis(x, axis, coeffs):
    """one pass over `axis` of an int64 tensor of 8-bit samples -> the same, the axis as long as the table"""
    xmin, n, k = coeffs
    x = x.movedim(axis, 0)
    idx = (xmin[:, None] + torch.arange(k.shape[1], dtype=torch.int64)[None, :]).clamp(max=x.shape[0] - 1)  # k is 0 beyond n
    acc = torch.full((k.shape[0],) + tuple(x.shape[1:]), 1 << (RESAMPLE_PRECISION_BITS - 1), dtype=torch.int64)
    for j in range(k.shape[1]):
        acc += x[idx[:, j]] * k[:, j].reshape((-1,) + (1,) * (x.dim() - 1))
    return (acc >> RESAMPLE_PRECISION_BITS).clamp(0, 255).movedim(0, axis)  # >> on a negative int64 is the arithmetic shift


def resample_window(what, h, w, window):
    """window = (xa, ya, wc, hc) of an h x w result, checked; None is the whole."""
    if window is None:
        return 0, 0, int(w), int(h)
    if len(window) != 4:
        raise ValueError("%s: window must be (xa, ya, wc, hc), got %r" % (what, window))
    xa, ya, wc, hc = (int(v) for v in window)
    if xa < 0 or ya < 0 or wc < 1 or hc < 1 or xa + wc > w or ya + hc > h:
        raise ValueError("%s: window %r lies outside the %d x %d result" % (what, tuple(window), h, w))
    return xa, ya, wc, hc


def resample_rgb8(frames8, h, w, filter, window=None):
    """(T, h_f, w_f, 3) uint8 -> (T, h, w, 3) uint8: Pillow's Image.resize((w, h), BICUBIC | LANCZOS) of every frame, bit for bit
    (tests/test_img_resample.py holds it to Pillow itself).  filter: "bicubic" | "lanczos".  The horizontal pass comes first and
    gives an 8-bit intermediate, the vertical pass follows; a pass whose two sizes are equal is skipped.  window = (xa, ya, wc,
    hc): only that part of the (h, w) result, (T, hc, wc, 3) - every output sample is independent, so it is the slice of the
    whole, and the whole is never formed (a box may be far larger than the image it is pasted into).  The definition
    `float_img_resample` (image.resample_frames_device) is held to bit for bit."""
    resample_filter_id("resample_rgb8", filter)
    if frames8.dtype != torch.uint8 or frames8.dim() != 4 or frames8.shape[-1] != 3 or 0 in frames8.shape:
        raise ValueError("resample_rgb8 takes (T, h, w, 3) uint8 frames, got %s %s" % (frames8.dtype, tuple(frames8.shape)))
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("resample_rgb8: the result %d x %d must be at least 1 x 1" % (h, w))
    xa, ya, wc, hc = resample_window("resample_rgb8", h, w, window)
    h_f, w_f = int(frames8.shape[1]), int(frames8.shape[2])
    cx = resample_coeffs(w_f, w, filter, xa, wc) if w != w_f else None
    cy = resample_coeffs(h_f, h, filter, ya, hc) if h != h_f else None
    x = frames8.cpu().to(torch.int64)
    if cy is not None:  # only the rows the window's rows reference go through the horizontal pass
        r0, r1 = int(cy[0].min()), int((cy[0] + cy[1]).max())
        x, cy = x[:, r0:r1], (cy[0] - r0, cy[1], cy[2])
    else:
        x = x[:, ya:ya + hc]
    x = _resample_axis(x, 2, cx) if cx is not None else x[:, :, xa:xa + wc]
    if cy is not None:
        x = _resample_axis(x, 1, cy)
    return x.to(torch.uint8).contiguous()


def default_feather(rect):
    """The feather a caller gets who passes None: rect_w // 16 source pixels.  A visual choice, not a measurement - there is no
    checkpoint here to judge a seam on."""
    return max(0, int(rect[2]) // 16)


def paste_alpha(H, W, rect, feather):
    """(h, w) int64: the weight 0 ... 255 of the generated face in every cell of the box `rect` = (x0, y0, w, h) over an H x W
    image.  d = the cell's distance to the nearest OPEN side of the box (u, w - 1 - u, v, h - 1 - v); a side is open only where
    the box edge lies strictly inside the image (x0 > 0, x0 + w < W, y0 > 0, y0 + h < H) - a side on or beyond the image's edge
    does not feather, so no static rim of the source sits at the picture's border and rect = whole image is a plain resize.
    a = min(255, 255 (d + 1) // (feather + 1)); no open side or feather == 0 gives 255."""
    x0, y0, w, h = (int(v) for v in rect)
    f = int(feather)
    big = 1 << 30

    def axis(n, lo_open, hi_open):
        u = torch.arange(n, dtype=torch.int64)
        return torch.minimum(u if lo_open else torch.full_like(u, big), (n - 1 - u) if hi_open else torch.full_like(u, big))

    d = torch.minimum(axis(h, y0 > 0, y0 + h < H)[:, None], axis(w, x0 > 0, x0 + w < W)[None, :])
    return torch.clamp((255 * (d + 1)) // (f + 1), max=255)


def paste_rgb8(src8, frames8, rect, feather, resample=None):
    """The generated frames back in the source portrait: src8 (H, W, 3) uint8, frames8 (T, h_f, w_f, 3) uint8, rect = (x0, y0, w,
    h) in source coordinates (it may reach outside the image or miss it), feather >= 0 in source pixels -> (T, H, W, 3) uint8.
      outside rect & image   out[t] = src8
      inside                 face = resize_rgb8(frames8[t], None, h, w) - the rule of the image front end unchanged, already
                             rounded to 8 bits - and out = (a face + (255 - a) src + 127) // 255 with a = paste_alpha (255 is odd:
                             no ties, this is round-to-nearest).
    The parts of the generated frame that map outside the image are discarded: they are the zero border the model was shown.
    resample: None as above; "bicubic" | "lanczos": face = resample_rgb8(frames8[t], h, w, resample) - Pillow's filter, sharper
    where the box is larger than the frame - in the place of the resize_rgb8 call; alpha, blend and the discard are unchanged.
    Integer arithmetic in torch on the CPU; the definition `float_img_paste` (image.paste_frames_device) is held to bit for
    bit, as resize_rgb8 is for the front end."""
    if src8.dtype != torch.uint8 or src8.dim() != 3 or src8.shape[-1] != 3:
        raise ValueError("paste_rgb8 takes an (H, W, 3) uint8 source, got %s %s" % (src8.dtype, tuple(src8.shape)))
    if frames8.dtype != torch.uint8 or frames8.dim() != 4 or frames8.shape[-1] != 3 or 0 in frames8.shape:
        raise ValueError("paste_rgb8 takes (T, h, w, 3) uint8 frames, got %s %s" % (frames8.dtype, tuple(frames8.shape)))
    if len(rect) != 4:
        raise ValueError("paste_rgb8: rect must be (x0, y0, w, h), got %r" % (rect,))
    if resample is not None:
        resample_filter_id("paste_rgb8", resample)
    x0, y0, w, h = (int(v) for v in rect)
    f = int(feather)
    if w < 1 or h < 1 or f < 0 or src8.shape[0] < 1 or src8.shape[1] < 1:
        raise ValueError("paste_rgb8: box %d x %d and source %d x %d must be at least 1 x 1, feather (%d) >= 0"
                         % (h, w, src8.shape[0], src8.shape[1], f))
    H, W = int(src8.shape[0]), int(src8.shape[1])
    src8, frames8 = src8.cpu(), frames8.cpu()
    out = src8[None].repeat(frames8.shape[0], 1, 1, 1)
    ya, yb, xa, xb = max(0, y0), min(H, y0 + h), max(0, x0), min(W, x0 + w)
    if yb <= ya or xb <= xa:
        return out
    a = paste_alpha(H, W, (x0, y0, w, h), f)[ya - y0:yb - y0, xa - x0:xb - x0, None]
    s = src8[ya:yb, xa:xb].to(torch.int64)
    if resample is not None:  # the window of the box that lies in the image, never the whole box
        faces = resample_rgb8(frames8, h, w, resample, (xa - x0, ya - y0, xb - xa, yb - ya)).to(torch.int64)
    for t in range(frames8.shape[0]):
        if resample is not None:
            face = faces[t]
        else:
            face = resize_rgb8(frames8[t], None, h, w)[ya - y0:yb - y0, xa - x0:xb - x0].to(torch.int64)
        out[t, ya:yb, xa:xb] = ((a * face + (255 - a) * s + 127) // 255).to(torch.uint8)
    return out


def resample_sinc(w, orig_rate, new_rate, zeros=24, rolloff=0.945):
    """Band-limited polyphase resampling of a 1-D waveform (Hann-windowed sinc, `zeros` zero crossings per side, cut-off at
    `rolloff` x the lower Nyquist): the anti-alias low-pass the reference gets from librosa's soxr_hq
    (utils/audio.py -> librosa.resample), which plain linear interpolation lacks - without it everything between 8 kHz and
    the source Nyquist folds into the wav2vec2 band when ComfyUI hands over 44.1 / 48 kHz audio."""
    orig_rate, new_rate = int(orig_rate), int(new_rate)
    if orig_rate == new_rate:
        return w
    g = math.gcd(orig_rate, new_rate)
    up, down = new_rate // g, orig_rate // g
    if up * (2 * int(math.ceil(zeros * max(up, down) / (min(up, down) * rolloff))) + down) > 2e7:
        # near-coprime rates (44099 -> 16000: up 16000, 44k taps per phase = 5.6 GB of kernel): quantise the source rate to
        # the nearest multiple of 50 Hz by a linear-interpolation pre-pass (error band far above the wav2vec2 band's needs:
        # a ratio change of <= 0.06 %), then run the polyphase filter at the friendly ratio
        snapped = max(50, int(round(orig_rate / 50.0)) * 50)
        if snapped != orig_rate:
            n_mid = max(1, int(round(w.shape[-1] * snapped / float(orig_rate))))
            w = F.interpolate(w[None, None].double(), size=n_mid, mode="linear", align_corners=False)[0, 0].to(w.dtype)
            return resample_sinc(w, snapped, new_rate, zeros, rolloff)
        # the SOURCE rate is friendly already, the TARGET is not (44100 -> 16001): filter to the nearest multiple of 50 Hz of
        # the target, then a linear-interpolation post-pass of <= 0.16 % (the signal is band-limited below it by then)
        tgt = max(50, int(round(new_rate / 50.0)) * 50)
        if tgt == new_rate:
            raise ValueError("cannot build a polyphase resampler for %d -> %d Hz" % (orig_rate, new_rate))
        y = resample_sinc(w, orig_rate, tgt, zeros, rolloff)
        n_out = max(1, int(math.ceil(w.shape[-1] * new_rate / float(orig_rate))))
        return F.interpolate(y[None, None].double(), size=n_out, mode="linear", align_corners=False)[0, 0].to(w.dtype)
    base = min(up, down) * rolloff          # cut-off in units of the common rate's Nyquist / max(up, down)
    width = int(math.ceil(zeros * down / base))
    # kernel[phase p of `up`, tap k]: output sample n * up + p reads input samples around n * down + p * down / up
    idx = torch.arange(-width, width + down, dtype=torch.float64)[None, :] / down
    ph = -torch.arange(up, dtype=torch.float64)[:, None] / up
    t = (idx + ph) * base
    t = t.clamp(-zeros, zeros)
    win = torch.cos(t * math.pi / zeros / 2) ** 2
    tpi = t * math.pi
    ker = torch.where(tpi == 0, torch.ones_like(tpi), torch.sin(tpi) / tpi) * win * (base / down)
    ker = ker.to(w.dtype)[:, None, :]
    n = w.shape[-1]
    x = F.pad(w[None, None], (width, width + down))
    y = F.conv1d(x, ker, stride=down)       # (1, up, frames)
    y = y.transpose(1, 2).reshape(-1)
    return y[: int(math.ceil(n * up / down))]


def resample_sinc_direct(w, orig_rate, new_rate, zeros=24, rolloff=0.945):
    """The closed form of what `resample_sinc` computes, in fp64 torch ops for ANY pair of rates (no polyphase table, so
    nothing is snapped): with g = gcd, up = new_rate / g, down = orig_rate / g, c = rolloff * min(1, up / down),
        y[m] = sum_j w[j] * sinc(t) * cos^2(pi t / (2 zeros)) * c,   t = clamp((j - m * down / up) * c, -zeros, zeros),
    for m = 0 ... ceil(n * up / down) - 1, w zero outside the clip.  The definition `float_aud_front` (the resampler on the
    device, audio.preprocess_audio_device) is held to, as rgb8_to_i420 is for the I420 kernels.  Returns fp64; equal rates
    return the input unchanged, like resample_sinc."""
    orig_rate, new_rate = int(orig_rate), int(new_rate)
    if orig_rate == new_rate:
        return w
    g = math.gcd(orig_rate, new_rate)
    up, down = new_rate // g, orig_rate // g
    c = rolloff * min(1.0, up / down)
    W = int(math.ceil(zeros / c))                    # taps j = q - W ... q + W + 1 cover every |j - pos| <= zeros / c
    n = w.shape[-1]
    n_out = -((-n * up) // down)
    x = F.pad(w.double(), (W, W + 2))                # x[j + W] = w[j]
    k = torch.arange(-W, W + 2, dtype=torch.int64)
    out = torch.empty(n_out, dtype=torch.float64, device=w.device)
    step = max(1, (1 << 22) // k.numel())
    for m0 in range(0, n_out, step):
        num = torch.arange(m0, min(m0 + step, n_out), dtype=torch.int64) * down  # exact integers: pos = q + r / up
        q, r = num // up, num % up
        t = ((k[None, :] * up - r[:, None]).double() / up * c).clamp(-zeros, zeros)
        tpi = t * math.pi
        ker = torch.where(tpi == 0, torch.ones_like(tpi), torch.sin(tpi) / tpi) * torch.cos(tpi / (2 * zeros)) ** 2 * c
        out[m0:m0 + step] = (x[(q[:, None] + (k[None, :] + W)).to(x.device)] * ker.to(x.device)).sum(dim=1)
    return out


def preprocess_audio(waveform, sample_rate, target_rate=16000, device=None):
    """ComfyUI AUDIO item (C,N) -> mono 16 kHz, zero-mean / unit-variance like
    Wav2Vec2FeatureExtractor(do_normalize=True) (generate.py:69-73).  A different source rate goes through a band-limited
    resampler (the reference: librosa soxr_hq)."""
    w = waveform
    if device is not None and sample_rate == target_rate:
        w = w.to(device, non_blocking=True)  # nothing to resample: mono mix and normalisation run where the encoder runs
    w = w.float()
    if w.dim() == 2:
        w = w.mean(dim=0)
    if sample_rate != target_rate:
        w = resample_sinc(w, sample_rate, target_rate)  # on the waveform's own device (the host for a ComfyUI AUDIO item)
    if device is not None:
        w = w.to(device, non_blocking=True)
    return ((w - w.mean()) / torch.sqrt(w.var(unbiased=False) + 1e-7))[None]


def process_img_view(img_hwc, front=None):
    """The 360-px-high uint8 copy of the image that process_img shows its detector (utils/image.py:142-146): `front(360)` for an
    image more than 360 px high when `front` is given, else the host resize (area down, bicubic up).  A caller that aligns a
    batch of portraits makes the views with this, runs the detector on all of them at once and hands process_img the rows."""
    mult = 360.0 / int(img_hwc.shape[0])
    if front is not None and mult < 1.0:
        return front(360)
    small = F.interpolate(img_hwc.permute(2, 0, 1)[None], scale_factor=mult, mode="area" if mult < 1.0 else "bicubic")
    return (small[0].permute(1, 2, 0).clamp(0, 1) * 255).round().to(torch.uint8)


def process_img(img_hwc, input_size, margin=1.6, index=1, logger=None, front=None, detector=None):
    """The reference's face-aligned crop (utils/image.py:135-180) on an (H,W,3) float image in [0,1]: detect faces on a
    360-px-high copy, take box `index`, crop a square of `margin` x the larger half side around its centre from the
    zero-bordered image, resize to input_size.  The detector (`face_alignment`, SFD) is an optional dependency: without it
    - or when it finds no face, exactly like the reference (utils/image.py:151-158) - the centre square is cropped and a
    warning is logged.  Returns (crop (S,S,3) float in [0,1], bbox (x, y, w, h)).
    front: a callable view_h -> the (view_h, round(W view_h / H), 3) uint8 copy of the image for the detector
    (image.detector_view_device of the image on the device).  With it, for an image more than 360 px high, that copy is the
    only thing that reaches the host, nothing is cropped or resized here (only the shape of img_hwc is read), and the function
    returns (rect, bbox): rect = (x0, y0, w, h), the crop window in source coordinates, which may reach outside the image -
    what image.preprocess_image_device takes.  Images of 360 px height or less (the reference's INTER_CUBIC route) ignore
    `front` and take the host route above.
    detector: a callable view -> [[x1, y1, x2, y2, score], ...] on the (view_h, view_w, 3) uint8 view (a device tensor on the
    `front` route, a host tensor otherwise) - the device detector (face.FaceDetectorHIP.detect); a caller passes it only where
    its weight file exists (face.find_sfd_weights).  FLOAT_AMD_FACE_DETECTOR (face_detector_mode, read per call) chooses:
    auto = the `face_alignment` package if it can be built, else `detector` if given, else the centre square with a warning;
    device = `detector` (ValueError without one); package = the package alone; off = the centre square.  detector=None with
    the switch unset is the code path as it was before the switch."""
    H, Wd = int(img_hwc.shape[0]), int(img_hwc.shape[1])
    mult = 360.0 / H
    use_front = front is not None and mult < 1.0
    bboxes = None
    fa = None
    mode = face_detector_mode()
    if mode == "device" and detector is None:
        raise ValueError("FLOAT_AMD_FACE_DETECTOR=device, but this call has no device detector (process_img(detector=...))")
    if mode in ("auto", "package"):
        try:  # ANY failure to obtain a detector (package absent, a stub or broken install, model files unreachable) takes the
            fa = _face_detector()  # reference's no-face branch below instead of failing the node at its default face_align=True
        except Exception as e:  # noqa: BLE001
            if (mode == "package" or detector is None) and logger is not None:
                logger.warning("face_align=True, but no face detector is available (%s: %s): no face detection, the centre square "
                               "of the image is used (install face_alignment for the reference's crop).  %s"
                               % (type(e).__name__, e, SFD_WEIGHTS_HINT))
    use_device = fa is None and detector is not None and mode in ("auto", "device")
    if fa is not None or use_device:
        import numpy as np
        small = process_img_view(img_hwc, front)
        if use_device:
            det = detector(small)
        else:
            det = fa.face_detector.detect_from_image(np.ascontiguousarray(small.cpu().numpy()))
        bboxes = [(int(x1 / mult), int(y1 / mult), int(x2 / mult), int(y2 / mult), sc) for (x1, y1, x2, y2, sc) in (det or []) if sc > 0.95]
    if not bboxes:
        if bboxes is not None and logger is not None:
            logger.warning("Failed to detect any face in the image, no face align performed")
        my, mx = H // 2, Wd // 2
        bs = min(mx, my)
        bbox_r = (mx - bs, my - bs, 2 * bs, 2 * bs)
        img = img_hwc
    else:
        if index > len(bboxes):
            if logger is not None:
                logger.warning("Only %d detected, using the first one" % len(bboxes))
            index = 1
        b = bboxes[index - 1]
        bsy, bsx = int((b[3] - b[1]) / 2), int((b[2] - b[0]) / 2)
        my, mx = int((b[1] + b[3]) / 2), int((b[0] + b[2]) / 2)
        bs = int(max(bsy, bsx) * margin)
        bbox_r = (mx - bs, my - bs, 2 * bs, 2 * bs)
        if not use_front:
            img = F.pad(img_hwc.permute(2, 0, 1), (bs, bs, bs, bs)).permute(1, 2, 0)  # cv2.copyMakeBorder(..., value=0)
        my, mx = my + bs, mx + bs
    if use_front:
        return bbox_r, bbox_r  # the crop is the window bbox_r of the zero-bordered image in both branches
    crop = img[my - bs:my + bs, mx - bs:mx + bs]
    if crop.shape[0] != input_size or crop.shape[1] != input_size:
        c = crop.permute(2, 0, 1)[None].float()
        if mult < 1.0 and c.shape[-1] >= input_size:
            c = F.adaptive_avg_pool2d(c, (input_size, input_size))      # cv2.INTER_AREA
        else:
            c = F.interpolate(c, size=(input_size, input_size), mode="bicubic", align_corners=False).clamp(0, 1)  # INTER_CUBIC
        crop = c[0].permute(1, 2, 0)
    return crop, bbox_r


_FA = None


def _face_detector():
    global _FA
    if _FA is None:
        import face_alignment
        _FA = face_alignment.FaceAlignment(face_alignment.LandmarksType.TWO_D, flip_input=False)
    return _FA


# ---------------------------------------------------------------------------------------------- the S3FD face detector
# Written from the published network (Zhang et al., "S3FD: Single Shot Scale-invariant Face Detector", ICCV 2017; VGG-16 trunk,
# six detection heads) with the state-dict key names and shapes of the `face_alignment` package's s3fd module, so that its weight
# file loads with a strict check.  The package is not a dependency and parity with it is not pinned.
FACE_DETECTOR_MODES = ("auto", "device", "package", "off")
SFD_WEIGHTS_HINT = ("Without the package, the built-in detector takes over once its weight file is at FLOAT_AMD_SFD_WEIGHTS or "
                    "<models>/face_alignment/s3fd.safetensors (also s3fd.pth, s3fd-619a316812.pth, or torch hub's checkpoint cache).")
SFD_MEAN_BGR = (104.0, 117.0, 123.0)
# (name, cin, cout, k, stride, pad); every trunk conv is followed by ReLU, `pool` = max_pool2d(2, 2) in floor mode behind it
SFD_TRUNK = [("conv1_1", 3, 64, 3, 1, 1), ("conv1_2", 64, 64, 3, 1, 1), "pool",
             ("conv2_1", 64, 128, 3, 1, 1), ("conv2_2", 128, 128, 3, 1, 1), "pool",
             ("conv3_1", 128, 256, 3, 1, 1), ("conv3_2", 256, 256, 3, 1, 1), ("conv3_3", 256, 256, 3, 1, 1), "pool",
             ("conv4_1", 256, 512, 3, 1, 1), ("conv4_2", 512, 512, 3, 1, 1), ("conv4_3", 512, 512, 3, 1, 1), "pool",
             ("conv5_1", 512, 512, 3, 1, 1), ("conv5_2", 512, 512, 3, 1, 1), ("conv5_3", 512, 512, 3, 1, 1), "pool",
             ("fc6", 512, 1024, 3, 1, 3), ("fc7", 1024, 1024, 1, 1, 0),
             ("conv6_1", 1024, 256, 1, 1, 0), ("conv6_2", 256, 512, 3, 2, 1),
             ("conv7_1", 512, 128, 1, 1, 0), ("conv7_2", 128, 256, 3, 2, 1)]
# (feature map, channels, L2Norm or not, conf channels) per level; stride of level i = 2^(i + 2)
SFD_LEVELS = [("conv3_3", 256, True, 4), ("conv4_3", 512, True, 2), ("conv5_3", 512, True, 2),
              ("fc7", 1024, False, 2), ("conv6_2", 512, False, 2), ("conv7_2", 256, False, 2)]
SFD_MIN_SIDE, SFD_MAX_SIDE = 16, 4096


def face_detector_mode():
    """FLOAT_AMD_FACE_DETECTOR, read per call: auto (default) | device | package | off."""
    mode = os.environ.get("FLOAT_AMD_FACE_DETECTOR", "auto").strip().lower() or "auto"
    if mode not in FACE_DETECTOR_MODES:
        raise ValueError("FLOAT_AMD_FACE_DETECTOR=%r: one of %s" % (mode, ", ".join(FACE_DETECTOR_MODES)))
    return mode


def sfd_state_shapes():
    """{key: shape} of the s3fd module's state dict: what a weight file must hold, no more and no less."""
    shapes = {}
    for layer in SFD_TRUNK:
        if layer != "pool":
            name, cin, cout, k = layer[:4]
            shapes[name + ".weight"], shapes[name + ".bias"] = (cout, cin, k, k), (cout,)
    for name, c, norm, nconf in SFD_LEVELS:
        head = name + ("_norm" if norm else "")
        if norm:
            shapes[head + ".weight"] = (c,)
        for what, co in (("conf", nconf), ("loc", 4)):
            shapes["%s_mbox_%s.weight" % (head, what)], shapes["%s_mbox_%s.bias" % (head, what)] = (co, c, 3, 3), (co,)
    return shapes


def sfd_check_state(state, where="state dict"):
    """The strict check: a missing or extra key, or a wrong shape, is a ValueError that names it."""
    want = sfd_state_shapes()
    missing, extra = sorted(set(want) - set(state)), sorted(set(state) - set(want))
    if missing or extra:
        raise ValueError("%s is not an s3fd state dict: missing %s, unexpected %s" % (where, missing or "none", extra or "none"))
    for k, shp in want.items():
        if tuple(state[k].shape) != shp:
            raise ValueError("%s: '%s' has shape %s, s3fd has %s" % (where, k, tuple(state[k].shape), shp))
    return state


def sfd_map_sizes(H, W):
    """[(h, w)] of the six feature maps of an H x W view: floor pooling, fc6's growth by 4, the two stride-2 convs."""
    sizes, at = [], {}
    h, w = int(H), int(W)
    for layer in SFD_TRUNK:
        if layer == "pool":
            h, w = h // 2, w // 2
        else:
            name, _, _, k, s, p = layer
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            at[name] = (h, w)
    for name, _, _, _ in SFD_LEVELS:
        sizes.append(at[name])
    return sizes


def _sfd_pool(x):
    if x.shape[-2] < 2 or x.shape[-1] < 2:  # floor mode down to an empty map (torch refuses it): fc6 then sees its padding alone
        return x[:, :, :x.shape[-2] // 2, :x.shape[-1] // 2]
    return F.max_pool2d(x, 2, 2)


def sfd_forward(state, rgb8):
    """The 12 maps of the (H, W, 3) uint8 RGB view: [conf_0 (1,2,h0,w0), loc_0 (1,4,h0,w0), conf_1, ...], after level 0's
    max-out and before the softmax.  Runs in the dtype and on the device of `state`'s tensors (fp32 on the CPU is the
    definition)."""
    w0 = state["conv1_1.weight"]
    H, W = int(rgb8.shape[0]), int(rgb8.shape[1])
    if min(H, W) < SFD_MIN_SIDE or max(H, W) > SFD_MAX_SIDE or rgb8.shape[-1] != 3:
        raise ValueError("the detector's view must be (H, W, 3) with sides in %d ... %d, got %s" % (SFD_MIN_SIDE, SFD_MAX_SIDE, tuple(rgb8.shape)))
    x = torch.as_tensor(rgb8).to(w0.device).float().flip(-1) - torch.tensor(SFD_MEAN_BGR, device=w0.device)
    x = x.permute(2, 0, 1)[None].to(w0.dtype)
    feats = {}
    for layer in SFD_TRUNK:
        if layer == "pool":
            x = _sfd_pool(x)
            continue
        name, _, _, _, s, p = layer
        if p > 1:  # fc6: pad by hand, so that a 0 x 0 map (a side below 32) still gives the 4 x 4 of its padding
            x, p = F.pad(x, (p, p, p, p)), 0
        x = F.relu(F.conv2d(x, state[name + ".weight"], state[name + ".bias"], stride=s, padding=p))
        feats[name] = x
    maps = []
    for i, (name, _, norm, nconf) in enumerate(SFD_LEVELS):
        f, head = feats[name], name + ("_norm" if norm else "")
        if norm:
            f = f / (f.float().pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10).to(f.dtype) * state[head + ".weight"].view(1, -1, 1, 1)
        conf = F.conv2d(f, state[head + "_mbox_conf.weight"], state[head + "_mbox_conf.bias"], padding=1)
        loc = F.conv2d(f, state[head + "_mbox_loc.weight"], state[head + "_mbox_loc.bias"], padding=1)
        if nconf == 4:
            conf = torch.cat([conf[:, :3].max(dim=1, keepdim=True).values, conf[:, 3:4]], dim=1)
        maps += [conf, loc]
    return maps


def sfd_decode_dense(maps):
    """Every position of the 12 maps decoded, in position order (level, y, x): a (P, 5) float64 array of
    [x1, y1, x2, y2, score].  Level i has stride s = 2^(i + 2) - level 3 too, although fc6 enlarged its map, and its
    positions beyond the image are kept; prior centre (s / 2 + x s, s / 2 + y s), prior size 4 s, variances (0.1, 0.2);
    score = softmax(conf)[1] = 1 / (1 + exp(c0 - c1))."""
    import numpy as np
    rows = []
    for i in range(len(maps) // 2):
        conf = maps[2 * i].detach().float().cpu().numpy().astype(np.float64)[0]
        loc = maps[2 * i + 1].detach().float().cpu().numpy().astype(np.float64)[0]
        s = float(2 ** (i + 2))
        h, w = conf.shape[-2:]
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        with np.errstate(over="ignore"):
            score = 1.0 / (1.0 + np.exp(conf[0] - conf[1]))
            bw, bh = 4 * s * np.exp(0.2 * loc[2]), 4 * s * np.exp(0.2 * loc[3])
        cx, cy = s / 2 + xs * s + loc[0] * 0.1 * 4 * s, s / 2 + ys * s + loc[1] * 0.1 * 4 * s
        rows.append(np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2, score], axis=-1).reshape(-1, 5))
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, 5))


def sfd_decode(maps, score_thr):
    """The candidates: rows of sfd_decode_dense with score > score_thr, in position order."""
    dense = sfd_decode_dense(maps)
    return dense[dense[:, 4] > score_thr]


def sfd_nms(boxes, iou_thr):
    """Greedy NMS of (N, 5) rows given in position order: indices in keep order.  Descending score, ties by position ascending
    (a stable sort: what numpy's argsort leaves open); areas and overlaps with the `+1` convention; a box is dropped when its
    IoU with a kept box EXCEEDS iou_thr."""
    import numpy as np
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
    x1, y1, x2, y2, sc = b[:, 0], b[:, 1], b[:, 2], b[:, 3], b[:, 4]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = np.argsort(-sc, kind="stable")
    keep = []
    while order.size > 0:
        i, rest = order[0], order[1:]
        keep.append(int(i))
        w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
        h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
        ovr = w * h / (areas[i] + areas[rest] - w * h)
        order = rest[ovr <= iou_thr]
    return keep


def sfd_select(dense, score_thr=0.5, iou_thr=0.3):
    """Dense rows -> the detections.  The package's detect_from_image takes candidates above 0.05, runs the NMS and then keeps
    score > 0.5; a box's fate in greedy NMS depends on boxes of HIGHER score only, so filtering by a score threshold commutes
    with it: the filter runs first here and the 0.05 pass is dropped (tests/test_face_detect.py states it on random boxes)."""
    cand = dense[dense[:, 4] > score_thr]
    return [[float(v) for v in cand[i]] for i in sfd_nms(cand, iou_thr)]


def sfd_detect(state, rgb8, score_thr=0.5, iou_thr=0.3):
    """[[x1, y1, x2, y2, score], ...] in keep order: what the package's detect_from_image returns for the view."""
    with torch.no_grad():
        return sfd_select(sfd_decode_dense(sfd_forward(state, rgb8)), score_thr, iou_thr)


EMOTION_LABELS = ["angry", "disgust", "fear", "happy", "neutral", "sad", "surprise"]  # FLOAT.py:390


def emotion_index(name):
    """label2id.get(str(emo).lower(), None) of the reference (FLOAT.py:196): None for anything that is not one of the seven
    labels - None itself, 'none', 'S2E' (run_inference's default) ... - which means "predict the scores from the audio"."""
    name = str(name).lower()
    return EMOTION_LABELS.index(name) if name in EMOTION_LABELS else None


def dynamic_emotion_chunk_sec(emo, default_sec=2.0):
    """The chunk length of a dynamic-emotion request, or None: emo == "dynamic" (any case) -> default_sec, ("dynamic", sec) ->
    float(sec), a TUPLE (a list of emo values means one per item wherever a call takes several clips: infer_device_batch).
    Everything else (a label, None, 'none', 'S2E', ...) is not dynamic."""
    if isinstance(emo, list):
        return None
    if isinstance(emo, tuple):
        if len(emo) == 2 and str(emo[0]).lower() == "dynamic":
            return float(emo[1])
        return None
    return float(default_sec) if str(emo).lower() == "dynamic" else None


def dynamic_emotion_plan(n_samples, rate, chunk_sec, fps):
    """(chunk, n_chunks, tail_len, T) of a dynamic-emotion clip, as the reference's FloatExtractEmotionWithCustomModelDyn
    computes them (src/nodes/nodes_vadv.py): chunk = int(chunk_sec * rate) samples per chunk, n_chunks = ceil(n_samples / chunk)
    (the last one tail_len = n_samples - (n_chunks - 1) * chunk samples long, == chunk when it is full) and
    T = ceil(n_samples / rate * fps) video frames."""
    chunk = int(chunk_sec * rate)
    if chunk == 0:
        raise ValueError("Chunk duration is too small for the sample rate.")
    n_samples = int(n_samples)
    n_chunks = math.ceil(n_samples / chunk)
    tail_len = n_samples - (n_chunks - 1) * chunk if n_chunks else 0
    return chunk, n_chunks, tail_len, math.ceil(n_samples / rate * fps)


def nearest_rows(seq, T):
    """F.interpolate(seq.transpose(1, 2), size=T, mode="nearest").transpose(1, 2) for (..., n, C) -> (..., T, C), bitwise: row t
    is row min(int(floor(fp32(t) * fp32(n / T))), n - 1), the scale and the product rounded to fp32 as torch's kernel does (the
    exact integer t * n // T differs for some pairs, e.g. (n, T) = (2, 82)).  The definition float_aud_expand_rows is held to."""
    import numpy as np
    n, T = int(seq.shape[-2]), int(T)
    if n == 1:
        idx = torch.zeros(T, dtype=torch.long)
    else:
        scale = np.float32(n) / np.float32(T)
        idx = torch.from_numpy(np.minimum(np.floor(np.arange(T, dtype=np.float32) * scale).astype(np.int64), n - 1))
    return seq.index_select(-2, idx.to(seq.device))


def emotion_one_hot(name, device="cpu"):
    """One-hot `we` (1,1,7) for a named emotion (FLOAT.py:196-200; float like nodes_adv.py:533-536)."""
    idx = emotion_index(name)
    if idx is None:
        raise ValueError("%r is not one of %s" % (name, EMOTION_LABELS))
    return F.one_hot(torch.tensor(idx, device=device), num_classes=len(EMOTION_LABELS)).float()[None, None]


# The colour matrices of the I420 outputs, by id: rows Y, U, V of (cr, cg, cb, rnd, off) for
#     plane = ((cr * r + cg * g + cb * b + rnd) >> 8) + off        in int32, >> the arithmetic shift (floor)
# The id is a flag word: bit 1 = BT.709, bit 2 = full range.  Every Y row sums to 220 (limited) or 256 (full) and every chroma
# row to 0, so a grey sample gives exactly U = V = 128 (the plainly rounded BT.709 U row -26, -87, 112 sums to -1 and tints bright
# greys: hence -86).  No clamp: limited range gives Y in [16, 235] and U, V in [16, 240], full range exactly [0, 255] - the
# chroma rounding term of 127 keeps pure blue and pure red at 255, as libjpeg's does.  Over all 2^24 RGB triples every plane is
# within 1.17 levels of the float64 formulas (Kr, Kb = 0.299, 0.114 / 0.2126, 0.0722; scales 219/255 and 224/255, or 1).
# csrc/common.hpp holds the same table for the kernels (float_yuv_matrix returns it).
YUV_MATRICES = {
    0: ((66, 129, 25, 128, 16), (-38, -74, 112, 128, 128), (112, -94, -18, 128, 128)),    # BT.601 limited
    2: ((47, 157, 16, 128, 16), (-26, -86, 112, 128, 128), (112, -102, -10, 128, 128)),   # BT.709 limited
    4: ((77, 150, 29, 128, 0), (-43, -85, 128, 127, 128), (128, -107, -21, 127, 128)),    # BT.601 full
    6: ((54, 183, 19, 128, 0), (-29, -99, 128, 127, 128), (128, -116, -12, 127, 128)),    # BT.709 full
}
YUV_MATRIX_NAMES = {"bt601": 0, "bt709": 2, "bt601-full": 4, "bt709-full": 6}


def yuv_matrix_id(m, width=None, height=None):
    """The id (0 | 2 | 4 | 6, a key of YUV_MATRICES) of a `matrix` argument: None -> 0 (BT.601 limited range, the default
    everywhere); an id; "bt601" | "bt709" | "bt601-full" | "bt709-full"; or "auto", which needs the size of the frames that
    leave: BT.709 limited when width >= 1280 or height > 576, else BT.601 limited.  That rule mirrors what players and encoders
    guess for untagged video (mpv's; ffmpeg-based players do likewise for HD) - a convention, not a measurement.  Anything else
    is a ValueError."""
    if m is None:
        return 0
    if isinstance(m, str):
        if m == "auto":
            if width is None or height is None:
                raise ValueError("matrix='auto' needs the size of the frames that leave (width, height)")
            return 2 if (int(width) >= 1280 or int(height) > 576) else 0
        if m in YUV_MATRIX_NAMES:
            return YUV_MATRIX_NAMES[m]
    elif isinstance(m, int) and not isinstance(m, bool) and m in YUV_MATRICES:
        return int(m)
    raise ValueError("matrix must be None, 0 | 2 | 4 | 6, 'auto' or one of %s (got %r)" % (sorted(YUV_MATRIX_NAMES), m))


def yuv_matrix_for(what, matrix, fmt, width=None, height=None):
    """The id of the `matrix` keyword of a call `what` whose frames leave in format `fmt` at width x height: yuv_matrix_id for
    "i420"; any other format (fp32 or uint8 RGB, JPEG) has no matrix to choose, and a `matrix` other than None there is a
    ValueError - raised at the call, before anything is enqueued or opened."""
    if fmt != "i420":
        if matrix is not None:
            raise ValueError("%s: matrix=%r applies to out_format='i420' only (these frames leave as %s)" % (what, matrix, fmt))
        return 0
    return yuv_matrix_id(matrix, width, height)


def yuv_full_range(matrix):
    """True where the matrix gives full-range samples (ids 4 and 6)."""
    return bool(yuv_matrix_id(matrix) & 4)


def yuv_ffmpeg_args(matrix):
    """The arguments that tell ffmpeg what raw or Y4M I420 frames of `matrix` (None | id | name, not "auto") hold - Y4M carries
    the range (XCOLORRANGE) but not the matrix, so a caller states it: ["-colorspace", .., "-color_primaries", .., "-color_trc",
    .., "-color_range", ..] with bt709 x 3 for BT.709 and smpte170m x 3 for BT.601, and tv (limited) or pc (full)."""
    i = yuv_matrix_id(matrix)
    name = "bt709" if i & 2 else "smpte170m"
    return ["-colorspace", name, "-color_primaries", name, "-color_trc", name, "-color_range", "pc" if i & 4 else "tv"]


def rgb8_to_i420(frames_u8, matrix=None):
    """(T, R, R, 3) or (R, R, 3) uint8 RGB -> (T, 3R/2, R) or (3R/2, R) uint8 planar YUV 4:2:0 (I420: the Y plane R x R, then U and
    V at R/2 x R/2 each, row-major, contiguous - OpenCV's *_I420 layout, ffmpeg's yuv420p).  matrix: as yuv_matrix_id reads it
    (not "auto"); None = 0 = 8-bit BT.601 limited range, all in int32 with >> an arithmetic shift (floor):
        Y  = ((66 R + 129 G + 25 B + 128) >> 8) + 16                        per pixel, in [16, 235]
        Mc = (c00 + c01 + c10 + c11 + 2) >> 2                               per 2 x 2 block and channel c
        U  = ((-38 MR - 74 MG + 112 MB + 128) >> 8) + 128                   in [16, 240]
        V  = ((112 MR - 94 MG - 18 MB + 128) >> 8) + 128                    in [16, 240]
    The other ids take their rows of YUV_MATRICES in the same arithmetic.
    Chroma is sited at the block centre (Y4M's C420jpeg).  This is the definition of what SynthesisHIP.decode_i420 and
    float_dec_frames[_host]_i420 produce: bitwise rgb8_to_i420(decode_u8(...), matrix).  Works on any device."""
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (3, 4) or frames_u8.shape[-1] != 3:
        raise ValueError("rgb8_to_i420 takes (T, H, W, 3) or (H, W, 3) uint8 frames, got %s %s" % (frames_u8.dtype, tuple(frames_u8.shape)))
    ky, ku, kv = YUV_MATRICES[yuv_matrix_id(matrix)]
    single = frames_u8.dim() == 3
    x = (frames_u8[None] if single else frames_u8).to(torch.int32)
    T, H, W, _ = x.shape
    if H % 2 or W % 2:
        raise ValueError("rgb8_to_i420 needs even sizes for 4:2:0 chroma (got %d x %d)" % (H, W))

    def plane(k, r, g, b):
        return ((k[0] * r + k[1] * g + k[2] * b + k[3]) >> 8) + k[4]

    y = plane(ky, x[..., 0], x[..., 1], x[..., 2])
    m = (x.reshape(T, H // 2, 2, W // 2, 2, 3).sum(dim=(2, 4)) + 2) >> 2
    u = plane(ku, m[..., 0], m[..., 1], m[..., 2])
    v = plane(kv, m[..., 0], m[..., 1], m[..., 2])
    out = torch.cat([y.reshape(T, -1), u.reshape(T, -1), v.reshape(T, -1)], dim=1).to(torch.uint8)
    out = out.reshape(T, H * 3 // 2, W)
    return out[0] if single else out


def paste_i420(src8, frames8, rect, feather, matrix=None, resample=None):
    """The pasted frames as planar YUV 4:2:0: rgb8_to_i420(paste_rgb8(src8, frames8, rect, feather), matrix) -> (T, 3H/2, W) uint8
    at the portrait's size, H and W even (ValueError otherwise - nothing is padded or cropped).  Chroma is the 2 x 2 mean of the PASTED
    8-bit RGB samples, so a block that straddles the box edge or the feather mixes pasted and source pixels; it is never a blend
    of chroma.  resample: as in paste_rgb8.  The definition `float_img_paste_i420` (image.paste_frames_device(out_format="i420")) is held to bit for bit."""
    if src8.dim() == 3 and (src8.shape[0] % 2 or src8.shape[1] % 2):
        raise ValueError("paste_i420: a %d x %d portrait has an odd side; 4:2:0 chroma needs even sides" % (src8.shape[0], src8.shape[1]))
    return rgb8_to_i420(paste_rgb8(src8, frames8, rect, feather, resample), matrix)


def y4m_rate(fps):
    """The frame rate of a Y4M header as a fraction.
    Rule 1 (NTSC family): a non-integer float fps with |fps * 1.001 - n| < 1e-4 for an integer n >= 1 is n * 1000 / 1001:
    23.976 -> 24000/1001, 29.97 -> 30000/1001, 59.94 -> 60000/1001 (the decimal shorthands mean the rate they abbreviate; the
    closest fraction alone would write 2997/100).  29.9, 30.0 and 29.98 are not within 1e-4 and do not snap.
    Rule 2 (everything else, and every fractions.Fraction): fractions.Fraction(fps).limit_denominator(1001), so 25 -> 25/1,
    12.5 -> 25/2, 29.9 -> 299/10."""
    k = float(fps) * 1001.0 / 1000.0
    if not isinstance(fps, fractions.Fraction) and round(k) >= 1 and abs(k - round(k)) < 1e-4 and float(fps) != round(float(fps)):
        return fractions.Fraction(int(round(k)) * 1000, 1001)
    return fractions.Fraction(fps).limit_denominator(1001)


class Y4MWriter:
    """A YUV4MPEG2 stream written block by block, for frames that arrive in pieces (InferenceAgent.stream_device with
    out_format="i420"): the header `YUV4MPEG2 W.. H.. F<num>:<den> Ip A1:1 C420jpeg XCOLORRANGE=LIMITED` goes out once, when the
    writer is made, and every write(frames) appends `FRAME` + the frame's bytes per frame.  path_or_file: a path (opened here
    and closed by close() / on leaving the `with` block), or an object with write() (a pipe to an encoder's stdin), which is
    left open.  fps: as y4m_rate reads it.  write() has handed the bytes on when it returns, so a view of a ring slot may be
    given back right after it.  matrix: as yuv_matrix_id reads it; the full-range ids (4, 6) write XCOLORRANGE=FULL.  Y4M has no
    tag for the matrix itself: yuv_ffmpeg_args states it to the consumer."""

    def __init__(self, path_or_file, width, height, fps, matrix=None):
        width, height = int(width), int(height)
        if width < 2 or height < 2 or width % 2 or height % 2:
            raise ValueError("Y4MWriter: 4:2:0 frames have even sides (got %d x %d)" % (width, height))
        self.width, self.height = width, height
        self.matrix = yuv_matrix_id(matrix, width, height)
        rate = y4m_rate(fps)
        header = "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=%s\n" % (width, height, rate.numerator, rate.denominator,
                                                                              "FULL" if self.matrix & 4 else "LIMITED")
        self.frames = 0
        self._own = not hasattr(path_or_file, "write")
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        try:
            self._f.write(header.encode("ascii"))
        except BaseException:
            self.close()
            raise

    def write(self, frames_i420):
        """Append (n, 3 * height / 2, width) uint8 I420 frames; returns the number of frames written so far."""
        if self._f is None:
            raise ValueError("Y4MWriter.write after close()")
        want = (3 * self.height // 2, self.width)
        if frames_i420.dtype != torch.uint8 or frames_i420.dim() != 3 or tuple(frames_i420.shape[1:]) != want:
            raise ValueError("Y4MWriter.write takes (n, %d, %d) uint8 I420 frames, got %s %s"
                             % (want + (frames_i420.dtype, tuple(frames_i420.shape))))
        data = frames_i420.detach().cpu().contiguous().numpy()
        for t in range(data.shape[0]):
            self._f.write(b"FRAME\n")
            self._f.write(data[t].tobytes())
        self.frames += data.shape[0]
        return self.frames

    def close(self):
        f, self._f = self._f, None
        if f is not None and self._own:
            f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def write_y4m(path_or_file, frames_i420, fps, matrix=None):
    """Write (T, 3R/2, R) uint8 I420 frames (rgb8_to_i420 / SynthesisHIP.decode_i420 / out_format="i420") as a YUV4MPEG2
    stream, which ffmpeg, x264 and mpv read as it is: the header `YUV4MPEG2 W.. H.. F<num>:<den> Ip A1:1 C420jpeg
    XCOLORRANGE=LIMITED`, then `FRAME` + the frame's bytes per frame.  fps: as y4m_rate reads it (25 -> 25:1, 29.97 ->
    30000:1001).  path_or_file: a path, or an object with write() (a pipe to an encoder's stdin).  Y4MWriter is the
    block-by-block form.  matrix: the matrix the frames were made with (XCOLORRANGE=FULL for ids 4 and 6)."""
    if frames_i420.dtype != torch.uint8 or frames_i420.dim() != 3 or frames_i420.shape[1] * 2 != frames_i420.shape[2] * 3:
        raise ValueError("write_y4m takes (T, 3R/2, R) uint8 I420 frames, got %s %s" % (frames_i420.dtype, tuple(frames_i420.shape)))
    T, H32, W = frames_i420.shape
    with Y4MWriter(path_or_file, W, H32 * 2 // 3, fps, matrix) as w:
        w.write(frames_i420)


# ---------------------------------------------------------------- baseline JPEG in integers (the definition of float_jpg_encode)
# ITU-T T.81 Annex K.1 / K.2 (quantiser tables, row-major) and K.3 (the four Huffman tables as BITS + HUFFVAL)
_JPEG_Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
                103, 99)
_JPEG_Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + \
    (99,) * 32
JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
               57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_JPEG_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_JPEG_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
# (class << 4 | id, BITS[1..16], HUFFVAL) in the order the header writes them: DC0, AC0, DC1, AC1
JPEG_HUFFMAN = ((0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
                (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), _JPEG_AC_LUMA_VALS),
                (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
                (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), _JPEG_AC_CHROMA_VALS))


def jpeg_tables(quality):
    """(luma, chroma) quantiser tables of a quality in 1 ... 100 as (64,) int32 arrays in row-major order: Annex K.1 / K.2 of
    ITU-T T.81 under the common scaling s = 5000 // q below 50, else 200 - 2 q; v = clamp((base s + 50) // 100, 1, 255)."""
    import numpy as np
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError("JPEG quality must be an integer in 1 ... 100 (got %r)" % (quality,))
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(base, dtype=np.int64) * s + 50) // 100, 1, 255).astype(np.int32) for base in (_JPEG_Q_LUMA, _JPEG_Q_CHROMA))


def jpeg_huffman_codes(bits, vals):
    """{symbol: (code, length)} of a BITS / HUFFVAL pair (T.81 Annex C: codes of one length count up, and double to the next)."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


JPEG_PAD_MAX_SIDE = 16384  # the largest side pad="edge" takes: float_jpg_encode_padded's


def _jpeg_geometry(h, w, restart, pad=None):
    h, w = int(h), int(w)
    if pad is None:
        if h < 16 or w < 16 or h % 16 or w % 16 or h > 65520 or w > 65520:
            raise ValueError("JPEG 4:2:0 frames have sides that are multiples of 16 (got %d x %d)" % (h, w))
    elif pad != "edge":
        raise ValueError("JPEG pad must be None or \"edge\" (got %r)" % (pad,))
    elif not (1 <= h <= JPEG_PAD_MAX_SIDE and 1 <= w <= JPEG_PAD_MAX_SIDE):
        raise ValueError("JPEG frames under pad=\"edge\" have sides in 1 ... %d (got %d x %d)" % (JPEG_PAD_MAX_SIDE, h, w))
    restart = -(-w // 16) if restart is None else int(restart)
    if not 0 <= restart <= 65535:
        raise ValueError("JPEG restart interval must be 0 ... 65535 MCUs (got %r)" % (restart,))
    return h, w, restart


def jpeg_header(h, w, quality, restart, pad=None):
    """Everything of the file in front of the scan data: SOI, APP0 (JFIF 1.1, density 1:1), DQT 0 and 1 (8-bit, zigzag order),
    SOF0 (8 bits, h x w, Y 2x2 with table 0, Cb and Cr 1x1 with table 1), DHT DC0, AC0, DC1, AC1 (Annex K.3), DRI when
    restart > 0, SOS (one interleaved scan, Ss 0, Se 63).  restart: MCUs per interval, 0 none, None one MCU row (ceil(w / 16)).
    pad: as in jpeg_encode_rgb8 - SOF0 carries the true h and w."""
    import struct
    h, w, restart = _jpeg_geometry(h, w, restart, pad)
    out = [b"\xff\xd8", b"\xff\xe0", struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)]
    for i, t in enumerate(jpeg_tables(quality)):
        out += [b"\xff\xdb", struct.pack(">HB", 67, i), bytes(int(t[z]) for z in JPEG_ZIGZAG)]
    out += [b"\xff\xc0", struct.pack(">HBHHB", 17, 8, h, w, 3), bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))]
    for tc_th, bits, vals in JPEG_HUFFMAN:
        out += [b"\xff\xc4", struct.pack(">HB", 19 + len(vals), tc_th), bytes(bits), vals]
    if restart > 0:
        out += [b"\xff\xdd", struct.pack(">HH", 4, restart)]
    out += [b"\xff\xda", struct.pack(">HB", 12, 3), bytes((1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))]
    return b"".join(out)


def jpeg_dct_matrix():
    """M = rint(2^14 A), A the orthonormal 8-point DCT-II matrix, as (8, 8) int64."""
    import numpy as np
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    A = 0.5 * np.cos((2 * n + 1) * k * np.pi / 16)
    A[0, :] = math.sqrt(1.0 / 8.0)
    return np.rint(A * 2.0**14).astype(np.int64)


def jpeg_quantised_blocks(frames_u8, quality):
    """The quantised DCT coefficients jpeg_encode_rgb8 codes: (T, MCUs, 6, 64) int32 in zigzag order, MCUs in raster order, per
    MCU the four Y blocks (raster), then Cb, then Cr.  frames_u8: (T, H, W, 3) uint8 as a numpy array."""
    import numpy as np
    x = frames_u8.astype(np.int64)
    T, H, W, _ = x.shape
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    sub = lambda c: (c.reshape(T, H // 2, 2, W // 2, 2).sum(axis=(2, 4)) + 2) >> 2
    my, mx = H // 16, W // 16
    yb = (y - 128).reshape(T, my, 2, 8, mx, 2, 8).transpose(0, 1, 4, 2, 5, 3, 6).reshape(T, my * mx, 4, 8, 8)
    cbb, crb = ((sub(c) - 128).reshape(T, my, 8, mx, 8).transpose(0, 1, 3, 2, 4).reshape(T, my * mx, 1, 8, 8) for c in (cb, cr))
    X = np.concatenate([yb, cbb, crb], axis=2)
    M = jpeg_dct_matrix()
    p1 = M @ X
    assert np.abs(p1).max() < 2**24
    t = (p1 + 2**10) >> 11
    p2 = t @ M.T
    assert np.abs(p2).max() < 2**28
    f8 = (p2 + 2**13) >> 14  # the coefficient x 8
    ql, qc = jpeg_tables(quality)
    q = np.stack([ql] * 4 + [qc] * 2).astype(np.int64).reshape(6, 8, 8)
    c = np.sign(f8) * ((np.abs(f8) + 4 * q) // (8 * q))
    return c.reshape(T, my * mx, 6, 64)[..., list(JPEG_ZIGZAG)].astype(np.int32)


def jpeg_encode_rgb8(frames_u8, quality=90, restart=None, stats=False, pad=None):
    """(T, H, W, 3) or (H, W, 3) uint8 RGB (a torch tensor on any device, or a numpy array) -> a list of `bytes`, one complete
    baseline JFIF file per frame (4:2:0, one interleaved scan, the standard Huffman tables).  H and W are multiples of 16 (any
    size with pad="edge").  This is the definition of what float_jpg_encode and float_jpg_encode_padded write: all of it is
    integer arithmetic, `>>` an arithmetic shift.
      pad      None: sides that are no multiples of 16 are refused.  "edge": any H and W in 1 ... 16384; the coded area is
               ceil(H / 16) x ceil(W / 16) MCUs and its sample (y, x) is the source pixel (min(y, H - 1), min(x, W - 1)) - the last
               row and column replicated, on RGB, in front of everything below, which is unchanged; SOF0 carries the true H and W
               and the decoder crops.  (Plain replication, not libjpeg's DC-only dummy blocks.)  Sides that are multiples of 16
               give the bytes of pad=None.
      colour   full-range BT.601 per pixel: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16,
               Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16;
               chroma subsampled 2 x 2 by (c00 + c01 + c10 + c11 + 2) >> 2 on the converted planes; level shift -128
      DCT      M = rint(2^14 A): t = (M X + 2^10) >> 11, F8 = (t M^T + 2^13) >> 14 (the coefficient x 8; |M X| < 2^24, |t M^T| < 2^28)
      quant    c = sign(F8) ((|F8| + 4 q) // (8 q)), q from jpeg_tables(quality)
      entropy  MCU = 4 Y blocks, Cb, Cr; DC differences per component; ZRL for runs above 15; EOB unless coefficient 63 is
               non-zero; `restart` MCUs per interval (0: none, None: one MCU row): before MCU m > 0 with m % restart == 0 the bit
               buffer is padded with 1-bits to a byte, RSTk follows (k cycling 0 ... 7) and the three predictors return to 0;
               every 0xFF data byte is followed by 0x00; the last byte of the scan is padded with 1-bits
    stats=True: also returns a dict of what the streams exercised: stuffed_bytes, zrl, blocks_without_eob, max_dc_category,
    max_ac_category, restart_markers (sums / maxima over the frames)."""
    import numpy as np
    x = frames_u8
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.uint8:
            raise ValueError("jpeg_encode_rgb8 takes uint8 frames, got %s" % (x.dtype,))
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] != 3:
        raise ValueError("jpeg_encode_rgb8 takes (T, H, W, 3) or (H, W, 3) uint8 frames, got %s %s" % (x.dtype, tuple(x.shape)))
    if x.ndim == 3:
        x = x[None]
    T, H, W, _ = x.shape
    H, W, ri = _jpeg_geometry(H, W, restart, pad)
    header = jpeg_header(H, W, quality, ri, pad)
    if H % 16 or W % 16:  # pad="edge": the last row and column fill the partial MCUs
        x = x[:, np.minimum(np.arange(-(-H // 16) * 16), H - 1)][:, :, np.minimum(np.arange(-(-W // 16) * 16), W - 1)]
    zz = jpeg_quantised_blocks(x, quality).astype(np.int64)
    nmcu = zz.shape[1]
    nblk = nmcu * 6
    span = ri if ri > 0 else nmcu
    n_int = -(-nmcu // span)
    comp = np.tile(np.array([0, 0, 0, 0, 1, 2]), nmcu)
    interval = np.repeat(np.arange(nmcu) // span, 6)
    cat_of = np.zeros(4096, dtype=np.int64)
    for k in range(1, 13):
        cat_of[1 << (k - 1):1 << k] = k
    code_tabs = [jpeg_huffman_codes(bits, vals) for _, bits, vals in JPEG_HUFFMAN]
    lut = np.zeros((4, 256, 2), dtype=np.int64)  # [DC0, AC0, DC1, AC1][symbol] = (code, length)
    for i, tab in enumerate(code_tabs):
        for sym, cl in tab.items():
            lut[i, sym] = cl
    tsel = (comp > 0).astype(np.int64) * 2  # index of the block's DC table; + 1 its AC table
    pos = np.arange(1, 64)
    st = dict(stuffed_bytes=0, zrl=0, blocks_without_eob=0, max_dc_category=0, max_ac_category=0, restart_markers=0)
    files = []
    for f in range(T):
        z = zz[f].reshape(nblk, 64)
        val = np.zeros((nblk, 129), dtype=np.uint64)  # slots: DC | (ZRLs, code + amplitude) per AC position | EOB | interval padding
        length = np.zeros((nblk, 129), dtype=np.int64)
        diff = np.zeros(nblk, dtype=np.int64)
        for c in range(3):
            idx = np.nonzero(comp == c)[0]
            dc = z[idx, 0]
            prev = np.concatenate([[0], dc[:-1]])
            prev[np.concatenate([[True], interval[idx][1:] != interval[idx][:-1]])] = 0
            diff[idx] = dc - prev
        cat = cat_of[np.abs(diff)]
        amp = np.where(diff < 0, diff + (1 << cat) - 1, diff)
        val[:, 0] = ((lut[tsel, cat, 0] << cat) | amp).astype(np.uint64)
        length[:, 0] = lut[tsel, cat, 1] + cat
        st["max_dc_category"] = max(st["max_dc_category"], int(cat.max()))
        ac = z[:, 1:]
        nz = ac != 0
        last = np.maximum.accumulate(np.where(nz, pos[None, :], 0), axis=1)
        run = pos[None, :] - np.concatenate([np.zeros((nblk, 1), dtype=np.int64), last[:, :-1]], axis=1) - 1
        acat = cat_of[np.abs(ac)]
        assert int(acat.max()) <= 10
        aamp = np.where(ac < 0, ac + (1 << acat) - 1, ac)
        sym = ((run & 15) << 4) | acat
        tac = (tsel + 1)[:, None]
        n_zrl = np.where(nz, run >> 4, 0)
        zc, zl = lut[tac, 0xF0, 0], lut[tac, 0xF0, 1]
        zv = np.zeros_like(run)
        for _ in range(3):
            zv = np.where(n_zrl > _, (zv << zl) | zc, zv)
        val[:, 1:127:2] = zv.astype(np.uint64)
        length[:, 1:127:2] = n_zrl * zl
        val[:, 2:127:2] = np.where(nz, (lut[tac, sym, 0] << acat) | aamp, 0).astype(np.uint64)
        length[:, 2:127:2] = np.where(nz, lut[tac, sym, 1] + acat, 0)
        eob = last[:, -1] < 63
        val[:, 127] = np.where(eob, lut[tsel + 1, 0, 0], 0).astype(np.uint64)
        length[:, 127] = np.where(eob, lut[tsel + 1, 0, 1], 0)
        st["zrl"] += int(n_zrl.sum())
        st["blocks_without_eob"] += int((~eob).sum())
        st["max_ac_category"] = max(st["max_ac_category"], int(acat.max()))
        bits_int = np.bincount(interval, weights=length.sum(axis=1), minlength=n_int).astype(np.int64)
        pad = (-bits_int) % 8
        ends = np.minimum((np.arange(n_int) + 1) * span, nmcu) * 6 - 1  # the last block of every interval
        val[ends, 128] = ((1 << pad) - 1).astype(np.uint64)
        length[ends, 128] = pad
        keep = length.reshape(-1) > 0
        v, n = val.reshape(-1)[keep], length.reshape(-1)[keep]
        start = np.cumsum(n) - n
        tok = np.repeat(np.arange(n.size), n)
        shift = (n[tok] - 1 - (np.arange(int(n.sum())) - start[tok])).astype(np.uint64)
        data = np.packbits(((v[tok] >> shift) & np.uint64(1)).astype(np.uint8)).tobytes()
        edge = np.concatenate([[0], np.cumsum(bits_int + pad) // 8])
        parts = [header]
        for i in range(n_int):
            if i:
                parts.append(bytes((0xFF, 0xD0 + ((i - 1) & 7))))
                st["restart_markers"] += 1
            piece = data[int(edge[i]):int(edge[i + 1])]
            st["stuffed_bytes"] += piece.count(b"\xff")
            parts.append(piece.replace(b"\xff", b"\xff\x00"))
        parts.append(b"\xff\xd9")
        files.append(b"".join(parts))
    return (files, st) if stats else files


def pcm16(samples):
    """Float samples in [-1, 1] -> little-endian 16-bit PCM bytes: rint(32767 x) after clipping x to [-1, 1].  (n,) or
    (n, channels) - interleaved as stored; a torch tensor or a numpy array."""
    import numpy as np
    x = samples.detach().cpu().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
    return np.rint(np.clip(x.astype(np.float64), -1.0, 1.0) * 32767.0).astype("<i2").tobytes()


class AviMjpegWriter:
    """A Motion-JPEG clip in an AVI container (RIFF `AVI `), written block by block: what ffmpeg, VLC, mpv and editors open.
    `hdrl` holds `avih`, a `strl` for the video stream (`vids` / `MJPG`, a BITMAPINFOHEADER) and, with audio_rate, a `strl` for
    16-bit PCM (`auds`); `movi` holds one `00dc` chunk per frame and one `01wb` chunk per write_audio call, word-aligned; `idx1`
    follows.  The rate is y4m_rate(fps) as dwRate / dwScale.  path_or_file: a path (opened here, closed by close()), or a
    SEEKABLE binary file object, left open: close() goes back and writes the sizes and counts that were unknown at open
    (ValueError at open for a sink that cannot seek).  write() has handed the bytes on when it returns, so a JpegFrames over a
    ring slot may be given back right after it.  A file that would pass 2^31 - 2^20 bytes is refused (ValueError from write /
    write_audio; OpenDML is not written)."""
    LIMIT = 2**31 - 2**20

    def __init__(self, path_or_file, width, height, fps, audio_rate=None, audio_channels=1):
        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1:
            raise ValueError("AviMjpegWriter: sides must be positive (got %d x %d)" % (self.width, self.height))
        self.rate = y4m_rate(fps)
        self.audio_rate = None if audio_rate is None else int(audio_rate)
        self.audio_channels = int(audio_channels)
        if self.audio_rate is not None and (self.audio_rate < 1 or self.audio_channels < 1):
            raise ValueError("AviMjpegWriter: audio_rate and audio_channels must be positive")
        self.frames = self.audio_samples = 0
        self._index, self._max_chunk, self._max_audio = [], 0, 0
        self._own = not hasattr(path_or_file, "write")
        if not self._own and not (hasattr(path_or_file, "seekable") and path_or_file.seekable()):
            raise ValueError("AviMjpegWriter needs a seekable sink: close() writes the sizes and frame counts into the header")
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        try:
            self._base = self._f.tell()
            self._f.write(self._header(0))
            self._movi = self._f.tell() - 4  # idx1 offsets count from the `movi` fourcc
            self._pos = self._f.tell()
        except BaseException:
            f, self._f = self._f, None
            if self._own:
                f.close()
            raise

    def _header(self, movi_bytes):
        import struct
        r, w, h = self.rate, self.width, self.height
        usec = (1000000 * r.denominator + r.numerator // 2) // r.numerator
        audio = self.audio_rate is not None
        align = 2 * self.audio_channels
        per_sec = int(self._max_chunk * r.numerator / r.denominator) + (self.audio_rate * align if audio else 0)
        avih = struct.pack("<14I", usec, per_sec, 0, 0x10, self.frames, 0, 2 if audio else 1, self._max_chunk, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, r.denominator, r.numerator, 0, self.frames, self._max_chunk,
                           0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        chunk = lambda cc, body: cc + struct.pack("<I", len(body)) + body
        lst = lambda kind, body: b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body
        strls = lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf))
        if audio:
            strh_a = struct.pack("<4s4sIHHIIIIIIII4h", b"auds", b"\0\0\0\0", 0, 0, 0, 0, align, self.audio_rate * align, 0, self.audio_samples,
                                 self._max_audio, 0xFFFFFFFF, align, 0, 0, 0, 0)
            strf_a = struct.pack("<HHIIHH", 1, self.audio_channels, self.audio_rate, self.audio_rate * align, align, 16)
            strls += lst(b"strl", chunk(b"strh", strh_a) + chunk(b"strf", strf_a))
        hdrl = lst(b"hdrl", chunk(b"avih", avih) + strls)
        idx_bytes = 8 + 16 * len(self._index)
        riff = 4 + len(hdrl) + 12 + movi_bytes + idx_bytes
        return b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"

    def _chunk(self, cc, data, flags):
        import struct
        if self._f is None:
            raise ValueError("AviMjpegWriter.write after close()")
        n = len(data)
        if self._pos - self._base + 8 + n + (n & 1) + 8 + 16 * (len(self._index) + 1) > self.LIMIT:
            raise ValueError("AviMjpegWriter: the file would pass %d bytes (an AVI without OpenDML extensions ends below 2 GiB)" % self.LIMIT)
        self._f.write(cc + struct.pack("<I", n))
        self._f.write(data)
        if n & 1:
            self._f.write(b"\0")
        self._index.append((cc, flags, self._pos - self._movi, n))
        self._pos += 8 + n + (n & 1)

    def write(self, frames):
        """Append frames: a jpeg.JpegFrames or an iterable of bytes-likes, one complete JPEG file each.  Returns the number of
        frames written so far."""
        if self._f is None:
            raise ValueError("AviMjpegWriter.write after close()")
        for fr in frames:
            self._video(fr)
        return self.frames

    def _video(self, fr):
        fr = memoryview(fr)
        self._chunk(b"00dc", fr, 0x10)
        self._max_chunk = max(self._max_chunk, fr.nbytes)
        self.frames += 1

    def write_audio(self, samples):
        """Append float samples in [-1, 1] - (n,), or (n, audio_channels) - as one `01wb` chunk of 16-bit PCM (pcm16).  Returns
        the number of samples per channel written so far."""
        if self._f is None:
            raise ValueError("AviMjpegWriter.write_audio after close()")
        if self.audio_rate is None:
            raise ValueError("AviMjpegWriter.write_audio: the writer was opened without audio_rate")
        data = pcm16(samples)
        if len(data) % (2 * self.audio_channels):
            raise ValueError("AviMjpegWriter.write_audio: %d samples are not whole frames of %d channels" % (len(data) // 2, self.audio_channels))
        if data:
            self._chunk(b"01wb", data, 0x10)
            self._max_audio = max(self._max_audio, len(data))
            self.audio_samples += len(data) // (2 * self.audio_channels)
        return self.audio_samples

    def close(self):
        import struct
        f, self._f = self._f, None
        if f is None:
            return
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
            f.write(b"".join(struct.pack("<4sIII", *e) for e in self._index))
            end = f.tell()
            f.seek(self._base)
            f.write(self._header(self._pos - self._movi - 4))
            f.seek(end)
        finally:
            if self._own:
                f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ---------------------------------------------------------------- lossless PNG in integers (the definition of float_png_encode)
# Eight code-length tables over the 256 byte values and end-of-block, one hex digit per symbol (csrc/png_kernels.hpp states the
# same digits).  Tables 0 ... 6: Huffman lengths of 0.97 Laplace(min(v, 256 - v) / s) + 0.03 uniform for s = 0.35, 0.7, 1.5, 3, 6,
# 12, 24 - residuals of growing spread; table 7 is flat: 8 bits, byte value 128 and end-of-block 9 - no band costs more than
# 9 bits per byte.
_PNG_LENGTHS = (
    "137abbbbbbbbbbbbbccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbb"
    "bbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbba72b",
    "13579acccccdddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddd"
    "dddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddccccca8652d",
    "233556789aabcccccccdddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddd"
    "dddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddcccccccbaa98765433d",
    "3344555667788999aabbbcccccccddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddd"
    "ddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddccccccbbbbaa999887766554443d",
    "44445555666667777888889999aaaabbbbbbcccccccccdddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddd"
    "dddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddcccccccccbbbbbaaaaa9999888887777666665555444d",
    "555555556666666677777777888888888999999999aaaaaaaaaabbbbbbbbbbbccccccccccccccccccdddddddddddddddddddddddddddddddddddddddddddddddd"
    "dddddddddddddddddddddddddddddddddddddddddddddddccccccccccccccccccbbbbbbbbbbbaaaaaaaaaa99999999988888888877777777666666665555555d",
    "6666666666666667777777777777777788888888888888888999999999999999999aaaaaaaaaaaaaaaaaaabbbbbbbbbbbbbbbbbbbbbcccccccccccccccccccccd"
    "ccccccccccccccccccccbbbbbbbbbbbbbbbbbbbbbbaaaaaaaaaaaaaaaaaaa999999999999999998888888888888888887777777777777777666666666666666d",
    "888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888889"
    "88888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888889",
)
PNG_MAX_SIDE = 16384
PNG_BAND_BYTES = 65536   # the most filter-plus-row bytes of one band
PNG_HEADER_BITS = 1106   # BFINAL, BTYPE, HLIT, HDIST, HCLEN, 19 x 3 bits, 258 x 4 bits
_PNG_CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_CRC_POLY = 0xEDB88320   # CRC-32, reflected: bit 31 is x^0


def png_code_lengths():
    """The 8 code-length tables of the PNG encoder: a tuple of 8 tuples of 257 lengths (byte values 0 ... 255, end-of-block).
    Every table is complete (the Kraft sum is exactly 1) and no length passes 15."""
    return tuple(tuple(int(c, 16) for c in t) for t in _PNG_LENGTHS)


def png_default_band(h, w):
    """Rows per band when none is given: 8, fewer for short frames, and never more bytes than PNG_BAND_BYTES."""
    return max(1, min(8, int(h), PNG_BAND_BYTES // (1 + 3 * int(w))))


def png_check_band(h, w, band=None):
    """The band of an (h, w) frame: None or 0 -> png_default_band; otherwise 1 ... h rows with band (1 + 3 w) <= 65536."""
    h, w = int(h), int(w)
    if not (1 <= h <= PNG_MAX_SIDE and 1 <= w <= PNG_MAX_SIDE):
        raise ValueError("PNG sides (%d x %d) must be in 1 ... %d" % (h, w, PNG_MAX_SIDE))
    band = png_default_band(h, w) if band is None or int(band) == 0 else int(band)
    if not 1 <= band <= h or band * (1 + 3 * w) > PNG_BAND_BYTES:
        raise ValueError("PNG band (%d) must be 1 ... h (%d) rows of at most %d bytes in all (a row is %d)" % (band, h, PNG_BAND_BYTES, 1 + 3 * w))
    return band


def png_slot_bytes(rows, w):
    """The worst case of one band of `rows` rows in bytes, float_png_encode's slot: the 1106-bit header, 9 bits per byte (the
    flat table bounds the chosen one), an end-of-block of at most 15 bits (9 in the flat table), the 3-bit header of the
    stored block, up to 7 bits to the byte boundary and 00 00 FF FF; rounded up to 16 bytes."""
    n = int(rows) * (1 + 3 * int(w))
    return ((PNG_HEADER_BITS + 9 * n + 15 + 3 + 7) // 8 + 4 + 15) & ~15


def png_filter_rows(frame_u8):
    """(h, w, 3) uint8 -> the h (1 + 3 w) bytes PNG compresses: per row the filter type, then the filtered bytes.  The five
    filters are the PNG specification's with bpp = 3 (the row above row 0 is zero); a row takes the filter whose
    sum of min(v, 256 - v) over its 3 w filtered bytes is smallest, ties to the smallest type."""
    import numpy as np
    x = frame_u8.detach().cpu().numpy() if isinstance(frame_u8, torch.Tensor) else np.asarray(frame_u8)
    if x.dtype != np.uint8 or x.ndim != 3 or x.shape[-1] != 3:
        raise ValueError("png_filter_rows takes (h, w, 3) uint8, got %s %s" % (x.dtype, tuple(x.shape)))
    h, w, _ = x.shape
    cur = x.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(cur)
    a[:, 3:] = cur[:, :-3]
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[1:, 3:] = cur[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([cur, cur - a, cur - b, cur - ((a + b) >> 1), cur - paeth]) & 255  # (5, h, 3w)
    cost = np.minimum(cand, 256 - cand).sum(axis=2)  # (5, h)
    f = np.argmin(cost, axis=0)  # the first of equal minima
    out = np.empty((h, 1 + 3 * w), np.uint8)
    out[:, 0] = f
    out[:, 1:] = cand[f, np.arange(h)]
    return out.tobytes()


def _crc_mul(a, b):
    """a(x) b(x) mod the CRC-32 polynomial, both reflected (bit 31 is x^0)"""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ _CRC_POLY if b & 1 else b >> 1
    return p


def _crc_xpow8(n):
    """x^(8 n) mod the CRC-32 polynomial, by square-and-multiply"""
    p, sq = 0x80000000, 0x00800000  # x^0, x^8
    while n:
        if n & 1:
            p = _crc_mul(sq, p)
        sq = _crc_mul(sq, sq)
        n >>= 1
    return p


def crc32_combine(crc_a, crc_b, len_b):
    """zlib.crc32(A + B) from crc_a = zlib.crc32(A), crc_b = zlib.crc32(B) and len_b = len(B): crc_a times x^(8 len_b) modulo the
    CRC polynomial (a carry-less multiplication, the power by square-and-multiply), xor crc_b.  What the kernels of
    float_png_encode and ApngWriter form chunk CRCs with instead of a pass over the data."""
    return (_crc_mul(_crc_xpow8(int(len_b)), int(crc_a) & 0xFFFFFFFF) ^ int(crc_b)) & 0xFFFFFFFF


_png_codes_cache = []


def _png_codes():
    """per table (lengths, codes bit-reversed for an LSB-first stream, the 1106 header bits as a 0 / 1 array)"""
    import numpy as np
    if not _png_codes_cache:
        for lens in png_code_lengths():
            lens = np.array(lens, np.int64)
            code, rev = 0, np.zeros(257, np.int64)
            for n in range(1, 16):  # canonical: the codes of one length count up in symbol order, and double to the next length
                for s in np.nonzero(lens == n)[0]:
                    rev[s] = int(format(code, "0%db" % n)[::-1], 2)
                    code += 1
                code <<= 1
            bits = [0, 0, 1] + [0] * 5 + [0] * 5 + [1, 1, 1, 1]  # BFINAL 0, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15: LSB first
            for s in _PNG_CLEN_ORDER:
                v = 4 if s < 16 else 0
                bits += [v & 1, (v >> 1) & 1, (v >> 2) & 1]
            for n in list(lens) + [0]:  # the code-length code is 4 bits for 0 ... 15: symbol n has code n, sent MSB first
                bits += [(n >> 3) & 1, (n >> 2) & 1, (n >> 1) & 1, n & 1]
            assert len(bits) == PNG_HEADER_BITS
            _png_codes_cache.append((lens, rev, np.array(bits, np.uint8)))
    return _png_codes_cache


def png_band_bytes(data, stats=None):
    """One band's filter-plus-row bytes -> its deflate bytes: a dynamic-Huffman block of literals in the cheapest of the 8
    tables (bits(k) = sum of hist[v] T_k[v]; ties to the smallest k), then an empty stored block (sync flush)."""
    import numpy as np
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    tabs = _png_codes()
    hist = np.bincount(d, minlength=256)
    cost = [int((hist * t[0][:256]).sum()) for t in tabs]
    k = cost.index(min(cost))
    if stats is not None:
        stats.append(k)
    lens, rev, head = tabs[k]
    sym = np.concatenate([d, [256]])
    n = lens[sym]
    start = PNG_HEADER_BITS + np.cumsum(n) - n
    total = int(start[-1] + n[-1]) + 3
    total = (total + 7) & ~7
    bits = np.zeros(total + 32, np.uint8)
    bits[:PNG_HEADER_BITS] = head
    code = rev[sym]
    for b in range(int(n.max())):
        m = n > b
        bits[start[m] + b] = (code[m] >> b) & 1
    bits[total + 16:] = 1  # 00 00 FF FF
    return np.packbits(bits, bitorder="little").tobytes()


def png_encode_rgb8(frames_u8, band=None, stats=False):
    """(T, H, W, 3) or (H, W, 3) uint8 RGB (a torch tensor on any device, or a numpy array) -> a list of `bytes`, one complete
    PNG file per frame (8 bits, colour type 2, no interlace, one IDAT).  This is the definition of what float_png_encode
    writes; all of it is integer arithmetic.
      filter   png_filter_rows
      bands    band b is rows [b band, min(H, (b + 1) band)); band: None or 0 = png_default_band(H, W), else png_check_band's rule
      band     png_band_bytes: literals only (no LZ77 matches) in one of 8 fixed tables, then a sync flush, so that the bands
               are independent, byte-aligned pieces
      zlib     78 01, the bands, 01 00 00 FF FF (the final, empty stored block), the Adler-32 of the filtered bytes
      file     signature, IHDR, IDAT, IEND
    stats=True: also returns the list of the tables chosen, band by band."""
    import struct
    import zlib

    import numpy as np
    x = frames_u8
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] != 3:
        raise ValueError("png_encode_rgb8 takes (T, H, W, 3) or (H, W, 3) uint8 frames, got %s %s" % (x.dtype, tuple(x.shape)))
    if x.ndim == 3:
        x = x[None]
    T, H, W, _ = x.shape
    band = png_check_band(H, W, band)
    stride = 1 + 3 * W
    chunk = lambda cc, body: struct.pack(">I", len(body)) + cc + body + struct.pack(">I", zlib.crc32(cc + body))  # noqa: E731
    ihdr = chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
    files, chosen = [], []
    for t in range(T):
        rows = png_filter_rows(x[t])
        z = [b"\x78\x01"] + [png_band_bytes(rows[r * stride:min(H, r + band) * stride], chosen) for r in range(0, H, band)]
        z += [b"\x01\x00\x00\xff\xff", struct.pack(">I", zlib.adler32(rows))]
        files.append(b"\x89PNG\r\n\x1a\n" + ihdr + chunk(b"IDAT", b"".join(z)) + chunk(b"IEND", b""))
    return (files, chosen) if stats else files


def png_idat(data):
    """(offset, length) of the IDAT data of a PNG file as png_encode_rgb8 and float_png_encode write it: 41 bytes of signature,
    IHDR and the IDAT chunk's head in front, 16 bytes (its CRC and IEND) behind."""
    return 41, len(data) - 57


class ApngWriter:
    """An animated PNG written block by block from the files of png_encode_rgb8 / float_png_encode (png.PngFrames): signature,
    IHDR, `acTL`, then per frame an `fcTL` (the whole canvas, delay 1 / fps as the fraction y4m_rate(fps) gives, no blending)
    and the frame's zlib stream - frame 0 as `IDAT`, the later ones as `fdAT` - and `IEND`.  The zlib streams are copied as they
    are, and a chunk's CRC is formed from `crcs[i]`, the CRC-32 of frame i's zlib stream, by crc32_combine - never by a pass
    over the data.  path_or_file: a path (opened here, closed by close()), or a SEEKABLE binary file object, left open: close()
    goes back and writes the frame count into `acTL` (ValueError at open for a sink that cannot seek; ValueError at close()
    when no frame was written: an APNG has at least one).  APNG carries NO AUDIO.  Players that do not know APNG show frame 0."""

    def __init__(self, path_or_file, width, height, fps):
        import struct
        self.width, self.height = int(width), int(height)
        if not (1 <= self.width <= PNG_MAX_SIDE and 1 <= self.height <= PNG_MAX_SIDE):
            raise ValueError("ApngWriter: sides (%d x %d) must be in 1 ... %d" % (self.width, self.height, PNG_MAX_SIDE))
        rate = y4m_rate(fps)
        self.delay = (rate.denominator, rate.numerator)  # seconds per frame as a fraction
        if not (1 <= self.delay[0] <= 65535 and 1 <= self.delay[1] <= 65535):
            raise ValueError("ApngWriter: the frame delay %d / %d does not fit fcTL's 16-bit fields" % self.delay)
        self.frames = self._seq = 0
        self._own = not hasattr(path_or_file, "write")
        if not self._own and not (hasattr(path_or_file, "seekable") and path_or_file.seekable()):
            raise ValueError("ApngWriter needs a seekable sink: close() writes the frame count into acTL")
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        try:
            ihdr = struct.pack(">IIBBBBB", self.width, self.height, 8, 2, 0, 0, 0)
            self._f.write(b"\x89PNG\r\n\x1a\n" + self._chunk(b"IHDR", ihdr))
            self._actl = self._f.tell()
            self._f.write(self._chunk(b"acTL", struct.pack(">II", 0, 0)))
        except BaseException:
            f, self._f = self._f, None
            if self._own:
                f.close()
            raise

    @staticmethod
    def _chunk(cc, body):
        import struct
        import zlib
        return struct.pack(">I", len(body)) + cc + body + struct.pack(">I", zlib.crc32(cc + body))

    def write(self, frames, crcs=None):
        """Append frames: a png.PngFrames (its .crcs are taken), or an iterable of bytes-likes with `crcs`, one CRC-32 of the
        zlib stream per frame - one complete PNG file each, of this writer's size, as png_encode_rgb8 lays it out.  Returns the
        number of frames written so far."""
        import struct
        import zlib
        if self._f is None:
            raise ValueError("ApngWriter.write after close()")
        crcs = getattr(frames, "crcs", None) if crcs is None else crcs
        if crcs is None:
            raise ValueError("ApngWriter.write: crcs (the CRC-32 of every frame's zlib stream) are needed")
        crcs = crcs.tolist() if hasattr(crcs, "tolist") else list(crcs)
        for i, fr in enumerate(frames):
            fr = memoryview(fr)
            at, n = png_idat(fr)
            if n < 11 or bytes(fr[16:24]) != struct.pack(">II", self.width, self.height) or bytes(fr[37:41]) != b"IDAT":
                raise ValueError("ApngWriter.write: frame %d is not a %d x %d file of png_encode_rgb8's layout" % (self.frames, self.width, self.height))
            fctl = struct.pack(">IIIIIHHBB", self._seq, self.width, self.height, 0, 0, self.delay[0], self.delay[1], 0, 0)
            self._f.write(self._chunk(b"fcTL", fctl))
            self._seq += 1
            if self.frames == 0:
                head, size = b"IDAT", n
            else:
                head, size = b"fdAT" + struct.pack(">I", self._seq), n + 4
                self._seq += 1
            self._f.write(struct.pack(">I", size) + head)
            self._f.write(fr[at:at + n])
            self._f.write(struct.pack(">I", crc32_combine(zlib.crc32(head), int(crcs[i]) & 0xFFFFFFFF, n)))
            self.frames += 1
        return self.frames

    def close(self):
        import struct
        f, self._f = self._f, None
        if f is None:
            return
        try:
            if self.frames == 0:
                raise ValueError("ApngWriter: no frame was written (an APNG holds at least one)")
            f.write(self._chunk(b"IEND", b""))
            end = f.tell()
            f.seek(self._actl)
            f.write(self._chunk(b"acTL", struct.pack(">II", self.frames, 0)))  # 0 plays: loop for ever
            f.seek(end)
        finally:
            if self._own:
                f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is not None and self.frames == 0:  # the block failed before a frame: its error is the one to report
            f, self._f = self._f, None
            if f is not None and self._own:
                f.close()
            return False
        self.close()
        return False
