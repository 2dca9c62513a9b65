"""Lossless PNG files from 8-bit frames on the device (`float_png_encode`, include/float_hip.h).  The definition is
host_models.png_encode_rgb8: the row filters, the choice among 8 fixed Huffman tables per band of rows, the deflate bits, Adler-32
and the CRCs are integer arithmetic, and the kernels give its bytes.  What crosses PCIe afterwards is the files, not the frames."""
import ctypes as C

import torch

from . import host_models, native
from .jpeg import JpegFrames


def default_band(h, w):
    """Rows per band when none is given: max(1, min(8, h, 65536 // (1 + 3 w))).  The bands of a frame are coded in parallel, one
    workgroup each."""
    return host_models.png_default_band(h, w)


def default_capacity(n_frames, h, w):
    """The default room for the files of n_frames frames: their raw size.  (A frame of noise needs 9 / 8 of it: the offsets tell,
    and the call is repeated with room.)"""
    return max(1, int(n_frames) * int(h) * int(w) * 3)


def _check_frames(x, band):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise ValueError("encode_png_device takes (T, H, W, 3) or (H, W, 3) uint8 frames on the GPU, got %s"
                         % ("%s %s on %s" % (x.dtype, tuple(x.shape), x.device) if isinstance(x, torch.Tensor) else type(x).__name__,))
    x = (x[None] if x.dim() == 3 else x).contiguous()
    return x, host_models.png_check_band(x.shape[1], x.shape[2], band)


def enqueue_encode(x, band, out, offsets, crcs=None, work=None):
    """One float_png_encode call on the current stream, nothing read back: x (T, H, W, 3) uint8 contiguous on the GPU, band as
    host_models.png_check_band returns it (or 0: the default), out 1-d uint8, offsets (T + 1,) int64 and crcs (T,) int32 or None
    on the same device; work: scratch of float_png_work_bytes or None (allocated here, from torch's allocator).  Returns work."""
    T, H, W, _ = (int(v) for v in x.shape)
    L = native.lib()
    need = int(L.float_png_work_bytes(max(T, 1), H, W, band))
    with torch.cuda.device(x.device):
        if work is None or work.numel() < need:
            work = torch.empty(max(16, need), dtype=torch.uint8, device=x.device)
        native.check(L.float_png_encode(C.c_void_p(x.data_ptr()), T, H, W, band, C.c_void_p(out.data_ptr()), out.numel(),
                                        C.c_void_p(offsets.data_ptr()), C.c_void_p(crcs.data_ptr()) if crcs is not None else None,
                                        C.c_void_p(work.data_ptr()), work.numel(), native.stream_ptr(x.device)))
    return work


def _encode(frames_u8_dev, band, out):
    """encode_png_device, also returning the offsets as the host tensor the one read gave."""
    x, band = _check_frames(frames_u8_dev, band)
    T, H, W, _ = (int(v) for v in x.shape)
    if out is not None and (not out.is_cuda or out.device != x.device or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()):
        raise ValueError("encode_png_device: out must be a contiguous 1-d uint8 tensor on %s" % (x.device,))
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty(default_capacity(T, H, W), dtype=torch.uint8, device=x.device)
        offsets = torch.empty(T + 1, dtype=torch.int64, device=x.device)
        crcs = torch.empty(T, dtype=torch.int32, device=x.device)
        work = enqueue_encode(x, band, out, offsets, crcs)
        edges = offsets.cpu()  # the one host read
        if int(edges[-1]) > out.numel():
            out = torch.empty(int(edges[-1]), dtype=torch.uint8, device=x.device)
            enqueue_encode(x, band, out, offsets, crcs, work)
    return out, offsets, crcs, edges


@torch.no_grad()
def encode_png_device(frames_u8_dev, band=None, out=None):
    """float_png_encode on (T, H, W, 3) or (H, W, 3) uint8 frames in HBM -> (data, offsets, crcs), all on the device: file i is
    data[offsets[i]:offsets[i + 1]], bitwise host_models.png_encode_rgb8(frames, band)[i]; a PNG decoder gives the frames back
    bit for bit.  offsets: (T + 1,) int64.  crcs: (T,) int32 - the bits of the CRC-32 of file i's zlib stream (its IDAT data;
    `& 0xFFFFFFFF` on the host), what host_models.ApngWriter forms its chunk CRCs from.
    band: rows per band, 1 ... H with band (1 + 3 W) <= 65536; None: default_band(H, W).  H, W: 1 ... 16384.
    out: a 1-d uint8 device tensor to write into; default: a new one of the frames' raw size (T * H * W * 3).  When the files
    need more than `out` holds, the one host read of the offsets (taken on every call: it synchronises the stream) tells, and
    the call is repeated into a new tensor of offsets[-1] bytes: the returned `data` is then NOT `out`.  Scratch comes from
    torch's allocator; everything runs on the current stream of the frames' device."""
    return _encode(frames_u8_dev, band, out)[:3]


class PngFrames(JpegFrames):
    """PNG files in host memory: jpeg.JpegFrames' interface - `data` a pinned 1-d uint8 tensor, `offsets` (n + 1,) int64 on the
    host, len(), indexing (a memoryview of the file, no copy), iteration, .nbytes - plus `crcs`: (n,) int64 on the host, the
    CRC-32 of every file's zlib stream (0 ... 2^32 - 1)."""

    def __init__(self, data, offsets, crcs):
        super().__init__(data, offsets)
        if crcs.is_cuda or crcs.dim() != 1 or crcs.numel() != len(self):
            raise ValueError("PngFrames takes one CRC per file, on the host")
        self.crcs = crcs.to(torch.int64) & 0xFFFFFFFF


def to_host(data_dev, edges, crcs, host=None, stream=None):
    """The files of (data on the device, offsets on the host, crcs on either side) -> PngFrames: offsets[-1] bytes and the CRCs
    cross PCIe, into `host` (a pinned uint8 tensor that holds them) or a new pinned tensor, on `stream` (default: the current
    one), which is synchronised."""
    total = int(edges[-1])
    if host is None:
        host = torch.empty(max(1, total), dtype=torch.uint8, pin_memory=True)
    elif host.numel() < total:
        raise ValueError("to_host: host holds %d bytes, the files need %d" % (host.numel(), total))
    stream = stream if stream is not None else torch.cuda.current_stream(data_dev.device)
    with torch.cuda.stream(stream):
        host[:total].copy_(data_dev[:total], non_blocking=True)
        crcs = crcs.cpu() if crcs.is_cuda else crcs  # synchronises `stream`: the copy above has landed too
    stream.synchronize()
    return PngFrames(host[:total], edges, crcs)


@torch.no_grad()
def encode_png_host(frames_u8_dev, band=None, out=None, host=None):
    """encode_png_device, then the files - offsets[-1] bytes and the CRCs, nothing else - into pinned host memory -> PngFrames,
    complete on return."""
    data, _, crcs, edges = _encode(frames_u8_dev, band, out)
    return to_host(data, edges, crcs, host)
