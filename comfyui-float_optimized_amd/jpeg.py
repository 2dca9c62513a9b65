"""Baseline JPEG files from 8-bit frames on the device (`float_jpg_encode`, include/float_hip.h).  The definition is
host_models.jpeg_encode_rgb8: colour conversion, chroma subsampling, the two DCT passes, the quantiser and the entropy coding are
integer arithmetic, and the kernels give its bytes.  What crosses PCIe afterwards is the files, not the frames."""
import ctypes as C

import torch

from . import native


def default_restart(w):
    """One MCU row per restart interval: the intervals of a frame are coded in parallel, one workgroup each."""
    return int(w) // 16


def check_pad(pad):
    """pad of the encode calls: None (sides must be multiples of 16) or "edge" (any size: float_jpg_encode_padded replicates the
    last row and column into the partial MCUs - host_models.jpeg_encode_rgb8(..., pad="edge") is the definition)."""
    if pad is not None and pad != "edge":
        raise ValueError("pad must be None or \"edge\" (got %r)" % (pad,))
    return pad


def pad_restart(w, pad=None):
    """The default restart interval, one MCU row: default_restart(w), with pad="edge" ceil(w / 16)."""
    return default_restart(w) if pad is None else -(-int(w) // 16)


def default_capacity(n_frames, h, w):
    """The default room for the files of n_frames frames: their I420 size."""
    return max(1, int(n_frames) * int(h) * int(w) * 3 // 2)


def _check_frames(x, quality, restart, pad=None):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise ValueError("encode_jpeg_device takes (T, H, W, 3) or (H, W, 3) uint8 frames on the GPU, got %s"
                         % ("%s %s on %s" % (x.dtype, tuple(x.shape), x.device) if isinstance(x, torch.Tensor) else type(x).__name__,))
    x = (x[None] if x.dim() == 3 else x).contiguous()
    return x, int(quality), pad_restart(x.shape[2], check_pad(pad)) if restart is None else int(restart)


def enqueue_encode(x, quality, restart, out, offsets, work=None, pad=None):
    """One float_jpg_encode call on the current stream, nothing read back: x (T, H, W, 3) uint8 contiguous on the GPU, out 1-d
    uint8 and offsets (T + 1,) int64 on the same device; work: scratch of float_jpg_work_bytes or None (allocated here, from
    torch's allocator).  pad="edge": float_jpg_encode_padded and float_jpg_work_bytes_padded instead - any H and W.  Returns work."""
    T, H, W, _ = (int(v) for v in x.shape)
    L = native.lib()
    work_bytes, encode = (L.float_jpg_work_bytes, L.float_jpg_encode) if check_pad(pad) is None else \
        (L.float_jpg_work_bytes_padded, L.float_jpg_encode_padded)
    need = int(work_bytes(max(T, 1), H, W, restart))
    with torch.cuda.device(x.device):
        if work is None or work.numel() < need:
            work = torch.empty(max(16, need), dtype=torch.uint8, device=x.device)
        native.check(encode(C.c_void_p(x.data_ptr()), T, H, W, quality, restart, C.c_void_p(out.data_ptr()), out.numel(),
                            C.c_void_p(offsets.data_ptr()), C.c_void_p(work.data_ptr()), work.numel(), native.stream_ptr(x.device)))
    return work


def _encode(frames_u8_dev, quality, restart, out, pad=None):
    """encode_jpeg_device, also returning the offsets as the host tensor the one read gave."""
    x, quality, restart = _check_frames(frames_u8_dev, quality, restart, pad)
    T, H, W, _ = (int(v) for v in x.shape)
    if out is not None and (not out.is_cuda or out.device != x.device or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous()):
        raise ValueError("encode_jpeg_device: out must be a contiguous 1-d uint8 tensor on %s" % (x.device,))
    with torch.cuda.device(x.device):
        if out is None:
            out = torch.empty(default_capacity(T, H, W), dtype=torch.uint8, device=x.device)
        offsets = torch.empty(T + 1, dtype=torch.int64, device=x.device)
        work = enqueue_encode(x, quality, restart, out, offsets, pad=pad)
        edges = offsets.cpu()  # the one host read
        if int(edges[-1]) > out.numel():
            out = torch.empty(int(edges[-1]), dtype=torch.uint8, device=x.device)
            enqueue_encode(x, quality, restart, out, offsets, work, pad)
    return out, offsets, edges


@torch.no_grad()
def encode_jpeg_device(frames_u8_dev, quality=90, restart=None, out=None, pad=None):
    """float_jpg_encode on (T, H, W, 3) or (H, W, 3) uint8 frames in HBM -> (data, offsets), both on the device: file i is
    data[offsets[i]:offsets[i + 1]], bitwise host_models.jpeg_encode_rgb8(frames, quality, restart)[i].  offsets: (T + 1,) int64.
    restart: MCUs per restart interval; None: one MCU row; 0: none (one serial chain per frame, slow).
    pad: None - H and W are multiples of 16, anything else is a ValueError; "edge" - any H and W in 1 ... 16384
    (float_jpg_encode_padded): the last row and column fill the partial MCUs, the files carry the true size and are bitwise
    host_models.jpeg_encode_rgb8(frames, quality, restart, pad="edge"); one MCU row is then ceil(W / 16) MCUs.
    out: a 1-d uint8 device tensor to write into; default: a new one of the frames' I420 size (T * H * W * 3 / 2).  When the
    files need more than `out` holds, the one host read of the offsets (taken on every call: it synchronises the stream) tells,
    and the call is repeated into a new tensor of offsets[-1] bytes: the returned `data` is then NOT `out`.  Scratch comes from
    torch's allocator; everything runs on the current stream of the frames' device."""
    return _encode(frames_u8_dev, quality, restart, out, pad)[:2]


class JpegFrames:
    """JPEG files in host memory: `data` a pinned 1-d uint8 tensor, `offsets` (n + 1,) int64 on the host; frame i is
    data[offsets[i]:offsets[i + 1]].  len(), indexing (a memoryview of the file, no copy), iteration, .nbytes (of the files)."""

    def __init__(self, data, offsets):
        if data.is_cuda or data.dtype != torch.uint8 or data.dim() != 1 or offsets.is_cuda or offsets.dtype != torch.int64 or offsets.dim() != 1:
            raise ValueError("JpegFrames takes a 1-d uint8 host tensor and 1-d int64 host offsets")
        self.data, self.offsets = data, offsets
        self._edges = offsets.tolist()
        self._bytes = data.numpy()

    def __len__(self):
        return len(self._edges) - 1

    def __getitem__(self, i):
        n = len(self)
        if not -n <= i < n:
            raise IndexError("frame %d of %d" % (i, n))
        i %= n
        return memoryview(self._bytes[self._edges[i]:self._edges[i + 1]])

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    @property
    def nbytes(self):
        return self._edges[-1] - self._edges[0]


def to_host(data_dev, edges, host=None, stream=None):
    """The files of (data on the device, offsets on the host) -> JpegFrames: offsets[-1] bytes cross PCIe, into `host` (a pinned
    uint8 tensor that holds them) or a new pinned tensor, on `stream` (default: the current one), which is synchronised."""
    total = int(edges[-1])
    if host is None:
        host = torch.empty(max(1, total), dtype=torch.uint8, pin_memory=True)
    elif host.numel() < total:
        raise ValueError("to_host: host holds %d bytes, the files need %d" % (host.numel(), total))
    stream = stream if stream is not None else torch.cuda.current_stream(data_dev.device)
    with torch.cuda.stream(stream):
        host[:total].copy_(data_dev[:total], non_blocking=True)
    stream.synchronize()
    return JpegFrames(host[:total], edges)


@torch.no_grad()
def encode_jpeg_host(frames_u8_dev, quality=90, restart=None, out=None, host=None, pad=None):
    """encode_jpeg_device, then the files - offsets[-1] bytes, nothing else - into pinned host memory -> JpegFrames, complete on
    return.  One host read of the offsets in all."""
    data, _, edges = _encode(frames_u8_dev, quality, restart, out, pad)
    return to_host(data, edges, host)
