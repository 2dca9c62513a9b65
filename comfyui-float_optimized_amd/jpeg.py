"""Baseline JPEG files from 8-bit frames on the device (`float_jpg_encode`, include/float_hip.h).  The definition is
host_models.jpeg_encode_rgb8: colour conversion, chroma subsampling, the two DCT passes, the quantiser and the entropy coding are
integer arithmetic, and the kernels give its bytes.  What crosses PCIe afterwards is the files, not the frames.
The way back is `float_jpg_decode`: baseline JPEG files -> 8-bit frames on the device, bitwise host_models.jpeg_decode_rgb8."""
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


def host_files(files):
    """JpegFrames, or a list of bytes-likes (one JPEG file each) -> (data, offsets): a 1-d uint8 host tensor holding the files
    back to back and (n + 1,) int64 host offsets counted from data[0].  A JpegFrames whose offsets start at 0 is used as it is."""
    if isinstance(files, JpegFrames):
        base = files._edges[0]
        return files.data[base:files._edges[-1]], files.offsets - base
    parts = [bytes(f) for f in files]
    if not parts:
        raise ValueError("decode_jpeg_device: no files")
    edges = [0]
    for p in parts:
        edges.append(edges[-1] + len(p))
    data = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8) if edges[-1] else torch.zeros(0, dtype=torch.uint8)
    return data, torch.tensor(edges, dtype=torch.int64)


ENTROPY = {None: 0, "interval": 0, "sync": 1, "auto": 2, "split": 3}


def entropy_id(entropy, sync_bytes=None):
    """(entropy, sync_bytes) of the decode calls -> float_jpg_decode_plan_entropy's two integers.  entropy: None or "interval" (a
    lane per restart interval), "sync" (every frame WITHOUT restart markers has its scan cut into up to 1024 subsequences that
    as many lanes decode, bit for bit the serial result), "auto" (sync for such frames from 64 KB of scan on) or "split" (every
    frame with at most 512 restart intervals has its intervals cut into subsequences, up to 1024 per frame dealt out by the
    intervals' lengths, and the chains never cross a marker; a frame without markers is one interval and decodes as under
    "sync").  sync_bytes: the shortest subsequence, 1 ... 65536; None is the library's default."""
    if entropy not in ENTROPY:
        raise ValueError("entropy must be None, \"interval\", \"sync\", \"auto\" or \"split\" (got %r)" % (entropy,))
    if sync_bytes is not None and (isinstance(sync_bytes, bool) or not isinstance(sync_bytes, int) or not 1 <= sync_bytes <= 65536):
        raise ValueError("sync_bytes must be None or an int in 1 ... 65536 (got %r)" % (sync_bytes,))
    return ENTROPY[entropy], 0 if sync_bytes is None else sync_bytes


class JpegPlan:
    """float_jpg_decode_plan of n files in host memory (data, offsets as host_files gives them): `.ints` the plan as an int32 host
    tensor cut to the words in use, and n, h, w, components, sampling, group.  No GPU is needed; what float_jpg_decode_plan
    refuses is a ValueError naming the frame.  entropy, sync_bytes: entropy_id's; anything but None / "interval" goes through
    float_jpg_decode_plan_entropy, and a plan in which no frame takes the sync or the split route is the plain plan word for word."""

    def __init__(self, data, offsets, entropy=None, sync_bytes=None):
        route, sync = entropy_id(entropy, sync_bytes)
        if data.is_cuda or offsets.is_cuda or data.dtype != torch.uint8 or offsets.dtype != torch.int64 or data.dim() != 1 or offsets.dim() != 1:
            raise ValueError("JpegPlan takes a 1-d uint8 host tensor and 1-d int64 host offsets")
        data, offsets = data.contiguous(), offsets.contiguous()
        n = offsets.numel() - 1
        if n < 1 or int(offsets[0]) < 0 or int(offsets[-1]) > data.numel():
            raise ValueError("JpegPlan: %d offsets over %d bytes" % (offsets.numel(), data.numel()))
        L = native.lib()
        ints = torch.empty(int(L.float_jpg_decode_plan_ints(n)), dtype=torch.int32)
        args = (C.c_void_p(data.data_ptr()), C.c_void_p(offsets.data_ptr()), n, C.c_void_p(ints.data_ptr()), ints.numel())
        native.check(L.float_jpg_decode_plan_entropy(*args, route, sync) if route else L.float_jpg_decode_plan(*args))
        self.ints = ints[:int(ints[1])].clone()
        self.n, self.h, self.w, self.components = (int(v) for v in self.ints[2:6])
        self.sampling, self.group = (int(self.ints[6]), int(self.ints[7])), int(self.ints[13])
        self.work_bytes = int(L.float_jpg_decode_work_bytes(C.c_void_p(self.ints.data_ptr())))


def decode_jpeg_host(files, entropy=None, sync_bytes=None):
    """float_jpg_decode_host: the kernels' rule run on the host, no GPU -> ((n, H, W, 3) uint8 host tensor, (n,) int32 status).
    entropy, sync_bytes: as in decode_jpeg_device; the sync and split routes' steps then run with their lanes as a loop."""
    data, offsets = host_files(files)
    plan = JpegPlan(data, offsets, entropy, sync_bytes)
    out = torch.empty(plan.n, plan.h, plan.w, 3, dtype=torch.uint8)
    status = torch.empty(plan.n, dtype=torch.int32)
    native.check(native.lib().float_jpg_decode_host(C.c_void_p(data.data_ptr()), C.c_void_p(offsets.data_ptr()), C.c_void_p(plan.ints.data_ptr()),
                                                    plan.n, C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr())))
    return out, status


def enqueue_decode(data_dev, offsets_dev, plan, out, status, work=None):
    """One float_jpg_decode call on the current stream, nothing read back: data_dev / offsets_dev the files and their offsets on
    the GPU, plan the JpegPlan made of their host copies, out (n, H, W, 3) uint8 and status (n,) int32 on the same device; work:
    scratch of plan.work_bytes or None (allocated here, from torch's allocator).  Returns (work, the plan's device copy).
    Lifetime: tensors that came from torch's caching allocator on this device (data_dev, offsets_dev, work, the plan's copy) may
    be dropped right after the call - the allocator hands a freed block only to work enqueued LATER on the same stream, and this
    call runs on the current stream.  Memory from anywhere else (another allocator, another stream's pool) must stay alive
    until the stream has run the call."""
    dev = data_dev.device
    with torch.cuda.device(dev):
        if work is None or work.numel() < plan.work_bytes:
            work = torch.empty(max(16, plan.work_bytes), dtype=torch.uint8, device=dev)
        plan_dev = plan.ints.to(dev, non_blocking=True)
        native.check(native.lib().float_jpg_decode(
            C.c_void_p(data_dev.data_ptr()), C.c_void_p(offsets_dev.data_ptr()), C.c_void_p(plan_dev.data_ptr()), C.c_void_p(plan.ints.data_ptr()),
            plan.n, C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(work.data_ptr()), work.numel(), native.stream_ptr(dev)))
    return work, plan_dev


STATUS_BITS = {1: "a code that matches no symbol or a run past coefficient 63", 2: "a wrong number of restart markers",
               4: "a scan that ends early"}


@torch.no_grad()
def decode_jpeg_device(files, offsets=None, strict=True, out=None, device=None, return_status=False, entropy=None, sync_bytes=None):
    """float_jpg_decode: baseline JPEG files -> (T, H, W, 3) uint8 frames on the device, frame i bitwise
    host_models.jpeg_decode_rgb8(file i) (which states what is accepted and the arithmetic; a valid file decodes as libjpeg-turbo
    decodes it).  files: a JpegFrames, a list of bytes-likes - planned on the host and uploaded as files, so only the files' bytes
    (and a plan of a few KB) cross PCIe - or a 1-d uint8 DEVICE tensor with `offsets` ((T + 1,) int64, host or device), the layout
    encode_jpeg_device returns: the headers are then read back for planning (one synchronising copy of the files to the host).
    All files of a call share size, components and sampling; tables and restart intervals may differ.
    entropy: None or "interval" gives every restart interval a lane, so a file without restart markers - what ffmpeg, Pillow
    and most cameras write - is decoded by a single lane; "sync" cuts such a file's scan into up to 1024 subsequences, decoded
    by as many lanes that fall into step with the serial decode (entropy_id; three more launches per group, the same bytes);
    "auto" does so from 64 KB of scan on.  Files with restart markers take the interval route under these.  "split" (opt-in)
    cuts the intervals of a file with up to 512 of them into subsequences as well, up to 1024 lanes per frame whose chains stop
    at the markers: for files with a marker every few MCU rows, which the interval route decodes on a handful of lanes; files
    with more intervals keep a lane per interval, files without markers decode as under "sync".
    sync_bytes: the shortest subsequence (None: the library's default).
    strict: a frame whose status word is not 0 raises ValueError naming the first such frame (one read-back of T words, which
    synchronises); strict=False returns the definition's pixels for damaged frames too and reads nothing back.
    out: a (T, H, W, 3) uint8 device tensor to write into.  return_status=True: (frames, (T,) int32 device tensor)."""
    if isinstance(files, torch.Tensor):
        if offsets is None or not files.is_cuda or files.dtype != torch.uint8 or files.dim() != 1:
            raise ValueError("decode_jpeg_device: a tensor of files must be 1-d uint8 on the GPU and come with offsets")
        dev = files.device
        edges = torch.as_tensor(offsets).to("cpu", torch.int64)
        base, end = int(edges[0]), int(edges[-1])
        data_dev = files[base:end].contiguous()
        data, edges = data_dev.cpu(), edges - base
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        data, edges = host_files(files)
        data_dev = None
    plan = JpegPlan(data, edges, entropy, sync_bytes)
    shape = (plan.n, plan.h, plan.w, 3)
    if out is not None and (not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous()):
        raise ValueError("decode_jpeg_device: out must be a contiguous %s uint8 tensor on the GPU" % (shape,))
    with torch.cuda.device(dev):
        if data_dev is None:
            data_dev = data.to(dev, non_blocking=True)
        out = torch.empty(shape, dtype=torch.uint8, device=dev) if out is None else out
        status = torch.empty(plan.n, dtype=torch.int32, device=dev)
        enqueue_decode(data_dev, edges.to(dev, non_blocking=True), plan, out, status)
        if strict:
            check_status(status.cpu())
    return (out, status) if return_status else out


def check_status(status_host, first=0):
    """ValueError naming the first frame of a decode whose status word is not 0."""
    bad = torch.nonzero(status_host).flatten()
    if bad.numel():
        i, st = int(bad[0]), int(status_host[int(bad[0])])
        raise ValueError("decode_jpeg_device: frame %d is damaged (status %d: %s)"
                         % (first + i, st, "; ".join(v for k, v in STATUS_BITS.items() if st & k)))


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
