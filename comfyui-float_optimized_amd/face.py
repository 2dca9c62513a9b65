"""The face detector of the face-aligned crop on the HIP operator `float_sfd_*` (include/float_hip.h): S3FD forward, score /
box decoding and NMS on the detector's view of the portrait, once per clip.  host_models.sfd_forward / sfd_decode_dense /
sfd_nms are the definition; the weight file is the `face_alignment` package's (s3fd-619a316812.pth), found on disk and never
downloaded."""
import ctypes as C
import os

import torch

from . import host_models, native

SFD_WEIGHTS_ENV = "FLOAT_AMD_SFD_WEIGHTS"
SFD_HUB_FILE = "s3fd-619a316812.pth"


def _models_dir():
    try:
        import folder_paths
        return folder_paths.models_dir
    except Exception:  # noqa: BLE001
        return os.environ.get("FLOAT_MODELS_DIR", os.path.join(os.path.expanduser("~"), "ComfyUI", "models"))


def sfd_weight_candidates(models_dir=None):
    """Where find_sfd_weights looks, in order."""
    d = os.path.join(models_dir if models_dir is not None else _models_dir(), "face_alignment")
    env = os.environ.get(SFD_WEIGHTS_ENV)
    return ([env] if env else []) + [os.path.join(d, "s3fd.safetensors"), os.path.join(d, "s3fd.pth"), os.path.join(d, SFD_HUB_FILE),
                                     os.path.join(os.path.expanduser("~"), ".cache", "torch", "hub", "checkpoints", SFD_HUB_FILE)]


def find_sfd_weights(models_dir=None):
    """The first existing file of sfd_weight_candidates, or None.  FLOAT_AMD_SFD_WEIGHTS naming a file that does not exist is
    an error, not a reason to look further.  Nothing is downloaded."""
    env = os.environ.get(SFD_WEIGHTS_ENV)
    if env and not os.path.isfile(env):
        raise FileNotFoundError("%s=%s: no such file" % (SFD_WEIGHTS_ENV, env))
    for p in sfd_weight_candidates(models_dir):
        if os.path.isfile(p):
            return p
    return None


def load_sfd_state(path):
    """The state dict of a weight file (.safetensors, or a .pth read with torch.load(weights_only=True)), checked strictly: a
    missing or extra key, or a wrong shape, is a ValueError that names it."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        state = load_file(path, device="cpu")
    else:
        state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict):
        raise ValueError("%s does not hold a state dict" % path)
    return host_models.sfd_check_state({k: v.float() for k, v in state.items()}, path)


@native.rebuildable
class FaceDetectorHIP:
    """S3FD on the device.  `state`: the s3fd state dict (checked strictly).  max_hw: the largest view (rows, columns) the
    handle's workspace is sized for - 360 rows is process_img's view, 4096 columns the image front end's limit for it."""

    def __init__(self, state, device="cuda:0", dtype="fp16", max_hw=(360, 4096), max_candidates=1024, max_boxes=256):
        host_models.sfd_check_state(state)
        self.device = torch.device(device)
        self.dtype = dtype = native.canon_dtype(dtype)
        self.max_hw = (int(max_hw[0]), int(max_hw[1]))
        self.max_candidates, self.max_boxes = int(max_candidates), int(max_boxes)
        self.fallbacks = 0  # calls whose candidates exceeded the capacity and were selected by the definition
        arr, keep = native.tensor_table(state)
        cfg = native.SfdCfg(native.DTYPES[dtype], self.max_hw[0], self.max_hw[1], self.max_candidates, self.max_boxes)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_create(C.byref(cfg), arr, len(state), C.byref(h)))
            self._boxes = torch.zeros(self.max_boxes, 5, dtype=torch.float32, device=self.device)
            self._counts = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._h = h
        self._reserved, self._bboxes, self._bcounts, self._last_counts = (0, 0, 0), None, None, []  # reserve_batch
        del keep

    def close(self):
        if getattr(self, "_h", None) and native is not None:
            native.lib().float_sfd_destroy(self._h)
            self._h = None
            self._boxes = self._counts = self._bboxes = self._bcounts = None
            self._reserved = (0, 0, 0)

    __del__ = close

    def saturation(self, reset=False):
        """Threads with a clamped (+-65504) 16-bit activation store since create / the last reset (float_sfd_saturation): 0
        unless the weights leave fp16's range; dtype="fp32" is the remedy.  Synchronises the current stream."""
        with torch.cuda.device(self.device):
            return native.saturation("float_sfd_saturation", self._h, self.device, reset)

    def _view(self, rgb8):
        v = torch.as_tensor(rgb8)
        if v.dim() != 3 or v.shape[-1] != 3 or v.dtype != torch.uint8:
            raise ValueError("the detector's view must be (H, W, 3) uint8, got %s %s" % (tuple(v.shape), v.dtype))
        return v.to(self.device).contiguous()  # a host-made view (the H <= 360 route) is uploaded here

    def _select(self, H, W, score_thr, iou_thr):
        """Rows and counts of the call just enqueued -> the list; the definition on the dense rows where the kernel's capacity
        (max_candidates, max_boxes) was exceeded."""
        counts = self._counts.cpu()  # synchronises: the two counts, then only the kept rows
        kept, cand = int(counts[0]), int(counts[1])
        if cand <= self.max_candidates and kept <= self.max_boxes:
            return [[float(v) for v in row] for row in self._boxes[:kept].cpu().tolist()]
        self.fallbacks += 1
        return host_models.sfd_select(self.dense(H, W).cpu().double().numpy(), score_thr, iou_thr)

    @torch.no_grad()
    def detect(self, rgb8, score_thr=0.5, iou_thr=0.3):
        """[[x1, y1, x2, y2, score], ...] in keep order for the (H, W, 3) uint8 view: what detect_from_image returns."""
        v = self._view(rgb8)
        H, W = int(v.shape[0]), int(v.shape[1])
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_detect(self._h, C.c_void_p(v.data_ptr()), H, W, float(score_thr), float(iou_thr),
                                                       C.c_void_p(self._boxes.data_ptr()), C.c_void_p(self._counts.data_ptr()),
                                                       native.stream_ptr(self.device)))
        return self._select(H, W, score_thr, iou_thr)

    __call__ = detect

    @torch.no_grad()
    def post(self, maps, H, W, score_thr=0.5, iou_thr=0.3):
        """The post-processing alone (float_sfd_post) on 12 maps in sfd_forward's format for an H x W view."""
        flat = torch.cat([m.to(self.device, torch.float32).reshape(-1) for m in maps]).contiguous()
        if flat.numel() != 6 * sum(h * w for h, w in host_models.sfd_map_sizes(H, W)):
            raise ValueError("the maps are not those of a %d x %d view" % (H, W))
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_post(self._h, native.dev_ptr(flat), int(H), int(W), float(score_thr), float(iou_thr),
                                                     C.c_void_p(self._boxes.data_ptr()), C.c_void_p(self._counts.data_ptr()),
                                                     native.stream_ptr(self.device)))
        return self._select(int(H), int(W), score_thr, iou_thr)

    def counts(self):
        """(kept, candidates) of the last detect / post call, as the kernel reported them."""
        c = self._counts.cpu()
        return int(c[0]), int(c[1])

    def dense(self, H, W):
        """The (P, 5) dense rows [x1, y1, x2, y2, score] of the last detect / post call, which was on an H x W view."""
        P = sum(h * w for h, w in host_models.sfd_map_sizes(H, W))
        out = torch.empty(P, 5, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_dense(self._h, native.dev_ptr(out), native.stream_ptr(self.device)))
        return out

    # ------------------------------------------------------------------------------------------ n stacked views in one pass
    def _views(self, views):
        v = torch.as_tensor(views)
        if v.dim() != 4 or v.shape[-1] != 3 or v.dtype != torch.uint8 or v.shape[0] < 1:
            raise ValueError("the detector's stacked views must be (N, H, W, 3) uint8 with N >= 1, got %s %s" % (tuple(v.shape), v.dtype))
        return v.to(self.device).contiguous()  # host-made views are uploaded here, once

    def reserve_batch(self, n, H, W):
        """Grow the handle's workspace to n views of H x W (float_sfd_reserve_batch): the only batched call that allocates.
        A no-op when the reservation already covers it."""
        n, H, W = int(n), int(H), int(W)
        rn, rh, rw = self._reserved
        if n <= rn and H <= rh and W <= rw:
            return
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_reserve_batch(self._h, n, H, W))
            self._reserved = (max(n, rn), max(H, rh), max(W, rw))
            self._bboxes = torch.zeros(self._reserved[0], self.max_boxes, 5, dtype=torch.float32, device=self.device)
            self._bcounts = torch.zeros(self._reserved[0], 2, dtype=torch.int32, device=self.device)

    def _select_batch(self, n, H, W, score_thr, iou_thr):
        """Rows and counts of the batched call just enqueued -> n lists, read back with ONE device-to-host copy (counts and
        rows packed into one buffer); the definition on a view's dense rows where that view exceeded the capacity."""
        packed = torch.cat([self._bcounts[:n].view(torch.float32).reshape(-1), self._bboxes[:n].reshape(-1)]).cpu()  # synchronises
        counts = packed[:2 * n].view(torch.int32).view(n, 2).tolist()
        rows = packed[2 * n:].view(n, self.max_boxes, 5)
        out, dense = [], None
        for i, (kept, cand) in enumerate(counts):
            if cand <= self.max_candidates and kept <= self.max_boxes:
                out.append([[float(v) for v in row] for row in rows[i, :kept].tolist()])
                continue
            self.fallbacks += 1
            if dense is None:
                dense = self.dense_batch(n, H, W).cpu().double().numpy()
            out.append(host_models.sfd_select(dense[i], score_thr, iou_thr))
        self._last_counts = [tuple(c) for c in counts]
        return out

    @torch.no_grad()
    def detect_batch(self, views, score_thr=0.5, iou_thr=0.3, max_batch=16):
        """N lists in detect's format for (N, H, W, 3) uint8 views of one size, on the device or on the host: the views go
        through float_sfd_detect_batch in groups of at most max_batch, with one device-to-host copy per group.  View i's list
        is bitwise detect's for that view alone."""
        v = self._views(views)
        N, H, W = int(v.shape[0]), int(v.shape[1]), int(v.shape[2])
        max_batch = max(1, min(int(max_batch), 64))
        out, counts = [], []
        for at in range(0, N, max_batch):
            n = min(max_batch, N - at)
            self.reserve_batch(n, H, W)
            with torch.cuda.device(self.device):
                native.check(native.lib().float_sfd_detect_batch(self._h, C.c_void_p(v[at:at + n].data_ptr()), n, H, W, float(score_thr),
                                                                 float(iou_thr), C.c_void_p(self._bboxes.data_ptr()),
                                                                 C.c_void_p(self._bcounts.data_ptr()), native.stream_ptr(self.device)))
            out += self._select_batch(n, H, W, score_thr, iou_thr)
            counts += self._last_counts
        self._last_counts = counts
        return out

    @torch.no_grad()
    def post_batch(self, maps, H, W, score_thr=0.5, iou_thr=0.3):
        """The post-processing alone (float_sfd_post_batch) on n views' maps: a list of n lists of 12 maps in sfd_forward's
        format, or an (n, 6 P) tensor in float_sfd_maps_batch's layout."""
        H, W = int(H), int(W)
        P6 = 6 * sum(h * w for h, w in host_models.sfd_map_sizes(H, W))
        if torch.is_tensor(maps):
            flat = maps.to(self.device, torch.float32).contiguous()
        else:
            flat = torch.stack([torch.cat([m.to(self.device, torch.float32).reshape(-1) for m in one]) for one in maps]).contiguous()
        if flat.dim() != 2 or flat.shape[1] != P6:
            raise ValueError("the maps are not those of %d x %d views" % (H, W))
        n = int(flat.shape[0])
        self.reserve_batch(n, H, W)
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_post_batch(self._h, native.dev_ptr(flat), n, H, W, float(score_thr), float(iou_thr),
                                                           C.c_void_p(self._bboxes.data_ptr()), C.c_void_p(self._bcounts.data_ptr()),
                                                           native.stream_ptr(self.device)))
        return self._select_batch(n, H, W, score_thr, iou_thr)

    def counts_batch(self):
        """[(kept, candidates), ...] per view of the last detect_batch / post_batch call, as the kernel reported them."""
        return list(self._last_counts)

    def dense_batch(self, n, H, W):
        """The (n, P, 5) dense rows of the last detect_batch / post_batch call, which was on n views of H x W."""
        P = sum(h * w for h, w in host_models.sfd_map_sizes(H, W))
        out = torch.empty(int(n), P, 5, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_dense_batch(self._h, native.dev_ptr(out), native.stream_ptr(self.device)))
        return out

    @torch.no_grad()
    def maps_batch(self, views):
        """Per view the 12 maps as sfd_forward returns them (float_sfd_maps_batch): a list of N lists, fp32, on the device."""
        v = self._views(views)
        N, H, W = int(v.shape[0]), int(v.shape[1]), int(v.shape[2])
        sizes = host_models.sfd_map_sizes(H, W)
        flat = torch.empty(N, 6 * sum(h * w for h, w in sizes), dtype=torch.float32, device=self.device)
        self.reserve_batch(N, H, W)
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_maps_batch(self._h, C.c_void_p(v.data_ptr()), N, H, W, native.dev_ptr(flat),
                                                           native.stream_ptr(self.device)))
        out = []
        for i in range(N):
            one, at = [], 0
            for h, w in sizes:
                one.append(flat[i, at:at + 2 * h * w].view(1, 2, h, w))
                one.append(flat[i, at + 2 * h * w:at + 6 * h * w].view(1, 4, h, w))
                at += 6 * h * w
            out.append(one)
        return out

    @torch.no_grad()
    def maps(self, rgb8):
        """The 12 maps of the view as sfd_forward returns them (float_sfd_maps): fp32, on the device."""
        v = self._view(rgb8)
        H, W = int(v.shape[0]), int(v.shape[1])
        sizes = host_models.sfd_map_sizes(H, W)
        flat = torch.empty(6 * sum(h * w for h, w in sizes), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            native.check(native.lib().float_sfd_maps(self._h, C.c_void_p(v.data_ptr()), H, W, native.dev_ptr(flat), native.stream_ptr(self.device)))
        out, at = [], 0
        for h, w in sizes:
            out.append(flat[at:at + 2 * h * w].view(1, 2, h, w))
            out.append(flat[at + 2 * h * w:at + 6 * h * w].view(1, 4, h, w))
            at += 6 * h * w
        return out
