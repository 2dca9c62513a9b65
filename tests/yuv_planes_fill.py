"""The one helper of the PlanarYuv tests: a buffer of frames in a given YuvPlanes layout, junk everywhere that is not a sample."""
import numpy as np
import torch


def fill_planes(fmt, frames, seed, values=None, extremes=False):
    """-> (flat uint8 tensor of `frames` frames of fmt, [Y, U, V] sample arrays (frames, rows, cols)).  Every byte is seeded junk
    first - padding, gaps, the unused bits of a 16-bit word - then the planes get seeded samples, or `values` (from another call).
    extremes: the first two samples of every plane are 0 and 2^depth - 1."""
    rs = np.random.RandomState(seed)
    buf = rs.randint(0, 256, (frames - 1) * fmt.frame_stride + fmt.last_end).astype(np.uint8)
    cw, ch, b = -(-fmt.w // fmt.hs), -(-fmt.h // fmt.vs), 1 if fmt.depth == 8 else 2
    made = []
    for i, (off, rows, cols, pitch, step) in enumerate(((fmt.y_off, fmt.h, fmt.w, fmt.y_pitch, b), (fmt.u_off, ch, cw, fmt.c_pitch, fmt.c_step),
                                                       (fmt.v_off, ch, cw, fmt.c_pitch, fmt.c_step))):
        v = rs.randint(0, 1 << fmt.depth, (frames, rows, cols)) if values is None else values[i]
        if extremes:
            v.reshape(frames, -1)[:, :2] = (0, (1 << fmt.depth) - 1)
        junk = rs.randint(0, 1 << 16, v.shape)
        keep = ((1 << fmt.depth) - 1) << fmt.shift
        word = (v << fmt.shift) | (junk & ~keep & (255 if b == 1 else 65535))
        at = lambda o: np.lib.stride_tricks.as_strided(buf[o:], v.shape, (fmt.frame_stride, pitch, step))  # noqa: E731
        at(off)[...] = word & 255
        if b == 2:
            at(off + 1)[...] = word >> 8
        made.append(v)
    return torch.from_numpy(buf), made
