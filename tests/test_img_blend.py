"""Multi-band (Laplacian pyramid) paste-back without a GPU: the properties of the definition, host_models.paste_multiband_rgb8; the
mask pyramid of float_img_blend_plan integer for integer against it; the refusals of the C entries; the public keyword."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
hm = pkg.host_models


def noise(seed, *shape):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


SRC, FRAMES = noise(1, 80, 96, 3), noise(2, 2, 32, 32, 3)  # a 96 x 80 portrait


@pytest.mark.parametrize("resample", [None, "bicubic"])
def test_equal_face_and_portrait_give_the_portrait(resample):
    """F == S: every D_l is zero.  The frames are the portrait's own window, pasted at scale one."""
    rect = (20, 10, 48, 40)
    frames = SRC[10:50, 20:68][None].repeat(2, 1, 1, 1)
    out = hm.paste_multiband_rgb8(SRC, frames, rect, inset=8, levels=2, resample=resample)
    assert torch.equal(out, SRC[None].repeat(2, 1, 1, 1))


@pytest.mark.parametrize("levels", [1, 3])
def test_no_open_side_gives_the_face(levels):
    rect = (-5, -6, 120, 110)
    out = hm.paste_multiband_rgb8(SRC, FRAMES, rect, inset=8, levels=levels)
    assert torch.equal(out, hm.paste_rgb8(SRC, FRAMES, rect, 0))
    assert torch.equal(hm.paste_multiband_rgb8(SRC, FRAMES, (200, 10, 20, 20)), SRC[None].repeat(2, 1, 1, 1))  # the box misses the image


def test_full_and_empty_support():
    """96 x 80 portrait, 64 x 48 box, inset 8, 2 levels: a pixel whose whole support has mask 256 is the face, mask 0 the portrait.
    With two levels pixel x reads M_2 at cells (x >> 2) - 2 ... + 1 or so, each of which reads M_0 at 4 c +- 6: worked through
    the shifts, M_0 within x - 15 ... x + 12.  The rim of mask 0 is 8 wide, narrower than that support, so the all-zero side of the
    property is checked outside the window and, with an inset that no cell of the box reaches, over the whole box."""
    rect, inset, m = (16, 16, 64, 48), 8, 15
    out = hm.paste_multiband_rgb8(SRC, FRAMES, rect, inset=inset, levels=2)
    face = hm.paste_rgb8(SRC, FRAMES, rect, 0)
    x0, y0, w, h = rect
    core = (slice(None), slice(y0 + inset + m, y0 + h - inset - m), slice(x0 + inset + m, x0 + w - inset - m))
    assert core[1].stop > core[1].start and torch.equal(out[core], face[core])
    outside = torch.ones(80, 96, dtype=torch.bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    portrait = SRC[None].repeat(2, 1, 1, 1)
    assert torch.equal(out[:, outside], portrait[:, outside])
    assert not torch.equal(out, face) and not torch.equal(out, hm.paste_rgb8(SRC, FRAMES, rect, inset))  # a blend of its own
    assert torch.equal(hm.paste_multiband_rgb8(SRC, FRAMES, rect, inset=24, levels=2), portrait)  # d <= 23 everywhere: mask 0


@pytest.mark.parametrize("levels", [0, 9, -1, 1.5])
def test_levels_outside_1_to_8_raise(levels):
    with pytest.raises(ValueError, match="levels"):
        hm.paste_multiband_rgb8(SRC, FRAMES, (16, 16, 64, 48), inset=8, levels=levels)


def test_default_levels():
    assert [hm.blend_levels("t", i) for i in (0, 2, 7, 8, 15, 16, 64, 16384)] == [1, 1, 1, 2, 2, 3, 5, 8]


# a box inside the image, clipped on two sides, reaching outside on all four, and one on the right and bottom edges
PLAN_CASES = [((80, 96), (16, 16, 64, 48), 8, 2), ((80, 96), (-7, -9, 50, 41), 5, 3), ((33, 31), (-2, -3, 40, 40), 4, 8),
              ((80, 97), (60, 50, 37, 30), 3, 1), ((5, 3), (1, 1, 1, 1), 0, 3)]


@pytest.mark.parametrize("hw,rect,inset,levels", PLAN_CASES)
def test_plan_is_the_definitions_mask_pyramid(hw, rect, inset, levels):
    table, sizes = pkg.image.blend_plan(*hw, rect, inset, levels)
    masks = hm.blend_masks(*hw, rect, inset, levels)
    assert len(masks) == levels + 1 and sizes == [m.shape for m in masks]
    assert table.dtype == torch.int16 and table.numel() == sum(m.size for m in masks)
    assert np.array_equal(table.numpy(), np.concatenate([m.ravel() for m in masks]))


def test_refusals_need_no_gpu():
    L = pkg.native.lib()
    t = (C.c_int16 * 64)()
    plan = lambda *a: L.float_img_blend_plan(*a, t, 64)  # noqa: E731  src_h, src_w, rect x, y, w, h, inset, levels
    for args, word in [((0, 8, 0, 0, 4, 4, 1, 1), "src_h"), ((8, 8, 0, 0, 0, 4, 1, 1), "rect_w"), ((8, 8, 0, 0, 4, 4, -1, 1), "inset"),
                       ((8, 8, 0, 0, 4, 4, 1, 9), "levels"), ((8, 8, 9, 0, 4, 4, 1, 1), "misses"), ((8, 8, 0, 0, 8, 8, 1, 1), "table_ints")]:
        assert plan(*args) == 1 and ("float_img_blend_plan: " in L.float_last_error().decode() and word in L.float_last_error().decode()), args
    assert L.float_img_blend_plan(8, 8, 0, 0, 4, 4, 1, 1, None, 64) == 1 and b"null" in L.float_last_error()
    assert L.float_img_blend_plan_ints(5, 3, 1) == 15 + 6 and L.float_img_blend_plan_ints(5, 3, 0) == 0
    assert L.float_img_blend_work_bytes(1, 5, 3, 9) == 0 and L.float_img_blend_work_bytes(0, 5, 3, 1) == 0
    assert L.float_img_blend_work_bytes(2, 5, 3, 2) == 2 * (48 + 16 + 80)  # D_1 3 x 2, D_2 2 x 1 as int16 x 3; R_1 as int32 x 3; 16-byte steps
    p = C.c_void_p(256)  # never dereferenced: every check comes before any HIP call
    blend = lambda **k: L.float_img_blend(*dict(dict(s=p, H=8, W=8, f=p, n=1, x=2, y=2, h=4, w=4, lv=1, m=p, wk=p, wb=1 << 20, o=p, st=None), **k).values())  # noqa: E731
    for k, word in [(dict(s=None), "null"), (dict(n=0), "n_frames"), (dict(lv=9), "levels"), (dict(x=5), "window"), (dict(h=0), "window"),
                    (dict(m=C.c_void_p(257)), "mask"), (dict(wk=C.c_void_p(264)), "work"), (dict(wb=8), "work_bytes"), (dict(W=0), "src_w")]:
        assert blend(**k) == 1 and word in L.float_last_error().decode(), k


def test_blend_defaults_to_none_everywhere():
    agent, hot = importlib.import_module(pkg.__name__ + ".src.nodes.generate").InferenceAgent, pkg.pipeline.FloatHotPath
    fns = [pkg.image.paste_frames_device, pkg.image.paste_scratch, agent.infer_pasted, agent.stream_pasted, agent.infer_pasted_jpeg,
           agent.stream_pasted_jpeg, agent.infer_pasted_png, agent.stream_pasted_png, agent.write_video, agent.write_apng,
           hot.generate_pasted, hot.stream_to_host_pasted, hot.generate_to_jpeg, hot.stream_to_jpeg, hot.generate_to_png, hot.stream_to_png]
    for fn in fns:
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in ("blend", "inset", "levels")] == [None, None, None], fn.__qualname__
    for kw, word in [(dict(blend="laplace"), "blend"), (dict(inset=4), "inset and levels"), (dict(blend="multiband", feather=3), "feather"),
                     (dict(blend="multiband", out_format="i420"), "RGB"), (dict(blend="multiband", inset=-1), "inset")]:
        with pytest.raises(ValueError, match=word):
            pkg.image.blend_spec("t", kw.pop("blend", None), rect=(0, 0, 64, 64), **kw)
