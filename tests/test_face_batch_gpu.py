"""The face detector on n stacked views (float_sfd_*_batch, FaceDetectorHIP.*_batch): view i of every batched call is, bit for
bit, the single-view call on that view alone - maps, dense rows, boxes and counts, in fp16, bf16 and fp32 - so the batched path
stands on the limits test_face_detect_gpu.py holds the single-view path to against host_models.sfd_*.  The post-processing is
also checked against the definition on constructed maps, per view."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import test_face_detect_gpu as single
from tests.util import load_pkg

pytestmark = pytest.mark.gpu

pkg = load_pkg()
hm = pkg.host_models


@functools.lru_cache(maxsize=None)
def views_of(hw, n):
    """n distinct seeded views of one size; view 0 is test_face_detect_gpu's."""
    more = [torch.from_numpy(np.random.RandomState(7000 + 10 * hw[0] + i).randint(0, 256, size=hw + (3,)).astype(np.uint8)) for i in range(1, n)]
    return torch.stack([single.view_of(hw)] + more)


@functools.lru_cache(maxsize=None)
def detector(dtype, max_candidates=1024):
    return pkg.face.FaceDetectorHIP(single.state(), "cuda:0", dtype=dtype, max_hw=(144, 200), max_candidates=max_candidates,
                                    max_boxes=min(64, max_candidates))


@pytest.mark.parametrize("hw,n", [((45, 61), 3), ((72, 100), 3), ((16, 17), 2), ((45, 61), 1)])
@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
def test_maps_batch_is_bitwise_the_single_views(dtype, hw, n):
    """maps_batch on n distinct views against maps of each view alone: torch.equal on all 12 maps.  45 x 61: every pool floors
    and every conv has a partial tile, and a 64-pixel tile of a deep map holds pixels of more than one view; 16 x 17: the fifth
    pool floors to nothing and fc6 sees only padding; n = 1 is the single call."""
    det = detector(dtype)
    det.saturation(reset=True)
    views = views_of(hw, n).cuda()
    got = det.maps_batch(views)
    assert len(got) == n
    for i in range(n):
        want = det.maps(views[i])
        assert [tuple(g.shape) for g in got[i]] == [tuple(w.shape) for w in want]
        for lvl, (g, w) in enumerate(zip(got[i], want)):
            assert torch.equal(g, w), (dtype, hw, i, lvl, float((g - w).abs().max()))
    assert any(not torch.equal(a, b) for a, b in zip(got[0], got[-1])) or n == 1  # distinct views, distinct maps
    assert det.saturation() == 0


def _threshold(hw):
    """In the widest gap of the definition's scores near the 30th, as test_detect_twice_is_bitwise_equal puts it."""
    sc = np.sort(hm.sfd_decode_dense(single.ref_maps(hw))[:, 4])[::-1]
    k = 20 + int(np.argmax(sc[20:40] - sc[21:41]))
    return float(0.5 * (sc[k] + sc[k + 1]))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_detect_batch_is_bitwise_the_single_calls(dtype):
    """detect_batch on 4 distinct 72 x 100 views: rows, counts and dense rows are those of four detect calls, bit for bit; a
    second call repeats the first; host views (uploaded once) give the same; float_sfd_dense afterwards is view 0's rows."""
    hw, n = (72, 100), 4
    thr = _threshold(hw)
    det = detector(dtype)
    det.saturation(reset=True)
    views = views_of(hw, n).cuda()
    want = []
    for i in range(n):
        rows = det.detect(views[i], score_thr=thr)
        want.append((rows, det._boxes.clone(), det._counts.clone(), det.dense(*hw)))
    runs = []
    for _ in range(2):
        rows = det.detect_batch(views, score_thr=thr)
        runs.append((rows, det._bboxes[:n].clone(), det._bcounts[:n].clone(), det.dense_batch(n, *hw)))
    (r0, b0, c0, d0), (r1, b1, c1, d1) = runs
    assert r0 == r1 and torch.equal(b0, b1) and torch.equal(c0, c1) and torch.equal(d0, d1)
    for i, (rows, boxes, counts, dense) in enumerate(want):
        kept = int(counts[0])
        assert r0[i] == rows and torch.equal(c0[i], counts) and torch.equal(d0[i], dense), i
        assert torch.equal(b0[i, :kept], boxes[:kept]), i
    assert det.counts_batch() == [tuple(int(v) for v in c) for c in c0.tolist()]
    assert 0 < int(c0[0, 0]) <= int(c0[0, 1]) <= 64  # view 0 selects something (the threshold is made for it)
    assert torch.equal(det.dense(*hw), d0[0])
    assert det.detect_batch(views_of(hw, n), score_thr=thr) == r0
    assert det.detect_batch(views, score_thr=thr, max_batch=3) == r0  # groups of 3 / 1
    assert det.saturation() == 0


def test_detect_batch_on_identical_views():
    hw, n = (72, 100), 4
    thr = _threshold(hw)
    det = detector("fp16")
    views = single.view_of(hw).cuda()[None].repeat(n, 1, 1, 1)
    rows = det.detect_batch(views, score_thr=thr)
    dense = det.dense_batch(n, *hw)
    assert len(rows[0]) > 0 and all(r == rows[0] for r in rows) and all(torch.equal(dense[i], dense[0]) for i in range(n))
    kept = len(rows[0])  # rows beyond the kept ones are not written
    assert torch.equal(det._bboxes[:n, :kept], det._bboxes[:1, :kept].expand(n, -1, -1))
    assert torch.equal(det._bcounts[:n], det._bcounts[:1].expand(n, -1))
    assert rows[0] == det.detect(views[0], score_thr=thr)


# ---------------------------------------------------------------------------------------------- post-processing
POST_HW = single.POST_HW
POST_SEEDS = (0, 3, 4)  # chosen on the CPU so that constructed_maps' margins (asserted there, with the definition alone) hold


def _empty_maps():
    """Background only: no position comes near the threshold."""
    maps = []
    for h, w in hm.sfd_map_sizes(*POST_HW):
        conf = torch.zeros(1, 2, h, w)
        conf[0, 0], conf[0, 1] = 10.0, -10.0
        maps += [conf, torch.zeros(1, 4, h, w)]
    return maps


def _thinned(maps, dense, keep):
    """The constructed maps with all but the `keep` best candidates turned into background: a subset of the candidates, so
    every margin of constructed_maps still holds."""
    maps = [m.clone() for m in maps]
    order = np.argsort(-dense[:, 4])
    sizes = hm.sfd_map_sizes(*POST_HW)
    firsts = np.cumsum([0] + [h * w for h, w in sizes])
    for p in order[keep:]:
        if dense[p, 4] <= 0.5:
            break
        lvl = int(np.searchsorted(firsts, p, side="right") - 1)
        y, x = divmod(int(p - firsts[lvl]), sizes[lvl][1])
        maps[2 * lvl][0, 0, y, x], maps[2 * lvl][0, 1, y, x] = 10.0, -10.0
    return maps, hm.sfd_decode_dense(maps)


@functools.lru_cache(maxsize=None)
def post_views():
    """[(maps, dense of the definition, candidates)]: three constructed views, an empty one, a thinned one (5 candidates)."""
    out = [single.constructed_maps(seed=s) for s in POST_SEEDS]
    e = _empty_maps()
    de = hm.sfd_decode_dense(e)
    assert float(de[:, 4].max()) < 0.5 - 1e-3
    out.append((e, de, 0))
    t, dt = _thinned(out[0][0], out[0][1], 5)
    assert int((dt[:, 4] > 0.5).sum()) == 5
    out.append((t, dt, 5))
    return out


def test_post_batch_on_constructed_maps():
    """post_batch on five views: each view's kept list, order and counts are sfd_select's on that view; the empty view reports
    {0, 0} and an empty list."""
    pv = post_views()
    det = detector("fp32")
    before = det.fallbacks
    got = det.post_batch([m for m, _, _ in pv], *POST_HW)
    counts = det.counts_batch()
    dense = det.dense_batch(len(pv), *POST_HW).cpu().double().numpy()
    for i, (maps, want_dense, n_cand) in enumerate(pv):
        want = hm.sfd_select(want_dense, 0.5, 0.3)
        single._same_list(got[i], want)
        assert counts[i] == (len(want), n_cand), i
        assert float(np.abs(dense[i][:, 4] - want_dense[:, 4]).max()) < 1e-5
    assert got[3] == [] and counts[3] == (0, 0)
    assert 0 < len(got[0]) < pv[0][2] and det.fallbacks == before
    # and each view alone, through the single-view call, bit for bit
    for i, (maps, _, _) in enumerate(pv):
        assert det.post(maps, *POST_HW) == got[i], i


def test_post_batch_with_one_view_beyond_the_capacity():
    """max_candidates = 8: the empty view, a constructed view (over 30 candidates) and the thinned view (5) in one batch.  The
    middle one reports {0, candidates} and is selected by the definition on its dense rows - fallbacks rises by exactly one -
    and its neighbours are selected by the kernel as if it were not there."""
    pv = post_views()
    batch = [pv[3], pv[1], pv[4]]
    det = detector("fp32", 8)
    before = det.fallbacks
    got = det.post_batch([m for m, _, _ in batch], *POST_HW)
    assert det.fallbacks == before + 1
    counts = det.counts_batch()
    want = [hm.sfd_select(d, 0.5, 0.3) for _, d, _ in batch]
    assert counts == [(0, 0), (0, batch[1][2]), (len(want[2]), 5)] and batch[1][2] > 8
    for g, w in zip(got, want):
        single._same_list(g, w)
    assert got[0] == [] and len(got[2]) > 0


def test_batch_refusals_against_the_reservation():
    """n above the reserved n and a view beyond the reserved size are refused with FLOAT_E_INVALID, naming the function and the
    argument; nothing was launched (the handle still works)."""
    det = pkg.face.FaceDetectorHIP(single.state(), "cuda:0", dtype="fp16", max_hw=(72, 100), max_candidates=64, max_boxes=16)
    L, N = pkg.native.lib(), pkg.native
    st = N.stream_ptr(det.device)
    views = views_of((45, 61), 3).cuda()
    flat = torch.zeros(3, 6 * sum(h * w for h, w in hm.sfd_map_sizes(45, 61)), device="cuda:0")
    boxes, counts = torch.zeros(3, 16, 5, device="cuda:0"), torch.zeros(3, 2, dtype=torch.int32, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def maps_call(n, H, W):
        return L.float_sfd_maps_batch(det._h, p(views), n, H, W, p(flat), st)

    assert maps_call(1, 45, 61) == 1 and b"float_sfd_maps_batch" in L.float_last_error() and b"float_sfd_reserve_batch" in L.float_last_error()
    N.check(L.float_sfd_reserve_batch(det._h, 2, 45, 61))
    assert maps_call(3, 45, 61) == 1 and b"n = 3" in L.float_last_error() and b"2 reserved" in L.float_last_error()
    assert maps_call(2, 46, 61) == 1 and b"46 x 61" in L.float_last_error() and b"reserved 45 x 61" in L.float_last_error()
    assert L.float_sfd_detect_batch(det._h, p(views), 3, 45, 61, 0.5, 0.3, p(boxes), p(counts), st) == 1
    assert b"float_sfd_detect_batch" in L.float_last_error() and b"n = 3" in L.float_last_error()
    assert L.float_sfd_post_batch(det._h, p(flat), 2, 45, 62, 0.5, 0.3, p(boxes), p(counts), st) == 1
    assert b"float_sfd_post_batch" in L.float_last_error() and b"45 x 62" in L.float_last_error()
    assert L.float_sfd_maps_batch(det._h, None, 2, 45, 61, p(flat), st) == 1 and b"null argument" in L.float_last_error()
    assert L.float_sfd_reserve_batch(det._h, 2, 73, 100) == 1 and b"max_h x max_w" in L.float_last_error()
    assert L.float_sfd_reserve_batch(det._h, 65, 45, 61) == 1 and b"1 ... 64" in L.float_last_error()
    N.check(L.float_sfd_reserve_batch(det._h, 1, 40, 50))  # never shrinks: 2 views of 45 x 61 still pass
    assert maps_call(2, 45, 61) == 0
    N.check(L.float_sfd_reserve_batch(det._h, 3, 45, 61))
    assert maps_call(3, 45, 61) == 0
    got = det.maps_batch(views)  # the wrapper after a reservation made behind its back
    assert torch.equal(torch.cat([m.reshape(-1) for m in got[2]]), flat[2])
    det.close()
