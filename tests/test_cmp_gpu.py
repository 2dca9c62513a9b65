"""float_cmp_segments against torch in fp64 on seeded data: every segment length class (shorter than a 16-byte group, no aligned
body, ragged head and tail, one latent window, one 512-px frame), one / eight / 250 segments, both inputs one element off an
aligned base (the body of `a` is aligned, the body of `b` is or is not), NaN and +-inf planted on both sides.
Bounds: counts and the maximum are exact (integers; fp64 max of exactly representable differences).  The sums are fp64 from the
first add, so against any other summation order they are within seg_len * 2^-53 relative (all terms are positive): 8.8e-11 for a
512-px frame, rounded up to 1e-10 for every case.  Two calls are bitwise equal (no atomics), a == b gives exact zeros."""
import numpy as np
import pytest
import torch

from tests.util import load_pkg

pkg = load_pkg()
N = pkg.native
pytestmark = pytest.mark.gpu

THR = 2.0 / 255
CASES = [(n_seg, seg_len) for seg_len in (1, 3, 1023, 25600, 786432) for n_seg in (1, 8)] + [(250, 1), (250, 3), (250, 1023), (250, 25600)]


def _pair(n_seg, seg_len, off_a, off_b, plant=True):
    """a, b as slices starting off_a / off_b elements into freshly allocated (aligned) buffers; b = a + a perturbation whose
    size straddles the threshold."""
    n = n_seg * seg_len
    rs = np.random.RandomState(1000 + 7 * n_seg + seg_len % 9973)
    base_b = rs.standard_normal(n).astype(np.float32) * 0.5
    base_a = base_b + rs.standard_normal(n).astype(np.float32) * np.float32(THR)
    if plant:
        idx = rs.randint(0, n, size=min(n, 12))
        vals = [np.nan, np.inf, -np.inf]
        for j, i in enumerate(idx):
            (base_a if j % 2 else base_b)[i] = vals[j % 3]
        if n >= 2:  # both sides non-finite in one pair counts once
            base_a[idx[0]] = np.inf
    buf_a = torch.zeros(n + 8, dtype=torch.float32, device="cuda:0")
    buf_b = torch.zeros(n + 8, dtype=torch.float32, device="cuda:0")
    assert buf_a.data_ptr() % 16 == 0 and buf_b.data_ptr() % 16 == 0
    a, b = buf_a[off_a:off_a + n], buf_b[off_b:off_b + n]
    a.copy_(torch.from_numpy(base_a))
    b.copy_(torch.from_numpy(base_b))
    return a, b


def _want(a, b, n_seg, seg_len):
    a64, b64 = a.double().reshape(n_seg, seg_len), b.double().reshape(n_seg, seg_len)
    fin = torch.isfinite(a64) & torch.isfinite(b64)
    zero = torch.zeros((), dtype=torch.float64, device=a.device)
    d = torch.where(fin, a64 - b64, zero)
    bb = torch.where(fin, b64, zero)
    thr = torch.tensor(THR, dtype=torch.float32).double().item()  # the C call takes thr as a float
    return torch.stack([(d * d).sum(1), (bb * bb).sum(1), d.abs().amax(1), (d.abs() > thr).sum(1).double(),
                        (~fin).sum(1).double()], dim=1)


@pytest.mark.parametrize("off_a,off_b", [(1, 1), (1, 0), (0, 3)])
@pytest.mark.parametrize("n_seg,seg_len", CASES)
def test_cmp_segments_vs_torch_fp64(n_seg, seg_len, off_a, off_b):
    a, b = _pair(n_seg, seg_len, off_a, off_b)
    got = N.cmp_segments(a, b, seg_len, THR)
    again = N.cmp_segments(a, b, seg_len, THR)
    want = _want(a, b, n_seg, seg_len)
    torch.cuda.synchronize()
    assert got.shape == (n_seg, 5) and got.dtype == torch.float64 and got.is_cuda
    assert torch.equal(got, again), "two calls on the same inputs must be bitwise equal"
    got, want = got.cpu(), want.cpu()
    rel = ((got[:, :2] - want[:, :2]).abs() / want[:, :2].clamp_min(1e-300)).max().item()
    print("cmp %d x %d (a + %d, b + %d): sums rel %.2e, non-finite pairs %d, beyond thr %d" % (
        n_seg, seg_len, off_a, off_b, rel, int(want[:, 4].sum()), int(want[:, 3].sum())))
    assert torch.equal(got[:, 2:], want[:, 2:]), "max and counts are exact"
    assert rel <= 1e-10
    if n_seg * seg_len >= 2:
        assert want[:, 4].sum() > 0  # the planted NaN / inf are in play


@pytest.mark.parametrize("n_seg,seg_len", [(1, 3), (8, 1023), (8, 786432)])
def test_identical_buffers_give_exact_zeros(n_seg, seg_len):
    a, _ = _pair(n_seg, seg_len, 1, 1, plant=False)
    got = N.cmp_segments(a, a.clone(), seg_len, 0.0).cpu()
    assert torch.equal(got[:, [0, 2, 3, 4]], torch.zeros(n_seg, 4, dtype=torch.float64))
    assert torch.allclose(got[:, 1], a.double().reshape(n_seg, seg_len).pow(2).sum(1).cpu(), rtol=1e-10, atol=0)


def test_work_buffer_needs_no_zeroing_and_host_mirror_validates():
    """A large comparison leaves partials in the cached scratch; a small one after it must not see them."""
    a, b = _pair(8, 786432, 1, 1)
    N.cmp_segments(a, b, 786432, THR)
    a2, b2 = _pair(8, 1023, 1, 0)
    got = N.cmp_segments(a2, b2, 1023, THR).cpu()
    want = _want(a2, b2, 8, 1023).cpu()
    assert torch.equal(got[:, 2:], want[:, 2:]) and torch.allclose(got[:, :2], want[:, :2], rtol=1e-10, atol=0)
    with pytest.raises(ValueError):
        N.cmp_segments(a2, b2, 1000, THR)  # not whole segments
    with pytest.raises(ValueError):
        N.cmp_segments(a2, b2[:-1], 1023, THR)
    with pytest.raises(ValueError):
        N.cmp_segments(a2.cpu(), b2.cpu(), 1023, THR)
    with pytest.raises(TypeError):
        N.cmp_segments(a2.double(), b2.double(), 1023, THR)
