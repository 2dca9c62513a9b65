"""bench.py's --dump-outputs writer on small host tensors (the GPU run itself: tests/test_bench_gpu.py)."""
import importlib.util
import os

import numpy as np
import torch

from tests.util import ROOT

spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _frames(n, size):
    return torch.rand(n, size, size, 3, generator=torch.Generator().manual_seed(5))


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_frames_when_they_fit(tmp_path):
    f = _frames(4, 16)
    bench.dump_outputs(str(tmp_path), f)
    out = _read(tmp_path)
    assert list(out) == ["frames"] and out["frames"].dtype == np.float32
    assert np.array_equal(out["frames"], f.numpy())


def test_dump_sample_is_fixed_and_within_the_limit(tmp_path):
    f = _frames(30, 32)
    limit = 120_000  # half of it goes to the pixel sample, the rest holds 4 whole frames of 12 KiB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), f, limit=limit)
    a, b = _read(tmp_path / "a"), _read(tmp_path / "b")
    assert sorted(a) == ["frames_pixels", "frames_sample"]
    assert all(np.array_equal(a[k], b[k]) for k in a)  # same arguments, same arrays
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= limit
    s = a["frames_sample"]
    assert 1 < len(s) < len(f) and np.array_equal(s[0], f[0].numpy()) and np.array_equal(s[-1], f[-1].numpy())
    assert a["frames_pixels"].size == limit // 8 and np.isin(a["frames_pixels"], f.numpy()).all()


def test_dump_default_limit_holds_a_full_clip():
    """The default budget at the benchmark's own size (250 frames of 512 x 512): under 64 MB whichever way MB is read."""
    frame = 512 * 512 * 3 * 4
    n_px = min(2**20, bench.DUMP_LIMIT // 8)
    k = (bench.DUMP_LIMIT - 4 * n_px) // frame
    assert k >= 8 and k * frame + 4 * n_px <= bench.DUMP_LIMIT < 64 * 10**6
