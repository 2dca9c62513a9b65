#!/usr/bin/env python3
"""Records the velocities one float_fmt_eval produces for every case of tests/test_fmt_launch_head_gpu.py into
tests/golden/fmt_tail_parent.npz, on an MI355X:

    python tools/make_tail_golden.py [out.npz]

Run on the build whose numbers are to be held - the commit BEFORE a change to the step chain's kernels that must not move a
bit; tests/test_fmt_launch_tail_gpu.py then compares the changed build with torch.equal.  Inputs, weights and the call are the
test's own (_case / _eval), so the fixture holds the project's output only.  Keys: "<n_prev>_<n_cur>_<way>_<dtype>[_full]"."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_fmt_launch_head_gpu as H  # noqa: E402

CASES = [(p, c, way, dt, False) for p, c in [(0, 1), (2, 15), (10, 50)] for way in (1, 3, 4) for dt in ("fp16", "bf16", "fp32")]
CASES.append((10, 50, 3, "fp16", True))


def key(n_prev, n_cur, way, dtype, full):
    return "%d_%d_%d_%s%s" % (n_prev, n_cur, way, dtype, "_full" if full else "")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fmt_tail_parent.npz")
    got = {}
    for n_prev, n_cur, way, dtype, full in CASES:
        cfg, sd, dev, ref = H._case(n_prev, n_cur, way, full)
        fmt = H.pkg.fmt.FlowMatchingTransformerHIP(sd, cfg, "cuda:0", dtype)
        try:
            v = H._eval(fmt, dev, way, torch.zeros(1, cfg.n_tokens, cfg.dim_w, device="cuda:0"))
            torch.cuda.synchronize()
            err = H.rel_l2(v.cpu(), ref)
            assert err < H.TOL[dtype], (key(n_prev, n_cur, way, dtype, full), err)
            got[key(n_prev, n_cur, way, dtype, full)] = v.cpu().numpy()
        finally:
            fmt.close()
    np.savez_compressed(out, **got)
    print("wrote %s: %d cases, %d bytes" % (out, len(got), os.path.getsize(out)))


if __name__ == "__main__":
    main()
