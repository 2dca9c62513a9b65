"""host_models.drive_rows, the plain definition of the driving rows, against the oracle's Direction in float64."""
import torch

from oracle import float_oracle as O
from tests.util import load_pkg

pkg = load_pkg()


def test_drive_rows_are_direction_of_composed_lambdas():
    dsd = pkg.weights.synth_decoder_state(64, seed=4)
    g = torch.Generator().manual_seed(1)
    lam, src, start = (torch.randn(n, 20, generator=g, dtype=torch.float64) for n in (6, 1, 1))
    q, _ = torch.linalg.qr(dsd["direction.weight"].double() + 1e-8)
    d = lambda x: O.direction(dsd, x, torch.float64)
    H = pkg.host_models
    assert torch.allclose(H.drive_rows(lam, q, "absolute"), d(lam), rtol=0, atol=1e-13)
    assert torch.allclose(H.drive_rows(lam, q, "relative", src, start), d(lam) - d(start) + d(src), rtol=0, atol=1e-13)
    assert torch.equal(H.drive_rows(lam, q, "relative", src), H.drive_rows(lam, q, "relative", src, lam[0:1]))
