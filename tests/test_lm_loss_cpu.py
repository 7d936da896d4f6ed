"""tests/blip_loss_ref.py (the float64 restatement of csrc/lm_loss.hip) against torch's cross_entropy and its
autograd in float64: both are exact formulas evaluated in float64, so they agree to 1e-12 of the largest value."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import blip_loss_ref as L

B, T1 = 3, 5  # 3 sequences of 5 scored positions


def _case(V, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B * T1, V, generator=g, dtype=torch.float64) * 3.0
    y = torch.randint(0, V, (B * T1,), generator=g)
    y[0], y[1] = 0, V - 1         # first and last column
    y[3] = L.IGNORE               # an ignored row inside a scored sequence
    y[T1:2 * T1] = L.IGNORE       # a sequence with all labels ignored
    return z, y


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", [200, 1001])
def test_restatement_matches_torch_float64(V, eps):
    z, y = _case(V, 7 + V)
    ref_rows = F.cross_entropy(z, y, reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    ref_mean = F.cross_entropy(z, y, reduction="mean", label_smoothing=eps, ignore_index=L.IGNORE)
    out = L.xent_fwd(z.numpy(), y.numpy(), eps, rows_per_seq=T1)
    tol = 1e-12 * max(1.0, ref_rows.abs().max().item())
    assert np.abs(out["loss_rows"] - ref_rows.numpy()).max() <= tol
    assert np.abs(out["lse"] - torch.logsumexp(z, 1).numpy()).max() <= tol
    assert abs(out["mean"] - ref_mean.item()) <= tol
    assert out["n_valid"] == int((y != L.IGNORE).sum()) == B * T1 - T1 - 1
    assert np.abs(out["seq_sums"] - ref_rows.view(B, T1).sum(1).numpy()).max() <= 10 * tol
    assert (out["loss_rows"][y.numpy() == L.IGNORE] == 0.0).all() and out["seq_sums"][1] == 0.0

    # mean form with an upstream factor, and the per-sequence form with one weight per sequence
    up = 0.75
    zt = z.clone().requires_grad_(True)
    (up * F.cross_entropy(zt, y, reduction="mean", label_smoothing=eps, ignore_index=L.IGNORE)).backward()
    d = L.xent_bwd(z.numpy(), y.numpy(), out["lse"], eps, upstream=up, n_valid=out["n_valid"])
    assert np.abs(d - zt.grad.numpy()).max() <= 1e-12
    assert (d[y.numpy() == L.IGNORE] == 0.0).all()
    w = torch.tensor([0.5, -2.0, 1.25], dtype=torch.float64)
    zt = z.clone().requires_grad_(True)
    rows = F.cross_entropy(zt, y, reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    (rows.view(B, T1).sum(1) * w).sum().backward()
    d = L.xent_bwd(z.numpy(), y.numpy(), out["lse"], eps, upstream=w.numpy(), rows_per_seq=T1)
    assert np.abs(d - zt.grad.numpy()).max() <= 1e-12
    assert (d[y.numpy() == L.IGNORE] == 0.0).all()


def test_no_valid_row_gives_nan_mean_and_zero_gradient():
    z, y = _case(200, 3)
    y[:] = L.IGNORE
    out = L.xent_fwd(z.numpy(), y.numpy(), 0.1, rows_per_seq=T1)
    assert np.isnan(out["mean"]) and out["n_valid"] == 0 and (out["seq_sums"] == 0.0).all()
    assert torch.isnan(F.cross_entropy(z, y, label_smoothing=0.1, ignore_index=L.IGNORE))
    d = L.xent_bwd(z.numpy(), y.numpy(), out["lse"], 0.1, n_valid=0)
    assert (d == 0.0).all()


def test_large_logits_stay_finite():
    z = np.where(np.arange(400).reshape(2, 200) % 2 == 0, 3.0e4, -3.0e4)
    out = L.xent_fwd(z, np.array([0, 1]), 0.1)
    assert np.isfinite(out["loss_rows"]).all() and np.isfinite(out["lse"]).all()
    ref = F.cross_entropy(torch.from_numpy(z), torch.tensor([0, 1]), reduction="none", label_smoothing=0.1)
    assert np.abs(out["loss_rows"] - ref.numpy()).max() <= 1e-12 * 6e4
