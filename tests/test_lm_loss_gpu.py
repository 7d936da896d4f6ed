"""mmfd_vocab_xent_fwd / mmfd_vocab_xent_bwd (csrc/lm_loss.hip) against the float64 restatement
tests/blip_loss_ref.py (itself held to torch in tests/test_lm_loss_cpu.py).

Bars, for loss rows, lse, the reductions and fp32 dlogits: 4 x the error of torch's own fp32 CPU computation
(cross_entropy, logsumexp, and cross_entropy's autograd) on the same inputs, measured against float64 inside
the test; the factor 4 is for a different reduction order. bf16 dlogits additionally get half a bf16 ulp of the
reference value. Every case prints its figures before it asserts (DESIGN.md, section 9 records them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import blip_loss_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CASES = {}


def _inputs(R, V, pad):
    """logits [R, V] as a view of a [R, V + pad] buffer (leading dimension > V when pad), labels with the first and
    the last column and (R > 1) one ignored row; cached per shape, never modified"""
    key = (R, V, pad)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * R + V + pad)
        z = torch.randn(R, V, generator=g) * 3.0
        y = torch.randint(0, V, (R,), generator=g)
        y[0] = V - 1
        if R > 1:
            y[1] = 0
        if R > 2:
            y[2] = L.IGNORE
        _CASES[key] = (z, y)
    return _CASES[key]


def _device_logits(z, pad):
    buf = torch.full((z.shape[0], z.shape[1] + pad), float("nan"), device=DEV)
    buf[:, :z.shape[1]] = z.to(DEV)
    return buf[:, :z.shape[1]]


def _ulp_bf16(x):
    """half a bf16 ulp of |x| (8 significand bits; the smallest normal's below 2^-126)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 0.5 * 2.0 ** (e - 7)


def _torch_fp32(z, y, eps, rps):
    """torch's own fp32 CPU results: loss rows, lse, mean, per-sequence sums, and the gradient of the mean"""
    zt = z.clone().requires_grad_(True)
    rows = F.cross_entropy(zt, y, reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    mean = F.cross_entropy(zt, y, reduction="mean", label_smoothing=eps, ignore_index=L.IGNORE)
    mean.backward()
    return dict(loss_rows=rows.detach().double().numpy(), lse=torch.logsumexp(z, 1).double().numpy(),
                mean=float(mean.detach().double()), seq_sums=rows.detach().view(-1, rps).sum(1).double().numpy(),
                grad=zt.grad.double().numpy())


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("pad", [0, 3], ids=["dense", "ld>V"])
@pytest.mark.parametrize("V", [200, 1001, 30524])
@pytest.mark.parametrize("R", [1, 5, 33])
def test_vocab_xent_matches_the_restatement(R, V, pad, eps):
    _check_case(R, V, pad, eps)


@pytest.mark.parametrize("V,ld", [(203, 208), (1001, 1008), (30524, 30528)])
def test_vector_paths_with_a_scalar_tail(V, ld):
    """rows padded to a multiple of 8 columns, as mmfd.blip lays them out (vocab_ld): both output dtypes take their
    16-byte path (8 bf16 / 4 fp32 columns per store) and V % 8 columns are left to the scalar tail, where row 0's
    label V - 1 lies"""
    assert ld % 8 == 0 and 0 < V % 8 and (V - 1) // 8 == V // 8
    _check_case(5, V, ld - V, 0.1)


def _check_case(R, V, pad, eps):
    from mmfd import kernels as K
    z, y = _inputs(R, V, pad)
    rps = R if R < 33 else 11
    ref = L.xent_fwd(z.numpy(), y.numpy(), eps, rows_per_seq=rps)
    t32 = _torch_fp32(z, y, eps, rps)
    zd, yd = _device_logits(z, pad), y.to(DEV)
    rows, lse, lse_lo, mean, n_valid, seq = K.vocab_xent_fwd(zd, yd, eps, rows_per_seq=rps)
    rows2, lse2, lse_lo2, mean2, _, seq2 = K.vocab_xent_fwd(zd, yd, eps, rows_per_seq=rps)
    torch.cuda.synchronize()
    for name, got in (("loss_rows", rows), ("lse", lse), ("mean", mean), ("seq_sums", seq)):
        err = np.abs(got.double().cpu().numpy() - ref[name]).max()
        bar = 4.0 * np.abs(t32[name] - ref[name]).max()
        print(f"vocab_xent_fwd R={R} V={V} ld={V + pad} eps={eps} {name}: err {err:.3e}, torch fp32 {bar / 4:.3e}, bar {bar:.3e}")
        assert err <= bar, name
    assert int(n_valid) == ref["n_valid"]
    assert (rows.cpu()[y == L.IGNORE] == 0.0).all()
    for a, b in ((rows, rows2), (lse, lse2), (lse_lo, lse_lo2), (mean, mean2), (seq, seq2)):  # the same inputs give the same bits
        assert torch.equal(a, b)

    ref_d = L.xent_bwd(z.numpy(), y.numpy(), ref["lse"], eps, n_valid=ref["n_valid"])
    bar = 4.0 * np.abs(t32["grad"] - ref_d).max()
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.full((R, V + pad), 7.0, device=DEV, dtype=dtype)
        d = K.vocab_xent_bwd(zd, yd, lse, lse_lo, eps, dtype, n_valid=n_valid, out=out[:, :V])
        d2 = K.vocab_xent_bwd(zd, yd, lse.clone(), lse_lo.clone(), eps, dtype, n_valid=n_valid)
        torch.cuda.synchronize()
        got = d.double().cpu().numpy()
        excess = np.abs(got - ref_d) - (_ulp_bf16(ref_d) if dtype == torch.bfloat16 else 0.0)
        print(f"vocab_xent_bwd R={R} V={V} ld={V + pad} eps={eps} {dtype}: err {np.abs(got - ref_d).max():.3e}, beyond the "
              f"storage rounding {excess.max():.3e}, torch fp32 {bar / 4:.3e}, bar {bar:.3e}")
        assert d.dtype == dtype and excess.max() <= bar
        assert torch.equal(d, d2)
        assert (got[y.numpy() == L.IGNORE] == 0.0).all()   # exact zeros
        assert (out[:, V:] == 7.0).all()                    # nothing written past V


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_per_sequence_weights_and_upstream(dtype):
    from mmfd import kernels as K
    R, V, rps, eps = 33, 1001, 11, 0.1
    z, y = _inputs(R, V, 0)
    ref = L.xent_fwd(z.numpy(), y.numpy(), eps, rows_per_seq=rps)
    zd, yd = z.to(DEV), y.to(DEV)
    _, lse, lse_lo, _, n_valid, _ = K.vocab_xent_fwd(zd, yd, eps, rows_per_seq=rps)
    w = torch.tensor([0.5, -2.0, 1.25])
    zt = z.clone().requires_grad_(True)
    rows = F.cross_entropy(zt, y, reduction="none", label_smoothing=eps, ignore_index=L.IGNORE)
    (rows.view(-1, rps).sum(1) * w).sum().backward()
    ref_d = L.xent_bwd(z.numpy(), y.numpy(), ref["lse"], eps, upstream=w.numpy(), rows_per_seq=rps)
    d = K.vocab_xent_bwd(zd, yd, lse, lse_lo, eps, dtype, upstream=w.to(DEV), rows_per_seq=rps)
    excess = np.abs(d.double().cpu().numpy() - ref_d) - (_ulp_bf16(ref_d) if dtype == torch.bfloat16 else 0.0)
    bar = 4.0 * np.abs(zt.grad.double().numpy() - ref_d).max()
    print(f"vocab_xent_bwd per-sequence {dtype}: beyond the storage rounding {excess.max():.3e}, bar {bar:.3e}")
    assert excess.max() <= bar
    up = torch.tensor([0.75], device=DEV)
    zt = z.clone().requires_grad_(True)
    (0.75 * F.cross_entropy(zt, y, label_smoothing=eps, ignore_index=L.IGNORE)).backward()
    ref_d = L.xent_bwd(z.numpy(), y.numpy(), ref["lse"], eps, upstream=0.75, n_valid=ref["n_valid"])
    d = K.vocab_xent_bwd(zd, yd, lse, lse_lo, eps, dtype, upstream=up, n_valid=n_valid)
    excess = np.abs(d.double().cpu().numpy() - ref_d) - (_ulp_bf16(ref_d) if dtype == torch.bfloat16 else 0.0)
    bar = 4.0 * np.abs(zt.grad.double().numpy() - ref_d).max()
    print(f"vocab_xent_bwd mean form with upstream {dtype}: beyond the storage rounding {excess.max():.3e}, bar {bar:.3e}")
    assert excess.max() <= bar


def test_no_valid_row_gives_nan_mean_and_zero_gradient():
    from mmfd import kernels as K
    z, _ = _inputs(5, 200, 0)
    y = torch.full((5,), L.IGNORE, dtype=torch.int64, device=DEV)
    rows, lse, lse_lo, mean, n_valid, seq = K.vocab_xent_fwd(z.to(DEV), y, 0.1, rows_per_seq=5)
    assert torch.isnan(mean).item() and int(n_valid) == 0 and (rows == 0).all() and (seq == 0).all()
    d = K.vocab_xent_bwd(z.to(DEV), y, lse, lse_lo, 0.1, torch.float32, n_valid=n_valid)
    assert (d == 0).all()


@pytest.mark.parametrize("V", [200, 30524])
def test_large_logits_stay_finite(V):
    from mmfd import kernels as K
    z = torch.where(torch.arange(2 * V).view(2, V) % 2 == 0, 3.0e4, -3.0e4)
    y = torch.tensor([0, 1])
    ref = L.xent_fwd(z.numpy(), y.numpy(), 0.1)
    t32 = F.cross_entropy(z, y, reduction="none", label_smoothing=0.1).double().numpy()
    rows, lse, lse_lo, mean, _, _ = K.vocab_xent_fwd(z.to(DEV), y.to(DEV), 0.1)
    d = K.vocab_xent_bwd(z.to(DEV), y.to(DEV), lse, lse_lo, 0.1, torch.float32, upstream=torch.ones(2, device=DEV),
                         rows_per_seq=1)
    assert torch.isfinite(rows).all() and torch.isfinite(lse).all() and torch.isfinite(mean) and torch.isfinite(d).all()
    err = np.abs(rows.double().cpu().numpy() - ref["loss_rows"]).max()
    bar = 4.0 * np.abs(t32 - ref["loss_rows"]).max()
    print(f"vocab_xent_fwd +-3e4 V={V}: loss {rows.tolist()}, err {err:.3e}, bar {bar:.3e}")
    assert err <= bar


def test_refusals_before_any_launch(monkeypatch):
    from mmfd import kernels as K
    z, y = _inputs(5, 200, 0)
    yd = y.to(DEV)
    flat = torch.zeros(5 * 200 + 8, device=DEV)
    off = flat[1:1 + 5 * 200].view(5, 200)  # 4 bytes past a 16-byte boundary
    with pytest.raises(RuntimeError, match="mmfd_vocab_xent_fwd.*aligned"):
        K.vocab_xent_fwd(off, yd)
    good = z.to(DEV)
    _, lse, lse_lo, _, n_valid, _ = K.vocab_xent_fwd(good, yd)
    with pytest.raises(RuntimeError, match="mmfd_vocab_xent_bwd.*aligned"):
        K.vocab_xent_bwd(off, yd, lse, lse_lo, 0.0, torch.float32, n_valid=n_valid)
    with pytest.raises(RuntimeError, match="mmfd_vocab_xent_bwd.*aligned"):
        K.vocab_xent_bwd(good, yd, lse, lse_lo, 0.0, torch.float32, n_valid=n_valid, out=off)
    # the wrapper takes lse and lse_lo only as the forward returned them: fp32, R entries, contiguous
    for a, b in ((lse, None), (lse.double(), lse_lo), (lse[:4], lse_lo), (lse, torch.zeros(10, device=DEV)[::2])):
        with pytest.raises(ValueError, match="lse"):
            K.vocab_xent_bwd(good, yd, a, b, 0.0, torch.float32, n_valid=n_valid)
    with pytest.raises(RuntimeError, match="mmfd_vocab_xent_fwd.*V = 0"):
        K.vocab_xent_fwd(good[:, :0], yd)
    with pytest.raises(RuntimeError, match="mmfd_vocab_xent_bwd.*V = 0"):
        K.vocab_xent_bwd(good[:, :0], yd, lse, lse_lo, 0.0, torch.float32, n_valid=n_valid,
                         out=torch.zeros(5, 8, device=DEV)[:, :0])
    # a label outside [0, V) that is not -100: refused on the host and nothing launched. Every launch of the wrappers
    # goes through kernels.lib() or kernels._ops(): here reaching either fails the test; and no device allocation is
    # made either (the wrapper allocates its outputs after the check)
    class Unreachable:
        def __getattr__(self, name):
            raise AssertionError(f"the library's {name} was reached")

    monkeypatch.setattr(K, "lib", lambda: Unreachable())
    monkeypatch.setattr(K, "_ops", lambda: Unreachable())
    for bad in (200, -1, -101):
        yb = y.clone()
        yb[3] = bad
        ybd = yb.to(DEV)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        with pytest.raises(ValueError, match="neither in"):
            K.vocab_xent_fwd(good, ybd, 0.1)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
