"""kernels.lm_head_argmax_wide (csrc/decode.hip): the LM head with the argmax fused for 1 <= B <= 256 rows, against
float64 products and, bit for bit, against kernels.lm_head_argmax on every 32-row block.

Constructions, tolerances and helpers are those of tests/test_caption_gpu.py (its `_planted`, `_bound`, `_rand`):
logits within atol + rtol * |ref|max with (3e-5, 3e-5) in fp32 and (2e-2, 2e-2) in bf16 of the float64 product of
the kernel's own (rounded) inputs. The shapes cover 1 .. 4 chunks of 16 bytes per lane in fp32 (1 and 2 in bf16:
wider bf16 rows do not fit a 32-row tile in LDS and are refused), a partial and a full last row tile, a vocabulary
that is no multiple of the slab, and B <= K (the planted rows are orthogonal)."""
import math

import pytest
import torch

from tests import test_caption_gpu as TC

pytestmark = pytest.mark.gpu
DEV = TC.DEV
DTYPES = TC.DTYPES
WIDE_CASES = [(33, 200, 96), (40, 1031, 96), (64, 200, 768), (255, 300, 768), (256, 300, 1024), (33, 200, 512)]


def _slab(dtype, V, Kd):
    """the wide kernel's slabs are the narrow kernel's at a full row tile"""
    from mmfd import kernels as K
    return K.lm_head_slab(dtype, 32, V, Kd)


def _check_planted(B, V, Kd, dtype):
    from mmfd import kernels as K
    slab = _slab(dtype, V, Kd)
    x, W, bias, win = TC._planted(B, V, Kd, dtype, slab)
    ref = x.double() @ W.double().t() + bias.double()
    bound32 = 3e-5 + 3e-5 * ref.abs().max().item()
    top2 = ref.topk(2, dim=-1)  # the planted winner leads by >= 100 x the fp32 bound: constructed, checked here
    assert (top2.indices[:, 0] == torch.tensor(win)).all()
    assert (top2.values[:, 0] - top2.values[:, 1]).min().item() >= 100 * bound32
    logits = torch.full((B, V + 3), 7.0, device=DEV)
    idx = K.lm_head_argmax_wide(x.to(DEV), W.to(DEV), bias.to(DEV), logits=logits[:, :V])
    idx2 = K.lm_head_argmax_wide(x.to(DEV), W.to(DEV), bias.to(DEV))  # without the logits output
    torch.cuda.synchronize()
    err = (logits[:, :V].double().cpu() - ref).abs().max().item()
    print(f"lm_head_wide {(B, V, Kd)} {dtype}: slab {slab}, logits err {err:.3e} (bound {TC._bound(dtype, ref):.3e})")
    assert err <= TC._bound(dtype, ref)
    assert (logits[:, V:] == 7.0).all()  # the three guard columns
    assert idx.dtype == torch.int64 and idx.cpu().tolist() == win and idx2.cpu().tolist() == win


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,V,Kd", WIDE_CASES)
def test_wide_logits_and_planted_winners(B, V, Kd, dtype):
    _check_planted(B, V, Kd, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,V,Kd", [(40, 1031, 96), (256, 300, 768)])
def test_every_32_row_block_is_the_narrow_kernel_bit_for_bit(B, V, Kd, dtype):
    from mmfd import kernels as K
    x, W, bias, _ = TC._planted(B, V, Kd, dtype, _slab(dtype, V, Kd))
    xd, Wd, bd = x.to(DEV), W.to(DEV), bias.to(DEV)
    wide = torch.zeros(B, V, device=DEV)
    idx = K.lm_head_argmax_wide(xd, Wd, bd, logits=wide)
    for r0 in range(0, B, 32):
        n = min(32, B - r0)
        blk = torch.zeros(32, Kd, device=DEV, dtype=dtype)  # a short last block is padded with zero rows
        blk[:n] = xd[r0:r0 + n]
        narrow = torch.zeros(32, V, device=DEV)
        nidx = K.lm_head_argmax(blk, Wd, bd, logits=narrow)
        assert torch.equal(wide[r0:r0 + n], narrow[:n]), f"rows {r0} .. {r0 + n - 1}"
        assert torch.equal(idx[r0:r0 + n], nidx[:n])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_wide_ties_and_nan_in_both_row_tiles(dtype):
    """test_caption_gpu's tie / NaN construction at B = 40, once on rows 0 .. 3 (row tile 0) and once on rows
    32 .. 35 (row tile 1): bit-identical rows of W with equal bias tie exactly and the lowest index wins, at two and
    at three positions across slabs; a NaN logit beside the winner is never chosen; nothing but NaN gives token 0"""
    from mmfd import kernels as K
    B, V, Kd = 40, 200, 96
    slab = _slab(dtype, V, Kd)
    assert 0 < slab < 40
    x, W, bias, _ = TC._planted(B, V, Kd, dtype, slab)
    W = W.double()
    W[[0, V - 1, slab - 1, slab]] = TC._rand(4, Kd, seed=14, scale=0.05).double()  # the planted winners go
    xr = x.double()
    plan = {0: dict(pair=(slab + 3, V - 2), triple=(5, slab + 1, 3 * slab + 2), nan_side=7, plain=150),
            32: dict(pair=(slab + 5, V - 4), triple=(9, 2 * slab + 1, 4 * slab + 2), nan_side=11, plain=151)}
    want = {}
    for base, p in plan.items():
        for rows, b in ((p["pair"], base), (p["triple"], base + 1)):
            W[list(rows)] = 2.0 * xr[b] / xr[b].norm()
            bias[list(rows)] = 0.25
            want[b] = min(rows)
        W[p["nan_side"]] = 2.0 * xr[base + 2] / xr[base + 2].norm()
        W[p["plain"]] = 2.0 * xr[base + 3] / xr[base + 3].norm()
        want[base + 2], want[base + 3] = p["nan_side"], p["plain"]
    W[8] = float("nan")  # beside row 7, and in every row's logits
    W = W.to(dtype)
    ref = x.double() @ W.double().t() + bias.double()
    assert torch.isnan(ref[:, 8]).all()
    for p in plan.values():
        assert torch.equal(W[p["pair"][0]], W[p["pair"][1]]) and torch.equal(W[p["triple"][0]], W[p["triple"][2]])
    rows = sorted(want)
    best = ref.nan_to_num(nan=-math.inf)
    top2 = best[rows].topk(4, dim=-1).values  # the tied rows hold the maximum, the others lie far below
    assert (top2[:, 0] - top2[:, 3]).min().item() > 1.0
    for b in rows:
        assert best[b, want[b]] >= best[b].max() - 1e-9  # (float64 BLAS may round tied columns apart in the last bit)
    idx = K.lm_head_argmax_wide(x.to(DEV), W.to(DEV), bias.to(DEV))
    torch.cuda.synchronize()
    assert [idx[b].item() for b in rows] == [want[b] for b in rows]
    idx = K.lm_head_argmax_wide(x.to(DEV), torch.full_like(W, float("nan")).to(DEV), bias.to(DEV))
    assert idx.cpu().tolist() == [0] * B


def test_wide_refuses_bad_arguments():
    from mmfd import kernels as K
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="mmfd_lm_head_argmax_wide"):
        K.lm_head_argmax_wide(z(0, 96), z(10, 96))       # no row
    with pytest.raises(RuntimeError, match="mmfd_lm_head_argmax_wide"):
        K.lm_head_argmax_wide(z(257, 96), z(10, 96))     # more than 256 rows
    with pytest.raises(RuntimeError, match="mmfd_lm_head_argmax_wide"):
        K.lm_head_argmax_wide(z(40, 98), z(10, 98))      # K * 4 bytes is no multiple of 16
    with pytest.raises(RuntimeError, match="mmfd_lm_head_argmax_wide"):  # a 32-row tile of x past 160 KiB of LDS
        K.lm_head_argmax_wide(z(40, 1536).bfloat16(), z(10, 1536).bfloat16())
    need = K.lm_head_wide_workspace_bytes(torch.float32, 40, 10, 96)
    assert need > 0
    small = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="mmfd_lm_head_argmax_wide.*workspace"):
        K.lm_head_argmax_wide(z(40, 96), z(10, 96), workspace=small)
    with pytest.raises(RuntimeError, match="mmfd_lm_head_argmax_wide"):
        K.lm_head_wide_workspace_bytes(torch.float32, 257, 10, 96)
    out = K.lm_head_argmax_wide(z(40, 96), z(10, 96), workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
    assert out.cpu().tolist() == [0] * 40                # all logits equal: the lowest index
