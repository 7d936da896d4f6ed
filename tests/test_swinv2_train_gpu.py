"""Trainable Swinv2 encoder on the HIP path: the new operators (csrc/swin_train.hip) against the float64
references of tests/swinv2_bwd_refs.py (proved against autograd in tests/test_swinv2_bwd_ref_cpu.py) and
tests/attention_refs.py, the model's gradients against transformers (tests/golden/swinv2_small_grads*.npz,
make_swinv2_grads.py), the opt-in semantics and the trainer.

Tolerances. Kernels: the suite's rule err <= atol + rtol * |ref|max with (3e-5, 3e-5) in fp32 and (2e-2,
2e-2) in bf16; the bias sum applies it per summed term: n * (atol + rtol * max_b |dS_b|max), n = B / M batch
rows per bias row. Model, fp32: every parameter gradient within 5e-4 * max(1, |ref|max) (the bar of
test_deberta_train_gpu.py; transformers' own fp32-vs-float64 deviation on this fixture is 6.6e-6). Model,
bf16: per tensor |delta|max / max(1, |ref|max) <= 2 * emul_worst_rel and cosine >= 1 - 2 * (1 -
emul_min_cos), both read from the fixture (the cost of bf16 activations with exact arithmetic, measured by
the generator: 9.25e-2 and 0.99678; the kernels round at more points than that emulation — the attention
probabilities, the normalised operands, the saved GELU derivative — hence the factor 2, as the DeBERTa
bf16 bar)."""
import numpy as np
import pytest
import torch

from tests import attention_refs as A
from tests import swinv2_bwd_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LS = (0.5, 2.3, 5.0, -1.0)  # cycled over the heads; 5.0 is past the clamp ln 100


def _tol(dtype):
    return (3e-5, 3e-5) if dtype == torch.float32 else (2e-2, 2e-2)


def _close(got, ref, dtype, what, n=1, scale=None):
    """err <= n * (atol + rtol * scale), scale = |ref|max unless given"""
    atol, rtol = _tol(dtype)
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    bound = n * (atol + rtol * (ref.abs().max().item() if scale is None else scale))
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


# ---------------------------------------------------------------------------------------------
# 1. cosine pass: training form and adjoint
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,rows,H,d", [(torch.float32, 300, 4, 32), (torch.bfloat16, 300, 4, 32),
                                            (torch.float32, 300, 4, 64), (torch.float32, 70, 32, 32)])
def test_swin_qk_norm_train_and_bwd(dtype, rows, H, d):
    """the train forward is the inference pass bit for bit (q, k and v) and its inverse norms are right;
    the adjoint against the float64 formulas on the kernel's own saved operands; the all-zero head row
    (gradient g * s / 1e-12) on its own with the rule's relative part; d logit_scale of the heads past the
    clamp exactly 0; two runs give the same bits"""
    from mmfd import kernels as K
    qkv = (R.rand(rows, 3 * H * d, seed=rows + d) * 2).to(dtype)
    qkv[5, :d] = 0  # all-zero q head: F.normalize's eps path
    ls = torch.tensor([LS[h % 4] for h in range(H)], device=DEV)
    g = R.rand(rows, 3 * H * d, seed=7).to(dtype)
    want = K.swin_qk_norm(qkv.to(DEV).clone(), H, d, ls, R.MAX_LOG)
    out, inv = K.swin_qk_norm_train(qkv.to(DEV).clone(), H, d, ls, R.MAX_LOG)
    dx, dls = K.swin_qk_norm_bwd(g.to(DEV).clone(), out, inv, H, d, ls, R.MAX_LOG)
    dx2, dls2 = K.swin_qk_norm_bwd(g.to(DEV).clone(), out, inv, H, d, ls, R.MAX_LOG)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(out[:, 2 * H * d:].cpu(), qkv[:, 2 * H * d:])
    assert torch.equal(dx, dx2) and torch.equal(dls, dls2)
    _, inv_ref = R.qk_norm_train_ref(qkv, H, d, ls.cpu())
    rel = ((inv.double().cpu() - inv_ref).abs() / inv_ref).max().item()
    print(f"inverse norms: max relative err {rel:.3e}")
    assert tuple(inv.shape) == (rows, 2, H) and rel <= 3e-5  # fp32 in both dtypes
    assert inv[5, 0, 0].item() == pytest.approx(1e12, rel=1e-6)
    ref_dx, ref_dls = R.qk_norm_bwd_ref(g, out.cpu(), inv.cpu(), H, d, ls.cpu())
    zero = torch.zeros(rows, 3 * H * d, dtype=torch.bool)
    zero[5, :d] = True
    got = dx.double().cpu()
    _close(got.masked_fill(zero, 0.0), ref_dx.masked_fill(zero, 0.0), dtype, "dqkv")
    zerr = ((got[zero] - ref_dx[zero]).abs() / ref_dx[zero].abs().clamp_min(1e-30)).max().item()
    print(f"zero row: max relative err {zerr:.3e}, |ref|max {ref_dx[zero].abs().max().item():.3e}")
    assert ref_dx[zero].abs().max().item() > 1e10 and zerr <= _tol(dtype)[1]
    assert torch.equal(dx[:, 2 * H * d:].cpu(), g[:, 2 * H * d:])  # the v third passes through
    _close(dls, ref_dls, dtype, "d_logit_scale")
    past = torch.tensor([LS[h % 4] > R.MAX_LOG for h in range(H)])
    assert past.any() and (dls.cpu()[past] == 0).all() and (dls.cpu()[~past] != 0).all()


def test_swin_qk_norm_train_refuses_head_dim_without_backward():
    """the inference pass takes d = 16; the training pair covers 32 and 64 only, and says so in the forward"""
    from mmfd import kernels as K
    qkv = torch.ones(8, 3 * 2 * 16, device=DEV)
    ls = torch.zeros(2, device=DEV)
    with pytest.raises(RuntimeError, match="head dim 16"):
        K.swin_qk_norm_train(qkv, 2, 16, ls, R.MAX_LOG)
    with pytest.raises(RuntimeError, match="head dim 16"):
        K.swin_qk_norm_bwd(qkv.clone(), qkv, torch.ones(8, 2, 2, device=DEV), 2, 16, ls, R.MAX_LOG)
    torch.cuda.synchronize()
    assert (qkv == 1).all()


# ---------------------------------------------------------------------------------------------
# 2. the gradient of a shared / modulo bias
# ---------------------------------------------------------------------------------------------
BIAS_CASES = [(3, 1, 3, 64, 64, 32), (8, 4, 2, 64, 64, 32), (6, 2, 2, 16, 16, 32), (4, 2, 2, 64, 64, 64),
              (4, 1, 2, 70, 100, 32), (2, 1, 2, 256, 256, 64)]


def _bias_inputs(B, M, H, Lq, Lk, D, dtype):
    q = R.rand(B, Lq, H * D, dtype=dtype, seed=20)
    k = R.rand(B, Lk, H * D, dtype=dtype, seed=21)
    v = R.rand(B, Lk, H * D, dtype=dtype, seed=22)
    dout = R.rand(B, Lq, H * D, dtype=dtype, seed=23)
    rb = R.rand(H, Lq, Lk, seed=24) if M == 1 else R.rand(M, H, Lq, Lk, seed=24)
    return q, k, v, dout, rb


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", BIAS_CASES)
def test_attn_bwd_bias_sum(dtype, case):
    """against float64 autograd of softmax attention with the shared ([H, Lq, Lk]) or modulo ([M, H, Lq, Lk])
    bias as a leaf — autograd does the sum over the batch rows — on the kernel's rounded inputs; dq / dk / dv
    bitwise those of the call without the extra launch; two runs give the same bits"""
    from mmfd import kernels as K
    B, M, H, Lq, Lk, D = case
    q, k, v, dout, rb = _bias_inputs(B, M, H, Lq, Lk, D, dtype)
    scale = D ** -0.5
    qd, kd, vd, dod, rbd = (t.to(DEV) for t in (q, k, v, dout, rb))
    o, lse = K.attn_fwd(qd, kd, vd, H, scale=scale, rel_bias=rbd)
    dq0, dk0, dv0 = K.attn_bwd(qd, kd, vd, o, lse, dod, H, scale=scale, rel_bias=rbd)
    delta = torch.full((B, H, Lq), float("nan"), device=DEV)
    dq, dk, dv = K.attn_bwd(qd, kd, vd, o, lse, dod, H, scale=scale, rel_bias=rbd, delta=delta)
    db = K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=rbd, scale=scale,
                             out=torch.full((M, H, Lq, Lk), float("nan"), device=DEV))
    db2 = K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=rbd, scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(dq, dq0) and torch.equal(dk, dk0) and torch.equal(dv, dv0)
    assert torch.isfinite(db).all() and torch.equal(db, db2)
    ref = A.attention_ref(q, k, v, H, scale, rel_bias=rb, dout=dout, want_d_rel_bias=True)
    ds_max = R.attn_ds_ref(q, k, v, dout, H, scale, rb).abs().max().item()  # max_b |dS_b|max
    _close(db, ref["d_rel_bias"].reshape(M, H, Lq, Lk), dtype, "d_bias", n=B // M, scale=ds_max)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attn_bwd_bias_sum_with_key_bias(dtype):
    """the entry point takes mmfd_attn_bwd's arguments, a key padding bias among them: the same check with
    ragged key masks (-FLT_MAX, mmfd_mask_to_bias) over a modulo bias; masked-key columns exactly 0"""
    from mmfd import kernels as K
    B, M, H, L, D = 4, 2, 2, 48, 32
    q, k, v, dout, rb = _bias_inputs(B, M, H, L, L, D, dtype)
    mask = (torch.arange(L)[None, :] < torch.tensor([48, 30, 30, 17])[:, None]).long()
    scale = D ** -0.5
    qd, kd, vd, dod, rbd = (t.to(DEV) for t in (q, k, v, dout, rb))
    kb = K.mask_to_bias(mask.to(DEV))
    o, lse = K.attn_fwd(qd, kd, vd, H, scale=scale, key_bias=kb, rel_bias=rbd)
    delta = torch.empty(B, H, L, device=DEV)
    K.attn_bwd(qd, kd, vd, o, lse, dod, H, scale=scale, key_bias=kb, rel_bias=rbd, delta=delta)
    db = K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=rbd, scale=scale, key_bias=kb)
    torch.cuda.synchronize()
    ref = A.attention_ref(q, k, v, H, scale, key_bias=kb.cpu(), rel_bias=rb, dout=dout, want_d_rel_bias=True)
    ds_max = R.attn_ds_ref(q, k, v, dout, H, scale, rb, key_bias=kb.cpu()).abs().max().item()
    _close(db, ref["d_rel_bias"], dtype, "d_bias (key_bias)", n=B // M, scale=ds_max)
    # bias row 1 serves batch rows 1 and 3, whose keys from 30 on are all masked
    assert (db.cpu()[1, :, :, 30:] == 0).all() and (db.cpu()[0, :, :, 30:] != 0).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attn_bwd_bias_sum_modulus_equal_to_batch(dtype):
    """M == B (Swinv2 with one image: the nW windows are the whole batch): a [B, H, L, L] tensor reads as a
    per-batch bias and is refused, the same tensor with rel_bias_mod = B named is a modulo bias with one
    term per row — the per-batch dS of the float64 reference, n = 1"""
    from mmfd import kernels as K
    B, H, L, D = 4, 2, 64, 32
    q, k, v, dout, rb = _bias_inputs(B, B, H, L, L, D, dtype)
    scale = D ** -0.5
    qd, kd, vd, dod, rbd = (t.to(DEV) for t in (q, k, v, dout, rb))
    o, lse = K.attn_fwd(qd, kd, vd, H, scale=scale, rel_bias=rbd)
    delta = torch.empty(B, H, L, device=DEV)
    K.attn_bwd(qd, kd, vd, o, lse, dod, H, scale=scale, rel_bias=rbd, delta=delta)
    with pytest.raises(RuntimeError, match="per-batch"):
        K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=rbd, scale=scale)
    db = K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=rbd, scale=scale, rel_bias_mod=B)
    torch.cuda.synchronize()
    ref = A.attention_ref(q, k, v, H, scale, rel_bias=rb, dout=dout, want_d_rel_bias=True)["d_rel_bias"]
    _close(db, ref, dtype, "d_bias (M == B)", n=1, scale=ref.abs().max().item())
    with pytest.raises(ValueError, match="rel_bias_mod"):
        K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=rbd, scale=scale, rel_bias_mod=2)


def test_attn_bwd_bias_sum_refuses_unsupported():
    """host checks, nothing launches: a per-batch bias, dropout, cosine attention, Lk = 257"""
    from mmfd import kernels as K
    B, H, L, D = 2, 2, 48, 32
    q, k, v, dout, _ = _bias_inputs(B, 1, H, L, L, D, torch.float32)
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, dout))
    shared = R.rand(H, L, L, seed=30).to(DEV)
    o, lse = K.attn_fwd(qd, kd, vd, H, rel_bias=shared)
    delta = torch.zeros(B, H, L, device=DEV)
    K.attn_bwd(qd, kd, vd, o, lse, dod, H, rel_bias=shared, delta=delta)
    out = torch.full((1, H, L, L), 7.0, device=DEV)
    per_batch = R.rand(B, H, L, L, seed=31).to(DEV)
    with pytest.raises(RuntimeError, match="per-batch"):
        K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=per_batch,
                            out=torch.full((B, H, L, L), 7.0, device=DEV))
    with pytest.raises(RuntimeError, match="dropout"):
        K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=shared, dropout_p=0.1, out=out)
    with pytest.raises(RuntimeError, match="cosine"):
        K.attn_bwd_bias_sum(qd, kd, vd, o, lse, dod, H, delta, rel_bias=shared, out=out,
                            cos_logit_scale=torch.zeros(H, device=DEV))
    Lk = 257
    k2 = torch.zeros(B, Lk, H * D, device=DEV)
    with pytest.raises(RuntimeError, match="257"):
        K.attn_bwd_bias_sum(qd, k2, k2, o, lse, dod, H, delta, rel_bias=torch.zeros(H, L, Lk, device=DEV),
                            out=torch.full((1, H, L, Lk), 7.0, device=DEV))
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---------------------------------------------------------------------------------------------
# 3. position bias: dB -> dtable -> MLP gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nW", [1, 16])
@pytest.mark.parametrize("H", [1, 4, 32])
@pytest.mark.parametrize("ws", [8, 4])
def test_swin_bias_and_cpb_bwd(ws, H, nW):
    """windows 8 (T = 225) and 4 (T = 49), with a shift mask in the forward when nW = 16: the mask is a
    constant, so the result is that of the mask-free formula (R.swin_bias_bwd_ref, proved equal to autograd
    through the masked forward on the CPU)"""
    from mmfd import kernels as K
    from mmfd.swinv2 import coords_table_and_index, shift_mask
    coords, rpi = coords_table_and_index(ws)
    L, T = ws * ws, (2 * ws - 1) ** 2
    w1, b1, w2 = R.rand(512, 2, seed=40) * 0.5, R.rand(512, seed=41) * 0.1, R.rand(H, 512, seed=42) * 0.05
    cd, rd, w1d, b1d, w2d = (t.to(DEV) for t in (coords, rpi, w1, b1, w2))
    table = K.swin_cpb(cd, w1d, b1d, w2d)
    mask = torch.from_numpy(shift_mask(4 * ws, ws, ws // 2)).to(DEV) if nW > 1 else None
    assert mask is None or mask.shape[0] == nW
    bias = K.swin_bias(table, rd, L, mask)                     # the forward this differentiates
    assert tuple(bias.shape) == (nW, H, L, L)
    d_bias = R.rand(nW, H, L, L, seed=43)
    dt = K.swin_bias_bwd(d_bias.to(DEV), table, rd, L)
    dt2 = K.swin_bias_bwd(d_bias.to(DEV), table, rd, L)
    grads = K.swin_cpb_bwd(dt, cd, w1d, b1d, w2d)
    grads2 = K.swin_cpb_bwd(dt, cd, w1d, b1d, w2d)
    torch.cuda.synchronize()
    assert tuple(dt.shape) == (T, H) and torch.equal(dt, dt2)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    _close(dt, R.swin_bias_bwd_ref(d_bias, table.cpu(), rpi), torch.float32, "d_table")
    refs = R.swin_cpb_bwd_ref(dt.cpu(), coords, w1, b1, w2)   # on the kernel's own d_table
    for got, ref, what in zip(grads, refs, ("d_w1", "d_b1", "d_w2")):
        _close(got, ref, torch.float32, what)


# ---------------------------------------------------------------------------------------------
# 4. the model
# ---------------------------------------------------------------------------------------------
def _cfg(**kw):
    from mmfd.swinv2 import Swinv2Config
    return Swinv2Config(**kw)


@pytest.fixture(scope="module")
def small():
    """swinv2_small.npz: state_dict, pixels, last_hidden_state"""
    z = np.load(R.GOLDEN + "/swinv2_small.npz")
    state = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}
    return state, torch.from_numpy(z["pixel_values"]), torch.from_numpy(z["last_hidden_state"])


def _small_model(state, precision="fp32", **kw):
    from mmfd.swinv2 import Swinv2Model
    m = Swinv2Model(_cfg(**R.SMALL, **kw))
    m.load_state_dict(state)
    return m.cuda().eval().set_precision(precision)


FIRST_LS = "encoder.layers.0.blocks.0.attention.self.logit_scale"


def test_trainable_swinv2_matches_transformers_gradients(small):
    """fp32: the output as the frozen model's bar (1e-4), every parameter's gradient within 5e-4 * max(1,
    |ref|max) of transformers', the clamped logit scale's exactly 0; pooler_output detached.
    Measured on an MI355X when this test was written: worst |delta|max / max(1, |ref|max) 1.069e-5
    (layers.2.blocks.1 logit_scale)."""
    state, px, want = small
    g = R.load_parts("swinv2_small_grads")
    m = _small_model(state, trainable=True)
    o = m(px.cuda())
    out = o.last_hidden_state
    assert out.requires_grad and not o.extra["pooler_output"].requires_grad
    assert (out.detach().cpu() - want).abs().max().item() < 1e-4
    (out * torch.from_numpy(g["R"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    fails, worst = [], (0.0, "")
    for n, p in m.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, n
        ref = torch.from_numpy(g["g." + n]).double()
        e, r = (p.grad.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
        worst = max(worst, (e / max(1.0, r), n))
        if e > 5e-4 * max(1.0, r):
            fails.append(f"{n}: {e:.3e} > {5e-4 * max(1.0, r):.3e} (|ref|max {r:.3e})")
    print(f"fp32 Swinv2: worst gradient error {worst[0]:.3e} ({worst[1]})")
    assert not fails, "; ".join(fails[:8])
    assert (m.get_parameter(FIRST_LS).grad == 0).all()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_single_image_forward_and_backward(small, precision):
    """one image: in the shifted blocks the attention batch is the nW windows, so the modulo bias has as many
    rows as the batch. Reference: the same image twice (B = 2, R stacked twice) — its gradients are exactly
    twice the B = 1 ones in exact arithmetic (and the fp32 output of the single image is held to row 0 of the
    transformers fixture, 1e-4: that output does not depend on the rest of the batch). Both runs launch the
    same kernels on each image's rows and no activation kernel mixes batch rows, so the per-image terms are the same numbers in both dtypes and only the
    fp32 accumulation of the parameter gradients over twice the rows differs: the fp32 model bar 5e-4 * max(1,
    |ref|max) in both dtypes. Measured on an MI355X when this test was written: 4.4e-7 (fp32), 4.5e-7 (bf16)."""
    state, px, want = small
    x1 = px[:1].cuda()
    R1 = R.rand(1, 64, 128, seed=23).cuda()
    grads = []
    outs = []
    for x, Rr in ((x1, R1), (x1.repeat(2, 1, 1, 1), R1.repeat(2, 1, 1))):
        m = _small_model(state if precision == "fp32" else R.bf16_round_state(state), precision, trainable=True)
        out = m(x).last_hidden_state
        (out.float() * Rr).sum().backward()
        torch.cuda.synchronize()
        outs.append(out.detach())
        grads.append({n: p.grad.double().cpu() for n, p in m.named_parameters()})
    if precision == "fp32":
        assert (outs[0][0].cpu() - want[0]).abs().max().item() < 1e-4
    rel_bar = 5e-4
    worst, fails = (0.0, ""), []
    for n, g1 in grads[0].items():
        ref = grads[1][n] / 2
        assert torch.isfinite(g1).all(), n
        rel = (g1 - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        worst = max(worst, (rel, n))
        if rel > rel_bar:
            fails.append(f"{n}: {rel:.3e}")
    print(f"{precision} single image vs the image twice: worst relative error {worst[0]:.3e} ({worst[1]}), bar {rel_bar:.3e}")
    assert not fails, (rel_bar, fails[:8])
    assert (grads[0][FIRST_LS] == 0).all()


def test_trainable_swinv2_bf16_gradients(small):
    """bf16 on bf16-rounded master weights and pixels (the shadow cast is exact) against the fixture's gb.*:
    per tensor |delta|max / max(1, |ref|max) <= 2 * emul_worst_rel and cosine >= 1 - 2 * (1 - emul_min_cos).
    Measured on an MI355X when this test was written: bars 1.851e-1 and 0.99355; worst relative error
    1.689e-1 (layers.2.blocks.1 query.weight), lowest cosine 0.99400 (layers.2.blocks.1 query.bias)."""
    state, px, _ = small
    gb = R.load_parts("swinv2_small_grads_bf16")
    g = R.load_parts("swinv2_small_grads")
    rel_bar = 2.0 * float(gb["emul_worst_rel"])
    cos_bar = 1.0 - 2.0 * (1.0 - float(gb["emul_min_cos"]))
    m = _small_model(R.bf16_round_state(state), "bf16", trainable=True)
    out = m(px.to(torch.bfloat16).float().cuda()).last_hidden_state
    assert out.dtype == torch.bfloat16
    (out.float() * torch.from_numpy(g["R"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    fails, worst_rel, worst_cos = [], (0.0, ""), (1.0, "")
    for n, p in m.named_parameters():
        ref = torch.from_numpy(gb["gb." + n].astype(np.float64)).reshape(-1)
        got = p.grad.double().cpu().reshape(-1)
        assert torch.isfinite(got).all(), n
        rel = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        worst_rel = max(worst_rel, (rel, n))
        if ref.abs().max().item() == 0.0:  # the clamped logit scale: exactly 0, no direction to compare
            assert (got == 0).all(), n
            cos = 1.0
        else:
            cos = (got @ ref / (got.norm() * ref.norm())).item()
        worst_cos = min(worst_cos, (cos, n))
        if rel > rel_bar or cos < cos_bar:
            fails.append(f"{n}: rel {rel:.3e} cos {cos:.5f}")
    print(f"bf16 Swinv2: worst relative error {worst_rel[0]:.3e} ({worst_rel[1]}), bar {rel_bar:.3e}; "
          f"lowest cosine {worst_cos[0]:.5f} ({worst_cos[1]}), bar {cos_bar:.5f}")
    assert not fails, (rel_bar, cos_bar, fails[:8])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainable_eval_forward_is_bit_identical(small, precision):
    """under no_grad a trainable model launches the frozen model's kernels: equal bits; under grad (eval
    mode) it returns a differentiable output (the training form's values are checked against transformers
    in test_trainable_swinv2_matches_transformers_gradients)"""
    state, px, _ = small
    a = _small_model(state, precision)
    b = _small_model(state, precision, trainable=True)
    with torch.no_grad():
        oa, ob = a(px.cuda()), b(px.cuda())
    og = b(px.cuda()).last_hidden_state
    torch.cuda.synchronize()
    assert torch.equal(oa.last_hidden_state, ob.last_hidden_state)
    assert torch.equal(oa.extra["pooler_output"], ob.extra["pooler_output"])
    assert og.requires_grad and not ob.last_hidden_state.requires_grad


def test_default_and_drop_path_raise(small):
    from mmfd.swinv2 import Swinv2Model
    state, px, _ = small
    x = px[:1].cuda()
    with pytest.raises(NotImplementedError, match="inference-only"):
        Swinv2Model(_cfg(**R.SMALL)).cuda()(x)
    m = Swinv2Model(_cfg(**R.SMALL, trainable=True, drop_path_rate=0.1)).cuda().train()
    with pytest.raises(NotImplementedError, match="stochastic depth"):
        m(x)
    out = m.eval()(x).last_hidden_state  # eval: stochastic depth is off anyway
    assert tuple(out.shape) == (1, 64, 128) and out.requires_grad
    assert tuple(Swinv2Model(_cfg(**R.SMALL, trainable=True)).cuda().train()(x).last_hidden_state.shape) == (1, 64, 128)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_backward_is_deterministic(small, precision):
    state, px, _ = small
    m = _small_model(state, precision, trainable=True)
    Rr = R.rand(2, 64, 128, seed=23).cuda()
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        (m(px.cuda()).last_hidden_state.float() * Rr).sum().backward()
        torch.cuda.synchronize()
        runs.append({n: p.grad.clone() for n, p in m.named_parameters()})
    bad = [n for n in runs[0] if not torch.equal(runs[0][n], runs[1][n])]
    assert not bad, bad[:8]


# ---------------------------------------------------------------------------------------------
# 5. trainer
# ---------------------------------------------------------------------------------------------
TRAIN_SWIN = dict(image_size=64, embed_dim=32, depths=(2, 2), num_heads=(1, 2), pretrained_window_sizes=(0, 0))


def _swin_trainer(precision):
    """the smallest trainer of test_trainer_gpu.py with a small trainable Swinv2 as image encoder: image 64 ->
    a 16x16 grid in four (shifted) windows, then one 8x8 window of width 64 = the head's image_input_dim"""
    from mmfd.swinv2 import Swinv2Model
    from mmfd.train import FusionTrainer
    from tests.smoke_impl import TINY, build_modules
    text, _, head, _ = build_modules(dropout=0.0, cfg=TINY, seed=5)
    torch.manual_seed(6)
    image = Swinv2Model(_cfg(**TRAIN_SWIN, trainable=True))
    dev = torch.device("cuda", 0)
    text, image, head = text.to(dev), image.to(dev), head.to(dev)
    return FusionTrainer(text, image, head, lr=1e-3, precision=precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainer_trains_swinv2_eager_and_captured(precision):
    """three captured replays after the capture's two warm-up steps against five eager steps from the same
    start: the losses and every parameter agree to 1e-5 (fp32) / 1e-3 (bf16) relative to max(1, |a|max); the
    first step moves the image encoder (logit scale and position-bias MLP included)"""
    from tests.smoke_impl import TINY, tiny_batch
    cfg = dict(TINY, img=64)
    tr_e, tr_g = _swin_trainer(precision), _swin_trainer(precision)
    assert not tr_e.freeze_image and any(p is q for p in tr_e.params for q in tr_e.image_encoder.parameters())
    b1 = {k: v.cuda() for k, v in tiny_batch(3, cfg=cfg, seed=41).items()}
    b2 = {k: v.cuda() for k, v in tiny_batch(3, cfg=cfg, seed=42).items()}
    ie = tr_e.image_encoder
    before = {n: p.detach().clone() for n, p in ie.named_parameters()}
    le = [tr_e.step(b1)]
    torch.cuda.synchronize()
    s = "encoder.layers.0.blocks.1.attention.self."
    for n in (s + "logit_scale", s + "continuous_position_bias_mlp.0.weight", s + "key.weight",
              "encoder.layers.0.downsample.reduction.weight", "embeddings.patch_embeddings.projection.weight"):
        assert not torch.equal(before[n], ie.get_parameter(n).detach()), n
    static = {k: v.clone() for k, v in b1.items()}
    tr_g.capture(static, warmup=2)
    le += [tr_e.step(b1)]
    le += [tr_e.step(b1), tr_e.step(b2), tr_e.step(b1)]
    lg = [tr_g.replay().clone(), tr_g.replay(b2).clone(), tr_g.replay(b1).clone()]
    torch.cuda.synchronize()
    tol = 1e-5 if precision == "fp32" else 1e-3
    for a, b in zip(le[2:], lg):
        assert torch.isfinite(a).all()
        assert (a.detach() - b).abs().max().item() <= tol * max(1.0, a.abs().max().item()), (a, b)
    for me, mg in ((tr_e.image_encoder, tr_g.image_encoder), (tr_e.text_encoder, tr_g.text_encoder),
                   (tr_e.head, tr_g.head)):
        for (n, a), (_, b) in zip(me.named_parameters(), mg.named_parameters()):
            assert (a.detach() - b.detach()).abs().max().item() <= tol * max(1.0, a.abs().max().item()), n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_base_shape_training_step(precision):
    """one eager training step's forward and backward of the default swinv2-base shape at B = 2 (heads up to
    32, 64 windows per image): output (2, 64, 1024), every parameter receives a finite gradient that is
    non-zero somewhere"""
    from mmfd.swinv2 import Swinv2Model
    torch.manual_seed(5)
    m = Swinv2Model(_cfg(trainable=True)).cuda().train().set_precision(precision)
    px = R.rand(2, 3, 256, 256, seed=6).cuda()
    out = m(px).last_hidden_state
    assert tuple(out.shape) == (2, 64, 1024)
    (out.float() * R.rand(2, 64, 1024, seed=7).cuda()).sum().backward()
    torch.cuda.synchronize()
    bad = [n for n, p in m.named_parameters()
           if p.grad is None or not torch.isfinite(p.grad).all() or not (p.grad != 0).any()]
    assert not bad, bad[:8]
