"""Trainable DeBERTa-v3 encoder on the HIP path: the three new kernels against float64 references, the
model's gradients against transformers (tests/golden/deberta_small_grads.npz) and the CPU oracle, the
opt-in semantics and the trainer.

Tolerances. Kernels: test_kernels_gpu.py's rule err <= atol + rtol * |ref|max with (3e-5, 3e-5) in
fp32 and (2e-2, 2e-2) in bf16. Model, fp32: output 1e-4 abs vs transformers (1e-3 vs the oracle at
xsmall width, test_deberta_gpu.py's bars), every parameter gradient 5e-4 * max(1, |ref|max)
(test_encoders_gpu.py), and the position tensors (rel_embeddings, encoder.LayerNorm) additionally
5e-4 * |ref|max without the floor. Model, bf16: output 0.25 max / 1e-2 mean abs; gradients twice the
worst |delta|max / max(1, |ref|max) that the bf16 BertModel shows on bert_small.npz in the same
session (each DeBERTa score adds two more bf16-rounded products, c2p and p2c)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POS_TENSORS = ("encoder.rel_embeddings.weight", "encoder.LayerNorm.weight", "encoder.LayerNorm.bias")


def _tol(dtype):
    return (3e-5, 3e-5) if dtype == torch.float32 else (2e-2, 2e-2)


def _close(got, ref, dtype, what=""):
    rtol, atol = _tol(dtype)
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = (got - ref).abs().max().item()
    bound = atol + rtol * ref.abs().max().item()
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _rand(*shape, dtype=torch.float32, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


# ---------------------------------------------------------------------------------------------
# 1. attention backward with d_rel_bias
# ---------------------------------------------------------------------------------------------
DS_CASES = [(2, 2, 80, 32, True), (2, 2, 45, 32, False), (1, 6, 160, 64, False), (1, 2, 300, 64, True)]


def _attn_inputs(B, H, L, D, masked, dtype):
    from mmfd import kernels as K
    q = _rand(B, L, H * D, dtype=dtype, seed=20)
    kv = _rand(B, L, 2 * H * D, dtype=dtype, seed=21)
    dout = _rand(B, L, H * D, dtype=dtype, seed=22)
    rb = _rand(B, H, L, L, seed=23)
    mask = kb = None
    if masked:
        lens = torch.randint(1, L + 1, (B,), generator=torch.Generator().manual_seed(3))
        mask = (torch.arange(L)[None, :] < lens[:, None]).long()
        kb = K.mask_to_bias(mask.to(DEV))
    return q, kv, dout, rb, mask, kb


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", DS_CASES)
def test_attn_bwd_d_rel_bias(dtype, case):
    """dS, dq, dk, dv against float64 autograd of softmax attention with the bias as a leaf, on the
    kernel's rounded inputs (L <= 256: resident backward kernels, L = 300: streaming ones; 45 and 300
    are no multiples of 16 or 4); masked-key columns exactly 0; dq / dk / dv bitwise those of the call
    without d_rel_bias"""
    from mmfd import kernels as K
    B, H, L, D, masked = case
    q, kv, dout, rb, mask, kb = _attn_inputs(B, H, L, D, masked, dtype)
    k, v = kv[..., : H * D], kv[..., H * D:]
    scale = 1.0 / math.sqrt(3 * D)
    qd, kvd, dod, rbd = q.to(DEV), kv.to(DEV), dout.to(DEV), rb.to(DEV)
    kd, vd = kvd[..., : H * D], kvd[..., H * D:]
    o, lse = K.attn_fwd(qd, kd, vd, H, scale=scale, key_bias=kb, rel_bias=rbd)
    ds = torch.full((B, H, L, L), float("nan"), device=DEV)
    dq, dk, dv = K.attn_bwd(qd, kd, vd, o, lse, dod, H, scale=scale, key_bias=kb, rel_bias=rbd, d_rel_bias=ds)
    dq0, dk0, dv0 = K.attn_bwd(qd, kd, vd, o, lse, dod, H, scale=scale, key_bias=kb, rel_bias=rbd)
    torch.cuda.synchronize()
    heads = lambda t: t.double().view(B, L, H, D).transpose(1, 2)  # noqa: E731
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    rr = rb.double().requires_grad_(True)
    s = heads(qr) @ heads(kr).transpose(-1, -2) * scale + rr
    if masked:
        s = s + kb.double().cpu()[:, None, None, :]
    oref = (torch.softmax(s, -1) @ heads(vr)).transpose(1, 2).reshape(B, L, H * D)
    oref.backward(dout.double())
    _close(o, oref, dtype, "o")
    _close(ds, rr.grad, dtype, "d_rel_bias")
    _close(dq, qr.grad, dtype, "dq")
    _close(dk, kr.grad, dtype, "dk")
    _close(dv, vr.grad, dtype, "dv")
    assert torch.isfinite(ds).all()
    if masked:
        dead = (mask == 0)[:, None, None, :].expand(B, H, L, L)
        assert dead.any() and (ds.cpu()[dead] == 0).all()
    assert torch.equal(dq, dq0) and torch.equal(dk, dk0) and torch.equal(dv, dv0)


def test_attn_bwd_d_rel_bias_refuses_unsupported():
    from mmfd import kernels as K
    B, H, L, D = 2, 2, 48, 32
    q, kv, dout, rb, _, _ = _attn_inputs(B, H, L, D, False, torch.float32)
    qd, kvd, dod = q.to(DEV), kv.to(DEV), dout.to(DEV)
    kd, vd = kvd[..., : H * D], kvd[..., H * D:]
    ds = torch.zeros(B, H, L, L, device=DEV)
    shared = rb[0].contiguous().to(DEV)  # [H, L, L]: one bias for the whole batch
    o, lse = K.attn_fwd(qd, kd, vd, H, rel_bias=shared)
    with pytest.raises(RuntimeError, match="d_rel_bias"):
        K.attn_bwd(qd, kd, vd, o, lse, dod, H, rel_bias=shared, d_rel_bias=ds)
    rbd = rb.to(DEV)
    seed = K.Seed(5)
    o, lse = K.attn_fwd(qd, kd, vd, H, rel_bias=rbd, dropout_p=0.1, seed=seed, salt=1)
    with pytest.raises(RuntimeError, match="d_rel_bias"):
        K.attn_bwd(qd, kd, vd, o, lse, dod, H, rel_bias=rbd, dropout_p=0.1, seed=seed, salt=1, d_rel_bias=ds)
    with pytest.raises(RuntimeError, match="alias"):
        K.attn_bwd(qd, kd, vd, o, lse, dod, H, rel_bias=rbd, d_rel_bias=rbd)
    torch.cuda.synchronize()
    assert (ds == 0).all()


# ---------------------------------------------------------------------------------------------
# 2. deberta_rel_bias_bwd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 2, 80, 32), (1, 3, 300, 256), (1, 2, 512, 256)])
def test_deberta_rel_bias_bwd(case):
    """against a float64 scatter-add over the same indices. fp32: err <= 2e-5 * inv_scale * max|ds| (a run
    has at most 16 fp32 terms: 16 * 2^-24 relative on a sum of at most 16 max|ds|); bf16 adds 2^-8 *
    |ref|max for the one output rounding. Unreached columns exactly 0, the adjoint identity with the
    forward kernel to 1e-5 relative, and two runs bitwise equal."""
    from mmfd import kernels as K
    from mmfd.deberta import _bias_indices
    B, H, L, S = case
    inv = 0.125
    ci, pi = _bias_indices(L, S, 512, torch.device(DEV, 0))
    ds = _rand(B, H, L, L, seed=31)
    dsd = ds.to(DEV)
    cl, pl = ci.cpu().long(), pi.cpu().long()
    ref_c = torch.zeros(B, H, L, 2 * S, dtype=torch.float64).scatter_add_(-1, cl.expand(B, H, L, L), ds.double())
    ref_p = torch.zeros(B, H, L, 2 * S, dtype=torch.float64).scatter_add_(-1, pl.expand(B, H, L, L),
                                                                         ds.double().transpose(-1, -2))
    cnt_c = torch.zeros(L, 2 * S).scatter_add_(-1, cl, torch.ones(L, L))
    cnt_p = torch.zeros(L, 2 * S).scatter_add_(-1, pl, torch.ones(L, L))
    assert cnt_c.max().item() <= 16 and cnt_p.max().item() <= 16  # the run length behind the fp32 bound
    lay = lambda t: (t * inv).permute(1, 0, 2, 3).reshape(H, B * L, 2 * S)  # noqa: E731
    ref_c, ref_p = lay(ref_c), lay(ref_p)
    dmax = ds.abs().max().item()
    for dtype in (torch.float32, torch.bfloat16):
        dc, dp = K.deberta_rel_bias_bwd(dsd, ci, pi, B, L, inv, 2 * S, dtype)
        dc2, dp2 = K.deberta_rel_bias_bwd(dsd, ci, pi, B, L, inv, 2 * S, dtype)
        torch.cuda.synchronize()
        assert dc.dtype == dtype and tuple(dc.shape) == (H, B * L, 2 * S)
        assert torch.equal(dc, dc2) and torch.equal(dp, dp2)
        for got, ref, cnt, what in ((dc, ref_c, cnt_c, "dc2p"), (dp, ref_p, cnt_p, "dp2c")):
            err = (got.double().cpu() - ref).abs().max().item()
            bound = 2e-5 * inv * dmax + (2.0 ** -8 * ref.abs().max().item() if dtype == torch.bfloat16 else 0.0)
            print(f"{what} {dtype}: err {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (what, dtype, err, bound)
            empty = (cnt == 0)[None, :, :].expand(H, L, 2 * S).repeat(1, B, 1)
            assert empty.any() and (got.cpu()[empty] == 0).all()
        if dtype == torch.float32:  # <deberta_rel_bias(c2p, p2c), ds> = <c2p, dc2p> + <p2c, dp2c>
            c2p, p2c = _rand(H, B * L, 2 * S, seed=32).to(DEV), _rand(H, B * L, 2 * S, seed=33).to(DEV)
            out = K.deberta_rel_bias(c2p, p2c, ci, pi, B, L, inv)
            torch.cuda.synchronize()
            lhs = (out.double() * dsd.double()).sum().item()
            rhs = (c2p.double() * dc.double()).sum().item() + (p2c.double() * dp.double()).sum().item()
            print(f"adjoint: {lhs:.9e} vs {rhs:.9e}")
            assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_deberta_rel_bias_bwd_refuses_unsorted_indices():
    from mmfd import kernels as K
    from mmfd.deberta import _bias_indices
    L, S = 80, 32
    ci, pi = _bias_indices(L, S, 512, torch.device(DEV, 0))
    bad = ci.clone()
    bad[5] = ci[5].flip(0)
    with pytest.raises(ValueError, match="monotone"):
        K.deberta_rel_bias_bwd(torch.zeros(1, 1, L, L, device=DEV), bad, pi, 1, L, 0.125, 2 * S, torch.float32)


# ---------------------------------------------------------------------------------------------
# 3. attn_fill_masked_rows_bwd
# ---------------------------------------------------------------------------------------------
def test_attn_fill_masked_rows_bwd():
    """against float64 autograd of o[b, i] = mask[b, i] ? o_attn[b, i] : mean_j v[b, j]; err < 1e-5 (the
    forward test's bar). dv is a strided view of a packed buffer that already holds a gradient."""
    from mmfd import kernels as K
    B, H, L, Dh = 2, 2, 40, 32
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, 25:] = 0
    do = _rand(B, L, H * Dh, seed=41)
    packed = _rand(B, L, 3 * H * Dh, seed=42)
    oa = _rand(B, L, H * Dh, seed=43).double().requires_grad_(True)
    v = _rand(B, L, H * Dh, seed=44).double().requires_grad_(True)
    o = torch.where(mask[:, :, None].bool(), oa, v.mean(1, keepdim=True).expand(B, L, H * Dh))
    o.backward(do.double())
    dod, pd = do.clone().to(DEV), packed.clone().to(DEV)
    gsum = K.attn_fill_masked_rows_bwd(dod, H, mask.to(DEV))
    dv = pd[..., 2 * H * Dh:]
    K.attn_fill_masked_rows_bwd(dod, H, mask.to(DEV), dv=dv, gsum=gsum)
    torch.cuda.synchronize()
    assert (dod.double().cpu() - oa.grad).abs().max().item() < 1e-5
    assert (dod.cpu()[1, 25:] == 0).all() and torch.equal(dod.cpu()[0], do[0])
    assert (dv.double().cpu() - packed[..., 2 * H * Dh:].double() - v.grad).abs().max().item() < 1e-5
    assert torch.equal(pd.cpu()[..., : 2 * H * Dh], packed[..., : 2 * H * Dh])


# ---------------------------------------------------------------------------------------------
# 4 / 5. the model
# ---------------------------------------------------------------------------------------------
def _small_cfg(**kw):
    from mmfd.deberta import DebertaV2Config
    c = dict(vocab_size=1000, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128)
    c.update(kw)
    return DebertaV2Config(**c)


def _grad_errors(m, ref_grads):
    """{name: (|delta|max, |ref|max)}"""
    out = {}
    for n, p in m.named_parameters():
        assert p.grad is not None, f"missing grad {n}"
        ref = ref_grads[n].double()
        out[n] = ((p.grad.double().cpu() - ref).abs().max().item(), ref.abs().max().item())
    return out


def _check_fp32_grads(errs):
    fails = []
    for n, (e, r) in errs.items():
        bound = 5e-4 * (r if n in POS_TENSORS else max(1.0, r))
        if n in POS_TENSORS:
            print(f"{n}: |delta|max {e:.3e}, |ref|max {r:.3e}, relative {e / r:.3e}")
        if e > bound:
            fails.append(f"{n}: {e:.3e} > {bound:.3e} (|ref|max {r:.3e})")
    assert not fails, "; ".join(fails)


def test_trainable_deberta_matches_transformers_gradients():
    from mmfd.deberta import DebertaV2Model
    z = np.load(os.path.join(G, "deberta_small.npz"))
    gz = np.load(os.path.join(G, "deberta_small_grads.npz"))
    m = DebertaV2Model(_small_cfg(trainable=True))
    m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")})
    m = m.cuda().eval()
    out = m(input_ids=torch.from_numpy(z["input_ids"]).cuda(),
            attention_mask=torch.from_numpy(z["attention_mask"]).cuda()).last_hidden_state
    assert out.requires_grad
    err = (out.detach().cpu() - torch.from_numpy(z["last_hidden_state"])).abs().max().item()
    assert err < 1e-4, err
    (out * torch.from_numpy(gz["R"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    _check_fp32_grads(_grad_errors(m, {k[2:]: torch.from_numpy(gz[k]) for k in gz.files if k.startswith("g.")}))
    # padded query rows (row 1 from token 171) reach value_proj through the mean of V only
    assert m.embeddings.word_embeddings.weight.grad[0].abs().max().item() == 0.0


def _oracle_grads(m, ids, mask, R):
    from oracle.deberta import deberta_forward
    P = {k: v.detach().float().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    out = deberta_forward(P, ids, mask, num_layers=m.config.num_hidden_layers,
                          num_heads=m.config.num_attention_heads, eps=m.config.layer_norm_eps)
    (out * R).sum().backward()
    return out.detach(), {k: v.grad for k, v in P.items()}


def _xsmall(layers, L, precision):
    from mmfd.deberta import DebertaV2Config, DebertaV2Model
    torch.manual_seed(3)
    m = DebertaV2Model(DebertaV2Config(vocab_size=2000, num_hidden_layers=layers, trainable=True))
    with torch.no_grad():
        for q in m.parameters():  # LayerNorm / bias parameters off their trivial init
            q.add_(torch.randn_like(q) * 0.02)
        m.embeddings.word_embeddings.weight[0].zero_()
    m = m.cuda().eval().set_precision(precision)
    g = torch.Generator().manual_seed(L)
    B = 2
    ids = torch.randint(1, 2000, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, L // 2:] = 0
    ids[1, L // 2:] = 0
    R = torch.randn(B, L, 384, generator=g)
    return m, ids, mask, R


@pytest.mark.parametrize("layers,L", [(2, 160), (1, 320)])
def test_trainable_deberta_xsmall_fp32_vs_oracle(layers, L):
    """xsmall width (hidden 384, 6 heads, d = 64, 256 buckets), row 1 padded from L / 2; L = 160 runs the
    resident attention kernels, L = 320 the streaming ones"""
    m, ids, mask, R = _xsmall(layers, L, "fp32")
    out = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    (out * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    ref, grads = _oracle_grads(m, ids, mask, R)
    assert (out.detach().cpu() - ref).abs().max().item() < 1e-3
    _check_fp32_grads(_grad_errors(m, grads))


@pytest.fixture(scope="module")
def bert_bf16_grad_error():
    """worst |delta|max / max(1, |ref|max) of the bf16 BertModel's parameter gradients against
    transformers' fp32 ones (tests/golden/bert_small.npz): existing code, the yardstick for bf16"""
    import json
    from mmfd.encoders import BertConfig, BertModel
    z = np.load(os.path.join(G, "bert_small.npz"), allow_pickle=False)
    m = BertModel(BertConfig(**json.loads(str(z["config"]))))
    m.load_state_dict({k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")})
    m = m.to(DEV).eval().set_precision("bf16")
    out = m(input_ids=torch.from_numpy(z["input_ids"]).to(DEV), attention_mask=torch.from_numpy(z["attention_mask"]).to(DEV),
            token_type_ids=torch.from_numpy(z["token_type_ids"]).to(DEV)).last_hidden_state
    (out.float() * torch.from_numpy(z["R"]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    worst = 0.0
    for n, p in m.named_parameters():
        ref = torch.from_numpy(z["grad/" + n]).double()
        worst = max(worst, (p.grad.double().cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item()))
    print(f"bf16 BertModel on bert_small.npz: worst gradient error {worst:.3e}")
    return worst


def test_trainable_deberta_xsmall_bf16_vs_oracle(bert_bf16_grad_error):
    """bf16 at xsmall width, 2 layers, L = 160: output 0.25 max / 1e-2 mean abs; every gradient within
    2 x the bf16 BertModel's own worst error on bert_small.npz, measured in the same session by the
    fixture above. Measured on an MI355X when this test was written: bf16 BertModel 9.851e-3, hence a
    bar of 1.970e-2; the bf16 DeBERTa's worst gradient error 1.023e-2 (layer 1 key_proj.weight)."""
    m, ids, mask, R = _xsmall(2, 160, "bf16")
    out = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    (out.float() * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    ref, grads = _oracle_grads(m, ids, mask, R)
    diff = (out.detach().float().cpu() - ref).abs()
    assert diff.max().item() < 0.25 and diff.mean().item() < 1e-2, (diff.max().item(), diff.mean().item())
    bar = 2.0 * bert_bf16_grad_error
    errs = _grad_errors(m, grads)
    worst = max(errs.items(), key=lambda kv: kv[1][0] / max(1.0, kv[1][1]))
    print(f"bf16 DeBERTa: worst gradient error {worst[1][0] / max(1.0, worst[1][1]):.3e} ({worst[0]}), bar {bar:.3e}")
    fails = [f"{n}: {e / max(1.0, r):.3e}" for n, (e, r) in errs.items() if e / max(1.0, r) > bar]
    assert not fails, (bar, fails[:8])


# ---------------------------------------------------------------------------------------------
# 6. opt-in semantics
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainable_eval_forward_is_bit_identical(precision):
    from mmfd.deberta import DebertaV2Model
    torch.manual_seed(11)
    a = DebertaV2Model(_small_cfg()).cuda().eval().set_precision(precision)
    b = DebertaV2Model(_small_cfg(trainable=True))
    b.load_state_dict(a.state_dict())
    b = b.cuda().eval().set_precision(precision)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 1000, (2, 70), generator=g).cuda()
    mask = torch.ones(2, 70, dtype=torch.long)
    mask[0, 40:] = 0
    with torch.no_grad():
        oa = a(input_ids=ids, attention_mask=mask.cuda()).last_hidden_state
        ob = b(input_ids=ids, attention_mask=mask.cuda()).last_hidden_state
    og = b(input_ids=ids, attention_mask=mask.cuda()).last_hidden_state  # under grad: the same kernels
    torch.cuda.synchronize()
    assert torch.equal(oa, ob)
    assert og.requires_grad and not ob.requires_grad
    assert (oa.float() - og.detach().float()).abs().max().item() <= (1e-5 if precision == "fp32" else 5e-2)


def test_trainable_dropout_and_frozen_default_raise():
    from mmfd.deberta import DebertaV2Model
    ids = torch.ones(1, 8, dtype=torch.long, device=DEV)
    for kw in (dict(hidden_dropout_prob=0.1), dict(attention_probs_dropout_prob=0.1)):
        m = DebertaV2Model(_small_cfg(trainable=True, **kw)).cuda().train()
        with pytest.raises(NotImplementedError, match="dropout"):
            m(input_ids=ids)
        assert m.eval()(input_ids=ids).last_hidden_state.shape == (1, 8, 64)  # eval: dropout is off anyway
    with pytest.raises(NotImplementedError, match="inference-only"):
        DebertaV2Model(_small_cfg()).cuda()(input_ids=ids)


# ---------------------------------------------------------------------------------------------
# 7. trainer
# ---------------------------------------------------------------------------------------------
def _deberta_trainer(precision):
    from mmfd.deberta import DebertaV2Model
    from mmfd.train import FusionTrainer
    from tests.smoke_impl import TINY, build_modules
    _, image, head, _ = build_modules(dropout=0.1, cfg=TINY, seed=5)
    torch.manual_seed(6)
    text = DebertaV2Model(_small_cfg(trainable=True))
    dev = torch.device("cuda", 0)
    text, image, head = text.to(dev), image.to(dev), head.to(dev)
    head.manual_seed(99)
    return FusionTrainer(text, image, head, lr=1e-3, precision=precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainer_trains_deberta_eager_and_captured(precision):
    """the smallest trainer of test_trainer_gpu.py with the small trainable DeBERTa as text encoder
    (head text_input_dim = 64): three captured replays match three eager steps from the same start
    (after the capture's two warm-up steps, as test_captured_step_replays_equal_eager_steps; losses
    to 1e-5 fp32 / 1e-3 bf16), and the first step moves exactly the parameters it should."""
    from tests.smoke_impl import tiny_batch
    tr_e, tr_g = _deberta_trainer(precision), _deberta_trainer(precision)
    assert not tr_e.freeze_text and any(p is q for p in tr_e.params for q in tr_e.text_encoder.parameters())
    b1 = {k: v.cuda() for k, v in tiny_batch(3, seed=41).items()}
    b2 = {k: v.cuda() for k, v in tiny_batch(3, seed=42).items()}
    te = tr_e.text_encoder
    before = {n: p.detach().clone() for n, p in te.named_parameters()}
    le = [tr_e.step(b1)]
    torch.cuda.synchronize()
    after = {n: p.detach().clone() for n, p in te.named_parameters()}
    for n in ("encoder.rel_embeddings.weight", "encoder.layer.0.attention.self.query_proj.weight"):
        assert not torch.equal(before[n], after[n]), n
    used = torch.unique(b1["input_ids"][b1["attention_mask"] > 0])
    assert 0 not in used.tolist()
    wb, wa = before["embeddings.word_embeddings.weight"], after["embeddings.word_embeddings.weight"]
    assert ((wb[used] != wa[used]).any(dim=1)).all()
    unused = torch.ones(wb.shape[0], dtype=torch.bool, device=wb.device)
    unused[used] = False  # (row pad_token_id = 0 stays in: the padded positions carry id 0)
    lr, wd = tr_e.optimizer.param_groups[0]["lr"], tr_e.optimizer.param_groups[0]["weight_decay"]
    assert ((wa[unused] - wb[unused]).abs() <= 1.01 * lr * wd * wb[unused].abs() + 1e-9).all()
    assert torch.equal(wa[0], wb[0])
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
    outs = tr_g.predict(b2)
    assert all(torch.isfinite(y).all() for pair in outs for y in pair if y is not None)
