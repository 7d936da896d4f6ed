"""The references of tests/memory_kernel_refs.py against independent formulations (torch's own
operators, closed forms, the oracle's dropout hash): proves, without a GPU, what
tests/test_memory_kernels_gpu.py compares the HIP kernels with."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.dropout_hash import dropout_hash, keep_mask
from tests import memory_kernel_refs as R

_rand = R.rand


def _ids(B, L, vocab, seed):
    return torch.randint(0, vocab, (B, L), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("shape,P", [((2, 3, 8, 12), 4), ((2, 3, 9, 12), 3), ((2, 3, 4, 6), 2), ((1, 3, 32, 48), 16)])
def test_patchify_ref_is_unfold(shape, P):
    px = _rand(*shape, seed=1)
    ref = R.patchify_ref(px, P)
    unf = F.unfold(px, kernel_size=P, stride=P)  # [B, C*P*P, np], columns (c, kh, kw), patches row-major
    assert torch.equal(ref, unf.transpose(1, 2).reshape(-1, shape[1] * P * P))


@pytest.mark.parametrize("with_type", [False, True])
@pytest.mark.parametrize("explicit_pos", [False, True])
def test_embed_ref_is_embedding_plus_layer_norm(with_type, explicit_pos):
    B, L, D = 3, 7, 40
    ids = _ids(B, L, 11, 2)
    tts = _ids(B, L, 2, 3) if with_type else None
    pos_ids = _ids(B, L, L + 2, 4) if explicit_pos else None
    word, pos = _rand(11, D, seed=5).double(), _rand(L + 2, D, seed=6).double()
    typ = _rand(2, D, seed=7).double() if with_type else None
    gamma, beta = 1 + 0.1 * _rand(D, seed=8).double(), _rand(D, seed=9).double()
    s = R.embed_sum_ref(ids, pos_ids, tts, word, pos, typ)
    want = F.embedding(ids, word) + F.embedding(pos_ids if explicit_pos else torch.arange(L).expand(B, L), pos)
    if with_type:
        want = want + F.embedding(tts, typ)
    assert torch.equal(s, want.reshape(B * L, D))
    y, mean, rstd = R.layernorm_ref(s, gamma, beta, 1e-5)
    assert torch.allclose(y, F.layer_norm(s, (D,), gamma, beta, 1e-5), rtol=0, atol=1e-12)
    assert torch.allclose(mean, s.mean(-1), rtol=0, atol=1e-14)
    assert torch.allclose(rstd, (s.var(-1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("pad", [0, 1])
def test_position_ids_ref_is_masked_cumsum(pad):
    ids = _ids(33, 9, 4, 10 + pad)
    ids[0] = pad      # all padding
    ids[1] = pad + 1  # none
    ids[2, 0] = pad   # padding first
    ids[3, 4] = pad   # padding in the middle
    m = (ids != pad).long()
    assert torch.equal(R.position_ids_ref(ids, pad), torch.cumsum(m, 1) * m + pad)


def test_rel_bias_ref_indexing():
    bucket = torch.randint(0, 32, (5, 7), generator=torch.Generator().manual_seed(12)).int()
    table = _rand(32, 3, seed=13)
    ref = R.rel_bias_ref(bucket, table)
    for h in range(3):
        for q in range(5):
            for k in range(7):
                assert ref[h, q, k] == table[bucket[q, k], h]


def test_vit_tokens_refs_are_cat_plus_pos_and_its_autograd():
    B, NP, D = 5, 6, 40
    patch = _rand(B * NP, D, seed=14).double().requires_grad_(True)
    cls = _rand(D, seed=15).double().requires_grad_(True)
    pos = _rand(NP + 1, D, seed=16).double().requires_grad_(True)
    want = torch.cat([cls.expand(B, 1, D), patch.reshape(B, NP, D)], 1) + pos
    assert torch.equal(R.vit_tokens_fwd_ref(patch.detach(), B, cls.detach(), pos.detach()), want.detach())
    dout = _rand(B, NP + 1, D, seed=17).double()
    want.backward(dout)
    dpatch, dcls, dpos = R.vit_tokens_bwd_ref(dout)
    assert torch.equal(dpatch, patch.grad)
    assert torch.allclose(dcls, cls.grad, rtol=0, atol=1e-14) and torch.allclose(dpos, pos.grad, rtol=0, atol=1e-14)


@pytest.mark.parametrize("paths,B,C", [(4, 100, 3), (1, 300, 2), (2, 64, 17)])
def test_xent_ref_is_cross_entropy(paths, B, C):
    logits = [_rand(B, C, seed=20 + i, scale=3.0) for i in range(paths)]
    labels = torch.randint(0, C, (B, 4), generator=torch.Generator().manual_seed(21))
    leaf = [l.double().requires_grad_(True) for l in logits]
    each = [F.cross_entropy(leaf[i], labels[:, i]) for i in range(paths)]
    (0.125 * sum(each)).backward()
    loss, grads = R.xent_ref(logits, labels, dloss_scale=0.125)
    want = torch.stack([sum(each)] + each).detach()
    assert torch.allclose(loss, want, rtol=1e-12, atol=1e-12)
    for g, l in zip(grads, leaf):
        assert torch.allclose(g, l.grad, rtol=0, atol=1e-14)


def test_xent_ref_label_columns_and_extreme_logits():
    logits = [_rand(6, 3, seed=30), _rand(6, 3, seed=31)]
    labels = torch.randint(0, 3, (6, 4), generator=torch.Generator().manual_seed(32))
    loss, _ = R.xent_ref(logits, labels, cols=[1, 3], n_slots=5)
    l1 = F.cross_entropy(logits[0].double(), labels[:, 1])
    l3 = F.cross_entropy(logits[1].double(), labels[:, 3])
    assert torch.allclose(loss, torch.stack([l1 + l3, torch.zeros(()).double(), l1, torch.zeros(()).double(), l3]),
                          rtol=1e-12, atol=0)
    z = torch.tensor([[1000.0, 0.0, -1000.0]] * 3)
    loss, grads = R.xent_ref([z], torch.tensor([0, 1, 2]))
    assert loss[0].item() == 1000.0  # rows 0, 1000, 2000
    assert torch.equal(grads[0], (torch.tensor([[1.0, 0, 0]] * 3) - torch.eye(3)).double() / 3)


@pytest.mark.parametrize("wd", [0.01, 0.0])
def test_adamw_ref_is_torch_adamw_on_doubles(wd):
    ps = [_rand(n, seed=40 + i).double() for i, n in enumerate((1, 257, 1001))]
    leaf = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.AdamW(leaf, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for step in (1, 2, 3):
        for i, l in enumerate(leaf):
            g = _rand(l.numel(), seed=50 + 10 * step + i).double()
            l.grad = g.clone()
            ps[i], ms[i], vs[i] = R.adamw_ref(ps[i], g, ms[i], vs[i], step, 1e-3, 0.9, 0.999, 1e-8, wd)
        opt.step()
        for i, l in enumerate(leaf):
            assert torch.allclose(ps[i], l.detach(), rtol=0, atol=1e-14)
            assert torch.allclose(ms[i], opt.state[l]["exp_avg"], rtol=0, atol=1e-15)
            assert torch.allclose(vs[i], opt.state[l]["exp_avg_sq"], rtol=0, atol=1e-15)


def test_gelu_grad_ref_is_autograd_of_gelu():
    x = torch.cat([torch.linspace(-12, 12, 4001), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 40.0, -40.0]),
                   _rand(500, seed=60)]).double().requires_grad_(True)
    F.gelu(x).sum().backward()
    assert torch.allclose(R.gelu_grad_ref(x.detach()), x.grad, rtol=0, atol=1e-15)
    tails = R.gelu_grad_ref(torch.tensor([40.0, -40.0]))
    assert tails[0].item() == 1.0 and tails[1].item() == 0.0


def test_act_bwd_ref_is_autograd_of_dropout_after_activation():
    x = _rand(300, seed=61).double().requires_grad_(True)
    dy = _rand(300, seed=62).double()
    keep = R.keep_mask_ref(123, 9, (300,), 0.5)
    for act, fn in (("gelu", F.gelu), ("relu", F.relu), ("none", lambda t: t)):
        x.grad = None
        (fn(x) * keep.double() / 0.5).backward(dy)
        assert torch.allclose(R.act_bwd_ref(dy, x.detach(), act, keep, 0.5), x.grad, rtol=0, atol=1e-14)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("seed,salt", [(123, 0), (123, 0xDEADBEEF12345678), ((1 << 40) + 5, 7)])
def test_keep_mask_ref_is_oracle_keep_mask(p, seed, salt):
    ref = R.keep_mask_ref(seed, salt, (37, 55), p)
    assert np.array_equal(ref.numpy(), keep_mask(seed, salt, (37, 55), p))
    assert abs((~ref).double().mean().item() - p) < 0.05
    x = _rand(37, 55, seed=63)
    d = R.dropout_ref(x, ref, p)
    assert torch.equal(d == 0, ~ref) and torch.allclose(d[ref], x[ref].double() / (1 - float(np.float32(p))))


@pytest.mark.parametrize("seed,idx,target", [(123, 777, 0), (123, 0, 429496729), ((1 << 40) + 5, (1 << 33) + 9, 0xFFFFFFFF)])
def test_salt_with_hash_hits_the_target(seed, idx, target):
    salt = R.salt_with_hash(seed, idx, target)
    assert 0 <= salt < (1 << 32) and R.hash_ref(seed, salt, idx) == target
    assert int(dropout_hash(seed, salt, [idx])[0]) == target


@pytest.mark.parametrize("shape,Kpad", [((5, 3, 7, 7), 152), ((8, 16, 3, 3), None)])
@pytest.mark.parametrize("with_bn", [False, True])
def test_conv_weight_prep_ref_is_folded_permuted_weight(shape, Kpad, with_bn):
    Cout, Cin, KH, KW = shape
    w = _rand(*shape, seed=70)
    bn = None
    if with_bn:
        var = _rand(Cout, seed=74).abs() + 0.1
        var[1] = 1e-7
        bn = (1 + 0.1 * _rand(Cout, seed=71), _rand(Cout, seed=72), _rand(Cout, seed=73), var)
    ow, ob = R.conv_weight_prep_ref(w, Kpad, bn, 1e-5)
    s = (bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)) if with_bn else torch.ones(Cout, dtype=torch.float64)
    K = KH * KW * Cin
    want = (w.double() * s[:, None, None, None]).permute(0, 2, 3, 1).reshape(Cout, K)
    assert torch.allclose(ow[:, :K], want, rtol=1e-15, atol=0)
    assert (ow[:, K:] == 0).all() and ow.shape == (Cout, Kpad or K)
    wantb = bn[1].double() - bn[2].double() * s if with_bn else torch.zeros(Cout, dtype=torch.float64)
    assert torch.allclose(ob, wantb, rtol=1e-14, atol=1e-14)


def test_remaining_refs_against_torch_operators():
    dout = _rand(3, 12, seed=80)
    leaf = _rand(3, 7, 12, seed=81).double().requires_grad_(True)
    leaf.mean(1).backward(dout.double())
    assert torch.allclose(R.seq_mean_bwd_ref(dout, 7), leaf.grad, rtol=0, atol=1e-15)
    x, y = _rand(255, seed=82), _rand(255, seed=83)
    assert torch.equal(R.axpby_ref(2.0, x, 0.5, y), torch.add(2.0 * x.double(), y.double(), alpha=0.5))
    assert torch.equal(R.axpby_ref(1.5, x, 7.0, None), 1.5 * x.double())
    xp = _rand(2 * 3, 100, seed=84)
    assert torch.allclose(R.global_avgpool_ref(xp, 2, 3, 100),
                          F.adaptive_avg_pool2d(xp.double().reshape(2, 3, 1, 100).permute(0, 3, 1, 2), 1).reshape(2, 100),
                          rtol=0, atol=1e-15)
    mask = torch.tensor([[1, 0, 3], [0, 0, 1]])
    assert torch.equal(R.mask_to_bias_ref(mask, -1e4), (1 - mask.clamp(max=1)).float() * -1e4)


def test_bounds_accept_one_rounding_and_reject_two():
    """the bf16 bound holds for a correctly rounded bf16 value of anything, and refuses an error of
    one whole bf16 ulp; the fp32 bound is the suite's 3e-5 + 3e-5"""
    x = torch.cat([_rand(20000, seed=90).double(), torch.tensor([1.0 + 2.0 ** -8, 2.0 - 2.0 ** -9])])
    r = x.float().to(torch.bfloat16)
    assert R.bf16_excess(r, x, scale=0.0) <= 0
    off = (r.double() + 2.0 ** -7 * r.double().abs()).to(torch.bfloat16)
    assert R.bf16_excess(off, x, scale=1.0) > 0
    assert R.f32_excess(x.float(), x) <= 0 and R.f32_excess((x * (1 + 1e-4)).float(), x) > 0
    assert math.isclose(R.BF16_EPS, 2.0 ** -8) and R.F32_TOL == 3e-5
