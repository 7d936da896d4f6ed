"""Trainable DeBERTa-v3 with dropout on the HIP path (hidden_dropout_prob = attention_probs_dropout_prob = 0.1,
transformers' default): the forward and every parameter gradient against the float64 restatement of
tests/deberta_dropout_ref.py under IDENTICAL masks (oracle.dropout_hash.Drop with the model's seed; the
restatement's sites are pinned to transformers' on the CPU, tests/test_deberta_dropout_ref_cpu.py), the
seed semantics, the opt-in semantics, and the trainer.

Bars, all taken from tests/test_deberta_train_gpu.py (the masks do not depend on values, so dropout flips
no element and adds no error term of its own). fp32: output 1e-4 abs at hidden 64, 1e-3 at xsmall width;
every parameter gradient 5e-4 * max(1, |ref|max), and the position tensors (rel_embeddings,
encoder.LayerNorm) additionally 5e-4 * |ref|max without the floor. bf16 at xsmall width: output 0.25 max /
1e-2 mean abs, gradients 1.97e-2 * max(1, |ref|max) — twice the bf16 BertModel's own worst error on
bert_small.npz (9.851e-3), the bar the dropout-free DeBERTa is held to."""
import pytest
import torch

from oracle.dropout_hash import Drop
from tests.deberta_dropout_ref import reference_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"
P_DROP = 0.1
SEED = 4242
POS_TENSORS = ("encoder.rel_embeddings.weight", "encoder.LayerNorm.weight", "encoder.LayerNorm.bias")
BF16_GRAD_BAR = 1.97e-2


def _model(precision, *, p=P_DROP, hidden=64, heads=2, layers=2, inter=128, vocab=1000, seed=3, train=True, **kw):
    from mmfd.deberta import DebertaV2Config, DebertaV2Model
    torch.manual_seed(seed)
    m = DebertaV2Model(DebertaV2Config(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers,
                                       num_attention_heads=heads, intermediate_size=inter, trainable=True,
                                       hidden_dropout_prob=p, attention_probs_dropout_prob=p, **kw))
    with torch.no_grad():
        for q in m.parameters():  # LayerNorm / bias parameters off their trivial init
            q.add_(torch.randn_like(q) * 0.02)
        m.embeddings.word_embeddings.weight[0].zero_()
    m = m.cuda().set_precision(precision)
    return m.train() if train else m.eval()


def _batch(lens, L, D, vocab=1000, seed=0):
    g = torch.Generator().manual_seed(seed + L)
    B = len(lens)
    ids = torch.randint(1, vocab, (B, L), generator=g)
    mask = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = ids * mask
    R = torch.randn(B, L, D, generator=g)
    return ids, mask, R


def _run(m, ids, mask, R):
    """(output, {name: grad}) of one forward/backward of (last_hidden_state * R).sum()"""
    m.zero_grad(set_to_none=True)
    out = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    (out.float() * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _reference(m, ids, mask, R, seed):
    c = m.config
    return reference_grads(m.state_dict(), ids, mask, R, num_layers=c.num_hidden_layers,
                           num_heads=c.num_attention_heads, eps=c.layer_norm_eps, drop=Drop(seed, P_DROP))


def _grad_errors(grads, ref_grads):
    out = {}
    for n, g in grads.items():
        ref = ref_grads[n].double()
        out[n] = ((g.double().cpu() - ref).abs().max().item(), ref.abs().max().item())
    return out


def _check_fp32_grads(errs):
    fails = []
    worst = max(errs.items(), key=lambda kv: kv[1][0] / max(1.0, kv[1][1]))
    print(f"worst gradient error / max(1, |ref|max): {worst[1][0] / max(1.0, worst[1][1]):.3e} ({worst[0]})")
    for n, (e, r) in errs.items():
        bound = 5e-4 * (r if n in POS_TENSORS else max(1.0, r))
        if n in POS_TENSORS:
            print(f"{n}: |delta|max {e:.3e}, |ref|max {r:.3e}, relative {e / r:.3e}")
        if e > bound:
            fails.append(f"{n}: {e:.3e} > {bound:.3e} (|ref|max {r:.3e})")
    assert not fails, "; ".join(fails)


# ---------------------------------------------------------------------------------------------
# 1. the model against the restatement, identical masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["small-L300-stream", "xsmall-L160-resident"])
def test_dropout_fp32_matches_reference(shape):
    """hidden 64 / 2 layers / 2 heads at L = 300 (streaming attention kernels, ragged lengths 300 / 171 / 233: two
    rows with padding); xsmall width (384, 6 heads, d = 64) with 2 layers at L = 160 (resident kernels, row 1
    padded from 80). The loss weights every row, padded ones included (the restatement has mmfd's rule)."""
    if shape.startswith("small"):
        m, (ids, mask, R), otol = _model("fp32"), _batch([300, 171, 233], 300, 64), 1e-4
    else:
        m = _model("fp32", hidden=384, heads=6, inter=1536, vocab=2000)
        (ids, mask, R), otol = _batch([160, 80], 160, 384, vocab=2000), 1e-3
    m.manual_seed(SEED)
    out, grads = _run(m, ids, mask, R)
    ref, ref_grads = _reference(m, ids, mask, R, SEED)
    oerr = (out.double().cpu() - ref).abs().max().item()
    print(f"{shape}: output |delta|max {oerr:.3e} (bar {otol:.0e})")
    assert oerr < otol, oerr
    # the masks are on: the dropout-free forward is far away
    plain, _ = reference_grads(m.state_dict(), ids, mask, R, num_layers=2, num_heads=m.config.num_attention_heads,
                               eps=m.config.layer_norm_eps)
    assert (plain - ref).abs().max().item() > 0.1
    _check_fp32_grads(_grad_errors(grads, ref_grads))
    # padded positions carry id 0 = padding_idx: no gradient reaches that embedding row
    assert grads["embeddings.word_embeddings.weight"][0].abs().max().item() == 0.0


def test_dropout_bf16_close_to_reference():
    """bf16 at xsmall width, 2 layers, L = 160, against the float64 restatement on the fp32 master weights"""
    m = _model("bf16", hidden=384, heads=6, inter=1536, vocab=2000)
    ids, mask, R = _batch([160, 80], 160, 384, vocab=2000)
    m.manual_seed(SEED)
    out, grads = _run(m, ids, mask, R)
    ref, ref_grads = _reference(m, ids, mask, R, SEED)
    diff = (out.double().cpu() - ref).abs()
    print(f"bf16 output: |delta| max {diff.max().item():.3e}, mean {diff.mean().item():.3e}")
    assert diff.max().item() < 0.25 and diff.mean().item() < 1e-2, (diff.max().item(), diff.mean().item())
    errs = _grad_errors(grads, ref_grads)
    worst = max(errs.items(), key=lambda kv: kv[1][0] / max(1.0, kv[1][1]))
    print(f"bf16 DeBERTa with dropout: worst gradient error {worst[1][0] / max(1.0, worst[1][1]):.3e} ({worst[0]}), "
          f"bar {BF16_GRAD_BAR:.3e}")
    fails = [f"{n}: {e / max(1.0, r):.3e}" for n, (e, r) in errs.items() if e / max(1.0, r) > BF16_GRAD_BAR]
    assert not fails, (BF16_GRAD_BAR, fails[:8])


# ---------------------------------------------------------------------------------------------
# 2. seeds
# ---------------------------------------------------------------------------------------------
def _equal(a, b):
    return all(torch.equal(a[n], b[n]) for n in a)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_seed_semantics(precision):
    """the same manual_seed gives bit-identical outputs and gradients; the next training forward differs
    (the device seed advanced); manual_seed on another value differs too"""
    m = _model(precision)
    ids, mask, R = _batch([70, 41], 70, 64)
    m.manual_seed(SEED)
    o1, g1 = _run(m, ids, mask, R)
    o2, g2 = _run(m, ids, mask, R)  # seed + 1
    m.manual_seed(SEED)
    o3, g3 = _run(m, ids, mask, R)
    m.manual_seed(SEED + 1)
    o4, g4 = _run(m, ids, mask, R)
    assert torch.equal(o1, o3) and _equal(g1, g3)
    assert not torch.equal(o1, o2) and not _equal(g1, g2)
    assert torch.equal(o2, o4) and _equal(g2, g4)  # advancing once == seeding with the next value


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_eval_and_p0_are_the_dropout_free_model(precision, monkeypatch):
    """eval mode with p = 0.1 is bit for bit the p = 0 model, output and gradients; a p = 0 model in training
    mode too, and its backward still takes dS from attn_bwd's d_rel_bias (attn_bwd_ds is never called);
    under no_grad a training-mode p = 0.1 model is the inference forward"""
    from mmfd import kernels as K
    ids, mask, R = _batch([70, 41], 70, 64)
    a = _model(precision, p=0.0, train=False)
    b = _model(precision, p=P_DROP, train=False)
    c = _model(precision, p=0.0, train=True)
    calls = {"ds": 0, "bwd_with_drel": 0, "bwd_without": 0}
    real_ds, real_bwd = K.attn_bwd_ds, K.attn_bwd

    def spy_ds(*x, **kw):
        calls["ds"] += 1
        return real_ds(*x, **kw)

    def spy_bwd(*x, **kw):
        calls["bwd_with_drel" if kw.get("d_rel_bias") is not None else "bwd_without"] += 1
        return real_bwd(*x, **kw)

    monkeypatch.setattr(K, "attn_bwd_ds", spy_ds)
    monkeypatch.setattr(K, "attn_bwd", spy_bwd)
    oa, ga = _run(a, ids, mask, R)
    ob, gb = _run(b, ids, mask, R)
    oc, gc = _run(c, ids, mask, R)
    assert calls == {"ds": 0, "bwd_with_drel": 6, "bwd_without": 0}, calls
    assert torch.equal(oa, ob) and _equal(ga, gb)
    assert torch.equal(oa, oc) and _equal(ga, gc)
    d = _model(precision, p=P_DROP, train=True)
    with torch.no_grad():  # (the inference forward: compared with the p = 0 model's own no_grad forward)
        od = d(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
        oa_ng = a(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    assert torch.equal(oa_ng, od) and not od.requires_grad
    od2, _ = _run(d, ids, mask, R)  # and under grad it drops: attn_bwd without d_rel_bias, then attn_bwd_ds
    assert not torch.equal(oa, od2)
    assert calls == {"ds": 2, "bwd_with_drel": 6, "bwd_without": 2}, calls


def test_unequal_probabilities_raise():
    from mmfd.deberta import DebertaV2Config, DebertaV2Model
    ids = torch.ones(1, 8, dtype=torch.long, device=DEV)
    for hp, ap in ((0.1, 0.2), (0.2, 0.1), (0.1, 0.0), (0.0, 0.1)):
        m = DebertaV2Model(DebertaV2Config(vocab_size=100, hidden_size=64, num_hidden_layers=1, num_attention_heads=2,
                                           intermediate_size=128, trainable=True, hidden_dropout_prob=hp,
                                           attention_probs_dropout_prob=ap)).cuda().train()
        with pytest.raises(NotImplementedError, match="dropout"):
            m(input_ids=ids)
        assert m.eval()(input_ids=ids).last_hidden_state.shape == (1, 8, 64)
    m = DebertaV2Model(DebertaV2Config(vocab_size=100, hidden_size=64, num_hidden_layers=1, num_attention_heads=2,
                                       intermediate_size=128, trainable=True, hidden_dropout_prob=0.1,
                                       attention_probs_dropout_prob=0.1)).cuda().train()
    assert m(input_ids=ids).last_hidden_state.requires_grad  # transformers' default now trains


# ---------------------------------------------------------------------------------------------
# 3. trainer
# ---------------------------------------------------------------------------------------------
def _trainer(precision, text_seed=77):
    from mmfd.deberta import DebertaV2Config, DebertaV2Model
    from mmfd.train import FusionTrainer
    from tests.smoke_impl import TINY, build_modules
    _, image, head, _ = build_modules(dropout=0.1, cfg=TINY, seed=5)
    torch.manual_seed(6)
    text = DebertaV2Model(DebertaV2Config(vocab_size=1000, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                                          intermediate_size=128, trainable=True, hidden_dropout_prob=P_DROP,
                                          attention_probs_dropout_prob=P_DROP))
    dev = torch.device("cuda", 0)
    text, image, head = text.to(dev), image.to(dev), head.to(dev)
    head.manual_seed(99)
    text.manual_seed(text_seed)
    return FusionTrainer(text, image, head, lr=1e-3, precision=precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_trainer_dropout_eager_and_captured(precision):
    """the smallest trainer with the small trainable DeBERTa at p = 0.1 as text encoder: three captured replays
    end where three eager steps from the same start end (after the capture's two warm-up steps, as
    test_trainer_gpu.py::test_captured_step_replays_equal_eager_steps does for BERT: losses to 1e-5 fp32 /
    1e-3 bf16, parameters to 3 steps x lr) — the device seed advances inside the graph exactly as eagerly"""
    from tests.smoke_impl import tiny_batch
    tr_e, tr_g = _trainer(precision), _trainer(precision)
    assert not tr_e.freeze_text
    b1 = {k: v.cuda() for k, v in tiny_batch(3, seed=41).items()}
    b2 = {k: v.cuda() for k, v in tiny_batch(3, seed=42).items()}
    static = {k: v.clone() for k, v in b1.items()}
    tr_g.capture(static, warmup=2)
    le = [tr_e.step(b1) for _ in range(2)]
    le += [tr_e.step(b1), tr_e.step(b2), tr_e.step(b1)]
    lg = [tr_g.replay().clone(), tr_g.replay(b2).clone(), tr_g.replay(b1).clone()]
    torch.cuda.synchronize()
    tol = 1e-5 if precision == "fp32" else 1e-3
    for a, b in zip(le[2:], lg):
        assert torch.isfinite(a).all()
        assert (a.detach() - b).abs().max().item() <= tol * max(1.0, a.abs().max().item()), (a, b)
    lr = tr_e.optimizer.param_groups[0]["lr"]
    for m_e, m_g in ((tr_e.text_encoder, tr_g.text_encoder), (tr_e.image_encoder, tr_g.image_encoder),
                     (tr_e.head, tr_g.head)):
        for (n, p), (_, q) in zip(m_e.named_parameters(), m_g.named_parameters()):
            assert (p - q).abs().max().item() <= 3 * lr + 1e-6, n
    # the text seed advanced once per step, inside the graph as eagerly
    assert int(tr_e.text_encoder._seed.t.item()) == int(tr_g.text_encoder._seed.t.item()) > 77


def test_trainer_second_step_draws_new_text_masks():
    """two steps on the same batch, twice: in the second run the text encoder's seed is put back before step
    two, so that step repeats step one's text masks on the same weights (the head's own seed advances in
    both runs). Step one agrees, step two does not: the seed a step uses matters, and it advances."""
    from tests.smoke_impl import tiny_batch
    b = {k: v.cuda() for k, v in tiny_batch(3, seed=41).items()}
    tr_a, tr_b = _trainer("fp32"), _trainer("fp32")
    la = [tr_a.step(b).clone(), tr_a.step(b).clone()]
    lb = [tr_b.step(b).clone()]
    tr_b.text_encoder.manual_seed(77)  # not advanced
    lb.append(tr_b.step(b).clone())
    torch.cuda.synchronize()
    print("losses, seed advancing:", la[1].tolist(), "seed put back:", lb[1].tolist())
    assert (la[0] - lb[0]).abs().max().item() <= 1e-5 * max(1.0, la[0].abs().max().item())
    assert (la[1] - lb[1]).abs().max().item() > 1e-4
