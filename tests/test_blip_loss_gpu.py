"""The caption loss of mmfd.blip (forward(labels=): one-pass teacher forcing, csrc/lm_loss.hip, the hand-written
text-decoder backward) against transformers' float64 results in tests/golden/blip_small_loss.npz
(tests/golden/make_blip_small_loss.py) and against the stepwise generation path.

Bars. logits bar(precision) = max(2 x bert_error, 1e-4 in fp32) x max(1, |logits|max), bert_error being the relative
error of mmfd's BertModel on bert_small.npz in the same session (tests/test_caption_gpu.py's rule): one-pass logits
against the fixture 1 bar, against the stepwise path 2 bars (each within one of the truth). Loss: 2 logits bars (the
loss is 2-Lipschitz in the logits' max norm), a per-sequence sum times its scored positions. Gradients, fp32: every
text_decoder tensor within 5e-4 |ref|max, no floor (the DeBERTa / Swinv2 bar); bf16: |delta|max / max(1, |ref|max)
within 2 x the bf16 BertModel's gradient error on bert_small.npz, measured in the same session as
tests/test_deberta_train_gpu.py measures it. The four attention key biases have a gradient of zero in exact
arithmetic (the fixture's recipe says why and does not store them): what the kernels leave there is held to the bar
of the query bias of the same attention block. Beside the issue's absolute bf16 bar (which a zeroed tensor of a small
gradient would pass), every bf16 gradient tensor with a non-zero reference must point along it: cosine >= 0.99, that
is a relative RMS error under 14 %. bf16 rounds by 2^-8 = 0.4 % and a gradient passes a few tens of roundings that
add like a random walk (a few percent); a tensor that is zero, transposed, misplaced or of the wrong sign has a
cosine near 0 or below.

The vocabulary of 203 (tests/golden/blip_small_loss_v203.npz): the same model with three more vocabulary rows, so
that V is no multiple of 8, as BLIP's 30,524 is none: the logits and dlogits buffers and the LM-head backward then
run on the padded vocabulary (blip.vocab_ld). Same bars; one label lies in the last, partial 8-column chunk.

Measured on an MI355X: DESIGN.md, section 9."""
import json
import os

import numpy as np
import pytest
import torch

from tests import blip_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    z, cfg, W = R.load_fixture()
    zl = np.load(os.path.join(R.G, "blip_small_loss.npz"), allow_pickle=False)
    t = lambda k: torch.from_numpy(zl[k])  # noqa: E731
    return dict(cfg=cfg, W=W, px=torch.from_numpy(z["pixel_values"]), seq=torch.from_numpy(z["sequences"]), zl=zl,
                ids=t("input_ids"), mask=t("attention_mask"), labels=t("labels"), n=t("n_scored"),
                logits=torch.from_numpy(zl["logits"]).double())


def _model(fx, precision="fp32", train=False, eps=0.0, frozen=True, **text):
    from mmfd.blip import BlipConfig, BlipForConditionalGeneration
    m = BlipForConditionalGeneration(BlipConfig(vision=fx["cfg"]["vision"],
                                                text=dict(fx["cfg"]["text"], label_smoothing=eps, **text),
                                                train_text_decoder=train))
    m.load_state_dict(fx["W"], strict=True)
    if frozen:
        for p in m.parameters():
            p.requires_grad_(False)
    return m.to(DEV).eval().set_precision(precision)


@pytest.fixture(scope="module")
def bert_error():
    """|delta|max / max(1, |ref|max) of mmfd's BertModel on bert_small.npz, per precision (existing code)"""
    from mmfd.encoders import BertConfig, BertModel
    z = np.load(os.path.join(R.G, "bert_small.npz"), allow_pickle=False)
    m = BertModel(BertConfig(**json.loads(str(z["config"]))))
    m.load_state_dict({k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")})
    m = m.to(DEV).eval()
    out = {}
    for prec in ("fp32", "bf16"):
        with torch.no_grad():
            y = m.set_precision(prec)(input_ids=torch.from_numpy(z["input_ids"]).to(DEV),
                                      attention_mask=torch.from_numpy(z["attention_mask"]).to(DEV),
                                      token_type_ids=torch.from_numpy(z["token_type_ids"]).to(DEV)).last_hidden_state
        ref = torch.from_numpy(z["out"]).double()
        out[prec] = (y.double().cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        print(f"BertModel on bert_small.npz, {prec}: relative error {out[prec]:.3e}")
    return out


@pytest.fixture(scope="module")
def bert_bf16_grad_error():
    """worst |delta|max / max(1, |ref|max) of the bf16 BertModel's parameter gradients on bert_small.npz"""
    from mmfd.encoders import BertConfig, BertModel
    z = np.load(os.path.join(R.G, "bert_small.npz"), allow_pickle=False)
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


def _logits_bar(fx, bert_error, precision):
    return max(2.0 * bert_error[precision], 1e-4 if precision == "fp32" else 0.0) * max(1.0, fx["logits"].abs().max().item())


def _loss(m, fx, **kw):
    return m(fx["px"], fx["ids"], attention_mask=fx["mask"], labels=fx["labels"], **kw)


def test_fixture_meets_its_conditions(fx):
    zl = fx["zl"]
    lengths = zl["attention_mask"].sum(1)
    assert len(set(lengths.tolist())) >= 2 and (zl["attention_mask"].shape[1] - lengths).max() >= 5
    assert zl["input_ids"].shape == (4, 21) and (zl["input_ids"][zl["attention_mask"] == 0] == 0).all()
    assert (zl["labels"][zl["attention_mask"] == 0] == -100).all()
    assert (zl["labels"][int(zl["prompt_row"]), :3] == -100).all()
    grads = [k for k in zl.files if k.startswith("g.")]
    assert len(grads) >= 40
    for k in grads:
        assert np.abs(zl[k]).max() >= 1e-4, k
    assert float(zl["fp32_loss_error"]) <= 1e-5
    assert sorted(str(k) for k in zl["zero_grads"]) == sorted(
        f"text_decoder.bert.encoder.layer.{i}.{a}.self.key.bias" for i in range(2) for a in ("attention", "crossattention"))


def test_one_pass_logits_match_the_stepwise_path_and_the_fixture(fx, bert_error):
    m = _model(fx)
    out = _loss(m, fx, return_logits=True)
    step = m.forward_logits(fx["px"], fx["ids"]).permute(1, 0, 2)  # [B, T, V]: step t follows ids[:, :t + 1]
    live = fx["mask"].bool()
    bar = _logits_bar(fx, bert_error, "fp32")
    one = out.logits.double().cpu()
    e_step = (one - step.double().cpu()).abs()[live].max().item()
    e_fix = (one - fx["logits"]).abs()[live].max().item()
    print(f"one-pass logits fp32: vs stepwise {e_step:.3e} (bar {2 * bar:.3e}), vs fixture {e_fix:.3e} (bar {bar:.3e})")
    assert out.logits.dtype == torch.float32 and tuple(out.logits.shape) == (4, 21, 200)
    assert e_step <= 2 * bar and e_fix <= bar


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_loss_matches_the_fixture(fx, bert_error, precision, eps):
    m = _model(fx, precision, eps=eps)
    bar = 2.0 * _logits_bar(fx, bert_error, precision)
    mean = _loss(m, fx).loss
    none = _loss(m, fx, reduction="none").loss
    ref_mean, ref_none = float(fx["zl"][f"loss_mean.{eps:g}"]), torch.from_numpy(fx["zl"][f"loss_none.{eps:g}"])
    e_mean = abs(mean.item() - ref_mean)
    e_none = (none.double().cpu() - ref_none).abs()
    print(f"caption loss {precision} eps {eps}: mean {mean.item():.6f} (ref {ref_mean:.6f}, err {e_mean:.3e}, bar {bar:.3e}); "
          f"sums err {e_none.tolist()}, bars {(bar * fx['n'].double()).tolist()}")
    assert mean.dtype == torch.float32 and mean.dim() == 0 and none.dtype == torch.float32 and tuple(none.shape) == (4,)
    assert _loss(m, fx).logits is None
    assert e_mean <= bar
    assert (e_none <= bar * fx["n"].double()).all()


def _grads(m, fx, **kw):
    for p in m.parameters():
        p.grad = None
    out = _loss(m, fx, **kw)
    out.loss.backward() if out.loss.dim() == 0 else (out.loss * kw_weights(fx)).sum().backward()
    torch.cuda.synchronize()
    return out, {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


def kw_weights(fx):
    """per-sequence weights that turn the reduction="none" sums into the mean"""
    return torch.full((4,), 1.0 / float(fx["n"].sum()), device=DEV)


def _grad_errors(fx, g):
    """name -> (|delta|max, |ref|max); a key bias (zero in exact arithmetic) is paired with the |ref|max of the query
    bias of its attention block"""
    zl, out = fx["zl"], {}
    for n, t in g.items():
        if n.startswith("vision_model."):
            assert t is None, n
            continue
        assert t is not None and t.dtype == torch.float32, n
        if n.endswith(".key.bias"):
            out[n] = (t.abs().max().item(), float(np.abs(zl["g." + n.replace(".key.bias", ".query.bias")]).max()))
            continue
        ref = torch.from_numpy(zl["g." + n]).double()
        assert tuple(t.shape) == tuple(ref.shape), n
        out[n] = ((t.double().cpu() - ref).abs().max().item(), ref.abs().max().item())
    assert len(out) == len([k for k in zl.files if k.startswith("g.")]) + len(zl["zero_grads"])
    return out


def _cosines(zl, g):
    """name -> cosine between a gradient and its stored reference (0 for a zero gradient)"""
    out = {}
    for k in zl.files:
        if k.startswith("g."):
            ref, got = torch.from_numpy(zl[k]).double().flatten(), g[k[2:]].double().cpu().flatten()
            out[k[2:]] = (got @ ref).item() / max(got.norm().item() * ref.norm().item(), 1e-300)
    return out


def test_gradients_fp32_match_transformers_and_repeat_bit_for_bit(fx):
    m = _model(fx, "fp32", train=True, eps=0.1, frozen=False)
    out, g = _grads(m, fx)
    assert out.loss.requires_grad and abs(out.loss.item() - float(fx["zl"]["loss_mean.0.1"])) <= 1e-4
    errs = _grad_errors(fx, g)
    worst = max(errs.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"caption-loss gradients fp32: worst |delta|max / |ref|max {worst[1][0] / worst[1][1]:.3e} ({worst[0]}), bar 5e-4")
    fails = [f"{n}: {e / r:.3e}" for n, (e, r) in errs.items() if e > 5e-4 * r]
    assert not fails, fails[:8]
    _, g2 = _grads(m, fx)
    for n, t in g.items():
        assert (t is None and g2[n] is None) or torch.equal(t, g2[n]), n
    # the per-sequence form of the backward, weighted so that it is the mean again
    _, g3 = _grads(m, fx, reduction="none")
    fails = [f"{n}: {e / r:.3e}" for n, (e, r) in _grad_errors(fx, g3).items() if e > 5e-4 * r]
    assert not fails, fails[:8]


def test_gradients_bf16_within_twice_bert(fx, bert_bf16_grad_error):
    m = _model(fx, "bf16", train=True, eps=0.1, frozen=False)
    _, g = _grads(m, fx)
    bar = 2.0 * bert_bf16_grad_error
    errs = _grad_errors(fx, g)
    worst = max(errs.items(), key=lambda kv: kv[1][0] / max(1.0, kv[1][1]))
    print(f"caption-loss gradients bf16: worst error {worst[1][0] / max(1.0, worst[1][1]):.3e} ({worst[0]}), bar {bar:.3e}; "
          f"worst relative to |ref|max {max(e / r for e, r in errs.values()):.3e}")
    fails = [f"{n}: {e / max(1.0, r):.3e}" for n, (e, r) in errs.items() if e / max(1.0, r) > bar]
    assert not fails, (bar, fails[:8])
    cos = _cosines(fx["zl"], g)
    print(f"caption-loss gradients bf16: smallest cosine {min(cos.values()):.5f} ({min(cos, key=cos.get)})")
    assert len(cos) >= 40 and not [n for n, c in cos.items() if c < 0.99], sorted(cos.items(), key=lambda kv: kv[1])[:8]
    _, g2 = _grads(m, fx)
    for n, t in g.items():
        assert (t is None and g2[n] is None) or torch.equal(t, g2[n]), n


@pytest.fixture(scope="module")
def fx203(fx):
    """the fixture's model with the three more vocabulary rows of blip_small_loss_v203.npz"""
    zl = np.load(os.path.join(R.G, "blip_small_loss_v203.npz"), allow_pickle=False)
    W = dict(fx["W"])
    for k, w in W.items():  # the tied table and the LM-head bias, under each of their names
        if k.startswith("text_decoder.") and w.shape[0] == 200 and ("word_embeddings" in k or "cls.predictions" in k):
            W[k] = torch.cat([w, torch.from_numpy(zl["extra_word"] if w.dim() == 2 else zl["extra_bias"])])
    cfg = dict(fx["cfg"], text=dict(fx["cfg"]["text"], vocab_size=203))
    t = lambda k: torch.from_numpy(zl[k])  # noqa: E731
    return dict(fx, cfg=cfg, W=W, zl=zl, ids=t("input_ids"), mask=t("attention_mask"), labels=t("labels"), n=t("n_scored"))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_vocabulary_that_is_no_multiple_of_8(fx203, bert_error, bert_bf16_grad_error, precision):
    from mmfd.blip import lm_head_gemm_paths, vocab_ld
    fx, zl = fx203, fx203["zl"]
    assert vocab_ld(203) == 208 and int(zl["labels"][0, 4]) == 201 and 201 // 8 == 203 // 8
    stored = [k[2:] for k in zl.files if k.startswith("g.")]
    assert len(stored) == 11 and all(np.abs(zl["g." + n]).max() >= 1e-4 for n in stored)
    dt = torch.float32 if precision == "fp32" else torch.bfloat16
    paths = lm_head_gemm_paths(dt, 4 * 21, 203, 96)
    print(f"LM-head products at V = 203, {precision}: {paths}")
    assert all(path != "simple" for path, _ in paths.values()), paths
    m = _model(fx, precision, train=True, eps=0.1, frozen=False)
    bar = 2.0 * max(2.0 * bert_error[precision], 1e-4 if precision == "fp32" else 0.0) * max(1.0, float(zl["logits_absmax"]))
    with torch.no_grad():
        none = _loss(m, fx, reduction="none").loss
        logits = _loss(m, fx, return_logits=True).logits
    assert tuple(logits.shape) == (4, 21, 203) and logits.is_contiguous()
    out, g = _grads(m, fx)
    e_mean = abs(out.loss.item() - float(zl["loss_mean.0.1"]))
    e_none = (none.double().cpu() - torch.from_numpy(zl["loss_none.0.1"])).abs()
    print(f"caption loss V = 203 {precision}: mean err {e_mean:.3e} (bar {bar:.3e}); sums err {e_none.tolist()}, "
          f"bars {(bar * fx['n'].double()).tolist()}")
    assert e_mean <= bar and (e_none <= bar * fx["n"].double()).all()
    gbar = 2.0 * bert_bf16_grad_error
    for n in stored:
        ref = torch.from_numpy(zl["g." + n]).double()
        assert g[n] is not None and tuple(g[n].shape) == tuple(ref.shape), n
        e, r = (g[n].double().cpu() - ref).abs().max().item(), ref.abs().max().item()
        print(f"  gradient V = 203 {precision} {n}: |delta|max {e:.3e}, |ref|max {r:.3e}")
        if precision == "fp32":
            assert e <= 5e-4 * r, n
        else:
            assert e / max(1.0, r) <= gbar, n
    if precision == "bf16":
        cos = _cosines(zl, g)
        print(f"  smallest cosine {min(cos.values()):.5f} ({min(cos, key=cos.get)})")
        assert not [n for n, c in cos.items() if c < 0.99], cos
    _, g2 = _grads(m, fx)
    for n, t in g.items():
        assert (t is None and g2[n] is None) or torch.equal(t, g2[n]), n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ids_under_the_padding_change_nothing(fx, precision):
    m = _model(fx, precision, train=True, eps=0.1, frozen=False)
    out, g = _grads(m, fx)
    other = dict(fx, ids=torch.where(fx["mask"] == 1, fx["ids"], torch.randint(1, 200, fx["ids"].shape,
                                                                                generator=torch.Generator().manual_seed(3))))
    assert not torch.equal(other["ids"], fx["ids"])
    out2, g2 = _grads(m, other)
    assert torch.equal(out.loss, out2.loss)
    none = _loss(m, fx, reduction="none").loss
    assert torch.equal(none, _loss(m, other, reduction="none").loss)
    for n, t in g.items():
        assert (t is None and g2[n] is None) or torch.equal(t, g2[n]), n


def test_a_token_changes_no_earlier_logits(fx):
    m = _model(fx)
    base = _loss(m, fx, return_logits=True).logits
    for row, t in ((0, 7), (0, 20), (1, 2)):
        ids = fx["ids"].clone()
        ids[row, t] = (ids[row, t] + 5) % 190 + 1
        got = m(fx["px"], ids, attention_mask=fx["mask"], labels=fx["labels"], return_logits=True).logits
        assert torch.equal(got[:, :t], base[:, :t])
        assert not torch.equal(got[row, t], base[row, t])
        others = [r for r in range(4) if r != row]
        assert torch.equal(got[others], base[others])


def test_contract(fx):
    from mmfd.blip import BlipCaptionLossOutput
    # a default-config model under grad is inference-only, with and without labels
    m = _model(fx, frozen=False)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m(fx["px"], fx["ids"])
    with pytest.raises(NotImplementedError, match="inference-only"):
        _loss(m, fx)
    with torch.no_grad():  # under no_grad the loss works on any model
        out = _loss(m, fx)
    assert isinstance(out, BlipCaptionLossOutput) and not out.loss.requires_grad
    # text dropout in training mode
    d = _model(fx, train=True, frozen=False, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        _loss(d.train(), fx)
    _loss(d.eval(), fx).loss.backward()
    # without labels: what forward returned before, bit for bit
    f = _model(fx)
    assert torch.equal(f(fx["px"], fx["ids"]), f.forward_logits(fx["px"], fx["ids"]))
    with pytest.raises(ValueError, match="pass labels"):
        f(fx["px"], fx["ids"], attention_mask=fx["mask"])
    # only right padding; labels inside the vocabulary
    left = fx["mask"].flip(1)
    with pytest.raises(ValueError, match="starts with padding"):
        f(fx["px"], fx["ids"], attention_mask=left, labels=fx["labels"])
    hole = fx["mask"].clone()
    hole[0, 5] = 0
    with pytest.raises(ValueError, match="follows padding"):
        f(fx["px"], fx["ids"], attention_mask=hole, labels=fx["labels"])
    bad = fx["labels"].clone()
    bad[0, 5] = 200
    with pytest.raises(ValueError, match="neither in"):
        f(fx["px"], fx["ids"], attention_mask=fx["mask"], labels=bad)
    with pytest.raises(ValueError, match="reduction"):
        _loss(f, fx, reduction="sum")


def test_generation_is_unchanged_after_a_loss_call(fx):
    m = _model(fx, train=True, eps=0.1)
    for p in m.text_decoder.parameters():
        p.requires_grad_(True)
    before = m.generate(fx["px"], use_graph=False)
    beams_before = m.generate(fx["px"], num_beams=3, use_graph=False)
    _loss(m, fx).loss.backward()
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    assert torch.equal(before, fx["seq"])
    assert torch.equal(m.generate(fx["px"], use_graph=False), fx["seq"])
    assert torch.equal(m.generate(fx["px"], use_graph=True), fx["seq"])
    assert torch.equal(m.generate(fx["px"], num_beams=3, use_graph=False), beams_before)


def test_a_batch_of_fewer_than_16_rows(fx):
    """B * T < 16: the pass pads the batch (blip.py, _loss_inputs); one short row gives what it gives in the batch"""
    m = _model(fx, eps=0.1)
    ids, mask, labels = fx["ids"][1:2, :6], fx["mask"][1:2, :6], fx["labels"][1:2, :6]
    assert int(mask.sum()) == 4
    got = m(fx["px"][1:2], ids, attention_mask=mask, labels=labels, reduction="none", return_logits=True)
    ref = _loss(m, fx, reduction="none", return_logits=True)
    assert tuple(got.loss.shape) == (1,) and tuple(got.logits.shape) == (1, 6, 200)
    assert abs(got.loss.item() - ref.loss[1].item()) <= 1e-4
    assert (got.logits[0, :4] - ref.logits[1, :4]).abs().max().item() <= 1e-4


def test_captioner_score_is_the_negated_per_sequence_loss(fx):
    from mmfd.caption import Captioner
    from tests.toy_tokenizer import toy_tokenizer
    tok = toy_tokenizer()
    m = _model(fx, eps=0.1)  # score ignores the configured smoothing
    cap = Captioner(m, tokenizer=tok)
    texts = ["w1 w2 w3", "w4", "w5 w6 w7 w8 w9 w10 w11", "w12 w13"]
    ll, n = cap.score(fx["px"], texts)
    enc = tok(texts, padding=True, return_tensors="pt")
    ids = enc["input_ids"].clone()
    ids[:, 0] = fx["cfg"]["text"]["bos_token_id"]
    labels = ids.masked_fill(enc["attention_mask"] == 0, -100)
    ref = _model(fx)(fx["px"], ids, attention_mask=enc["attention_mask"], labels=labels, reduction="none").loss
    assert torch.equal(ll, -ref) and m.config.text.label_smoothing == 0.1
    assert n.tolist() == [len(t.split()) + 1 for t in texts]  # the words and [SEP]; the first token is not scored
    assert (ll < 0).all()
