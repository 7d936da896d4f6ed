"""Writes tests/golden/blip_small_loss.npz: transformers' caption loss (BlipTextLMHeadModel with labels) of the
model of blip_small.npz, run on the CPU in float64, and the gradients of its text decoder.

  input_ids       int64 [4, 21]: blip_small.npz's four generated rows (bos first), cut after their [SEP] and
                  right-padded with 0; attention_mask int64 [4, 21] follows the row lengths
  labels          int64 [4, 21]: the ids, -100 on the padding and on the first three positions of row `prompt_row`
                  (a prompt that is not scored)
  loss_mean.<e>   float64 scalar, loss_none.<e> float64 [4] (reduction="none": per-sequence sums), for label
                  smoothing e in {0, 0.1} (keys "0" and "0.1")
  n_scored        int64 [4]: scored positions per row
  logits          float32 [4, 21, 200] (the float64 logits, rounded once)
  g.<name>        float32: for smoothing 0.1, the gradient of the mean loss with respect to every text_decoder
                  parameter (mmfd's names; the tied table under ...word_embeddings.weight), computed in float64 —
                  but for the four attention key biases (`zero_grads`): a key bias adds the same q . b to every
                  score of a query row, softmax ignores it, and its gradient is zero in exact arithmetic (1e-18
                  here in float64). No |g|max >= 1e-4 can be asked of them, so they are not stored; the tests hold
                  them to the bar of the query bias of the same attention block.
  fp32_loss_error the largest |fp32 - float64| over the four stored losses of transformers' own fp32 pass

Asserted here and again by the tests: the row lengths differ and one row has >= 5 pads; every stored gradient has
|g|max >= 1e-4; transformers' fp32 loss lies within 1e-5 of the float64 one.

Run from the repository root: python tests/golden/make_blip_small_loss.py
(needs the `transformers` package; the test suite only reads the .npz)."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = (0.0, 0.1)
IGNORE = -100


def inputs(seq, sep, pad):
    """(ids, mask, labels, prompt_row) from the generated rows"""
    seq = np.asarray(seq)
    B, T = seq.shape
    mask = np.ones((B, T), dtype=np.int64)
    for b in range(B):
        hit = np.nonzero(seq[b, 1:] == sep)[0]
        if hit.size:
            mask[b, hit[0] + 2:] = 0
    ids = np.where(mask == 1, seq, pad).astype(np.int64)
    lengths = mask.sum(1)
    assert len(set(lengths.tolist())) >= 2, f"row lengths do not differ: {lengths}"
    assert (T - lengths).max() >= 5, f"no row with >= 5 pads: {lengths}"
    labels = np.where(mask == 1, ids, IGNORE).astype(np.int64)
    prompt_row = int(lengths.argmax())
    labels[prompt_row, :3] = IGNORE
    return ids, mask, labels, prompt_row


def check(z):
    """the conditions the fixture has to meet (re-asserted by the tests)"""
    lengths = z["attention_mask"].sum(1)
    assert len(set(lengths.tolist())) >= 2 and (z["attention_mask"].shape[1] - lengths).max() >= 5
    for k in z:
        if k.startswith("g."):
            assert np.abs(z[k]).max() >= 1e-4, (k, np.abs(z[k]).max())
    assert float(z["fp32_loss_error"]) <= 1e-5


def run(model, px, ids, mask, labels, eps, reduction, grad=False):
    model.text_decoder.label_smoothing = eps
    with torch.no_grad():
        emb = model.vision_model(pixel_values=px).last_hidden_state
    with torch.set_grad_enabled(grad):
        return model.text_decoder(input_ids=ids, attention_mask=mask, encoder_hidden_states=emb, labels=labels,
                                  reduction=reduction)


def main():
    from transformers import BlipConfig, BlipForConditionalGeneration
    z = np.load(os.path.join(HERE, "blip_small.npz"), allow_pickle=False)
    cfg = json.loads(str(z["config"]))
    tc = cfg["text"]
    model = BlipForConditionalGeneration(BlipConfig(vision_config=dict(cfg["vision"]), text_config=dict(tc))).eval()
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}, strict=True)
    ids, mask, labels, prompt_row = inputs(z["sequences"], tc["sep_token_id"], tc["pad_token_id"])
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    px = torch.from_numpy(z["pixel_values"])
    res = dict(input_ids=ids, attention_mask=mask, labels=labels, prompt_row=np.int64(prompt_row),
               n_scored=(labels[:, 1:] != IGNORE).sum(1).astype(np.int64))
    err = 0.0
    m64 = model.double()
    out64 = {}
    for eps in EPS:
        mean = run(m64, px.double(), t(ids), t(mask), t(labels), eps, "mean")
        none = run(m64, px.double(), t(ids), t(mask), t(labels), eps, "none")
        out64[eps] = (mean.loss.item(), none.loss.numpy().copy())
        res[f"loss_mean.{eps:g}"], res[f"loss_none.{eps:g}"] = np.float64(mean.loss.item()), none.loss.numpy().copy()
        res["logits"] = mean.logits.numpy().astype(np.float32)
    # gradients for smoothing 0.1, mean reduction, in float64
    zero = []
    for p in m64.parameters():
        p.grad = None
    run(m64, px.double(), t(ids), t(mask), t(labels), 0.1, "mean", grad=True).loss.backward()
    for n, p in m64.named_parameters():  # (each tied tensor once, under its first name: mmfd's names)
        if n.startswith("text_decoder."):
            assert p.grad is not None, n
            if n.endswith(".key.bias"):
                assert p.grad.abs().max().item() < 1e-12, n
                zero.append(n)
                continue
            res["g." + n] = p.grad.numpy().astype(np.float32)
    res["zero_grads"] = np.array(zero)
    m32 = model.float()
    for eps in EPS:
        mean = run(m32, px, t(ids), t(mask), t(labels), eps, "mean")
        none = run(m32, px, t(ids), t(mask), t(labels), eps, "none")
        err = max(err, abs(mean.loss.item() - out64[eps][0]), np.abs(none.loss.double().numpy() - out64[eps][1]).max())
    res["fp32_loss_error"] = np.float64(err)
    check(res)
    path = os.path.join(HERE, "blip_small_loss.npz")
    np.savez_compressed(path, **res)
    print("lengths", mask.sum(1), "prompt row", prompt_row, "scored", res["n_scored"])
    for eps in EPS:
        print(f"eps {eps:g}: mean {out64[eps][0]:.6f}, sums {out64[eps][1]}")
    print(f"fp32 loss error {err:.2e}; smallest |g|max {min(np.abs(v).max() for k, v in res.items() if k.startswith('g.')):.2e}")
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
