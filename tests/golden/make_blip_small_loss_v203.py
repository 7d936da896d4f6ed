"""Writes tests/golden/blip_small_loss_v203.npz: the caption loss of make_blip_small_loss.py for a vocabulary that
is no multiple of 8. The model is blip_small.npz's with three more vocabulary rows (203 = 25 * 8 + 3), so that the
rows of a dense [R, V] matrix are not 16-byte aligned in bf16 or fp32; transformers on the CPU in float64.

  extra_word      float32 [3, 96], extra_bias float32 [3]: rows 200..202 of the tied table and of the LM-head bias
  input_ids, attention_mask, labels, n_scored: as blip_small_loss.npz, but that token 201 (a new row) stands at
                  row 0, position 4, in the ids and in the labels: a label in the last, partial 8-column chunk
  loss_mean.0.1   float64 scalar, loss_none.0.1 float64 [4]; logits_absmax float64 (the largest |logit|)
  g.<name>        float32: for smoothing 0.1, the float64 gradient of the mean loss with respect to the parameters
                  around the LM head and one deep in the stack (SELECT): the tied table, the LM-head bias, the head
                  transform, the embeddings' position table and LayerNorm, and layer 0's self-attention query.
                  dlogits reaches every one of them through the two LM-head products.

Asserted here and again by the tests: every stored gradient has |g|max >= 1e-4.

Run from the repository root: python tests/golden/make_blip_small_loss_v203.py
(needs the `transformers` package; the test suite only reads the .npz)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_blip_small_loss import IGNORE, inputs, run  # noqa: E402

V_NEW, NEW_TOKEN, ROW, POS = 203, 201, 0, 4
WORD = "text_decoder.bert.embeddings.word_embeddings.weight"
BIAS = "text_decoder.cls.predictions.bias"
SELECT = ("text_decoder.bert.embeddings.", "text_decoder.cls.predictions.",
          "text_decoder.bert.encoder.layer.0.attention.self.query.")


def main():
    from transformers import BlipConfig, BlipForConditionalGeneration
    z = np.load(os.path.join(HERE, "blip_small.npz"), allow_pickle=False)
    cfg = json.loads(str(z["config"]))
    tc = dict(cfg["text"], vocab_size=V_NEW)
    rng = np.random.default_rng(V_NEW)
    W = {k[2:]: z[k] for k in z.files if k.startswith("w.")}
    n_old = W[WORD].shape[0]
    extra_word = (rng.standard_normal((V_NEW - n_old, W[WORD].shape[1])) * W[WORD].std()).astype(np.float32)
    extra_bias = (rng.standard_normal(V_NEW - n_old) * 0.1).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in W.items()}
    for k in sd:  # the tied table and the bias, under each of their names
        if k.startswith("text_decoder.") and sd[k].shape[0] == n_old and ("word_embeddings" in k or "cls.predictions" in k):
            sd[k] = torch.cat([sd[k], torch.from_numpy(extra_word if sd[k].dim() == 2 else extra_bias)])
    model = BlipForConditionalGeneration(BlipConfig(vision_config=dict(cfg["vision"]), text_config=tc)).eval()
    model.load_state_dict(sd, strict=True)
    ids, mask, labels, prompt_row = inputs(z["sequences"], tc["sep_token_id"], tc["pad_token_id"])
    assert mask[ROW, POS] == 1 and labels[ROW, POS] != IGNORE
    ids[ROW, POS] = labels[ROW, POS] = NEW_TOKEN
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    px = torch.from_numpy(z["pixel_values"]).double()
    m64 = model.double()
    none = run(m64, px, t(ids), t(mask), t(labels), 0.1, "none")
    for p in m64.parameters():
        p.grad = None
    mean = run(m64, px, t(ids), t(mask), t(labels), 0.1, "mean", grad=True)
    mean.loss.backward()
    res = dict(extra_word=extra_word, extra_bias=extra_bias, input_ids=ids, attention_mask=mask, labels=labels,
               n_scored=(labels[:, 1:] != IGNORE).sum(1).astype(np.int64),
               logits_absmax=np.float64(mean.logits.detach().abs().max().item()))
    res["loss_mean.0.1"], res["loss_none.0.1"] = np.float64(mean.loss.item()), none.loss.numpy().copy()
    for n, p in m64.named_parameters():
        if n.startswith(SELECT):
            res["g." + n] = p.grad.numpy().astype(np.float32)
            assert np.abs(res["g." + n]).max() >= 1e-4, n
    assert res["g." + WORD].shape == (V_NEW, W[WORD].shape[1]) and res["g." + BIAS].shape == (V_NEW,)
    path = os.path.join(HERE, "blip_small_loss_v203.npz")
    np.savez_compressed(path, **res)
    print("mean", res["loss_mean.0.1"], "sums", res["loss_none.0.1"], "stored", sorted(k for k in res if k.startswith("g.")))
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
