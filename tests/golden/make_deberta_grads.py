"""Writes tests/golden/deberta_small_grads.npz: the parameter gradients of transformers'
DebertaV2Model on the weights and inputs of deberta_small.npz (make_golden.py gen_deberta_small:
hidden 64, 2 heads, 2 layers, vocab 1000, B=2, L=300, row 1 with 171 valid tokens).

  R        fp32 [2, 300, 64], randn from seed 23
  g.<name> the gradient of (last_hidden_state * R).sum() with respect to parameter <name>
           (eval mode, both dropout probabilities 0, fp32)

Run from the repository root: python tests/golden/make_deberta_grads.py
(needs the `transformers` package; the test suite only reads the .npz)."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    from transformers import DebertaV2Config, DebertaV2Model
    z = np.load(os.path.join(HERE, "deberta_small.npz"))
    cfg = DebertaV2Config(vocab_size=1000, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                          intermediate_size=128, max_position_embeddings=512, relative_attention=True,
                          position_buckets=256, norm_rel_ebd="layer_norm", share_att_key=True,
                          pos_att_type=["p2c", "c2p"], layer_norm_eps=1e-7, position_biased_input=False,
                          type_vocab_size=0, hidden_act="gelu", max_relative_positions=-1, pad_token_id=0,
                          hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = DebertaV2Model(cfg).float().eval()
    res = m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    R = torch.randn(2, 300, 64, generator=torch.Generator().manual_seed(23))
    out = m(input_ids=ids, attention_mask=mask).last_hidden_state
    assert (out.detach() - torch.from_numpy(z["last_hidden_state"])).abs().max().item() < 1e-5
    (out * R).sum().backward()
    res = {"R": R.numpy()}
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        res["g." + n] = p.grad.numpy()
    path = os.path.join(HERE, "deberta_small_grads.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
