"""Writes tests/golden/blip_small.npz: a tiny BlipForConditionalGeneration from transformers, run on the
CPU in fp32 (greedy generate with default arguments, and a teacher-forced pass over what it generated).

  vision  width 64, 2 layers, 2 heads, MLP 128, image 80, patch 8 (101 tokens), LayerNorm eps 1e-5
  text    vocab 200, width 96, 3 heads (D = 32), 2 layers, FFN 192, 32 positions, bos 198, sep / eos 2,
          pad 0, dropout 0, LayerNorm eps 1e-12
  4 images, N(0, 1) pixels on a 1/64 grid; every drawn weight on a 1/256 grid

Every non-LayerNorm tensor is drawn explicitly from one seeded generator (transformers' own init leaves
the tiny vision tower near 1e-9 and the captions independent of the image): vision matrices N(0, 0.1^2),
class / position embeddings 0.5, the text embedding tables 0.16, the other text matrices 0.08,
cross-attention matrices 0.15, vectors 0.02, and cls.predictions.bias[eos] += 2. (With every text matrix at
0.16 and cross-attention matrices at 0.4 the cross-attention scores over the 101 image tokens reach +-30:
2e-4 of fp32 noise in the logits, and a decoder so sharp that bf16 storage alone moves them by 0.8. The
milder decoder keeps the greedy margins, which the tied 0.16 embedding table sets, and needs the larger
eos bias for a row to stop early.) Seeds are searched from 0 until the four greedy rows are pairwise
distinct, one stops early after >= 3 generated tokens, one runs all 20, and the smallest top-1 / top-2
logit margin over the live (row, step) pairs is >= 0.05.

  w.<name>       the state_dict (keys: `keys`)
  pixel_values   fp32 [4, 3, 80, 80]        image_embeds  fp32 [4, 101, 64]
  sequences      int64 [4, 21] (bos first)  scores        fp32 [20, 4, 200] (generate's per-step scores)
  logits         float64 [20, 4, 200]: step t's logits with sequences[:, :t+1] forced, from the same model
                 and weights run in float64. transformers' own fp32 pass carries rounding noise of the
                 order of the 1e-5 a float64 restatement of the step is held to (fp32_error, measured
                 against this array; 3e-5 .. 8e-5 with a sharper decoder), so the array the restatement
                 and the kernels are compared with is the exact one; the fp32 pass is asserted to lie within 1e-4 of it and to
                 pick the same tokens.
  margin         the smallest live top-1 / top-2 margin of `scores`; seed: the seed kept; config: JSON

Run from the repository root: python tests/golden/make_blip_small.py
(needs the `transformers` package; the test suite only reads the .npz)."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VISION = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, image_size=80,
              patch_size=8, layer_norm_eps=1e-5)
TEXT = dict(vocab_size=200, hidden_size=96, num_attention_heads=3, num_hidden_layers=2, intermediate_size=192,
            max_position_embeddings=32, bos_token_id=198, sep_token_id=2, eos_token_id=2, pad_token_id=0,
            hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, encoder_hidden_size=64, layer_norm_eps=1e-12)
NEW = 20
EMBED_STD, TEXT_STD, CROSS_STD, EOS_BIAS = 0.16, 0.08, 0.15, 2.0


def grid(t, step=256.0):
    """values on a 1 / step grid (|k| <= 255: exact in bf16 too, and the committed file stays under 1 MiB)"""
    return torch.round(t * step).clamp(-255, 255) / step


def init(model, seed):
    g = torch.Generator().manual_seed(seed)
    eos = TEXT["eos_token_id"]
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "layer_norm" in n.lower() or "layernorm" in n.lower():
                p.copy_(torch.ones_like(p) if n.endswith("weight") else torch.zeros_like(p))
                continue
            if n.endswith("class_embedding") or n.endswith("position_embedding"):
                std = 0.5
            elif p.dim() < 2:
                std = 0.02
            elif n.startswith("vision_model"):
                std = 0.1
            elif "crossattention" in n:
                std = CROSS_STD
            elif "embeddings" in n:
                std = EMBED_STD
            else:
                std = TEXT_STD
            p.copy_(grid(torch.randn(p.shape, generator=g) * std))
        model.text_decoder.cls.predictions.bias[eos] += EOS_BIAS
    return g


def live_mask(seq, eos):
    """[NEW, B]: row b has not produced eos before step t"""
    B = seq.shape[0]
    live = np.ones((NEW, B), dtype=bool)
    for b in range(B):
        hit = np.nonzero(seq[b, 1:] == eos)[0]
        if hit.size:
            live[hit[0] + 1:, b] = False
    return live


def check(seq, scores, eos, pad):
    """the conditions the fixture has to meet (re-asserted by the tests): returns the live margin"""
    B = seq.shape[0]
    assert seq.shape == (B, NEW + 1), seq.shape
    assert len({tuple(r) for r in seq.tolist()}) == B, "rows not pairwise distinct"
    n_gen = [(int(np.nonzero(r[1:] == eos)[0][0]) + 1) if (r[1:] == eos).any() else NEW for r in seq]
    early = [n for r, n in zip(seq, n_gen) if (r[1:] == eos).any() and n < NEW]
    assert any(n >= 3 for n in early), f"no row stops early after >= 3 tokens: {n_gen}"
    assert any(not (r[1:] == eos).any() for r in seq), "no row runs all steps"
    live = live_mask(seq, eos)
    top2 = np.sort(scores, axis=-1)[..., -2:]
    margin = (top2[..., 1] - top2[..., 0])[live].min()
    assert margin >= 0.05, f"margin {margin}"
    return float(margin)


def forced_logits(model, px, seq):
    """(image_embeds, logits [NEW, B, V]) of the teacher-forced pass over seq[:, :NEW], in the model's dtype"""
    with torch.no_grad():
        emb = model.vision_model(pixel_values=px).last_hidden_state
        forced = torch.from_numpy(seq[:, :NEW])
        logits = model.text_decoder(input_ids=forced, encoder_hidden_states=emb,
                                    attention_mask=torch.ones_like(forced)).logits
    return emb, logits.permute(1, 0, 2).contiguous().numpy()


def main():
    from transformers import BlipConfig, BlipForConditionalGeneration
    cfg = BlipConfig(vision_config=dict(VISION), text_config=dict(TEXT))
    eos, pad = TEXT["eos_token_id"], TEXT["pad_token_id"]
    for seed in range(2000):
        model = BlipForConditionalGeneration(cfg).float().eval()
        g = init(model, seed)
        px = grid(torch.randn(4, 3, VISION["image_size"], VISION["image_size"], generator=g), 64.0)
        with torch.no_grad():
            out = model.generate(pixel_values=px, output_scores=True, return_dict_in_generate=True)
        seq = out.sequences.numpy()
        if seq.shape[1] < NEW + 1:  # every row stopped early: generate returns a shorter array
            continue
        scores = torch.stack(out.scores).numpy()
        try:
            margin = check(seq, scores, eos, pad)
            emb, logits32 = forced_logits(model, px, seq)
            _, logits = forced_logits(model.double(), px.double(), seq)
            model.float()
            live = live_mask(seq, eos)
            err = np.abs(logits32 - logits)[live].max()
            assert err <= 1e-4 and 4 * err <= margin, f"fp32 logits {err:.2e} from float64"
            assert (logits.argmax(-1).T[live.T] == seq[:, 1:][live.T]).all(), "float64 picks other tokens"
        except AssertionError as e:
            print(f"seed {seed}: {e}")
            continue
        break
    else:
        raise SystemExit("no seed meets the conditions: adjust the recipe")
    assert np.abs(logits - scores)[live].max() < 2e-4, np.abs(logits - scores)[live].max()
    sd = model.state_dict()
    res = {"w." + k: v.numpy() for k, v in sd.items()}
    res.update(keys=np.array(list(sd.keys())), pixel_values=px.numpy(), image_embeds=emb.numpy(), fp32_error=np.float64(err), sequences=seq,
               scores=scores, logits=logits, margin=np.float64(margin), seed=np.int64(seed),
               config=np.array(json.dumps(dict(vision=VISION, text=TEXT))))
    path = os.path.join(HERE, "blip_small.npz")
    np.savez_compressed(path, **res)
    print(f"seed {seed}: margin {margin:.4f}, |logit|max {np.abs(scores[live]).max():.2f}, fp32 error {err:.2e}")
    print(seq)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
