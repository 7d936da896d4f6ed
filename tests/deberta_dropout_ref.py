"""TEST INFRASTRUCTURE ONLY. The DeBERTa-v3 forward of oracle/deberta.py restated in float64 torch with a
`drop(site, x)` hook at the five places where transformers' DebertaV2Model has an nn.Dropout:

    <site>.emb            DebertaV2Embeddings.dropout: on LayerNorm(word[id]) (transformers masks first and
                          drops second; the mask is a 0 / 1 factor per row, so the two commute)
    <site>.L<i>.pos       DisentangledSelfAttention.pos_dropout: on the LayerNorm'd [2S, D] relative
                          embeddings, a fresh mask in every layer
    <site>.L<i>.attn      DisentangledSelfAttention.dropout: on the attention probabilities [B, H, L, L]
    <site>.L<i>.attn_out  DebertaV2SelfOutput.dropout: on the attention-output projection [B, L, D]
    <site>.L<i>.ffn_out   DebertaV2Output.dropout: on the FFN-output projection [B, L, D]

With `drop = oracle.dropout_hash.Drop(seed, p)` these are exactly the masks the HIP kernels draw (sites
ending in ".attn" with the pair hash, every other site by the flat index of its contiguous tensor).

Fully padded query rows (attention_mask[b, i] == 0) follow mmfd's rule, not transformers': their
attention output is the mean of V over all keys — the softmax of an all-masked row — WITHOUT attention
dropout; hidden dropout applies to them like to any row. No real-token row reads a padded row (padded keys
are masked, everything else is per row), so real-token outputs and the gradients of a loss over real-token
rows do not depend on the rule: tests/test_deberta_dropout_ref_cpu.py compares those with transformers.
With drop=None this is oracle.deberta.deberta_forward in the dtype of P."""
import math

import torch
import torch.nn.functional as F

from oracle.deberta import log_bucket_relative_positions

SITE = "deberta"


def sites(num_layers, site=SITE):
    """every dropout site of a model with `num_layers` layers, in forward order"""
    out = [site + ".emb"]
    for i in range(num_layers):
        out += [f"{site}.L{i}.{n}" for n in ("pos", "attn", "attn_out", "ffn_out")]
    return out


def _lin(P, name, x):
    return F.linear(x, P[name + ".weight"], P[name + ".bias"])


def deberta_forward_drop(P, input_ids, attention_mask=None, *, num_layers, num_heads, position_buckets=256,
                         max_position_embeddings=512, eps=1e-7, drop=None, site=SITE, score_scale=None):
    """last_hidden_state [B, L, D] in the dtype of P (float64 for a reference). `score_scale`: the divisor
    sqrt(3 d) of the scores when the caller needs another rounding of it than float64's (transformers
    computes it in float32 whatever the model's dtype, which alone moves a float64 output by 4e-10)"""
    drop = drop or (lambda s, x: x)
    B, L = input_ids.shape
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    w = P["embeddings.word_embeddings.weight"]
    m = attention_mask.to(w.dtype)
    x = F.embedding(input_ids, w)
    D = x.shape[-1]
    x = F.layer_norm(x, (D,), P["embeddings.LayerNorm.weight"], P["embeddings.LayerNorm.bias"], eps)
    x = drop(site + ".emb", x) * m[:, :, None]
    live = attention_mask.bool()
    amask = live[:, None, :, None] & live[:, None, None, :]  # [B, 1, L, L] = mask[i] * mask[j]
    S = position_buckets if position_buckets > 0 else max_position_embeddings
    rel = torch.from_numpy(log_bucket_relative_positions(L, position_buckets, max_position_embeddings))
    c2p_pos = torch.clamp(rel + S, 0, 2 * S - 1)
    p2c_pos = torch.clamp(-rel + S, 0, 2 * S - 1)
    relE = P["encoder.rel_embeddings.weight"][: 2 * S]
    relE = F.layer_norm(relE, (D,), P["encoder.LayerNorm.weight"], P["encoder.LayerNorm.bias"], eps)
    H = num_heads
    d = D // H
    scale = math.sqrt(d * 3) if score_scale is None else float(score_scale)

    def heads(t):  # [B, L, D] -> [B, H, L, d]
        return t.view(t.shape[0], t.shape[1], H, d).permute(0, 2, 1, 3)

    for i in range(num_layers):
        p = f"encoder.layer.{i}"
        s = f"{site}.L{i}"
        a = p + ".attention.self"
        q = heads(_lin(P, a + ".query_proj", x))
        k = heads(_lin(P, a + ".key_proj", x))
        v = heads(_lin(P, a + ".value_proj", x))
        rel_i = drop(s + ".pos", relE)
        pq = _lin(P, a + ".query_proj", rel_i).view(2 * S, H, d).permute(1, 0, 2)  # [H, 2S, d]
        pk = _lin(P, a + ".key_proj", rel_i).view(2 * S, H, d).permute(1, 0, 2)
        scores = q @ (k / scale).transpose(-1, -2)
        c2p = q @ pk.transpose(-1, -2)                                      # [B, H, L, 2S]
        c2p = torch.gather(c2p, -1, c2p_pos.expand(B, H, L, L))
        p2c = k @ pq.transpose(-1, -2)                                      # [B, H, L(key), 2S]
        p2c = torch.gather(p2c, -1, p2c_pos.expand(B, H, L, L)).transpose(-1, -2)
        scores = scores + (c2p / scale + p2c / scale)
        scores = scores.masked_fill(~amask, torch.finfo(torch.float32).min)
        probs = torch.softmax(scores, -1)
        # the padded-row rule: a fully padded query row keeps its uniform probabilities, undropped
        probs = torch.where(live[:, None, :, None], drop(s + ".attn", probs), probs)
        ctx = (probs @ v).permute(0, 2, 1, 3).reshape(B, L, D)
        o = drop(s + ".attn_out", _lin(P, p + ".attention.output.dense", ctx))
        x = F.layer_norm(o + x, (D,), P[p + ".attention.output.LayerNorm.weight"],
                         P[p + ".attention.output.LayerNorm.bias"], eps)
        f = F.gelu(_lin(P, p + ".intermediate.dense", x))
        o = drop(s + ".ffn_out", _lin(P, p + ".output.dense", f))
        x = F.layer_norm(o + x, (D,), P[p + ".output.LayerNorm.weight"], P[p + ".output.LayerNorm.bias"], eps)
    return x


def reference_grads(state_dict, ids, mask, R, *, num_layers, num_heads, eps, drop=None, site=SITE):
    """(last_hidden_state, {name: gradient of (last_hidden_state * R).sum()}) in float64"""
    P = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in state_dict.items()}
    out = deberta_forward_drop(P, ids, mask, num_layers=num_layers, num_heads=num_heads, eps=eps, drop=drop, site=site)
    (out * R.double()).sum().backward()
    return out.detach(), {k: v.grad for k, v in P.items()}
