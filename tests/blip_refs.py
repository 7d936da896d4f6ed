"""float64 restatement (torch, CPU) of what mmfd.blip runs: BLIP's vision tower, and the text decoder as
ONE token per step against a self-attention K|V cache and the per-image cross-attention K|V, plus the
greedy select rule. tests/test_blip_ref_cpu.py holds it to transformers' own outputs
(tests/golden/blip_small.npz), so the GPU tests can compare the kernels with it on any input without
transformers on the GPU machine."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = "text_decoder.bert."
HEAD = "text_decoder.cls.predictions."


def load_fixture():
    z = np.load(os.path.join(G, "blip_small.npz"), allow_pickle=False)
    cfg = json.loads(str(z["config"]))
    W = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}
    return z, cfg, W


def load_model(cfg, W, precision="fp32", device="cuda"):
    """mmfd's BlipForConditionalGeneration with the fixture's weights, frozen, on `device` in `precision`"""
    from mmfd.blip import BlipConfig, BlipForConditionalGeneration
    m = BlipForConditionalGeneration(BlipConfig(vision=cfg["vision"], text=cfg["text"]))
    res = m.load_state_dict(W, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for p in m.parameters():
        p.requires_grad_(False)
    return m.to(device).eval().set_precision(precision)


def live_mask(seq, eos):
    """[steps, B] bool: row b has not produced eos before step t (seq [B, 1 + steps], bos first)"""
    seq = np.asarray(seq)
    B, n = seq.shape[0], seq.shape[1] - 1
    live = np.ones((n, B), dtype=bool)
    for b in range(B):
        hit = np.nonzero(seq[b, 1:] == eos)[0]
        if hit.size:
            live[hit[0] + 1:, b] = False
    return live


def _lin(W, name, x):
    return x @ W[name + ".weight"].double().t() + W[name + ".bias"].double()


def _ln(W, name, x, eps):
    return F.layer_norm(x, (x.shape[-1],), W[name + ".weight"].double(), W[name + ".bias"].double(), eps)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _heads(x, H):
    return x.view(*x.shape[:-1], H, x.shape[-1] // H)


def vision(W, cfg, px):
    """image_embeds [B, 1 + patches, width] (float64)"""
    vc = cfg["vision"]
    D, H, P, eps = vc["hidden_size"], vc["num_attention_heads"], vc["patch_size"], vc["layer_norm_eps"]
    px = px.double()
    B = px.shape[0]
    w = W["vision_model.embeddings.patch_embedding.weight"].double()
    x = F.conv2d(px, w, W["vision_model.embeddings.patch_embedding.bias"].double(), stride=P).flatten(2).transpose(1, 2)
    x = torch.cat([W["vision_model.embeddings.class_embedding"].double().expand(B, 1, D), x], 1)
    x = x + W["vision_model.embeddings.position_embedding"].double()
    for i in range(vc["num_hidden_layers"]):
        p = f"vision_model.encoder.layers.{i}"
        h = _ln(W, p + ".layer_norm1", x, eps)
        q, k, v = (_heads(t, H).transpose(1, 2) for t in _lin(W, p + ".self_attn.qkv", h).split(D, dim=-1))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // H), -1) @ v
        x = x + _lin(W, p + ".self_attn.projection", a.transpose(1, 2).reshape(B, -1, D))
        h = _ln(W, p + ".layer_norm2", x, eps)
        x = x + _lin(W, p + ".mlp.fc2", _gelu(_lin(W, p + ".mlp.fc1", h)))
    return _ln(W, "vision_model.post_layernorm", x, eps)


def attend(q, k, v, H):
    """one query per row: q [B, E], k / v [B, L, E] -> [B, E]"""
    B, E = q.shape
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)           # [B, H, d], [B, L, H, d]
    s = torch.einsum("bhd,blhd->bhl", qh, kh) / math.sqrt(E // H)
    return torch.einsum("bhl,blhd->bhd", torch.softmax(s, -1), vh).reshape(B, E)


class Decoder:
    """the single-token text decoder with its caches: step(tokens [B]) -> logits [B, V] (float64)"""

    def __init__(self, W, cfg, image_embeds):
        self.W, self.tc = W, cfg["text"]
        self.L = self.tc["num_hidden_layers"]
        emb = image_embeds.double()
        self.cross = [(_lin(W, f"{T}encoder.layer.{i}.crossattention.self.key", emb),
                       _lin(W, f"{T}encoder.layer.{i}.crossattention.self.value", emb)) for i in range(self.L)]
        self.k = [[] for _ in range(self.L)]
        self.v = [[] for _ in range(self.L)]
        self.t = 0

    def step(self, tokens):
        W, tc = self.W, self.tc
        H, eps = tc["num_attention_heads"], tc["layer_norm_eps"]
        x = W[T + "embeddings.word_embeddings.weight"].double()[tokens] \
            + W[T + "embeddings.position_embeddings.weight"].double()[self.t]
        x = _ln(W, T + "embeddings.LayerNorm", x, eps)
        for i in range(self.L):
            p = f"{T}encoder.layer.{i}"
            self.k[i].append(_lin(W, p + ".attention.self.key", x))
            self.v[i].append(_lin(W, p + ".attention.self.value", x))
            a = attend(_lin(W, p + ".attention.self.query", x), torch.stack(self.k[i], 1), torch.stack(self.v[i], 1), H)
            x = _ln(W, p + ".attention.output.LayerNorm", x + _lin(W, p + ".attention.output.dense", a), eps)
            a = attend(_lin(W, p + ".crossattention.self.query", x), *self.cross[i], H)
            x = _ln(W, p + ".crossattention.output.LayerNorm", x + _lin(W, p + ".crossattention.output.dense", a), eps)
            f = _lin(W, p + ".output.dense", _gelu(_lin(W, p + ".intermediate.dense", x)))
            x = _ln(W, p + ".output.LayerNorm", x + f, eps)
        self.t += 1
        g = _ln(W, HEAD + "transform.LayerNorm", _gelu(_lin(W, HEAD + "transform.dense", x)), eps)
        return g @ W[T + "embeddings.word_embeddings.weight"].double().t() + W[HEAD + "bias"].double()


def select(argmax, finished, eos, pad, forced=None):
    """the greedy rule of one step: (tokens [B], finished [B]); `finished` is the state before the step"""
    tok = torch.where(finished, torch.full_like(argmax, pad), argmax) if forced is None else forced.clone()
    return tok, finished | (tok == eos)


def forced_logits(W, cfg, image_embeds, ids):
    """[T, B, V]: step t's logits with ids[:, :t + 1] forced"""
    dec = Decoder(W, cfg, image_embeds)
    return torch.stack([dec.step(ids[:, t]) for t in range(ids.shape[1])])


def greedy(W, cfg, image_embeds, max_new_tokens=20, prompt=None):
    """transformers' greedy generate: [B, P + n] ids, bos first, stopping once every row has finished"""
    tc = cfg["text"]
    B = image_embeds.shape[0]
    prompt = [tc["bos_token_id"]] if prompt is None else [tc["bos_token_id"], *prompt[1:]]
    dec = Decoder(W, cfg, image_embeds)
    seq = [torch.full((B,), prompt[0], dtype=torch.long)]
    fin = torch.zeros(B, dtype=torch.bool)
    for t in range(len(prompt) - 1 + max_new_tokens):
        logits = dec.step(seq[-1])
        forced = torch.full((B,), prompt[t + 1], dtype=torch.long) if t + 1 < len(prompt) else None
        tok, fin = select(logits.argmax(-1), fin, tc["sep_token_id"], tc["pad_token_id"], forced)
        seq.append(tok)
        if forced is None and bool(fin.all()):
            break
    return torch.stack(seq, 1)
