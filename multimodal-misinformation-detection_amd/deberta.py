"""DeBERTa-v3 text encoder on HIP kernels — the reference's default text encoder
(`AutoModel.from_pretrained("microsoft/deberta-v3-xsmall")`, train.py:330-331, called with
`.last_hidden_state` at train.py:136-140, preprocess_embeddings.py:63-80, evaluate.py:112-132).

HF parameter names (a hub / transformers state_dict loads unchanged) and HF's arithmetic
(transformers modeling_deberta_v2.py, restated in oracle/deberta.py): word embedding -> LayerNorm
-> times the mask; per layer the disentangled self-attention

    S = Q (K / sqrt(3 d))^T + c2p[i, clamp(rel(i,j) + 256)] / sqrt(3 d) + p2c[j, clamp(-rel(j,i) + 256)] / sqrt(3 d)

with c2p = Q_h . posK_h^T, p2c = K_h . posQ_h^T, posQ|posK = the layer's own Q/K projections of
LayerNorm(rel_embeddings) (share_att_key), rel = log-bucket relative positions (256 buckets,
max 512); padded keys masked with finfo.min; a fully padded query row averages V over all keys
(masked_fill + softmax semantics). Then the post-LN BERT block (out proj + residual + LN, GELU
FFN + residual + LN).

MI355X mapping: QKV is one packed GEMM; the position projections of all heads are one GEMM of the
512 relative embeddings against the same packed weight; c2p / p2c are per-head MFMA GEMMs
([B*L, d] x [d, 512]); one gather kernel turns them into the [B, H, L, L] fp32 additive bias the
flash-attention kernels consume (batch-strided rel_bias); padded-row fix-ups are two tiny kernels.

By default inference only (the reference freezes its encoders, train.py:335-340, and the
pre-embedding pass runs under no_grad): a forward that would need gradients raises. With
`DebertaV2Config(trainable=True)` a forward under grad runs as ONE autograd node (`_DebertaFn`, shaped
like encoders._BertFn) whose backward is `deberta_backward`: the post-LN layer backward BERT also runs
(blocks.post_ln_bwd) and the shared attention backward into a packed gradient (blocks.attn_bwd_packed), and
through the disentangled bias the attention backward's dS (mmfd_attn_args.d_rel_bias), its scatter
back to dc2p / dp2c (mmfd_deberta_rel_bias_bwd), four per-head GEMMs into dQ, dK and the position
projections' gradients, and the padded-row fix-up's adjoint (mmfd_attn_fill_masked_rows_bwd). Each
layer keeps its [B, H, L, L] fp32 bias for the backward (DESIGN f1).

Dropout (training mode of a trainable model, p = hidden_dropout_prob = attention_probs_dropout_prob > 0;
mmfd's config defaults are 0 / 0, HF's 0.1 / 0.1) sits at HF's five sites, drawn from the counter hash
all mmfd kernels share (site names "deberta.emb", "deberta.L<i>.pos | .attn | .attn_out | .ffn_out"; a
hidden site's mask index is the flat index of its contiguous tensor):
  embeddings    dropout(LayerNorm(word[id])) in the embedding kernel, then the mask (HF masks first;
                the two commute)
  positions     the layer's position projection reads dropout(LayerNorm(rel_embeddings)), one mask per
                layer (HF's pos_dropout inside every DisentangledSelfAttention)
  attention     dropout(P) inside the attention kernels; the backward takes dq / dk / dv from
                mmfd_attn_bwd and the bias gradient dS = P (M dP / (1 - p) - delta) from mmfd_attn_bwd_ds
  hidden        after the attention-output and the FFN-output projections (GEMM epilogues)
One probability serves all five, as in BertModel: a training forward with two different values raises.
The seed is device-resident (manual_seed; blocks.StepSeeded) and advances once per training forward.
Fully padded query rows keep the inference rule under dropout: their attention output is the mean of V
(mmfd_attn_fill_masked_rows) with NO attention dropout, their dO is zeroed before the attention backward
so their dS is 0, and hidden dropout applies to them like to any row. (HF drops their uniform
probabilities too; either way these rows are padding whose values no caller reads.)
With p = 0, in eval mode or under no_grad the model launches exactly the kernels it launched before
dropout existed; the p = 0 backward still takes dS from mmfd_attn_bwd's d_rel_bias.
"""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from . import blocks as Bk
from . import kernels as K
from .encoders import BERT_LAYER, EncoderOutput


@dataclass
class DebertaV2Config:
    """microsoft/deberta-v3-xsmall defaults (relative_attention, share_att_key, pos_att_type
    p2c|c2p, norm_rel_ebd layer_norm, position_biased_input False, type_vocab_size 0 are fixed)."""
    vocab_size: int = 128100
    hidden_size: int = 384
    num_hidden_layers: int = 12
    num_attention_heads: int = 6
    intermediate_size: int = 1536
    max_position_embeddings: int = 512
    position_buckets: int = 256
    max_relative_positions: int = -1
    layer_norm_eps: float = 1e-7
    pad_token_id: int = 0
    # fine-tuning (opt-in): with trainable=False the model is inference-only exactly as before
    trainable: bool = False
    hidden_dropout_prob: float = 0.0            # (HF default 0.1; training takes one value for both)
    attention_probs_dropout_prob: float = 0.0


def log_bucket_relative_positions(L: int, bucket_size: int, max_position: int) -> np.ndarray:
    """rel[i, j] = make_log_bucket_position(i - j, bucket_size, max_position) (modeling_deberta_v2.py:57-95),
    computed on the host in float64 like torch's float path, int64 [L, L]"""
    rel = (np.arange(L)[:, None] - np.arange(L)[None, :]).astype(np.int64)
    if bucket_size <= 0 or max_position <= 0:
        return rel
    mid = bucket_size // 2
    sign = np.sign(rel)
    abs_pos = np.where((rel < mid) & (rel > -mid), mid - 1, np.abs(rel)).astype(np.float32)
    log_pos = np.ceil(np.log(abs_pos / np.float32(mid)) / np.log(np.float32((max_position - 1) / mid))
                      * np.float32(mid - 1)).astype(np.float32) + mid
    return np.where(abs_pos <= mid, rel.astype(np.float32), log_pos * sign).astype(np.int64)


_IDX = {}


def _bias_indices(L, S, max_position, device):
    """int32 [L, L] c2p and p2c gather indices: clamp(rel + S) and clamp(-rel + S) (:323, :339)"""
    key = (L, S, max_position, str(device))
    t = _IDX.get(key)
    if t is None:
        rel = log_bucket_relative_positions(L, S, max_position)
        c2p = np.clip(rel + S, 0, 2 * S - 1).astype(np.int32)
        p2c = np.clip(-rel + S, 0, 2 * S - 1).astype(np.int32)
        t = _IDX[key] = (torch.from_numpy(c2p).to(device), torch.from_numpy(p2c).to(device))
        # the backward's run-sum kernel needs monotone index rows: checked here once per cached pair,
        # on the host copies (raises otherwise), so a captured training step finds the pair verified
        K.verify_rel_indices(*t, host=(c2p, p2c))
    return t


class DebertaV2Model(Bk.CachedWeights, Bk.StepSeeded, nn.Module):
    def __init__(self, config: DebertaV2Config | None = None, **kw):
        super().__init__()
        c = config or DebertaV2Config(**kw)
        self.config = c
        D, I = c.hidden_size, c.intermediate_size
        self.embeddings = nn.Module()
        self.embeddings.word_embeddings = nn.Embedding(c.vocab_size, D, padding_idx=c.pad_token_id)
        self.embeddings.LayerNorm = nn.LayerNorm(D, eps=c.layer_norm_eps)
        self.encoder = nn.Module()
        self.encoder.layer = nn.ModuleList()
        for _ in range(c.num_hidden_layers):
            L = nn.Module()
            L.attention = nn.Module()
            L.attention.self = nn.Module()
            for n in ("query_proj", "key_proj", "value_proj"):
                setattr(L.attention.self, n, nn.Linear(D, D))
            L.attention.output = nn.Module()
            L.attention.output.dense = nn.Linear(D, D)
            L.attention.output.LayerNorm = nn.LayerNorm(D, eps=c.layer_norm_eps)
            L.intermediate = nn.Module()
            L.intermediate.dense = nn.Linear(D, I)
            L.output = nn.Module()
            L.output.dense = nn.Linear(I, D)
            L.output.LayerNorm = nn.LayerNorm(D, eps=c.layer_norm_eps)
            self.encoder.layer.append(L)
        self.encoder.rel_embeddings = nn.Embedding(2 * self.att_span, D)
        self.encoder.LayerNorm = nn.LayerNorm(D, eps=c.layer_norm_eps)
        self.compute_dtype = torch.float32
        self._zero_pos = {}
        self._init_weights()

    @property
    def att_span(self):
        c = self.config
        mrp = c.max_relative_positions if c.max_relative_positions > 0 else c.max_position_embeddings
        return c.position_buckets if c.position_buckets > 0 else mrp

    @property
    def max_relative_positions(self):
        c = self.config
        return c.max_relative_positions if c.max_relative_positions > 0 else c.max_position_embeddings

    def _init_weights(self, std=0.02):
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.normal_(m.weight, 0.0, std)
                if isinstance(m, nn.Linear) and m.bias is not None:
                    nn.init.zeros_(m.bias)
                if isinstance(m, nn.Embedding) and m.padding_idx is not None:
                    with torch.no_grad():
                        m.weight[m.padding_idx].zero_()
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def set_precision(self, precision):
        self.compute_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[precision]
        return self

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, **unused):
        params = dict(self.named_parameters())
        first = next(iter(params.values()))
        if not first.is_cuda:
            raise RuntimeError("mmfd DebertaV2Model runs on the HIP device: call .to('cuda') first")
        c = self.config
        keep = torch.is_grad_enabled() and any(p.requires_grad for p in params.values())
        if keep and not c.trainable:
            raise NotImplementedError("mmfd DebertaV2Model is inference-only (frozen encoder, train.py:335-340): "
                                      "call it under torch.no_grad() or freeze its parameters, or build it with "
                                      "DebertaV2Config(trainable=True)")
        if c.trainable and self.training and c.hidden_dropout_prob != c.attention_probs_dropout_prob:
            raise NotImplementedError("mmfd DebertaV2Model uses one dropout probability for hidden and attention "
                                      "dropout: set hidden_dropout_prob = attention_probs_dropout_prob")
        if keep:
            out = _DebertaFn.apply(self, list(params.keys()), input_ids, attention_mask, *params.values())
            return EncoderOutput(last_hidden_state=out)
        P = {n: p.detach() for n, p in params.items()}
        ctx = Bk.StepCtx(P, self.compute_dtype, shadows=Bk.shadow_store(self))
        # frozen encoder: packed QKV biases persist across calls (not for a trainable model: mmfd's
        # AdamW moves its parameters without bumping their version counters, see StepCtx.derived)
        ctx.cache_derived = not c.trainable
        out = deberta_forward(self, ctx, input_ids, attention_mask)
        return EncoderOutput(last_hidden_state=out)


DEBERTA_QKV = (".attention.self.query_proj", ".attention.self.key_proj", ".attention.self.value_proj")


# x: layer input; qkv [B, L, 3D]; pos [2S, 3D]: position projections; rb [B, H, L, L] fp32: disentangled bias;
# relE [2S, D]: what the position projection read (the layer's dropped copy under dropout); akw: attn_fwd's
# dropout keywords
DebertaLayerState = namedtuple("DebertaLayerState", "x qkv pos rb lse post relE akw")


def deberta_forward(model: DebertaV2Model, ctx: Bk.StepCtx, input_ids, attention_mask, st=None, site="deberta"):
    """`st` (a dict, training): filled with what deberta_backward reads; the kernels and their order
    are the same either way, so the outputs are too. With ctx.p > 0 (a training-mode forward of a
    trainable model) the five dropout sites of the module docstring are on."""
    cfg = model.config
    keep = st is not None
    dev = ctx.P["embeddings.word_embeddings.weight"].device
    ids = input_ids.to(dev).long().contiguous()
    B, L = ids.shape
    mask = (attention_mask.to(dev).long().contiguous() if attention_mask is not None else torch.ones_like(ids))
    D, H = cfg.hidden_size, cfg.num_attention_heads
    d = D // H
    S = model.att_span
    eps = cfg.layer_norm_eps
    dt = ctx.dt
    # embeddings: LN(word[id]) * mask (no absolute positions, no token types)
    zp = model._zero_pos.get((L, str(dev)))
    if zp is None:
        zp = model._zero_pos[(L, str(dev))] = torch.zeros(L, D, device=dev, dtype=torch.float32)
    emb_drop = ctx.drop(site + ".emb")
    if keep:
        s0, x, m0, r0 = K.embed_ln_train(ids, None, ctx.P["embeddings.word_embeddings.weight"], zp,
                                         ctx.P["embeddings.LayerNorm.weight"], ctx.P["embeddings.LayerNorm.bias"],
                                         eps, dt, **emb_drop)
    else:
        x = K.embed_ln_infer(ids, None, ctx.P["embeddings.word_embeddings.weight"], zp,
                             ctx.P["embeddings.LayerNorm.weight"], ctx.P["embeddings.LayerNorm.bias"], eps, dt)
    K.mask_rows(x, mask)
    key_bias = K.mask_to_bias(mask)
    c2p_idx, p2c_idx = _bias_indices(L, S, model.max_relative_positions, dev)
    rel = ctx.P["encoder.rel_embeddings.weight"][: 2 * S]
    rel_in = K.cast(rel, dt) if dt != torch.float32 else rel.contiguous()
    relE, mr, rr = K.layernorm_fwd(rel_in, ctx.P["encoder.LayerNorm.weight"], ctx.P["encoder.LayerNorm.bias"], eps)
    scale = 1.0 / math.sqrt(d * 3)
    c2p = torch.empty((H, B * L, 2 * S), device=dev, dtype=dt)
    p2c = torch.empty((H, B * L, 2 * S), device=dev, dtype=dt)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layer.{i}"
        s = f"{site}.L{i}"
        names = [p + n for n in DEBERTA_QKV]
        qkv = Bk.linear_packed(ctx, x, names)                # [B*L, 3D]
        pdrop = ctx.drop(s + ".pos")                         # HF pos_dropout: a mask per layer on the one table
        relE_i = K.dropout(relE, pdrop["dropout_p"], pdrop["seed"], pdrop["salt"]) if pdrop else relE
        pos = Bk.linear_packed(ctx, relE_i, names)           # [2S, 3D]: posQ | posK | (unused V)
        for h in range(H):
            qh, kh = qkv[:, h * d:(h + 1) * d], qkv[:, D + h * d:D + (h + 1) * d]
            pqh, pkh = pos[:, h * d:(h + 1) * d], pos[:, D + h * d:D + (h + 1) * d]
            K.gemm(qh, pkh, out=c2p[h])                      # c2p = Q_h posK_h^T  [B*L, 2S]
            K.gemm(kh, pqh, out=p2c[h])                      # p2c = K_h posQ_h^T
        rb = K.deberta_rel_bias(c2p, p2c, c2p_idx, p2c_idx, B, L, scale)
        q3 = qkv.view(B, L, 3 * D)
        akw = ctx.attn_drop(s + ".attn", q3[..., :D], q3[..., D:2 * D], H)
        o, lse = K.attn_fwd(q3[..., :D], q3[..., D:2 * D], q3[..., 2 * D:], H, scale=scale, key_bias=key_bias,
                            rel_bias=rb, **akw)
        K.attn_fill_masked_rows(q3[..., 2 * D:], o, H, mask)  # (padded query rows: mean of V, no dropout)
        x_out, _, post = Bk.post_ln_fwd(ctx, x, o, p, BERT_LAYER, eps, keep=keep, planes=False,
                                        sites=(s + ".attn_out", s + ".ffn_out") if ctx.p > 0 else (None, None))
        if keep:
            st["layers"].append(DebertaLayerState(x, q3, pos, rb, lse, post, relE_i, akw))
        x = x_out
    if keep:
        st.update(ids=ids, mask=mask, key_bias=key_bias, idx=(c2p_idx, p2c_idx), s0=s0, m0=m0, r0=r0, rel_in=rel_in,
                  mr=mr, rr=rr, scale=scale, bufs=(c2p, p2c), emb_drop=emb_drop, site=site)
    return x.view(B, L, D)


def deberta_backward(model: DebertaV2Model, ctx: Bk.StepCtx, dout, st):
    """Gradients of every parameter into ctx.grads, layers in reverse. Per layer: blocks.post_ln_bwd
    (FFN, both LayerNorms, output projection), then through the attention
        S = scale Q K^T + key_bias + inv (c2p[i, c2p_idx[i, j]] + p2c[j, p2c_idx[j, i]])
    with c2p = Q_h posK_h^T, p2c = K_h posQ_h^T: attn_bwd also emits dS (without dropout; under dropout
    attn_bwd keeps its delta and attn_bwd_ds follows with the forward's mask), its scatter gives
    dc2p / dp2c, and per head dQ_h += dc2p_h posK_h, dK_h += dp2c_h posQ_h, dposK_h =
    dc2p_h^T Q_h, dposQ_h = dp2c_h^T K_h. The packed Q|K|V weights collect two gradients: the token
    stream (dqkv, x) and the position stream (dpos = dposQ | dposK, the layer's — under dropout
    dropped — LayerNorm(rel_embeddings)); the relative embeddings collect dpos W over all layers (fp32
    accumulator; under dropout each layer's term passes its position mask in the GEMM epilogue:
    drelE += M_i (dpos W) / (1 - p))."""
    cfg = model.config
    ids, mask = st["ids"], st["mask"]
    B, L = ids.shape
    D, H = cfg.hidden_size, cfg.num_attention_heads
    d = D // H
    S2 = 2 * model.att_span
    dt, scale = ctx.dt, st["scale"]
    c2p_idx, p2c_idx = st["idx"]
    dev = dout.device
    dx = Bk.as2d(dout).contiguous()
    dsb = torch.empty((B, H, L, L), device=dev, dtype=torch.float32)  # dS of one layer at a time
    dc2p, dp2c = st["bufs"]                     # the forward's c2p / p2c buffers, free by now
    drelE = torch.empty((S2, D), device=dev, dtype=torch.float32)
    delta = torch.empty((B, H, L), device=dev, dtype=torch.float32) if ctx.p > 0 else None  # attn_bwd -> attn_bwd_ds
    for i in reversed(range(cfg.num_hidden_layers)):
        ls = st["layers"][i]
        st["layers"][i] = None
        qkv, pos = Bk.as2d(ls.qkv), ls.pos
        do, ds1 = Bk.post_ln_bwd(ctx, dx, ls.post)
        # padded query rows: their dO goes to dV of every key (mean of V in the forward), not into the attention
        gsum = K.attn_fill_masked_rows_bwd(do, H, mask)
        if ctx.p > 0:  # mmfd_attn_bwd refuses d_rel_bias with dropout: dS from its own entry, on the delta kept here
            dqkv, _, _ = Bk.attn_bwd_packed(ctx, ls.qkv, ls.post.o, ls.lse, do, H, planes=False, scale=scale,
                                            key_bias=st["key_bias"], rel_bias=ls.rb, delta=delta, **ls.akw)
            K.attn_bwd_ds(ls.qkv[..., :D], ls.qkv[..., D:2 * D], ls.qkv[..., 2 * D:], ls.lse, do, H, delta,
                          rel_bias=ls.rb, key_bias=st["key_bias"], scale=scale, out=dsb, **ls.akw)
        else:
            dqkv, _, _ = Bk.attn_bwd_packed(ctx, ls.qkv, ls.post.o, ls.lse, do, H, planes=False, scale=scale,
                                            key_bias=st["key_bias"], rel_bias=ls.rb, d_rel_bias=dsb)
        K.attn_fill_masked_rows_bwd(do, H, mask, dv=dqkv.view(B, L, 3 * D)[..., 2 * D:], gsum=gsum)
        K.deberta_rel_bias_bwd(dsb, c2p_idx, p2c_idx, B, L, scale, S2, dt, dc2p=dc2p, dp2c=dp2c)
        dpos = torch.empty((S2, 2 * D), device=dev, dtype=dt)  # dposQ | dposK (the V third of pos is unused)
        for h in range(H):
            hq, hk = slice(h * d, (h + 1) * d), slice(D + h * d, D + (h + 1) * d)
            K.gemm(dc2p[h], pos[:, hk], trans_b=True, out=dqkv[:, hq], beta=1.0)   # dQ_h += dc2p_h posK_h
            K.gemm(dp2c[h], pos[:, hq], trans_b=True, out=dqkv[:, hk], beta=1.0)   # dK_h += dp2c_h posQ_h
            K.gemm(dc2p[h], qkv[:, hq], trans_a=True, trans_b=True, out=dpos[:, hk])  # dposK_h = dc2p_h^T Q_h
            K.gemm(dp2c[h], qkv[:, hk], trans_a=True, trans_b=True, out=dpos[:, hq])  # dposQ_h = dp2c_h^T K_h
        names = [f"encoder.layer.{i}" + n for n in DEBERTA_QKV]
        # (as blocks.self_attn_bwd, with the position stream's GEMMs between the weight and data gradients)
        ctx.lin_grads(names, dqkv, ls.x)                # token stream (one packed GEMM)
        ctx.lin_grads(names[:2], dpos, ls.relE)         # position stream: accumulates onto the Q and K blocks
        Wp, _ = ctx.w_packed(names)
        K.gemm(dpos, Wp[:2 * D], trans_b=True, out=drelE, beta=0.0 if i == cfg.num_hidden_layers - 1 else 1.0,
               **ctx.drop(f"{st['site']}.L{i}.pos"))
        dx = Bk.linear_dx(ctx, dqkv, Wp, residual=ds1)  # dx_in = ds1 + dQKV [Wq;Wk;Wv]
        ctx.flush_ready()
    # relative embeddings: LayerNorm backward of the summed position gradient
    drel, _ = Bk.layernorm_bwd(ctx, drelE if dt == torch.float32 else K.cast(drelE, dt), st["rel_in"],
                               "encoder.LayerNorm", st["mr"], st["rr"])
    grel = K.zeros(ctx.P["encoder.rel_embeddings.weight"].shape, device=dev)  # rows past 2S (none by default): 0
    K.cast(drel, torch.float32, out=grel[:S2])
    ctx.grads["encoder.rel_embeddings.weight"] = grel
    # embeddings: x = dropout(LayerNorm(word[id])) * mask
    K.mask_rows(dx, mask)
    if st["emb_drop"]:
        dx = K.dropout(dx, st["emb_drop"]["dropout_p"], st["emb_drop"]["seed"], st["emb_drop"]["salt"])
    dsum, _ = Bk.layernorm_bwd(ctx, dx, st["s0"], "embeddings.LayerNorm", st["m0"], st["r0"])
    dword = K.zeros(ctx.P["embeddings.word_embeddings.weight"].shape, device=dev)
    K.embed_bwd(ids, None, dsum, dword, None, None, padding_idx=cfg.pad_token_id)
    ctx.grads["embeddings.word_embeddings.weight"] = dword
    ctx.flush_ready()


class _DebertaFn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, model, names, input_ids, attention_mask, *params):
        cfg = model.config
        p = cfg.hidden_dropout_prob if model.training else 0.0  # (== attention_probs_dropout_prob: forward() checked)
        dev = params[0].device
        sc = Bk.module_ctx(model, names, params, p, model._fork_seed(dev) if p > 0 else None)
        st = {"layers": []}
        out = deberta_forward(model, sc, input_ids, attention_mask, st=st)
        fctx.sc, fctx.st, fctx.model, fctx.names = sc, st, model, names
        return out

    @staticmethod
    def backward(fctx, dout):
        grads = Bk.fn_backward(fctx, dout, lambda sc, d: deberta_backward(fctx.model, sc, d, fctx.st))
        return (None, None, None, None, *grads)
