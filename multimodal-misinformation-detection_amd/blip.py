"""BLIP image captioning on HIP kernels: the reference's captioning stage (src/preprocess/caption.py:22-31
and src/demo/app.py run `BlipForConditionalGeneration.from_pretrained("Salesforce/blip-image-captioning-
large").generate(**inputs)` over every claim and evidence image). Inference only.

`BlipForConditionalGeneration` keeps transformers' parameter names, so its `state_dict` loads with
`strict=True`; `generate` follows transformers' greedy default (20 new tokens, decoding from [bos], stop
at sep_token_id, pad afterwards) or, with num_beams > 1, its beam search (csrc/beam.hip; the last item below).

What runs where:
  * vision tower (pre-LN ViT, packed qkv): patchify + GEMM, class token + positions, then per layer
    LayerNorm -> qkv GEMM -> attn_fwd -> projection GEMM (+ residual) -> LayerNorm -> fc1 GELU -> fc2
    (+ residual), and post_layernorm: the encoders' kernels (mmfd.blocks);
  * once per image and decoder layer the cross-attention K|V of the image tokens, one packed GEMM into
    [B, Li, 2D];
  * the text decoder (post-LN BERT with a cross-attention block) ONE token per step: the new token's K|V
    GEMM writes row t of the self-attention cache [B, Tmax, 2D] directly, the single query attends to
    rows 0..t and to the Li image keys with kernels.attn_decode, and the vocabulary projection never
    writes its logits: kernels.lm_head_argmax reads the tied embedding table once per step and returns
    the token, kernels.greedy_select applies the stop / pad / forced-token rule and writes the token
    where the next step's embedding kernel reads it. No token visits the host between steps, so the
    whole unrolled loop (vision tower included) is one captured HIP graph per (batch, steps, precision).
  * beam search: B images x nb beams are B * nb decoder rows that share the image's cross-attention K|V. A step
    writes its fp32 logits, kernels.beam_select leaves the 2 nb best (score, beam, token) per image,
    kernels.beam_update does transformers' bookkeeping on device state (running and finished hypotheses, the
    early-stop heuristic, the next token and the parent row of every beam) and kernels.beam_reorder gathers the
    self-attention caches by parent into a second set of buffers: still no host decision between steps and one
    captured graph per (batch, steps, precision, num_beams, length_penalty, early_stopping).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch
import torch.nn as nn

from . import blocks as Bk
from . import kernels as K


@dataclass
class BlipVisionConfig:
    hidden_size: int = 1024
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    intermediate_size: int = 4096
    image_size: int = 384
    patch_size: int = 16
    num_channels: int = 3
    layer_norm_eps: float = 1e-5


@dataclass
class BlipTextConfig:
    vocab_size: int = 30524
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    max_position_embeddings: int = 512
    layer_norm_eps: float = 1e-12
    bos_token_id: int = 30522
    sep_token_id: int = 102
    eos_token_id: int = 102
    pad_token_id: int = 0
    encoder_hidden_size: int | None = None  # width of the image tokens (default: the vision width)
    hidden_dropout_prob: float = 0.0        # inference only: accepted and unused
    attention_probs_dropout_prob: float = 0.0


@dataclass
class BlipConfig:
    """defaults: Salesforce/blip-image-captioning-large"""
    vision: BlipVisionConfig = field(default_factory=BlipVisionConfig)
    text: BlipTextConfig = field(default_factory=BlipTextConfig)

    def __post_init__(self):
        if isinstance(self.vision, dict):
            self.vision = BlipVisionConfig(**self.vision)
        if isinstance(self.text, dict):
            self.text = BlipTextConfig(**self.text)
        if self.text.encoder_hidden_size is None:
            self.text.encoder_hidden_size = self.vision.hidden_size


V = "vision_model."
T = "text_decoder.bert."
HEAD = "text_decoder.cls.predictions."
WORD = T + "embeddings.word_embeddings"
PATCH_W = V + "embeddings.patch_embedding.weight"


def _attn_block(D, kv_in, eps):
    a = nn.Module()
    a.self = nn.Module()
    a.self.query = nn.Linear(D, D)
    a.self.key = nn.Linear(kv_in, D)
    a.self.value = nn.Linear(kv_in, D)
    a.output = nn.Module()
    a.output.dense = nn.Linear(D, D)
    a.output.LayerNorm = nn.LayerNorm(D, eps=eps)
    return a


class BlipForConditionalGeneration(Bk.CachedWeights, nn.Module):
    """transformers' BlipForConditionalGeneration parameter layout (vision_model.*, text_decoder.bert.*,
    text_decoder.cls.predictions.*; the decoder weight and bias are the word embeddings and
    cls.predictions.bias). `generate` returns the token ids transformers' greedy `generate` returns."""

    def __init__(self, config: BlipConfig | None = None, **kw):
        super().__init__()
        c = self.config = config or BlipConfig(**kw)
        vc, tc = c.vision, c.text
        D = vc.hidden_size
        npatch = (vc.image_size // vc.patch_size) ** 2
        vm = self.vision_model = nn.Module()
        vm.embeddings = nn.Module()
        vm.embeddings.class_embedding = nn.Parameter(torch.zeros(1, 1, D))
        vm.embeddings.position_embedding = nn.Parameter(torch.zeros(1, npatch + 1, D))
        vm.embeddings.patch_embedding = nn.Conv2d(vc.num_channels, D, vc.patch_size, vc.patch_size)
        vm.encoder = nn.Module()
        vm.encoder.layers = nn.ModuleList()
        for _ in range(vc.num_hidden_layers):
            L = nn.Module()
            L.self_attn = nn.Module()
            L.self_attn.qkv = nn.Linear(D, 3 * D)
            L.self_attn.projection = nn.Linear(D, D)
            L.layer_norm1 = nn.LayerNorm(D, eps=vc.layer_norm_eps)
            L.mlp = nn.Module()
            L.mlp.fc1 = nn.Linear(D, vc.intermediate_size)
            L.mlp.fc2 = nn.Linear(vc.intermediate_size, D)
            L.layer_norm2 = nn.LayerNorm(D, eps=vc.layer_norm_eps)
            vm.encoder.layers.append(L)
        vm.post_layernorm = nn.LayerNorm(D, eps=vc.layer_norm_eps)

        E = tc.hidden_size
        td = self.text_decoder = nn.Module()
        td.bert = nn.Module()
        td.bert.embeddings = nn.Module()
        td.bert.embeddings.word_embeddings = nn.Embedding(tc.vocab_size, E, padding_idx=tc.pad_token_id)
        td.bert.embeddings.position_embeddings = nn.Embedding(tc.max_position_embeddings, E)
        td.bert.embeddings.LayerNorm = nn.LayerNorm(E, eps=tc.layer_norm_eps)
        td.bert.encoder = nn.Module()
        td.bert.encoder.layer = nn.ModuleList()
        for _ in range(tc.num_hidden_layers):
            L = nn.Module()
            L.attention = _attn_block(E, E, tc.layer_norm_eps)
            L.crossattention = _attn_block(E, tc.encoder_hidden_size, tc.layer_norm_eps)
            L.intermediate = nn.Module()
            L.intermediate.dense = nn.Linear(E, tc.intermediate_size)
            L.output = nn.Module()
            L.output.dense = nn.Linear(tc.intermediate_size, E)
            L.output.LayerNorm = nn.LayerNorm(E, eps=tc.layer_norm_eps)
            td.bert.encoder.layer.append(L)
        td.cls = nn.Module()
        pr = td.cls.predictions = nn.Module()
        pr.bias = nn.Parameter(torch.zeros(tc.vocab_size))
        pr.transform = nn.Module()
        pr.transform.dense = nn.Linear(E, E)
        pr.transform.LayerNorm = nn.LayerNorm(E, eps=tc.layer_norm_eps)
        pr.decoder = nn.Linear(E, tc.vocab_size)
        pr.decoder.weight = td.bert.embeddings.word_embeddings.weight  # tied, as in transformers
        pr.decoder.bias = pr.bias
        self.compute_dtype = torch.float32
        self._states = {}
        self._init_weights()

    def _init_weights(self, std=0.02):
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding, nn.Conv2d)):
                nn.init.normal_(m.weight, 0.0, std)
                if not isinstance(m, nn.Embedding) and m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        nn.init.trunc_normal_(self.vision_model.embeddings.class_embedding, 0.0, std)
        nn.init.trunc_normal_(self.vision_model.embeddings.position_embedding, 0.0, std)

    def set_precision(self, precision):
        self.compute_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[precision]
        return self

    def invalidate_caches(self):
        self._states.clear()
        return super().invalidate_caches()

    # ---- plumbing ----------------------------------------------------------------------------------
    def _ctx(self):
        """(StepCtx, device) of one call; refuses a CPU model and a call that would need gradients"""
        params = dict(self.named_parameters())
        dev = next(iter(params.values())).device
        if dev.type != "cuda":
            raise RuntimeError("mmfd BlipForConditionalGeneration runs on the HIP device: call .to('cuda') first")
        if torch.is_grad_enabled() and any(p.requires_grad for p in params.values()):
            raise NotImplementedError("mmfd BlipForConditionalGeneration is inference-only (the reference only "
                                      "captions with it, caption.py:22-31): call it under torch.no_grad() or "
                                      "freeze its parameters")
        P = {n: p.detach() for n, p in params.items()}
        # the two tied names are one parameter and named_parameters() lists it once
        P[HEAD + "decoder.weight"], P[HEAD + "decoder.bias"] = P[WORD + ".weight"], P[HEAD + "bias"]
        P[PATCH_W] = P[PATCH_W].reshape(P[PATCH_W].shape[0], -1)  # conv P/s P == GEMM over patches
        sc = Bk.StepCtx(P, self.compute_dtype, shadows=Bk.shadow_store(self))
        sc.cache_derived = True
        return sc, dev

    @staticmethod
    def _packed(sc, names):
        """(W, bias) of the row-concatenated Linears `names` in the compute dtype, kept across calls: a
        captured graph must not re-pack the fp32 weights on every replay (bf16 packs are shadows already)"""
        if sc.dt != torch.float32:
            return sc.w_packed(names)

        def pack():
            ws = [sc.P[n + ".weight"] for n in names]
            t = torch.empty((sum(w.shape[0] for w in ws), ws[0].shape[1]), device=ws[0].device, dtype=torch.float32)
            r = 0
            for w in ws:
                K.cast(w, torch.float32, out=t[r:r + w.shape[0]])
                r += w.shape[0]
            return t

        def pack_bias():
            bs = [sc.P[n + ".bias"] for n in names]
            t = torch.empty(sum(b.numel() for b in bs), device=bs[0].device, dtype=torch.float32)
            r = 0
            for b in bs:
                K.cast(b, torch.float32, out=t[r:r + b.numel()])
                r += b.numel()
            return t

        key = "|".join(names)
        return (sc.derived(key + "#w32", [n + ".weight" for n in names], pack),
                sc.derived(key + "#b32", [n + ".bias" for n in names], pack_bias))

    def _signature(self):
        """(data_ptr, version) of every parameter: a captured graph is baked with the addresses of the
        weights and of the shadows / packed biases built from them (as predict.PairPredictor)"""
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _state(self, B, steps, dev):
        """the device buffers of one (batch, steps, precision): static inputs, caches, workspaces"""
        key = (B, steps, self.compute_dtype, str(dev))
        st = self._states.get(key)
        if st is not None:
            return st
        vc, tc = self.config.vision, self.config.text
        dt, E, H = self.compute_dtype, tc.hidden_size, tc.num_attention_heads
        Li = (vc.image_size // vc.patch_size) ** 2 + 1
        # mmfd_gemm runs products of fewer than 16 rows on its scalar path: the decoder's activations carry
        # at least 16 rows (the padding rows embed token 0 and are never selected, attended across or read)
        Bp = max(B, 16)
        st = dict(
            B=B, Bp=Bp, steps=steps, Li=Li,
            px=torch.zeros(B, vc.num_channels, vc.image_size, vc.image_size, device=dev),
            # token ids step-major: row t is what step t embeds (contiguous), row t + 1 what it selects
            seq=torch.zeros(steps + 1, Bp, dtype=torch.int64, device=dev),
            forced=torch.zeros(steps + 1, B, dtype=torch.int64, device=dev),
            pos=torch.arange(steps + 1, dtype=torch.int64, device=dev)[:, None].expand(steps + 1, Bp).contiguous(),
            finished=torch.zeros(B, dtype=torch.int32, device=dev),
            argmax=torch.zeros(B, dtype=torch.int64, device=dev),
            self_kv=[torch.zeros(Bp, steps, 2 * E, device=dev, dtype=dt) for _ in range(tc.num_hidden_layers)],
            cross_o=torch.zeros(Bp, E, device=dev, dtype=dt),  # cross-attention output: rows >= B stay 0
            graph=None, sig=None, n_forced=-1)
        need = max(K.lib().mmfd_attn_decode_workspace_bytes(B, H, E // H, Li),
                   K.lib().mmfd_attn_decode_workspace_bytes(Bp, H, E // H, steps), 16)
        st["attn_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        need = K.lib().mmfd_lm_head_argmax_workspace_bytes(K.dtype_code(dt), B, tc.vocab_size, E)
        if need <= 0:
            raise ValueError(f"mmfd BLIP: the LM head kernel takes at most 32 rows and widths up to 1024 (fp32) / 2048 "
                             f"(bf16), got batch {B}, width {E}")
        st["lm_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        if len(self._states) >= 8:
            self._states.clear()
        self._states[key] = st
        return st

    # ---- vision tower ------------------------------------------------------------------------------
    def _vision(self, sc, px):
        vc = self.config.vision
        B, D, H, eps = px.shape[0], vc.hidden_size, vc.num_attention_heads, vc.layer_norm_eps
        patches = K.patchify(px, vc.patch_size, sc.dt)
        pe, _ = Bk.linear(sc, patches, V + "embeddings.patch_embedding")
        x = K.vit_tokens_fwd(pe, B, sc.P[V + "embeddings.class_embedding"], sc.P[V + "embeddings.position_embedding"])
        Tn = x.shape[1]
        x = Bk.as2d(x)
        for i in range(vc.num_hidden_layers):
            p = f"{V}encoder.layers.{i}"
            h, _, _ = Bk.layernorm(sc, x, p + ".layer_norm1", eps)
            qkv, _ = Bk.linear(sc, h, p + ".self_attn.qkv")  # columns [q | k | v], heads inside each third
            qkv = qkv.view(B, Tn, 3 * D)
            o, _ = K.attn_fwd(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], H)
            x1, _ = Bk.linear(sc, Bk.as2d(o), p + ".self_attn.projection", residual=x)
            h2, _, _ = Bk.layernorm(sc, x1, p + ".layer_norm2", eps)
            x, _ = Bk.ffn_fwd(sc, h2, p + ".mlp.fc1", p + ".mlp.fc2", residual=x1, keep=False, planes=False)
        y, _, _ = Bk.layernorm(sc, x, V + "post_layernorm", eps)
        return y.view(B, Tn, D)

    @torch.no_grad()
    def image_embeds(self, pixel_values):
        """vision_model(pixel_values).last_hidden_state: [B, 1 + patches, width] in the compute dtype"""
        sc, dev = self._ctx()
        return self._vision(sc, pixel_values.to(dev).float().contiguous())

    # ---- text decoder, one token per step ------------------------------------------------------------
    def _cross_kv(self, sc, emb):
        """per decoder layer the image tokens' cross-attention K|V [B, Li, 2E], one packed GEMM each"""
        B, Li, _ = emb.shape
        out = []
        for i in range(self.config.text.num_hidden_layers):
            p = f"{T}encoder.layer.{i}.crossattention.self"
            W, b = self._packed(sc, [p + ".key", p + ".value"])
            out.append(K.gemm(Bk.as2d(emb), W, bias=b).view(B, Li, -1))
        return out

    def _hidden(self, sc, st, cross, t, self_kv, nb=1):
        """the decoder body of step t: embeds st['seq'][t] at position t, appends its K|V to row t of the caches
        `self_kv`, and returns the LM head's input [Bp, E]. nb > 1: rows b*nb .. b*nb + nb - 1 are the beams of
        image b and attend the one cross-attention K|V of that image (attn_decode's group argument: no copy of the
        image keys per beam)"""
        tc = self.config.text
        E, H, eps, B, Bp = tc.hidden_size, tc.num_attention_heads, tc.layer_norm_eps, st["B"], st["Bp"]
        P = sc.P
        x = K.embed_ln_infer(st["seq"][t].view(Bp, 1), st["pos"][t].view(Bp, 1), P[WORD + ".weight"],
                             P[T + "embeddings.position_embeddings.weight"], P[T + "embeddings.LayerNorm.weight"],
                             P[T + "embeddings.LayerNorm.bias"], eps, sc.dt)
        for i in range(tc.num_hidden_layers):
            p = f"{T}encoder.layer.{i}"
            q, _ = Bk.linear(sc, x, p + ".attention.self.query")
            Wkv, bkv = self._packed(sc, [p + ".attention.self.key", p + ".attention.self.value"])
            kv = self_kv[i]
            K.gemm(x, Wkv, bias=bkv, out=kv[:, t, :])  # row t of the cache is the GEMM's output
            o = K.attn_decode(q, kv[..., :E], kv[..., E:], H, t + 1, workspace=st["attn_ws"])
            s1, _ = Bk.linear(sc, o, p + ".attention.output.dense", residual=x)
            h, _, _ = Bk.layernorm(sc, s1, p + ".attention.output.LayerNorm", eps)
            cq, _ = Bk.linear(sc, h, p + ".crossattention.self.query")
            ckv = cross[i]  # every image key takes part (transformers passes an all-ones mask)
            co = st["cross_o"]
            if nb == 1:
                K.attn_decode(cq[:B], ckv[..., :E], ckv[..., E:], H, ckv.shape[1], out=co[:B], workspace=st["attn_ws"])
            else:
                K.attn_decode(cq[:B * nb], ckv[..., :E], ckv[..., E:], H, ckv.shape[1], out=co[:B * nb],
                              workspace=st["attn_ws"], group=nb)
            s2, _ = Bk.linear(sc, co, p + ".crossattention.output.dense", residual=h)
            h2, _, _ = Bk.layernorm(sc, s2, p + ".crossattention.output.LayerNorm", eps)
            s3, _ = Bk.ffn_fwd(sc, h2, p + ".intermediate.dense", p + ".output.dense", residual=h2, keep=False,
                               planes=False)
            x, _, _ = Bk.layernorm(sc, s3, p + ".output.LayerNorm", eps)
        g, _ = Bk.linear(sc, x, HEAD + "transform.dense", act=K.ACT_GELU)
        g, _, _ = Bk.layernorm(sc, g, HEAD + "transform.LayerNorm", eps)
        return g

    def _step(self, sc, st, cross, t, forced, logits=None, select=True):
        """decoder step t: embeds st['seq'][t] at position t, appends its K|V to the self cache, and
        (select) writes the next token to st['seq'][t + 1]"""
        tc = self.config.text
        B, P = st["B"], sc.P
        g = self._hidden(sc, st, cross, t, st["self_kv"])
        K.lm_head_argmax(g[:B], sc.w(WORD), P[HEAD + "bias"], out=st["argmax"], logits=logits, workspace=st["lm_ws"])
        if select:
            K.greedy_select(st["argmax"], st["finished"], tc.sep_token_id, tc.pad_token_id, st["seq"][t + 1, :B],
                            forced=st["forced"][t + 1] if forced else None)

    def _run(self, st, n_forced, logits=None):
        """vision tower, cross K|V and every step on the state's static buffers; steps t < n_forced take
        their next token from st['forced'][t + 1]"""
        sc, _ = self._ctx()
        cross = self._cross_kv(sc, self._vision(sc, st["px"]))
        for t in range(st["steps"]):
            self._step(sc, st, cross, t, forced=t < n_forced, logits=None if logits is None else logits[t],
                       select=logits is None or t + 1 < st["steps"])

    def _begin(self, st, first_tokens):
        st["seq"].zero_()
        st["seq"][0, :st["B"]].copy_(first_tokens)
        st["finished"].zero_()

    def _prompt(self, input_ids):
        """the shared prompt as a list of ids starting with bos (transformers' generate: input_ids[:, 0] = bos
        and the tokenizer's trailing [SEP] dropped)"""
        tc = self.config.text
        if input_ids is None:
            return [tc.bos_token_id]
        ids = torch.as_tensor(input_ids).reshape(-1).tolist()
        if not ids:
            return [tc.bos_token_id]
        ids[0] = tc.bos_token_id
        if len(ids) > 1 and ids[-1] == tc.sep_token_id:
            ids = ids[:-1]
        return [int(i) for i in ids]

    @torch.no_grad()
    def generate(self, pixel_values, input_ids=None, max_new_tokens=20, use_graph=True, num_beams=1,
                 length_penalty=1.0, early_stopping=False):
        """Captions, greedy (num_beams=1) or by beam search (below). Greedy: int64 [B, P + n] ids (the prompt, bos first, then n <= max_new_tokens generated
        tokens: a row that produced sep_token_id is padded with pad_token_id, and n is where the last row
        stopped) — the array transformers' `generate(pixel_values, input_ids)` returns by default.
        `input_ids`: an optional prompt shared by all rows, fed one token per step in place of the argmax.
        use_graph: replay one captured HIP graph of all steps and trim on the host; else run eagerly and
        stop once every row has finished.
        num_beams in 2 .. 8 (num_beams * batch <= 32, the LM head's rows): transformers' beam search with
        `length_penalty` and `early_stopping` (False or True), no sampling, one returned sequence per image — the
        array `generate(pixel_values, input_ids, num_beams=..., length_penalty=..., early_stopping=...,
        max_new_tokens=...)` returns there, unused positions filled as transformers fills them
        (`pad_token_id or sep_token_id`). `self.sequences_scores` then holds the fp32 scores [B] of the returned
        hypotheses. Among equal scores the lower beam, then the lower token wins (torch.topk leaves that open)."""
        tc = self.config.text
        B = int(pixel_values.shape[0])
        if early_stopping not in (False, True):
            raise ValueError(f"early_stopping must be False or True, got {early_stopping!r} ('never' is not implemented)")
        if int(num_beams) != num_beams or not 1 <= num_beams <= 8:
            raise ValueError(f"num_beams must lie in [1, 8], got {num_beams}")
        if num_beams > 1 and (num_beams > tc.vocab_size // 2 or B * num_beams > 32):
            raise ValueError(f"beam search needs num_beams <= vocab_size / 2 and batch * num_beams <= 32 (the LM head "
                             f"kernel's rows), got batch {B}, num_beams {num_beams}, vocabulary {tc.vocab_size}")
        sc, dev = self._ctx()
        px = pixel_values.to(dev).float().contiguous()
        prompt = self._prompt(input_ids)
        if num_beams > 1:
            return self._generate_beams(sc, dev, px, prompt, int(max_new_tokens), bool(use_graph), int(num_beams),
                                        float(length_penalty), bool(early_stopping))
        n_forced = len(prompt) - 1
        steps = n_forced + int(max_new_tokens)
        if steps < 1 or steps + 1 > tc.max_position_embeddings:
            raise ValueError(f"prompt ({len(prompt)}) + max_new_tokens ({max_new_tokens}) must lie in "
                             f"[2, {tc.max_position_embeddings}]")
        st = self._state(B, steps, dev)
        if tuple(px.shape) != tuple(st["px"].shape):
            raise ValueError(f"pixel_values must be {tuple(st['px'].shape)}, got {tuple(px.shape)}")
        st["px"].copy_(px)
        st["forced"].zero_()
        st["forced"][:len(prompt)] = torch.tensor(prompt, dtype=torch.int64, device=dev)[:, None]
        self._begin(st, st["forced"][0])
        if use_graph:
            if st["graph"] is None or st["sig"] != self._signature() or st["n_forced"] != n_forced:
                self._capture(st, n_forced, dev)
                self._begin(st, st["forced"][0])
            st["graph"].replay()
            seq = st["seq"][:, :B].t().cpu()
            done = seq[:, n_forced + 1:] == tc.sep_token_id
            first = torch.where(done.any(1), done.int().argmax(1) + 1, torch.tensor(int(max_new_tokens)))
            return seq[:, :n_forced + 1 + int(first.max())].contiguous()
        cross = self._cross_kv(sc, self._vision(sc, st["px"]))
        n = steps
        for t in range(steps):
            self._step(sc, st, cross, t, forced=t < n_forced)
            if t >= n_forced and bool(st["finished"].all()):
                n = t + 1
                break
        return st["seq"][:n + 1, :B].t().contiguous().cpu()

    def _capture(self, st, n_forced, dev, run=None):
        run = run or self._run
        st["graph"] = None
        st["sig"], st["n_forced"] = self._signature(), n_forced
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            run(st, n_forced)  # warm up: weight shadows, packed biases, kernel attributes
        torch.cuda.current_stream(dev).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run(st, n_forced)
        st["graph"] = g

    # ---- beam search ---------------------------------------------------------------------------------
    def _beam_state(self, B, steps, dev, nb, lp, early):
        """the device buffers of one (batch, steps, precision, beam parameters): what _state holds for B * nb rows,
        a second set of self-attention caches (the reorder gathers from one into the other), the fp32 logits of
        one step and the search state of csrc/beam.hip"""
        key = (B, steps, self.compute_dtype, str(dev), nb, lp, early)
        st = self._states.get(key)
        if st is not None:
            return st
        vc, tc = self.config.vision, self.config.text
        dt, E, H, L = self.compute_dtype, tc.hidden_size, tc.num_attention_heads, tc.num_hidden_layers
        Li = (vc.image_size // vc.patch_size) ** 2 + 1
        R, T = B * nb, steps + 1
        Bp = max(R, 16)
        i32 = dict(dtype=torch.int32, device=dev)
        kv = [[torch.zeros(Bp, steps, 2 * E, device=dev, dtype=dt) for _ in range(L)] for _ in range(2)]
        st = dict(
            B=B, Bp=Bp, R=R, nb=nb, lp=lp, early=early, steps=steps, Li=Li,
            px=torch.zeros(B, vc.num_channels, vc.image_size, vc.image_size, device=dev),
            seq=torch.zeros(T, Bp, dtype=torch.int64, device=dev),
            pos=torch.arange(T, dtype=torch.int64, device=dev)[:, None].expand(T, Bp).contiguous(),
            argmax=torch.zeros(R, dtype=torch.int64, device=dev),
            kv=kv, kv_table=[K.ptr_table(kv[0]), K.ptr_table(kv[1])],
            cross_o=torch.zeros(Bp, E, device=dev, dtype=dt),
            logits=torch.zeros(R, tc.vocab_size, device=dev),
            cand=(torch.zeros(B, 2 * nb, device=dev), torch.zeros(B, 2 * nb, **i32), torch.zeros(B, 2 * nb, **i32)),
            beam=dict(run_score=torch.zeros(B, nb, device=dev), fin_score=torch.zeros(B, nb, device=dev),
                      fin_flag=torch.zeros(B, nb, **i32), fin_len=torch.zeros(B, nb, **i32),
                      run_seq=torch.zeros(B, nb, T, **i32), fin_seq=torch.zeros(B, nb, T, **i32),
                      flags=torch.zeros(B, 4, **i32), parent=torch.zeros(R, **i32)),
            graph=None, sig=None, n_forced=-1)
        need = max(K.lib().mmfd_attn_decode_workspace_bytes(B, H, E // H, Li),
                   K.lib().mmfd_attn_decode_workspace_bytes(R, H, E // H, Li),
                   K.lib().mmfd_attn_decode_workspace_bytes(Bp, H, E // H, steps), 16)
        st["attn_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        need = K.lib().mmfd_lm_head_argmax_workspace_bytes(K.dtype_code(dt), R, tc.vocab_size, E)
        if need <= 0:
            raise ValueError(f"mmfd BLIP: the LM head kernel takes at most 32 rows and widths up to 1024 (fp32) / 2048 "
                             f"(bf16), got {R} rows, width {E}")
        st["lm_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        st["sel_ws"] = torch.empty(K.beam_select_workspace_bytes(B, nb, tc.vocab_size), dtype=torch.uint8, device=dev)
        if len(self._states) >= 8:
            self._states.clear()
        self._states[key] = st
        return st

    def _beam_begin(self, st, prompt):
        """the state before the first step (transformers' step 3): every beam holds the prompt, which the forced
        steps embed token by token; running scores [0, -1e9, ...]; nothing finished"""
        tc = self.config.text
        bs, R = st["beam"], st["R"]
        ids = torch.tensor(prompt, dtype=torch.int64, device=st["seq"].device)
        st["seq"].zero_()
        st["seq"][:len(prompt), :R] = ids[:, None]
        bs["run_seq"].fill_(tc.pad_token_id or tc.sep_token_id)  # transformers: `pad_token_id or eos_token_id[0]`
        bs["run_seq"][:, :, :len(prompt)] = ids.int()
        bs["fin_seq"].copy_(bs["run_seq"])
        bs["run_score"].fill_(-1.0e9)
        bs["run_score"][:, 0] = 0.0
        bs["fin_score"].fill_(-1.0e9)
        bs["fin_flag"].zero_()
        bs["fin_len"].zero_()
        bs["flags"].zero_()
        bs["flags"][:, 0] = 1
        bs["parent"].copy_(torch.arange(R, dtype=torch.int32, device=bs["parent"].device))

    def _beam_unfinished(self, st):
        """transformers' loop condition, from one host read of the per-image flags"""
        f = st["beam"]["flags"].cpu().bool()
        return bool(f[:, 0].any()) and not (st["early"] and bool(f[:, 1].all())) and not bool(f[:, 2].all())

    def _beam_run(self, st, n_forced, eager=False):
        """vision tower, cross K|V and every step. A forced step only feeds the decoder: its next token is the
        prompt's, already in st['seq']. A free step writes the fp32 logits, selects the 2 nb candidates of every
        image, updates the search state (which writes the next tokens and the parent rows) and gathers the
        caches by parent into the other set. eager: leave once transformers would (the remaining steps change
        nothing: every update of an image that cannot improve is masked)."""
        tc = self.config.text
        sc, _ = self._ctx()
        R, nb, steps = st["R"], st["nb"], st["steps"]
        cross = self._cross_kv(sc, self._vision(sc, st["px"]))
        cur = 0
        for t in range(steps):
            g = self._hidden(sc, st, cross, t, st["kv"][cur], nb)
            if t < n_forced:
                continue
            K.lm_head_argmax(g[:R], sc.w(WORD), sc.P[HEAD + "bias"], out=st["argmax"], logits=st["logits"],
                             workspace=st["lm_ws"])
            K.beam_select(st["logits"], st["beam"]["run_score"].view(-1), nb, out=st["cand"], workspace=st["sel_ws"])
            K.beam_update(st["cand"], st["beam"], t, n_forced, t + 1 == steps, tc.sep_token_id, st["lp"], st["early"],
                          st["seq"][t + 1, :R])
            if t + 1 < steps:
                K.beam_reorder(st["kv"][cur], st["kv"][1 - cur], st["kv_table"][cur], st["kv_table"][1 - cur],
                               st["beam"]["parent"], R, t + 1)
                cur = 1 - cur
            if eager and not self._beam_unfinished(st):
                break

    def _generate_beams(self, sc, dev, px, prompt, max_new_tokens, use_graph, nb, lp, early):
        tc = self.config.text
        B = px.shape[0]
        n_forced = len(prompt) - 1
        steps = n_forced + max_new_tokens
        if max_new_tokens < 1 or steps + 1 > tc.max_position_embeddings:
            raise ValueError(f"prompt ({len(prompt)}) + max_new_tokens ({max_new_tokens}) must lie in "
                             f"[2, {tc.max_position_embeddings}]")
        st = self._beam_state(B, steps, dev, nb, lp, early)
        if tuple(px.shape) != tuple(st["px"].shape):
            raise ValueError(f"pixel_values must be {tuple(st['px'].shape)}, got {tuple(px.shape)}")
        st["px"].copy_(px)
        self._beam_begin(st, prompt)
        if use_graph:
            if st["graph"] is None or st["sig"] != self._signature() or st["n_forced"] != n_forced:
                self._capture(st, n_forced, dev, run=self._beam_run)
                self._beam_begin(st, prompt)
            st["graph"].replay()
        else:
            self._beam_run(st, n_forced, eager=True)
        bs = st["beam"]
        n = int(bs["fin_len"][:, 0].max())  # transformers counts the entries of the chosen hypotheses' beam trail
        self.sequences_scores = bs["fin_score"][:, 0].clone()
        return bs["fin_seq"][:, 0, :len(prompt) + n].long().cpu().contiguous()

    @torch.no_grad()
    def _forward_logits(self, pixel_values, forced_ids):
        sc, dev = self._ctx()
        ids = torch.as_tensor(forced_ids).to(dev).long()
        B, Tn = ids.shape
        if Tn + 1 > self.config.text.max_position_embeddings:
            raise ValueError("forced_ids is longer than the position table")
        st = self._state(B, Tn, dev)
        st["px"].copy_(pixel_values.to(dev).float())
        st["forced"].zero_()
        st["forced"][:Tn] = ids.t()
        self._begin(st, st["forced"][0])
        logits = torch.empty(Tn, B, self.config.text.vocab_size, device=dev, dtype=torch.float32)
        self._run(st, Tn, logits=logits)
        return logits

    def forward_logits(self, pixel_values, forced_ids):
        """the generation steps with every token forced: fp32 logits [T, B, V], logits[t] being step t's (what
        follows forced_ids[:, :t + 1]); forced_ids int64 [B, T]. The same kernels and caches as generate."""
        self._ctx()  # (refuses a call that would need gradients before no_grad hides it)
        return self._forward_logits(pixel_values, forced_ids)

    def forward(self, pixel_values, input_ids):
        """teacher-forced logits [T, B, V] (forward_logits); inference only"""
        return self.forward_logits(pixel_values, input_ids)
