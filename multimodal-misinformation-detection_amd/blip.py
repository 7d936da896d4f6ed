"""BLIP image captioning on HIP kernels: the reference's captioning stage (src/preprocess/caption.py:22-31
and src/demo/app.py run `BlipForConditionalGeneration.from_pretrained("Salesforce/blip-image-captioning-
large").generate(**inputs)` over every claim and evidence image), and the caption loss of transformers'
`forward(..., labels=)`: scoring on any model, fine-tuning of the text decoder with
`BlipConfig(train_text_decoder=True)` (the vision tower stays frozen; the last item below).

`BlipForConditionalGeneration` keeps transformers' parameter names, so its `state_dict` loads with
`strict=True`; `generate` follows transformers' greedy default (20 new tokens, decoding from [bos], stop
at sep_token_id, pad afterwards) or, with num_beams > 1, its beam search (csrc/beam.hip).

What runs where:
  * vision tower (pre-LN ViT, packed qkv): patchify + GEMM, class token + positions, then per layer
    LayerNorm -> qkv GEMM -> attn_fwd -> projection GEMM (+ residual) -> LayerNorm -> fc1 GELU -> fc2
    (+ residual), and post_layernorm: the encoders' kernels (mmfd.blocks);
  * once per image and decoder layer the cross-attention K|V of the image tokens, one packed GEMM into
    [B, Li, 2D];
  * the text decoder (post-LN BERT with a cross-attention block) ONE token per step, one loop for all modes (_run):
    the new token's K|V GEMM writes row t of the self-attention cache [Bp, Tmax, 2D] directly, the single query
    attends to rows 0..t and to the Li image keys with kernels.attn_decode (_hidden), and the mode selects the next
    token and writes it where the next step's embedding kernel reads it. Greedy (_Greedy): kernels.lm_head_argmax
    reads the tied embedding table once and returns the token without writing logits, kernels.greedy_select applies
    the stop / pad / forced-token rule. Sampling (_Sample, n rows per image): the LM head writes fp32 logits,
    kernels.sample_select draws, then the greedy rule. Beam search (_Beams, nb rows per image): kernels.beam_select
    leaves the 2 nb best (score, beam, token) per image, kernels.beam_update does transformers' bookkeeping on
    device state and kernels.beam_reorder gathers the caches by parent into a second set. An image's rows share its
    cross-attention K|V. No token visits the host between steps, so the unrolled loop (vision tower included) is
    one captured HIP graph per state (_state: mode and parameters, batch, steps, precision), replayed by _decode.
  * the caption loss (forward(labels=)) shares no code with generation: ONE pass of the decoder over all T
    positions with no K|V cache — embeddings, per layer the packed Q|K|V GEMM, attn_fwd under a causal additive
    bias [H, T, T] and the key-padding bias, output projection + LayerNorm, cross-attention of the text rows over
    the image's K|V, FFN + LayerNorm, then the head transform — the fp32 logits of all B * T rows from one GEMM
    against the tied embedding table, and kernels.vocab_xent_fwd (csrc/lm_loss.hip). Under grad with
    train_text_decoder the whole pass is one autograd node (_BlipLossFn) with a hand-written backward that fills
    the gradient of every text_decoder parameter; vision_model parameters receive None, so the optimizer is
    handed `model.text_decoder.parameters()` only. Eager; right-padded batches only.
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
    hidden_dropout_prob: float = 0.0        # generation: accepted and unused; the loss path refuses > 0 in training mode
    attention_probs_dropout_prob: float = 0.0
    label_smoothing: float = 0.0            # of the caption loss (transformers' BlipTextConfig.label_smoothing)


@dataclass
class BlipConfig:
    """defaults: Salesforce/blip-image-captioning-large"""
    vision: BlipVisionConfig = field(default_factory=BlipVisionConfig)
    text: BlipTextConfig = field(default_factory=BlipTextConfig)
    train_text_decoder: bool = False  # forward(labels=) under grad fills the text_decoder gradients (else: refused)

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
QKV = (".attention.self.query", ".attention.self.key", ".attention.self.value")
CROSS_KV = (".crossattention.self.key", ".crossattention.self.value")
# The causal mask value. It is added to the key-padding bias of kernels.mask_to_bias (the most negative fp32,
# -3.4028e38, on a padded key) and to a scaled score: -1e30 is below any score by more than exp() can resolve
# (exp(-1e30 - m) == 0 exactly), and -3.4028e38 - 1e30 rounds back to -3.4028e38 (1e30 is under half an ulp
# there), so mask + padding bias stays finite: the softmax never sees -inf, and never forms inf - inf.
CAUSAL_NEG = -1.0e30


def vocab_ld(V):
    """columns of the logits and dlogits buffers, and rows of the tied table as the LM-head backward reads it: V
    rounded up to a multiple of 8. Rows of V bf16 or fp32 elements then start 16 bytes aligned, which the vector
    paths of csrc/lm_loss.hip and the MFMA kernels of mmfd_gemm need of a contiguous extent (BLIP's 30,524 is
    4 * 7631: unpadded, the two bf16 LM-head backward products fall to the one-output-per-thread kernel)"""
    return -(-V // 8) * 8


def lm_head_gemm_paths(dtype, R, V, E):
    """the launch plans (kernels.gemm_path: host arithmetic only) of the three LM-head products of the caption loss
    as _loss_forward and _loss_backward issue them for R rows: the logits, dG = dlogits W, dW = dlogits^T G"""
    Vp = vocab_ld(V)
    return {"logits": K.gemm_path(dtype, R, V, E, ldc=Vp, out_dtype=torch.float32, bias=True),
            "dG": K.gemm_path(dtype, R, E, Vp, trans_b=True),
            "dW": K.gemm_path(dtype, Vp, E, R, trans_a=True, trans_b=True, out_dtype=torch.float32, a_rowsum=True)}


@dataclass
class BlipCaptionLossOutput:
    """forward(labels=): `loss` fp32, a scalar (reduction="mean") or the per-sequence sums [B] ("none");
    `logits` fp32 [B, T, V] when asked for, else None"""
    loss: torch.Tensor
    logits: torch.Tensor | None = None


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


class _Greedy:
    """What a decoding mode adds to the one state builder, loop and driver of BlipForConditionalGeneration (_state,
    _run, _decode), here for greedy decoding: its state key and buffers, the state before the first step, the
    selection of step t (from the LM head to the write of seq[t + 1]), when an eager run may stop, and the result.
    `m` is the model, `st` the state, `g` the LM head's input of the step (_hidden)."""
    rows = 1         # decoder rows per image
    min_new = 0      # the fewest max_new_tokens: a prompt of two ids with nothing to generate is accepted
    wide_ok = False  # more than 32 rows on the wide LM head: generate's greedy calls only

    def __init__(self, wide_ok=False):
        self.wide_ok = wide_ok

    def key(self, B, steps, dt, dev):
        return (B, steps, dt, dev)

    def buffers(self, m, st, dev):
        st["forced"] = torch.zeros(st["steps"] + 1, st["R"], dtype=torch.int64, device=dev)
        st["finished"] = torch.zeros(st["R"], dtype=torch.int32, device=dev)

    def begin(self, m, st, prompt):
        """prompt: the ids [P] shared by all rows, or [P, rows] (forward_logits)"""
        ids = torch.as_tensor(prompt, dtype=torch.int64, device=st["seq"].device)
        st["forced"].zero_()
        st["forced"][:len(ids)] = ids.view(len(ids), -1)
        st["seq"].zero_()
        st["seq"][0, :st["R"]].copy_(st["forced"][0])
        st["finished"].zero_()

    def cache(self, st, t, n_forced):
        return st["self_kv"]

    def select(self, m, sc, st, g, t, n_forced, logits=None):
        """the fused argmax, then the stop / pad / forced-token rule. logits (forward_logits): where the LM head also
        writes the step's fp32 logits; the last step then selects nothing"""
        tc = m.config.text
        R, P, forced = st["R"], sc.P, t < n_forced
        # more than 32 rows: the wide LM head, the narrow kernel's body over 32-row tiles
        lm_head = K.lm_head_argmax_wide if st["wide"] else K.lm_head_argmax
        if st.get("proc") is None or logits is not None:
            # (a forced step discards this argmax: wasted work, and a launch less is another captured graph)
            lm_head(g[:R], sc.w(WORD), P[HEAD + "bias"], out=st["argmax"], logits=logits, workspace=st["lm_ws"])
        elif not forced:
            # logits processors: the LM head stores its fp32 logits, the edits run on them, and the argmax is taken
            # of the edited row (a fix-up of the fused argmax would not do: were the raw winner an edited column,
            # the best unedited one would be unknown). A forced step needs neither: its token is the prompt's.
            lm_head(g[:R], sc.w(WORD), P[HEAD + "bias"], out=st["argmax"], logits=st["logits"], workspace=st["lm_ws"])
            m._edit(st, st["logits"], st["seq"], "steps", t)
            K.row_argmax(st["logits"], out=st["argmax"])
        if logits is None or t + 1 < st["steps"]:
            K.greedy_select(st["argmax"], st["finished"], tc.sep_token_id, tc.pad_token_id, st["seq"][t + 1, :R],
                            forced=st["forced"][t + 1] if forced else None)

    def stop(self, st, t, n_forced):
        return t >= n_forced and bool(st["finished"].all())

    def result(self, m, st, n_prompt, max_new_tokens, ran):
        """int64 [rows, P + n] ids. ran: the steps an eager run took; None after a replay, which ran them all: the
        ids are then trimmed on the host to where the last row stopped"""
        R = st["R"]
        if ran is not None:
            return st["seq"][:ran + 1, :R].t().contiguous().cpu()
        seq = st["seq"][:, :R].t().cpu()
        done = seq[:, n_prompt:] == m.config.text.sep_token_id
        first = torch.where(done.any(1), done.int().argmax(1) + 1, torch.tensor(max_new_tokens))
        return seq[:, :n_prompt + int(first.max())].contiguous()


class _Sample(_Greedy):
    """sampling: the greedy mode with the argmax replaced, n rows per image"""
    min_new = 1

    def __init__(self, m, n, temperature, top_k, top_p, seed, row_offset):
        if row_offset < 0:
            raise ValueError(f"row_offset must be >= 0, got {row_offset}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        self.seed = m.sample_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.rows, self.temperature, self.top_k, self.top_p, self.row_offset = n, temperature, top_k, top_p, row_offset

    def key(self, B, steps, dt, dev):
        return ("sample", B, self.rows, steps, dt, dev, self.temperature, self.top_k, self.top_p)

    def buffers(self, m, st, dev):
        """beside the greedy ones: the fp32 logits of one step, the sampled tokens and the {seed, row offset} the
        selection reads on the device"""
        super().buffers(m, st, dev)
        R, V_ = st["R"], m.config.text.vocab_size
        st["token"] = torch.zeros(R, dtype=torch.int64, device=dev)
        st["ctl"] = torch.zeros(2, dtype=torch.int64, device=dev)
        st["logits"] = torch.zeros(R, V_, device=dev)
        st["smp_ws"] = torch.empty(K.sample_select_workspace_bytes(R, V_), dtype=torch.uint8, device=dev)

    def begin(self, m, st, prompt):
        super().begin(m, st, prompt)
        seed = self.seed - (1 << 64) if self.seed >= (1 << 63) else self.seed
        st["ctl"].copy_(torch.tensor([seed, self.row_offset], dtype=torch.int64))

    def select(self, m, sc, st, g, t, n_forced, logits=None):
        """the LM head writes the fp32 logits, sample_select draws the row's token from them, and the unchanged
        greedy rule applies forced / finished / pad / eos. A forced step needs no logits: its token is the prompt's."""
        tc = m.config.text
        R, forced = st["R"], t < n_forced
        if not forced:
            K.lm_head_argmax(g[:R], sc.w(WORD), sc.P[HEAD + "bias"], out=st["argmax"], logits=st["logits"],
                             workspace=st["lm_ws"])
            if st.get("proc") is not None:  # the processors come before the warpers, as in transformers
                m._edit(st, st["logits"], st["seq"], "steps", t)
            K.sample_select(st["logits"], self.temperature, self.top_k, self.top_p, st["ctl"], t, out=st["token"],
                            workspace=st["smp_ws"])
        K.greedy_select(st["token"], st["finished"], tc.sep_token_id, tc.pad_token_id, st["seq"][t + 1, :R],
                        forced=st["forced"][t + 1] if forced else None)


class _Beams:
    """beam search: nb rows per image, the search state of csrc/beam.hip, and two sets of self-attention caches
    between which the reorder gathers by parent"""
    min_new = 1
    wide_ok = False

    def __init__(self, nb, lp, early):
        self.rows, self.lp, self.early = nb, lp, early

    def key(self, B, steps, dt, dev):
        return (B, steps, dt, dev, self.rows, self.lp, self.early)

    def buffers(self, m, st, dev):
        B, R, nb, T_, V_ = st["B"], st["R"], self.rows, st["steps"] + 1, m.config.text.vocab_size
        i32 = dict(dtype=torch.int32, device=dev)
        st["kv"] = [st["self_kv"], [torch.zeros_like(c) for c in st["self_kv"]]]
        st["kv_table"] = [K.ptr_table(st["kv"][0]), K.ptr_table(st["kv"][1])]
        st["logits"] = torch.zeros(R, V_, device=dev)
        st["cand"] = (torch.zeros(B, 2 * nb, device=dev), torch.zeros(B, 2 * nb, **i32), torch.zeros(B, 2 * nb, **i32))
        st["beam"] = dict(run_score=torch.zeros(B, nb, device=dev), fin_score=torch.zeros(B, nb, device=dev),
                          fin_flag=torch.zeros(B, nb, **i32), fin_len=torch.zeros(B, nb, **i32),
                          run_seq=torch.zeros(B, nb, T_, **i32), fin_seq=torch.zeros(B, nb, T_, **i32),
                          flags=torch.zeros(B, 4, **i32), parent=torch.zeros(R, **i32))
        st["sel_ws"] = torch.empty(K.beam_select_workspace_bytes(B, nb, V_), dtype=torch.uint8, device=dev)

    def begin(self, m, st, prompt):
        """the state before the first step (transformers' step 3): every beam holds the prompt, which the forced
        steps embed token by token; running scores [0, -1e9, ...]; nothing finished"""
        tc = m.config.text
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

    def cache(self, st, t, n_forced):
        return st["kv"][max(t - n_forced, 0) & 1]  # every free step but the last gathers into the other set

    def select(self, m, sc, st, g, t, n_forced, logits=None):
        """A forced step only feeds the decoder: its next token is the prompt's, already in st['seq']. A free step
        writes the fp32 logits, selects the 2 nb candidates of every image, updates the search state (which writes
        the next tokens and the parent rows) and gathers the caches by parent into the other set."""
        if t < n_forced:
            return
        tc = m.config.text
        R, nb, steps = st["R"], self.rows, st["steps"]
        K.lm_head_argmax(g[:R], sc.w(WORD), sc.P[HEAD + "bias"], out=st["argmax"], logits=st["logits"],
                         workspace=st["lm_ws"])
        if st.get("proc") is None:
            K.beam_select(st["logits"], st["beam"]["run_score"].view(-1), nb, out=st["cand"], workspace=st["sel_ws"])
        else:
            # transformers hands log_softmax(logits) of every running beam to the processors and adds the running
            # score afterwards: normalise once (over the unprocessed row), edit from the beam's own sequence as
            # the last update left it, select without a second normalisation
            K.row_log_softmax(st["logits"], workspace=st["sel_ws"])
            m._edit(st, st["logits"], st["beam"]["run_seq"].view(R, steps + 1), "rows", t)
            K.beam_select_logprobs(st["logits"], st["beam"]["run_score"].view(-1), nb, out=st["cand"],
                                   workspace=st["sel_ws"])
        K.beam_update(st["cand"], st["beam"], t, n_forced, t + 1 == steps, tc.sep_token_id, self.lp, self.early,
                      st["seq"][t + 1, :R])
        if t + 1 < steps:
            cur = (t - n_forced) & 1
            K.beam_reorder(st["kv"][cur], st["kv"][1 - cur], st["kv_table"][cur], st["kv_table"][1 - cur],
                           st["beam"]["parent"], R, t + 1)

    def stop(self, st, t, n_forced):
        """transformers' loop condition, from one host read of the per-image flags: an eager run leaves once
        transformers would (the remaining steps change nothing: every update of an image that cannot improve is
        masked)"""
        if t < n_forced:
            return False
        f = st["beam"]["flags"].cpu().bool()
        return not (bool(f[:, 0].any()) and not (self.early and bool(f[:, 1].all())) and not bool(f[:, 2].all()))

    def result(self, m, st, n_prompt, max_new_tokens, ran):
        bs = st["beam"]
        n = int(bs["fin_len"][:, 0].max())  # transformers counts the entries of the chosen hypotheses' beam trail
        m.sequences_scores = bs["fin_score"][:, 0].clone()
        return bs["fin_seq"][:, 0, :n_prompt + n].long().cpu().contiguous()


class BlipForConditionalGeneration(Bk.CachedWeights, nn.Module):
    """transformers' BlipForConditionalGeneration parameter layout (vision_model.*, text_decoder.bert.*,
    text_decoder.cls.predictions.*; the decoder weight and bias are the word embeddings and
    cls.predictions.bias). `generate` returns the token ids transformers' greedy `generate` returns."""

    # rows of one greedy generate call. kernels.lm_head_argmax_wide takes 256; a 256-row call of the default model
    # did not complete on an MI355X and the cause is not known ("Captioning"), 128 rows is what ran
    MAX_GREEDY_ROWS = 128

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
        self._causal = {}
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
    def _ctx(self, train=False):
        """(StepCtx, device) of one call; refuses a CPU model and a call that would need gradients (`train`: the
        context of _BlipLossFn, whose weight-derived tensors are rebuilt on every call)"""
        params = dict(self.named_parameters())
        dev = next(iter(params.values())).device
        if dev.type != "cuda":
            raise RuntimeError("mmfd BlipForConditionalGeneration runs on the HIP device: call .to('cuda') first")
        if not train and torch.is_grad_enabled() and any(p.requires_grad for p in params.values()):
            raise NotImplementedError("mmfd BlipForConditionalGeneration is inference-only (the reference only "
                                      "captions with it, caption.py:22-31): call it under torch.no_grad() or "
                                      "freeze its parameters")
        P = {n: p.detach() for n, p in params.items()}
        # the two tied names are one parameter and named_parameters() lists it once
        P[HEAD + "decoder.weight"], P[HEAD + "decoder.bias"] = P[WORD + ".weight"], P[HEAD + "bias"]
        P[PATCH_W] = P[PATCH_W].reshape(P[PATCH_W].shape[0], -1)  # conv P/s P == GEMM over patches
        sc = Bk.StepCtx(P, self.compute_dtype, shadows=Bk.shadow_store(self))
        sc.cache_derived = not train
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

    @staticmethod
    def _proc_key(proc):
        """what a state key carries of the logits processors: nothing when all are off (the keys, and so the
        captured graphs, of a model that never uses them are what they were); else the launch scalars and the
        LENGTH of the suppress list, whose ids live in a device buffer filled before every run"""
        return () if proc is None else ("proc",) + tuple(proc[:4]) + (len(proc[4]),)

    def _proc_buffers(self, st, proc, rows, dev):
        """what a state with logits processors holds beside the others: the suppress list and, where the mode has
        none yet (greedy), the fp32 logits of one step"""
        if proc is None:
            return
        st["proc"] = proc
        st["suppress"] = torch.zeros(max(1, len(proc[4])), dtype=torch.int64, device=dev)
        if "logits" not in st:
            st["logits"] = torch.zeros(rows, self.config.text.vocab_size, device=dev)

    @staticmethod
    def _proc_begin(st, proc, n_prompt):
        """before a run: the prompt's length (min_new_tokens counts from it) and this call's suppress list"""
        st["n_prompt"] = n_prompt
        if proc is not None and proc[4]:
            st["suppress"].copy_(torch.tensor(proc[4], dtype=torch.int64))

    def _edit(self, st, scores, history, layout, t):
        """the logits processors of step t on `scores` (csrc/logits.hip): the row's history holds positions 0 .. t.
        Whether eos is banned is a host constant of the unrolled step, like every other length here."""
        p, n, min_len, min_new, sup = st["proc"]
        cur = t + 1
        no_eos = cur < min_len or cur - st["n_prompt"] < min_new
        if p == 1.0 and n == 0 and not no_eos and not sup:
            return
        K.logits_process(scores, history, cur, repetition_penalty=p, no_repeat_ngram_size=n, suppress_eos=no_eos,
                         eos=self.config.text.sep_token_id, suppress=st["suppress"] if sup else None,
                         n_suppress=len(sup), history_layout=layout)

    def _state(self, mode, B, steps, dev, proc=None):
        """the device buffers of one (mode and its parameters, batch, steps, precision): static inputs, caches and
        workspaces for B * mode.rows decoder rows, then what the mode adds (mode.buffers); with logits processors also
        the suppress list and, where the mode has none, the fp32 logits of one step. Where the mode allows it (greedy
        generate) more than 32 rows get the wide LM head's workspace; such a state is large (its graph holds the
        cross-attention K|V of every row), so the cached states and their graphs go before its buffers are allocated"""
        dt = self.compute_dtype
        key = mode.key(B, steps, dt, str(dev)) + self._proc_key(proc)
        st = self._states.get(key)
        if st is not None:
            return st
        R = B * mode.rows
        wide = bool(mode.wide_ok) and R > 32
        if wide:
            self._states.clear()
        vc, tc = self.config.vision, self.config.text
        E, H = tc.hidden_size, tc.num_attention_heads
        Li = (vc.image_size // vc.patch_size) ** 2 + 1
        # mmfd_gemm runs products of fewer than 16 rows on its scalar path: the decoder's activations carry
        # at least 16 rows (the padding rows embed token 0 and are never selected, attended across or read)
        Bp = max(R, 16)
        st = dict(
            B=B, R=R, Bp=Bp, steps=steps, Li=Li, wide=wide,
            px=torch.zeros(B, vc.num_channels, vc.image_size, vc.image_size, device=dev),
            # token ids step-major: row t is what step t embeds (contiguous), row t + 1 what it selects
            seq=torch.zeros(steps + 1, Bp, dtype=torch.int64, device=dev),
            pos=torch.arange(steps + 1, dtype=torch.int64, device=dev)[:, None].expand(steps + 1, Bp).contiguous(),
            argmax=torch.zeros(R, dtype=torch.int64, device=dev),
            self_kv=[torch.zeros(Bp, steps, 2 * E, device=dev, dtype=dt) for _ in range(tc.num_hidden_layers)],
            cross_o=torch.zeros(Bp, E, device=dev, dtype=dt),  # cross-attention output: rows >= R stay 0
            graph=None, sig=None, n_forced=-1)
        need = max(K.lib().mmfd_attn_decode_workspace_bytes(B, H, E // H, Li),
                   K.lib().mmfd_attn_decode_workspace_bytes(R, H, E // H, Li),
                   K.lib().mmfd_attn_decode_workspace_bytes(Bp, H, E // H, steps), 16)
        st["attn_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        if wide:
            need = K.lib().mmfd_lm_head_argmax_wide_workspace_bytes(K.dtype_code(dt), R, tc.vocab_size, E)
            if need <= 0:
                raise ValueError(f"mmfd BLIP: the wide LM head kernel takes at most 256 rows and widths up to 1024, "
                                 f"got batch {B}, width {E}")
        else:
            need = K.lib().mmfd_lm_head_argmax_workspace_bytes(K.dtype_code(dt), R, tc.vocab_size, E)
            if need <= 0:
                raise ValueError(f"mmfd BLIP: the LM head kernel takes at most 32 rows and widths up to 1024 (fp32) / "
                                 f"2048 (bf16), got {R} rows, width {E}")
        st["lm_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        mode.buffers(self, st, dev)
        self._proc_buffers(st, proc, R, dev)
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

    def _run(self, st, n_forced, eager=False, logits=None, sc=None):
        """vision tower, cross K|V, then per step the decoder body and the mode's selection, all on the state's static
        buffers; steps t < n_forced take their next token from the prompt. eager: ask the mode after every step
        whether to stop (one host read). Returns the steps run. logits: forward_logits' sink [steps, B, V]. sc: the
        caller's context, so that an eager call builds one and not two"""
        mode = st["mode"]
        sc = sc or self._ctx()[0]
        cross = self._cross_kv(sc, self._vision(sc, st["px"]))
        for t in range(st["steps"]):
            g = self._hidden(sc, st, cross, t, mode.cache(st, t, n_forced), mode.rows)
            mode.select(self, sc, st, g, t, n_forced, None if logits is None else logits[t])
            if eager and mode.stop(st, t, n_forced):
                return t + 1
        return st["steps"]

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
                 length_penalty=1.0, early_stopping=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0,
                 num_return_sequences=1, seed=None, row_offset=0, repetition_penalty=1.0, no_repeat_ngram_size=0,
                 min_length=0, min_new_tokens=0, suppress_tokens=None):
        """Captions, greedy (num_beams=1) or by beam search (below). Greedy: int64 [B, P + n] ids (the prompt, bos first, then n <= max_new_tokens generated
        tokens: a row that produced sep_token_id is padded with pad_token_id, and n is where the last row
        stopped) — the array transformers' `generate(pixel_values, input_ids)` returns by default.
        `input_ids`: an optional prompt shared by all rows, fed one token per step in place of the argmax.
        use_graph: replay one captured HIP graph of all steps and trim on the host; else run eagerly and
        stop once every row has finished.
        Greedy decoding takes up to 128 rows per call (MAX_GREEDY_ROWS): up to 32 on kernels.lm_head_argmax, 33 ..
        128 on kernels.lm_head_argmax_wide, whose logits are bit for bit those of the narrow kernel on the row's
        32-row block, so the LM head never makes a caption depend on how many images share the call. (The kernel
        takes 256 rows; `generate` stops at 128 because a 256-row call of the default model did not complete on an
        MI355X and the cause is not known: DESIGN.md, "Captioning".) A state of more than 32 rows is large (5.4 GB
        of cross-attention K|V at 128 rows in fp32): creating one drops the other cached states and their graphs
        first. Beam search, sampling and forward_logits keep 32 rows.
        num_beams in 2 .. 8 (num_beams * batch <= 32, the LM head's rows): transformers' beam search with
        `length_penalty` and `early_stopping` (False or True), no sampling, one returned sequence per image — the
        array `generate(pixel_values, input_ids, num_beams=..., length_penalty=..., early_stopping=...,
        max_new_tokens=...)` returns there, unused positions filled as transformers fills them
        (`pad_token_id or sep_token_id`). `self.sequences_scores` then holds the fp32 scores [B] of the returned
        hypotheses. Among equal scores the lower beam, then the lower token wins (torch.topk leaves that open).
        do_sample=True: transformers' sampling — `temperature`, `top_k` (0: off) and `top_p` (1: off) filters in
        that order, then one draw per row and step (csrc/sample.hip) — with `num_return_sequences` = n samples per
        image: int64 [B * n, P + len], rows b*n .. b*n + n - 1 being the samples of image b (the vision tower and the
        cross-attention K|V run once per image), padded like the greedy result; B * n <= 32. The draw of row r at
        decoder step t is u = (mmfd_hash(seed, t, row_offset + r) >> 8) * 2^-24 (t counts the prompt's steps too):
        a pure function of its arguments, so a call is reproducible, and a batch cut into chunks that pass their
        first global row as `row_offset` draws what the whole batch would. seed=None takes one from torch's global
        CPU generator (torch.manual_seed makes the call reproducible); `self.sample_seed` holds the seed used. A
        new seed replays the captured graph. num_beams > 1 together with do_sample is refused.
        Logits processors, in all three modes, with transformers' names, defaults (off) and rules, applied on the
        device (csrc/logits.hip) from each row's own history, the prompt included:
        `repetition_penalty` p > 0: the score s of every id the row already holds becomes s * p (s < 0) or s / p, once
        however often the id occurs; `no_repeat_ngram_size` n: an id that would complete an n-gram the row already
        holds is banned (-inf); `min_length` / `min_new_tokens`: sep_token_id is banned while the row holds fewer
        than min_length ids (prompt and bos counted) or fewer than min_new_tokens generated ones (either rule bans:
        where both are given and min_length > prompt + min_new_tokens, transformers lets min_new_tokens replace
        min_length); `suppress_tokens`: up to 64 ids banned at every step. The penalty comes first, the bans after it.
        Greedy decoding and sampling edit the raw logits (the sampling filters run afterwards, and a banned id has
        probability 0); beam search edits log_softmax(logits) of every running beam before the running score is
        added, as transformers does. min_new_tokens > max_new_tokens is accepted: the row runs to the last step. A
        new suppress list of the same length, like a new seed, replays the captured graph; the other values are
        launch constants and part of the graph's key."""
        tc = self.config.text
        B = int(pixel_values.shape[0])
        proc = K.check_processors(repetition_penalty, no_repeat_ngram_size, min_length, min_new_tokens, suppress_tokens,
                                  tc.vocab_size)
        if proc == (1.0, 0, 0, 0, ()):
            proc = None
        n_ret = num_return_sequences
        if int(n_ret) != n_ret or n_ret < 1:
            raise ValueError(f"num_return_sequences must be an integer >= 1, got {n_ret!r}")
        if do_sample:
            if num_beams != 1:
                raise ValueError("do_sample together with num_beams > 1 (beam sampling) is not implemented")
            K.check_sampling(temperature, top_k, top_p)
            if B * int(n_ret) > 32:
                raise ValueError(f"sampling needs batch * num_return_sequences <= 32 (the LM head kernel's rows), got "
                                 f"batch {B}, num_return_sequences {n_ret}")
        elif n_ret != 1:
            raise ValueError("num_return_sequences > 1 needs do_sample=True (one deterministic caption per image "
                             "otherwise)")
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
        if do_sample:
            mode = _Sample(self, int(n_ret), float(temperature), int(top_k), float(top_p), seed, int(row_offset))
        elif num_beams > 1:
            mode = _Beams(int(num_beams), float(length_penalty), bool(early_stopping))
        else:
            if B > self.MAX_GREEDY_ROWS:
                raise ValueError(f"greedy decoding takes at most {self.MAX_GREEDY_ROWS} rows per call, got batch {B}")
            mode = _Greedy(wide_ok=True)
        return self._decode(mode, sc, dev, px, prompt, int(max_new_tokens), bool(use_graph), proc)

    def _decode(self, mode, sc, dev, px, prompt, max_new_tokens, use_graph, proc):
        """the driver of every mode: the state, this call's inputs, then one replay of the captured graph of all
        steps (captured first where the state has none, or the weights or the prompt's length changed since) or an
        eager run that stops once the mode says so"""
        tc = self.config.text
        n_forced = len(prompt) - 1
        steps = n_forced + max_new_tokens
        if max_new_tokens < mode.min_new or steps < 1 or steps + 1 > tc.max_position_embeddings:
            raise ValueError(f"prompt ({len(prompt)}) + max_new_tokens ({max_new_tokens}) must lie in "
                             f"[2, {tc.max_position_embeddings}]")
        st = self._state(mode, px.shape[0], steps, dev, proc)
        if tuple(px.shape) != tuple(st["px"].shape):
            raise ValueError(f"pixel_values must be {tuple(st['px'].shape)}, got {tuple(px.shape)}")
        st["px"].copy_(px)
        st["mode"] = mode  # (this call's: the seed and the row offset of a sampling call are not in the state's key)
        mode.begin(self, st, prompt)
        self._proc_begin(st, proc, len(prompt))
        ran = None
        if not use_graph:
            ran = self._run(st, n_forced, eager=True, sc=sc)
        else:
            if st["graph"] is None or st["sig"] != self._signature() or st["n_forced"] != n_forced:
                self._capture(st, n_forced, dev)
                mode.begin(self, st, prompt)
            st["graph"].replay()
        return mode.result(self, st, len(prompt), max_new_tokens, ran)

    def _capture(self, st, n_forced, dev):
        st["graph"] = None
        st["sig"], st["n_forced"] = self._signature(), n_forced
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            self._run(st, n_forced)  # warm up: weight shadows, packed biases, kernel attributes
        torch.cuda.current_stream(dev).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._run(st, n_forced)
        st["graph"] = g

    @torch.no_grad()
    def _forward_logits(self, pixel_values, forced_ids):
        sc, dev = self._ctx()
        ids = torch.as_tensor(forced_ids).to(dev).long()
        B, Tn = ids.shape
        if Tn + 1 > self.config.text.max_position_embeddings:
            raise ValueError("forced_ids is longer than the position table")
        mode = _Greedy()
        st = self._state(mode, B, Tn, dev)
        st["px"].copy_(pixel_values.to(dev).float())
        st["mode"] = mode
        mode.begin(self, st, ids.t())
        logits = torch.empty(Tn, B, self.config.text.vocab_size, device=dev, dtype=torch.float32)
        self._run(st, Tn, logits=logits, sc=sc)
        return logits

    def forward_logits(self, pixel_values, forced_ids):
        """the generation steps with every token forced: fp32 logits [T, B, V], logits[t] being step t's (what
        follows forced_ids[:, :t + 1]); forced_ids int64 [B, T]. The same kernels and caches as generate."""
        self._ctx()  # (refuses a call that would need gradients before no_grad hides it)
        return self._forward_logits(pixel_values, forced_ids)

    def forward(self, pixel_values, input_ids, attention_mask=None, labels=None, reduction="mean", return_logits=False):
        """Without `labels`: teacher-forced logits [T, B, V] (forward_logits); inference only.
        With `labels` (int64 [B, T], -100 = not scored): transformers' caption loss, CrossEntropy(logits[:, :-1],
        labels[:, 1:]) with config.text.label_smoothing, as a BlipCaptionLossOutput — `loss` the mean over the scored
        positions, or with reduction="none" the per-sequence sums [B]; `logits` [B, T, V] with return_logits.
        `attention_mask` [B, T] marks right padding (a row starting with padding, or with a token after padding, is
        refused). Under no_grad this works on any model. Under grad it needs BlipConfig.train_text_decoder: the loss
        is then one autograd node whose backward fills the gradient of every text_decoder parameter; the vision
        tower is frozen (its parameters receive None: hand the optimizer model.text_decoder.parameters())."""
        if labels is None:
            if attention_mask is not None or return_logits:
                raise ValueError("attention_mask / return_logits belong to the loss path: pass labels")
            return self.forward_logits(pixel_values, input_ids)
        return self._caption_loss(pixel_values, input_ids, attention_mask, labels, reduction, return_logits)

    # ---- caption loss: one pass over all positions -------------------------------------------------------
    def _causal_bias(self, T_, dev):
        """the shared additive bias [H, T, T] of the causal mask: 0 on and below the diagonal, CAUSAL_NEG above;
        built once per (T, device)"""
        H = self.config.text.num_attention_heads
        key = (H, T_, str(dev))
        b = self._causal.get(key)
        if b is None:
            if len(self._causal) >= 8:
                self._causal.clear()
            m = torch.triu(torch.full((T_, T_), CAUSAL_NEG, dtype=torch.float32, device=dev), diagonal=1)
            b = self._causal[key] = m[None].expand(H, T_, T_).contiguous()
        return b

    def _loss_inputs(self, input_ids, attention_mask, labels, dev):
        """host-side checks, then the device inputs of the pass: ids, positions, mask (or None) [Bp, T] and the
        shifted labels [Bp * T] (row b * T + t scores token t + 1; the last position of a row, the padding and the
        rows >= B are -100). Bp > B only when B * T < 16: mmfd_gemm runs fewer than 16 rows on its scalar path"""
        tc = self.config.text
        ids = torch.as_tensor(input_ids).long()
        lab = torch.as_tensor(labels).long()
        if ids.dim() != 2 or tuple(lab.shape) != tuple(ids.shape):
            raise ValueError(f"input_ids and labels must be [B, T], got {tuple(ids.shape)} and {tuple(lab.shape)}")
        B, T_ = ids.shape
        if not 2 <= T_ <= tc.max_position_embeddings:
            raise ValueError(f"the sequence length must lie in [2, {tc.max_position_embeddings}], got {T_}")
        ids_h = ids.cpu()
        if int(ids_h.min()) < 0 or int(ids_h.max()) >= tc.vocab_size:
            raise ValueError(f"input_ids outside [0, {tc.vocab_size})")
        K.check_vocab_labels(lab, tc.vocab_size)
        mask = None
        if attention_mask is not None:
            mask = (torch.as_tensor(attention_mask).cpu() != 0).long()
            if tuple(mask.shape) != (B, T_):
                raise ValueError(f"attention_mask must be {(B, T_)}, got {tuple(mask.shape)}")
            if bool((mask[:, 0] == 0).any()):
                raise ValueError("a row starts with padding: only right-padded batches are supported")
            if bool((mask[:, 1:] > mask[:, :-1]).any()):
                raise ValueError("a token follows padding: only right-padded batches are supported")
            # what lies under the padding is never attended by a scored position: it is replaced by pad_token_id, so
            # that no bit of the result depends on it (the embedding backward's summation order follows the sorted
            # ids, padding included)
            ids_h = torch.where(mask == 1, ids_h, torch.full_like(ids_h, tc.pad_token_id))
            if bool(mask.all()):
                mask = None
        Bp = B if B * T_ >= 16 else -(-16 // T_)
        ids_p = torch.zeros(Bp, T_, dtype=torch.int64)
        ids_p[:B] = ids_h
        lab_p = torch.full((Bp, T_), K.IGNORE_INDEX, dtype=torch.int64)
        lab_p[:B, :-1] = lab.cpu()[:, 1:]
        if mask is not None:
            mask_p = torch.ones(Bp, T_, dtype=torch.int64)
            mask_p[:B] = mask
            mask = mask_p.to(dev)
        pos = torch.arange(T_, dtype=torch.int64)[None].expand(Bp, T_).contiguous()
        return ids_p.to(dev), pos.to(dev), mask, lab_p.view(-1).to(dev)

    def _decoder_pass(self, sc, emb, ids, pos, mask, keep):
        """the decoder over all positions at once: (the LM head's input [Bp * T, E], what the backward reads or
        None). emb: the image tokens [Bp, Li, Dv]"""
        tc = self.config.text
        Bp, T_ = ids.shape
        E, H, eps, P = tc.hidden_size, tc.num_attention_heads, tc.layer_norm_eps, sc.P
        emb_args = (ids, pos, P[WORD + ".weight"], P[T + "embeddings.position_embeddings.weight"],
                    P[T + "embeddings.LayerNorm.weight"], P[T + "embeddings.LayerNorm.bias"], eps, sc.dt)
        if keep:
            s0, x, m0, r0 = K.embed_ln_train(*emb_args)
        else:
            x, s0, m0, r0 = K.embed_ln_infer(*emb_args), None, None, None
        kb = K.mask_to_bias(mask) if mask is not None else None
        causal = self._causal_bias(T_, ids.device)
        emb2d = Bk.as2d(emb)
        cross = self._cross_kv(sc, emb)  # per layer the image's packed K|V [Bp, Li, 2E]
        layers = []
        for i in range(tc.num_hidden_layers):
            p = f"{T}encoder.layer.{i}"
            o, _, attn = Bk.self_attn_fwd(sc, x, [p + n for n in QKV], Bp, H, keep=keep, planes=False, key_bias=kb,
                                          rel_bias=causal)
            s1, _ = Bk.linear(sc, Bk.as2d(o), p + ".attention.output.dense", residual=x)
            h, m1, r1 = Bk.layernorm(sc, s1, p + ".attention.output.LayerNorm", eps)
            cq, _ = Bk.linear(sc, h, p + ".crossattention.self.query")
            ckv = cross[i]
            cq = cq.view(Bp, T_, E)
            co, clse = K.attn_fwd(cq, ckv[..., :E], ckv[..., E:], H)  # every image key takes part
            s2, _ = Bk.linear(sc, Bk.as2d(co), p + ".crossattention.output.dense", residual=h)
            h2, m2, r2 = Bk.layernorm(sc, s2, p + ".crossattention.output.LayerNorm", eps)
            s3, ffn = Bk.ffn_fwd(sc, h2, p + ".intermediate.dense", p + ".output.dense", residual=h2, keep=keep,
                                 planes=False)
            x, m3, r3 = Bk.layernorm(sc, s3, p + ".output.LayerNorm", eps)
            if keep:
                layers.append(dict(attn=attn, o=o, s1=s1, m1=m1, r1=r1, h=h, cq=cq, ckv=ckv, co=co, clse=clse, s2=s2,
                                   m2=m2, r2=r2, ffn=ffn, s3=s3, m3=m3, r3=r3))
        # the head transform: dense + GELU (the pre-activation kept for the backward), then LayerNorm
        W = sc.w(HEAD + "transform.dense")
        pre = torch.empty((x.shape[0], E), device=x.device, dtype=sc.dt) if keep else None
        g = K.gemm(x, W, bias=sc.b(HEAD + "transform.dense"), act=K.ACT_GELU, aux=pre)
        gl, mg, rg = Bk.layernorm(sc, g, HEAD + "transform.LayerNorm", eps)
        st = dict(s0=s0, m0=m0, r0=r0, layers=layers, x=x, pre=pre, g=g, mg=mg, rg=rg, gl=gl, emb2d=emb2d, ids=ids,
                  Bp=Bp, T=T_) if keep else None
        return gl, st

    def _loss_forward(self, sc, dev, pixel_values, input_ids, attention_mask, labels, keep, eps):
        """the vision tower (never kept: frozen), the decoder pass, the logits of all Bp * T rows and the loss
        kernels with label smoothing eps: a dict of device tensors and, with `keep`, the backward's state"""
        tc = self.config.text
        ids, pos, mask, lab = self._loss_inputs(input_ids, attention_mask, labels, dev)
        Bp, T_ = ids.shape
        B = int(torch.as_tensor(input_ids).shape[0])
        px = pixel_values.to(dev).float().contiguous()
        if px.shape[0] != B:
            raise ValueError(f"pixel_values holds {px.shape[0]} images, input_ids {B} rows")
        emb = self._vision(sc, px)
        if Bp > B:
            pad = torch.zeros((Bp,) + tuple(emb.shape[1:]), device=dev, dtype=emb.dtype)
            pad[:B] = emb
            emb = pad
        gl, st = self._decoder_pass(sc, emb, ids, pos, mask, keep)
        V = tc.vocab_size
        logits = torch.empty((gl.shape[0], vocab_ld(V)), device=dev, dtype=torch.float32)[:, :V]  # [Bp * T, V]
        K.gemm(gl, sc.w(WORD), bias=sc.P[HEAD + "bias"], out=logits)
        rows, lse, lse_lo, mean, n_valid, seq = K.vocab_xent_fwd(logits, lab, eps, rows_per_seq=T_,
                                                                 check_labels=False)
        out = dict(B=B, T=T_, eps=eps, logits=logits, labels=lab, lse=lse, lse_lo=lse_lo, mean=mean, n_valid=n_valid,
                   seq=seq)
        return out, st

    def _loss_backward(self, sc, out, st, reduction, dout):
        """fills sc.grads with the gradient of every text_decoder parameter (fp32), in a fixed order"""
        tc = self.config.text
        E, H, eps = tc.hidden_size, tc.num_attention_heads, tc.layer_norm_eps
        Bp, T_, B = st["Bp"], st["T"], out["B"]
        dev = out["logits"].device
        V = tc.vocab_size
        Vp = vocab_ld(V)
        # 1. dlogits in the compute dtype, in vocab_ld(V) columns: the vocabulary is the K of one LM-head product and
        #    the M of the other, and the columns past V are zeros, so they add nothing to either
        dl = torch.empty((Bp * T_, Vp), device=dev, dtype=sc.dt)
        if Vp > V:
            dl[:, V:].zero_()
        xent = (out["logits"], out["labels"], out["lse"], out["lse_lo"], out["eps"], sc.dt)
        if reduction == "mean":
            K.vocab_xent_bwd(*xent, upstream=dout.reshape(1).float().contiguous(), n_valid=out["n_valid"], out=dl[:, :V])
        else:
            up = torch.zeros(Bp, device=dev, dtype=torch.float32)
            up[:B] = dout.float()
            K.vocab_xent_bwd(*xent, upstream=up, rows_per_seq=T_, out=dl[:, :V])
        # 2. the LM head: dG = dlogits W; dW = dlogits^T G and d(bias) = column sums, into the fp32 gradient of the
        #    tied table (the embedding scatter is added to it at the end: one fixed order). With Vp > V the table is
        #    copied into Vp rows, the last ones zero, and the gradients are the first V rows of Vp-row buffers
        Wv = sc.w(WORD)
        if Vp > V:
            Wv = torch.empty((Vp, E), device=dev, dtype=sc.dt)
            K.cast(sc.P[WORD + ".weight"], sc.dt, out=Wv[:V])
            Wv[V:].zero_()
        gword = torch.empty((Vp, E), device=dev, dtype=torch.float32)
        gbias = torch.empty(Vp, device=dev, dtype=torch.float32)
        K.gemm(dl, st["gl"], trans_a=True, trans_b=True, out=gword, a_rowsum=gbias)
        gword, gbias = gword[:V], gbias[:V]
        sc.grads[WORD + ".weight"], sc.grads[HEAD + "bias"] = gword, gbias
        dgl = Bk.linear_dx(sc, dl, Wv)
        del dl, Wv
        # 3. the head transform
        dg, _ = Bk.layernorm_bwd(sc, dgl, st["g"], HEAD + "transform.LayerNorm", st["mg"], st["rg"])
        dpre = K.act_bwd(dg, st["pre"], K.ACT_GELU)
        sc.lin_grads([HEAD + "transform.dense"], dpre, st["x"])
        dx = Bk.linear_dx(sc, dpre, HEAD + "transform.dense")
        # 4. the layers in reverse
        for i in reversed(range(tc.num_hidden_layers)):
            p = f"{T}encoder.layer.{i}"
            ls = st["layers"][i]
            ds3, _ = Bk.layernorm_bwd(sc, dx, ls["s3"], p + ".output.LayerNorm", ls["m3"], ls["r3"])
            dh2 = Bk.ffn_bwd(sc, ds3, None, ls["ffn"], residual=ds3)
            ds2, _ = Bk.layernorm_bwd(sc, dh2, ls["s2"], p + ".crossattention.output.LayerNorm", ls["m2"], ls["r2"])
            dco = Bk.attn_out_bwd(sc, p + ".crossattention.output.dense", ds2, None, ls["co"], None)
            ckv = ls["ckv"]
            dkv = torch.empty_like(ckv)
            dcq, _, _ = K.attn_bwd(ls["cq"], ckv[..., :E], ckv[..., E:], ls["co"], ls["clse"], dco, H,
                                   dk=dkv[..., :E], dv=dkv[..., E:])
            # dK|dV reach the key / value projections, whose input is the saved image tokens; no gradient is
            # formed for the image tokens themselves (the vision tower is frozen)
            sc.lin_grads([p + n for n in CROSS_KV], Bk.as2d(dkv), st["emb2d"])
            sc.lin_grads([p + ".crossattention.self.query"], Bk.as2d(dcq), ls["h"])
            dh = Bk.linear_dx(sc, Bk.as2d(dcq), p + ".crossattention.self.query", residual=ds2)
            ds1, _ = Bk.layernorm_bwd(sc, dh, ls["s1"], p + ".attention.output.LayerNorm", ls["m1"], ls["r1"])
            do = Bk.attn_out_bwd(sc, p + ".attention.output.dense", ds1, None, ls["o"], None)
            dx = Bk.self_attn_bwd(sc, do, ls["attn"], residual=ds1)
        # 5. the embedding LayerNorm, then the scatter into the word table (on top of the LM-head term) and the
        #    position table
        dsum, _ = Bk.layernorm_bwd(sc, dx, st["s0"], T + "embeddings.LayerNorm", st["m0"], st["r0"])
        pname = T + "embeddings.position_embeddings.weight"
        dpos = K.zeros(sc.P[pname].shape, device=dev)
        K.embed_bwd(st["ids"], None, dsum, gword, dpos, None, padding_idx=tc.pad_token_id)
        sc.grads[pname] = dpos

    def _caption_loss(self, pixel_values, input_ids, attention_mask, labels, reduction, return_logits,
                      label_smoothing=None):
        """forward(labels=); label_smoothing: a value to use in place of config.text.label_smoothing
        (Captioner.score: 0)"""
        tc = self.config.text
        eps = float(tc.label_smoothing if label_smoothing is None else label_smoothing)
        if reduction not in ("mean", "none"):
            raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
        if self.training and (tc.hidden_dropout_prob > 0 or tc.attention_probs_dropout_prob > 0):
            raise NotImplementedError("mmfd BLIP's caption loss supports the BLIP text configuration (dropout 0): "
                                      "call .eval() or set the text dropout probabilities to 0")
        named = [(n, p) for n, p in self.named_parameters() if n.startswith("text_decoder.")]
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if grad and not self.config.train_text_decoder:
            self._ctx()  # raises the inference-only error
        if grad:
            loss, logits = _BlipLossFn.apply(self, [n for n, _ in named], pixel_values, input_ids, attention_mask, labels,
                                             reduction, bool(return_logits), eps, *[p for _, p in named])
            return BlipCaptionLossOutput(loss=loss, logits=logits if return_logits else None)
        with torch.no_grad():
            sc, dev = self._ctx()
            out, _ = self._loss_forward(sc, dev, pixel_values, input_ids, attention_mask, labels, False, eps)
        return BlipCaptionLossOutput(loss=self._pick_loss(out, reduction), logits=self._pick_logits(out, return_logits))

    @staticmethod
    def _pick_loss(out, reduction):
        return out["mean"] if reduction == "mean" else out["seq"][:out["B"]]

    @staticmethod
    def _pick_logits(out, return_logits):
        if not return_logits:
            return None
        B, T_ = out["B"], out["T"]
        return out["logits"][:B * T_].contiguous().view(B, T_, -1)  # (a copy only where vocab_ld(V) > V)


class _BlipLossFn(torch.autograd.Function):
    """the caption loss of a model with train_text_decoder as one autograd node over the text_decoder parameters"""

    @staticmethod
    def forward(fctx, model, names, pixel_values, input_ids, attention_mask, labels, reduction, return_logits, eps,
                *params):
        sc, dev = model._ctx(train=True)
        out, st = model._loss_forward(sc, dev, pixel_values, input_ids, attention_mask, labels, True, eps)
        fctx.sc, fctx.st, fctx.out, fctx.model, fctx.names, fctx.reduction = sc, st, out, model, names, reduction
        loss = model._pick_loss(out, reduction).clone()
        logits = model._pick_logits(out, return_logits)
        if logits is None:
            logits = loss.new_empty(0)
        fctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(fctx, dloss, _dlogits):
        sc = fctx.sc
        if sc is None:
            raise RuntimeError("mmfd BLIP: the caption loss was already backpropagated (its saved state is dropped)")
        sc.enable_side_stream(dloss.device)
        fctx.model._loss_backward(sc, fctx.out, fctx.st, fctx.reduction, dloss)
        sc.join_side()
        grads = [sc.grads.get(n) for n in fctx.names]
        fctx.sc = fctx.st = fctx.out = None
        return (None,) * 9 + tuple(grads)
