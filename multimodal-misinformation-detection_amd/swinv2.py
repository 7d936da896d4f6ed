"""Swinv2 image encoder on HIP kernels — the reference's default image encoder
(`Swinv2Model.from_pretrained("microsoft/swinv2-base-patch4-window8-256")`, train.py:332, called
with `.last_hidden_state` at train.py:142-143 and preprocess_embeddings.py:91-92: [B,3,256,256] ->
[B,64,1024]).

HF parameter names (a hub / transformers state_dict loads unchanged) and HF's arithmetic
(transformers modeling_swinv2.py, restated in oracle/swinv2.py): 4x4 patch conv -> LayerNorm; per
stage `depth` blocks of shifted-window cosine attention with res-post-norm

    h = x + LN_before(W_o . attn(x));   x = h + LN_after(W_2 . gelu(W_1 . h))
    attn: softmax(cos(q_h, k_h) * exp(min(logit_scale_h, ln 100)) + 16 sigmoid(cpb_mlp[rpi]) + 2 mask)

(odd blocks roll the grid by -window/2 first; the mask separates the rolled-in regions and HF adds
it twice), then 2x2 patch merging (concat 4 neighbours -> Linear(4C, 2C, no bias) -> LN); the model
ends in a LayerNorm. Windows never exceed the stage's resolution (window = min(res, 8), no shift
when res <= window).

MI355X mapping: tokens stay `[B*R*R, C]` rows; every block's attention runs over the rows in that
block's (shifted) window order, so the per-token GEMMs / LayerNorms run on the permuted rows as
they are and the only data movement is ONE `mmfd_row_gather` per block that composes the previous
block's order with the next one (roll + window_partition + window_reverse + roll back in a single
pass), and one for each patch merge (which reads the 2x2 neighbours straight out of window order).
QKV is one packed GEMM; the cosine normalisation and the per-head logit scale happen inside the
attention kernel while it stages K and the query fragments (bf16; the fp32 parity mode uses one
in-place pass over the packed rows, `mmfd_swin_qk_norm`); the continuous position bias (+ shift mask) is computed once per block into a
[nW, H, 64, 64] fp32 table that the flash-attention kernel reads with a batch modulus
(`rel_bias_mod`): windows are batch-major per image, so window w of every image shares bias row w.
By default inference only (the reference freezes its encoders, train.py:335-340, and the
pre-embedding pass runs under no_grad): a forward that would need gradients raises.

With `Swinv2Config(trainable=True)` a forward under grad runs as ONE autograd node (`_Swinv2Fn`, shaped
like deberta._DebertaFn) whose backward is `swinv2_backward`. Under grad each block's attention is
"normalise first, then the attention that already has a backward": packed QKV GEMM, the separate
cosine pass in BOTH dtypes in its training form (`mmfd_swin_qk_norm_train`: the same results, plus
the inverse norms), then plain `mmfd_attn_fwd` with scale 1 and the block's bias, so dQ / dK / dV
come from `mmfd_attn_bwd`. New in the backward: the bias gradient summed over the windows that share a
bias row (`mmfd_attn_bwd_bias_sum`), the cosine pass's adjoint with the logit-scale gradient
(`mmfd_swin_qk_norm_bwd`), and the bias construction's (`mmfd_swin_bias_bwd`, `mmfd_swin_cpb_bwd`).
Every row gather of the forward is a bijection on rows (the 2x2 patch merge too: each source row lands
in one (output row, group) slot), so its adjoint is `mmfd_row_gather` with the inverse table. Under
no_grad / eval a trainable model launches the frozen model's kernels in the frozen model's order and
is bit-identical to it (bf16: the fused cosine forward). In bf16 the training forward therefore
differs from the eval forward by the rounding of the normalised operands to bf16, at most
delta_h = exp(min(logit_scale_h, ln 100)) * 2^-8 per logit (the bound
tests/test_swinv2_gpu.py::test_attention_fused_cosine_matches_separate_pass holds). Gradients flow
through `last_hidden_state` only (`pooler_output` is returned detached under grad; pixels take no
gradient). Stochastic depth is not implemented (HF's Swinv2Config default drop_path_rate is 0.1 and
acts in training mode): a trainable model in training mode needs drop_path_rate = 0.
"""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn as nn

from . import blocks as Bk
from . import kernels as K
from .encoders import EncoderOutput


@dataclass
class Swinv2Config:
    """microsoft/swinv2-base-patch4-window8-256 defaults"""
    image_size: int = 256
    patch_size: int = 4
    num_channels: int = 3
    embed_dim: int = 128
    depths: tuple = (2, 2, 18, 2)
    num_heads: tuple = (4, 8, 16, 32)
    window_size: int = 8
    mlp_ratio: float = 4.0
    qkv_bias: bool = True
    layer_norm_eps: float = 1e-5
    pretrained_window_sizes: tuple = (0, 0, 0, 0)
    # fine-tuning (opt-in): with trainable=False the model is inference-only exactly as before
    trainable: bool = False
    drop_path_rate: float = 0.0                 # (HF default 0.1; only 0 is implemented for training)


MAX_LOG = math.log(1.0 / 0.01)                  # the logit-scale clamp (Swinv2SelfAttention.forward)
PATCH_W = "embeddings.patch_embeddings.projection.weight"

# ------------------------------------------------------------------------------------------------
# host-side geometry (constants per (resolution, window, shift); cached on the device)
# ------------------------------------------------------------------------------------------------
def stage_geometry(cfg: Swinv2Config):
    """[(R, dim, heads, [(window, shift) per block])] per stage (Swinv2Encoder / Swinv2Layer
    _compute_window_shift)"""
    R = cfg.image_size // cfg.patch_size
    out = []
    for i, depth in enumerate(cfg.depths):
        Ri = R // (2 ** i)
        ws = min(Ri, cfg.window_size)
        blocks = []
        for j in range(depth):
            shift = 0 if (j % 2 == 0) else cfg.window_size // 2
            if Ri <= ws:
                shift = 0
            blocks.append((ws, shift))
        out.append((Ri, int(cfg.embed_dim * 2 ** i), cfg.num_heads[i], blocks))
    return out


def window_order(R, ws, shift):
    """natural raster index of every row in (rolled by -shift) window order: window (wy, wx)
    batch-major, tokens row-major inside the window (torch.roll + window_partition)"""
    n = R // ws
    wy, wx, iy, ix = np.meshgrid(np.arange(n), np.arange(n), np.arange(ws), np.arange(ws), indexing="ij")
    y = (wy * ws + iy + shift) % R
    x = (wx * ws + ix + shift) % R
    return (y * R + x).reshape(-1).astype(np.int64)


def shift_mask(R, ws, shift):
    """[nW, L, L] fp32: 0 within a cyclic-shift region, -100 across (Swinv2Layer.get_attn_mask)"""
    idx = np.arange(R)
    reg = (idx >= R - ws).astype(np.int64) + (idx >= R - shift).astype(np.int64)
    img = reg[:, None] * 3 + reg[None, :]                         # label on the rolled grid
    n = R // ws
    lab = img.reshape(n, ws, n, ws).transpose(0, 2, 1, 3).reshape(n * n, ws * ws)
    m = lab[:, None, :] - lab[:, :, None]
    return np.where(m != 0, -100.0, 0.0).astype(np.float32)


def coords_table_and_index(ws, pretrained_ws=0):
    """(relative_coords_table [(2ws-1)^2, 2] fp32, relative_position_index int32 [ws^2 * ws^2])
    as Swinv2SelfAttention.create_coords_table_and_index (computed with torch on the host)"""
    rh = torch.arange(-(ws - 1), ws, dtype=torch.int64).float()
    t = torch.stack(torch.meshgrid([rh, rh], indexing="ij")).permute(1, 2, 0).contiguous().unsqueeze(0)
    if pretrained_ws > 0:
        t[:, :, :, 0] /= pretrained_ws - 1
        t[:, :, :, 1] /= pretrained_ws - 1
    elif ws > 1:
        t[:, :, :, 0] /= ws - 1
        t[:, :, :, 1] /= ws - 1
    t *= 8
    t = torch.sign(t) * torch.log2(torch.abs(t) + 1.0) / math.log2(8)
    c = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return t.reshape(-1, 2).float(), rel.sum(-1).reshape(-1).to(torch.int32)


class _Geo:
    """device-resident index tables / masks, built once per (device, config)"""

    def __init__(self, dev):
        self.dev = dev
        self._c = {}

    def get(self, key, make):
        t = self._c.get(key)
        if t is None:
            t = self._c[key] = make()
        return t

    def idx(self, arr):
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(self.dev)


# ------------------------------------------------------------------------------------------------
# module tree (HF names)
# ------------------------------------------------------------------------------------------------
def _linear(i, o, bias=True):
    return nn.Linear(i, o, bias=bias)


class Swinv2Model(Bk.CachedWeights, nn.Module):
    def __init__(self, config: Swinv2Config | None = None, **kw):
        super().__init__()
        c = config or Swinv2Config(**kw)
        self.config = c
        eps = c.layer_norm_eps
        self.embeddings = nn.Module()
        self.embeddings.patch_embeddings = nn.Module()
        self.embeddings.patch_embeddings.projection = nn.Conv2d(c.num_channels, c.embed_dim, c.patch_size,
                                                                stride=c.patch_size)
        self.embeddings.norm = nn.LayerNorm(c.embed_dim, eps=eps)
        self.encoder = nn.Module()
        self.encoder.layers = nn.ModuleList()
        geo = stage_geometry(c)
        for i, (R, dim, H, blocks) in enumerate(geo):
            st = nn.Module()
            st.blocks = nn.ModuleList()
            for _ in blocks:
                b = nn.Module()
                b.attention = nn.Module()
                s = b.attention.self = nn.Module()
                s.logit_scale = nn.Parameter(torch.log(10 * torch.ones((H, 1, 1))))
                s.continuous_position_bias_mlp = nn.Sequential(nn.Linear(2, 512, bias=True), nn.ReLU(inplace=True),
                                                               nn.Linear(512, H, bias=False))
                s.query = _linear(dim, dim, c.qkv_bias)
                s.key = _linear(dim, dim, False)
                s.value = _linear(dim, dim, c.qkv_bias)
                b.attention.output = nn.Module()
                b.attention.output.dense = _linear(dim, dim)
                b.layernorm_before = nn.LayerNorm(dim, eps=eps)
                b.intermediate = nn.Module()
                b.intermediate.dense = _linear(dim, int(c.mlp_ratio * dim))
                b.output = nn.Module()
                b.output.dense = _linear(int(c.mlp_ratio * dim), dim)
                b.layernorm_after = nn.LayerNorm(dim, eps=eps)
                st.blocks.append(b)
            if i < len(geo) - 1:
                st.downsample = nn.Module()
                st.downsample.reduction = _linear(4 * dim, 2 * dim, False)
                st.downsample.norm = nn.LayerNorm(2 * dim, eps=eps)
            self.encoder.layers.append(st)
        nf = int(c.embed_dim * 2 ** (len(c.depths) - 1))
        self.layernorm = nn.LayerNorm(nf, eps=eps)
        self.num_features = nf
        self.compute_dtype = torch.float32
        self._geo = {}
        self._init_weights()

    def _init_weights(self, std=0.02):
        """Swinv2PreTrainedModel._init_weights: normal(0, 0.02) Linear/Conv, zero bias, LN 1/0"""
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Conv2d)):
                nn.init.normal_(m.weight, 0.0, std)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def set_precision(self, precision):
        self.compute_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[precision]
        return self

    def forward(self, pixel_values, **unused):
        params = dict(self.named_parameters())
        first = next(iter(params.values()))
        if not first.is_cuda:
            raise RuntimeError("mmfd Swinv2Model runs on the HIP device: call .to('cuda') first")
        c = self.config
        keep = torch.is_grad_enabled() and any(p.requires_grad for p in params.values())
        if keep and not c.trainable:
            raise NotImplementedError("mmfd Swinv2Model is inference-only (frozen encoder, train.py:335-340): "
                                      "call it under torch.no_grad() or freeze its parameters")
        if c.trainable and self.training and c.drop_path_rate > 0:
            raise NotImplementedError("mmfd Swinv2Model trains without stochastic depth only: set drop_path_rate "
                                      "to 0 (HF's default is 0.1)")
        geo = self._geo.get(str(first.device))
        if geo is None:
            geo = self._geo[str(first.device)] = _Geo(first.device)
        if keep:
            out = _Swinv2Fn.apply(self, list(params.keys()), geo, pixel_values, *params.values())
            # gradients flow through last_hidden_state only
            return EncoderOutput(last_hidden_state=out, extra={"pooler_output": K.seq_mean_fwd(out.detach())})
        P = {n: p.detach() for n, p in params.items()}
        P[PATCH_W] = P[PATCH_W].reshape(P[PATCH_W].shape[0], -1)   # conv as a [C_out, 3*p*p] GEMM weight
        ctx = Bk.StepCtx(P, self.compute_dtype, shadows=Bk.shadow_store(self))
        # frozen encoder: packed biases / position-bias tables persist (not for a trainable model: mmfd's
        # AdamW moves its parameters without bumping their version counters, see StepCtx.derived)
        ctx.cache_derived = not c.trainable
        out = swinv2_forward(self, ctx, geo, pixel_values)
        pooled = K.seq_mean_fwd(out)                               # Swinv2Model.pooler (AdaptiveAvgPool1d)
        return EncoderOutput(last_hidden_state=out, extra={"pooler_output": pooled})


def _inverse(table):
    """the inverse of a permutation table (host)"""
    out = np.empty_like(table)
    out[table] = np.arange(table.shape[0])
    return out


def swinv2_forward(model: Swinv2Model, ctx: Bk.StepCtx, geo: _Geo, pixel_values, st=None):
    """`st` (a dict, training): filled with what swinv2_backward reads — st["tape"] lists the row
    gathers (with their inverse tables, built on the host and cached in `geo` like the forward ones, so
    they exist before any graph capture), blocks and patch merges in forward order"""
    cfg = model.config
    keep = st is not None
    tape = st.setdefault("tape", []) if keep else None
    dev = ctx.P["layernorm.weight"].device
    px = pixel_values.to(dev)
    B, Cin, Hh, Ww = px.shape
    p = cfg.patch_size
    if Hh != cfg.image_size or Ww != cfg.image_size or Cin != cfg.num_channels:
        raise ValueError(f"Swinv2Model expects [B,{cfg.num_channels},{cfg.image_size},{cfg.image_size}] pixels, "
                         f"got {tuple(px.shape)}")
    eps = cfg.layer_norm_eps
    dt = ctx.dt
    # embeddings: conv 4x4/4 as patchify + GEMM, then LayerNorm (dropout is identity in eval)
    patches = K.patchify(px.float().contiguous(), p, dt)        # [B*R*R, 3*p*p]
    s0, _ = Bk.linear(ctx, patches, "embeddings.patch_embeddings.projection")
    x, m0, r0 = Bk.layernorm(ctx, s0, "embeddings.norm", eps)
    if keep:
        st.update(B=B, patches=patches, s0=s0, m0=m0, r0=r0)
    stages = stage_geometry(cfg)
    for i, (R, dim, H, blocks) in enumerate(stages):
        d = dim // H
        order = np.arange(R * R)                                # natural index of each row
        inv = np.arange(R * R)
        for j, (ws, shift) in enumerate(blocks):
            pre = f"encoder.layers.{i}.blocks.{j}"
            L = ws * ws
            nW = (R // ws) ** 2
            tgt = window_order(R, ws, shift)
            if not np.array_equal(tgt, order):
                idx = geo.get(("perm", i, j), lambda: geo.idx(inv[tgt]))
                x = K.row_gather(x, idx, B, R * R)
                if keep:
                    tape.append(("gather", geo.get(("perm^-1", i, j), lambda: geo.idx(_inverse(inv[tgt]))), R * R))
                order = tgt
                inv = np.empty_like(order)
                inv[order] = np.arange(R * R)
            if keep:
                x, bs = _swin_block_train(ctx, geo, x, pre, B, R, dim, H, d, ws, shift, nW, L, eps, cfg)
                tape.append(("block", bs))
            else:
                x = _swin_block(ctx, geo, x, pre, B, R, dim, H, d, ws, shift, nW, L, eps, cfg)
        if i < len(stages) - 1:
            # patch merging: out (y2, x2) = [x(2y2,2x2), x(2y2+1,2x2), x(2y2,2x2+1), x(2y2+1,2x2+1)]
            R2 = R // 2
            y2, x2 = np.meshgrid(np.arange(R2), np.arange(R2), indexing="ij")
            y2, x2 = y2.reshape(-1), x2.reshape(-1)
            nat = np.stack([(2 * y2) * R + 2 * x2, (2 * y2 + 1) * R + 2 * x2, (2 * y2) * R + 2 * x2 + 1,
                            (2 * y2 + 1) * R + 2 * x2 + 1], axis=1).reshape(-1)
            idx = geo.get(("merge", i), lambda: geo.idx(inv[nat]))
            xm = K.row_gather(x, idx, B, R2 * R2, G=4)            # [B*R2*R2, 4*dim]
            pre = f"encoder.layers.{i}.downsample"
            sm, _ = Bk.linear(ctx, xm, pre + ".reduction")
            x, mm, rm = Bk.layernorm(ctx, sm, pre + ".norm", eps)
            if keep:
                # each source row lands in exactly one (output row, group) slot: the adjoint is a G = 1
                # gather on the merged gradient viewed as [B*R2*R2*4, dim]
                back = geo.get(("merge^-1", i), lambda: geo.idx(_inverse(inv[nat])))
                tape.append(("merge", MergeState(back, R * R, dim, pre, xm, sm, mm, rm)))
        elif not np.array_equal(order, np.arange(R * R)):
            idx = geo.get(("final", i), lambda: geo.idx(inv[np.arange(R * R)]))
            x = K.row_gather(x, idx, B, R * R)
            if keep:
                tape.append(("gather", geo.get(("final^-1", i), lambda: geo.idx(_inverse(inv))), R * R))
    y, mf, rf = Bk.layernorm(ctx, x, "layernorm", eps)
    if keep:
        st.update(x_last=x, mf=mf, rf=rf)
    Rl = stages[-1][0]
    return y.view(B, Rl * Rl, -1)


# x: the block's input rows; qkv [B*nW, L, 3*dim]: the normalised packed projections (q scaled), inv
# [rows, 2, H]: their inverse norms; table [T, H] / rb: the position-bias table and the attention's
# rel_bias; (y, m1, r1), (m, m2, r2): the two res-post-norm LayerNorms' inputs and statistics
SwinBlockState = namedtuple("SwinBlockState", "pre x qkv inv table rb coords rpi o lse y m1 r1 ffn m m2 r2 H d L")
# back: inverse gather table; rows: source rows per image; xm: merged rows; (s, m, r): the norm's input / stats
MergeState = namedtuple("MergeState", "back rows dim pre xm s m r")
SWIN_QKV = (".attention.self.query", ".attention.self.key", ".attention.self.value")


def _cpb_names(s):
    return [s + ".continuous_position_bias_mlp.0.weight", s + ".continuous_position_bias_mlp.0.bias",
            s + ".continuous_position_bias_mlp.2.weight"]


def _swin_block_train(ctx, geo, x, pre, B, R, dim, H, d, ws, shift, nW, L, eps, cfg):
    """_swin_block under grad, both dtypes: the cosine pass on the packed rows in its training form, then
    plain attention (scale 1, the block's bias) — the form mmfd_attn_bwd differentiates"""
    s = pre + ".attention.self"
    qkv = Bk.linear_packed(ctx, x, [pre + n for n in SWIN_QKV])              # [N, 3*dim]
    _, inv = K.swin_qk_norm_train(qkv, H, d, ctx.P[s + ".logit_scale"], MAX_LOG)
    pws = cfg.pretrained_window_sizes[int(pre.split(".")[2])]
    coords, rpi = geo.get(("cpb", ws, pws), lambda: tuple(t.to(geo.dev) for t in coords_table_and_index(ws, pws)))
    mask = None
    if shift > 0:
        mask = geo.get(("mask", R, ws, shift), lambda: torch.from_numpy(shift_mask(R, ws, shift)).to(geo.dev))
    table = K.swin_cpb(coords, *[ctx.P[n] for n in _cpb_names(s)])
    bias = K.swin_bias(table, rpi, L, mask)
    rb = bias if shift > 0 else bias.view(H, L, L)
    q3 = qkv.view(B * nW, L, 3 * dim)
    o, lse = K.attn_fwd(q3[..., :dim], q3[..., dim:2 * dim], q3[..., 2 * dim:], H, scale=1.0, rel_bias=rb)
    y, _ = Bk.linear(ctx, Bk.as2d(o), pre + ".attention.output.dense")
    h, m1, r1 = K.layernorm_fwd_res(y, ctx.P[pre + ".layernorm_before.weight"], ctx.P[pre + ".layernorm_before.bias"],
                                    eps, res=x, stats=True)
    m, ffn = Bk.ffn_fwd(ctx, h, pre + ".intermediate.dense", pre + ".output.dense", residual=None, keep=True,
                        planes=False)
    out, m2, r2 = K.layernorm_fwd_res(m, ctx.P[pre + ".layernorm_after.weight"], ctx.P[pre + ".layernorm_after.bias"],
                                      eps, res=h, stats=True)
    return out, SwinBlockState(pre, x, q3, inv, table, rb, coords, rpi, o, lse, y, m1, r1, ffn, m, m2, r2, H, d, L)


def _swin_block_bwd(ctx, dout, bs: SwinBlockState):
    """gradient of the block's input rows from that of its output rows; parameter gradients into ctx.grads"""
    pre, H, d, L = bs.pre, bs.H, bs.d, bs.L
    s = pre + ".attention.self"
    dim = H * d
    # out = h + LN_after(FFN(h)),  h = x + LN_before(Wo attn(x)): the residual gradients pass straight through
    dm, _ = Bk.layernorm_bwd(ctx, dout, bs.m, pre + ".layernorm_after", bs.m2, bs.r2)
    dh = Bk.ffn_bwd(ctx, dm, None, bs.ffn, residual=dout)
    dy, _ = Bk.layernorm_bwd(ctx, dh, bs.y, pre + ".layernorm_before", bs.m1, bs.r1)
    do = Bk.attn_out_bwd(ctx, pre + ".attention.output.dense", dy, None, bs.o, None)
    q3 = bs.qkv
    q, k, v = q3[..., :dim], q3[..., dim:2 * dim], q3[..., 2 * dim:]
    dqkv = torch.empty_like(q3)
    delta = torch.empty((q3.shape[0], H, L), device=q3.device, dtype=torch.float32)
    K.attn_bwd(q, k, v, bs.o, bs.lse, do, H, dq=dqkv[..., :dim], dk=dqkv[..., dim:2 * dim], dv=dqkv[..., 2 * dim:],
               scale=1.0, rel_bias=bs.rb, delta=delta)
    # the bias: summed over the windows that share a row, then through 16 sigmoid(.) and the MLP
    # (the modulus is named: with one image the nW windows ARE the batch, and [nW, H, L, L] would read as per-batch)
    dbias = K.attn_bwd_bias_sum(q, k, v, bs.o, bs.lse, do, H, delta, rel_bias=bs.rb, scale=1.0,
                                rel_bias_mod=bs.rb.shape[0] if bs.rb.dim() == 4 else None)
    dtable = K.swin_bias_bwd(dbias, bs.table, bs.rpi, L)
    cpb = _cpb_names(s)
    for n, g in zip(cpb, K.swin_cpb_bwd(dtable, bs.coords, *[ctx.P[n] for n in cpb])):
        ctx.grads[n] = g
    # the cosine pass, in place on the q and k thirds of the packed gradient
    d2 = Bk.as2d(dqkv)
    _, dls = K.swin_qk_norm_bwd(d2, Bk.as2d(q3), bs.inv, H, d, ctx.P[s + ".logit_scale"], MAX_LOG)
    ctx.grads[s + ".logit_scale"] = dls.view(H, 1, 1)
    names = [pre + n for n in SWIN_QKV]
    ctx.lin_grads(names, d2, bs.x)
    Wp, _ = ctx.w_packed(names)
    return Bk.linear_dx(ctx, d2, Wp, residual=dh)


def swinv2_backward(model: Swinv2Model, ctx: Bk.StepCtx, dout, st):
    """Gradients of every parameter into ctx.grads: the forward's tape in reverse (each entry's saved
    state is dropped as soon as it is used). Pixels take no gradient."""
    B = st["B"]
    dx, _ = Bk.layernorm_bwd(ctx, Bk.as2d(dout).contiguous(), st["x_last"], "layernorm", st["mf"], st["rf"])
    st["x_last"] = None
    tape = st["tape"]
    while tape:
        kind, *rec = tape.pop()
        if kind == "gather":
            dx = K.row_gather(dx, rec[0], B, rec[1])
        elif kind == "block":
            dx = _swin_block_bwd(ctx, dx, rec[0])
            ctx.flush_ready()
        else:
            ms = rec[0]
            ds, _ = Bk.layernorm_bwd(ctx, dx, ms.s, ms.pre + ".norm", ms.m, ms.r)
            ctx.lin_grads([ms.pre + ".reduction"], ds, ms.xm)
            dxm = Bk.linear_dx(ctx, ds, ms.pre + ".reduction")
            dx = K.row_gather(dxm.view(-1, ms.dim), ms.back, B, ms.rows)
            ctx.flush_ready()
        del rec
    ds0, _ = Bk.layernorm_bwd(ctx, dx, st["s0"], "embeddings.norm", st["m0"], st["r0"])
    ctx.lin_grads(["embeddings.patch_embeddings.projection"], ds0, st["patches"])
    ctx.flush_ready()


class _Swinv2Fn(torch.autograd.Function):
    @staticmethod
    def forward(fctx, model, names, geo, pixel_values, *params):
        sc = Bk.module_ctx(model, names, params)
        sc.P[PATCH_W] = sc.P[PATCH_W].reshape(sc.P[PATCH_W].shape[0], -1)   # conv as a [C_out, 3*p*p] GEMM weight
        st = {}
        out = swinv2_forward(model, sc, geo, pixel_values, st=st)
        fctx.sc, fctx.st, fctx.model, fctx.names = sc, st, model, names
        fctx.wshape = params[names.index(PATCH_W)].shape
        return out

    @staticmethod
    def backward(fctx, dout):
        i = fctx.names.index(PATCH_W)
        wshape = fctx.wshape
        grads = Bk.fn_backward(fctx, dout, lambda sc, d: swinv2_backward(fctx.model, sc, d, fctx.st))
        grads[i] = grads[i].view(wshape)
        return (None, None, None, None, *grads)


def _swin_block(ctx, geo, x, pre, B, R, dim, H, d, ws, shift, nW, L, eps, cfg):
    s = pre + ".attention.self"
    qkv = Bk.linear_packed(ctx, x, [s + ".query", s + ".key", s + ".value"])   # [N, 3*dim]
    fused = ctx.dt == torch.bfloat16          # bf16: the attention kernel normalises q / k while staging
    if not fused:
        K.swin_qk_norm(qkv, H, d, ctx.P[s + ".logit_scale"], math.log(1.0 / 0.01))
    stage = int(pre.split(".")[2])
    pws = cfg.pretrained_window_sizes[stage]
    coords, rpi = geo.get(("cpb", ws, pws), lambda: tuple(t.to(geo.dev) for t in coords_table_and_index(ws, pws)))
    cpb = [s + ".continuous_position_bias_mlp.0.weight", s + ".continuous_position_bias_mlp.0.bias",
           s + ".continuous_position_bias_mlp.2.weight"]
    mask = None
    if shift > 0:
        mask = geo.get(("mask", R, ws, shift), lambda: torch.from_numpy(shift_mask(R, ws, shift)).to(geo.dev))
    # [nW|1, H, L, L]: depends on the block's weights only -> rebuilt only when they change
    bias = ctx.derived(s + "#swin_bias", cpb,
                       lambda: K.swin_bias(K.swin_cpb(coords, *[ctx.P[n] for n in cpb]), rpi, L, mask))
    q3 = qkv.view(B * nW, L, 3 * dim)
    o, _ = K.attn_fwd(q3[..., :dim], q3[..., dim:2 * dim], q3[..., 2 * dim:], H, scale=1.0,
                      rel_bias=bias if shift > 0 else bias.view(H, L, L),
                      cos_logit_scale=ctx.P[s + ".logit_scale"].view(-1) if fused else None,
                      cos_max_log=math.log(1.0 / 0.01))
    y, _ = Bk.linear(ctx, Bk.as2d(o), pre + ".attention.output.dense")
    h = K.layernorm_fwd_res(y, ctx.P[pre + ".layernorm_before.weight"], ctx.P[pre + ".layernorm_before.bias"], eps,
                            res=x)
    f, _ = Bk.linear(ctx, h, pre + ".intermediate.dense", act=K.ACT_GELU)
    m, _ = Bk.linear(ctx, f, pre + ".output.dense")
    return K.layernorm_fwd_res(m, ctx.P[pre + ".layernorm_after.weight"], ctx.P[pre + ".layernorm_after.bias"], eps,
                               res=h)
