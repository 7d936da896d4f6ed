"""TEST INFRASTRUCTURE ONLY. Float64 reference formulas of the Swinv2 fine-tuning operators
(csrc/swin_train.hip), written from the formulas in include/mmfd.h, torch on the CPU.
tests/test_swinv2_bwd_ref_cpu.py proves each against autograd of the expression it differentiates;
tests/test_swinv2_train_gpu.py compares the HIP kernels with them. Also here: the gradient fixtures'
reader (tests/golden/make_swinv2_grads.py writes them in parts) and the bf16 rounding rule the fixture
and the bf16 model test share.
"""
import glob
import math
import os

import numpy as np
import torch

MAX_LOG = math.log(1.0 / 0.01)  # the logit-scale clamp
NORM_EPS = 1e-12                # F.normalize's default
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = dict(image_size=128, embed_dim=32, depths=(2, 2, 2), num_heads=(1, 2, 4), pretrained_window_sizes=(0, 0, 0))


def rand(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# ---------------------------------------------------------------------------------------------
# cosine pass on packed rows [rows, 3*H*d]: q | k | v thirds, heads inside a third
# ---------------------------------------------------------------------------------------------
def qk_norm_train_ref(qkv, H, d, logit_scale, max_log=MAX_LOG):
    """(normalised packed rows, inv [rows, 2, H]) in float64: q_h / max(|q_h|, eps) * exp(min(ls_h, c)),
    k_h / max(|k_h|, eps), v untouched; inv = 1 / max(|.|, eps)"""
    x = qkv.detach().double().reshape(qkv.shape[0], 3, H, d).clone()
    mult = torch.exp(torch.clamp(logit_scale.detach().double().reshape(H), max=max_log))
    inv = 1.0 / x[:, :2].norm(dim=-1).clamp_min(NORM_EPS)           # [rows, 2, H]
    x[:, 0] = x[:, 0] * inv[:, 0, :, None] * mult[None, :, None]
    x[:, 1] = x[:, 1] * inv[:, 1, :, None]
    return x.reshape(qkv.shape[0], 3 * H * d), inv


def qk_norm_bwd_ref(g, qkv_norm, inv, H, d, logit_scale, max_log=MAX_LOG):
    """(packed gradient rows, d_logit_scale [H]) in float64 from g = dL/d(normalised rows): with
    qh = q/|q|, s = exp(min(ls_h, c)), qn = s qh:  dq = (s/|q|)(g - qh (qh . g)) when |q| >= eps, else
    (s/eps) g; k the same with s = 1; v passes through; d ls_h = [ls_h <= c] sum_rows g . qn"""
    rows = g.shape[0]
    g4 = g.detach().double().reshape(rows, 3, H, d)
    n4 = qkv_norm.detach().double().reshape(rows, 3, H, d)
    inv = inv.detach().double().reshape(rows, 2, H)
    ls = logit_scale.detach().double().reshape(H)
    s = torch.stack([torch.exp(torch.clamp(ls, max=max_log)), torch.ones(H, dtype=torch.float64)])  # [2, H]
    out = g4.clone()
    hat = n4[:, :2] / s[None, :, :, None]                               # unit vectors (0 for a zero row)
    dot = (hat * g4[:, :2]).sum(-1, keepdim=True)
    proj = g4[:, :2] - hat * dot
    clamped = (inv >= 0.999 / NORM_EPS)[..., None]   # (0.999: an fp32 inverse norm of the clamp is 1e12 (1 - 4e-8))
    out[:, :2] = torch.where(clamped, g4[:, :2], proj) * (s[None] * inv)[..., None]
    dls = (g4[:, 0] * n4[:, 0]).sum(dim=(0, 2)) * (ls <= max_log).double()
    return out.reshape(rows, 3 * H * d), dls


# ---------------------------------------------------------------------------------------------
# the gradient of a shared / modulo attention bias
# ---------------------------------------------------------------------------------------------
def attn_ds_ref(q, k, v, dout, H, scale, rel_bias, key_bias=None):
    """per-batch dS = P (dP - delta) [B, H, Lq, Lk] in float64, written out: P = softmax(scale q k^T +
    bias), dP = dO V^T, delta = rowsum(dO * O). rel_bias [H, Lq, Lk] or [M, H, Lq, Lk] (row b % M)."""
    B, Lq, W = q.shape
    D = W // H
    heads = lambda t: t.detach().double().reshape(B, -1, H, D).transpose(1, 2)  # noqa: E731
    qh, kh, vh, doh = heads(q), heads(k), heads(v), heads(dout)
    rb = rel_bias.detach().double()
    rb = rb[None].expand(B, -1, -1, -1) if rb.dim() == 3 else rb[torch.arange(B) % rb.shape[0]]
    s = qh @ kh.transpose(-1, -2) * scale + rb
    if key_bias is not None:
        s = s + key_bias.detach().double()[:, None, None, :]
    p = torch.softmax(s, -1)
    o = p @ vh
    dp = doh @ vh.transpose(-1, -2)
    delta = (doh * o).sum(-1, keepdim=True)
    return p * (dp - delta)


def bias_sum_ref(ds, M):
    """[B, H, Lq, Lk] -> [M, H, Lq, Lk]: row m sums the batch rows b = m (mod M)"""
    B = ds.shape[0]
    return ds.reshape(B // M, M, *ds.shape[1:]).sum(0)


# ---------------------------------------------------------------------------------------------
# position bias: 16 sigmoid(table[rpi]) (+ 2 mask) and the MLP relu(coords W1^T + b1) W2^T
# ---------------------------------------------------------------------------------------------
def swin_bias_bwd_ref(d_bias, table, rpi):
    """d_table [T, H] in float64 = 16 sg (1 - sg) * sum over windows and over the (i, j) with rpi[i, j] == r"""
    nW, H, L, _ = d_bias.shape
    T = table.shape[0]
    g = d_bias.detach().double().sum(0).reshape(H, L * L)                  # the mask is a constant
    acc = torch.zeros(T, H, dtype=torch.float64)
    acc.index_add_(0, rpi.reshape(-1).long(), g.t().contiguous())
    sg = torch.sigmoid(table.detach().double())
    return 16.0 * sg * (1.0 - sg) * acc


def swin_cpb_bwd_ref(d_table, coords, w1, b1, w2):
    """(d_w1 [512, 2], d_b1 [512], d_w2 [H, 512]) in float64 of table = relu(coords W1^T + b1) W2^T"""
    dt, c, w1, b1, w2 = (t.detach().double() for t in (d_table, coords, w1, b1, w2))
    pre = c @ w1.t() + b1                                                   # [T, 512]
    hid = pre.clamp_min(0.0)
    d_w2 = dt.t() @ hid
    d_pre = (dt @ w2) * (pre > 0).double()
    return d_pre.t() @ c, d_pre.sum(0), d_w2


# ---------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------
def load_parts(name):
    """the arrays of tests/golden/<name>.npz and its continuation parts <name>.<i>.npz as one dict (the
    generator splits a fixture so that no committed file exceeds 1 MiB)"""
    base = os.path.join(GOLDEN, name)
    out = {}
    for path in [base + ".npz"] + sorted(glob.glob(base + ".[0-9]*.npz")):
        with np.load(path, allow_pickle=False) as z:
            for k in z.files:
                assert k not in out, (k, path)
                out[k] = z[k]
    return out


def is_bf16_weight(name, tensor):
    """the bf16 fixture's rounding rule: every weight of >= 2 dimensions except the logit scales and the
    position-bias MLP (mmfd computes those in fp32 in both modes)"""
    return tensor.dim() >= 2 and "logit_scale" not in name and "continuous_position_bias_mlp" not in name


def bf16_round_state(state):
    """state_dict with the weights of is_bf16_weight rounded to bf16 (kept as fp32 tensors)"""
    return {k: (v.to(torch.bfloat16).float() if v.is_floating_point() and is_bf16_weight(k, v) else v.clone())
            for k, v in state.items()}
