"""TEST INFRASTRUCTURE ONLY. Plain references of the memory-bound training kernels (csrc/misc.hip,
csrc/runtime.hip and the small kernels of csrc/conv.hip): torch on the CPU, fp64 wherever arithmetic
happens, written as directly as the operation's definition allows (loops where a loop is the
definition). tests/test_memory_kernels_ref_cpu.py proves each against an independent formulation;
tests/test_memory_kernels_gpu.py compares the HIP kernels with them.
"""
import math

import numpy as np
import torch

BF16_EPS = 2.0 ** -8  # one round-to-nearest rounding to 8 significant bits: |err| <= 2^-8 |x|
F32_TOL = 3e-5        # the suite's fp32 convention (tests/test_kernels_gpu.py::_tol)


def rand(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


# ---------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------
def f32_excess(got, ref, scale=1.0):
    """max |got - ref| minus the fp32 bound 3e-5 * scale + 3e-5 * max |ref| (<= 0 passes)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    return (got - ref).abs().max().item() - (F32_TOL * scale + F32_TOL * ref.abs().max().item())


def bf16_excess(got, ref, scale=1.0):
    """max over elements of |got - ref| - (2^-8 |ref| + 3e-5 * scale): a bf16 output of an fp32
    computation is one rounding of the fp32 value (<= 0 passes)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    return ((got - ref).abs() - (BF16_EPS * ref.abs() + F32_TOL * scale)).max().item()


def excess(got, ref, scale=1.0):
    """the bound of the output's own dtype"""
    return (bf16_excess if got.dtype == torch.bfloat16 else f32_excess)(got, ref, scale)


# ---------------------------------------------------------------------------------------------
# dropout mask (csrc/common.h mmfd_hash / mmfd_drop_threshold), one element at a time
# ---------------------------------------------------------------------------------------------
_U32 = 0xFFFFFFFF


def _mix32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _U32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _U32
    return x ^ (x >> 16)


def hash_ref(seed, salt, idx):
    """mmfd_hash of csrc/common.h in Python integers"""
    seed, salt = seed & 0xFFFFFFFFFFFFFFFF, salt & 0xFFFFFFFFFFFFFFFF
    k0 = _mix32((seed & _U32) ^ _mix32((seed >> 32) ^ 0x85EBCA6B))
    key = _mix32(k0 ^ (salt & _U32) ^ _mix32((salt >> 32) ^ 0xC2B2AE35))
    return _mix32(key ^ (((idx & _U32) * 0x9E3779B1) & _U32) ^ (((idx >> 32) * 0x85EBCA77) & _U32))


def _unmix32(x):
    x ^= x >> 16
    x = (x * pow(0x846CA68B, -1, 1 << 32)) & _U32
    x ^= (x >> 15) ^ (x >> 30)
    x = (x * pow(0x7FEB352D, -1, 1 << 32)) & _U32
    return x ^ (x >> 16)


def salt_with_hash(seed, idx, target):
    """a salt (high word 0) with mmfd_hash(seed, salt, idx) == target: every step of the hash is a
    bijection of 32-bit words, so the salt's low word is solved for. Puts one element exactly on the
    dropout threshold (keep <=> hash >= threshold), which random salts hit once in 2^32 elements."""
    seed &= 0xFFFFFFFFFFFFFFFF
    k0 = _mix32((seed & _U32) ^ _mix32((seed >> 32) ^ 0x85EBCA6B))
    key = _unmix32(target) ^ (((idx & _U32) * 0x9E3779B1) & _U32) ^ (((idx >> 32) * 0x85EBCA77) & _U32)
    return _unmix32(key) ^ k0 ^ _mix32(0xC2B2AE35)


def keep_mask_ref(seed, salt, shape, p):
    """keep <=> hash(seed, salt, flat index) >= min(floor(float32(p) * 2^32), 2^32 - 1), one element
    at a time (small shapes: the GPU tests draw their masks with oracle.dropout_hash.keep_mask, the
    vectorised form this one is checked against)"""
    n = int(np.prod(shape))
    thr = min(int(float(np.float32(p)) * 4294967296.0), _U32)
    return torch.tensor([hash_ref(seed, salt, i) >= thr for i in range(n)], dtype=torch.bool).reshape(shape)


def dropout_ref(x, keep, p):
    """fp64: x / (1 - p) where kept, else 0"""
    return torch.where(keep, x.double() / (1.0 - float(np.float32(p))), torch.zeros((), dtype=torch.float64))


# ---------------------------------------------------------------------------------------------
# embeddings + LayerNorm
# ---------------------------------------------------------------------------------------------
def embed_sum_ref(ids, pos_ids, tts, word, pos, typ):
    """fp64 [B*L, D]: word[id] + pos[pos_id or t] (+ type[tt or 0]), row by row"""
    B, L = ids.shape
    out = torch.empty(B * L, word.shape[1], dtype=torch.float64)
    for b in range(B):
        for t in range(L):
            r = b * L + t
            pi = int(pos_ids[b, t]) if pos_ids is not None else t
            e = word[int(ids[b, t])].double() + pos[pi].double()
            if typ is not None:
                e = e + typ[int(tts[b, t]) if tts is not None else 0].double()
            out[r] = e
    return out


def layernorm_ref(s, gamma, beta, eps):
    """fp64 (y, mean, rstd) of LayerNorm over the last dim of s (biased variance)"""
    s = s.double()
    mean = s.sum(-1) / s.shape[-1]
    var = ((s - mean[:, None]) ** 2).sum(-1) / s.shape[-1]
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (s - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    return y, mean, rstd


def position_ids_ref(ids, padding_idx):
    """HF create_position_ids_from_input_ids as a loop: the running count of non-pad tokens plus
    padding_idx on a token, padding_idx on padding"""
    out = torch.empty_like(ids)
    for b in range(ids.shape[0]):
        c = 0
        for t in range(ids.shape[1]):
            if int(ids[b, t]) != padding_idx:
                c += 1
                out[b, t] = c + padding_idx
            else:
                out[b, t] = padding_idx
    return out


def rel_bias_ref(bucket, table):
    """[H, Lq, Lk] = table[bucket[q, k], h]"""
    return table[bucket.long()].permute(2, 0, 1).contiguous()


# ---------------------------------------------------------------------------------------------
# ViT
# ---------------------------------------------------------------------------------------------
def patchify_ref(px, P):
    """[B, C, H, W] -> [B * (H/P) * (W/P), C*P*P], patch rows in (ph, pw) order, columns (c, kh, kw);
    pure data movement (the dtype of px is kept)"""
    B, C, H, W = px.shape
    nph, npw = H // P, W // P
    return px.reshape(B, C, nph, P, npw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * nph * npw, C * P * P).contiguous()


def vit_tokens_fwd_ref(patch, B, cls, pos):
    """fp64 [B, NP+1, D]: token 0 = cls + pos[0], token t = patch[b, t-1] + pos[t]"""
    NP, D = patch.shape[0] // B, patch.shape[1]
    out = torch.empty(B, NP + 1, D, dtype=torch.float64)
    out[:, 0] = cls.double() + pos[0].double()
    out[:, 1:] = patch.double().reshape(B, NP, D) + pos[1:].double()
    return out


def vit_tokens_bwd_ref(dout):
    """(dpatch in dout's dtype (a copy), dcls fp64 [D], dpos fp64 [NP+1, D])"""
    B, T, D = dout.shape
    dpos = dout.double().sum(0)
    return dout[:, 1:].reshape(B * (T - 1), D).contiguous(), dpos[0].clone(), dpos


# ---------------------------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------------------------
def gelu_grad_ref(x):
    """fp64 d/dx [x Phi(x)] = Phi(x) + x phi(x)"""
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def act_bwd_ref(dy, aux, act, keep=None, p=0.0):
    """fp64 (dropout-undone dy) * act'(aux); act in {"none", "gelu", "relu"}"""
    z = dy.double() if keep is None else dropout_ref(dy, keep, p)
    if act == "gelu":
        z = z * gelu_grad_ref(aux)
    elif act == "relu":
        z = torch.where(aux.double() > 0, z, torch.zeros((), dtype=torch.float64))
    return z


def axpby_ref(a, x, b=0.0, y=None):
    out = float(a) * x.double()
    return out if y is None else out + float(b) * y.double()


def seq_mean_bwd_ref(dout, L):
    """fp64 [B, L, D]: every position receives dout / L"""
    return (dout.double() / L)[:, None, :].expand(dout.shape[0], L, dout.shape[1]).contiguous()


def mask_to_bias_ref(mask, neg):
    return torch.where(mask != 0, torch.zeros((), dtype=torch.float32), torch.tensor(neg, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------
# cross entropy summed over paths
# ---------------------------------------------------------------------------------------------
def xent_ref(logits, labels, cols=None, n_slots=None, dloss_scale=1.0):
    """(loss fp64 [n_slots] = [total, one slot per label column], [dlogits fp64]); path i is trained
    on labels[:, cols[i]] with the mean over the batch; only the gradients carry dloss_scale"""
    n = len(logits)
    cols = list(range(n)) if cols is None else list(cols)
    n_slots = n_slots or 2 + max(cols)
    labels = labels.reshape(labels.shape[0], -1)
    loss = torch.zeros(n_slots, dtype=torch.float64)
    grads = []
    for z, col in zip(logits, cols):
        z = z.double()
        B, C = z.shape
        y = labels[:, col]
        mx = z.max(dim=1, keepdim=True).values
        lse = (mx + torch.log(torch.exp(z - mx).sum(1, keepdim=True))).squeeze(1)
        picked = z[torch.arange(B), y]
        lp = (lse - picked).sum() / B
        loss[1 + col] = lp
        loss[0] += lp
        onehot = torch.zeros(B, C, dtype=torch.float64)
        onehot[torch.arange(B), y] = 1.0
        grads.append((torch.exp(z - lse[:, None]) - onehot) * float(dloss_scale) / B)
    return loss, grads


# ---------------------------------------------------------------------------------------------
# AdamW (torch.optim.AdamW: decoupled weight decay, bias-corrected moments)
# ---------------------------------------------------------------------------------------------
def adamw_ref(p, g, m, v, step, lr, b1, b2, eps, wd):
    """one step on fp64 tensors; `step` is the count after this step. Returns (p, m, v)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (torch.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


# ---------------------------------------------------------------------------------------------
# convolution helpers
# ---------------------------------------------------------------------------------------------
def conv_weight_prep_ref(w, Kpad=None, bn=None, eps=1e-5):
    """fp64 (GEMM weight [Cout, Kpad] with column (kh*KW + kw)*Cin + ci = w[co, ci, kh, kw] * s[co]
    and zero padding columns, bias [Cout] = beta - mean * s), s = gamma / sqrt(var + eps); s = 1 and
    bias = 0 without BatchNorm. Element by element."""
    Cout, Cin, KH, KW = w.shape
    Kpad = Kpad or KH * KW * Cin
    ow = torch.zeros(Cout, Kpad, dtype=torch.float64)
    ob = torch.zeros(Cout, dtype=torch.float64)
    for co in range(Cout):
        s = 1.0
        if bn is not None:
            gamma, beta, mean, var = (float(t[co]) for t in bn)
            s = gamma / math.sqrt(var + eps)
            ob[co] = beta - mean * s
        for ci in range(Cin):
            for kh in range(KH):
                for kw in range(KW):
                    ow[co, (kh * KW + kw) * Cin + ci] = float(w[co, ci, kh, kw]) * s
    return ow, ob


def global_avgpool_ref(x, N, HW, C):
    """NHWC rows [N*HW, C] -> fp64 [N, C]"""
    return x.double().reshape(N, HW, C).sum(1) / HW
