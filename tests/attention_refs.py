"""TEST INFRASTRUCTURE ONLY. Multi-head attention in plain float64 torch on the CPU, written from the
definition (not from the kernels) and evaluated on the kernels' rounded inputs:

    S = scale * Q K^T + key_bias[b, k] + rel_bias[b, h, q, k]
    P = softmax_k(S),  lse = logsumexp_k(S)
    O = (P * keep / (1 - p)) V

`rel_bias` is [H, Lq, Lk] (shared), [B, H, Lq, Lk] (per batch row) or [M, H, Lq, Lk] with B % M == 0
(batch row b reads row b % M). `keep` is the boolean keep mask of the probabilities [B, H, Lq, Lk]
(oracle.dropout_hash.attn_keep_mask). Cosine attention (Swinv2): q and k are L2-normalised per head with
F.normalize's eps and q is multiplied by exp(min(logit_scale[h], max_log)).

Gradients come from autograd on the float64 graph. tests/test_attention_ref_cpu.py checks this file
against torch's scaled_dot_product_attention."""
import math

import torch
import torch.nn.functional as F

COS_EPS = 1e-12  # F.normalize's default


def to_heads(t, H):
    """[B, L, H*D] -> [B, H, L, D]"""
    B, L, W = t.shape
    return t.reshape(B, L, H, W // H).transpose(1, 2)


def from_heads(t):
    """[B, H, L, D] -> [B, L, H*D]"""
    B, H, L, D = t.shape
    return t.transpose(1, 2).reshape(B, L, H * D)


def batch_rel_bias(rel_bias, B):
    """any of the three forms -> [B, H, Lq, Lk] (a differentiable view / gather of the argument)"""
    if rel_bias.dim() == 3:
        return rel_bias[None].expand(B, -1, -1, -1)
    M = rel_bias.shape[0]
    if M == B:
        return rel_bias
    assert B % M == 0, (B, M)
    return rel_bias[torch.arange(B) % M]


def logits(q, k, H, scale, key_bias=None, rel_bias=None, cos_logit_scale=None, cos_max_log=None):
    """S [B, H, Lq, Lk] of float64 q [B, Lq, H*D] and k [B, Lk, H*D]"""
    qh, kh = to_heads(q, H), to_heads(k, H)
    if cos_logit_scale is not None:
        mult = torch.exp(torch.clamp(cos_logit_scale.double(), max=cos_max_log))
        qh = F.normalize(qh, dim=-1, eps=COS_EPS) * mult[None, :, None, None]
        kh = F.normalize(kh, dim=-1, eps=COS_EPS)
    s = qh @ kh.transpose(-1, -2) * scale
    if key_bias is not None:
        s = s + key_bias.double()[:, None, None, :]
    if rel_bias is not None:
        s = s + batch_rel_bias(rel_bias, q.shape[0])
    return s


def attention_ref(q, k, v, H, scale, *, key_bias=None, rel_bias=None, keep=None, p=0.0, cos_logit_scale=None,
                  cos_max_log=None, dout=None, want_d_rel_bias=False):
    """Returns {"o": [B, Lq, H*D], "lse": [B, H, Lq]} and, with `dout`, "dq", "dk", "dv" (and "d_rel_bias" in
    rel_bias's own shape), all float64. q, k, v, dout are taken as they are (any float dtype) and
    promoted exactly."""
    qr, kr, vr = (t.detach().double().clone().requires_grad_(dout is not None) for t in (q, k, v))
    rb = None
    if rel_bias is not None:
        rb = rel_bias.detach().double().clone().requires_grad_(want_d_rel_bias)
    s = logits(qr, kr, H, scale, key_bias, rb, cos_logit_scale, cos_max_log)
    lse = torch.logsumexp(s, -1)
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * torch.as_tensor(keep).double() / (1.0 - p)
    o = from_heads(pr @ to_heads(vr, H))
    out = {"o": o.detach(), "lse": lse.detach()}
    if dout is not None:
        o.backward(dout.detach().double())
        out.update(dq=qr.grad, dk=kr.grad, dv=vr.grad)
        if want_d_rel_bias:
            out["d_rel_bias"] = rb.grad
    return out


# ------------------------------------------------------------------------------------------------------
# CPU emulations of a kernel's arithmetic: what a correct kernel of that precision can reach. They
# bound the test inputs (tests/test_attention_ref_cpu.py: within half of the GPU test's bound), they are
# not a reference.
# ------------------------------------------------------------------------------------------------------
def emulated_attention(q, k, v, dout, H, scale, *, key_bias=None, keep=None, p=0.0, bf16=False):
    """fp32 flash-style forward and backward written out by hand; with bf16=True the probabilities, dS
    and the outputs are rounded to bf16 (the inputs are the caller's rounded tensors), everything else
    stays fp32. Returns o, lse, dq, dk, dv as float32 / bfloat16 tensors promoted to float64."""
    f = torch.float32
    rnd = (lambda t: t.to(torch.bfloat16).to(f)) if bf16 else (lambda t: t)
    qh, kh, vh, doh = (to_heads(t.to(f), H) for t in (q, k, v, dout))
    s = (qh @ kh.transpose(-1, -2)) * f_(scale)
    if key_bias is not None:
        s = s + key_bias.to(f)[:, None, None, :]
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = (m + torch.log(l)).squeeze(-1)
    pr = e / l
    ks = 1.0 if keep is None else torch.as_tensor(keep).to(f) * f_(1.0 / (1.0 - p))
    pd = rnd(pr * ks)
    o = rnd(pd @ vh)
    dv = rnd(pd.transpose(-1, -2) @ doh)
    dp = (doh @ vh.transpose(-1, -2)) * ks
    delta = (doh * o).sum(-1, keepdim=True)
    ds = rnd(pr * (dp - delta))
    dq = rnd((ds @ kh) * f_(scale))
    dk = rnd((ds.transpose(-1, -2) @ qh) * f_(scale))
    return {"o": from_heads(o).double(), "lse": lse.double(), "dq": from_heads(dq).double(),
            "dk": from_heads(dk).double(), "dv": from_heads(dv).double()}


def f_(x):
    return torch.tensor(x, dtype=torch.float32)


def emulated_cosine_forward(q, k, v, H, rel_bias, cos_logit_scale, cos_max_log, *, round_normalised):
    """bf16 cosine forward (scale 1) in fp32 with P and o rounded to bf16. round_normalised=False: the
    raw bf16 q, k enter the product and the norms and exp(min(logit_scale, max_log)) scale its fp32
    result (what a bf16 MFMA kernel can do); True: q / |q| * mult and k / |k| are rounded to bf16 first,
    as a separate normalisation pass that writes bf16 would leave them."""
    f = torch.float32
    rnd = lambda t: t.to(torch.bfloat16).to(f)  # noqa: E731
    qh, kh, vh = (to_heads(t.to(f), H) for t in (q, k, v))
    mult = torch.exp(torch.clamp(cos_logit_scale.to(f), max=cos_max_log))[None, :, None, None]
    qn = 1.0 / qh.norm(dim=-1, keepdim=True).clamp_min(COS_EPS)
    kn = 1.0 / kh.norm(dim=-1, keepdim=True).clamp_min(COS_EPS)
    if round_normalised:
        s = rnd(qh * qn * mult) @ rnd(kh * kn).transpose(-1, -2)
    else:
        s = (qh @ kh.transpose(-1, -2)) * (qn * mult) * kn.transpose(-1, -2)
    s = s + batch_rel_bias(rel_bias.to(f), q.shape[0])
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return {"o": from_heads(rnd(rnd(e / l) @ vh)).double(), "lse": (m + torch.log(l)).squeeze(-1).double()}


# ------------------------------------------------------------------------------------------------------
# the error rule of tests/test_kernels_gpu.py, per (batch row, head) slice
# ------------------------------------------------------------------------------------------------------
TOL = {"f32": (3e-5, 3e-5), "bf16": (2e-2, 2e-2)}  # (atol, rtol): err <= atol + rtol * max|ref|
LSE_TOL = {"f32": 1e-4, "bf16": 2e-2}  # absolute


def _slices(name, t, H):
    """[n_slices, -1]: one row per (batch row, head)"""
    if name == "lse":  # [B, H, Lq]
        return t.reshape(t.shape[0] * t.shape[1], -1)
    if name == "d_rel_bias":  # [B, H, Lq, Lk]
        return t.reshape(t.shape[0] * t.shape[1], -1)
    B, L, W = t.shape  # [B, L, H*D]
    return t.reshape(B, L, H, W // H).permute(0, 2, 1, 3).reshape(B * H, -1)


def worst_ratio(name, got, ref, H, dtype, base=None):
    """max over the (batch row, head) slices of err / bound, bound = atol + rtol * max|ref| of that slice
    (lse: the absolute bound). `base` (accumulate): got is compared with base + ref and the bound taken
    on |base + ref|. Returns (ratio, slice index); NaN in `got` gives inf."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    if base is not None:
        ref = ref + base.detach().double().cpu()
    g, r = _slices(name, got, H), _slices(name, ref, H)
    err = (g - r).abs().amax(1)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    if name == "lse":
        bound = torch.full_like(err, LSE_TOL[dtype])
    else:
        atol, rtol = TOL[dtype]
        bound = atol + rtol * r.abs().amax(1)
    ratio = err / bound
    i = int(ratio.argmax())
    return float(ratio[i]), i
