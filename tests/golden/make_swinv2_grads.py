"""Writes the Swinv2 gradient fixtures: the parameter gradients of transformers' Swinv2Model on the
weights and pixels of swinv2_small.npz (make_golden.py gen_swinv2_small: image 128, embed 32, depths
2/2/2, heads 1/2/4, window 8; the first block's logit scale is 5.0, past the ln 100 clamp, so its
gradient is exactly 0).

swinv2_small_grads.npz (+ continuation parts swinv2_small_grads.<i>.npz):
  R          fp32 [2, 64, 128], randn from seed 23
  g.<name>   fp32: the gradient of (last_hidden_state * R).sum() with respect to parameter <name>
             (eval mode, drop_path_rate 0, fp32)
swinv2_small_grads_bf16.npz (+ parts):
  gb.<name>  float16: the same with every weight of >= 2 dimensions (except the logit scales and the
             position-bias MLP) and the pixels rounded to bf16 first, fp32 arithmetic
  emul_worst_rel, emul_min_cos
             measured between gb and a run of the same model whose Linear / LayerNorm / Conv2d outputs
             are rounded to bf16 in forward and backward (what bf16 activations cost with exact
             arithmetic): the worst per-tensor |delta|max / max(1, |ref|max) and the lowest per-tensor
             cosine. The bf16 model test's bars are twice these.
A fixture is split into parts so that no committed file exceeds 1 MiB (tests.swinv2_bwd_refs.load_parts
reads them back as one dict).

Run from the repository root: python tests/golden/make_swinv2_grads.py
(needs the `transformers` package; the test suite only reads the .npz files)."""
import glob
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
PART_BYTES = 900_000  # raw array bytes per part (random gradients do not compress)


class _RoundBf16(torch.autograd.Function):
    """y = bf16(x) in the forward, dx = bf16(dy) in the backward"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _model(state):
    from transformers import Swinv2Config, Swinv2Model
    cfg = Swinv2Config(image_size=128, patch_size=4, num_channels=3, embed_dim=32, depths=[2, 2, 2],
                       num_heads=[1, 2, 4], window_size=8, mlp_ratio=4.0, qkv_bias=True, hidden_act="gelu",
                       hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0,
                       layer_norm_eps=1e-5, pretrained_window_sizes=[0, 0, 0])
    m = Swinv2Model(cfg).float().eval()
    res = m.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m


def _grads(m, px, R, dtype=torch.float32):
    m = m.to(dtype)
    m.zero_grad(set_to_none=True)
    out = m(pixel_values=px.to(dtype)).last_hidden_state
    (out * R.to(dtype)).sum().backward()
    g = {}
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        g[n] = p.grad.detach().clone()
    return out.detach(), g


def _write(name, arrays):
    for old in glob.glob(os.path.join(HERE, name + "*.npz")):
        if os.path.basename(old) == name + ".npz" or os.path.basename(old)[len(name) + 1:-4].isdigit():
            os.remove(old)
    parts, cur, size = [], {}, 0
    for k, v in arrays.items():
        if cur and size + v.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    parts.append(cur)
    for i, part in enumerate(parts):
        path = os.path.join(HERE, name + (".npz" if i == 0 else f".{i}.npz"))
        np.savez_compressed(path, **part)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 1 << 20, path


def main():
    from tests.swinv2_bwd_refs import bf16_round_state
    z = np.load(os.path.join(HERE, "swinv2_small.npz"))
    state = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}
    px = torch.from_numpy(z["pixel_values"])
    R = torch.randn(2, 64, 128, generator=torch.Generator().manual_seed(23))

    m = _model(state)
    out, g = _grads(m, px, R)
    assert (out - torch.from_numpy(z["last_hidden_state"])).abs().max().item() < 1e-5
    _, g64 = _grads(_model(state), px, R, torch.float64)
    dev = max((g[n].double() - g64[n]).abs().max().item() / max(1.0, g64[n].abs().max().item()) for n in g)
    print(f"fp32 vs float64 gradients: worst |delta|max / max(1, |ref|max) = {dev:.3e}")
    first = "encoder.layers.0.blocks.0.attention.self.logit_scale"
    assert g[first].abs().max().item() == 0.0, g[first]
    res = {"R": R.numpy()}
    res.update({"g." + n: t.numpy() for n, t in g.items()})
    _write("swinv2_small_grads", res)

    # bf16: rounded weights and pixels, fp32 arithmetic; then the same with bf16-rounded activations
    state_b = bf16_round_state(state)
    px_b = px.to(torch.bfloat16).float()
    _, gb = _grads(_model(state_b), px_b, R)
    me = _model(state_b)
    for mod in me.modules():
        if isinstance(mod, (nn.Linear, nn.LayerNorm, nn.Conv2d)):
            mod.register_forward_hook(lambda _m, _i, o: _RoundBf16.apply(o))
    _, ge = _grads(me, px_b, R)
    worst, mincos = 0.0, 1.0
    for n in gb:
        a, b = ge[n].double().reshape(-1), gb[n].double().reshape(-1)
        worst = max(worst, (a - b).abs().max().item() / max(1.0, b.abs().max().item()))
        if b.abs().max().item() > 0:
            mincos = min(mincos, (a @ b / (a.norm() * b.norm())).item())
    print(f"bf16 activation emulation: emul_worst_rel {worst:.4e}, emul_min_cos {mincos:.6f}")
    resb = {"emul_worst_rel": np.float64(worst), "emul_min_cos": np.float64(mincos)}
    for n, t in gb.items():
        h = t.numpy().astype(np.float16)
        assert np.isfinite(h).all(), n
        resb["gb." + n] = h
    _write("swinv2_small_grads_bf16", resb)


if __name__ == "__main__":
    main()
