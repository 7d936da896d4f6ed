"""The references of tests/swinv2_bwd_refs.py against torch autograd of the expressions they differentiate
(proves, without a GPU, what tests/test_swinv2_train_gpu.py compares the HIP kernels with), plus the parts
of the trainable Swinv2 encoder that need no GPU: configuration and CLI surface, and the gradient
fixtures' keys."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attention_refs as A
from tests import swinv2_bwd_refs as R


@pytest.mark.parametrize("H,d", [(4, 32), (2, 64)])
def test_qk_norm_refs_are_autograd_of_normalize(H, d):
    rows = 37
    qkv = R.rand(rows, 3 * H * d, seed=1).double()
    qkv[5, :d] = 0                      # an all-zero q head: F.normalize's eps path
    qkv[6, H * d + d:H * d + 2 * d] = 0  # and a k head
    ls = torch.tensor([0.5, 2.3, 5.0, -1.0], dtype=torch.float64)[:H].clone()
    g = R.rand(rows, 3 * H * d, seed=2).double()
    x = qkv.clone().requires_grad_(True)
    lsr = ls.clone().requires_grad_(True)
    x4 = x.view(rows, 3, H, d)
    mult = torch.exp(torch.clamp(lsr, max=R.MAX_LOG))
    want = torch.stack([F.normalize(x4[:, 0], dim=-1) * mult[None, :, None], F.normalize(x4[:, 1], dim=-1), x4[:, 2]], 1)
    want = want.reshape(rows, 3 * H * d)
    out, inv = R.qk_norm_train_ref(qkv, H, d, ls)
    assert torch.allclose(out, want.detach(), rtol=1e-13, atol=1e-15)
    assert inv[5, 0, 0].item() == 1.0 / R.NORM_EPS and inv[6, 1, 1].item() == 1.0 / R.NORM_EPS
    (want * g).sum().backward()
    dx, dls = R.qk_norm_bwd_ref(g, out, inv, H, d, ls)
    zero = torch.zeros(rows, 3 * H * d, dtype=torch.bool)
    zero[5, :d] = True
    zero[6, H * d + d:H * d + 2 * d] = True
    assert torch.allclose(dx[~zero], x.grad[~zero], rtol=1e-11, atol=1e-12)
    # the clamped rows: g * s / eps, 1e12 times larger than the rest — relative
    assert torch.allclose(dx[zero], x.grad[zero], rtol=1e-12, atol=0)
    assert dx[5, :d].abs().max().item() > 1e10
    assert torch.allclose(dls, lsr.grad, rtol=1e-11, atol=1e-12)
    if H > 2:
        assert dls[2].item() == 0.0 and lsr.grad[2].item() == 0.0  # 5.0 is past ln 100


@pytest.mark.parametrize("B,M,H,Lq,Lk,D", [(3, 1, 2, 16, 16, 32), (4, 2, 2, 20, 24, 32)])
def test_bias_sum_ref_is_autograd_of_attention(B, M, H, Lq, Lk, D):
    q, k, v = R.rand(B, Lq, H * D, seed=3), R.rand(B, Lk, H * D, seed=4), R.rand(B, Lk, H * D, seed=5)
    dout = R.rand(B, Lq, H * D, seed=6)
    rb = R.rand(H, Lq, Lk, seed=7) if M == 1 else R.rand(M, H, Lq, Lk, seed=7)
    want = A.attention_ref(q, k, v, H, 0.7, rel_bias=rb, dout=dout, want_d_rel_bias=True)["d_rel_bias"]
    got = R.bias_sum_ref(R.attn_ds_ref(q, k, v, dout, H, 0.7, rb), M)
    assert tuple(got.shape) == (M, H, Lq, Lk)
    assert torch.allclose(got.reshape(want.shape), want, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("ws,H,nW", [(8, 4, 16), (4, 1, 1), (4, 32, 16)])
def test_bias_and_cpb_bwd_refs_are_autograd(ws, H, nW):
    from mmfd.swinv2 import coords_table_and_index
    coords, rpi = coords_table_and_index(ws)
    L, T = ws * ws, (2 * ws - 1) ** 2
    assert tuple(coords.shape) == (T, 2)
    w1, b1, w2 = (R.rand(512, 2, seed=8) * 0.5).double(), (R.rand(512, seed=9) * 0.1).double(), \
        (R.rand(H, 512, seed=10) * 0.05).double()
    mask = torch.where(R.rand(nW, L, L, seed=11) > 1.0, -100.0, 0.0).double() if nW > 1 else None
    d_bias = R.rand(nW, H, L, L, seed=12).double()
    ps = [t.clone().requires_grad_(True) for t in (w1, b1, w2)]
    table = torch.relu(coords.double() @ ps[0].t() + ps[1]) @ ps[2].t()
    table.retain_grad()
    bias = 16 * torch.sigmoid(table[rpi.long()].view(L, L, H).permute(2, 0, 1)).unsqueeze(0)
    bias = bias.expand(nW, -1, -1, -1)
    if mask is not None:
        bias = (bias + mask[:, None]) + mask[:, None]
    (bias * d_bias).sum().backward()
    d_table = R.swin_bias_bwd_ref(d_bias, table.detach(), rpi)
    assert torch.allclose(d_table, table.grad, rtol=1e-11, atol=1e-13)
    for got, p in zip(R.swin_cpb_bwd_ref(d_table, coords, w1, b1, w2), ps):
        assert torch.allclose(got, p.grad, rtol=1e-10, atol=1e-12)


def test_config_defaults_and_cli_flag():
    from mmfd.swinv2 import Swinv2Config
    from mmfd.train import parse_args
    c = Swinv2Config()
    assert c.trainable is False and c.drop_path_rate == 0.0
    assert parse_args([]).train_image_encoder is False
    assert parse_args(["--train_image_encoder"]).train_image_encoder is True


def test_build_encoders_trainable_swinv2():
    from mmfd.encoders import ViTModel
    from mmfd.swinv2 import Swinv2Model
    from mmfd.train import build_encoders, parse_args
    bert = ["--text_encoder", "bert-base-uncased", "--freeze_text"]
    _, image, _, frozen = build_encoders(parse_args(bert + ["--train_image_encoder"]), "cpu")
    assert isinstance(image, Swinv2Model) and image.config.trainable and frozen is False
    _, image, _, frozen = build_encoders(parse_args(bert + ["--train_image_encoder", "--freeze_image"]), "cpu")
    assert isinstance(image, Swinv2Model) and not image.config.trainable and frozen is True
    _, image, _, frozen = build_encoders(parse_args(bert), "cpu")
    assert isinstance(image, Swinv2Model) and not image.config.trainable and frozen is True
    vit = bert + ["--image_encoder", "google/vit-base-patch16-224"]
    _, image, _, frozen = build_encoders(parse_args(vit + ["--train_image_encoder"]), "cpu")
    assert isinstance(image, ViTModel) and frozen is False  # no effect on ViT-B/16: it trains unless --freeze_image
    _, image, _, frozen = build_encoders(parse_args(vit + ["--train_image_encoder", "--freeze_image"]), "cpu")
    assert isinstance(image, ViTModel) and frozen is True


def test_gradient_fixture_keys_are_the_parameter_names():
    from mmfd.swinv2 import Swinv2Config, Swinv2Model
    names = {n for n, _ in Swinv2Model(Swinv2Config(**R.SMALL)).named_parameters()}
    g = R.load_parts("swinv2_small_grads")
    gb = R.load_parts("swinv2_small_grads_bf16")
    assert {k[2:] for k in g if k.startswith("g.")} == names
    assert {k[3:] for k in gb if k.startswith("gb.")} == names
    assert set(g) == {"R"} | {"g." + n for n in names}
    assert set(gb) == {"emul_worst_rel", "emul_min_cos"} | {"gb." + n for n in names}
    assert tuple(g["R"].shape) == (2, 64, 128)
    # the first block's logit scale (5.0) is past the clamp ln 100 = 4.6: its gradient is exactly 0
    first = "encoder.layers.0.blocks.0.attention.self.logit_scale"
    assert 5.0 > math.log(100.0) and (g["g." + first] == 0).all() and (gb["gb." + first] == 0).all()
    assert 0 < float(gb["emul_worst_rel"]) < 0.5 and 0.9 < float(gb["emul_min_cos"]) < 1.0
