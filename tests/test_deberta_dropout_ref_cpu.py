"""The float64 DeBERTa restatement with dropout hooks (tests/deberta_dropout_ref.py), the reference of
tests/test_deberta_dropout_gpu.py, checked on the CPU: without dropout it is oracle.deberta.deberta_forward,
and with oracle.dropout_hash.Drop(seed, 0.1) its five sites are where transformers' DebertaV2Model has its
nn.Dropout modules — the same Drop installed as the forward of every dropout module of a transformers model
in training mode gives the same last_hidden_state on real-token rows and the same parameter gradients of a
loss over real-token rows, to 1e-10 relative (float64 on both sides). Padded rows are excluded: mmfd's rule
for them (mean of V, no attention dropout) differs from transformers', see the helper's docstring.

transformers computes the score divisor sqrt(3 d) in float32 even in a float64 model (scaled_size_sqrt);
at d = 32 that alone moves the float64 output by 3.8e-10 relative (measured without dropout), above the
1e-10 of this comparison. The comparison therefore hands the restatement transformers' own float32-rounded
divisor (score_scale): the check is about where the masks sit, and both sides then compute the same
function. The restatement's default stays the float64 sqrt, which is what the oracle and the kernels use."""
import numpy as np
import torch

from oracle.deberta import deberta_forward
from oracle.dropout_hash import Drop
from tests.deberta_dropout_ref import SITE, deberta_forward_drop, sites

CFG = dict(vocab_size=200, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128)
SEED, P_DROP = 1234, 0.1
B, L, VALID = 2, 37, 21  # batch row 1 has 21 real tokens, the rest is padding


def _hf_model(p):
    from transformers import DebertaV2Config, DebertaV2Model
    cfg = DebertaV2Config(max_position_embeddings=512, relative_attention=True, position_buckets=256,
                          norm_rel_ebd="layer_norm", share_att_key=True, pos_att_type=["p2c", "c2p"], layer_norm_eps=1e-7,
                          position_biased_input=False, type_vocab_size=0, hidden_act="gelu", max_relative_positions=-1,
                          pad_token_id=0, hidden_dropout_prob=p, attention_probs_dropout_prob=p, **CFG)
    torch.manual_seed(7)
    m = DebertaV2Model(cfg).double()
    with torch.no_grad():
        for q in m.parameters():  # LayerNorm / bias parameters off their trivial init
            q.add_(torch.randn_like(q) * 0.05)
    return m


def _inputs():
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, CFG["vocab_size"], (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, VALID:] = 0
    ids[1, VALID:] = 0
    R = torch.randn(B, L, CFG["hidden_size"], generator=g, dtype=torch.float64) * mask[:, :, None]
    return ids, mask, R


class CountingDrop(Drop):
    """Drop that records (kept, total) per site"""

    def __init__(self, seed, p):
        super().__init__(seed, p)
        self.seen = {}

    def __call__(self, site, x):
        y = super().__call__(site, x)
        kept = int(((y != 0) | (x == 0)).sum())
        self.seen[site] = (kept, x.numel())
        return y


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def test_without_dropout_it_is_the_oracle():
    m = _hf_model(0.0)
    ids, mask, _ = _inputs()
    P = {k: v.detach() for k, v in m.state_dict().items()}
    kw = dict(num_layers=CFG["num_hidden_layers"], num_heads=CFG["num_attention_heads"])
    a = deberta_forward_drop(P, ids, mask, **kw)
    b = deberta_forward(P, ids, mask, **kw)
    assert a.dtype == torch.float64 and _rel(a, b) <= 1e-12, _rel(a, b)


def test_every_site_drops_some_and_keeps_some():
    m = _hf_model(0.0)
    ids, mask, _ = _inputs()
    P = {k: v.detach() for k, v in m.state_dict().items()}
    drop = CountingDrop(SEED, P_DROP)
    deberta_forward_drop(P, ids, mask, num_layers=2, num_heads=2, drop=drop)
    assert sorted(drop.seen) == sorted(sites(2))
    for s, (kept, n) in drop.seen.items():
        print(f"{s}: kept {kept} of {n}")
        assert 0 < kept < n, (s, kept, n)


def _hf_site(name):
    """module name of a transformers dropout -> mmfd site"""
    if name == "embeddings.dropout":
        return SITE + ".emb"
    parts = name.split(".")
    assert parts[:2] == ["encoder", "layer"], name
    tail = ".".join(parts[3:])
    leaf = {"attention.self.dropout": "attn", "attention.self.pos_dropout": "pos", "attention.output.dropout": "attn_out",
            "output.dropout": "ffn_out"}[tail]
    return f"{SITE}.L{parts[2]}.{leaf}"


def test_dropout_sites_are_where_transformers_has_them():
    m = _hf_model(P_DROP).train()
    ids, mask, R = _inputs()
    H = CFG["num_attention_heads"]
    drop = Drop(SEED, P_DROP)
    hooked = []
    for name, mod in m.named_modules():
        if type(mod).__name__ in ("Dropout", "StableDropout"):
            site = _hf_site(name)

            def fwd(x, site=site):
                if site.endswith(".attn"):  # [B, H, L, L], or the same flattened over (B, H)
                    return drop(site, x.reshape(-1, H, x.shape[-2], x.shape[-1])).reshape(x.shape)
                return drop(site, x)

            mod.forward = fwd
            hooked.append(site)
    assert sorted(hooked) == sorted(sites(CFG["num_hidden_layers"])), hooked
    out = m(input_ids=ids, attention_mask=mask).last_hidden_state
    (out * R).sum().backward()  # R is 0 on the padded rows: a loss over real-token rows only
    hf_grads = {n: p.grad for n, p in m.named_parameters()}

    P = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    d = CFG["hidden_size"] // H
    hf_scale = float(torch.sqrt(torch.tensor(d, dtype=torch.float) * 3))  # transformers' scaled_size_sqrt
    ref = deberta_forward_drop(P, ids, mask, num_layers=CFG["num_hidden_layers"], num_heads=H, drop=drop,
                               score_scale=hf_scale)
    (ref * R).sum().backward()
    real = mask.bool()
    e = _rel(ref.detach()[real], out.detach()[real])
    print(f"last_hidden_state, real-token rows: relative error {e:.3e}")
    assert e <= 1e-10, e
    # dropout really changed the result (the check above is not vacuous)
    plain = deberta_forward_drop({k: v.detach() for k, v in P.items()}, ids, mask, num_layers=2, num_heads=H)
    assert _rel(plain[real], out.detach()[real]) > 1e-2
    worst = ("", 0.0)
    for n, g in hf_grads.items():
        assert g is not None and P[n].grad is not None, n
        e = _rel(P[n].grad, g)
        worst = max(worst, (n, e), key=lambda t: t[1])
        assert e <= 1e-10, (n, e)
    print(f"parameter gradients: worst relative error {worst[1]:.3e} ({worst[0]})")
    assert np.isfinite(worst[1])
