"""Trainable DeBERTa-v3 encoder, the parts that need no GPU: configuration and CLI surface, the
oracle's gradient pinned against the transformers fixture (tests/golden/deberta_small_grads.npz,
make_deberta_grads.py), and the host check that guards the relative-bias backward kernel."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_config_defaults_and_state_dict_names():
    from mmfd.deberta import DebertaV2Config, DebertaV2Model
    c = DebertaV2Config()
    assert c.trainable is False and c.hidden_dropout_prob == 0.0 and c.attention_probs_dropout_prob == 0.0
    m = DebertaV2Model(vocab_size=50, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64)
    assert m.config.trainable is False
    z = np.load(os.path.join(G, "deberta_small.npz"))
    hf = {k[2:] for k in z.files if k.startswith("w.")}
    from mmfd.deberta import DebertaV2Model as M
    small = M(vocab_size=1000, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
              trainable=True)
    assert set(small.state_dict().keys()) == hf
    assert set(DebertaV2Model().state_dict().keys()) >= {"encoder.rel_embeddings.weight", "encoder.LayerNorm.weight",
                                                         "embeddings.word_embeddings.weight",
                                                         "encoder.layer.11.attention.self.query_proj.weight"}


def test_cli_flag_parses():
    from mmfd.train import parse_args
    assert parse_args([]).train_text_encoder is False
    assert parse_args(["--train_text_encoder"]).train_text_encoder is True


def test_build_encoders_trainable_deberta():
    from mmfd.deberta import DebertaV2Model
    from mmfd.train import build_encoders, parse_args
    vit = ["--image_encoder", "google/vit-base-patch16-224"]
    text, _, text_frozen, _ = build_encoders(parse_args(vit + ["--train_text_encoder"]), "cpu")
    assert isinstance(text, DebertaV2Model) and text.config.trainable and text_frozen is False
    text, _, text_frozen, _ = build_encoders(parse_args(vit + ["--train_text_encoder", "--freeze_text"]), "cpu")
    assert isinstance(text, DebertaV2Model) and text_frozen is True
    text, _, text_frozen, _ = build_encoders(parse_args(vit), "cpu")
    assert not text.config.trainable and text_frozen is True


def test_oracle_gradients_match_transformers_fixture():
    """autograd through oracle.deberta.deberta_forward reproduces transformers' gradients of
    (last_hidden_state * R).sum(): |delta|max <= 1e-6 * max(1, |g|max) for every parameter"""
    from oracle.deberta import deberta_forward
    z = np.load(os.path.join(G, "deberta_small.npz"))
    gz = np.load(os.path.join(G, "deberta_small_grads.npz"))
    P = {k[2:]: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files if k.startswith("w.")}
    out = deberta_forward(P, torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"]), num_layers=2,
                          num_heads=2, eps=1e-7)
    (out * torch.from_numpy(gz["R"])).sum().backward()
    names = [k[2:] for k in gz.files if k.startswith("g.")]
    assert set(names) == set(P.keys())
    for n in names:
        ref = torch.from_numpy(gz["g." + n])
        err = (P[n].grad - ref).abs().max().item()
        assert err <= 1e-6 * max(1.0, ref.abs().max().item()), (n, err, ref.abs().max().item())
    # padded query rows reach value_proj but not query_proj: the fixture has such rows
    assert int(z["attention_mask"][1].sum()) == 171


@pytest.mark.parametrize("S,L", [(32, 80), (256, 300), (256, 512)])
def test_host_monotonicity_check(S, L):
    from mmfd import kernels as K
    from mmfd.deberta import log_bucket_relative_positions
    rel = log_bucket_relative_positions(L, S, 512)
    c2p = np.clip(rel + S, 0, 2 * S - 1).astype(np.int32)
    p2c = np.clip(-rel + S, 0, 2 * S - 1).astype(np.int32)
    hi, lo = K.check_rel_index_runs(c2p, p2c)
    assert 0 <= lo and hi < 2 * S
    K.check_rel_index_runs(torch.from_numpy(c2p), torch.from_numpy(p2c))  # tensors too
    rng = np.random.default_rng(L)
    for which in (0, 1):
        bad = [c2p.copy(), p2c.copy()]
        row = L // 2
        perm = rng.permutation(L)
        while np.array_equal(bad[which][row][perm], bad[which][row]):
            perm = rng.permutation(L)
        bad[which][row] = bad[which][row][perm]
        with pytest.raises(ValueError):
            K.check_rel_index_runs(*bad)
