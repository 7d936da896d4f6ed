"""The float64 single-token restatement of BLIP's decoder (tests/blip_refs.py) against transformers' own
outputs in tests/golden/blip_small.npz (make_blip_small.py): its logits match to 1e-5, its greedy loop
reproduces the generated ids exactly. This pins the step formulation (K|V caches, select rule) that
tests/test_caption_gpu.py compares the kernels with. The fixture's own conditions are re-asserted from
the stored arrays."""
import numpy as np
import torch

from tests import blip_refs as R


def test_fixture_meets_its_conditions():
    z, cfg, _ = R.load_fixture()
    tc = cfg["text"]
    seq, scores = z["sequences"], z["scores"]
    eos, pad = tc["sep_token_id"], tc["pad_token_id"]
    assert seq.shape == (4, 21) and (seq[:, 0] == tc["bos_token_id"]).all()
    assert len({tuple(r) for r in seq.tolist()}) == 4                      # pairwise distinct
    stops = [int(np.nonzero(r[1:] == eos)[0][0]) + 1 if (r[1:] == eos).any() else None for r in seq]
    assert any(n is not None and 3 <= n < 20 for n in stops), stops        # one stops early after >= 3 tokens
    assert any(n is None for n in stops), stops                            # one runs all 20
    for r, n in zip(seq, stops):                                           # pad after eos
        assert n is None or (r[1 + n:] == pad).all()
    live = R.live_mask(seq, eos)
    top2 = np.sort(scores, axis=-1)[..., -2:]
    margin = float((top2[..., 1] - top2[..., 0])[live].min())
    assert margin >= 0.05 and abs(margin - float(z["margin"])) < 1e-6, (margin, float(z["margin"]))
    assert (scores.argmax(-1).T[live.T] == seq[:, 1:][live.T]).all()       # the scores are those of the ids
    assert list(z["keys"]) == [k[2:] for k in z.files if k.startswith("w.")]
    assert np.abs(z["logits"] - scores)[live].max() < 2e-4                 # float64 pass vs generate's fp32 scores


def test_vision_restatement_matches_transformers():
    z, cfg, W = R.load_fixture()
    emb = R.vision(W, cfg, torch.from_numpy(z["pixel_values"]))
    err = (emb - torch.from_numpy(z["image_embeds"]).double()).abs().max().item()
    print(f"image_embeds: float64 restatement vs transformers fp32 {err:.3e}")
    assert err < 1e-5, err


def test_single_token_step_logits_match_transformers():
    z, cfg, W = R.load_fixture()
    seq = torch.from_numpy(z["sequences"])
    emb = R.vision(W, cfg, torch.from_numpy(z["pixel_values"]))
    logits = R.forced_logits(W, cfg, emb, seq[:, :20])
    err = (logits - torch.from_numpy(z["logits"]).double()).abs().max().item()
    print(f"teacher-forced logits: restatement vs the fixture {err:.3e}")
    assert logits.shape == (20, 4, cfg["text"]["vocab_size"])
    assert err < 1e-5, err


def test_greedy_loop_reproduces_the_generated_ids():
    z, cfg, W = R.load_fixture()
    emb = R.vision(W, cfg, torch.from_numpy(z["pixel_values"]))
    out = R.greedy(W, cfg, emb)
    assert torch.equal(out, torch.from_numpy(z["sequences"]))
    # a prompt of a stored row's first tokens continues that row as stored
    row = int(np.argmax([(r[1:] != cfg["text"]["pad_token_id"]).sum() for r in z["sequences"]]))
    out = R.greedy(W, cfg, emb, max_new_tokens=18, prompt=z["sequences"][row, :3].tolist())
    assert torch.equal(out[row], torch.from_numpy(z["sequences"][row]))


def test_select_rule():
    am = torch.tensor([5, 2, 7, 9])
    fin = torch.tensor([False, False, True, False])
    tok, f2 = R.select(am, fin, eos=2, pad=0)
    assert tok.tolist() == [5, 2, 0, 9] and f2.tolist() == [False, True, True, False]
    tok, f3 = R.select(am, f2, eos=2, pad=0, forced=torch.tensor([1, 1, 1, 2]))
    assert tok.tolist() == [1, 1, 1, 2] and f3.tolist() == [False, True, True, True]
