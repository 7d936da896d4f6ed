"""Beam search without a GPU: tests/beam_ref.py (the plain-torch restatement the kernels are compared with)
against transformers' own `generate(num_beams=...)`, the claim that the steps a captured graph runs after
transformers has left its loop change nothing, the conditions of tests/golden/blip_small_beams.npz, and
PIL's bicubic taps (mmfd.preprocess.pil_taps) against Image.resize."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import beam_ref as BR
from tests import blip_refs as R

CASES = [(2, 1.0, False), (3, 1.0, False), (3, 0.0, True), (4, 2.0, False)]
NEW = 20
# image sizes as array shapes (h, w) -> square output; the list of mmfd.preprocess's "blip" mode
SIZES = [((5, 7), 16), ((33, 47), 16), ((16, 40), 16), ((97, 61), 48), ((1, 1), 8), ((2, 300), 24), ((400, 384), 384),
         ((13, 384), 384)]


def _maker():
    spec = importlib.util.spec_from_file_location("make_blip_small_beams",
                                                  os.path.join(R.G, "make_blip_small_beams.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def hf():
    mk = _maker()
    model, px, z, cfg = mk.hf_model()
    mk.EOS = cfg["text"]["sep_token_id"]
    return dict(mk=mk, model=model, px=px, z=z, tc=cfg["text"])


@pytest.mark.parametrize("with_prompt", [False, True], ids=["bos", "prompt3"])
@pytest.mark.parametrize("nb,lp,es", CASES)
def test_restatement_returns_transformers_ids_and_extra_steps_are_harmless(hf, nb, lp, es, with_prompt):
    """transformers' generate against the restatement driven step by step with the same model's logits — once
    leaving the loop where transformers does, once forced through all max_new_tokens steps (what a captured graph
    runs): the same ids and scores both times"""
    mk, model, px, tc = hf["mk"], hf["model"], hf["px"], hf["tc"]
    greedy = hf["z"]["sequences"]
    row = int((greedy[:, 1:] != tc["pad_token_id"]).sum(1).argmax())
    prompt_ids = torch.from_numpy(greedy[row, :3].copy()) if with_prompt else None
    prompt = mk.prompt_list(prompt_ids, tc)
    out = mk.hf_generate(model, px, prompt_ids, nb, lp, es, NEW)
    fn = mk.logits_fn(model, px, nb)
    args = (fn, px.shape[0], nb, prompt, NEW, tc["sep_token_id"], tc["pad_token_id"], lp, es)
    trace = []
    (ids, scores), _ = BR.search(*args, trace=trace)
    (ids_all, scores_all), _ = BR.search(*args, run_all_steps=True)
    print(f"{(nb, lp, es)} prompt {prompt}: transformers' loop ran {len(trace)} of {NEW} steps, width {ids.shape[1]}")
    assert torch.equal(ids, out.sequences)
    assert (scores.double() - out.sequences_scores.double()).abs().max().item() < 1e-4
    assert torch.equal(ids_all, ids) and torch.equal(scores_all, scores)
    # a batch leaves only when its last image is done: one image at a time the loop ends (much) earlier
    left_early = 0
    for b in range(px.shape[0]):
        one = (mk.logits_fn(model, px[b:b + 1], nb), 1) + args[2:]
        trace = []
        (i1, s1), _ = BR.search(*one, trace=trace)
        (i2, s2), _ = BR.search(*one, run_all_steps=True)
        left_early += len(trace) < NEW
        assert torch.equal(i1, i2) and torch.equal(s1, s2)
        w = min(i1.shape[1], ids.shape[1])
        assert torch.equal(i1[0, :w], ids[b, :w])  # (and the rows of a batch are independent)
    print(f"  single images: {left_early} of {px.shape[0]} left before the last step")


def test_extra_steps_are_taken_somewhere(hf):
    """the harmlessness test above is not vacuous: with early_stopping=True transformers leaves before the last step"""
    mk, model, px, tc = hf["mk"], hf["model"], hf["px"], hf["tc"]
    trace = []
    BR.search(mk.logits_fn(model, px[3:4], 3), 1, 3, [tc["bos_token_id"]], NEW, tc["sep_token_id"],
              tc["pad_token_id"], 0.0, True, trace=trace)
    assert len(trace) < NEW - 5


def test_topk_rule():
    nan = float("nan")
    v = torch.tensor([[1.0, 3.0, 3.0, nan, -float("inf"), 0.0, -0.0], [nan, nan, nan, nan, nan, nan, nan]])
    assert BR.topk_rule(v, 7).tolist() == [[1, 2, 0, 5, 6, 4, 3], [0, 1, 2, 3, 4, 5, 6]]


def test_beam_fixture_meets_its_conditions():
    z = np.load(os.path.join(R.G, "blip_small_beams.npz"), allow_pickle=False)
    g, cfg, _ = R.load_fixture()
    tc = cfg["text"]
    cases = json.loads(str(z["cases"]))
    assert [(c["num_beams"], c["length_penalty"], c["early_stopping"]) for c in cases] == CASES + CASES
    differs = early = runs_out = False
    for i, c in enumerate(cases):
        seq, P = z[f"c{i}.sequences"], len(c["prompt"])
        assert float(z[f"c{i}.margin"]) >= 4e-4
        assert seq.shape[0] == 4 and (seq[:, :P] == np.array(c["prompt"])).all() and seq[0, 0] == tc["bos_token_id"]
        assert (f"c{i}.pixels64" in z.files) == (c["pixel_seed"] >= 0)
        gen = seq[:, P:]
        stopped = (gen == tc["sep_token_id"]).any(1)
        early |= bool((stopped & ((gen == tc["sep_token_id"]).argmax(1) + 1 < c["max_new_tokens"])).any())
        runs_out |= bool((~stopped).any()) and gen.shape[1] == c["max_new_tokens"]
        if P == 1 and c["pixel_seed"] < 0:
            w = min(seq.shape[1], g["sequences"].shape[1])
            differs |= bool((seq[:, :w] != g["sequences"][:, :w]).any())
    assert differs and early and runs_out


# ---------------------------------------------------------------------------------------------
# PIL's taps
# ---------------------------------------------------------------------------------------------
def two_pass(a, taps_x, taps_y):
    """PIL's 8-bit resize of an [h, w, 3] array: the horizontal pass, then the vertical one, each 22-bit fixed
    point with rounding and a clip to uint8 (what csrc/preprocess.hip runs with these taps)"""
    def run(x, taps):
        out = np.zeros((x.shape[0], taps.shape[0], 3), np.uint8)
        for i, rec in enumerate(taps):
            acc = np.full((x.shape[0], 3), 1 << 21, np.int64)
            for k in range(rec[1]):
                acc += x[:, rec[0] + k, :].astype(np.int64) * int(rec[2 + k])
            out[:, i, :] = np.clip(acc >> 22, 0, 255)
        return out
    return run(run(a, taps_x).transpose(1, 0, 2), taps_y).transpose(1, 0, 2)


def random_image(h, w, seed):
    """uint8 [h, w, 3] with about 30 % of the pixels saturated (the clip after a negative bicubic lobe matters)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    sat = rng.random((h, w, 3))
    a[sat < 0.15] = 0
    a[sat > 0.85] = 255
    return a


@pytest.mark.parametrize("hw,S", SIZES)
def test_bicubic_taps_reproduce_pil(hw, S):
    from PIL import Image
    from mmfd.preprocess import pil_taps
    h, w = hw
    a = random_image(h, w, seed=h * 1000 + w)
    ref = np.asarray(Image.fromarray(a).resize((S, S), Image.BICUBIC))
    got = two_pass(a, pil_taps(w, S, "bicubic"), pil_taps(h, S, "bicubic"))
    assert got.shape == ref.shape and int((got != ref).sum()) == 0


def test_bilinear_taps_are_what_they_were():
    from mmfd.preprocess import MODES, pil_taps
    z = np.load(os.path.join(R.G, "pil_taps_bilinear.npz"), allow_pickle=False)  # written by the code before "bicubic"
    for i, o in ((5, 16), (33, 16), (640, 384)):
        t = pil_taps(i, o)
        assert t.dtype == np.int32 and np.array_equal(t, z[f"t{i}_{o}"])
        assert np.array_equal(pil_taps(i, o, "bilinear"), t)
    assert (pil_taps(33, 16, "bicubic")[:, 2:] < 0).any()  # the negative lobes
    with pytest.raises(ValueError):
        pil_taps(5, 16, "lanczos")
    assert set(MODES) == {"train", "retrieval", "evaluate", "blip"} and MODES["blip"]["resize"] == (384, 384)
