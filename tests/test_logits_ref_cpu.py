"""tests/logits_ref.py (the restatement csrc/logits.hip is compared with bit for bit) against transformers' own
logits processor classes, bit for bit on random fp32 rows; and, driven with the recorded float64 logits of
tests/golden/blip_small_processors.npz, against that fixture's ids without transformers. The host-side argument
checks of mmfd.kernels.check_processors are here too: they need no GPU."""
import json
import os

import numpy as np
import pytest
import torch

from tests import blip_refs as R
from tests import logits_ref as LR

EOS = 2


def _rows(Rn, V, cur, seed, dup=True):
    g = torch.Generator().manual_seed(seed)
    scores = torch.randn(Rn, V, generator=g) * 3.0
    hist = torch.randint(0, V, (Rn, cur), generator=g)
    if dup and cur >= 4:
        hist[:, 1] = hist[:, 3] = hist[:, 0]  # one id three times in every row
    return scores, hist


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def LP():
    pytest.importorskip("transformers")
    from transformers.generation import logits_process
    return logits_process


@pytest.mark.parametrize("Rn,V,cur", [(1, 7, 3), (3, 200, 9), (4, 500, 21), (2, 50, 1)])
def test_penalty_equals_transformers_bit_for_bit(LP, Rn, V, cur):
    scores, hist = _rows(Rn, V, cur, seed=V + cur)
    scores[0, hist[0, 0]] = 0.0      # a penalised column that is exactly 0, and one that is -0.0
    scores[-1, hist[-1, -1]] = -0.0
    for b in range(Rn):              # negative and positive scores under the penalty
        scores[b, hist[b, cur // 2]] = (-1.0) ** b * 2.5
    for p in (1.3, 0.7, 2.0):
        want = LP.RepetitionPenaltyLogitsProcessor(p)(hist, scores.clone())
        got = LR.process(scores, hist, repetition_penalty=p)
        assert _bits(got, want)
        assert not torch.equal(got, scores)
    assert _bits(LR.process(scores, hist), scores)  # every default: nothing happens


def test_penalty_counts_a_repeated_id_once(LP):
    scores = torch.tensor([[4.0, -4.0, 1.0, 8.0]])
    hist = torch.tensor([[0, 1, 0, 0, 1, 0]])
    got = LR.process(scores, hist, repetition_penalty=2.0)
    assert got.tolist() == [[2.0, -8.0, 1.0, 8.0]]
    assert _bits(got, LP.RepetitionPenaltyLogitsProcessor(2.0)(hist, scores.clone()))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 9, 10])
def test_ngram_equals_transformers(LP, n):
    V, cur = 12, 9  # a small vocabulary: n-grams repeat by chance
    scores, hist = _rows(6, V, cur, seed=n, dup=False)
    # row 0: the suffix (3, 4) matches two windows with different last ids, 5 and 7
    hist[0] = torch.tensor([3, 4, 5, 1, 3, 4, 7, 3, 4])
    want = LP.NoRepeatNGramLogitsProcessor(n)(hist, scores.clone())
    got = LR.process(scores, hist, no_repeat_ngram_size=n)
    assert _bits(got, want)
    if n == 3:
        assert sorted(LR.banned_ngram_tokens(hist[0].tolist(), 3)) == [5, 7]
        assert torch.isinf(got[0, [5, 7]]).all() and torch.isfinite(got[0, [3, 4]]).all()
    if n == 1:
        for b in range(6):
            assert set(torch.nonzero(torch.isinf(got[b]))[:, 0].tolist()) == set(hist[b].tolist())
    if n > cur:
        assert _bits(got, scores)  # no window of more ids than the row holds


@pytest.mark.parametrize("cur,prompt_len,min_length,min_new", [(3, 1, 5, 0), (5, 1, 5, 0), (4, 3, 0, 2), (5, 3, 0, 2),
                                                               (4, 3, 0, 1), (6, 2, 9, 3)])
def test_min_lengths_equal_transformers(LP, cur, prompt_len, min_length, min_new):
    scores, hist = _rows(3, 40, cur, seed=cur + min_length)
    want = scores.clone()
    if min_length:
        want = LP.MinLengthLogitsProcessor(min_length, EOS)(hist, want)
    if min_new:
        want = LP.MinNewTokensLengthLogitsProcessor(prompt_len, min_new, EOS)(hist, want)
    got = LR.process(scores, hist, min_length=min_length, min_new_tokens=min_new, eos=EOS, prompt_len=prompt_len)
    assert _bits(got, want)
    assert bool(torch.isinf(got[:, EOS]).all()) == LR.suppress_eos(cur, prompt_len, min_length, min_new)


def test_suppress_tokens_equal_transformers(LP):
    scores, hist = _rows(3, 200, 5, seed=3)
    for sup in ([7], [EOS, 0, 199], list(range(100, 164))):  # eos inside the list; 64 ids
        want = LP.SuppressTokensLogitsProcessor(sup)(hist, scores.clone())
        assert _bits(LR.process(scores, hist, suppress_tokens=sup), want)
    assert _bits(LR.process(scores, hist, suppress_tokens=[]), scores)


def test_all_rules_in_transformers_order(LP):
    from transformers import LogitsProcessorList
    scores, hist = _rows(5, 60, 11, seed=8)
    hist[:, -1] = hist[:, 2]  # the last id has occurred before: its successor then is banned under n = 2
    chain = LogitsProcessorList([LP.RepetitionPenaltyLogitsProcessor(1.3), LP.NoRepeatNGramLogitsProcessor(2),
                                 LP.MinLengthLogitsProcessor(20, EOS), LP.MinNewTokensLengthLogitsProcessor(3, 12, EOS),
                                 LP.SuppressTokensLogitsProcessor([5, 6, EOS])])
    want = chain(hist, scores.clone())
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=20, min_new_tokens=12,
              suppress_tokens=[5, 6, EOS], eos=EOS, prompt_len=3)
    got = LR.process(scores, hist, **kw)
    assert _bits(got, want)
    for b, cols in enumerate(LR.touched(hist, **kw)):
        same = torch.ones(60, dtype=torch.bool)
        same[list(cols)] = False
        assert _bits(got[b][same], scores[b][same])  # nothing outside the touched columns moves
    # on log-probabilities (the beam path) the penalty multiplies: every penalised entry falls
    lp = torch.log_softmax(scores, -1)
    pen = LR.beam_logprobs(scores, hist, repetition_penalty=1.3)
    for b in range(5):
        ids = hist[b].unique()
        assert _bits(pen[b, ids], lp[b, ids] * torch.tensor(1.3)) and (pen[b, ids] < lp[b, ids]).all()


def test_argmax_rule():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[1.0, 3.0, 3.0, nan], [nan, -inf, -inf, nan], [nan, nan, nan, nan], [-0.0, 0.0, -1.0, -2.0]])
    assert LR.argmax_rule(x).tolist() == [1, 1, 0, 0]


# ---------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(R.G, "blip_small_processors.npz"), allow_pickle=False)
    return z, json.loads(str(z["cases"]))


def test_fixture_meets_its_conditions(fx):
    z, cases = fx
    assert [c["mode"] for c in cases] == ["greedy"] * 5 + ["beams"] * 3
    assert os.path.getsize(os.path.join(R.G, "blip_small_processors.npz")) < 1 << 20
    for i, c in enumerate(cases):
        assert float(z[f"c{i}.margin"]) >= 4e-4
    assert cases[0]["special"] and cases[5]["special"]
    assert cases[4]["prompt"][0] == 198 and len(cases[4]["prompt"]) == 3
    assert cases[7]["length_penalty"] == 0.0 and cases[7]["early_stopping"] is True


@pytest.mark.parametrize("case", range(5))
def test_restatement_reproduces_the_greedy_fixture_from_recorded_logits(fx, case):
    """no transformers: the recorded float64 logits are those of the fixture's own ids, so feeding them step by
    step is a faithful model as long as the restatement keeps choosing the fixture's tokens — and one wrong
    choice shows as a wrong id"""
    z, cases = fx
    c = cases[case]
    want = torch.from_numpy(z[f"c{case}.sequences"])
    logits = torch.from_numpy(z[f"c{case}.logits"])
    P = len(c["prompt"])
    assert logits.dtype == torch.float64 and logits.shape[0] == want.shape[1] - P
    step = iter(range(logits.shape[0]))
    trace = []
    got = LR.greedy(lambda ids: logits[next(step)], want.shape[0], c["prompt"], c["max_new_tokens"], EOS, 0, trace=trace,
                    **c["processors"])
    assert torch.equal(got, want)
    # the margin the fixture records is the one of these processed scores
    gaps = [float(s.sort(-1, descending=True)[0][b, 0] - s.sort(-1, descending=True)[0][b, 1])
            for _, s, live in trace for b in range(want.shape[0]) if live[b]]
    assert abs(min(gaps) - float(z[f"c{case}.margin"])) <= 1e-12
    # and fp32 processors on the fp32-rounded logits choose the same ids: what the GPU test relies on
    step = iter(range(logits.shape[0]))
    got32 = LR.greedy(lambda ids: logits[next(step)].float(), want.shape[0], c["prompt"], c["max_new_tokens"], EOS, 0,
                      **c["processors"])
    assert torch.equal(got32, want)
    if case == 0:
        hit = False
        for i, (raw, _, live) in enumerate(trace):
            cols = LR.touched(want[:, :P + i], eos=EOS, prompt_len=P, **c["processors"])
            hit |= any(live[b] and int(raw[b].argmax()) in cols[b] for b in range(want.shape[0]))
        assert hit  # a step whose raw argmax is a penalised column: the fused argmax alone would be wrong


# ---------------------------------------------------------------------------------------------
# argument checks (host only)
# ---------------------------------------------------------------------------------------------
def test_check_processors():
    from mmfd import kernels as K
    assert K.check_processors() == (1.0, 0, 0, 0, ())
    assert K.check_processors(1.3, 2, 10, 12, [3, 4], 200) == (1.3, 2, 10, 12, (3, 4))
    assert K.check_processors(suppress_tokens=torch.tensor([5, 6]))[4] == (5, 6)
    assert K.check_processors(suppress_tokens=list(range(64)), vocab_size=64)[4] == tuple(range(64))
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
               dict(repetition_penalty=float("inf")), dict(repetition_penalty="a"), dict(no_repeat_ngram_size=-1),
               dict(no_repeat_ngram_size=1.5), dict(min_length=-2), dict(min_length=2.5), dict(min_new_tokens=-1),
               dict(min_new_tokens=0.5), dict(suppress_tokens=list(range(65))), dict(suppress_tokens=[-1]),
               dict(suppress_tokens=[200], vocab_size=200), dict(suppress_tokens=[1.5])):
        with pytest.raises(ValueError):
            K.check_processors(**kw)
