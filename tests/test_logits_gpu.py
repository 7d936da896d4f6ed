"""Logits processors on the HIP path: csrc/logits.hip against tests/logits_ref.py bit for bit on the same fp32
input; the row argmax after the edits; the beam path (log-softmax once, edits, selection without a second
normalisation) against float64; sample_select on edited logits; mmfd.blip's `generate(repetition_penalty=...,
no_repeat_ngram_size=..., min_length=..., min_new_tokens=..., suppress_tokens=...)` in all three decoding modes
against transformers' outputs (tests/golden/blip_small_processors.npz, whose restatement
tests/test_logits_ref_cpu.py holds to transformers' classes); graph keys, defaults, refusals and the Captioner.

Tolerances. Kernel: none (bit for bit; the division is IEEE fp32). Beam log-probabilities: err <= 3e-5 + 3e-5
|ref|max, test_beam_gpu.py's selection bound, the reference being float64 log_softmax of the same fp32 logits, then
the rule in float64 (a penalised entry is at most 1.3 x a log-probability, inside |ref|max). Sampling: sample_ref's
TOL. Model: ids equal, beam scores within margin / 4 of the fixture's."""
import json
import os

import numpy as np
import pytest
import torch

from tests import blip_refs as R
from tests import logits_ref as LR
from tests import sample_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
INF = float("inf")
EOS = 2


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------
# the edit kernel
# ---------------------------------------------------------------------------------------------
SHAPES = [(1, 7, 3), (3, 200, 9), (32, 30524, 21), (16, 30524, 1)]
_INPUTS = {}


def _inputs(Rn, V, cur):
    """(scores fp32 [R, V], history int64 [R, cur]) of a shape, built once and never modified. Every row: the ids
    N(0, 3^2) scores and random ids; the last id has occurred before where cur >= 3 (so n = 2 bans its successor);
    row 0 holds one id four times where cur >= 5; with three rows or more the column of row 0's first id is exactly
    0 and that of the last row's second id -0.0."""
    key = (Rn, V, cur)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(V * 31 + cur)
        scores = torch.randn(Rn, V, generator=g) * 3.0
        hist = torch.randint(0, V, (Rn, cur), generator=g)
        if cur >= 3:
            hist[:, -1] = hist[:, 0]
        if cur >= 5:
            hist[0, 1] = hist[0, 2] = hist[0, 4] = hist[0, 3]
        if Rn >= 3:
            scores[0, hist[0, 0]] = 0.0
            if cur >= 2:
                scores[-1, hist[-1, 1]] = -0.0
        _INPUTS[key] = (scores, hist)
    return _INPUTS[key]


def _device_history(hist, layout):
    """the history inside a larger buffer whose other entries hold an id that must never be read (V + 9 would be
    ignored; a valid one would show): int64 step-major with a row stride larger than R, or int32 row-major"""
    Rn, cur = hist.shape
    if layout == "steps":
        buf = torch.full((cur + 2, Rn + 3), 1, dtype=torch.int64)
        buf[:cur, :Rn] = hist.t()
        return buf.to(DEV)
    buf = torch.full((Rn + 1, cur + 2), 1, dtype=torch.int32)
    buf[:Rn, :cur] = hist.int()
    return buf.to(DEV)


def _run_edit(scores, hist, layout, **kw):
    """one launch on scores staged as a strided view whose padding columns hold NaN, inside a buffer with guard
    rows; returns (edited scores on the CPU, the whole buffer)"""
    from mmfd import kernels as K
    Rn, V = scores.shape
    buf = torch.full((Rn + 2, V + 5), NAN)
    buf[0] = buf[-1] = 7.0
    buf[1:1 + Rn, :V] = scores
    dbuf = buf.to(DEV)
    sup = kw.pop("suppress_tokens", None)
    dsup = None if sup is None else torch.tensor(list(sup) + [1, 1], dtype=torch.int64, device=DEV)
    K.logits_process(dbuf[1:1 + Rn, :V], _device_history(hist, layout), hist.shape[1], suppress=dsup,
                     n_suppress=None if sup is None else len(sup), history_layout=layout, **kw)
    torch.cuda.synchronize()
    out = dbuf.cpu()
    assert (out[0] == 7.0).all() and (out[-1] == 7.0).all() and torch.isnan(out[1:1 + Rn, V:]).all()
    return out[1:1 + Rn, :V]


def _rules(V, cur):
    sup64 = [EOS] + list(range(V - 63, V)) if V >= 64 else list(range(V))
    return [
        ("penalty", dict(repetition_penalty=1.3), {}),
        ("penalty < 1", dict(repetition_penalty=0.7), {}),
        ("n = 1", dict(no_repeat_ngram_size=1), {}),
        ("n = 2", dict(no_repeat_ngram_size=2), {}),
        ("n = cur", dict(no_repeat_ngram_size=cur), {}),
        ("n = cur + 1", dict(no_repeat_ngram_size=cur + 1), {}),
        ("eos", dict(), dict(suppress_eos=True, eos=EOS)),
        ("64 ids", dict(suppress_tokens=sup64), {}),
        ("empty list", dict(suppress_tokens=[]), {}),
        ("all", dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=sup64[:5]),
         dict(suppress_eos=True, eos=EOS)),
    ]


@pytest.mark.parametrize("layout", ["steps", "rows"])
@pytest.mark.parametrize("Rn,V,cur", SHAPES)
def test_edit_kernel_matches_the_restatement_bit_for_bit(Rn, V, cur, layout):
    scores, hist = _inputs(Rn, V, cur)
    for name, ref_kw, dev_kw in _rules(V, cur):
        ref_extra = dict(min_length=cur + 1, eos=EOS) if dev_kw else {}
        want = LR.process(scores, hist, **ref_kw, **ref_extra)
        got = _run_edit(scores, hist, layout, **ref_kw, **dev_kw)
        assert _bits(got, want), (name, (got != want).nonzero()[:8])
        if name in ("n = cur + 1", "empty list"):
            assert _bits(got, scores)
        elif name != "n = cur" and not (name == "n = 2" and cur < 3):
            assert not _bits(got, scores), name


def test_an_id_held_four_times_is_penalised_once_and_zeros_keep_their_sign():
    scores, hist = _inputs(3, 200, 9)
    got = _run_edit(scores, hist, "steps", repetition_penalty=2.0)
    col = int(hist[0, 3])
    assert hist[0].tolist().count(col) == 4
    s = scores[0, col]
    assert got[0, col] == (s * 2.0 if s < 0 else s / 2.0)
    assert got[0, hist[0, 0]] == 0.0 and not torch.signbit(got[0, hist[0, 0]])
    assert got[-1, hist[-1, 1]] == 0.0 and torch.signbit(got[-1, hist[-1, 1]])
    # ids outside [0, V) touch nothing, in either width
    from mmfd import kernels as K
    for dt in (torch.int64, torch.int32):
        x = scores.to(DEV).clone()
        bad = torch.tensor([[-1, 200, 2 ** 31 - 1, -5]] * 3, dtype=dt, device=DEV)
        K.logits_process(x, bad, 4, repetition_penalty=1.5, no_repeat_ngram_size=1)
        assert _bits(x.cpu(), scores)


def test_edit_wrapper_refuses_bad_arguments():
    from mmfd import kernels as K
    x = torch.zeros(2, 50, device=DEV)
    h = torch.zeros(2, 6, dtype=torch.int64, device=DEV)
    sup = torch.zeros(70, dtype=torch.int64, device=DEV)
    for bad in (lambda: K.logits_process(x, h, 7), lambda: K.logits_process(x, h, 0),
                lambda: K.logits_process(x, h[:1], 3), lambda: K.logits_process(x, h.float(), 3),
                lambda: K.logits_process(x, h, 3, repetition_penalty=0.0),
                lambda: K.logits_process(x, h, 3, no_repeat_ngram_size=-1),
                lambda: K.logits_process(x, h, 3, suppress_eos=True, eos=50),
                lambda: K.logits_process(x, h, 3, suppress=sup), lambda: K.logits_process(x, h, 3, suppress=sup[:4].int()),
                lambda: K.logits_process(x.double(), h, 3), lambda: K.logits_process(x, h, 3, history_layout="cols")):
        with pytest.raises(ValueError):
            bad()
    lib, vp = K.lib(), K._ptr
    assert lib.mmfd_logits_process(2, 50, vp(x), 50, vp(h), 6, 1, 8, 3, 1.0, 0, 0, 0, None, 0, None) == 0
    assert lib.mmfd_logits_process(2, 50, vp(x), 50, vp(h), 6, 1, 2, 3, 1.0, 0, 0, 0, None, 0, None) != 0  # int16 ids
    assert lib.mmfd_logits_process(2, 50, vp(x), 50, vp(h), 6, 1, 8, 1025, 1.0, 0, 0, 0, None, 0, None) != 0
    assert lib.mmfd_logits_process(2, 50, vp(x), 50, vp(h), 6, 1, 8, 3, 1.0, 0, 0, 0, None, 3, None) != 0  # no list
    assert lib.mmfd_logits_process(2, 50, vp(x), 50, vp(h), 6, 1, 8, 3, 1.0, 0, 0, 0, vp(sup), 65, None) != 0
    assert lib.mmfd_logits_process(2, 50, vp(x), 49, vp(h), 6, 1, 8, 3, 1.0, 0, 0, 0, None, 0, None) != 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the argmax after the edits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rn,V", [(1, 7), (3, 200), (32, 30524), (5, 30523)])
def test_row_argmax_after_edits(Rn, V):
    """rows at every alignment (ld = V + 5 with V odd and even): the planted raw argmax sits on a banned column in
    row 0 and on a penalised column that falls to second place in the last row"""
    from mmfd import kernels as K
    g = torch.Generator().manual_seed(V)
    scores = torch.randn(Rn, V, generator=g)
    hist = torch.randint(0, V, (Rn, 4), generator=g)
    a, b = 3 % V, 5 % V
    hist[:, 0] = a
    hist[-1, 1:] = a          # (the last row's history must not hold b)
    scores[:, a] = 10.0       # the raw argmax: penalised to 5 ...
    scores[-1, b] = 8.0       # ... below this one in the last row
    buf = torch.full((Rn, V + 5), NAN)
    buf[:, :V] = scores
    dbuf = buf.to(DEV)
    view = dbuf[:, :V]
    assert K.row_argmax(view).tolist() == [a] * Rn
    dh = hist.to(DEV)
    K.logits_process(view, dh, 4, repetition_penalty=2.0)
    want = LR.argmax_rule(LR.process(scores, hist, repetition_penalty=2.0))
    got = K.row_argmax(view).cpu()
    assert torch.equal(got, want) and got[-1] == b and (Rn == 1 or got[0] == a)
    ban = torch.tensor([a], dtype=torch.int64, device=DEV)
    K.logits_process(view, dh, 4, suppress=ban)
    want = LR.argmax_rule(LR.process(LR.process(scores, hist, repetition_penalty=2.0), hist, suppress_tokens=[a]))
    out = torch.full((Rn + 2,), -1, dtype=torch.int64, device=DEV)
    K.row_argmax(view, out=out[1:1 + Rn])
    assert torch.equal(out[1:1 + Rn].cpu(), want) and a not in out.tolist() and out[0] == -1 and out[-1] == -1


def test_row_argmax_ties_nans_and_infinities():
    from mmfd import kernels as K
    V = 30524
    x = torch.randn(6, V, generator=torch.Generator().manual_seed(1))
    x[0, 29000] = x[0, 1200] = x[0, 30523] = 9.0     # a tie: the lowest index
    x[1, 77] = NAN                                  # a NaN never wins ...
    x[1, 5000] = 9.0
    x[2] = NAN                                      # ... unless there is nothing else: 0
    x[3] = -INF
    x[3, 0] = NAN                                   # -inf is a number: the first of them
    x[4] = -INF
    x[4, 30522] = -1e30
    x[5, 4] = INF
    x[5, 3] = NAN
    want = LR.argmax_rule(x)
    assert want.tolist() == [1200, 5000, 0, 1, 30522, 4]
    assert torch.equal(K.row_argmax(x.to(DEV)).cpu(), want)
    with pytest.raises(ValueError):
        K.row_argmax(x.to(DEV).double())


# ---------------------------------------------------------------------------------------------
# the beam path
# ---------------------------------------------------------------------------------------------
def _bound(ref):
    return 3e-5 + 3e-5 * ref[torch.isfinite(ref)].abs().max().item()


def _beam_inputs(B, nb, V, cur, seed):
    """fp32 logits [B * nb, V] with planted, well-separated winners per image and histories that edit them: in
    beam 0 token 0 (30: banned by the suppress list) and token 1 (28: held twice by the beam's history, penalised
    once), in the last beam token V - 1 (26) and token 4 (24: held by beam 0's history only, so untouched here), in
    beam 1 % nb token 3 (22); then the rows' own best, about 18 below. The log-softmax is over the unprocessed row, so
    the banned 30 still weighs on its row's other entries. running: -0.25 per beam below the first."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B * nb, V, generator=g)
    hist = torch.randint(5, V - 1, (B * nb, cur), generator=g)
    running = (-0.25 * torch.arange(nb, dtype=torch.float32))[None].repeat(B, 1)
    for b in range(B):
        r0, rl, r1 = b * nb, b * nb + nb - 1, b * nb + 1 % nb
        logits[r0, 0], logits[r0, 1], logits[rl, V - 1], logits[rl, 4], logits[r1, 3] = 30.0, 28.0, 26.0, 24.0, 22.0
        hist[r0, 0] = hist[r0, cur - 1] = 1
        hist[r0, 1] = 4
    return logits, hist, running.reshape(-1)


@pytest.mark.parametrize("B,nb,V", [(1, 2, 7), (2, 3, 200), (2, 3, 30524)])
def test_beam_path_matches_float64(B, nb, V):
    from mmfd import kernels as K
    cur = 6
    logits, hist, running = _beam_inputs(B, nb, V, cur, seed=V + nb)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[0], min_length=cur + 1, eos=EOS)
    ref = LR.beam_logprobs(logits, hist, dtype=torch.float64, **kw)
    wide = torch.full((B * nb, V + 5), NAN)
    wide[:, :V] = logits
    x = wide.to(DEV)[:, :V]
    K.row_log_softmax(x)
    plain = x.cpu().clone()
    ref_plain = torch.log_softmax(logits.double(), -1)
    assert (plain.double() - ref_plain).abs().max().item() <= _bound(ref_plain)
    K.logits_process(x, hist.int().to(DEV), cur, repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_eos=True,
                     eos=EOS, suppress=torch.tensor([0], dtype=torch.int64, device=DEV), history_layout="rows")
    got = x.cpu()
    banned = torch.isinf(ref)
    assert torch.equal(torch.isinf(got) & (got < 0), banned) and banned[:, [0, EOS]].all()
    err = (got.double() - ref)[~banned].abs().max().item()
    print(f"beam log-probabilities {(B, nb, V)}: err {err:.3e}, bound {_bound(ref):.3e}")
    assert err <= _bound(ref)
    # an entry no processor touched is bit for bit the normalised one, and the edits are the rule on it
    assert _bits(got, LR.process(plain, hist, **kw))
    # the selection: float64's (beam, token), scores within the bound, no second normalisation
    cand = tuple(t.cpu() for t in K.beam_select_logprobs(x, running.to(DEV), nb))
    want = LR.beam_select_logprobs(ref, running.double(), nb)
    assert torch.equal(cand[1], want[1]) and torch.equal(cand[2], want[2])
    assert (cand[0].double() - want[0]).abs().max().item() <= _bound(ref)
    for b in range(B):
        flat = cand[1][b].long() * V + cand[2][b].long()
        assert len(set(flat.tolist())) == 2 * nb
        got_b = list(zip(cand[1][b].tolist(), cand[2][b].tolist()))
        assert (0, 0) not in got_b and (0, 1) in got_b  # the raw winner is banned; the penalised 28 is still chosen
    # against the unedited path: the same logits through mmfd_beam_select score what the split path's untouched
    # entries score
    s0, b0, t0 = (t.cpu() for t in K.beam_select(wide.to(DEV)[:, :V], running.to(DEV), nb))
    s1, b1, t1 = (t.cpu() for t in K.beam_select_logprobs(plain.to(DEV), running.to(DEV), nb))
    assert torch.equal(b0, b1) and torch.equal(t0, t1) and _bits(s0, s1)


def test_beam_selection_with_all_but_five_candidates_banned():
    """nb = 3: 2 nb - 1 = 5 numbers in an image's 3 V candidates, the rest -inf: still 2 nb distinct valid indices,
    the numbers first in order, then the -inf candidate of the lowest flat index"""
    from mmfd import kernels as K
    nb, V = 3, 200
    lp = torch.full((2 * nb, V), -INF)
    spots = [(0, 7, -0.5), (2, 199, -0.1), (1, 0, -3.0), (0, 150, -0.7), (2, 3, -2.0)]
    for j, tok, v in spots:
        lp[j, tok] = v
        lp[nb + j, tok] = v
    lp[nb, 0] = -4.0  # image 1 has six numbers
    running = torch.zeros(2 * nb)
    s, bm, tk = (t.cpu() for t in K.beam_select_logprobs(lp.to(DEV), running.to(DEV), nb))
    order = [(2, 199), (0, 7), (0, 150), (2, 3), (1, 0)]
    assert list(zip(bm[0].tolist(), tk[0].tolist())) == order + [(0, 0)]
    assert s[0, :5].tolist() == pytest.approx([-0.1, -0.5, -0.7, -2.0, -3.0]) and s[0, 5] == -INF
    assert list(zip(bm[1].tolist(), tk[1].tolist())) == order + [(0, 0)] and s[1, 5] == -4.0
    for b in range(2):
        assert ((0 <= bm[b]) & (bm[b] < nb) & (0 <= tk[b]) & (tk[b] < V)).all()
        assert len(set((bm[b].long() * V + tk[b].long()).tolist())) == 2 * nb


# ---------------------------------------------------------------------------------------------
# sampling on edited logits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 5, 0.95)])
@pytest.mark.parametrize("V", [200, 1001])
def test_sample_select_on_edited_logits(V, T, k, p):
    """processors, then warpers: probs equal the float64 softmax over what survives both, banned columns have
    probability exactly 0 and are not counted as kept"""
    from mmfd import kernels as K
    Rn, cur = 8, 7
    x = torch.from_numpy(np.stack([S.make_logits(V, s) for s in range(40, 40 + 3 * Rn)]))
    g = torch.Generator().manual_seed(V)
    hist_all = torch.randint(0, V, (x.shape[0], cur), generator=g)
    hist_all[:, -1] = hist_all[:, 1]
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[EOS, 9, 11], min_length=cur + 1, eos=EOS)
    edited_all = LR.process(x, hist_all, **kw)
    for r in range(x.shape[0]):  # the row's largest logit is banned too: the maximum the kernel scales by moves
        edited_all[r, int(x[r].argmax())] = -INF
    refs_all = [S.filter_ref(S.quotients(row.numpy(), T), k, p) for row in edited_all]
    rows = [r for r, f in enumerate(refs_all) if S.usable(f)][:Rn]
    assert len(rows) == Rn
    x, hist, refs = x[rows], hist_all[rows], [refs_all[r] for r in rows]
    top = x.argmax(1)
    dx = x.to(DEV)
    sup = torch.tensor([EOS, 9, 11], dtype=torch.int64, device=DEV)
    K.logits_process(dx, hist.t().contiguous().to(DEV), cur, repetition_penalty=1.3, no_repeat_ngram_size=2,
                     suppress_eos=True, eos=EOS, suppress=sup, history_layout="steps")
    dx[torch.arange(Rn, device=DEV), top.to(DEV)] = -INF
    assert _bits(dx.cpu(), edited_all[rows])
    ctl = torch.tensor([77, 5], dtype=torch.int64, device=DEV)
    probs = torch.full((Rn, V), -7.0, device=DEV)
    kept = torch.full((Rn,), -1, dtype=torch.int32, device=DEV)
    tok = K.sample_select(dx, T, k, p, ctl, 3, probs=probs, kept=kept).cpu().numpy()
    probs, kept = probs.cpu().numpy(), kept.cpu().numpy()
    for r, f in enumerate(refs):
        banned = np.isinf(edited_all[rows[r]].numpy())
        assert banned.sum() >= 4 and (probs[r][banned] == 0.0).all() and not f.kept[banned].any()
        assert kept[r] == f.n_kept and kept[r] <= V - banned.sum()
        assert not ((probs[r] > 0) & ~f.kept).any()
        assert np.abs(probs[r] - f.probs).max() <= S.TOL
        assert f.kept[tok[r]] and not banned[tok[r]] and S.accepted(f, tok[r], S.uniform_ref(77, 3, 5 + r))


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    z, cfg, W = R.load_fixture()
    zp = np.load(os.path.join(R.G, "blip_small_processors.npz"), allow_pickle=False)
    cases = json.loads(str(zp["cases"]))
    for i, c in enumerate(cases):
        c["sequences"] = torch.from_numpy(zp[f"c{i}.sequences"])
        c["margin"] = float(zp[f"c{i}.margin"])
        if c["mode"] == "beams":
            c["scores"] = torch.from_numpy(zp[f"c{i}.sequences_scores"])
        c["px"] = torch.from_numpy(zp[f"c{i}.pixels64"]).float() / 64.0 if c["pixel_seed"] >= 0 else \
            torch.from_numpy(z["pixel_values"])
    return dict(z=z, cfg=cfg, W=W, px=torch.from_numpy(z["pixel_values"]), seq=torch.from_numpy(z["sequences"]),
                cases=cases)


def _model(fx, precision="fp32"):
    return R.load_model(fx["cfg"], fx["W"], precision, DEV)


@pytest.fixture(scope="module")
def model32(fx):
    return _model(fx)


def _kw(c):
    ids = None if len(c["prompt"]) == 1 else torch.tensor(c["prompt"] + [EOS])  # (generate drops the trailing [SEP])
    kw = dict(input_ids=ids, max_new_tokens=c["max_new_tokens"], **c["processors"])
    if c["mode"] == "beams":
        kw.update(num_beams=c["num_beams"], length_penalty=c["length_penalty"], early_stopping=c["early_stopping"])
    return kw


@pytest.mark.parametrize("case", range(8))
def test_fp32_reproduces_transformers(fx, model32, case):
    c = fx["cases"][case]
    for use_graph in (False, True):
        out = model32.generate(c["px"], use_graph=use_graph, **_kw(c))
        assert out.dtype == torch.int64 and torch.equal(out, c["sequences"]), (use_graph, out, c["sequences"])
        if c["mode"] == "beams":
            err = (model32.sequences_scores.double().cpu() - c["scores"]).abs().max().item()
            print(f"case {case} {'graph' if use_graph else 'eager'}: score error {err:.3e}, margin {c['margin']:.3e}")
            assert err <= c["margin"] / 4


def test_bf16_graph_equals_eager(fx):
    m = _model(fx, "bf16")
    for case in (4, 6):
        c = fx["cases"][case]
        eager = m.generate(c["px"], use_graph=False, **_kw(c))
        s_eager = m.sequences_scores.clone() if c["mode"] == "beams" else None
        graph = m.generate(c["px"], use_graph=True, **_kw(c))
        assert torch.equal(graph, eager)
        if s_eager is not None:
            assert torch.equal(m.sequences_scores, s_eager)
    kw = dict(do_sample=True, top_k=20, seed=5, num_return_sequences=2, no_repeat_ngram_size=2, repetition_penalty=1.2)
    assert torch.equal(m.generate(fx["px"], use_graph=True, **kw), m.generate(fx["px"], use_graph=False, **kw))


@pytest.mark.parametrize("mode", ["greedy", "beams", "sample"])
def test_a_new_suppress_list_replays_and_a_new_penalty_captures(fx, model32, mode):
    """the graph key and the device list: a second call with another suppress list of the same length, and one
    with another repetition_penalty, return what a fresh model returns"""
    m = model32
    m.invalidate_caches()
    extra = dict(greedy={}, beams=dict(num_beams=3), sample=dict(do_sample=True, top_k=30, seed=9))[mode]
    px = fx["px"]
    first = dict(repetition_penalty=1.3, suppress_tokens=[62, 189], **extra)
    base = m.generate(px, **first)
    assert sum(s["graph"] is not None for s in m._states.values()) == 1
    st = next(s for s in m._states.values() if s["graph"] is not None)
    g0 = st["graph"]
    calls = [dict(repetition_penalty=1.3, suppress_tokens=[14, 87], **extra),
             dict(repetition_penalty=1.1, suppress_tokens=[14, 87], **extra), first]
    got = [m.generate(px, **kw) for kw in calls]
    assert st["graph"] is g0                                                   # the same length: a replay
    assert sum(s["graph"] is not None for s in m._states.values()) == 2        # another penalty: its own graph
    assert torch.equal(got[2], base)
    fresh = _model(fx)
    for kw, out in zip(calls[:2], got[:2]):
        want = fresh.generate(px, use_graph=False, **kw)
        assert torch.equal(out, want)
        assert not any(t in out[:, 1:].tolist()[b] for b in range(out.shape[0]) for t in kw["suppress_tokens"])


def test_sampled_invariants(fx, model32):
    tc = fx["cfg"]["text"]
    kw = dict(do_sample=True, num_return_sequences=3, seed=123, max_new_tokens=20)
    out = {}
    for use_graph in (False, True):
        a = model32.generate(fx["px"], use_graph=use_graph, no_repeat_ngram_size=2, **kw)
        b = model32.generate(fx["px"], use_graph=use_graph, min_new_tokens=9, **kw)
        out[use_graph] = (a, b)
        assert a.shape[0] == 12 and b.shape[0] == 12
        for row in a.tolist():
            gen = row[:row.index(tc["sep_token_id"]) + 1] if tc["sep_token_id"] in row else row
            grams = list(zip(gen, gen[1:]))
            assert len(grams) == len(set(grams)), row
        for row in b.tolist():
            assert tc["sep_token_id"] not in row[1:1 + 9], row
        assert torch.equal(a, model32.generate(fx["px"], use_graph=use_graph, no_repeat_ngram_size=2, **kw))
    assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][1], out[True][1])


def test_min_new_tokens_beyond_max_new_tokens_runs_to_the_last_step(fx, model32):
    for extra in ({}, dict(num_beams=2), dict(do_sample=True, seed=1)):
        out = model32.generate(fx["px"], max_new_tokens=6, min_new_tokens=9, **extra)
        assert out.shape == (4, 7) and EOS not in out[:, 1:6].flatten().tolist()


def test_defaults_are_what_they_were(fx):
    from mmfd import kernels as K
    m = _model(fx)
    px = fx["px"]
    off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0, suppress_tokens=None)
    for extra in ({}, dict(num_beams=3), dict(do_sample=True, top_k=10, seed=4)):
        base = m.generate(px, **extra)
        score = m.sequences_scores.clone() if "num_beams" in extra else None
        keys = set(m._states)
        graphs = {k: s["graph"] for k, s in m._states.items()}
        launched = []
        real = {n: getattr(K, n) for n in ("logits_process", "row_argmax", "row_log_softmax", "beam_select_logprobs")}
        try:
            for n in real:
                setattr(K, n, lambda *a, _n=n, **k: launched.append(_n))
            out = m.generate(px, **off, **extra)
            eager = m.generate(px, use_graph=False, **off, **extra)
        finally:
            for n, f in real.items():
                setattr(K, n, f)
        assert torch.equal(out, base) and torch.equal(eager, base) and not launched
        if score is not None:
            assert torch.equal(m.sequences_scores, score)
        assert set(m._states) == keys                                         # no new state ...
        assert all(m._states[k]["graph"] is g for k, g in graphs.items())     # ... and no new capture
    assert torch.equal(m.generate(px), fx["seq"])


def test_generate_refuses_bad_processor_arguments(fx, model32, monkeypatch):
    from mmfd import kernels as K
    launched = []
    for name in ("gemm", "lm_head_argmax", "logits_process", "patchify"):
        monkeypatch.setattr(K, name, lambda *a, _n=name, **k: launched.append(_n))
    V = fx["cfg"]["text"]["vocab_size"]
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.3), dict(no_repeat_ngram_size=-1),
               dict(no_repeat_ngram_size=2.5), dict(min_length=-1), dict(min_length=1.5), dict(min_new_tokens=-3),
               dict(min_new_tokens=0.5), dict(suppress_tokens=list(range(65))), dict(suppress_tokens=[V]),
               dict(suppress_tokens=[-1])):
        for extra in ({}, dict(num_beams=2), dict(do_sample=True)):
            with pytest.raises(ValueError):
                model32.generate(fx["px"], **kw, **extra)
    with pytest.raises(ValueError, match="repetition_penalty"):
        model32.generate(fx["px"], repetition_penalty=0)
    with pytest.raises(ValueError, match="at most 64"):
        model32.generate(fx["px"], suppress_tokens=list(range(65)))
    assert not launched


def test_captioner_passes_the_processors_through_its_chunks(fx, model32):
    from mmfd.caption import Captioner
    from tests.toy_tokenizer import toy_tokenizer
    g = torch.Generator().manual_seed(5)
    extra = torch.round(torch.randn(5, *fx["px"].shape[1:], generator=g) * 64.0).clamp(-255, 255) / 64.0
    px = torch.cat((fx["px"], extra), 0)
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4, suppress_tokens=[62])
    cap = Captioner(model32, tokenizer=toy_tokenizer(), max_new_tokens=10, use_graph=False, num_beams=4, **proc)
    text = cap.caption(px)                                    # 9 images, 8 per chunk
    assert len(text) == 9
    assert text == cap.caption(px[:8]) + cap.caption(px[8:])  # the strings of the unchunked calls
    ids = cap.generate_ids(px)
    first = model32.generate(px[:8], use_graph=False, num_beams=4, max_new_tokens=10, **proc)
    assert torch.equal(ids[:8, :first.shape[1]], first)
    assert 62 not in ids[:, 1:].flatten().tolist() and EOS not in ids[:, 1:5].flatten().tolist()
    plain = Captioner(model32, max_new_tokens=10, use_graph=False, num_beams=4).generate_ids(px)
    assert plain.shape != ids.shape or not torch.equal(plain, ids)
    greedy = Captioner(model32, max_new_tokens=10, use_graph=False, **proc).generate_ids(px)
    assert torch.equal(greedy, model32.generate(px, use_graph=False, max_new_tokens=10, **proc))
    with pytest.raises(ValueError):
        Captioner(model32, repetition_penalty=0.0)
