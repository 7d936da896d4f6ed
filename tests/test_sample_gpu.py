"""Sampling on the HIP path: mmfd_sample_select (csrc/sample.hip) against tests/sample_ref.py — the float64
restatement of transformers' temperature / top-k / top-p warpers and the draw, held to transformers by
tests/test_sample_ref_cpu.py — and mmfd.blip's `generate(do_sample=True, ...)` / mmfd.caption.Captioner on
tests/golden/blip_small.npz.

Tolerance: sample_ref.TOL = 64 * 2^-24, derived there for the kernel's arithmetic. Kept sets must be equal on the
recorded (usable) rows, probabilities lie within TOL, and every drawn token j must satisfy
C_{j-1} - TOL <= u < C_j + TOL against the float64 prefix table. In the model tests the interval is widened by
2 * 1e-4: 1e-4 is the bar test_caption_gpu.py holds the fp32 logits to, and a logit shift d moves a prefix by at
most 2 d."""
import functools

import numpy as np
import pytest
import torch

from tests import blip_refs as R
from tests import sample_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = float("nan"), float("inf")
POISON = -7.0


@functools.lru_cache(maxsize=None)
def _case(V, si):
    """(logits [32, V], [Filtered per row]) of a case, computed once and never modified"""
    T, k, p = S.SETTINGS[si]
    x = S.case_logits(V, si, S.MAX_ROWS)
    x.setflags(write=False)
    return x, [S.filter_ref(S.quotients(row, T), k, p) for row in x]


def _run(x, T, k, p, seed, row0, step, ldl=None, want_probs=True, want_kept=True):
    """one launch on logits x [R, V] staged in a [R, ldl] buffer whose other columns hold 1e30 (a kernel that
    read them would keep nothing else); probs in a [R, V + 5] buffer poisoned beforehand"""
    from mmfd import kernels as K
    Rn, V = x.shape
    ldl = ldl or V
    buf = torch.full((Rn, ldl), 1e30)
    buf[:, :V] = torch.from_numpy(np.array(x, np.float32))
    buf = buf.to(DEV)
    ctl = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed, row0], dtype=torch.int64, device=DEV)
    pbuf = torch.full((Rn, V + 5), POISON, device=DEV) if want_probs else None
    kept = torch.full((Rn,), -1, dtype=torch.int32, device=DEV) if want_kept else None
    tok = K.sample_select(buf[:, :V], T, k, p, ctl, step, probs=None if pbuf is None else pbuf[:, :V], kept=kept)
    torch.cuda.synchronize()
    return (tok.cpu().numpy(), None if pbuf is None else pbuf.cpu().numpy(), None if kept is None else kept.cpu().numpy())


def _check_rows(tok, probs, kept, refs, T, k, p, seed, row0, step, what):
    V = refs[0].kept.shape[0]
    assert (probs[:, V:] == POISON).all(), what
    for r, f in enumerate(refs):
        pr = probs[r, :V]
        if f.n_kept == 0:  # a row without a number
            assert tok[r] == 0 and kept[r] == 0 and (pr == 0).all(), (what, r)
            continue
        got = pr > 0
        assert not (got & ~f.kept).any(), (what, r)
        missing = f.kept & ~got  # a kept entry may carry a mass below 2^-41, which the kernel rounds to 0
        assert (f.probs[missing] < 2.0 ** -40).all(), (what, r)
        assert kept[r] == f.n_kept, (what, r, int(kept[r]), f.n_kept)
        assert np.abs(pr - f.probs).max() <= S.TOL, (what, r, float(np.abs(pr - f.probs).max()))
        u = S.uniform_ref(seed, step, row0 + r)
        assert 0 <= tok[r] < V and f.kept[tok[r]] and S.accepted(f, tok[r], u), (what, r, int(tok[r]), u)


@pytest.mark.parametrize("si", range(len(S.SETTINGS)), ids=[f"T{t}-k{k}-p{p}" for t, k, p in S.SETTINGS])
@pytest.mark.parametrize("V", S.TEST_VOCABS)
def test_kernel_matches_the_restatement(V, si):
    from mmfd import kernels as K
    assert K.sample_select_resident_max() == S.RESIDENT_MAX  # V = 32768 / 32769 lie on the two sides of the switch
    T, k, p = S.SETTINGS[si]
    x, refs = _case(V, si)
    for Rn in (1, 5, 32):
        for ldl in (V, V + 3):
            seed, row0, step = 1234 + Rn, 3 * Rn, Rn + (ldl - V)
            tok, probs, kept = _run(x[:Rn], T, k, p, seed, row0, step, ldl=ldl)
            _check_rows(tok, probs, kept, refs[:Rn], T, k, p, seed, row0, step, (V, si, Rn, ldl))


def _planted(rows, T=1.0, k=0, p=1.0, seed=5, step=2):
    x = np.array(rows, np.float32)
    tok, probs, kept = _run(x, T, k, p, seed, 0, step)
    refs = [S.filter_ref(S.quotients(r, T), k, p) for r in x]
    assert all(S.usable(f) for f in refs)
    _check_rows(tok, probs, kept, refs, T, k, p, seed, 0, step, "planted")
    return tok, probs[:, :x.shape[1]], kept, refs


def test_planted_ties_at_the_kth_value_survive():
    V = 300
    x = np.linspace(-3, 0, V).astype(np.float32)
    x[[7, 150, 299]] = 1.0  # three entries share the 2nd largest value
    x[40] = 2.0
    tok, probs, kept, _ = _planted([x, x[::-1].copy()], k=2)
    assert kept.tolist() == [4, 4]
    assert sorted(np.nonzero(probs[0])[0].tolist()) == [7, 40, 150, 299]


def test_planted_equal_run_across_the_nucleus_boundary_keeps_lower_indices():
    # ten equal logits far above the rest: masses 1/10 each; p = 0.55 keeps the six lowest indices of the run
    V = 2000
    x = np.full(V, -40.0, np.float32)
    run = [3, 64, 65, 700, 701, 1023, 1024, 1500, 1998, 1999]
    x[run] = 2.5
    tok, probs, kept, _ = _planted([x], p=0.55)
    assert kept.tolist() == [6] and np.nonzero(probs[0])[0].tolist() == run[:6]
    assert np.abs(probs[0][run[:6]] - 1 / 6).max() <= S.TOL


def test_planted_top_k_1_and_top_p_0_keep_one_token():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 999)).astype(np.float32)
    x[1, [5, 900]] = 9.0  # a duplicated maximum: top_p = 0 keeps the lower index
    tok, probs, kept, _ = _planted(x, p=0.0)
    assert kept.tolist() == [1] * 4 and tok.tolist() == [int(r.argmax()) for r in x] and tok[1] == 5
    y = x.copy()
    y[1, 900] = 8.0  # top_k = 1 on rows with one maximum: the argmax
    tok, probs, kept, _ = _planted(y, k=1)
    assert kept.tolist() == [1] * 4 and tok.tolist() == [int(r.argmax()) for r in y]
    # (a duplicated maximum survives top_k = 1 twice, as `scores < topk(scores)[..., -1]` leaves it: the draw decides)
    tok, probs, kept, _ = _planted(x[1:2], k=1)
    assert kept.tolist() == [2] and tok[0] in (5, 900)


def test_planted_nan_and_infinities():
    V = 777
    rng = np.random.default_rng(4)
    x = rng.standard_normal((5, V)).astype(np.float32)
    x[0, [0, 50, 100, V - 1]] = NAN
    x[1] = -INF
    x[1, 321] = -3.0              # -inf everywhere but one number
    x[2] = NAN                    # no number at all
    x[3] = -INF                   # no number at all
    x[3, 5] = NAN
    x[4, 9] = np.array([0xFFFFFFFF], np.uint32).view(np.float32)[0]  # the largest bit pattern there is: a NaN
    x[4, 10] = np.array([0x7FFFFFFF], np.uint32).view(np.float32)[0]
    for T, k, p in ((1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 3, 1.0), (1.0, 0, 0.3)):
        tok, probs, kept, refs = _planted(x, T=T, k=k, p=p)
        assert np.isfinite(probs).all()
        assert (probs[0][[0, 50, 100, V - 1]] == 0).all() and tok[0] not in (0, 50, 100, V - 1)
        assert tok[1] == 321 and kept[1] == 1 and probs[1][321] == 1.0
        assert tok[2] == 0 and kept[2] == 0 and (probs[2] == 0).all()
        assert tok[3] == 0 and kept[3] == 0 and (probs[3] == 0).all()
        assert (probs[4][[9, 10]] == 0).all() and tok[4] not in (9, 10)


def test_draw_follows_seed_step_and_row_offset():
    # 4096 equal logits: the prefix table is (j + 1) / 4096 exactly, in the kernel's integers too, so the token IS
    # floor(u * 4096)
    V, Rn = 4096, 5
    x = np.zeros((Rn, V), np.float32)
    seen = set()
    for seed, row0, step in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2 ** 40 + 5, 2 ** 33, 19), (2 ** 64 - 1, 7, 127)):
        tok, _, _ = _run(x, 1.0, 0, 1.0, seed, row0, step)
        want = [int(S.uniform_ref(seed, step, row0 + r) * V) for r in range(Rn)]
        assert tok.tolist() == want, (seed, row0, step)
        seen.add(tuple(want))
    assert len(seen) == 6


def test_rows_are_independent_runs_repeat_and_outputs_are_optional():
    V, Rn, si = 1001, 5, 2
    T, k, p = S.SETTINGS[si]
    x, _ = _case(V, si)
    x = x[:Rn]
    tok, probs, kept = _run(x, T, k, p, 99, 10, 4)
    tok2, probs2, kept2 = _run(x, T, k, p, 99, 10, 4)
    assert np.array_equal(tok, tok2) and np.array_equal(kept, kept2)
    assert np.array_equal(probs.view(np.uint32), probs2.view(np.uint32))  # the same bits
    for r in range(Rn):
        t1, p1, k1 = _run(x[r:r + 1], T, k, p, 99, 10 + r, 4)
        assert t1[0] == tok[r] and k1[0] == kept[r] and np.array_equal(p1[0].view(np.uint32), probs[r].view(np.uint32))
    t3, p3, k3 = _run(x, T, k, p, 99, 10, 4, want_probs=False, want_kept=False)
    assert p3 is None and k3 is None and np.array_equal(t3, tok)


def test_python_wrapper_refuses_bad_tensors():
    from mmfd import kernels as K
    x = torch.zeros(2, 8, device=DEV)
    ctl = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="logits"):
        K.sample_select(x.double(), 1.0, 0, 1.0, ctl, 0)
    with pytest.raises(ValueError, match="ctl"):
        K.sample_select(x, 1.0, 0, 1.0, ctl.int(), 0)
    with pytest.raises(ValueError, match="temperature"):
        K.sample_select(x, 0.0, 0, 1.0, ctl, 0)
    with pytest.raises(ValueError, match="probs"):
        K.sample_select(x, 1.0, 0, 1.0, ctl, 0, probs=torch.zeros(2, 7, device=DEV))
    with pytest.raises(ValueError, match="step"):
        K.sample_select(x, 1.0, 0, 1.0, ctl, -1)
    with pytest.raises(RuntimeError, match="GPU"):
        K.sample_select(x.cpu(), 1.0, 0, 1.0, ctl, 0)


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    z, cfg, W = R.load_fixture()
    return dict(z=z, cfg=cfg, W=W, seq=torch.from_numpy(z["sequences"]), px=torch.from_numpy(z["pixel_values"]))


def _model(fx, precision="fp32"):
    return R.load_model(fx["cfg"], fx["W"], precision, DEV)


@pytest.fixture(scope="module")
def model(fx):
    return _model(fx)


MODEL_SETTINGS = [(1.0, 0, 1.0), (0.8, 20, 0.9)]
WIDEN = 2 * 1e-4


def _check_samples(m, px_rows, ids, tc, T, k, p, seed, row_offset=0):
    """every live (row, step) token of ids [rows, 1 + len] is accepted against forward_logits on the same pixel rows;
    a row that drew sep is padded afterwards"""
    ids = ids.cpu()
    assert ids.dtype == torch.int64 and (ids[:, 0] == tc["bos_token_id"]).all()
    logits = m.forward_logits(px_rows, ids[:, :-1]).cpu().numpy()  # [len, rows, V]
    live = R.live_mask(ids.numpy(), tc["sep_token_id"])
    n = 0
    for t in range(ids.shape[1] - 1):
        for b in range(ids.shape[0]):
            tok = int(ids[b, t + 1])
            if not live[t, b]:
                assert tok == tc["pad_token_id"]
                continue
            f = S.filter_ref(S.quotients(logits[t, b], T), k, p)
            u = S.uniform_ref(seed, t, row_offset + b)
            assert S.accepted(f, tok, u, widen=WIDEN), (t, b, tok, u)
            n += 1
    assert live[-1].any()  # the array ends where the last row stopped
    return n


def test_top_k_1_is_greedy(fx, model):
    for use_graph in (False, True):
        out = model.generate(fx["px"], do_sample=True, top_k=1, seed=3, use_graph=use_graph)
        assert torch.equal(out, fx["seq"])


@pytest.mark.parametrize("T,k,p", MODEL_SETTINGS)
def test_sampled_tokens_are_the_draws_of_their_logits(fx, model, T, k, p):
    tc = fx["cfg"]["text"]
    for seed in (11, 2 ** 40 + 5):
        out = model.generate(fx["px"], do_sample=True, temperature=T, top_k=k, top_p=p, seed=seed, use_graph=False)
        assert model.sample_seed == seed and out.shape[0] == 4 and 2 <= out.shape[1] <= 21
        assert _check_samples(model, fx["px"], out, tc, T, k, p, seed) >= 4


def test_graph_equals_eager_and_replays_with_a_new_seed(fx, model):
    T, k, p = MODEL_SETTINGS[1]
    kw = dict(do_sample=True, temperature=T, top_k=k, top_p=p)
    eager = [model.generate(fx["px"], seed=s, use_graph=False, **kw) for s in (21, 22)]
    assert not torch.equal(eager[0], eager[1])
    g0 = model.generate(fx["px"], seed=21, use_graph=True, **kw)
    captured = lambda: [st["graph"] for key, st in model._states.items()  # noqa: E731
                        if key[0] == "sample" and key[-3:] == (T, k, p) and st["graph"] is not None]
    graphs = captured()
    assert len(graphs) == 1 and torch.equal(g0, eager[0])
    g1 = model.generate(fx["px"], seed=22, use_graph=True, **kw)
    assert torch.equal(g1, eager[1])
    assert captured() == graphs and captured()[0] is graphs[0]  # a new seed replays: nothing was captured again
    # seed=None takes the seed from torch's global CPU generator
    torch.manual_seed(5)
    a = model.generate(fx["px"], use_graph=True, **kw)
    sa = model.sample_seed
    torch.manual_seed(5)
    b = model.generate(fx["px"], use_graph=True, **kw)
    assert model.sample_seed == sa and torch.equal(a, b)


def test_three_samples_per_image(fx, model):
    tc = fx["cfg"]["text"]
    T, k, p = MODEL_SETTINGS[0]
    px3 = fx["px"].repeat_interleave(3, 0)
    for use_graph in (False, True):
        out = model.generate(fx["px"], do_sample=True, temperature=T, top_k=k, top_p=p, num_return_sequences=3, seed=77,
                             use_graph=use_graph)
        assert out.shape[0] == 12
        _check_samples(model, px3, out, tc, T, k, p, 77)
        assert any(not (torch.equal(out[3 * b], out[3 * b + 1]) and torch.equal(out[3 * b], out[3 * b + 2]))
                   for b in range(4))
    off = model.generate(fx["px"], do_sample=True, num_return_sequences=3, seed=77, row_offset=5, use_graph=False)
    _check_samples(model, px3, off, tc, T, k, p, 77, row_offset=5)


def test_bf16_sampling(fx):
    m = _model(fx, "bf16")
    V = fx["cfg"]["text"]["vocab_size"]
    greedy = m.generate(fx["px"], use_graph=False)
    assert torch.equal(m.generate(fx["px"], do_sample=True, top_k=1, seed=1, use_graph=False), greedy)
    kw = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=9, num_return_sequences=2)
    eager, graph = m.generate(fx["px"], use_graph=False, **kw), m.generate(fx["px"], use_graph=True, **kw)
    assert torch.equal(eager, graph) and eager.shape[0] == 8
    assert ((0 <= eager) & (eager < V)).all()


def test_captioner_chunks_equal_generate_with_row_offsets(fx, model):
    from mmfd.caption import Captioner
    from tests.toy_tokenizer import toy_tokenizer
    px = fx["px"].repeat(3, 1, 1, 1)  # 12 images, 36 rows: chunks of 10 and 2 images
    kw = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, num_return_sequences=3)
    cap = Captioner(model, tokenizer=toy_tokenizer(), seed=31, **kw)
    ids = cap.generate_ids(px)
    parts = [model.generate(px[:10], seed=31, row_offset=0, **kw), model.generate(px[10:], seed=31, row_offset=30, **kw)]
    width = max(q.shape[1] for q in parts)
    pad = fx["cfg"]["text"]["pad_token_id"]
    want = torch.cat([torch.nn.functional.pad(q, (0, width - q.shape[1]), value=pad) for q in parts], 0)
    assert cap.sample_seed == 31 and tuple(ids.shape) == (36, width) and torch.equal(ids, want)
    texts = cap.caption(px)
    assert len(texts) == 36 and all(isinstance(t, str) for t in texts)


def test_greedy_and_beams_are_untouched_by_a_sampling_call(fx, model):
    greedy = [model.generate(fx["px"], use_graph=g) for g in (False, True)]
    beams = model.generate(fx["px"], num_beams=3, use_graph=True)
    model.generate(fx["px"], do_sample=True, top_k=10, seed=4, num_return_sequences=2, use_graph=True)
    assert all(torch.equal(model.generate(fx["px"], use_graph=g), greedy[i]) for i, g in enumerate((False, True)))
    assert torch.equal(model.generate(fx["px"], num_beams=3, use_graph=True), beams)
    assert torch.equal(greedy[0], fx["seq"])


def test_generate_refusals(fx, model):
    px = fx["px"]
    bad = [dict(do_sample=True, num_beams=2), dict(num_return_sequences=2), dict(do_sample=True, num_return_sequences=9),
           dict(do_sample=True, temperature=0.0), dict(do_sample=True, temperature=NAN), dict(do_sample=True, top_k=-1),
           dict(do_sample=True, top_p=1.5), dict(do_sample=True, top_p=-0.5), dict(do_sample=True, num_return_sequences=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            model.generate(px, **kw)
    from mmfd.caption import Captioner
    with pytest.raises(ValueError):
        Captioner(model, num_return_sequences=2)
    with pytest.raises(ValueError):
        Captioner(model, do_sample=True, num_beams=2)
