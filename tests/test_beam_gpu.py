"""Beam search on the HIP path: the kernels of csrc/beam.hip against float64 (selection) and against
tests/beam_ref.py bit for bit (update, reorder); mmfd.blip's `generate(num_beams=...)` against transformers'
outputs (tests/golden/blip_small_beams.npz, whose restatement tests/test_beam_cpu.py holds to transformers);
graph behaviour, refusals and the Captioner's chunking.

Selection tolerance: err <= 3e-5 + 3e-5 |ref|max (test_caption_gpu.py's bound for the fp32 LM head), the
reference being float64 log-softmax of the same fp32 logits. Update: integers exact, scores equal; the one place
that may differ by 1 ulp is a finished hypothesis' score (torch divides by the fp32 length divisor on the CPU,
the kernel on the device). Model: ids equal, scores within margin / 4 of the fixture's."""
import json
import os

import numpy as np
import pytest
import torch

from tests import beam_ref as BR
from tests import blip_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _bound(ref):
    return 3e-5 + 3e-5 * ref.abs().max().item()


# ---------------------------------------------------------------------------------------------
# candidate selection
# ---------------------------------------------------------------------------------------------
def _select_inputs(B, nb, V, slab, seed):
    """fp32 logits [B * nb, V], N(0, 1), with planted winners far above the rest of their rows: token 0 (30) and
    the last entry of the first slab (26) in beam 0, token V - 1 (28) in the last beam, the first entry of the
    second slab (24) in beam 1 % nb. A row's best token scores about 0 + running, so the running scores order the
    planted rows: image 0 of a batch starts as [0, -1e9, ...] (only beam 0 is alive), the others hold
    -0.25 (nb - 1 - j) for beam j — the last beam's token V - 1 is the winner, 0.25 (>= 100 x the bound) ahead."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B * nb, V, generator=g)
    running = (-0.25 * (nb - 1 - torch.arange(nb, dtype=torch.float32)))[None].repeat(B, 1)
    if B > 1:
        running[0] = BR.NEG
        running[0, 0] = 0.0
    spots = [(0, 0, 30.0), (nb - 1, V - 1, 28.0)] + ([(0, slab - 1, 26.0), (1 % nb, slab, 24.0)] if slab < V else [])
    for b in range(B):
        for j, tok, val in spots:
            logits[b * nb + j, tok] = val
    return logits, running.reshape(-1), [(j, tok) for j, tok, _ in spots]


def _check_selection(got, logits, running, nb):
    """got (score, beam, token) [B, 2 nb] against float64 on the same logits: the scores in order and within the
    bound, distinct valid indices, and the float64 winners themselves in the float64 order"""
    R_, V = logits.shape
    score, beam, tok = (t.cpu() for t in got)
    ref = BR.select(logits, running, nb, dtype=torch.float64)
    acc = (torch.log_softmax(logits.double(), -1) + running.double()[:, None]).view(R_ // nb, nb * V)
    for b in range(R_ // nb):
        bound = _bound(ref[0][b])
        assert ((0 <= beam[b]) & (beam[b] < nb) & (0 <= tok[b]) & (tok[b] < V)).all()
        flat = beam[b].long() * V + tok[b].long()
        assert len(set(flat.tolist())) == 2 * nb
        assert (score[b].double() - ref[0][b]).abs().max().item() <= bound
        assert (score[b].double() - acc[b][flat]).abs().max().item() <= bound
        assert (score[b][:-1] >= score[b][1:]).all()
        assert torch.equal(beam[b], ref[1][b]) and torch.equal(tok[b], ref[2][b])
    return ref


SELECT_CASES = [(1, 2, 7), (1, 2, 4), (2, 3, 200), (4, 8, 96), (2, 3, 30524)]


@pytest.mark.parametrize("B,nb,V", SELECT_CASES)
def test_beam_select_matches_float64_and_planted_winners(B, nb, V):
    from mmfd import kernels as K
    slab = K.beam_select_slab(V)
    logits, running, spots = _select_inputs(B, nb, V, slab, seed=V + nb)
    # the logits as a strided view whose padding columns hold NaN; the outputs inside larger buffers
    wide = torch.full((B * nb, V + 5), NAN)
    wide[:, :V] = logits
    wide = wide.to(DEV)
    bufs = [torch.full((B + 2, 2 * nb), 7, device=DEV, dtype=dt) for dt in (torch.float32, torch.int32, torch.int32)]
    out = tuple(b[1:1 + B] for b in bufs)
    K.beam_select(wide[:, :V], running.to(DEV), nb, out=out)
    torch.cuda.synchronize()
    ref = _check_selection(out, logits, running, nb)
    print(f"beam_select {(B, nb, V)}: slab {slab}, score error "
          f"{(out[0].cpu().double() - ref[0]).abs().max().item():.3e}, bound {_bound(ref[0]):.3e}")
    for b in range(B):
        got = list(zip(out[1][b].tolist(), out[2][b].tolist()))
        alive = [s for s in spots if s[0] == 0] if (B > 1 and b == 0) else spots
        assert got[0] == ((0, 0) if (B > 1 and b == 0) else (nb - 1, V - 1))
        if nb <= 3:  # (with 8 beams the unplanted rows' best tokens outrank a row's second planted one)
            assert set(alive) <= set(got)
    for b in bufs:
        assert (b[0] == 7).all() and (b[-1] == 7).all()
    if V == 30524:
        assert slab < V and (V + slab - 1) // slab > 1  # more than one workgroup per row


def test_beam_select_ties_go_to_the_lower_beam_then_the_lower_token():
    from mmfd import kernels as K
    nb, V = 3, 200
    slab = K.beam_select_slab(V)
    row = torch.randn(V, generator=torch.Generator().manual_seed(3))
    row[5] = row[slab + 6] = 10.0  # equal logits in two workgroups' slabs
    row[100] = 8.0
    logits = row[None].repeat(2 * nb, 1)  # bit-identical rows, equal running scores
    running = torch.tensor([-1.5] * nb + [0.0, -1e9, -1e9])
    s, b, t = (x.cpu() for x in K.beam_select(logits.to(DEV), running.to(DEV), nb))
    assert list(zip(b[0].tolist(), t[0].tolist())) == [(j, tok) for j in range(nb) for tok in (5, slab + 6)]
    assert (s[0] == s[0, 0]).all()
    assert list(zip(b[1].tolist(), t[1].tolist()))[:3] == [(0, 5), (0, slab + 6), (0, 100)] and (b[1] == 0).all()


def test_beam_select_never_prefers_a_nan():
    from mmfd import kernels as K
    nb, V = 2, 200
    logits = torch.randn(3 * nb, V, generator=torch.Generator().manual_seed(4))
    best = int(logits[0].argmax())
    logits[0, best] = NAN     # image 0: the would-be winner of beam 0 is NaN
    logits[2] = NAN           # image 1: beam 0 is NaN throughout
    logits[4:6] = NAN         # image 2: nothing but NaN
    running = torch.zeros(3 * nb)
    s, b, t = (x.cpu() for x in K.beam_select(logits.to(DEV), running.to(DEV), nb))
    clean = logits.clone()
    clean[0, best] = -float("inf")
    ref = BR.select(clean[:2], running[:2], nb, dtype=torch.float64)
    assert torch.equal(b[0], ref[1][0]) and torch.equal(t[0], ref[2][0]) and (best not in t[0][b[0] == 0].tolist())
    assert (s[0].double() - ref[0][0]).abs().max().item() <= _bound(ref[0])
    assert (b[1] == 1).all() and torch.isfinite(s[1]).all()
    assert torch.isnan(s[2]).all() and list(zip(b[2].tolist(), t[2].tolist())) == [(0, 0), (0, 1), (0, 2), (0, 3)]


# ---------------------------------------------------------------------------------------------
# beam update and cache reorder
# ---------------------------------------------------------------------------------------------
def _to_dev(st):
    return {k: v.to(DEV) for k, v in st.items()}


def _ulps(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max().item()


@pytest.mark.parametrize("nb,lp,early", [(2, 1.0, False), (3, 0.0, True), (4, 2.0, False), (3, 1.0, True)])
def test_beam_update_matches_the_restatement_bit_for_bit(nb, lp, early):
    from mmfd import kernels as K
    B, V, steps, eos, fill = 3, 50, 8, 2, 2
    T = steps + 1
    g = torch.Generator().manual_seed(nb)
    ref = BR.new_state(B, nb, T, [49], fill)
    dev = _to_dev(ref)
    nxt = torch.zeros(B * nb, dtype=torch.int64, device=DEV)
    worst = 0
    for t in range(steps):
        # candidates as the selection leaves them: scores descending, below the best running score
        score = ref["run_score"].max(1, keepdim=True)[0] - torch.rand(B, 2 * nb, generator=g).cumsum(1)
        beam = torch.randint(0, nb, (B, 2 * nb), generator=g).int()
        tok = torch.randint(3, V, (B, 2 * nb), generator=g).int()
        if t == 1:
            tok[0, 0] = eos        # a top-nb slot
        if t == 2:
            tok[1, nb] = eos       # only a backup slot: must not finish anything
        if t == 3:
            tok[2, :] = eos        # every slot at once (transformers cannot meet this; the rule still holds)
            tok[0, nb - 1] = eos
        if t == 5:
            tok[:, 1] = eos
            score[1, 2] = NAN      # a NaN candidate is ranked last
        cand = (score, beam, tok)
        want_next = BR.step(ref, cand, t, 0, t + 1 == steps, eos, lp, early)
        K.beam_update(tuple(c.to(DEV) for c in cand), dev, t, 0, t + 1 == steps, eos, lp, early, nxt)
        torch.cuda.synchronize()
        for k in ("fin_flag", "fin_len", "run_seq", "fin_seq", "flags", "parent"):
            assert torch.equal(dev[k].cpu(), ref[k]), (t, k)
        assert torch.equal(nxt.cpu(), want_next), t
        assert torch.equal(dev["run_score"].cpu(), ref["run_score"]) or \
            torch.equal(torch.isnan(dev["run_score"].cpu()), torch.isnan(ref["run_score"])), t
        ok = ~torch.isnan(ref["run_score"])
        assert torch.equal(dev["run_score"].cpu()[ok], ref["run_score"][ok]), t
        okf = ~torch.isnan(ref["fin_score"])
        assert torch.equal(torch.isnan(dev["fin_score"].cpu()), ~okf)
        worst = max(worst, _ulps(dev["fin_score"].cpu()[okf], ref["fin_score"][okf]))
        dev["fin_score"].copy_(ref["fin_score"])  # (a 1-ulp quotient must not leak into the later steps)
    print(f"beam_update nb {nb}, length_penalty {lp}: finished scores within {worst} ulp")
    assert worst <= 1
    assert ref["fin_flag"].any() and ref["fin_len"].max() >= 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_beam_reorder_gathers_rows_and_leaves_the_tail(dtype):
    from mmfd import kernels as K
    L, rows, beam_rows, steps, width, n_pos = 2, 16, 6, 8, 64, 5
    g = torch.Generator().manual_seed(9)
    src = [torch.randn(rows, steps, width, generator=g).to(dtype) for _ in range(L)]
    for s in src:
        s[:, n_pos:] = NAN
    dst = [torch.full((rows, steps, width), 3.0).to(dtype) for _ in range(L)]
    for d in dst:
        d[:, n_pos:] = NAN
    parent = torch.tensor([0, 0, 2, 5, 3, 3], dtype=torch.int32)  # a repeated parent; rows 1 and 4 are dropped
    sd, dd = [s.to(DEV) for s in src], [d.to(DEV) for d in dst]
    K.beam_reorder(sd, dd, K.ptr_table(sd), K.ptr_table(dd), parent.to(DEV), beam_rows, n_pos)
    torch.cuda.synchronize()
    frm = parent.long().tolist() + list(range(beam_rows, rows))
    for s, s_after, d in zip(src, sd, dd):
        d = d.cpu()
        assert torch.equal(d[:, :n_pos], s[frm][:, :n_pos])
        assert torch.isnan(d[:, n_pos:]).all()
        assert torch.equal(s_after.cpu()[:, :n_pos], s[:, :n_pos]) and torch.isnan(s_after.cpu()[:, n_pos:]).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,nb,H,D,Lk", [(2, 3, 3, 32, 101), (1, 2, 2, 64, 17), (4, 8, 12, 64, 577)])
def test_attn_decode_groups_share_the_keys_of_their_image(B, nb, H, D, Lk, dtype):
    """query row b attends k / v row b // nb: against float64 on the keys repeated per beam, test_caption_gpu.py's
    bounds; the keys past Lk hold NaN and are never read"""
    import math
    from mmfd import kernels as K
    g = torch.Generator().manual_seed(B * nb + Lk)
    q = torch.randn(B * nb, H * D, generator=g).to(dtype)
    kv = torch.randn(B, Lk + 3, 2 * H * D, generator=g).to(dtype)
    k, v = kv[..., :H * D], kv[..., H * D:]
    kr, vr = (x.double()[:, :Lk].repeat_interleave(nb, 0).reshape(B * nb, Lk, H, D) for x in (k, v))
    s = torch.einsum("bhd,blhd->bhl", q.double().view(B * nb, H, D), kr) / math.sqrt(D)
    ref = torch.einsum("bhl,blhd->bhd", torch.softmax(s, -1), vr).reshape(B * nb, H * D)
    kv[:, Lk:] = NAN
    kvd = kv.to(DEV)
    o = K.attn_decode(q.to(DEV), kvd[..., :H * D], kvd[..., H * D:], H, Lk, group=nb)
    torch.cuda.synchronize()
    atol, rtol = (3e-5, 3e-5) if dtype == torch.float32 else (2e-2, 2e-2)
    err = (o.double().cpu() - ref).abs().max().item()
    print(f"attn_decode grouped {(B, nb, H, D, Lk)} {dtype}: err {err:.3e}")
    assert o.dtype == dtype and err <= atol + rtol * ref.abs().max().item()
    with pytest.raises(ValueError):
        K.attn_decode(q.to(DEV)[:B * nb - 1], kvd[..., :H * D], kvd[..., H * D:], H, Lk, group=nb)
    if nb > 2:
        with pytest.raises(ValueError):
            K.attn_decode(q.to(DEV), kvd[..., :H * D], kvd[..., H * D:], H, Lk, group=nb - 1)


def test_beam_kernels_refuse_bad_arguments():
    from mmfd import kernels as K
    lib, vp = K.lib(), K._ptr
    f = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    ws = torch.zeros(K.beam_select_workspace_bytes(1, 2, 8) + 16, dtype=torch.uint8, device=DEV)
    ok = lambda w, n, nb=2, V=8: lib.mmfd_beam_select(1, nb, V, vp(f), 8, vp(f), vp(f), vp(i), vp(i), w, n, None)  # noqa: E731
    import ctypes
    assert ok(ctypes.c_void_p(ws.data_ptr()), ws.numel()) == 0
    assert ok(ctypes.c_void_p(ws.data_ptr() + 4), ws.numel() - 4) != 0          # misaligned workspace
    assert b"aligned" in lib.mmfd_last_error_string()
    assert ok(ctypes.c_void_p(ws.data_ptr()), ws.numel() - 24) != 0             # too small
    assert ok(ctypes.c_void_p(ws.data_ptr()), ws.numel(), nb=9, V=64) != 0      # num_beams
    assert ok(ctypes.c_void_p(ws.data_ptr()), ws.numel(), nb=2, V=3) != 0       # V < 2 num_beams
    with pytest.raises(RuntimeError, match="mmfd_beam_select_workspace_bytes"):
        K.beam_select_workspace_bytes(1, 2, 3)
    st = _to_dev(BR.new_state(1, 2, 4, [1], 0))
    cand = (torch.zeros(1, 4, device=DEV), torch.zeros(1, 4, dtype=torch.int32, device=DEV),
            torch.zeros(1, 4, dtype=torch.int32, device=DEV))
    nxt = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="mmfd_beam_update.*position"):
        K.beam_update(cand, st, 3, 0, True, 2, 1.0, False, nxt)                  # would write position 4 of 4
    with pytest.raises(ValueError):
        K.beam_update(cand, st, 0, 1, False, 2, 1.0, False, nxt)                 # a forced step
    a, b = [torch.zeros(4, 4, 6, device=DEV)], [torch.zeros(4, 4, 6, device=DEV)]
    with pytest.raises(RuntimeError, match="mmfd_beam_reorder.*multiples of 16"):
        K.beam_reorder(a, b, K.ptr_table(a), K.ptr_table(b), i[:4], 4, 1)        # 24-byte positions
    with pytest.raises(ValueError):
        K.beam_reorder(a, a, K.ptr_table(a), K.ptr_table(a), i[:4], 4, 1)        # in place
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    z, cfg, W = R.load_fixture()
    zb = np.load(os.path.join(R.G, "blip_small_beams.npz"), allow_pickle=False)
    cases = json.loads(str(zb["cases"]))
    for i, c in enumerate(cases):
        c["sequences"] = torch.from_numpy(zb[f"c{i}.sequences"])
        c["scores"] = torch.from_numpy(zb[f"c{i}.sequences_scores"])
        c["margin"] = float(zb[f"c{i}.margin"])
        c["px"] = torch.from_numpy(zb[f"c{i}.pixels64"]).float() / 64.0 if c["pixel_seed"] >= 0 else \
            torch.from_numpy(z["pixel_values"])
    return dict(z=z, cfg=cfg, W=W, px=torch.from_numpy(z["pixel_values"]), seq=torch.from_numpy(z["sequences"]),
                cases=cases)


def _model(fx, precision="fp32"):
    return R.load_model(fx["cfg"], fx["W"], precision, DEV)


@pytest.fixture(scope="module")
def model32(fx):
    return _model(fx)


def _kw(c):
    sep = 2
    ids = None if len(c["prompt"]) == 1 else torch.tensor(c["prompt"] + [sep])  # (generate drops the trailing [SEP])
    return dict(input_ids=ids, num_beams=c["num_beams"], length_penalty=c["length_penalty"],
                early_stopping=c["early_stopping"], max_new_tokens=c["max_new_tokens"])


@pytest.mark.parametrize("case", range(8))
def test_beam_search_fp32_reproduces_transformers(fx, model32, case):
    c = fx["cases"][case]
    for use_graph in (False, True):
        out = model32.generate(c["px"], use_graph=use_graph, **_kw(c))
        err = (model32.sequences_scores.double().cpu() - c["scores"]).abs().max().item()
        print(f"case {case} {'graph' if use_graph else 'eager'}: score error {err:.3e}, margin {c['margin']:.3e}")
        assert out.dtype == torch.int64 and torch.equal(out, c["sequences"])
        assert err <= c["margin"] / 4


def test_greedy_is_what_it_was(fx, model32):
    model32.generate(fx["px"], num_beams=2)
    for use_graph in (False, True):
        assert torch.equal(model32.generate(fx["px"], use_graph=use_graph), fx["seq"])
        assert torch.equal(model32.generate(fx["px"], use_graph=use_graph, num_beams=1, length_penalty=2.0), fx["seq"])


def _valid_beam_structure(ids, tc, n_prompt, max_new_tokens):
    """the checks of test_caption_gpu.py's _valid_structure for a beam result: ids in range, bos first, after the
    first sep only the fill (transformers: pad_token_id or sep_token_id), and the array ends where the longest
    row does"""
    fill = tc["pad_token_id"] or tc["sep_token_id"]
    rows = ids.tolist()
    lens = []
    for r in rows:
        assert all(0 <= t < tc["vocab_size"] for t in r) and r[0] == tc["bos_token_id"]
        gen = r[n_prompt:]
        if tc["sep_token_id"] in gen:
            k = gen.index(tc["sep_token_id"])
            assert all(t == fill for t in gen[k + 1:])
            lens.append(k + 1)
        else:
            lens.append(len(gen))
    assert 1 <= len(rows[0]) - n_prompt <= max_new_tokens and len(rows[0]) == n_prompt + max(lens)


def test_beam_search_bf16_graph_equals_eager(fx):
    m = _model(fx, "bf16")
    eager = m.generate(fx["px"], use_graph=False, num_beams=3)
    s_eager = m.sequences_scores.clone()
    graph = m.generate(fx["px"], use_graph=True, num_beams=3)
    assert torch.equal(graph, eager) and torch.equal(m.sequences_scores, s_eager)
    _valid_beam_structure(eager, fx["cfg"]["text"], 1, 20)


def test_beam_graphs_replay_and_coexist(fx, model32):
    m = model32
    m.invalidate_caches()  # (the states of the tests before this one: at most 8 are kept)
    c = fx["cases"][1]
    eager = m.generate(fx["px"], use_graph=False, num_beams=3)
    assert torch.equal(eager, c["sequences"])
    assert torch.equal(m.generate(fx["px"], use_graph=True, num_beams=3), eager)
    st3 = [s for k, s in m._states.items() if len(k) > 4 and k[4] == 3 and s["graph"] is not None]
    assert len(st3) == 1
    g3 = st3[0]["graph"]
    perm = torch.tensor([2, 0, 3, 1])
    assert torch.equal(m.generate(fx["px"][perm], use_graph=True, num_beams=3), eager[perm])
    assert st3[0]["graph"] is g3  # a replay, not a new capture
    two = m.generate(fx["px"], use_graph=True, num_beams=2)
    assert torch.equal(two, fx["cases"][0]["sequences"])
    graphs = {id(s["graph"]) for s in m._states.values() if s["graph"] is not None}
    assert len(graphs) >= 2 and st3[0]["graph"] is g3  # num_beams = 2 captured its own
    greedy = m.generate(fx["px"], use_graph=True)
    assert torch.equal(greedy, fx["seq"]) and torch.equal(greedy, m.generate(fx["px"], use_graph=False))
    assert torch.equal(m.generate(fx["px"], use_graph=True, num_beams=3), eager)


def test_generate_refuses_bad_beam_arguments(fx, model32, monkeypatch):
    from mmfd import kernels as K
    launched = []
    for name in ("gemm", "lm_head_argmax", "beam_select", "patchify"):
        monkeypatch.setattr(K, name, lambda *a, _n=name, **k: launched.append(_n))
    px = fx["px"]
    for kw in (dict(num_beams=0), dict(num_beams=9), dict(num_beams=3, early_stopping="never")):
        with pytest.raises(ValueError):
            model32.generate(px, **kw)
    with pytest.raises(ValueError, match="batch \\* num_beams"):
        model32.generate(px[:1].expand(11, -1, -1, -1), num_beams=3)  # 33 rows
    assert not launched


def test_captioner_chunks_a_batch_of_nine(fx, model32):
    from mmfd.caption import Captioner
    g = torch.Generator().manual_seed(5)
    extra = torch.round(torch.randn(5, *fx["px"].shape[1:], generator=g) * 64.0).clamp(-255, 255) / 64.0
    px = torch.cat((fx["px"], extra), 0)
    cap = Captioner(model32, max_new_tokens=12, use_graph=False, num_beams=4)
    ids = cap.generate_ids(px)
    singles = [cap.generate_ids(px[i]) for i in range(9)]
    tc = fx["cfg"]["text"]
    assert ids.shape == (9, max(s.shape[1] for s in singles))
    for i, s in enumerate(singles):
        # what a row generated is what the image generates alone; behind it the chunk's fill (transformers' beam
        # search fills with sep where pad is 0) and the pad that brings the chunks to one width
        n = s.shape[1]
        assert s.shape[0] == 1 and torch.equal(ids[i, :n], s[0])
        assert set(ids[i, n:].tolist()) <= {tc["pad_token_id"], tc["sep_token_id"]}
    first = model32.generate(px[:8], use_graph=False, num_beams=4, max_new_tokens=12)
    assert torch.equal(ids[:8, :first.shape[1]], first) and (ids[:8, first.shape[1]:] == tc["pad_token_id"]).all()
