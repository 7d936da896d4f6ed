"""Beam search restated in plain torch on the CPU: one step of transformers' GenerationMixin._beam_search
(generation/utils.py, steps b - g) on the state layout of csrc/beam.hip, and the final crop. The kernels
are compared with this module bit for bit (tests/test_beam_gpu.py); tests/test_beam_cpu.py holds it to
transformers' own `generate(num_beams=...)`.

The one thing transformers leaves open is the order torch.topk gives equal scores. Here, as in the
kernels: the larger score first, equal scores by the lower index, a NaN after every number.

State (a dict of tensors; B images, nb beams, T = prompt + max_new_tokens positions):
  run_score, fin_score  fp32 [B, nb]     fin_flag, fin_len  int32 [B, nb] (is_sent_finished; generated length)
  run_seq, fin_seq      int32 [B, nb, T]  parent int32 [B * nb]
  flags                 int32 [B, 4]: heuristic still unsatisfied, every hypothesis finished, every candidate
                        stopped, unused
transformers keeps the beam-index trail of every hypothesis only to count its entries at the end; fin_len is
that count."""
import numpy as np
import torch
import torch.nn.functional as F

NEG = -1.0e9


def topk_rule(v, k):
    """indices [.., k] of the k best entries of v [.., n] under the rule above"""
    a = v.detach().cpu().numpy()
    flat = a.reshape(-1, a.shape[-1])
    out = np.empty((flat.shape[0], k), np.int64)
    idx = np.arange(flat.shape[1])
    for r, row in enumerate(flat):
        nan = np.isnan(row)
        key = np.where(nan, -np.inf, row)
        out[r] = np.lexsort((idx, -key, nan))[:k]  # last key first: numbers, then larger, then lower index
    return torch.from_numpy(out.reshape(a.shape[:-1] + (k,)))


def fill_value(eos, pad):
    """what transformers fills the unused positions with: `pad_token_id or eos_token_id[0]` — BLIP's pad id is 0, so
    its beam results are filled with eos (the greedy path fills with pad)"""
    return int(pad) or int(eos)


def new_state(B, nb, T, prompt, fill):
    run_seq = torch.full((B, nb, T), int(fill), dtype=torch.int32)
    run_seq[:, :, :len(prompt)] = torch.tensor(prompt, dtype=torch.int32)
    run_score = torch.zeros(B, nb)
    run_score[:, 1:] = NEG
    flags = torch.zeros(B, 4, dtype=torch.int32)
    flags[:, 0] = 1
    return dict(run_score=run_score, fin_score=torch.full((B, nb), NEG), fin_flag=torch.zeros(B, nb, dtype=torch.int32),
                fin_len=torch.zeros(B, nb, dtype=torch.int32), run_seq=run_seq, fin_seq=run_seq.clone(), flags=flags,
                parent=torch.arange(B * nb, dtype=torch.int32))


def clone_state(st):
    return {k: v.clone() for k, v in st.items()}


def select(logits, running, nb, dtype=torch.float32):
    """(score [B, 2 nb], beam, token): the 2 nb best of log_softmax(logits [B * nb, V]) + running [B * nb] per
    image; dtype float64 gives the reference the selection kernel is measured against"""
    R, V = logits.shape
    acc = F.log_softmax(logits.to(dtype), dim=-1) + running.to(dtype)[:, None]
    acc = acc.view(R // nb, nb * V)
    idx = topk_rule(acc, 2 * nb)
    return acc.gather(1, idx), (idx // V).int(), (idx % V).int()


def step(st, cand, t, n_forced, last, eos, length_penalty, early_stopping):
    """one beam step in place: the step that embedded position t chooses position t + 1. Returns the token of
    every new beam, int64 [B * nb] (st['parent'] holds the rows they continue)."""
    score, beam, tok = cand[0].float(), cand[1].long(), cand[2].long()
    B, nb, T = st["run_seq"].shape
    early = early_stopping is True or early_stopping == 1
    gen_len = t + 1 - n_forced  # transformers' cur_len + 1 - decoder_prompt_len
    div = float(gen_len) ** float(length_penalty)
    hit = (tok == eos) | bool(last)
    seqs = st["run_seq"].gather(1, beam[:, :, None].expand(B, 2 * nb, T)).clone()
    seqs[:, :, t + 1] = tok.int()
    # e. the running beams of the next step
    rl = score + hit.to(torch.float32) * NEG
    nxt = topk_rule(rl, nb)
    unsat = st["flags"][:, :1].bool()
    was_finished = st["fin_flag"].bool()
    # f. the finished hypotheses
    did = hit & (torch.arange(2 * nb) < nb)[None, :]
    s = score / div
    s = s + (was_finished.all(-1, keepdim=True) & early).to(torch.float32) * NEG
    s = s + (~unsat).to(torch.float32) * NEG
    s = s + (~did) * NEG
    m_score = torch.cat((st["fin_score"], s), 1)
    m_seq = torch.cat((st["fin_seq"], seqs), 1)
    m_flag = torch.cat((was_finished, did), 1)
    m_len = torch.cat((st["fin_len"], torch.full((B, 2 * nb), gen_len, dtype=torch.int32)), 1)
    top = topk_rule(m_score, nb)
    st["run_seq"] = seqs.gather(1, nxt[:, :, None].expand(B, nb, T))
    st["run_score"] = rl.gather(1, nxt)
    st["parent"] = (beam.gather(1, nxt) + torch.arange(B)[:, None] * nb).reshape(-1).int()
    st["fin_seq"] = m_seq.gather(1, top[:, :, None].expand(B, nb, T))
    st["fin_score"] = m_score.gather(1, top)
    st["fin_flag"] = m_flag.gather(1, top).int()
    st["fin_len"] = m_len.gather(1, top)
    # g. the early-stop heuristic (early_stopping False or True: the hypothetical length is the current one)
    best = st["run_score"][:, :1] / div
    worst = torch.where(st["fin_flag"].bool(), st["fin_score"].min(1, keepdim=True)[0], NEG)
    flags = st["flags"].clone()
    flags[:, 0] = (unsat & (best > worst).any(-1, keepdim=True)).int()[:, 0]
    flags[:, 1] = st["fin_flag"].bool().all(-1).int()
    flags[:, 2] = hit.all(-1).int()
    st["flags"] = flags
    return tok.gather(1, nxt).reshape(-1)


def unfinished(flags, early_stopping):
    """_beam_search_has_unfinished_sequences over the whole batch, from the per-image flags"""
    f = flags.bool()
    early = early_stopping is True or early_stopping == 1
    return bool(f[:, 0].any()) and not (bool(f[:, 1].all()) and early) and not bool(f[:, 2].all())


def result(st, n_prompt):
    """the array generate returns: the best hypothesis of every image, cropped to the prompt plus the longest
    generated length (the fill is in the state already); and its scores"""
    n = int(st["fin_len"][:, 0].max())
    return st["fin_seq"][:, 0, :n_prompt + n].long().contiguous(), st["fin_score"][:, 0].clone()


def search(logits_fn, B, nb, prompt, max_new_tokens, eos, pad, length_penalty=1.0, early_stopping=False,
           run_all_steps=False, trace=None):
    """the whole loop: logits_fn(run_seq int64 [B * nb, cur_len]) -> fp32 logits [B * nb, V] of the next token.
    run_all_steps: never leave early (what a captured graph does)."""
    P = len(prompt)
    T = P + max_new_tokens
    st = new_state(B, nb, T, prompt, fill_value(eos, pad))
    for t in range(P - 1, T - 1):
        logits = logits_fn(st["run_seq"][:, :, :t + 1].reshape(B * nb, t + 1).long())
        cand = select(logits.float(), st["run_score"].reshape(-1), nb)
        step(st, cand, t, P - 1, t + 1 == T - 1, eos, length_penalty, early_stopping)
        if trace is not None:
            trace.append((clone_state(st), cand, logits))
        if not run_all_steps and not unfinished(st["flags"], early_stopping):
            break
    return result(st, P), st
