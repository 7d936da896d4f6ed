"""The logits processors of transformers' `generate` restated in plain torch on the CPU (generation/
logits_process.py: RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor,
MinNewTokensLengthLogitsProcessor, SuppressTokensLogitsProcessor). csrc/logits.hip is compared with this module
bit for bit (tests/test_logits_gpu.py); tests/test_logits_ref_cpu.py holds it to transformers' own classes.

`scores` [R, V] keep their dtype (fp32 in, fp32 out; float64 gives the reference of the fixtures' margins);
`history` int [R, cur_len] is each row's sequence so far, the prompt (bos first) included. What the scores are
differs by decoding mode: greedy and sampling hand over the raw logits, beam search log_softmax(logits) of every
running beam. Order: the penalty first, on the scores as received; then the union of the bans (-inf), which
commute with each other and with the penalty."""
import torch

NEG_INF = float("-inf")


def apply_penalty(scores, history, penalty):
    """a column whose id occurs in the row's history becomes s * p (s < 0) or s / p, computed from the score as
    received: gather, then scatter, so an id that occurs several times is penalised once"""
    history = history.long()
    s = torch.gather(scores, 1, history)
    p = torch.tensor(penalty, dtype=scores.dtype)
    s = torch.where(s < 0, s * p, s / p)
    return scores.scatter(1, history, s)


def banned_ngram_tokens(row, n):
    """the ids that would complete an n-gram the row already holds: for every window of n ids whose first n - 1
    equal the row's last n - 1, the window's last id"""
    row = [int(i) for i in row]
    cur = len(row)
    if n <= 0 or n > cur:
        return []
    suffix = row[cur - (n - 1):] if n > 1 else []
    return [row[i + n - 1] for i in range(cur - n + 1) if row[i:i + n - 1] == suffix]


def no_repeat_ngram(scores, history, n):
    out = scores.clone()
    for r in range(scores.shape[0]):
        ban = banned_ngram_tokens(history[r].tolist(), int(n))
        if ban:
            out[r, torch.tensor(ban, dtype=torch.long)] = NEG_INF
    return out


def suppress_eos(cur_len, prompt_len, min_length, min_new_tokens):
    """whether eos is banned when the sequence holds cur_len ids, prompt_len of them the prompt's"""
    return cur_len < int(min_length) or cur_len - int(prompt_len) < int(min_new_tokens)


def process(scores, history, *, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0,
            suppress_tokens=None, eos=None, prompt_len=1):
    """all rules in transformers' order; history [R, cur_len]"""
    cur_len = history.shape[1]
    out = scores.clone()
    if float(repetition_penalty) != 1.0:
        out = apply_penalty(out, history, float(repetition_penalty))
    if int(no_repeat_ngram_size) > 0:
        out = no_repeat_ngram(out, history, int(no_repeat_ngram_size))
    if eos is not None and suppress_eos(cur_len, prompt_len, min_length, min_new_tokens):
        out[:, int(eos)] = NEG_INF
    if suppress_tokens is not None and len(suppress_tokens):
        out[:, torch.tensor([int(i) for i in suppress_tokens], dtype=torch.long)] = NEG_INF
    return out


def touched(history, *, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0,
            suppress_tokens=None, eos=None, prompt_len=1):
    """per row the set of columns an edit may change"""
    cur_len = history.shape[1]
    out = []
    for r in range(history.shape[0]):
        row = history[r].tolist()
        cols = set()
        if float(repetition_penalty) != 1.0:
            cols |= set(row)
        cols |= set(banned_ngram_tokens(row, int(no_repeat_ngram_size)))
        if eos is not None and suppress_eos(cur_len, prompt_len, min_length, min_new_tokens):
            cols.add(int(eos))
        cols |= {int(i) for i in (suppress_tokens or [])}
        out.append(cols)
    return out


def argmax_rule(scores):
    """the row argmax as the kernels take it: the largest number, ties to the lowest index, a NaN never wins (a
    row of nothing but NaN gives 0)"""
    s = torch.where(torch.isnan(scores), torch.full_like(scores, NEG_INF), scores)
    m = s.max(1, keepdim=True)[0]
    idx = torch.arange(scores.shape[1])[None].expand_as(s)
    first = torch.where((s == m) & ~torch.isnan(scores), idx, torch.full_like(idx, scores.shape[1])).min(1)[0]
    return torch.where(first == scores.shape[1], torch.zeros_like(first), first)


def greedy(logits_fn, B, prompt, max_new_tokens, eos, pad, trace=None, **proc):
    """transformers' greedy loop with the processors: logits_fn(ids int64 [B, cur_len]) -> logits [B, V] of the
    next token (any float dtype: the processors run in it). Returns int64 [B, P + n]. trace: receives per free step
    (raw logits, processed scores, unfinished rows before the step)."""
    P = len(prompt)
    seq = torch.tensor(prompt, dtype=torch.int64)[None].repeat(B, 1)
    finished = torch.zeros(B, dtype=torch.bool)
    for _ in range(max_new_tokens):
        raw = logits_fn(seq)
        scores = process(raw, seq, eos=eos, prompt_len=P, **proc)
        if trace is not None:
            trace.append((raw, scores, ~finished))
        tok = argmax_rule(scores)
        tok = torch.where(finished, torch.full_like(tok, pad), tok)
        seq = torch.cat((seq, tok[:, None]), 1)
        finished = finished | (tok == eos)
        if bool(finished.all()):
            break
    return seq


def beam_select_logprobs(logprobs, running, nb):
    """tests/beam_ref.py's select on scores that are log-probabilities already (processed ones): no second
    normalisation"""
    from tests import beam_ref as BR
    R, V = logprobs.shape
    acc = (logprobs + running.to(logprobs.dtype)[:, None]).view(R // nb, nb * V)
    idx = BR.topk_rule(acc, 2 * nb)
    return acc.gather(1, idx), (idx // V).int(), (idx % V).int()


def beam_logprobs(logits, history, dtype=torch.float32, **proc):
    """what transformers' beam search hands to the selection: the processors on log_softmax of the unprocessed
    row"""
    return process(torch.log_softmax(logits.to(dtype), -1), history, **proc)


def beam_search(logits_fn, B, nb, prompt, max_new_tokens, eos, pad, length_penalty=1.0, early_stopping=False,
                run_all_steps=False, trace=None, **proc):
    """tests/beam_ref.py's search with the processors between the log-softmax and the selection. trace: receives
    per step (state after it, candidates, processed log-probabilities, running sequences before it)."""
    from tests import beam_ref as BR
    P = len(prompt)
    T = P + max_new_tokens
    st = BR.new_state(B, nb, T, prompt, BR.fill_value(eos, pad))
    for t in range(P - 1, T - 1):
        hist = st["run_seq"][:, :, :t + 1].reshape(B * nb, t + 1).long()
        lp = beam_logprobs(logits_fn(hist).float(), hist, eos=eos, prompt_len=P, **proc)
        cand = beam_select_logprobs(lp, st["run_score"].reshape(-1), nb)
        BR.step(st, cand, t, P - 1, t + 1 == T - 1, eos, length_penalty, early_stopping)
        if trace is not None:
            trace.append((BR.clone_state(st), cand, lp, hist))
        if not run_all_steps and not BR.unfinished(st["flags"], early_stopping):
            break
    return BR.result(st, P), st
