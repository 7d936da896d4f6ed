"""Writes tests/golden/blip_small_processors.npz: transformers' `generate` with logits processors on the model of
blip_small.npz (tests/golden/make_blip_small.py), run on the CPU in float64 as make_blip_small_beams.py runs it.

Cases, max_new_tokens 20 (18 with the 3-token prompt: the first three tokens of the longest greedy row):
  greedy   repetition_penalty 1.3 | no_repeat_ngram_size 2 | min_new_tokens 12 | min_length 10 |
           all of them and suppress_tokens, with the prompt
  3 beams  repetition_penalty 1.3 | no_repeat_ngram_size 2 + min_new_tokens 10 |
           length_penalty 0, early_stopping=True, no_repeat_ngram_size 3
Per case `c<i>`:

  c<i>.sequences         int64 [4, P + n]   what generate returns
  c<i>.sequences_scores  float64 [4]        (beams)
  c<i>.logits            float64 [n, 4, V]  (greedy) the raw next-token logits of every step run, from uncached
                         forward passes on the returned ids: tests/logits_ref.py driven with them returns the ids
                         without transformers (tests/test_logits_ref_cpu.py)
  c<i>.margin            float64: the decisive margin. Greedy: the smallest top-1 - top-2 gap of the PROCESSED float64
                         scores over unfinished rows and free steps. Beams: the gaps of make_blip_small_beams.py, taken
                         on the processed log-probabilities (tests/logits_ref.py beam_search, which returns
                         transformers' ids, asserted here).
  c<i>.pixels64          int16 [4, 3, 80, 80], only where the case does not run on blip_small.npz's pixels: 64 x the
                         pixels of the first seed (cases[i].pixel_seed, of 36) that meets the conditions
  cases                  JSON list of {mode, num_beams, length_penalty, early_stopping, prompt, max_new_tokens,
                         processors, pixel_seed}

Conditions (asserted): every margin >= 4e-4 (four times the fp32 logits bar of
test_forward_logits_match_the_fixture, the bar of the beams fixture: what lets an fp32 run return float64's ids);
every case differs from its unconstrained run on the same pixels; the greedy penalty case holds a step of an
unfinished row whose raw argmax is a penalised or banned column; the beam penalty case penalises a column whose id
occurs twice in the history of a beam that is alive.

Run from the repository root: python tests/golden/make_blip_small_processors.py
(needs the `transformers` package; the tests only read the .npz)."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

NEW = 20
GREEDY = [
    (dict(repetition_penalty=1.3), False),
    (dict(no_repeat_ngram_size=2), False),
    (dict(min_new_tokens=12), False),
    (dict(min_length=10), False),
    (dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=12, min_length=10,
          suppress_tokens=[62, 189, 14]), True),
]
BEAMS = [
    (3, 1.0, False, dict(repetition_penalty=1.3)),
    (3, 1.0, False, dict(no_repeat_ngram_size=2, min_new_tokens=10)),
    (3, 0.0, True, dict(no_repeat_ngram_size=3)),
]
BAR = 4e-4


def _beams_maker():
    spec = importlib.util.spec_from_file_location("make_blip_small_beams", os.path.join(HERE, "make_blip_small_beams.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def hf_generate(model, px, prompt_ids, eos, new, **kw):
    extra = {} if prompt_ids is None else dict(input_ids=torch.cat((prompt_ids, torch.tensor([eos])))[None]
                                               .expand(px.shape[0], -1).contiguous())
    with torch.no_grad():
        return model.generate(pixel_values=px, max_new_tokens=new, do_sample=False, output_scores=True,
                              return_dict_in_generate=True, **extra, **kw)


def logits_fn(model, px, nb, dtype):
    with torch.no_grad():
        emb = model.vision_model(pixel_values=px).last_hidden_state.repeat_interleave(nb, dim=0)

    def fn(ids):
        with torch.no_grad():
            out = model.text_decoder(input_ids=ids, encoder_hidden_states=emb, attention_mask=torch.ones_like(ids))
        return out.logits[:, -1, :].to(dtype)
    return fn


def run_greedy(model, px, prompt_ids, prompt, proc, new, eos, pad):
    from tests import logits_ref as LR
    seq = hf_generate(model, px, prompt_ids, eos, new, num_beams=1, **proc).sequences
    plain = hf_generate(model, px, prompt_ids, eos, new, num_beams=1).sequences
    trace = []
    ids = LR.greedy(logits_fn(model, px, 1, torch.float64), px.shape[0], prompt, new, eos, pad, trace=trace, **proc)
    assert ids.shape == seq.shape and torch.equal(ids, seq), (proc, ids, seq)
    gaps, raw_hit = [], False
    P = len(prompt)
    for i, (raw, scores, live) in enumerate(trace):
        top = scores.sort(-1, descending=True)[0]
        cols = LR.touched(ids[:, :P + i], eos=eos, prompt_len=P, **proc)
        for b in range(px.shape[0]):
            if live[b]:
                gaps.append(float(top[b, 0] - top[b, 1]))
                raw_hit |= int(raw[b].argmax()) in cols[b]
    differs = seq.shape != plain.shape or not torch.equal(seq, plain)
    return dict(margin=min(gaps), seq=seq.numpy(), logits=torch.stack([t[0] for t in trace]).numpy(), differs=differs,
                special=raw_hit)


def run_beams(MB, model, px, prompt_ids, prompt, nb, lp, es, proc, new, eos, pad):
    from tests import beam_ref as BR
    from tests import logits_ref as LR
    out = hf_generate(model, px, prompt_ids, eos, new, num_beams=nb, length_penalty=lp, early_stopping=es, **proc)
    plain = hf_generate(model, px, prompt_ids, eos, new, num_beams=nb, length_penalty=lp, early_stopping=es).sequences
    seq = out.sequences
    trace = []
    (ids, scores), final = LR.beam_search(logits_fn(model, px, nb, torch.float32), px.shape[0], nb, prompt, new, eos,
                                          pad, lp, es, trace=trace, **proc)
    assert ids.shape == seq.shape and torch.equal(ids, seq), (nb, lp, es, proc, ids, seq)
    assert np.abs(scores.numpy() - out.sequences_scores.numpy()).max() < 1e-4
    B = px.shape[0]
    gaps, twice = [], False
    prev = None
    for st, cand, lps, hist in trace:
        run0 = prev["run_score"] if prev is not None else BR.new_state(B, nb, 2, [0], 0)["run_score"]
        acc = (lps + run0.reshape(-1)[:, None]).view(B, -1)
        top = acc.sort(-1, descending=True)[0][:, :2 * nb + 1].double()
        for b in range(B):
            if prev is not None and (not prev["flags"][b, 0] or (es and bool(prev["fin_flag"][b].all()))):
                continue
            gaps.append(float(top[b, 2 * nb - 1] - top[b, 2 * nb]))
            gaps.append(float(top[b, nb - 1] - top[b, nb]))
            if not st["flags"][b, 2]:
                hit = cand[2][b] == eos
                rl = (cand[0][b] + hit.float() * BR.NEG).sort(descending=True)[0].double()
                gaps.append(float(rl[nb - 1] - rl[nb]))
            for j in range(nb):
                row = hist[b * nb + j].tolist()
                twice |= run0[b, j] > -5e8 and len(set(row)) < len(row)
        prev = st
    # (merged_gaps reads a trace of (state, candidates, _) and the module's EOS)
    MB.EOS = eos
    gaps += MB.merged_gaps([(st, cand, None) for st, cand, _, _ in trace], nb, es, len(prompt) - 1, lp)
    fs = final["fin_score"].double()
    gaps += [float(fs[b, 0] - fs[b, 1]) for b in range(B)]
    gaps = [g for g in gaps if g == g]  # (-inf against -inf: neither can be chosen over a number)
    differs = seq.shape != plain.shape or not torch.equal(seq, plain)
    return dict(margin=min(gaps), seq=seq.numpy(), scores=out.sequences_scores.numpy().astype(np.float64),
                differs=differs, special=bool(twice))


def main():
    MB = _beams_maker()
    model, px0, z, cfg = MB.hf_model()
    tc = cfg["text"]
    eos, pad = tc["sep_token_id"], tc["pad_token_id"]
    greedy = z["sequences"]
    row = int((greedy[:, 1:] != pad).sum(1).argmax())
    prompt3 = torch.from_numpy(greedy[row, :3].copy())
    jobs = [("greedy", 1, 1.0, False, proc, wp, i == 0) for i, (proc, wp) in enumerate(GREEDY)]
    jobs += [("beams", nb, lp, es, proc, False, i == 0) for i, (nb, lp, es, proc) in enumerate(BEAMS)]
    res, cases = {}, []
    for mode, nb, lp, es, proc, with_prompt, need_special in jobs:
        prompt_ids = prompt3 if with_prompt else None
        prompt = MB.prompt_list(prompt_ids, tc)
        new = NEW - (len(prompt) - 1)
        found = None
        for seed in range(-1, 36):  # -1: blip_small.npz's own pixels
            px = px0 if seed < 0 else MB.seeded_pixels(seed, px0)
            if mode == "greedy":
                run = run_greedy(model, px, prompt_ids, prompt, proc, new, eos, pad)
            else:
                run = run_beams(MB, model, px, prompt_ids, prompt, nb, lp, es, proc, new, eos, pad)
            ok = run["margin"] >= BAR and run["differs"] and (run["special"] or not need_special)
            print(f"  {mode} {proc} pixel seed {seed}: margin {run['margin']:.3e}, differs {run['differs']}, "
                  f"special {run['special']}{'' if ok else ' (rejected)'}")
            if ok:
                found = dict(run, seed=seed, px=px)
                break
        assert found is not None, f"{mode} {proc}: no pixel seed of 36 meets the conditions"
        i = len(cases)
        res[f"c{i}.sequences"] = found["seq"]
        res[f"c{i}.margin"] = np.float64(found["margin"])
        if mode == "greedy":
            res[f"c{i}.logits"] = found["logits"]
        else:
            res[f"c{i}.sequences_scores"] = found["scores"]
        if found["seed"] >= 0:
            res[f"c{i}.pixels64"] = torch.round(found["px"] * 64).to(torch.int16).numpy()
        cases.append(dict(mode=mode, num_beams=nb, length_penalty=lp, early_stopping=es, prompt=prompt,
                          max_new_tokens=new, processors=proc, pixel_seed=found["seed"], special=found["special"]))
        print(f"case {i} {mode} {(nb, lp, es)} {proc} prompt {prompt} pixel seed {found['seed']}: margin "
              f"{found['margin']:.3e}")
        print(found["seq"])
    res["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "blip_small_processors.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
