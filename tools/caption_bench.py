"""Times greedy BLIP captioning (mmfd.blip) at the default configuration (blip-image-captioning-large
shapes, random weights and pixels) and the LM-head kernel alone.

  python tools/caption_bench.py [--batches 1 20] [--num-beams 1] [--reps 3] [--out FILE]
  python tools/caption_bench.py --loss [--batches 20] [--seq 21] [--reps 7] [--out FILE]
  python tools/caption_bench.py --sample [--top-k 50] [--top-p 0.9] [--temperature 1.0] [--num-return-sequences 1]
  python tools/caption_bench.py --processors [--reps 7] [--out FILE]
  python tools/caption_bench.py --lm-head-wide [--out FILE]
  python tools/caption_bench.py --csv 512 [--batch-rows 64] [--csv-side 400] [--out FILE]

Per (batch, precision): wall time of `generate` (20 new tokens; host-synchronised, the ids copied back)
eager and as one graph replay, and per precision the device time of kernels.lm_head_argmax at
V = 30524, K = 768 with the bytes it has to read (W + bias + x) per second. Prints one JSON line.
Random weights seldom produce the stop token, so eager mode runs all 20 steps like the graph.
--num-beams N > 1 times beam search instead (batch * N decoder rows) and, per precision and batch, the device time
of one step's three beam kernel groups (selection, update, cache reorder at position 10) on the model's shapes.
--loss times the caption loss instead (forward(labels=), train_text_decoder, label smoothing 0.1): per precision
and batch the wall time of the forward under no_grad and of forward + backward (host-synchronised, median of
--reps runs after one warm-up), the vision tower's share (image_embeds alone), and the device time of the two
vocabulary cross-entropy kernels on the model's [B * T, 30524] logits with the bytes they have to move.
--sample times `generate(do_sample=True, ...)` instead (batch * num_return_sequences decoder rows), eager and graph,
with greedy decoding of as many rows in the same run as its yardstick, and `sample_step_times`: the device time of
kernels.sample_select alone on [rows, 30524] logits for the call's filters and for each filter alone, beside
kernels.beam_select at the same row count.
--processors times the logits processors (repetition_penalty 1.3, no_repeat_ngram_size 2, min_new_tokens 12 and three
suppressed ids together): per precision, for greedy decoding, 3 beams and 3 samples per image, at batch 1 and at the
largest batch the mode takes (32 decoder rows), the graph-replay wall time of `generate` with them off and on in
the same run; and `processor_step_times`: the device time of kernels.logits_process, kernels.row_argmax and the
beam path's kernels.row_log_softmax alone at V = 30524 on 1 and 32 rows of a 21-token history.
--batches takes greedy batches up to 128 (above 32 rows `generate` and the LM-head probe run on
kernels.lm_head_argmax_wide). --lm-head-wide times the LM head alone: the narrow kernel at 32 rows, the wide one at
32, 64, 128 and 256, warm and cold. --csv N writes N synthetic JPEGs and a CSV of N / 2 rows to a temporary directory
and times mmfd.caption.process_csv end to end (images/s, JPEG decode included) beside the same files decoded in this
process and captioned in 32-row chunks, the decode pool alone and the GPU alone."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmfd import kernels as K  # noqa: E402
from mmfd.blip import BlipForConditionalGeneration  # noqa: E402


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, sorted(ts)[len(ts) // 2] * 1e3


def lm_head_rate(dtype, B, V=30524, Kd=768, reps=20, wide=None):
    """wide: time kernels.lm_head_argmax_wide (default: whenever B > 32, the rows the narrow kernel refuses)"""
    wide = B > 32 if wide is None else wide
    head = K.lm_head_argmax_wide if wide else K.lm_head_argmax
    x = torch.randn(B, Kd, device="cuda").to(dtype)
    W = (torch.randn(V, Kd, device="cuda") * 0.02).to(dtype)
    bias = torch.zeros(V, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")  # larger than the 256 MiB last-level cache
    out = torch.empty(B, dtype=torch.int64, device="cuda")
    head(x, W, bias, out=out)
    cold, warm = [], []
    for i in range(reps):
        if i % 2 == 0:
            flush.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        head(x, W, bias, out=out)
        e1.record()
        torch.cuda.synchronize()
        (cold if i % 2 == 0 else warm).append(e0.elapsed_time(e1) * 1e-3)
    nbytes = W.numel() * W.element_size() + bias.numel() * 4 + x.numel() * x.element_size()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return {"B": B, "kernel": "wide" if wide else "narrow", "row_tiles": (B + 31) // 32 if wide else 1,
            "bytes": nbytes, "us_cold": round(med(cold) * 1e6, 1), "us_warm": round(med(warm) * 1e6, 1),
            "TBps_cold": round(nbytes / med(cold) / 1e12, 3), "TBps_warm": round(nbytes / med(warm) / 1e12, 3),
            "note": "both launches (partials + final reduce) between the events; cold = after a 512 MiB fill"}


def beam_step_times(dt, B, nb, V=30524, E=768, L=12, steps=20, t=10, reps=20):
    """device time (us, median of reps, each between two events) of the three kernel groups of one beam step on
    random state: the selection over [B * nb, V] logits, the update, and the reorder of L caches up to position t"""
    R, T, dev = B * nb, steps + 1, "cuda"
    i32 = dict(dtype=torch.int32, device=dev)
    logits = torch.randn(R, V, device=dev)
    st = dict(run_score=-torch.rand(B, nb, device=dev), fin_score=torch.full((B, nb), -1e9, device=dev),
              fin_flag=torch.zeros(B, nb, **i32), fin_len=torch.zeros(B, nb, **i32), run_seq=torch.zeros(B, nb, T, **i32),
              fin_seq=torch.zeros(B, nb, T, **i32), flags=torch.ones(B, 4, **i32), parent=torch.zeros(R, **i32))
    cand = K.beam_select(logits, st["run_score"].view(-1), nb)
    ws = torch.empty(K.beam_select_workspace_bytes(B, nb, V), dtype=torch.uint8, device=dev)
    nxt = torch.zeros(R, dtype=torch.int64, device=dev)
    Bp = max(R, 16)
    kv = [[torch.zeros(Bp, steps, 2 * E, device=dev, dtype=dt) for _ in range(L)] for _ in range(2)]
    tab = [K.ptr_table(kv[0]), K.ptr_table(kv[1])]
    groups = {
        "select_us": lambda: K.beam_select(logits, st["run_score"].view(-1), nb, out=cand, workspace=ws),
        "update_us": lambda: K.beam_update(cand, st, t, 0, False, 102, 1.0, False, nxt),
        "reorder_us": lambda: K.beam_reorder(kv[0], kv[1], tab[0], tab[1], st["parent"], R, t + 1),
    }
    out = {"B": B, "num_beams": nb, "position": t}
    for name, fn in groups.items():
        fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        out[name] = round(sorted(ts)[len(ts) // 2], 1)
    return out


def _device_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 1)


def sample_step_times(R, temperature, top_k, top_p, V=30524, reps=20):
    """device time (us, median of reps, each between two events) of sample_select on random N(0, 1) logits [R, V]:
    the call's filters, every filter alone, no filter, and the call's filters with the probabilities written; and
    of beam_select over the same rows (3 beams per image when R is a multiple of 3, else 1)"""
    dev = "cuda"
    logits = torch.randn(R, V, device=dev)
    ctl = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    tok = torch.zeros(R, dtype=torch.int64, device=dev)
    probs = torch.zeros(R, V, device=dev)
    ws = torch.empty(K.sample_select_workspace_bytes(R, V), dtype=torch.uint8, device=dev)
    out = {"rows": R, "V": V, "temperature": temperature, "top_k": top_k, "top_p": top_p}
    cases = {"select_us": (temperature, top_k, top_p), "no_filter_us": (1.0, 0, 1.0), "temperature_only_us": (0.7, 0, 1.0),
             "top_k_only_us": (1.0, 50, 1.0), "top_p_only_us": (1.0, 0, 0.9)}
    for name, (t, k, p) in cases.items():
        out[name] = _device_us(lambda: K.sample_select(logits, t, k, p, ctl, 3, out=tok, workspace=ws), reps)
    out["select_with_probs_us"] = _device_us(
        lambda: K.sample_select(logits, temperature, top_k, top_p, ctl, 3, out=tok, probs=probs, workspace=ws), reps)
    nb = 3 if R % 3 == 0 else 1
    running = -torch.rand(R, device=dev)
    cand = K.beam_select(logits, running, nb)
    bws = torch.empty(K.beam_select_workspace_bytes(R // nb, nb, V), dtype=torch.uint8, device=dev)
    out["beam_select_us"] = _device_us(lambda: K.beam_select(logits, running, nb, out=cand, workspace=bws), reps)
    out["beam_select_num_beams"] = nb
    return out


def sample_main(a):
    torch.manual_seed(0)
    m = BlipForConditionalGeneration().to("cuda").eval()
    for p in m.parameters():
        p.requires_grad_(False)
    n = a.num_return_sequences
    kw = dict(do_sample=True, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, num_return_sequences=n, seed=1)
    res = {"generate": [], "sample_step_times": [], "sampling": {k: v for k, v in kw.items() if k != "do_sample"}}
    for prec in ("fp32", "bf16"):
        m.set_precision(prec)
        for B in a.batches:
            R = B * n
            px = torch.randn(B, 3, 384, 384, device="cuda")
            pxr = torch.randn(R, 3, 384, 384, device="cuda")
            row = {"precision": prec, "B": B, "rows": R}
            for mode, g in (("eager", False), ("graph", True)):
                t_min, t_med = wall(lambda: m.generate(px, use_graph=g, **kw), a.reps)
                row["sample_" + mode + "_ms"], row["sample_" + mode + "_ms_min"] = round(t_med, 2), round(t_min, 2)
                t_min, t_med = wall(lambda: m.generate(pxr, use_graph=g), a.reps)
                row["greedy_same_rows_" + mode + "_ms"] = round(t_med, 2)
                row["greedy_same_rows_" + mode + "_ms_min"] = round(t_min, 2)
                t_min, t_med = wall(lambda: m.generate(px, use_graph=g), a.reps)
                row["greedy_same_images_" + mode + "_ms"] = round(t_med, 2)
            row["tokens"] = int(m.generate(px, use_graph=True, **kw).shape[1]) - 1
            row["note"] = ("greedy_same_rows runs the vision tower on `rows` images, sampling on B; greedy_same_images "
                           "decodes B rows")
            res["generate"].append(row)
            print(row, file=sys.stderr, flush=True)
            if prec == "fp32":  # the selection reads fp32 logits in both precisions
                res["sample_step_times"].append(sample_step_times(R, a.temperature, a.top_k, a.top_p))
                print(res["sample_step_times"][-1], file=sys.stderr, flush=True)
        m.invalidate_caches()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def wide_head_main(a):
    """the LM head alone at the model's shapes: the narrow kernel at 32 rows, the wide one at 32 .. 256"""
    res = {"lm_head": []}
    for prec, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for B, wide in ((32, False), (32, True), (64, True), (128, True), (256, True)):
            res["lm_head"].append(dict(lm_head_rate(dt, B, wide=wide), precision=prec))
            print(res["lm_head"][-1], file=sys.stderr, flush=True)
    _emit(res, a)


def _emit(res, a):
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


class IdTokenizer:
    """stands in for a tokenizer (none is needed to time the driver): a caption is its ids in decimal"""

    def batch_decode(self, ids, skip_special_tokens=True):
        return [" ".join(str(i) for i in row) for row in ids]


def csv_main(a):
    """the driver end to end on a.csv synthetic JPEGs (a.csv // 2 rows): images/s of mmfd.caption.process_csv, JPEG
    decode included, beside the same files decoded in this process and captioned by Captioner.caption in 32-row
    chunks (what a driver on the 32-row model would do), the decode pool alone and the GPU alone"""
    import tempfile

    import numpy as np
    import pandas as pd
    from PIL import Image

    from mmfd.caption import Captioner, process_csv
    from mmfd.hostdecode import DecodePool
    n = a.csv // 2 * 2
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    m = BlipForConditionalGeneration().to("cuda").eval()
    for p in m.parameters():
        p.requires_grad_(False)
    res = {"csv": [], "images": n, "image_size": [a.csv_side, a.csv_side], "batch_rows": a.batch_rows}
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "img"))
        low = rng.integers(0, 256, (n, a.csv_side // 8, a.csv_side // 8, 3), dtype=np.uint8)
        for i in range(n):  # smooth noise: JPEGs of a photograph's size on disk rather than of white noise's
            Image.fromarray(low[i]).resize((a.csv_side, a.csv_side), Image.BICUBIC).save(
                os.path.join(root, "img", f"{i}.jpg"), quality=90)
        rows = [{"claim": f"c{r}", "evidence": f"e{r}", "claim_image": f"img/{2 * r}.jpg",
                 "evidence_image": f"img/{2 * r + 1}.jpg"} for r in range(n // 2)]
        src = os.path.join(root, "in.csv")
        pd.DataFrame(rows).to_csv(src, index=False)
        paths = [os.path.join(root, "img", f"{i}.jpg") for i in range(n)]
        for prec in ("fp32", "bf16"):
            m.set_precision(prec)
            row = {"precision": prec}
            wide = Captioner(m, tokenizer=IdTokenizer(), max_rows=max(32, 2 * a.batch_rows))
            warm = os.path.join(root, "warm.csv")
            process_csv(src, warm, wide, root=root, batch_rows=a.batch_rows, max_batches=1)  # captures the graph
            dst = os.path.join(root, f"out_{prec}.csv")
            t0 = time.perf_counter()
            process_csv(src, dst, wide, root=root, batch_rows=a.batch_rows)
            row["driver_s"] = round(time.perf_counter() - t0, 3)
            row["driver_images_per_s"] = round(n / row["driver_s"], 1)
            pool = DecodePool(group=1)
            t0 = time.perf_counter()
            imgs = [DecodePool.get([f])[0][0] for f in pool.submit(paths)]
            row["decode_pool_alone_s"] = round(time.perf_counter() - t0, 3)
            row["decode_workers"] = pool.workers
            pool.close()
            step = 2 * a.batch_rows
            wide.caption(imgs[:step])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(0, n, step):
                wide.caption(imgs[i:i + step])
            row["gpu_alone_wide_s"] = round(time.perf_counter() - t0, 3)
            m.invalidate_caches()
            narrow = Captioner(m, tokenizer=IdTokenizer())
            narrow.caption(imgs[:32])  # captures the 32-row graph
            t0 = time.perf_counter()
            for i in range(0, n, 32):
                with_decode = [np.asarray(Image.open(q).convert("RGB")) for q in paths[i:i + 32]]
                narrow.caption(with_decode)
            row["narrow_inline_decode_s"] = round(time.perf_counter() - t0, 3)
            row["narrow_images_per_s"] = round(n / row["narrow_inline_decode_s"], 1)
            t0 = time.perf_counter()
            for i in range(0, n, 32):
                narrow.caption(imgs[i:i + 32])
            row["gpu_alone_narrow_s"] = round(time.perf_counter() - t0, 3)
            m.invalidate_caches()
            res["csv"].append(row)
            print(row, file=sys.stderr, flush=True)
    _emit(res, a)


PROCESSORS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=12, suppress_tokens=[100, 101, 103])


def processor_step_times(R, V=30524, cur=21, reps=20):
    """device time (us, median of reps, each between two events) of the kernels a step with processors adds, on
    random N(0, 1) scores [R, V] and a random int64 step-major history of `cur` ids per row: the edits (all rules,
    and the penalty alone), the row argmax of the greedy path, and the in-place log-softmax of the beam path beside
    the selection with and without its own normalisation (3 beams per image when R is a multiple of 3, else 1)"""
    dev = "cuda"
    scores = torch.randn(R, V, device=dev)
    hist = torch.randint(0, V, (cur, max(R, 16)), device=dev)
    sup = torch.tensor(PROCESSORS["suppress_tokens"], dtype=torch.int64, device=dev)
    tok = torch.zeros(R, dtype=torch.int64, device=dev)
    out = {"rows": R, "V": V, "cur_len": cur, "argmax_bytes_per_row": V * 4}
    out["edit_all_us"] = _device_us(lambda: K.logits_process(scores, hist, cur, repetition_penalty=1.3,
                                                             no_repeat_ngram_size=2, suppress_eos=True, eos=102,
                                                             suppress=sup, history_layout="steps"), reps)
    scores = torch.randn(R, V, device=dev)
    out["edit_penalty_us"] = _device_us(lambda: K.logits_process(scores, hist, cur, repetition_penalty=1.3,
                                                                 history_layout="steps"), reps)
    out["row_argmax_us"] = _device_us(lambda: K.row_argmax(scores, out=tok), reps)
    nb = 3 if R % 3 == 0 else 1
    running = -torch.rand(R, device=dev)
    ws = torch.empty(K.beam_select_workspace_bytes(R // nb, nb, V), dtype=torch.uint8, device=dev)
    cand = K.beam_select(scores, running, nb)
    out["beam_select_us"] = _device_us(lambda: K.beam_select(scores, running, nb, out=cand, workspace=ws), reps)
    out["beam_select_logprobs_us"] = _device_us(lambda: K.beam_select_logprobs(scores, running, nb, out=cand,
                                                                                workspace=ws), reps)
    out["row_log_softmax_us"] = _device_us(lambda: K.row_log_softmax(scores, workspace=ws), reps)
    out["beam_select_num_beams"] = nb
    return out


def processors_main(a):
    torch.manual_seed(0)
    m = BlipForConditionalGeneration().to("cuda").eval()
    for p in m.parameters():
        p.requires_grad_(False)
    modes = {"greedy": (dict(), 1, [1, 32]), "beams3": (dict(num_beams=3), 3, [1, 10]),
             "samples3": (dict(do_sample=True, top_k=50, top_p=0.9, num_return_sequences=3, seed=1), 3, [1, 10])}
    res = {"generate": [], "processor_step_times": [], "processors": PROCESSORS}
    for prec in ("fp32", "bf16"):
        m.set_precision(prec)
        for name, (kw, per_image, batches) in modes.items():
            for B in batches:
                px = torch.randn(B, 3, 384, 384, device="cuda")
                row = {"precision": prec, "mode": name, "B": B, "rows": B * per_image}
                for tag, proc in (("off", {}), ("on", PROCESSORS)):
                    t_min, t_med = wall(lambda: m.generate(px, use_graph=True, **kw, **proc), a.reps)
                    row[tag + "_ms"], row[tag + "_ms_min"] = round(t_med, 2), round(t_min, 2)
                    row[tag + "_ms_per_image"] = round(t_med / B, 3)
                    row[tag + "_tokens"] = int(m.generate(px, use_graph=True, **kw, **proc).shape[1]) - 1
                row["on_minus_off_us_per_step"] = round((row["on_ms"] - row["off_ms"]) * 1e3 / 20, 1)
                res["generate"].append(row)
                print(row, file=sys.stderr, flush=True)
            m.invalidate_caches()
    for R in (1, 32, 30):
        res["processor_step_times"].append(processor_step_times(R))
        print(res["processor_step_times"][-1], file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def xent_times(dt, R, V=30524, reps=20):
    """device time (us, median) of vocab_xent_fwd (both launches) and vocab_xent_bwd on random [R, V] logits, laid
    out as the model lays them out: rows of vocab_ld(V) columns"""
    from mmfd.blip import vocab_ld
    ld = vocab_ld(V)
    z = torch.randn(R, ld, device="cuda")[:, :V]
    y = torch.randint(0, V, (R,), device="cuda")
    rows, lse, lse_lo, mean, n_valid, _ = K.vocab_xent_fwd(z, y, 0.1, check_labels=False)
    d = torch.zeros(R, ld, device="cuda", dtype=dt)[:, :V]
    esz = d.element_size()
    out = {"R": R, "V": V, "ld": ld, "fwd_bytes": R * V * 4, "bwd_bytes": R * V * (4 + esz)}
    for name, fn, nbytes in (("fwd", lambda: K.vocab_xent_fwd(z, y, 0.1, check_labels=False), R * V * 4),
                             ("bwd", lambda: K.vocab_xent_bwd(z, y, lse, lse_lo, 0.1, dt, n_valid=n_valid, out=d),
                              R * V * (4 + esz))):
        fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        med = sorted(ts)[len(ts) // 2]
        out[name + "_us"] = round(med * 1e6, 1)
        out[name + "_TBps"] = round(nbytes / med / 1e12, 3)
    out["note"] = "warm: the logits (R * V * 4 bytes) fit the last-level cache when R * V * 4 < 256 MiB"
    return out


def loss_main(a):
    from mmfd.blip import BlipConfig, lm_head_gemm_paths
    torch.manual_seed(0)
    m = BlipForConditionalGeneration(BlipConfig(train_text_decoder=True)).to("cuda").eval()
    m.config.text.label_smoothing = 0.1
    T = a.seq
    res = {"loss": [], "xent": [], "T": T}
    for prec, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        m.set_precision(prec)
        for B in a.batches:
            px = torch.randn(B, 3, 384, 384, device="cuda")
            ids = torch.randint(1000, 30000, (B, T))
            ids[:, 0] = m.config.text.bos_token_id

            def fwd():
                with torch.no_grad():
                    return m(px, ids, labels=ids).loss

            def fwd_bwd():
                for p in m.parameters():
                    p.grad = None
                m(px, ids, labels=ids).loss.backward()

            def vision():
                return m.image_embeds(px)

            row = {"precision": prec, "B": B, "T": T}
            for name, fn in (("forward", fwd), ("forward_backward", fwd_bwd), ("vision_tower", vision)):
                t_min, t_med = wall(fn, a.reps)
                row[name + "_ms"], row[name + "_ms_min"] = round(t_med, 2), round(t_min, 2)
            row["loss"] = round(float(fwd()), 4)
            tc = m.config.text
            row["lm_head_gemms"] = {k: v[1] for k, v in lm_head_gemm_paths(dt, B * T, tc.vocab_size, tc.hidden_size).items()}
            res["loss"].append(row)
            print(row, file=sys.stderr, flush=True)
            res["xent"].append(dict(xent_times(dt, B * T), precision=prec))
            print(res["xent"][-1], file=sys.stderr, flush=True)
        m.invalidate_caches()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 20])
    ap.add_argument("--num-beams", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loss", action="store_true", help="time the caption loss (forward, forward + backward)")
    ap.add_argument("--seq", type=int, default=21, help="--loss: tokens per caption")
    ap.add_argument("--sample", action="store_true", help="time generate(do_sample=True) and sample_select")
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--num-return-sequences", type=int, default=1)
    ap.add_argument("--processors", action="store_true", help="time generate with the logits processors off and on")
    ap.add_argument("--lm-head-wide", action="store_true", help="time the LM head alone, narrow at 32 rows and wide up to 256")
    ap.add_argument("--csv", type=int, default=0, help="time mmfd.caption.process_csv on this many synthetic JPEGs")
    ap.add_argument("--csv-side", type=int, default=400, help="--csv: side of the synthetic JPEGs")
    ap.add_argument("--batch-rows", type=int, default=64, help="--csv: rows per batch of the driver")
    a = ap.parse_args()
    if a.lm_head_wide:
        return wide_head_main(a)
    if a.csv:
        return csv_main(a)
    if a.processors:
        a.reps = max(a.reps, 7)
        return processors_main(a)
    if a.sample:
        return sample_main(a)
    if a.loss:
        if a.batches == [1, 20]:
            a.batches = [20]
        a.reps = max(a.reps, 7)
        return loss_main(a)
    torch.manual_seed(0)
    m = BlipForConditionalGeneration().to("cuda").eval()
    for p in m.parameters():
        p.requires_grad_(False)
    nb = a.num_beams
    gen = (lambda px, g: m.generate(px, use_graph=g)) if nb == 1 else \
        (lambda px, g: m.generate(px, use_graph=g, num_beams=nb))
    res = {"generate": [], "lm_head": [], "num_beams": nb, "beam_step": []}
    for prec, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        m.set_precision(prec)
        for B in a.batches:
            px = torch.randn(B, 3, 384, 384, device="cuda")
            row = {"precision": prec, "B": B, "rows": B * nb}
            for mode, g in (("eager", False), ("graph", True)):
                t_min, t_med = wall(lambda: gen(px, g), a.reps)
                row[mode + "_ms"] = round(t_med, 2)
                row[mode + "_ms_per_image"] = round(t_med / B, 2)
                row[mode + "_ms_min"] = round(t_min, 2)
            row["tokens"] = int(gen(px, True).shape[1]) - 1
            res["generate"].append(row)
            print(row, file=sys.stderr, flush=True)
            if nb == 1 or B * nb <= 32:
                res["lm_head"].append(dict(lm_head_rate(dt, B * nb), precision=prec))
                print(res["lm_head"][-1], file=sys.stderr, flush=True)
            if nb > 1:
                res["beam_step"].append(dict(beam_step_times(dt, B, nb), precision=prec))
                print(res["beam_step"][-1], file=sys.stderr, flush=True)
        m.invalidate_caches()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
