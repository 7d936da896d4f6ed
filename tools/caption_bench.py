"""Times greedy BLIP captioning (mmfd.blip) at the default configuration (blip-image-captioning-large
shapes, random weights and pixels) and the LM-head kernel alone.

  python tools/caption_bench.py [--batches 1 20] [--reps 3] [--out FILE]

Per (batch, precision): wall time of `generate` (20 new tokens; host-synchronised, the ids copied back)
eager and as one graph replay, and per precision the device time of kernels.lm_head_argmax at
V = 30524, K = 768 with the bytes it has to read (W + bias + x) per second. Prints one JSON line.
Random weights seldom produce the stop token, so eager mode runs all 20 steps like the graph."""
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


def lm_head_rate(dtype, B, V=30524, Kd=768, reps=20):
    x = torch.randn(B, Kd, device="cuda").to(dtype)
    W = (torch.randn(V, Kd, device="cuda") * 0.02).to(dtype)
    bias = torch.zeros(V, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")  # larger than the 256 MiB last-level cache
    out = torch.empty(B, dtype=torch.int64, device="cuda")
    K.lm_head_argmax(x, W, bias, out=out)
    cold, warm = [], []
    for i in range(reps):
        if i % 2 == 0:
            flush.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.lm_head_argmax(x, W, bias, out=out)
        e1.record()
        torch.cuda.synchronize()
        (cold if i % 2 == 0 else warm).append(e0.elapsed_time(e1) * 1e-3)
    nbytes = W.numel() * W.element_size() + bias.numel() * 4 + x.numel() * x.element_size()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return {"B": B, "bytes": nbytes, "us_cold": round(med(cold) * 1e6, 1), "us_warm": round(med(warm) * 1e6, 1),
            "TBps_cold": round(nbytes / med(cold) / 1e12, 3), "TBps_warm": round(nbytes / med(warm) / 1e12, 3),
            "note": "both launches (partials + final reduce) between the events; cold = after a 512 MiB fill"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    m = BlipForConditionalGeneration().to("cuda").eval()
    for p in m.parameters():
        p.requires_grad_(False)
    res = {"generate": [], "lm_head": []}
    for prec, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        m.set_precision(prec)
        for B in a.batches:
            px = torch.randn(B, 3, 384, 384, device="cuda")
            row = {"precision": prec, "B": B}
            for mode, g in (("eager", False), ("graph", True)):
                t_min, t_med = wall(lambda: m.generate(px, use_graph=g), a.reps)
                row[mode + "_ms"] = round(t_med, 2)
                row[mode + "_ms_per_image"] = round(t_med / B, 2)
                row[mode + "_ms_min"] = round(t_min, 2)
            row["tokens"] = int(m.generate(px, use_graph=True).shape[1]) - 1
            res["generate"].append(row)
            print(row, file=sys.stderr, flush=True)
            res["lm_head"].append(dict(lm_head_rate(dt, B), precision=prec))
            print(res["lm_head"][-1], file=sys.stderr, flush=True)
        m.invalidate_caches()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
