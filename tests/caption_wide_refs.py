"""float64 greedy captions with their top-2 margins, for the wide-batch captioning tests: tests/blip_refs.py's vision
tower and single-token decoder under tests/logits_ref.py's greedy loop (its processors included).

A GPU result is compared with the float64 ids only on rows whose smallest top-2 margin over their live steps is at
least MARGIN = 1e-3: ten times the 1e-4 fp32 logits bar of tests/test_caption_gpu.py (3.4e-6 measured there), so a
kernel within its bar cannot flip such a row's token."""
import torch

from tests import blip_refs as R
from tests import logits_ref as LR

MARGIN = 1e-3


def greedy_with_margins(W, cfg, px, max_new_tokens=20, **proc):
    """(ids int64 [B, 1 + n], margin float64 [B]): margin[b] is the smallest (best - second best) processed score of
    row b over the steps before it finished"""
    tc = cfg["text"]
    dec = R.Decoder(W, cfg, R.vision(W, cfg, px))
    trace = []
    # LR.greedy hands over the whole history once per step, in order: the cached decoder takes its last column
    ids = LR.greedy(lambda seq: dec.step(seq[:, -1]), px.shape[0], [tc["bos_token_id"]], max_new_tokens,
                    tc["sep_token_id"], tc["pad_token_id"], trace=trace, **proc)
    margin = torch.full((px.shape[0],), float("inf"), dtype=torch.float64)
    for _, scores, live in trace:
        top = scores.topk(2, dim=-1).values
        gap = top[:, 0] - top[:, 1]
        margin = torch.where(live, torch.minimum(margin, gap), margin)
    return ids, margin


def pad_to(ids, width, pad):
    return torch.nn.functional.pad(ids, (0, width - ids.shape[1]), value=pad)


def rows_equal(got, ref, rows, pad):
    """whether `got` and `ref` hold the same ids on `rows` once both are padded to one width"""
    w = max(got.shape[1], ref.shape[1])
    return torch.equal(pad_to(got, w, pad)[rows], pad_to(ref, w, pad)[rows])
