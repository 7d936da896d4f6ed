"""The reference's captioning call site on the HIP path: src/preprocess/caption.py:22-31
(`inputs = processor(image, return_tensors="pt"); out = model.generate(**inputs);
processor.decode(out[0], skip_special_tokens=True)`) and the same call in src/demo/app.py.

`Captioner` takes already preprocessed pixel tensors ([B, 3, S, S], BLIP's mean / std normalisation
applied): BLIP's processor resizes with PIL's bicubic filter, which preprocess.hip does not have yet
(bilinear taps only), so raw-image input is a follow-up, as are the resumable CSV driver, beam search /
sampling, and training."""
from __future__ import annotations

import torch

from .blip import BlipForConditionalGeneration


class Captioner:
    """captions for batches of preprocessed images: `.generate_ids(pixel_values)` -> int64 [B, 1 + n] ids
    (bos first), `.caption(pixel_values)` -> list of B strings through `tokenizer` (any object with
    transformers' `batch_decode(ids, skip_special_tokens=True)` or `decode`; loaded by the caller from a
    local directory — nothing is fetched here)."""

    def __init__(self, model: BlipForConditionalGeneration, tokenizer=None, max_new_tokens=20, use_graph=True):
        self.model = model.eval()
        self.tokenizer = tokenizer
        self.max_new_tokens, self.use_graph = int(max_new_tokens), bool(use_graph)

    @torch.no_grad()
    def generate_ids(self, pixel_values, input_ids=None):
        px = torch.as_tensor(pixel_values)
        if px.dim() == 3:
            px = px[None]
        return self.model.generate(px, input_ids=input_ids, max_new_tokens=self.max_new_tokens,
                                   use_graph=self.use_graph)

    def caption(self, pixel_values, input_ids=None):
        if self.tokenizer is None:
            raise ValueError("Captioner.caption needs a tokenizer (Captioner(model, tokenizer=...))")
        ids = self.generate_ids(pixel_values, input_ids)
        if hasattr(self.tokenizer, "batch_decode"):
            out = self.tokenizer.batch_decode(ids.tolist(), skip_special_tokens=True)
        else:
            out = [self.tokenizer.decode(r, skip_special_tokens=True) for r in ids.tolist()]
        return [s.strip() for s in out]
