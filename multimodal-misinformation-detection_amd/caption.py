"""The reference's captioning call site on the HIP path: src/preprocess/caption.py:22-31
(`inputs = processor(image, return_tensors="pt"); out = model.generate(**inputs);
processor.decode(out[0], skip_special_tokens=True)`) and the same call in src/demo/app.py.

`Captioner` takes what the reference's processor takes — a PIL image, or a list of PIL images / uint8 HWC
arrays, resized and normalised on the device by mmfd.preprocess.ImagePreprocessor("blip") bit for bit as
transformers' BlipImageProcessor does it — or already preprocessed pixel tensors ([B, 3, S, S]). Decoding is
greedy, with num_beams > 1 transformers' beam search (mmfd.blip, csrc/beam.hip), or with do_sample=True
transformers' temperature / top-k / top-p sampling with num_return_sequences captions per image (csrc/sample.hip:
caption variants for augmentation, hypotheses for `score`). `Captioner.score` gives the log-likelihood of given
captions (the model's forward(labels=), csrc/lm_loss.hip): perplexity on held-out captions, re-scoring of
hypotheses. `repetition_penalty`, `no_repeat_ngram_size`, `min_length`, `min_new_tokens` and `suppress_tokens` are
transformers' logits processors, on the device in every decoding mode (csrc/logits.hip): what keeps a caption from
looping or stopping after three words. Still to follow: the resumable CSV driver."""
from __future__ import annotations

import torch

from . import kernels as K
from .blip import BlipForConditionalGeneration


class Captioner:
    """captions for batches of images: `.generate_ids(images)` -> int64 [B, 1 + n] ids (bos first),
    `.caption(images)` -> list of B strings through `tokenizer` (any object with transformers'
    `batch_decode(ids, skip_special_tokens=True)` or `decode`; loaded by the caller from a local directory —
    nothing is fetched here). `images`: a pixel tensor [B, 3, S, S] / [3, S, S], a PIL image, or a list of PIL
    images / uint8 HWC arrays. The model takes at most 32 rows per call (32 // num_beams images): larger
    batches run in chunks whose rows are padded with pad_token_id to one width.
    do_sample=True: num_return_sequences = n sampled captions per image, [B * n, ...] ids / a flat list of B * n
    strings, image-major (rows b*n .. b*n + n - 1 belong to image b), as transformers' generate and batch_decode
    return them. Chunks hold 32 // n images; every chunk gets the call's one seed (seed=None: drawn once per call
    from torch's global CPU generator) and its first global row as `row_offset`, so the result is the concatenation
    of those `generate` calls and does not depend on where the chunks are cut. `self.sample_seed`: the seed used."""

    def __init__(self, model: BlipForConditionalGeneration, tokenizer=None, max_new_tokens=20, use_graph=True,
                 num_beams=1, length_penalty=1.0, early_stopping=False, do_sample=False, temperature=1.0, top_k=0,
                 top_p=1.0, num_return_sequences=1, seed=None, repetition_penalty=1.0, no_repeat_ngram_size=0,
                 min_length=0, min_new_tokens=0, suppress_tokens=None):
        self.model = model.eval()
        self.tokenizer = tokenizer
        self.max_new_tokens, self.use_graph = int(max_new_tokens), bool(use_graph)
        self.num_beams, self.length_penalty, self.early_stopping = int(num_beams), float(length_penalty), early_stopping
        self.do_sample, self.temperature, self.top_k, self.top_p = bool(do_sample), temperature, top_k, top_p
        self.num_return_sequences, self.seed, self.sample_seed = int(num_return_sequences), seed, None
        if self.num_return_sequences < 1 or self.num_return_sequences > 32:
            raise ValueError(f"num_return_sequences must lie in [1, 32], got {num_return_sequences}")
        if self.num_return_sequences > 1 and not self.do_sample:
            raise ValueError("num_return_sequences > 1 needs do_sample=True")
        if self.do_sample and self.num_beams != 1:
            raise ValueError("do_sample together with num_beams > 1 (beam sampling) is not implemented")
        # transformers' logits processors (mmfd.blip generate, csrc/logits.hip); checked here so that a bad value is
        # refused where it is given. Only the ones that are on are passed on: a captioner without them calls
        # generate as it always did
        p, n, ml, mn, sup = K.check_processors(repetition_penalty, no_repeat_ngram_size, min_length, min_new_tokens,
                                               suppress_tokens, model.config.text.vocab_size)
        self.processors = {k: v for k, v, off in (("repetition_penalty", p, 1.0), ("no_repeat_ngram_size", n, 0),
                                                  ("min_length", ml, 0), ("min_new_tokens", mn, 0),
                                                  ("suppress_tokens", list(sup), [])) if v != off}
        self._pre = None

    def pixels(self, images):
        """images -> the model's pixel tensor [B, 3, S, S]"""
        if isinstance(images, torch.Tensor):
            return images[None] if images.dim() == 3 else images
        if not isinstance(images, (list, tuple)):
            images = [images]
        if self._pre is None:
            from .preprocess import ImagePreprocessor
            dev = next(self.model.parameters()).device
            self._pre = ImagePreprocessor("blip", device=dev, size=self.model.config.vision.image_size)
        return self._pre(list(images))

    @torch.no_grad()
    def generate_ids(self, pixel_values, input_ids=None):
        px = self.pixels(pixel_values)
        kw = dict(input_ids=input_ids, max_new_tokens=self.max_new_tokens, use_graph=self.use_graph, **self.processors)
        if self.num_beams != 1:
            kw.update(num_beams=self.num_beams, length_penalty=self.length_penalty, early_stopping=self.early_stopping)
        n = self.num_return_sequences
        if self.do_sample:
            seed = self.seed
            if seed is None:
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            self.sample_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            kw.update(do_sample=True, temperature=self.temperature, top_k=self.top_k, top_p=self.top_p,
                      num_return_sequences=n, seed=self.sample_seed)
        chunk = max(1, 32 // max(1, self.num_beams, n))
        if px.shape[0] <= chunk:
            return self.model.generate(px, **kw)
        row = (lambda i: dict(row_offset=i * n)) if self.do_sample else (lambda i: {})
        outs = [self.model.generate(px[i:i + chunk], **kw, **row(i)) for i in range(0, px.shape[0], chunk)]
        width = max(o.shape[1] for o in outs)
        pad = self.model.config.text.pad_token_id
        return torch.cat([torch.nn.functional.pad(o, (0, width - o.shape[1]), value=pad) for o in outs], 0)

    def caption(self, pixel_values, input_ids=None):
        if self.tokenizer is None:
            raise ValueError("Captioner.caption needs a tokenizer (Captioner(model, tokenizer=...))")
        ids = self.generate_ids(pixel_values, input_ids)
        if hasattr(self.tokenizer, "batch_decode"):
            out = self.tokenizer.batch_decode(ids.tolist(), skip_special_tokens=True)
        else:
            out = [self.tokenizer.decode(r, skip_special_tokens=True) for r in ids.tolist()]
        return [s.strip() for s in out]

    @torch.no_grad()
    def score(self, pixel_values, captions):
        """(log-likelihoods fp32 [B], token counts int64 [B]): for every (image, caption) pair the summed
        log-probability of the caption's tokens after the first — the negated reduction="none" caption loss without
        label smoothing — and the number of tokens summed. The captions are tokenised with the captioner's tokenizer
        and padded on the right; the first token becomes bos_token_id, as in `generate`; padding is not scored."""
        if self.tokenizer is None:
            raise ValueError("Captioner.score needs a tokenizer (Captioner(model, tokenizer=...))")
        px = self.pixels(pixel_values)
        if isinstance(captions, str):
            captions = [captions]
        if self.tokenizer.padding_side != "right":
            raise ValueError("Captioner.score needs a tokenizer that pads on the right")
        enc = self.tokenizer(list(captions), padding=True, return_tensors="pt")
        ids, mask = enc["input_ids"].long().clone(), enc["attention_mask"].long()
        if ids.shape[0] != px.shape[0]:
            raise ValueError(f"{px.shape[0]} images but {ids.shape[0]} captions")
        tc = self.model.config.text
        ids[:, 0] = tc.bos_token_id
        labels = ids.masked_fill(mask == 0, -100)
        out = self.model._caption_loss(px, ids, mask, labels, "none", False, label_smoothing=0.0)
        return -out.loss, (labels[:, 1:] != -100).sum(1)
