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
looping or stopping after three words.

`process_csv` is the reference's driver of that call (src/preprocess/caption.py:22-117, its `process_csv`): it
walks a CSV, captions the claim image and the evidence image of every row, writes `claim_image_caption`,
`evidence_image_caption`, `claim_enriched` and `evidence_enriched`, saves after every batch of rows and resumes
after an interruption — the file mmfd.evidence.TextCorpus and mmfd.dataset.prepare_h5_dataset(enriched=True)
read. A batch's 2 * batch_rows images are ONE `Captioner.caption` call (`Captioner(max_rows=...)`: greedy
decoding of up to 128 rows per call, kernels.lm_head_argmax_wide), and the files of the next batch are decoded
by mmfd.hostdecode.DecodePool's worker processes while the GPU captions this one. `python -m mmfd.caption` is its
command line (weights and tokenizer from local directories; nothing is fetched)."""
from __future__ import annotations

import os
import sys

import torch

from . import kernels as K
from .blip import BlipForConditionalGeneration


class Captioner:
    """captions for batches of images: `.generate_ids(images)` -> int64 [B, 1 + n] ids (bos first),
    `.caption(images)` -> list of B strings through `tokenizer` (any object with transformers'
    `batch_decode(ids, skip_special_tokens=True)` or `decode`; loaded by the caller from a local directory —
    nothing is fetched here). `images`: a pixel tensor [B, 3, S, S] / [3, S, S], a PIL image, or a list of PIL
    images / uint8 HWC arrays. A call of the model takes `max_rows` rows (default 32; greedy decoding up to 128,
    beam search and sampling 32, i.e. 32 // num_beams images): larger batches run in chunks whose rows are padded
    with pad_token_id to one width.
    do_sample=True: num_return_sequences = n sampled captions per image, [B * n, ...] ids / a flat list of B * n
    strings, image-major (rows b*n .. b*n + n - 1 belong to image b), as transformers' generate and batch_decode
    return them. Chunks hold 32 // n images; every chunk gets the call's one seed (seed=None: drawn once per call
    from torch's global CPU generator) and its first global row as `row_offset`, so the result is the concatenation
    of those `generate` calls and does not depend on where the chunks are cut. `self.sample_seed`: the seed used."""

    def __init__(self, model: BlipForConditionalGeneration, tokenizer=None, max_new_tokens=20, use_graph=True,
                 num_beams=1, length_penalty=1.0, early_stopping=False, do_sample=False, temperature=1.0, top_k=0,
                 top_p=1.0, num_return_sequences=1, seed=None, repetition_penalty=1.0, no_repeat_ngram_size=0,
                 min_length=0, min_new_tokens=0, suppress_tokens=None, max_rows=32):
        self.model = model.eval()
        self.max_rows = int(max_rows)
        if int(max_rows) != max_rows or not 1 <= self.max_rows <= BlipForConditionalGeneration.MAX_GREEDY_ROWS:
            raise ValueError(f"max_rows must lie in [1, {BlipForConditionalGeneration.MAX_GREEDY_ROWS}], got {max_rows!r}")
        if self.max_rows > 32 and (int(num_beams) > 1 or do_sample):
            raise ValueError(f"max_rows = {max_rows} needs greedy decoding: beam search and sampling take at most 32 "
                             f"rows per call")
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
        if self.num_beams == 1 and not self.do_sample:
            chunk = self.max_rows
        else:
            chunk = max(1, min(32, self.max_rows) // max(1, self.num_beams, n))
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


# ---- the resumable CSV driver ------------------------------------------------------------------------
CAPTION_COLUMNS = ("claim_image_caption", "evidence_image_caption", "claim_enriched", "evidence_enriched")
MAX_BATCH_ROWS = BlipForConditionalGeneration.MAX_GREEDY_ROWS // 2  # 2 * 64 images: the rows of one generate call


def _last_processed_index(df):
    """the last row whose evidence_image_caption is not NA, -1 when there is none"""
    import pandas as pd
    done = pd.notna(df["evidence_image_caption"]).to_numpy().nonzero()[0]
    return int(done[-1]) if len(done) else -1


def _save_csv(df, path):
    """written beside `path` and moved over it: a kill during a save leaves the previous file, never a torn one"""
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        df.to_csv(tmp, index=False)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def process_csv(input_csv, output_csv, captioner, root=".", batch_rows=64, workers=None, max_batches=None):
    """The reference's process_csv on the HIP path; returns the number of rows captioned in this call.

    `input_csv` is read with pandas. `output_csv` is loaded if it exists and has the input's length, else created
    as a copy of the input with the four CAPTION_COLUMNS set to NA (an output of another length is reinitialised
    from the input; the reference says so and then goes on with the stale frame). Work resumes after the last
    row whose evidence_image_caption is not NA; rows past it that already hold one are skipped. Per row the
    images `f"{root}/{row['claim_image']}"` and `f"{root}/{row['evidence_image']}"` are opened as RGB; one that
    cannot be opened or decoded is reported and gets the caption "" without touching the rest of its batch.
    claim_enriched = f"{claim}. {caption}", evidence_enriched likewise. After every `batch_rows` rows the output is
    written (index=False; to a temporary file in the same directory, then os.replace) and progress is printed.

    The 2 * batch_rows images of a batch go through one `captioner.caption(list of uint8 HWC arrays)` call (build
    the captioner with max_rows >= 2 * batch_rows to make that one generate call: a captioner whose max_rows is
    smaller cuts the batch into several and is warned about; batch_rows above 64 is refused), and the files of batch k + 1 are decoded while batch k is captioned: hostdecode.DecodePool, one image
    per task so that a bad file costs one caption, at most min(16, CPUs of this process) workers (`workers`).
    `max_batches`: stop after that many batches (a trial run). The default batch_rows is 64, the reference's is 20:
    128 rows per call is what measured fastest per image ("Captioning")."""
    from concurrent.futures.process import BrokenProcessPool

    import pandas as pd

    from .hostdecode import DecodePool
    if int(batch_rows) != batch_rows or not 1 <= batch_rows <= MAX_BATCH_ROWS:
        raise ValueError(f"batch_rows must lie in [1, {MAX_BATCH_ROWS}] (2 * batch_rows images are one captioning "
                         f"call of at most {2 * MAX_BATCH_ROWS} rows), got {batch_rows!r}")
    batch_rows = int(batch_rows)
    rows_per_call = getattr(captioner, "max_rows", None)
    if rows_per_call is not None and rows_per_call < 2 * batch_rows:
        import warnings
        warnings.warn(f"process_csv: the captioner takes {rows_per_call} rows per call, so the {2 * batch_rows} images of "
                      f"a batch are captioned in several calls; build it with max_rows >= {2 * batch_rows} (greedy "
                      f"decoding) or lower batch_rows", stacklevel=2)
    input_df = pd.read_csv(input_csv)
    output_df = None
    if os.path.exists(output_csv):
        output_df = pd.read_csv(output_csv)
        if len(output_df) != len(input_df) or any(c not in output_df.columns for c in CAPTION_COLUMNS):
            print(f"{output_csv} does not match {input_csv} (rows or columns): starting it again from the input")
            output_df = None
    if output_df is None:
        output_df = input_df.copy()
        for col in CAPTION_COLUMNS:
            output_df[col] = pd.NA
    for col in CAPTION_COLUMNS:  # (a column read back as all-NA is float64: strings go into object columns)
        output_df[col] = output_df[col].astype(object)
    total = len(input_df)
    start = _last_processed_index(output_df) + 1
    print(f"caption: {output_csv}: starting at row {start} of {total}")
    spans = [(i, min(i + batch_rows, total)) for i in range(start, total, batch_rows)]
    if max_batches is not None:
        spans = spans[:max(0, int(max_batches))]
    if not spans:
        return 0
    limit = min(16, len(os.sched_getaffinity(0)))
    pool = DecodePool(workers=max(1, min(int(workers or limit), limit)), group=1)

    def submit(span):
        rows = [r for r in range(*span) if pd.isna(output_df.at[r, "evidence_image_caption"])]
        paths = [f"{root}/{input_df.at[r, col]}" for r in rows for col in ("claim_image", "evidence_image")]
        return rows, paths, pool.submit(paths)

    done = 0
    try:
        nxt = submit(spans[0])
        for k, span in enumerate(spans):
            rows, paths, handle = nxt
            nxt = submit(spans[k + 1]) if k + 1 < len(spans) else None  # decoded while this batch is captioned
            images, slots = [], []
            for i, (path, fut) in enumerate(zip(paths, handle)):
                try:
                    images += DecodePool.get([fut])[0]
                    slots.append(i)
                except BrokenProcessPool:  # the workers are gone: not a property of this file
                    raise
                except Exception as e:  # a missing or broken file costs its own caption only
                    print(f"caption: cannot read {path} ({type(e).__name__}: {e}); its caption stays empty")
            captions = [""] * len(paths)
            if images:
                for i, text in zip(slots, captioner.caption(images)):
                    captions[i] = text
            for j, r in enumerate(rows):
                claim_cap, evidence_cap = captions[2 * j], captions[2 * j + 1]
                output_df.at[r, "claim_image_caption"] = claim_cap
                output_df.at[r, "evidence_image_caption"] = evidence_cap
                output_df.at[r, "claim_enriched"] = f"{input_df.at[r, 'claim']}. {claim_cap}"
                output_df.at[r, "evidence_enriched"] = f"{input_df.at[r, 'evidence']}. {evidence_cap}"
            done += len(rows)
            _save_csv(output_df, output_csv)
            print(f"caption: rows up to {span[1]} of {total} saved", flush=True)
    finally:
        pool.close()
    return done


def load_captioner(model_dir, tokenizer, precision="fp32", device="cuda", **captioner_kw):
    """a Captioner from local files: `model_dir` holds HF-layout weights (`model.safetensors`, else
    `pytorch_model.bin`) and `config.json`; `tokenizer` is a local tokenizer directory
    (`AutoTokenizer.from_pretrained(dir, local_files_only=True)`) or a tokenizer object. Nothing is fetched by name.

    A safetensors file holds no aliases: `text_decoder.cls.predictions.decoder.weight` / `.bias`, which transformers
    ties to the word embeddings and `cls.predictions.bias`, may be absent and are tied here as well. Sizes come from
    `config.json`'s `vision_config` / `text_config`; a field it omits keeps this project's default, which is
    blip-image-captioning-large's, not transformers' (a config written as a diff against transformers' defaults
    builds other shapes: the mismatch is reported with both shapes). Decoding stops on `sep_token_id`, as
    transformers' BLIP does; `eos_token_id` is carried and unused. Without a `config.json` the defaults are used."""
    import json
    from dataclasses import fields

    from .blip import BlipConfig, BlipTextConfig, BlipVisionConfig
    cfg = BlipConfig()
    cj = os.path.join(model_dir, "config.json")
    if os.path.exists(cj):
        with open(cj) as f:
            hf = json.load(f)
        pick = lambda cls, d: cls(**{f.name: d[f.name] for f in fields(cls) if d.get(f.name) is not None})  # noqa: E731
        cfg = BlipConfig(vision=pick(BlipVisionConfig, hf.get("vision_config") or {}),
                         text=pick(BlipTextConfig, hf.get("text_config") or {}))
    model = BlipForConditionalGeneration(cfg)
    _load_blip_weights(model, model_dir)
    for p in model.parameters():
        p.requires_grad_(False)
    model = model.to(device).eval().set_precision(precision)
    if isinstance(tokenizer, (str, os.PathLike)):
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(tokenizer, local_files_only=True)
    return Captioner(model, tokenizer=tokenizer, **captioner_kw)


TIED = {"text_decoder.cls.predictions.decoder.weight": "text_decoder.bert.embeddings.word_embeddings.weight",
        "text_decoder.cls.predictions.decoder.bias": "text_decoder.cls.predictions.bias"}


def _load_blip_weights(model, model_dir):
    """model.safetensors (preferred, as transformers prefers it) or pytorch_model.bin into `model`; the tied decoder
    entries may be missing (TIED), anything else missing, unexpected or of another shape is an error"""
    st, pt = os.path.join(model_dir, "model.safetensors"), os.path.join(model_dir, "pytorch_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.exists(pt):
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{model_dir}: no model.safetensors or pytorch_model.bin")
    own = model.state_dict()
    sd = {k: v for k, v in sd.items() if k in own}  # (buffers such as position_ids of older checkpoints are dropped)
    for alias, src in TIED.items():
        if alias not in sd and src in sd:
            sd[alias] = sd[src]
    missing = sorted(set(own) - set(sd))
    if missing:
        raise RuntimeError(f"{model_dir}: weights missing for {missing[:5]}{' ...' if len(missing) > 5 else ''}")
    bad = [(k, tuple(sd[k].shape), tuple(own[k].shape)) for k in own if tuple(sd[k].shape) != tuple(own[k].shape)]
    if bad:
        k, got, want = bad[0]
        raise RuntimeError(f"{model_dir}: {k} is {got} in the file but {want} by config.json and this project's "
                           f"defaults for the fields it omits ({len(bad)} such tensors)")
    model.load_state_dict(sd, strict=True)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m mmfd.caption", description=(
        "Captions the claim and evidence image of every row of a CSV and writes the enriched CSV; resumes an "
        "interrupted run. Without --input / --output: data/preprocessed/{train,test}.csv -> {train,test}_enriched.csv "
        "under --root."))
    ap.add_argument("--input")
    ap.add_argument("--output")
    ap.add_argument("--model", required=True, help="local HF-layout directory of the BLIP weights")
    ap.add_argument("--tokenizer", required=True, help="local tokenizer directory")
    ap.add_argument("--root", default=".", help="the directory image paths are relative to")
    ap.add_argument("--batch-rows", type=int, default=64, help="rows per batch and save (the reference: 20)")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--max-new-tokens", type=int, default=20)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--max-batches", type=int, default=None)
    ap.add_argument("--num-beams", type=int, default=1)
    ap.add_argument("--length-penalty", type=float, default=1.0)
    ap.add_argument("--early-stopping", action="store_true")
    ap.add_argument("--do-sample", action="store_true")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--no-repeat-ngram-size", type=int, default=0)
    ap.add_argument("--min-length", type=int, default=0)
    ap.add_argument("--min-new-tokens", type=int, default=0)
    ap.add_argument("--suppress-tokens", type=int, nargs="*", default=None)
    a = ap.parse_args(argv)
    if (a.input is None) != (a.output is None):
        ap.error("--input and --output go together")
    if not 1 <= a.batch_rows <= MAX_BATCH_ROWS:
        ap.error(f"--batch-rows must lie in [1, {MAX_BATCH_ROWS}]")
    greedy = a.num_beams == 1 and not a.do_sample
    cap = load_captioner(
        a.model, a.tokenizer, precision=a.precision, max_new_tokens=a.max_new_tokens, num_beams=a.num_beams,
        length_penalty=a.length_penalty, early_stopping=a.early_stopping, do_sample=a.do_sample,
        temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=a.seed, repetition_penalty=a.repetition_penalty,
        no_repeat_ngram_size=a.no_repeat_ngram_size, min_length=a.min_length, min_new_tokens=a.min_new_tokens,
        suppress_tokens=a.suppress_tokens, max_rows=max(32, 2 * a.batch_rows) if greedy else 32, device=a.device)
    if a.input is not None:
        jobs = [(a.input, a.output)]
    else:
        pre = os.path.join(a.root, "data", "preprocessed")
        jobs = [(os.path.join(pre, f"{name}.csv"), os.path.join(pre, f"{name}_enriched.csv")) for name in ("train", "test")]
    for src, dst in jobs:
        if not os.path.exists(src):
            raise FileNotFoundError(f"no such input CSV: {src}")
        process_csv(src, dst, cap, root=a.root, batch_rows=a.batch_rows, workers=a.workers, max_batches=a.max_batches)
        print(f"caption: {dst} is complete" if a.max_batches is None else f"caption: stopped after {a.max_batches} batches")
    return 0


if __name__ == "__main__":
    sys.exit(main())
