"""mmfd.caption.load_captioner and the command line `python -m mmfd.caption` without a GPU: a small HF-layout model
directory (blip_small.npz's weights and sizes) as `model.safetensors` — which holds no tied aliases, as transformers
writes it — and as `pytorch_model.bin`, a tokenizer directory, and `main([...])` with a stub captioner."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests import blip_refs as R

ALIASES = ("text_decoder.cls.predictions.decoder.weight", "text_decoder.cls.predictions.decoder.bias")


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    from safetensors.torch import save_file

    from tests.toy_tokenizer import toy_tokenizer
    _, cfg, W = R.load_fixture()
    root = tmp_path_factory.mktemp("hf")
    hf = {"model_type": "blip", "vision_config": cfg["vision"], "text_config": cfg["text"]}
    for name in ("st", "bin", "both", "diff"):
        os.makedirs(root / name)
        with open(root / name / "config.json", "w") as f:
            json.dump(hf, f)
    untied = {k: v.clone().contiguous() for k, v in W.items() if k not in ALIASES}
    assert len(untied) == len(W) - 2
    save_file(untied, str(root / "st" / "model.safetensors"))
    torch.save(dict(W), root / "bin" / "pytorch_model.bin")
    save_file(untied, str(root / "both" / "model.safetensors"))
    torch.save({k: torch.zeros_like(v) for k, v in W.items()}, root / "both" / "pytorch_model.bin")
    save_file(untied, str(root / "diff" / "model.safetensors"))
    text = {k: v for k, v in cfg["text"].items() if k != "hidden_size"}  # a config that leaves a size to the defaults
    with open(root / "diff" / "config.json", "w") as f:
        json.dump({"vision_config": cfg["vision"], "text_config": text}, f)
    toy_tokenizer().save_pretrained(str(root / "tok"))
    return root, cfg, W


@pytest.mark.parametrize("name", ["st", "bin", "both"])
def test_load_captioner_reads_both_weight_formats(dirs, name):
    from mmfd.caption import load_captioner
    root, cfg, W = dirs
    cap = load_captioner(str(root / name), str(root / "tok"), device="cpu", max_rows=40, max_new_tokens=7)
    m = cap.model
    sd = m.state_dict()
    assert set(sd) == set(W)
    for k, v in W.items():  # ("both": the safetensors file is the one that is read, not the zeroed .bin)
        assert torch.equal(sd[k], v), k
    pr = m.text_decoder.cls.predictions
    assert pr.decoder.weight is m.text_decoder.bert.embeddings.word_embeddings.weight and pr.decoder.bias is pr.bias
    assert m.config.text.hidden_size == cfg["text"]["hidden_size"] and m.config.vision.image_size == 80
    assert not any(p.requires_grad for p in m.parameters()) and not m.training
    assert cap.max_rows == 40 and cap.max_new_tokens == 7
    assert cap.tokenizer.decode([2, 5, 6, 3], skip_special_tokens=True) == "w0 w1"
    assert load_captioner(str(root / name), cap.tokenizer, device="cpu").tokenizer is cap.tokenizer  # an object passes


def test_load_captioner_reports_missing_files_and_other_shapes(dirs, tmp_path):
    from mmfd.caption import load_captioner
    root, _, _ = dirs
    with pytest.raises(FileNotFoundError, match="model.safetensors or pytorch_model.bin"):
        load_captioner(str(tmp_path), str(root / "tok"), device="cpu")
    with pytest.raises(RuntimeError, match=r"is \(\d+, \d+\) in the file but \(\d+, \d+\) by config.json"):
        load_captioner(str(root / "diff"), str(root / "tok"), device="cpu")


class Stub:
    max_rows = 40

    def caption(self, images):
        return [f"h{im.shape[0]}w{im.shape[1]}" for im in images]


def _project(root, names, rows=5):
    from PIL import Image
    os.makedirs(root / "data" / "preprocessed")
    os.makedirs(root / "img")
    rng = np.random.default_rng(1)
    for name in names:
        rec = []
        for r in range(rows):
            row = {"claim": f"c{r}", "evidence": f"e{r}"}
            for j, col in enumerate(("claim_image", "evidence_image")):
                row[col] = f"img/{name}_{r}_{j}.png"
                Image.fromarray(rng.integers(0, 256, (9 + r, 8 + j, 3), dtype=np.uint8)).save(root / row[col])
            rec.append(row)
        pd.DataFrame(rec).to_csv(root / "data" / "preprocessed" / f"{name}.csv", index=False)


def test_command_line_runs_one_file_and_the_reference_loop(tmp_path, monkeypatch):
    import mmfd.caption as C
    seen = {}

    def fake(model_dir, tokenizer, **kw):
        seen.update(kw, model_dir=model_dir, tokenizer=tokenizer)
        return Stub()

    monkeypatch.setattr(C, "load_captioner", fake)
    _project(tmp_path, ("train", "test"))
    pre = tmp_path / "data" / "preprocessed"
    out = tmp_path / "one.csv"
    assert C.main(["--input", str(pre / "train.csv"), "--output", str(out), "--model", "M", "--tokenizer", "T",
                   "--root", str(tmp_path), "--batch-rows", "3", "--precision", "bf16", "--max-new-tokens", "9",
                   "--repetition-penalty", "1.3", "--workers", "2"]) == 0
    assert (seen["model_dir"], seen["tokenizer"], seen["precision"], seen["max_new_tokens"]) == ("M", "T", "bf16", 9)
    assert seen["max_rows"] == 32 and seen["repetition_penalty"] == 1.3 and seen["num_beams"] == 1
    got = pd.read_csv(out)
    assert got["claim_image_caption"].tolist() == [f"h{9 + r}w8" for r in range(5)]
    assert got["evidence_enriched"].tolist() == [f"e{r}. h{9 + r}w9" for r in range(5)]
    # neither --input nor --output: {root}/data/preprocessed/{train,test}.csv -> {train,test}_enriched.csv
    assert C.main(["--model", "M", "--tokenizer", "T", "--root", str(tmp_path), "--batch-rows", "40", "--workers", "2"]) == 0
    assert seen["max_rows"] == 80
    for name in ("train", "test"):
        assert pd.read_csv(pre / f"{name}_enriched.csv")["claim_enriched"].tolist() == [f"c{r}. h{9 + r}w8" for r in range(5)]
    with pytest.raises(SystemExit):
        C.main(["--input", "x.csv", "--model", "M", "--tokenizer", "T"])           # --output is missing
    with pytest.raises(SystemExit):
        C.main(["--model", "M", "--tokenizer", "T", "--batch-rows", "65"])         # more than 128 rows per call
    os.remove(pre / "test.csv")
    with pytest.raises(FileNotFoundError, match="test.csv"):
        C.main(["--model", "M", "--tokenizer", "T", "--root", str(tmp_path), "--workers", "2"])


def test_a_captioner_of_fewer_rows_than_a_batch_is_warned_about(tmp_path):
    from mmfd.caption import process_csv
    _project(tmp_path, ("train",))
    src = str(tmp_path / "data" / "preprocessed" / "train.csv")
    narrow = Stub()
    narrow.max_rows = 32
    with pytest.warns(UserWarning, match="max_rows >= 40"):
        assert process_csv(src, str(tmp_path / "o.csv"), narrow, root=str(tmp_path), batch_rows=20, workers=2) == 5
    with pytest.raises(ValueError, match="batch_rows"):
        process_csv(src, str(tmp_path / "p.csv"), Stub(), root=str(tmp_path), batch_rows=65)
