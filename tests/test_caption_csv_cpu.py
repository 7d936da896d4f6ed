"""mmfd.caption.process_csv, the resumable captioning driver, with a stub captioner and no GPU: the four columns,
failed images, resuming, a stale output file, the atomic save and the batch_rows limit. Every run passes the
reference's batch_rows=20 (the driver's own default is 64).

45 rows and 90 small PNGs of distinct sizes; two paths do not exist and one file is not an image. The stub's caption
of an image is f"h{H}w{W}", so every caption names the file it was made from."""
import os

import numpy as np
import pandas as pd
import pytest

ROWS = 45
COLS = ["claim_image_caption", "evidence_image_caption", "claim_enriched", "evidence_enriched"]
MISSING = {(3, "claim_image"), (27, "evidence_image")}  # paths without a file
BROKEN = (21, "claim_image")                            # a text file with a .png name


class Stub:
    """caption(images) -> f"h{H}w{W}" per image; records the sizes of every call and runs `hook` first"""

    def __init__(self, hook=None):
        self.calls, self.hook = [], hook

    def caption(self, images):
        if self.hook is not None:
            self.hook()
        self.calls.append([tuple(im.shape) for im in images])
        for im in images:
            assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3
        return [f"h{im.shape[0]}w{im.shape[1]}" for im in images]


def _size(r, col):
    i = 2 * r + (col == "evidence_image")
    return 8 + i // 10, 8 + i % 10  # (H, W): 90 distinct sizes


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("csv")
    os.makedirs(root / "img")
    rng = np.random.default_rng(0)
    rec = []
    for r in range(ROWS):
        row = {"id": r, "claim": f"claim {r}", "evidence": f"evidence {r}", "label": r % 3}
        for col in ("claim_image", "evidence_image"):
            rel = f"img/{r}_{col}.png"
            row[col] = rel
            h, w = _size(r, col)
            if (r, col) in MISSING:
                continue
            if (r, col) == BROKEN:
                (root / rel).write_text("not an image")
                continue
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / rel)
        rec.append(row)
    pd.DataFrame(rec).to_csv(root / "in.csv", index=False)
    return root


def _expected(root):
    df = pd.read_csv(root / "in.csv")
    caps = {}
    for r in range(ROWS):
        for col in ("claim_image", "evidence_image"):
            bad = (r, col) in MISSING or (r, col) == BROKEN
            caps[r, col] = "" if bad else "h%dw%d" % _size(r, col)
    df["claim_image_caption"] = [caps[r, "claim_image"] for r in range(ROWS)]
    df["evidence_image_caption"] = [caps[r, "evidence_image"] for r in range(ROWS)]
    df["claim_enriched"] = [f"claim {r}. {caps[r, 'claim_image']}" for r in range(ROWS)]
    df["evidence_enriched"] = [f"evidence {r}. {caps[r, 'evidence_image']}" for r in range(ROWS)]
    return df


@pytest.fixture(scope="module")
def full(data):
    """one uninterrupted run, shared: (the output file's bytes, the stub, rows processed)"""
    from mmfd.caption import process_csv
    stub = Stub()
    n = process_csv(str(data / "in.csv"), str(data / "full.csv"), stub, root=str(data), batch_rows=20, workers=2)
    return (data / "full.csv").read_bytes(), stub, n


def test_full_run_writes_the_four_columns(data, full):
    raw, stub, n = full
    assert n == ROWS
    got = pd.read_csv(data / "full.csv", keep_default_na=False)
    exp = _expected(data)
    assert list(got.columns) == list(exp.columns) and list(got.columns[-4:]) == COLS
    for c in exp.columns:
        assert got[c].astype(str).tolist() == exp[c].astype(str).tolist(), c
    # one captioning call per batch of 20 rows: 40, 40 and 10 images less the ones that failed
    assert [len(c) for c in stub.calls] == [39, 38, 10]
    assert got.at[3, "claim_image_caption"] == "" and got.at[3, "claim_enriched"] == "claim 3. "
    assert got.at[3, "evidence_image_caption"] == "h%dw%d" % _size(3, "evidence_image")  # the rest of the row stands
    assert got.at[21, "claim_image_caption"] == "" and got.at[27, "evidence_enriched"] == "evidence 27. "


def test_interrupted_run_resumes_where_it_stopped(data, full):
    from mmfd.caption import process_csv
    out = str(data / "resume.csv")
    first = Stub()
    assert process_csv(str(data / "in.csv"), out, first, root=str(data), batch_rows=20, workers=2, max_batches=1) == 20
    part = pd.read_csv(out)
    assert len(part) == ROWS and part["evidence_image_caption"].notna().sum() == 20
    assert part["evidence_image_caption"].iloc[20:].isna().all() and part["claim_enriched"].iloc[20:].isna().all()
    second = Stub()
    assert process_csv(str(data / "in.csv"), out, second, root=str(data), batch_rows=20, workers=2) == ROWS - 20
    early = {_size(r, c) + (3,) for r in range(20) for c in ("claim_image", "evidence_image")}
    assert not early & {s for call in second.calls for s in call}  # rows 0..19 are not captioned again
    assert [len(c) for c in second.calls] == [38, 10]
    assert open(out, "rb").read() == full[0]
    assert process_csv(str(data / "in.csv"), out, Stub(), root=str(data), batch_rows=20, workers=2) == 0  # nothing left


def test_output_of_another_length_is_reinitialised(data, full):
    from mmfd.caption import process_csv
    out = str(data / "stale.csv")
    stale = pd.read_csv(data / "full.csv").iloc[:30]  # 30 finished rows of some other input
    stale.to_csv(out, index=False)
    stub = Stub()
    assert process_csv(str(data / "in.csv"), out, stub, root=str(data), batch_rows=20, workers=2) == ROWS
    assert sum(len(c) for c in stub.calls) == 90 - 3
    assert open(out, "rb").read() == full[0]


def test_output_is_never_seen_half_written(data, full):
    """the stub reads the output at the start of every batch: a complete CSV with as many finished rows as batches
    have been saved, and no temporary file is left behind"""
    from mmfd.caption import process_csv
    out = str(data / "atomic.csv")
    seen = []

    def hook():
        if os.path.exists(out):
            df = pd.read_csv(out)
            assert len(df) == ROWS and list(df.columns[-4:]) == COLS
            seen.append(int(df["claim_enriched"].notna().sum()))
        else:
            seen.append(None)

    assert process_csv(str(data / "in.csv"), out, Stub(hook), root=str(data), batch_rows=20, workers=2) == ROWS
    assert seen == [None, 20, 40]
    assert open(out, "rb").read() == full[0]
    assert sorted(f for f in os.listdir(data) if f.startswith("atomic.csv")) == ["atomic.csv"]


def test_batch_rows_above_the_rows_of_a_call_is_refused(data):
    from mmfd.caption import process_csv
    for rows in (129, 65, 0):  # 2 * batch_rows images are one call of at most 128 rows
        with pytest.raises(ValueError, match="batch_rows"):
            process_csv(str(data / "in.csv"), str(data / "never.csv"), Stub(), root=str(data), batch_rows=rows)
    assert not os.path.exists(data / "never.csv")
