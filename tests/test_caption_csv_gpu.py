"""mmfd.caption.process_csv end to end on the GPU: the fixture model (blip_small.npz), the toy tokenizer, 45 rows
with 90 random PNGs (48 x 40 and 40 x 56), batch_rows=20 — captioning calls of 40, 40 and 10 images — interrupted
after one batch and resumed.

Every caption must equal `Captioner(model, tokenizer).caption([image])` of that image alone, for the images whose
float64 greedy decode (tests/caption_wide_refs.py, on the pixels the device preprocessing produced) has a top-2
margin >= 1e-3 at every live step; at least 90 % of the images must qualify. SEED = 3, chosen on the CPU with PIL's
own bicubic resize in place of the device's (the two agree bit for bit, tests/test_preprocess_gpu.py): all 90 images
qualify (smallest margins 0.0012, 0.0029, 0.0039; seeds 7, 1 and 2 gave 88, 89 and 88), and the evidence image of
row 19 has a caption that is not empty — an empty one reads back as NA, and the resumed run would start at row 19
instead of 20, as the reference's would."""
import numpy as np
import pandas as pd
import pytest

from tests import blip_refs as R
from tests import caption_wide_refs as CW
from tests import test_caption_gpu as TC

pytestmark = pytest.mark.gpu
ROWS, SEED = 45, 3


def make_images(seed=SEED):
    """90 uint8 HWC images: claim images 48 x 40, evidence images 40 x 56"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (48, 40, 3) if i % 2 == 0 else (40, 56, 3), dtype=np.uint8) for i in range(2 * ROWS)]


class CountingCaptioner:
    """passes `caption` through and records how many images each call held"""

    def __init__(self, cap):
        self.cap, self.calls = cap, []

    def caption(self, images):
        self.calls.append(len(images))
        return self.cap.caption(images)


def test_driver_matches_single_image_captions_and_resumes(tmp_path):
    from PIL import Image

    from mmfd.caption import Captioner, process_csv
    from tests.toy_tokenizer import toy_tokenizer
    z, cfg, W = R.load_fixture()
    model = TC._model(dict(cfg=cfg, W=W))
    tok = toy_tokenizer()
    images = make_images()
    (tmp_path / "img").mkdir()
    rec = []
    for r in range(ROWS):
        row = {"id": r, "claim": f"claim {r}", "evidence": f"evidence {r}"}
        for j, col in enumerate(("claim_image", "evidence_image")):
            row[col] = f"img/{r}_{j}.png"
            Image.fromarray(images[2 * r + j]).save(tmp_path / row[col])
        rec.append(row)
    pd.DataFrame(rec).to_csv(tmp_path / "in.csv", index=False)

    cap = CountingCaptioner(Captioner(model, tokenizer=tok, max_rows=40))
    src, dst = str(tmp_path / "in.csv"), str(tmp_path / "out.csv")
    assert process_csv(src, dst, cap, root=str(tmp_path), batch_rows=20, workers=4, max_batches=1) == 20
    part = pd.read_csv(dst)
    assert len(part) == ROWS and part["claim_enriched"].iloc[:20].notna().all()
    assert part[["evidence_image_caption", "claim_enriched"]].iloc[20:].isna().all().all()
    assert process_csv(src, dst, cap, root=str(tmp_path), batch_rows=20, workers=4) == 25
    assert cap.calls == [40, 40, 10]
    out = pd.read_csv(dst, keep_default_na=False)
    got = [out.at[r, c] for r in range(ROWS) for c in ("claim_image_caption", "evidence_image_caption")]

    single = Captioner(model, tokenizer=tok)
    px = single.pixels(images).float().cpu()
    assert tuple(px.shape) == (90, 3, 80, 80)
    _, margin = CW.greedy_with_margins(W, cfg, px)
    ok = (margin >= CW.MARGIN).tolist()
    print(f"csv driver: {sum(ok)} of 90 images compared, smallest margins {sorted(margin.tolist())[:3]}")
    assert sum(ok) >= 81
    alone = [single.caption([im])[0] for im in images]
    assert any(alone)
    bad = [i for i in range(90) if ok[i] and got[i] != alone[i]]
    assert not bad, [(i, got[i], alone[i]) for i in bad[:5]]
    for r in range(ROWS):
        assert out.at[r, "claim_enriched"] == f"claim {r}. {got[2 * r]}"
        assert out.at[r, "evidence_enriched"] == f"evidence {r}. {got[2 * r + 1]}"
