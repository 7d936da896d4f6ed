"""Greedy BLIP captioning of more than 32 rows in one call (mmfd.blip generate on kernels.lm_head_argmax_wide) and
`Captioner(max_rows=...)`, on blip_small.npz.

40 images: the fixture's 4, then 36 of seeded noise. The reference is the float64 restatement (tests/
caption_wide_refs.py: blip_refs' vision tower and decoder under logits_ref's greedy loop). A row is compared only if
its smallest top-2 margin over its live steps is >= 1e-3 (ten times the fp32 logits bar of tests/test_caption_gpu.py);
at most 4 of the 40 rows may be left out. Checked on the CPU when this file was written: 39 rows qualify (smallest
margins 0.0006, 0.0038, 0.0048) and the restatement reproduces the fixture's four `sequences`; with the processors
of the last-but-one case 38 qualify (0.0001, 0.0006, 0.0026)."""
import pytest
import torch

from tests import blip_refs as R
from tests import caption_wide_refs as CW
from tests import test_caption_gpu as TC

pytestmark = pytest.mark.gpu
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3)


@pytest.fixture(scope="module")
def fx():
    z, cfg, W = R.load_fixture()
    px4 = torch.from_numpy(z["pixel_values"])
    noise = torch.randn(36, 3, 80, 80, generator=torch.Generator().manual_seed(40))
    px = torch.cat([px4, (noise * 64).round().clamp(-255, 255) / 64])
    ids, margin = CW.greedy_with_margins(W, cfg, px)
    assert torch.equal(ids[:4], CW.pad_to(torch.from_numpy(z["sequences"]), ids.shape[1], cfg["text"]["pad_token_id"]))
    rows = torch.nonzero(margin >= CW.MARGIN)[:, 0]
    print(f"wide captions: {len(rows)} of 40 rows compared, smallest margins {sorted(margin.tolist())[:3]}")
    assert len(rows) >= 36
    return dict(z=z, cfg=cfg, W=W, px=px, ref=ids, rows=rows, pad=cfg["text"]["pad_token_id"])


@pytest.fixture(scope="module")
def model32(fx):
    return TC._model(fx)


@pytest.fixture(scope="module")
def wide32(fx, model32):
    """generate(px40) in fp32, eager and graph: shared by the cases below"""
    return model32.generate(fx["px"], use_graph=False), model32.generate(fx["px"], use_graph=True)


def test_fp32_forty_rows_match_float64_eager_and_graph(fx, wide32):
    eager, graph = wide32
    assert eager.dtype == torch.int64 and eager.shape[0] == 40
    assert CW.rows_equal(eager, fx["ref"], fx["rows"], fx["pad"])
    assert torch.equal(eager, graph)


def test_fp32_two_narrow_calls_match_float64(fx, model32):
    for use_graph in (False, True):
        a, b = model32.generate(fx["px"][:32], use_graph=use_graph), model32.generate(fx["px"][32:], use_graph=use_graph)
        w = max(a.shape[1], b.shape[1])
        both = torch.cat([CW.pad_to(a, w, fx["pad"]), CW.pad_to(b, w, fx["pad"])])
        assert CW.rows_equal(both, fx["ref"], fx["rows"], fx["pad"])


def test_second_call_replays_the_captured_graph(fx, model32, wide32):
    model32.generate(fx["px"], use_graph=True)
    st = [s for s in model32._states.values() if s["B"] == 40 and s.get("wide")]
    assert len(st) == 1 and st[0]["graph"] is not None
    g = st[0]["graph"]
    perm = torch.arange(39, -1, -1)
    again = model32.generate(fx["px"][perm], use_graph=True)  # other pixels on the same static buffers
    now = [s for s in model32._states.values() if s["B"] == 40]
    assert len(now) == 1 and now[0] is st[0] and st[0]["graph"] is g  # the same state, no new capture
    assert CW.rows_equal(again[perm], fx["ref"], fx["rows"], fx["pad"])


def test_bf16_forty_rows_graph_equals_eager(fx):
    m = TC._model(fx, "bf16")
    eager, graph = m.generate(fx["px"], use_graph=False), m.generate(fx["px"], use_graph=True)
    assert torch.equal(eager, graph)
    assert eager.shape[0] == 40 and 2 <= eager.shape[1] <= 21
    TC._valid_structure(eager, fx["cfg"]["text"])


def test_fp32_forty_rows_with_logits_processors(fx, model32):
    ref, margin = CW.greedy_with_margins(fx["W"], fx["cfg"], fx["px"], **PROC)
    rows = torch.nonzero(margin >= CW.MARGIN)[:, 0]
    print(f"wide captions with processors: {len(rows)} of 40 rows compared, smallest margins {sorted(margin.tolist())[:3]}")
    assert len(rows) >= 36
    eager = model32.generate(fx["px"], use_graph=False, **PROC)
    graph = model32.generate(fx["px"], use_graph=True, **PROC)
    assert CW.rows_equal(eager, ref, rows, fx["pad"])
    assert torch.equal(eager, graph)


def test_row_limits(fx, model32):
    for rows in (129, 257):  # the kernel takes 256 rows, `generate` 128 (blip.py, MAX_GREEDY_ROWS)
        with pytest.raises(ValueError, match="at most 128 rows"):
            model32.generate(torch.zeros(rows, 3, 80, 80))
    with pytest.raises(ValueError, match="at most 32 rows"):  # teacher forcing keeps the narrow kernel
        model32.forward_logits(fx["px"][:33], torch.zeros(33, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"batch \* num_beams <= 32"):
        model32.generate(fx["px"][:11], num_beams=3)
    with pytest.raises(ValueError, match=r"batch \* num_return_sequences <= 32"):
        model32.generate(fx["px"][:33], do_sample=True)


def test_captioner_max_rows(fx, model32, wide32):
    from mmfd.caption import Captioner
    assert torch.equal(Captioner(model32, max_rows=64).generate_ids(fx["px"]), wide32[1])
    chunks = Captioner(model32, max_rows=20).generate_ids(fx["px"])  # two calls of 20 rows
    assert chunks.shape[0] == 40 and CW.rows_equal(chunks, fx["ref"], fx["rows"], fx["pad"])
    with pytest.raises(ValueError, match="max_rows"):
        Captioner(model32, max_rows=64, num_beams=2)
    with pytest.raises(ValueError, match="max_rows"):
        Captioner(model32, max_rows=64, do_sample=True)
    for rows in (0, 129, 257):
        with pytest.raises(ValueError, match="max_rows"):
            Captioner(model32, max_rows=rows)
