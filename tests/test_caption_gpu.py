"""Greedy BLIP captioning on the HIP path: the decoding kernels (csrc/decode.hip) against float64
references, and mmfd.blip / mmfd.caption against transformers' outputs (tests/golden/blip_small.npz,
pinned to the single-token formulation by tests/test_blip_ref_cpu.py).

Kernel tolerances: test_kernels_gpu.py's rule err <= atol + rtol * |ref|max with (3e-5, 3e-5) in fp32 and
(2e-2, 2e-2) in bf16, references in float64 on the kernel's own (rounded) inputs. Model: image embeds 1e-4
abs in fp32 (test_encoders_gpu.py's bar for vit_small.npz); teacher-forced logits within 2 x the
|delta|max / max(1, |ref|max) that mmfd's BertModel shows on bert_small.npz in the same session and
precision (test_deberta_train_gpu.py's rule), with a floor of 1e-4 in fp32.

Measured on an MI355X when this file was written (single run): see DESIGN.md, "Captioning"."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import blip_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float32: (3e-5, 3e-5), torch.bfloat16: (2e-2, 2e-2)}
DTYPES = [torch.float32, torch.bfloat16]


def _rand(*shape, seed, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _bound(dtype, ref):
    atol, rtol = TOL[dtype]
    return atol + rtol * ref.abs().max().item()


# ---------------------------------------------------------------------------------------------
# attn_decode
# ---------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, H, Lk):
    B, HD = q.shape
    D = HD // H
    qh = q.double().view(B, H, D)
    kh, vh = k.double()[:, :Lk].reshape(B, Lk, H, D), v.double()[:, :Lk].reshape(B, Lk, H, D)
    s = torch.einsum("bhd,blhd->bhl", qh, kh) / math.sqrt(D)
    return torch.einsum("bhl,blhd->bhd", torch.softmax(s, -1), vh).reshape(B, HD)


ATTN_CASES = [(1, 1, 32, 1), (3, 2, 64, 17), (2, 3, 64, 64), (2, 3, 64, 65), (1, 12, 64, 577), (4, 2, 32, 1000)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,H,D,Lk", ATTN_CASES)
def test_attn_decode_matches_float64_and_attn_fwd(B, H, D, Lk, dtype):
    from mmfd import kernels as K
    q, k, v = (_rand(*s, seed=i, dtype=dtype) for i, s in enumerate(((B, H * D), (B, Lk, H * D), (B, Lk, H * D))))
    ref = _attn_ref(q, k, v, H, Lk)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o = K.attn_decode(qd, kd, vd, H, Lk)
    o2, _ = K.attn_fwd(qd[:, None, :], kd, vd, H)  # the tiled forward with one query row: a second reference
    torch.cuda.synchronize()
    err = (o.double().cpu() - ref).abs().max().item()
    err2 = (o.double().cpu() - o2[:, 0].double().cpu()).abs().max().item()
    splits = K.attn_decode_splits(B, H, Lk)
    print(f"attn_decode {(B, H, D, Lk)} {dtype}: splits {splits}, err {err:.3e}, vs attn_fwd {err2:.3e}, "
          f"bound {_bound(dtype, ref):.3e}")
    assert o.dtype == dtype and tuple(o.shape) == (B, H * D)
    assert err <= _bound(dtype, ref) and err2 <= _bound(dtype, ref)
    if Lk == 1000:
        assert splits > 1  # the split path with its combine kernel
    if Lk <= 64:
        assert splits == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_attn_decode_on_views_of_a_packed_cache(dtype):
    """K|V views of one [B, Lmax, 2*H*D] cache with Lmax > Lk: rows at and past Lk hold NaN and are never
    read; the output goes into the middle of a larger buffer whose other bytes stay as they were"""
    from mmfd import kernels as K
    B, H, D, Lk, Lmax = 3, 2, 64, 70, 96
    HD = H * D
    cache = _rand(B, Lmax, 2 * HD, seed=5, dtype=dtype)
    q = _rand(B, HD, seed=6, dtype=dtype)
    ref = _attn_ref(q, cache[..., :HD], cache[..., HD:], H, Lk)
    cache[:, Lk:] = float("nan")
    cd = cache.to(DEV)
    buf = torch.full((B + 2, HD + 16), 7.0, device=DEV, dtype=dtype)
    out = buf[1:1 + B, 8:8 + HD]
    assert K.attn_decode_splits(B, H, Lk) > 1
    K.attn_decode(q.to(DEV), cd[..., :HD], cd[..., HD:], H, Lk, out=out)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.isfinite(got).all()
    assert (got[1:1 + B, 8:8 + HD].double() - ref).abs().max().item() <= _bound(dtype, ref)
    got[1:1 + B, 8:8 + HD] = 7.0
    assert (got == 7.0).all()


def test_attn_decode_refuses_bad_arguments():
    from mmfd import kernels as K
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="mmfd_attn_decode.*head_dim"):
        K.attn_decode(z(1, 128), z(1, 4, 128), z(1, 4, 128), 1, 4)                       # D = 128
    with pytest.raises(RuntimeError, match="mmfd_attn_decode.*Lk"):
        K.attn_decode(z(1, 64), z(1, 4, 64), z(1, 4, 64), 1, 0)                          # no key
    flat = z(4 * 64 + 8)
    with pytest.raises(RuntimeError, match="mmfd_attn_decode.*aligned"):
        K.attn_decode(flat[1:65].view(1, 64), z(1, 4, 64), z(1, 4, 64), 1, 4)            # q off by 4 bytes
    with pytest.raises(RuntimeError, match="mmfd_attn_decode.*aligned"):
        K.attn_decode(z(1, 64), flat[2:2 + 256].view(1, 4, 64), z(1, 4, 64), 1, 4)       # k off by 8 bytes


# ---------------------------------------------------------------------------------------------
# lm_head_argmax
# ---------------------------------------------------------------------------------------------
LM_CASES = [(1, 1, 96), (4, 63, 96), (20, 200, 96), (4, 30524, 768)]


def _planted(B, V, K_, dtype, slab):
    """x with orthogonal rows and W with one planted winner per batch row: W[w_b] = C * sum of the unit rows
    planted there, so row b's logit at w_b is C |x_b| and (x being orthogonal) 0 for the rows planted
    elsewhere; every other vocabulary row is small noise. Winners cycle over the first row, the last row
    and the two rows around the kernel's first slab boundary."""
    x = torch.linalg.qr(_rand(K_, B, seed=11).double())[0].t().contiguous() * 4.0  # B <= K orthogonal rows, norm 4
    W = _rand(V, K_, seed=12, scale=0.05).double()
    cand = sorted({c for c in (0, V - 1, slab - 1, slab) if 0 <= c < V})
    win = [cand[b % len(cand)] for b in range(B)]
    xr = x.to(dtype).double()
    for c in set(win):
        W[c] = 2.0 * sum(xr[b] / xr[b].norm() for b in range(B) if win[b] == c)
    bias = _rand(V, seed=13, scale=0.1)
    return x.to(dtype), W.to(dtype), bias, win


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,V,Kd", LM_CASES)
def test_lm_head_argmax_logits_and_planted_winners(B, V, Kd, dtype):
    from mmfd import kernels as K
    slab = K.lm_head_slab(dtype, B, V, Kd)
    x, W, bias, win = _planted(B, V, Kd, dtype, slab)
    ref = x.double() @ W.double().t() + bias.double()
    bound32 = 3e-5 + 3e-5 * ref.abs().max().item()
    if V > 1:  # the planted winner leads the runner-up by >= 100 x the fp32 bound: constructed, checked here
        top2 = ref.topk(2, dim=-1)
        assert (top2.indices[:, 0] == torch.tensor(win)).all()
        assert (top2.values[:, 0] - top2.values[:, 1]).min().item() >= 100 * bound32
    logits = torch.full((B, V + 3), 7.0, device=DEV)
    idx = K.lm_head_argmax(x.to(DEV), W.to(DEV), bias.to(DEV), logits=logits[:, :V])
    idx2 = K.lm_head_argmax(x.to(DEV), W.to(DEV), bias.to(DEV))  # without the logits output
    torch.cuda.synchronize()
    err = (logits[:, :V].double().cpu() - ref).abs().max().item()
    print(f"lm_head {(B, V, Kd)} {dtype}: slab {slab}, logits err {err:.3e} (bound {_bound(dtype, ref):.3e}), winners {win}")
    assert err <= _bound(dtype, ref)
    assert (logits[:, V:] == 7.0).all()
    assert idx.dtype == torch.int64 and idx.cpu().tolist() == win and idx2.cpu().tolist() == win


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_lm_head_argmax_ties_and_nan(dtype):
    """bit-identical rows of W with equal bias tie exactly: the lowest index wins, at two positions (batch
    row 0) and at three (batch row 1), across slabs; a NaN logit beside the winner is never chosen"""
    from mmfd import kernels as K
    B, V, Kd = 4, 200, 96
    slab = K.lm_head_slab(dtype, B, V, Kd)
    assert 0 < slab < 100
    x, W, bias, _ = _planted(B, V, Kd, dtype, slab)
    W = W.double()
    W[[0, V - 1, slab - 1, slab]] = _rand(4, Kd, seed=14, scale=0.05).double()  # the planted winners go
    xr = x.double()
    pair, triple = (slab + 3, V - 2), (5, slab + 1, 3 * slab + 2)
    for rows, b in ((pair, 0), (triple, 1)):
        W[list(rows)] = 2.0 * xr[b] / xr[b].norm()
        bias[list(rows)] = 0.25
    W[7] = 2.0 * xr[2] / xr[2].norm()       # row 2: a plain winner with a NaN row next to it
    W[8] = float("nan")
    W[150] = 2.0 * xr[3] / xr[3].norm()
    W = W.to(dtype)
    ref = x.double() @ W.double().t() + bias.double()
    assert torch.isnan(ref[:, 8]).all() and torch.equal(W[pair[0]], W[pair[1]]) and torch.equal(W[triple[0]], W[triple[2]])
    assert ref.nan_to_num(nan=-math.inf).argmax(-1).tolist()[2:] == [7, 150]
    idx = K.lm_head_argmax(x.to(DEV), W.to(DEV), bias.to(DEV))
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == [min(pair), min(triple), 7, 150]
    # nothing but NaN: a valid token all the same
    idx = K.lm_head_argmax(x.to(DEV), torch.full_like(W, float("nan")).to(DEV), bias.to(DEV))
    assert idx.cpu().tolist() == [0, 0, 0, 0]


def test_lm_head_argmax_refuses_bad_arguments():
    from mmfd import kernels as K
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="mmfd_lm_head_argmax"):
        K.lm_head_argmax(z(33, 96), z(10, 96))      # more than 32 rows
    with pytest.raises(RuntimeError, match="mmfd_lm_head_argmax"):
        K.lm_head_argmax(z(2, 98), z(10, 98))       # K * 4 bytes is no multiple of 16


# ---------------------------------------------------------------------------------------------
# greedy_select
# ---------------------------------------------------------------------------------------------
def test_greedy_select_rule():
    from mmfd import kernels as K
    am = torch.tensor([5, 2, 7, 9], device=DEV)
    fin = torch.tensor([0, 0, 1, 0], dtype=torch.int32, device=DEV)
    seq = torch.full((3, 4), -1, dtype=torch.int64, device=DEV)       # step-major, as mmfd.blip keeps it
    K.greedy_select(am, fin, 2, 0, seq[1])
    assert seq.cpu().tolist() == [[-1] * 4, [5, 2, 0, 9], [-1] * 4]  # eos as produced, pad for the finished row
    assert fin.cpu().tolist() == [0, 1, 1, 0]                         # eos marks its row at this step
    forced = torch.tensor([[1, 9], [1, 9], [1, 9], [2, 9]], device=DEV)
    K.greedy_select(am, fin, 2, 0, seq[2], forced=forced[:, 0])       # a forced token overrides (strided view)
    assert seq[2].cpu().tolist() == [1, 1, 1, 2] and fin.cpu().tolist() == [0, 1, 1, 1]
    col = torch.full((4, 3), -1, dtype=torch.int64, device=DEV)       # batch-major output column
    K.greedy_select(am, fin, 2, 0, col[:, 1])
    assert col.cpu().tolist() == [[-1, 5, -1], [-1, 0, -1], [-1, 0, -1], [-1, 0, -1]]


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    z, cfg, W = R.load_fixture()
    return dict(z=z, cfg=cfg, W=W, seq=torch.from_numpy(z["sequences"]), px=torch.from_numpy(z["pixel_values"]))


def _model(fx, precision="fp32"):
    return R.load_model(fx["cfg"], fx["W"], precision, DEV)


@pytest.fixture(scope="module")
def bert_error():
    """|delta|max / max(1, |ref|max) of mmfd's BertModel on bert_small.npz, per precision: existing code, the
    yardstick of the logits bar"""
    from mmfd.encoders import BertConfig, BertModel
    z = np.load(os.path.join(R.G, "bert_small.npz"), allow_pickle=False)
    m = BertModel(BertConfig(**json.loads(str(z["config"]))))
    m.load_state_dict({k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")})
    m = m.to(DEV).eval()
    out = {}
    for prec in ("fp32", "bf16"):
        with torch.no_grad():
            y = m.set_precision(prec)(input_ids=torch.from_numpy(z["input_ids"]).to(DEV),
                                      attention_mask=torch.from_numpy(z["attention_mask"]).to(DEV),
                                      token_type_ids=torch.from_numpy(z["token_type_ids"]).to(DEV)).last_hidden_state
        ref = torch.from_numpy(z["out"]).double()
        out[prec] = (y.double().cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        print(f"BertModel on bert_small.npz, {prec}: relative error {out[prec]:.3e}")
    return out


def test_loading_names_and_tied_decoder(fx):
    from mmfd.blip import BlipConfig, BlipForConditionalGeneration
    m = BlipForConditionalGeneration(BlipConfig(vision=fx["cfg"]["vision"], text=fx["cfg"]["text"]))
    assert list(m.state_dict().keys()) == [str(k) for k in fx["z"]["keys"]]
    m.load_state_dict(fx["W"], strict=True)
    pr = m.text_decoder.cls.predictions
    assert pr.decoder.weight is m.text_decoder.bert.embeddings.word_embeddings.weight and pr.decoder.bias is pr.bias
    with pytest.raises(RuntimeError, match=r"call \.to\('cuda'\) first"):
        m.generate(fx["px"])
    m = m.to(DEV)
    assert pr.decoder.weight.data_ptr() == m.text_decoder.bert.embeddings.word_embeddings.weight.data_ptr()
    with pytest.raises(NotImplementedError, match="inference-only"):  # parameters still require grad
        m(fx["px"], fx["seq"][:, :3])
    d = BlipConfig()  # the defaults are blip-image-captioning-large
    assert (d.vision.hidden_size, d.vision.num_hidden_layers, d.vision.image_size, d.vision.patch_size) == (1024, 24, 384, 16)
    assert (d.text.vocab_size, d.text.hidden_size, d.text.num_hidden_layers, d.text.bos_token_id,
            d.text.sep_token_id, d.text.pad_token_id, d.text.encoder_hidden_size) == (30524, 768, 12, 30522, 102, 0, 1024)


def test_image_embeds_match_transformers(fx):
    m = _model(fx)
    emb = m.image_embeds(fx["px"])
    err = (emb.double().cpu() - torch.from_numpy(fx["z"]["image_embeds"]).double()).abs().max().item()
    print(f"image_embeds fp32: err {err:.3e}")
    assert tuple(emb.shape) == (4, 101, 64) and err <= 1e-4


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_logits_match_the_fixture(fx, bert_error, precision):
    """Teacher-forced logits on the fixture's sequences against the stored ones, relative error
    |delta|max / max(1, |ref|max) within 2 x BertModel's on bert_small.npz (floor 1e-4 in fp32).

    Measured on an MI355X when this test was written (single run): fp32 |delta|max 3.379e-06, relative
    4.582e-07 (bar 1e-4; BertModel 2.044e-07); bf16 |delta|max 7.455e-02, relative 1.011e-02 against a bar of
    1.775e-02 (BertModel 8.876e-03). The float64 restatement with only its GEMM operands / outputs and
    LayerNorm outputs rounded to bf16 (no kernel involved) lies 0.007 from the fixture: the distance is the
    bf16 storage, and it is what decided the fixture's recipe (tests/golden/make_blip_small.py)."""
    m = _model(fx, precision)
    logits = m.forward_logits(fx["px"], fx["seq"][:, :20])
    ref = torch.from_numpy(fx["z"]["logits"]).double()
    err = (logits.double().cpu() - ref).abs().max().item()
    rel = err / max(1.0, ref.abs().max().item())
    bar = max(2.0 * bert_error[precision], 1e-4 if precision == "fp32" else 0.0)
    print(f"forward_logits {precision}: |delta|max {err:.3e}, relative {rel:.3e}, bar {bar:.3e}")
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (20, 4, 200)
    assert rel <= bar


def _valid_structure(ids, tc, n_prompt=1):
    ids = ids.tolist()
    for r in ids:
        assert all(0 <= t < tc["vocab_size"] for t in r) and r[0] == tc["bos_token_id"]
        gen = r[n_prompt:]
        if tc["sep_token_id"] in gen:
            assert all(t == tc["pad_token_id"] for t in gen[gen.index(tc["sep_token_id"]) + 1:])
    # the array ends where the last row stopped
    n = max((r[n_prompt:].index(tc["sep_token_id"]) + 1) if tc["sep_token_id"] in r[n_prompt:] else len(r) - n_prompt
            for r in ids)
    assert len(ids[0]) == n_prompt + n


def test_greedy_fp32_reproduces_transformers_ids(fx):
    m = _model(fx)
    live = torch.from_numpy(R.live_mask(fx["z"]["sequences"], fx["cfg"]["text"]["sep_token_id"]))
    logits = m.forward_logits(fx["px"], fx["seq"][:, :20])
    err = (logits.double().cpu() - torch.from_numpy(fx["z"]["logits"]).double()).abs()[live].max().item()
    margin = float(fx["z"]["margin"])
    print(f"greedy fp32: live logit error {err:.3e}, stored margin {margin:.4f}")
    assert err <= margin / 4
    out = m.generate(fx["px"], use_graph=False)
    assert out.dtype == torch.int64 and torch.equal(out, fx["seq"])  # all 4 rows, pads included


def test_greedy_bf16_structure(fx):
    m = _model(fx, "bf16")
    out = m.generate(fx["px"], use_graph=False)
    assert out.shape[0] == 4 and 2 <= out.shape[1] <= 21
    _valid_structure(out, fx["cfg"]["text"])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_matches_eager_and_refreshes(fx, precision):
    m = _model(fx, precision)
    tc = fx["cfg"]["text"]
    eager = m.generate(fx["px"], use_graph=False)
    graph = m.generate(fx["px"], use_graph=True)
    assert torch.equal(graph, eager)
    perm = torch.tensor([2, 0, 3, 1])
    again = m.generate(fx["px"][perm], use_graph=True)  # a replay on refreshed static buffers
    assert torch.equal(again, eager[perm])
    # new weights: every logit but one far below -> the graph is captured again and follows them
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["text_decoder.cls.predictions.bias"][7] += 100.0
    sd["text_decoder.cls.predictions.decoder.bias"] = sd["text_decoder.cls.predictions.bias"]
    m.load_state_dict(sd, strict=True)
    out = m.generate(fx["px"], use_graph=True)
    assert torch.equal(out, torch.tensor([[tc["bos_token_id"]] + [7] * 20] * 4))
    assert torch.equal(out, m.generate(fx["px"], use_graph=False))


def test_prompt_continues_a_stored_row(fx):
    m = _model(fx)
    seq, tc = fx["seq"], fx["cfg"]["text"]
    row = int((seq[:, 1:] != tc["pad_token_id"]).sum(1).argmax())
    for use_graph in (False, True):
        out = m.generate(fx["px"], input_ids=seq[row, :3], max_new_tokens=18, use_graph=use_graph)
        assert torch.equal(out[row], seq[row])
        assert (out[:, :3] == seq[row, :3]).all()


def test_captioner_decodes_without_special_tokens(fx):
    from mmfd.caption import Captioner
    from tests.toy_tokenizer import toy_tokenizer
    cap = Captioner(_model(fx), tokenizer=toy_tokenizer())
    ids = cap.generate_ids(fx["px"])
    assert torch.equal(ids, fx["seq"])
    texts = cap.caption(fx["px"])
    assert len(texts) == 4 and all(isinstance(t, str) for t in texts)
    assert not any(s in t for t in texts for s in ("[PAD]", "[CLS]", "[SEP]", "[UNK]", "[MASK]"))
    assert any(t for t in texts)
