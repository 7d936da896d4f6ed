"""The attention reference tests' own footing, checked without a GPU (the built library is needed for
mmfd_debug_attn_plan, as in tests/test_attn_plan_cpu.py):

1. tests/attention_refs.py agrees with independent code: torch's scaled_dot_product_attention and its
   autograd in float64 where SDPA can express the call, a second plain formulation with hand-derived
   gradients for dropout, F.normalize for the cosine form. 1e-12 relative.
2. The GPU test's bounds are attainable on its inputs: a CPU emulation of a bf16 kernel (inputs, P, dS
   and outputs rounded to bf16, the rest fp32) and a plain fp32 emulation stay within HALF the bound on
   every input kind. The half is a condition on the inputs, not a measurement.
3. The case table of tests/attn_cases.py reaches every kernel of the attention unit, each with the
   options it can take."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import attn_cases as C
from tests import attention_refs as R

RTOL = 1e-12
OUTS = ("o", "lse", "dq", "dk", "dv")


def _rel_close(got, want, what):
    err = (got - want).abs().max().item()
    assert err <= RTOL * max(want.abs().max().item(), 1.0), (what, err)


def _inputs(B, H, Lq, Lk, D, seed, rel=None, mask=False):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x = dict(q=rn(B, Lq, H * D), k=rn(B, Lk, H * D), v=rn(B, Lk, H * D), dout=rn(B, Lq, H * D), key_bias=None, rel_bias=None)
    if mask:
        lens = torch.tensor([Lk - 3, 5, Lk, 1][:B])
        x["key_bias"] = torch.where(torch.arange(Lk)[None] < lens[:, None], 0.0, -10000.0)
    if rel:
        x["rel_bias"] = rn(*{"shared": (), "batch": (B,), "mod": (2,)}[rel], H, Lq, Lk)
    return x


def _sdpa(x, H, scale, qh=None, kh=None):
    """SDPA on float64 leaves; the additive mask carries key_bias + rel_bias and is a leaf itself"""
    B = x["q"].shape[0]
    q, k, v = (x[n].clone().requires_grad_(True) for n in "qkv")
    m = torch.zeros(B, H, x["q"].shape[1], x["k"].shape[1], dtype=torch.float64)
    if x["key_bias"] is not None:
        m = m + x["key_bias"].double()[:, None, None, :]
    rb = None
    if x["rel_bias"] is not None:
        rb = x["rel_bias"].clone().requires_grad_(True)
        m = m + R.batch_rel_bias(rb, B)
    qq, kk = R.to_heads(q, H), R.to_heads(k, H)
    if qh is not None:
        qq, kk = qh(qq), kh(kk)
    o = R.from_heads(F.scaled_dot_product_attention(qq, kk, R.to_heads(v, H), attn_mask=m, scale=scale))
    o.backward(x["dout"])
    return o.detach(), q.grad, k.grad, v.grad, (rb.grad if rb is not None else None)


@pytest.mark.parametrize("rel", [None, "shared", "batch", "mod"])
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("shape", [(4, 3, 13, 29, 16), (2, 3, 70, 100, 32), (2, 2, 257, 40, 8)])
def test_reference_matches_sdpa(shape, mask, rel):
    B, H, Lq, Lk, D = shape
    x = _inputs(B, H, Lq, Lk, D, 11, rel, mask)
    scale = 0.37
    ref = R.attention_ref(x["q"], x["k"], x["v"], H, scale, key_bias=x["key_bias"], rel_bias=x["rel_bias"],
                          dout=x["dout"], want_d_rel_bias=rel is not None)
    o, dq, dk, dv, drb = _sdpa(x, H, scale)
    for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        _rel_close(ref[name], t, name)
    if rel:
        assert ref["d_rel_bias"].shape == x["rel_bias"].shape
        _rel_close(ref["d_rel_bias"], drb, "d_rel_bias")
    s = R.logits(x["q"], x["k"], H, scale, x["key_bias"], x["rel_bias"])
    m = s.max(-1, keepdim=True).values
    _rel_close(ref["lse"], (m + (s - m).exp().sum(-1, keepdim=True).log()).squeeze(-1), "lse")


def test_reference_batch_modulus_reads_row_b_mod_m():
    B, H, Lq, Lk, D = 4, 3, 13, 29, 16
    x = _inputs(B, H, Lq, Lk, D, 12, "mod")
    a = R.attention_ref(x["q"], x["k"], x["v"], H, 0.25, rel_bias=x["rel_bias"])
    rows = torch.stack([x["rel_bias"][b % 2] for b in range(B)])
    b = R.attention_ref(x["q"], x["k"], x["v"], H, 0.25, rel_bias=rows)
    assert torch.equal(a["o"], b["o"]) and torch.equal(a["lse"], b["lse"])
    assert not torch.equal(rows[0], rows[1])


@pytest.mark.parametrize("mask", [False, True])
def test_reference_dropout_matches_hand_derived_gradients(mask):
    """a second plain formulation: per-head loops, the softmax and every gradient written out"""
    B, H, Lq, Lk, D, p, scale = 2, 3, 24, 70, 16, 0.1, 0.3
    x = _inputs(B, H, Lq, Lk, D, 13, "batch", mask)
    keep = C.attn_keep_mask(5, 9, (B, H, Lq, Lk), p)
    assert 0.8 < keep.mean() < 0.97
    ref = R.attention_ref(x["q"], x["k"], x["v"], H, scale, key_bias=x["key_bias"], rel_bias=x["rel_bias"],
                          keep=keep, p=p, dout=x["dout"], want_d_rel_bias=True)
    kt = torch.from_numpy(keep).double()
    out = {n: torch.zeros_like(x[m]) for n, m in (("o", "q"), ("dq", "q"), ("dk", "k"), ("dv", "k"))}
    ds_all = torch.zeros(B, H, Lq, Lk, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            c = slice(h * D, (h + 1) * D)
            q, k, v, do = x["q"][b, :, c], x["k"][b, :, c], x["v"][b, :, c], x["dout"][b, :, c]
            s = scale * q @ k.T + x["rel_bias"][b, h]
            if mask:
                s = s + x["key_bias"][b][None, :]
            e = (s - s.max(1, keepdim=True).values).exp()
            P = e / e.sum(1, keepdim=True)
            Pd = P * kt[b, h] / (1 - p)
            out["o"][b, :, c] = Pd @ v
            out["dv"][b, :, c] = Pd.T @ do
            dP = (do @ v.T) * kt[b, h] / (1 - p)
            dS = P * (dP - (dP * P).sum(1, keepdim=True))
            ds_all[b, h] = dS
            out["dq"][b, :, c] = scale * dS @ k
            out["dk"][b, :, c] = scale * dS.T @ q
    for n, t in out.items():
        _rel_close(ref[n], t, n)
    _rel_close(ref["d_rel_bias"], ds_all, "d_rel_bias")


def test_reference_cosine_matches_normalize():
    B, H, Lq, Lk, D = 2, 4, 13, 29, 16
    x = _inputs(B, H, Lq, Lk, D, 14, "shared")
    x["k"][0, 3] = 0.0  # a zero key row: F.normalize's eps decides
    ls = torch.tensor(C.COS_LOGIT_SCALES)
    mult = torch.tensor([ls_.exp().item() if ls_ < C.COS_MAX_LOG else 100.0 for ls_ in ls.double()], dtype=torch.float64)
    assert mult[2] == 100.0 and mult[3] < 1.0  # the clamp is active on one head, a negative scale on another
    ref = R.attention_ref(x["q"], x["k"], x["v"], H, 1.0, rel_bias=x["rel_bias"], cos_logit_scale=ls,
                          cos_max_log=C.COS_MAX_LOG, dout=x["dout"])
    o, dq, dk, dv, _ = _sdpa(x, H, 1.0, qh=lambda t: F.normalize(t, dim=-1) * mult[None, :, None, None],
                             kh=lambda t: F.normalize(t, dim=-1))
    for name, t in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
        _rel_close(ref[name], t, name)
    s = R.logits(x["q"], x["k"], H, 1.0, None, None, ls, C.COS_MAX_LOG)
    assert s[:, 2].abs().max().item() <= 100.0 * (1 + 1e-12) and s[:, 2].abs().max().item() > 50.0


# ------------------------------------------------------------------------------------------------------
# 2. attainability
# ------------------------------------------------------------------------------------------------------
EMU_SHAPES = ((13, 29, 16), (70, 100, 32), (256, 256, 64), (24, 257, 48), (257, 40, 8))
EMU_KINDS = {"randn": ("plain", "drop", "drop_mask"), "ramp0.1": ("plain", "drop", "drop_mask"),
             "ramp0.4": ("plain", "drop", "drop_mask"), "lead_mask": ("mask", "drop_mask")}


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("kind", list(EMU_KINDS))
@pytest.mark.parametrize("shape", EMU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bounds_are_attainable_on_the_table_inputs(shape, kind, dtype):
    """measured when written: worst ratio 0.48 in bf16, 0.034 in fp32"""
    Lq, Lk, D = shape
    worst = {}
    for feature in EMU_KINDS[kind]:
        s = C.Spec(dtype, None, 2, 3, Lq, Lk, D, feature, kind)
        x = C.make_inputs(s)
        ref = C.reference(s, x)
        emu = R.emulated_attention(x["q"], x["k"], x["v"], x["dout"], s.H, x["scale"], key_bias=x["key_bias"],
                                   keep=x["keep"], p=x["p"], bf16=dtype == "bf16")
        for n in OUTS:
            worst[(feature, n)] = R.worst_ratio(n, emu[n], ref[n], s.H, dtype)[0]
    bad = {k: round(v, 3) for k, v in worst.items() if not v <= 0.5}
    print(f"{dtype} {shape} {kind}: worst {max(worst.values()):.3f}")
    assert not bad, bad


@pytest.mark.parametrize("shape", [(13, 29, 16), (70, 100, 32), (256, 256, 64)], ids=lambda s: "x".join(map(str, s)))
def test_cosine_bounds_are_attainable_with_unrounded_norms(shape):
    """a bf16 kernel that multiplies the raw q.k products by the fp32 norms and logit scale stays within
    half the bound at the clamp (x 100); rounding the normalised operands to bf16 first (printed, not
    asserted) costs up to 100 * 2^-8 in a logit and misses it"""
    Lq, Lk, D = shape
    s = C.Spec("bf16", None, 2, 3, Lq, Lk, D, "cos", "randn")
    x = C.make_inputs(s)
    ref = C.reference(s, x)
    ratio = {}
    for rounded in (False, True):
        emu = R.emulated_cosine_forward(x["q"], x["k"], x["v"], s.H, x["rel_bias"], x["cos_logit_scale"], x["cos_max_log"],
                                        round_normalised=rounded)
        ratio[rounded] = {n: round(R.worst_ratio(n, emu[n], ref[n], s.H, "bf16")[0], 3) for n in ("o", "lse")}
    print(f"cos {shape}: unrounded norms {ratio[False]}, normalised operands rounded to bf16 {ratio[True]}")
    assert max(ratio[False].values()) <= 0.5, ratio


def test_ramp_inputs_raise_the_running_maximum():
    """the logits of a ramp case rise by `slope` log2 units per key on average, so the maximum over the
    first j keys keeps growing: by less than the lazy-rescale threshold (8) per 32-key chunk at 0.1, by
    more at 0.4"""
    for kind, slope in C.RAMP_SLOPES.items():
        s = C.Spec("bf16", None, 2, 3, 70, 100, 64, "plain", kind)
        x = C.make_inputs(s)
        lg = R.logits(x["q"].double(), x["k"].double(), s.H, x["scale"]) * 1.4426950408889634
        per_key = (lg[..., -1] - lg[..., 0]).mean().item() / (s.Lk - 1)
        assert abs(per_key - slope) < 0.15 * slope, (kind, per_key)
        step = (lg[..., 64:96].amax(-1) - lg[..., 32:64].amax(-1)).median().item()  # chunk to chunk
        assert (step > 8.0) == (slope == 0.4), (kind, step)


def test_lead_mask_inputs_are_no_prefix_masks():
    x = C.make_inputs(C.Spec("f32", "split", 2, 3, 70, 100, 32, "mask", "lead_mask"))
    live = x["key_bias"] == 0
    assert not live[0, :53].any() and live[0, 53:].all()  # 100 // 2 + 3 leading keys masked
    assert live[1, :5].all() and not live[1, 5:].any()


# ------------------------------------------------------------------------------------------------------
# 3. coverage
# ------------------------------------------------------------------------------------------------------
PLAN_ENV = ("MMFD_ATTN_V1", "MMFD_ATTN_V2_GENERIC", "MMFD_FP32_ATTN", "MMFD_FP32_GEMM")


def _all_kernels():
    """the attention unit's kernels as tests/test_attn_plan_cpu.py lists them, without mmfd_split3"""
    want = {"dm_fill_kernel"}
    for t in ("float", "bf16"):
        for d in (32, 64):
            want |= {f"attn_{k}_kernel<{t},{d}>" for k in ("fwd", "delta", "bwd_dkdv", "bwd_dq", "bwd_ds")}
            want |= {f"attn_fwd_v2_kernel<{t},{d},{h},{r},{m}>" for h, r, m in
                     ((1, 0, 0), (1, 0, 1), (1, 0, 2), (1, 1, 0), (2, 0, 0), (2, 1, 0), (4, 0, 0), (4, 1, 0))}
            nth = 512 if t == "float" else 256
            for r, m in ((0, 0), (0, 1), (0, 2), (1, 0)):
                want |= {f"attn_dq_v2_kernel<{t},{d},{r},{m}>", f"attn_dkdv_v2_kernel<{t},{d},{nth},{r},{m}>"}
    for d in (32, 64):
        want |= {f"attn_fwd_x6_kernel<{d},{x}>" for x in (0, 1)}
        want |= {f"attn_{k}_x6_kernel<{d},{x}>" for k in ("dq", "dkdv") for x in (0, 1, 2)}
    assert len(want) == 101
    return want


@pytest.fixture(scope="module")
def reached():
    set_ = [v for v in PLAN_ENV if os.environ.get(v) is not None]
    if set_:
        pytest.skip(f"{', '.join(set_)} set in the environment: it changes the launch plans at load time")
    by = {}
    for s in C.table():
        for bwd, a in C.plan_args(s):
            for line in C.plan_lines(a, bwd, s.mode)[1:]:
                if not line.startswith("mmfd_split3"):
                    by.setdefault(line.split(" ")[0], []).append((s, bool(a.drop_mask)))
    return by


def _targs(name):
    return re.search(r"<(.*)>", name).group(1).split(",") if "<" in name else []


def _is_rel(name):
    a = _targs(name)
    return "_v2_kernel" in name and a[-2] == "1"


def _mode(name):
    return int(_targs(name)[-1])


def test_table_reaches_every_kernel(reached):
    want = _all_kernels()
    assert set(reached) == want, (sorted(want - set(reached)), sorted(set(reached) - want))
    ids = [C.spec_id(s) for s in C.table()]
    assert len(set(ids)) == len(ids)
    print(f"{len(ids)} cases; fewest cases on one kernel: {min(len(v) for v in reached.values())}")


def test_table_reaches_every_kernel_with_its_options(reached):
    """forward kernels other than the relative-bias and the plain fixed-mode ones: a key mask;
    relative-bias kernels: a bias of each form; streaming and resident mode-0 backward: hashed and
    keep-bitmask dropout (a resident call with hashed dropout and no relative bias is planned on mode 2,
    so the bias-free mode-0 kernels take only the bitmask); resident forwards with several heads per
    workgroup: a B*H that the count does not divide. Accumulate: the GPU test runs every backward case
    with each accumulate flag, so reaching a backward kernel at all is reaching it with accumulate."""
    feat = C.FEATURES
    missing = []

    def need(name, what, ok):
        if not any(ok(s, bits) for s, bits in reached[name]):
            missing.append((name, what))

    for name in reached:
        fwd = name.startswith("attn_fwd")
        v2 = "_v2_kernel" in name
        stream_bwd = name.startswith(("attn_bwd_dkdv_kernel", "attn_bwd_dq_kernel"))
        if fwd and not (v2 and (_is_rel(name) or _mode(name) == 1)):
            need(name, "key mask", lambda s, b: feat[s.feature].mask)
        if _is_rel(name):
            for form in ("shared", "batch", "mod"):
                need(name, "rel_bias " + form, lambda s, b, form=form: feat[s.feature].rel == form)
        if stream_bwd or (v2 and not fwd and _mode(name) == 0):
            need(name, "keep-bitmask dropout", lambda s, b: b)
            if stream_bwd or _is_rel(name):
                need(name, "hashed dropout", lambda s, b: feat[s.feature].p > 0 and not b)
        if v2 and fwd and int(_targs(name)[2]) > 1:
            hpb = int(_targs(name)[2])
            need(name, f"B*H % {hpb} != 0", lambda s, b, hpb=hpb: (s.B * s.H) % hpb != 0)
        if not fwd and name not in ("dm_fill_kernel",):
            need(name, "backward case", lambda s, b: not feat[s.feature].cos)
    assert not missing, missing


def test_table_modulus_bias_cases_have_more_batch_rows_than_the_modulus():
    """at B = RB_MOD an [RB_MOD, H, Lq, Lk] bias is the per-batch form and `b % rb_mod` is never taken
    (found by the mutation that replaces it by 0)"""
    mod = [s for s in C.table() if C.FEATURES[s.feature].rel == "mod"]
    assert mod and all(s.B == 2 * C.RB_MOD for s in mod)
    x = C.make_inputs(mod[0])
    assert x["rel_bias"].shape[0] == C.RB_MOD and not torch.equal(x["rel_bias"][0], x["rel_bias"][1])


def test_table_ramps_reach_every_resident_bf16_forward(reached):
    names = [n for n in reached if n.startswith("attn_fwd_v2_kernel<bf16")]
    assert len(names) == 16
    missing = [(n, kind) for n in names for kind in C.RAMP_SLOPES if not any(s.kind == kind for s, _ in reached[n])]
    assert not missing, missing


def test_table_loses_no_kernel_of_the_full_product(reached):
    """the table is trimmed from the nine shapes x four head dims x ten features; the trimming may
    not lose a (kernel, feature) pair whose feature carries an option the kernel implements itself
    (mask, dropout form, bias form, bias gradient)"""
    full = set()
    for s in C.full_product():
        for k in C.kernels_of(s):
            full.add((k, s.feature))
    have = {(k, s.feature) for k, v in reached.items() for s, _ in v}
    lost = sorted(p for p in full - have if p[1] not in ("drop", "bits_mask", "relb_mask"))
    # dropout without a mask, the bitmask with one and the per-batch bias without its gradient run at
    # alternating head dims / fewer shapes: their options are each covered by drop_mask, bits and drel
    assert not lost, lost
    assert len(C.table()) < len(C.full_product())
