"""Which attention kernels a call launches, pinned without a GPU: mmfd_debug_attn_plan (a host-only
export of csrc/attention.hip, not part of include/mmfd.h) must reproduce, for every case of
tests/golden/attn_plans.json, the launches recorded from the commit before the launch plan existed —
kernel instantiation, grid, block, dynamic LDS bytes, host-set AttnP flags, follow-up launches — and
refuse what that commit refused, with the same message.

A case is {"c": [bwd, dtype, B, H, Lq, Lk, D], "o": {options of attn_args below}, "plan": [lines]},
with "rc" and "error" when the call is refused."""
import ctypes
import json
import os

import pytest

from mmfd import kernels as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plans.json")
FAMILY_OF = (("_x6_kernel", "split"), ("_v2_kernel", "resident"), ("_kernel", "stream"))
# dummy 16-B-aligned addresses: a plan never dereferences them
PTR = {n: (i + 1) << 20 for i, n in enumerate(
    ("q", "k", "v", "o", "lse", "key_bias", "rel_bias", "seed", "dout", "dq", "dk", "dv", "delta", "d_rel_bias",
     "cos_logit_scale", "dqkv_planes", "o_planes", "drop_mask"))}


def attn_args(bwd, dtype, B, H, Lq, Lk, D, *, mode="split", generic=0, key_bias=0, rel_bias=0, p=0.0, drop_mask=0,
              d_rel_bias=0, cos=0, o_planes=0, dqkv_planes=0, planes_only=0, acc=0, planes_off=0, dq_off=0, rb_mod=0):
    """q, k, v, o, dout and the gradients as separate contiguous [B, L, H*D] buffers; rel_bias "shared" =
    one [H][Lq][Lk] bias, else per batch row (or per rb_mod rows); dqkv_planes packs dq | dk | dv in one
    [B, L, 3*H*D] buffer; planes_off / dq_off move those pointers off their alignment. `mode` (fp32
    attention: split / native) and `generic` are library switches, not fields."""
    W = H * D
    a = K.AttnArgs()
    a.dtype = {"f32": K.F32, "bf16": K.BF16}.get(dtype, 7)
    a.B, a.H, a.Lq, a.Lk, a.D, a.scale, a.salt = B, H, Lq, Lk, D, 0.125, 7
    for t, L in (("q", Lq), ("k", Lk), ("v", Lk), ("o", Lq)):
        setattr(a, t, PTR[t]), setattr(a, t + "_sb", L * W), setattr(a, t + "_st", W)
    a.lse = PTR["lse"]
    if key_bias:
        a.key_bias = PTR["key_bias"]
    if rel_bias:
        a.rel_bias, a.rel_bias_sb, a.rel_bias_mod = PTR["rel_bias"], 0 if rel_bias == "shared" else H * Lq * Lk, rb_mod
    if p > 0:
        a.dropout_p, a.seed = p, PTR["seed"]
    if drop_mask:
        a.drop_mask = PTR["drop_mask"]
    if cos:
        a.cos_logit_scale, a.cos_max_log = PTR["cos_logit_scale"], 4.6
    if o_planes:
        a.o_planes = PTR["o_planes"] + planes_off
    if bwd:
        a.dout, a.do_sb, a.do_st, a.delta = PTR["dout"], Lq * W, W, PTR["delta"]
        a.accumulate_dq = a.accumulate_dkv = acc
        a.dq, a.dq_sb, a.dq_st = PTR["dq"] + dq_off, Lq * W, W
        a.dk, a.dk_sb, a.dk_st = PTR["dk"], Lk * W, W
        a.dv, a.dv_sb, a.dv_st = PTR["dv"], Lk * W, W
        if dqkv_planes:
            a.dk, a.dv = a.dq + 4 * W, a.dq + 8 * W
            a.dq_st = a.dk_st = a.dv_st = 3 * W
            a.dq_sb = a.dk_sb = a.dv_sb = Lq * 3 * W
            a.dqkv_planes, a.planes_only = PTR["dqkv_planes"] + planes_off, planes_only
        if d_rel_bias:
            a.d_rel_bias = PTR["d_rel_bias"]
    return a


@pytest.fixture(scope="module")
def plan():
    lib = K.load()
    fn = lib.mmfd_debug_attn_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(K.AttnArgs), ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]
    buf = ctypes.create_string_buffer(4096)

    def run(case):
        a = attn_args(*case["c"], **case["o"])
        old_mode = lib.mmfd_set_fp32_attn_mode(0 if case["o"].get("mode") == "native" else 1)
        old_generic = lib.mmfd_debug_set_attn_v2_generic(case["o"].get("generic", 0))
        try:
            rc = fn(ctypes.byref(a), case["c"][0], buf, len(buf))
        finally:
            lib.mmfd_set_fp32_attn_mode(old_mode)
            lib.mmfd_debug_set_attn_v2_generic(old_generic)
        return rc, buf.value.decode().splitlines(), (lib.mmfd_last_error_string().decode() if rc else "")

    return run


def test_plans_match_the_recorded_launches(plan):
    cases = json.load(open(GOLDEN))["cases"]
    assert len(cases) >= 200
    bad = []
    for c in cases:
        got = plan(c)
        lines = list(c["plan"])
        if lines:  # the family line is implied by the first recorded kernel
            first = lines[0].split(" ")[0].split("<")[0]
            lines.insert(0, "family=" + next(fam for suffix, fam in FAMILY_OF if first.endswith(suffix)))
        want = (c.get("rc", 0), lines, c.get("error", ""))
        if got != want:
            bad.append((c["c"], c["o"], got, want))
    assert not bad, f"{len(bad)} of {len(cases)} plans differ; first: {bad[0]}"


def test_golden_covers_every_kernel():
    """the recorded table reaches every one of the 101 kernels of the attention unit and the split3
    follow-up, so no instantiation's routing is left unpinned"""
    cases = json.load(open(GOLDEN))["cases"]
    kernels = {line.split(" ")[0] for c in cases for line in c["plan"]}
    want = {"dm_fill_kernel", "mmfd_split3"}
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
    assert kernels == want, (sorted(want - kernels), sorted(kernels - want))
    assert len(want) == 101 + 1


def test_plan_export_needs_a_buffer(plan):
    lib = K.lib()
    a = K.AttnArgs()
    assert lib.mmfd_debug_attn_plan(ctypes.byref(a), 0, None, 0) == 1000
    assert "no buffer" in lib.mmfd_last_error_string().decode()
