"""Every attention kernel instantiation and option against the float64 reference of
tests/attention_refs.py, over the case table of tests/attn_cases.py (tests/test_attention_ref_cpu.py
proves on the CPU that the table reaches all kernels with their options and that the bounds below are
attainable on its inputs).

Error rule: tests/test_kernels_gpu.py's own numbers, err <= atol + rtol * max|ref| with (3e-5, 3e-5) in
fp32 and (2e-2, 2e-2) in bf16, lse 1e-4 / 2e-2 absolute — evaluated per (batch row, head) slice, so one
wrong head is not diluted by the rest.

Operands are strided views: q, dout and o sit at column 8 of wider buffers, k | v are fused, dq | dk |
dv sit in one [B, L + 64, 3*H*D + 8] buffer; every buffer has 64 rows per batch row beyond the view.
Input columns and rows outside the views are NaN (a read that leaks into a result shows); outputs
are NaN where the kernel must write and a sentinel elsewhere, which must stay bitwise unchanged: a store
from a padded query / key row or the zero-padded head dimension lands inside the buffer and is seen.

Every backward case runs again with accumulate_dq, and again with accumulate_dkv: the accumulated
output starts from small integers and must equal prefill + gradient within the bound on
|prefill + ref|; the other outputs must be bitwise those of the plain call. Keep-bitmask cases run
their hashed twin first: the mask words equal the oracle's on the valid keys and all five outputs are
bitwise the twin's, which is itself compared with the reference.

Cosine cases: the forward scales the fp32 scores of the raw q . k by the norms and the logit scale. It
used to round q / |q| * exp(logit scale) and k / |k| to bf16 before the MFMA, which these cases found:
lse up to 12.7 x its bound, o up to 2.4 x, on the head clamped at log(100)."""
import json
import os

import numpy as np
import pytest
import torch

from mmfd import kernels as K
from tests import attn_cases as C
from tests import attention_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD_ROWS, PAD_COLS = 64, 8
SENTINEL = -3.0
NAN = float("nan")
WORST = {}  # (dtype, output) -> (ratio, case id): the suite-wide worst error / bound


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    lines = {f"{dt} {name}": [round(r, 4), cid] for (dt, name), (r, cid) in sorted(WORST.items())}
    print("\nworst error / bound per dtype and output:", json.dumps(lines, indent=1))
    path = os.environ.get("MMFD_ATTN_RATIO_LOG")
    if path:
        with open(path, "w") as f:
            json.dump(lines, f, indent=1)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class Buf:
    """a [B, L + PAD_ROWS, width] device buffer filled with `fill`, and views [:, :L, c0:c1] into it"""

    def __init__(self, B, L, width, dtype, fill):
        self.t = torch.full((B, L + PAD_ROWS, width), fill, dtype=dtype, device=DEV)
        self.inside = torch.zeros(self.t.shape, dtype=torch.bool)
        self.before = None

    def view(self, L, c0, c1, value=None):
        v = self.t[:, :L, c0:c1]
        if isinstance(value, float):
            v.fill_(value)
        elif value is not None:
            v.copy_(value)
        self.inside[:, :L, c0:c1] = True
        return v

    def freeze(self):
        self.before = self.t.cpu()

    def outside_unchanged(self):
        out = ~self.inside
        return torch.equal(_bits(self.t.cpu())[out], _bits(self.before)[out])


class Call:
    """one case's device operands and its launches"""

    def __init__(self, s, x):
        self.s, self.x, self.f = s, x, C.FEATURES[s.feature]
        B, H, Lq, Lk, D = s.B, s.H, s.Lq, s.Lk, s.D
        self.W = W = H * D
        self.dt = dt = C.torch_dtype(s)
        self.q = Buf(B, Lq, W + PAD_COLS, dt, NAN).view(Lq, PAD_COLS, PAD_COLS + W, x["q"])
        kv = Buf(B, Lk, 2 * W + PAD_COLS, dt, NAN)
        self.k, self.v = kv.view(Lk, 0, W, x["k"]), kv.view(Lk, W, 2 * W, x["v"])
        self.dout = Buf(B, Lq, W + PAD_COLS, dt, NAN).view(Lq, PAD_COLS, PAD_COLS + W, x["dout"])
        dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
        self.kb, self.rb, self.cos = dev(x["key_bias"]), dev(x["rel_bias"]), dev(x["cos_logit_scale"])
        if self.f.rel:  # the library reads the bias in the form the case means
            assert K._rel_bias_args(self.rb, B, H, Lq, Lk)[1:] == {"shared": (0, 0), "batch": (H * Lq * Lk, 0),
                                                                    "mod": (H * Lq * Lk, C.RB_MOD)}[self.f.rel]
        self.seed = K.Seed(C.SEED) if self.f.p > 0 else None
        self.kw = dict(scale=x["scale"], key_bias=self.kb, rel_bias=self.rb, dropout_p=self.f.p, seed=self.seed, salt=C.SALT)
        self.problems = []

    def fwd(self, bits):
        s = self.s
        ob = Buf(s.B, s.Lq, self.W + PAD_COLS, self.dt, SENTINEL)
        o = ob.view(s.Lq, PAD_COLS, PAD_COLS + self.W, NAN)
        ob.freeze()
        dm = K.drop_mask_buffer(s.B, s.H, s.Lq, s.Lk, DEV) if bits else None
        cos = dict(cos_logit_scale=self.cos, cos_max_log=self.x["cos_max_log"]) if self.f.cos else {}
        _, lse = K.attn_fwd(self.q, self.k, self.v, s.H, out=o, drop_mask=dm, **cos, **self.kw)
        torch.cuda.synchronize()
        what = "forward" + (" (bitmask)" if bits else "")
        if not ob.outside_unchanged():
            self.problems.append(f"{what}: a store outside the o view")
        if torch.isnan(o).any() or not torch.isfinite(lse).all():
            self.problems.append(f"{what}: o or lse not written everywhere")
        return dict(o=o, lse=lse, dm=dm)

    def bwd(self, fw, *, acc_dq=None, acc_dkv=None, drel=False, what="backward"):
        """acc_dq / acc_dkv: the prefill(s) the accumulated outputs start from"""
        s, W = self.s, self.W
        gb = Buf(s.B, max(s.Lq, s.Lk), 3 * W + PAD_COLS, self.dt, SENTINEL)
        dq = gb.view(s.Lq, 0, W, NAN if acc_dq is None else acc_dq)
        dk = gb.view(s.Lk, W, 2 * W, NAN if acc_dkv is None else acc_dkv[0])
        dv = gb.view(s.Lk, 2 * W, 3 * W, NAN if acc_dkv is None else acc_dkv[1])
        gb.freeze()
        ds = torch.full((s.B, s.H, s.Lq, s.Lk), NAN, device=DEV) if drel else None
        K.attn_bwd(self.q, self.k, self.v, fw["o"], fw["lse"], self.dout, s.H, dq=dq, dk=dk, dv=dv,
                   accumulate_dq=acc_dq is not None, accumulate_dkv=acc_dkv is not None, drop_mask=fw["dm"],
                   d_rel_bias=ds, **self.kw)
        torch.cuda.synchronize()
        if not gb.outside_unchanged():
            self.problems.append(f"{what}: a store outside the dq | dk | dv views")
        if any(torch.isnan(t).any() for t in (dq, dk, dv)) or (drel and torch.isnan(ds).any()):
            self.problems.append(f"{what}: a gradient not written everywhere")
        out = dict(dq=dq, dk=dk, dv=dv)
        if drel:
            out["d_rel_bias"] = ds
        return out


def _compare(call, got, ref, names, ratios, tag="", base=None):
    s = call.s
    for n in names:
        r, i = R.worst_ratio(n, got[n], ref[n], s.H, s.dtype, base=None if base is None else base[n])
        ratios[tag + n] = round(r, 3)
        if not tag:
            key = (s.dtype, ("cosine " if call.f.cos else "") + n)
            if r > WORST.get(key, (-1.0, ""))[0]:
                WORST[key] = (r, C.spec_id(s))
        if not r <= 1.0:
            call.problems.append(f"{tag}{n}: error {r:.3g} x bound at (batch row, head) = {divmod(i, s.H)}")


def _check_planes(call, ref, ratios):
    """fp32, packed Lq = Lk: the split planes beside o and beside dq | dk | dv equal split3 of the fp32
    result bit for bit; planes_only leaves the fp32 gradient buffer untouched off the streaming family"""
    s, x, W = call.s, call.x, call.W
    B, L = s.B, s.Lq
    qkv = torch.cat([x["q"], x["k"], x["v"]], -1).to(DEV)
    q, k, v = qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:]
    do = x["dout"].to(DEV)
    o0, l0 = K.attn_fwd(q, k, v, s.H)
    pl = torch.full((3, B * L, W), NAN, device=DEV, dtype=torch.bfloat16)
    o1, l1 = K.attn_fwd(q, k, v, s.H, o_planes=pl)
    g0 = torch.full_like(qkv, NAN)
    views = lambda g: dict(dq=g[..., :W], dk=g[..., W:2 * W], dv=g[..., 2 * W:])  # noqa: E731
    K.attn_bwd(q, k, v, o0, l0, do, s.H, **views(g0))
    g1, gpl = torch.full_like(qkv, NAN), torch.full((3, B * L, 3 * W), NAN, device=DEV, dtype=torch.bfloat16)
    K.attn_bwd(q, k, v, o0, l0, do, s.H, dqkv_planes=gpl, **views(g1))
    g2, gpl2 = torch.full_like(qkv, 5.0), torch.full_like(gpl, NAN)
    K.attn_bwd(q, k, v, o0, l0, do, s.H, dqkv_planes=gpl2, planes_only=True, **views(g2))
    torch.cuda.synchronize()
    _compare(call, dict(o=o0, lse=l0, **views(g0)), ref, ("o", "lse", "dq", "dk", "dv"), ratios, tag="packed ")
    if not (_same_bits(o0, o1) and _same_bits(l0, l1)):
        call.problems.append("o_planes: o or lse differ from the call without planes")
    if not _same_bits(pl, K.split3(o1.view(B * L, W))):
        call.problems.append("o_planes != split3(o)")
    if not _same_bits(g0, g1):
        call.problems.append("dqkv_planes: gradients differ from the call without planes")
    want = K.split3(g0.view(B * L, 3 * W))
    if not _same_bits(gpl, want):
        call.problems.append("dqkv_planes != split3(dq | dk | dv)")
    if not _same_bits(gpl2, want):
        call.problems.append("planes_only: dqkv_planes != split3(dq | dk | dv)")
    if L <= 256 and not bool((g2 == 5.0).all()):
        call.problems.append("planes_only wrote the fp32 gradients")


def _check_bitmask(call, fw, base, got):
    s, x = call.s, call.x
    for n in ("o", "lse", "dq", "dk", "dv"):
        if not _same_bits(got[n], base[n]):
            call.problems.append(f"bitmask: {n} differs from the hashed call")
    W = (s.Lk + 31) // 32
    words = fw["dm"].cpu().numpy().view(np.uint32).reshape(s.B, s.H * s.Lq, W)
    want = C.pack_keep_bits(x["keep"], s.Lk).reshape(s.B, s.H * s.Lq, W)
    # compared on the keys a query attends to (a forward that records the mask from P leaves masked-out
    # keys 0 whatever the hash: their backward P is 0 as well)
    live = np.ones((s.B, s.Lk), dtype=bool) if x["key_bias"] is None else (x["key_bias"] == 0).numpy()
    for b in range(s.B):
        valid = C.pack_keep_bits(live[b][None], s.Lk).reshape(-1)
        if not np.array_equal(words[b] & valid, want[b] & valid):
            call.problems.append(f"bitmask: words of batch row {b} differ from the oracle's keep mask")


def _run_case(s):
    f = C.FEATURES[s.feature]
    x = C.make_inputs(s)
    ref = C.reference(s, x)
    call = Call(s, x)
    ratios = {}
    fw = call.fwd(bits=False)
    if f.cos:
        _compare(call, fw, ref, ("o", "lse"), ratios)
        return call, ratios
    names = ("dq", "dk", "dv") + (("d_rel_bias",) if f.drel else ())
    base = dict(fw, **call.bwd(fw, drel=f.drel))
    _compare(call, base, ref, ("o", "lse") + names, ratios)
    if f.bits:  # the case's own call; `base` is its hashed twin
        fw = call.fwd(bits=True)
        got = dict(fw, **call.bwd(fw, what="backward (bitmask)"))
        _check_bitmask(call, fw, base, got)
    if f.drel:
        plain = call.bwd(fw, what="backward (no d_rel_bias)")
        if not all(_same_bits(plain[n], base[n]) for n in ("dq", "dk", "dv")):
            call.problems.append("d_rel_bias: dq, dk or dv differ from the call without it")
        dead = (x["key_bias"] != 0)[:, None, None, :].expand(s.B, s.H, s.Lq, s.Lk)
        if not (dead.any() and bool((base["d_rel_bias"].cpu()[dead] == 0).all())):
            call.problems.append("d_rel_bias: a masked key column is not exactly 0")
    # accumulate: small integers are exact in bf16
    g = torch.Generator().manual_seed(s.Lq * 1000 + s.Lk)
    ints = lambda t: torch.randint(-4, 5, t.shape, generator=g).to(call.dt)  # noqa: E731
    pre = {n: ints(x[m]) for n, m in (("dq", "q"), ("dk", "k"), ("dv", "v"))}
    a = call.bwd(fw, acc_dq=pre["dq"], drel=f.drel, what="backward (accumulate_dq)")
    _compare(call, a, ref, ("dq",), ratios, tag="acc ", base=pre)
    b = call.bwd(fw, acc_dkv=(pre["dk"], pre["dv"]), drel=f.drel, what="backward (accumulate_dkv)")
    _compare(call, b, ref, ("dk", "dv"), ratios, tag="acc ", base=pre)
    for got, same, flag in ((a, ("dk", "dv"), "accumulate_dq"), (b, ("dq",), "accumulate_dkv")):
        for n in same + (("d_rel_bias",) if f.drel else ()):
            if not _same_bits(got[n], base[n]):
                call.problems.append(f"{flag}: {n} differs from the plain call")
    if f.planes:
        _check_planes(call, ref, ratios)
    return call, ratios


@pytest.mark.parametrize("s", C.table(), ids=C.spec_id)
def test_attention_against_reference(s):
    old = K.set_fp32_attn_mode(s.mode) if s.mode else None
    try:
        call, ratios = _run_case(s)
    finally:
        if old is not None:
            K.set_fp32_attn_mode(old)
    print(C.spec_id(s), ratios)
    assert not call.problems, (f"{C.spec_id(s)}: {call.problems}; kernels: {C.kernels_of(s)}; "
                               f"error / bound per output: {ratios}")
