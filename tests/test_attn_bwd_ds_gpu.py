"""mmfd_attn_bwd_ds (kernels.attn_bwd_ds): the gradient of a per-batch relative bias under attention dropout,
against tests/attention_refs.attention_ref(..., keep=, p=, want_d_rel_bias=True) with the masks of
oracle.dropout_hash.attn_keep_mask, on the kernel's rounded inputs.

Error rule: tests/attention_refs.worst_ratio("d_rel_bias", ...) <= 1, i.e. err <= atol + rtol * max|ref| per
(batch row, head) slice with the project's TOL, (3e-5, 3e-5) in fp32 and (2e-2, 2e-2) in bf16.

B = 2, H = 3, p = 0.1, a per-batch bias, with and without a prefix key mask (attn_cases' -10000 bias, no row
fully masked). Shapes (Lq, Lk) from attn_cases.SHAPES: (13, 29) odd Lk, the last key pair has one key,
4-byte stores | (70, 100) two key blocks, 16-byte stores, a ragged query block | (130, 65) odd Lk, more
queries than keys | (256, 256) the resident limit of the preceding attn_bwd | (24, 257), (257, 40) its dK/dV
and dQ kernels stream. D = 32 and 64 everywhere, 16 and 48 (zero-padded to 32 / 64) at the first two.

Every case also checks: masked key columns exactly 0; a repeat call bit-identical; a call that passes the
forward's keep-bitmask bit-identical to the hashed call; at p = 0 the entry bit-identical to attn_bwd's
d_rel_bias; dq / dk / dv of the preceding attn_bwd bit-identical to those of a call never followed by the
entry, and the entry's inputs unchanged (it writes nothing but its output)."""
import zlib

import pytest
import torch

from mmfd import kernels as K
from oracle.dropout_hash import attn_keep_mask
from tests import attention_refs as R
from tests import attn_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, P_DROP = 2, 3, 0.1
SEED, SALT = 90211, K.salt_of("test.attn_bwd_ds")
SHAPES = ((13, 29), (70, 100), (130, 65), (256, 256), (24, 257), (257, 40))
assert set(SHAPES) <= set(C.SHAPES)
CASES = [(Lq, Lk, D) for Lq, Lk in SHAPES for D in (32, 64)] + \
        [(Lq, Lk, D) for Lq, Lk in ((13, 29), (70, 100)) for D in (16, 48)]


def _inputs(dtype, Lq, Lk, D, masked):
    g = torch.Generator().manual_seed(zlib.crc32(f"{dtype}-{Lq}-{Lk}-{D}-{masked}".encode()))
    dt = torch.float32 if dtype == "f32" else torch.bfloat16
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q, k, v, dout = (rn(B, L, H * D).to(dt) for L in (Lq, Lk, Lk, Lq))
    rb = rn(B, H, Lq, Lk).contiguous()
    kb = None
    if masked:  # prefix masks as attn_cases.make_inputs: at least MIN_LIVE keys, row 0 never complete
        lens = torch.randint(min(C.MIN_LIVE, Lk), Lk + 1, (B,), generator=g)
        lens[0] = min(int(lens[0]), Lk - 1)
        kb = torch.where(torch.arange(Lk)[None, :] < lens[:, None], 0.0, -10000.0).to(torch.float32)
    return q, k, v, dout, rb, kb


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int16),
                       b.contiguous().view(torch.int32 if b.element_size() == 4 else torch.int16))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("Lq,Lk,D", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_attn_bwd_ds_against_reference(dtype, Lq, Lk, D, masked):
    q, k, v, dout, rb, kb = _inputs(dtype, Lq, Lk, D, masked)
    scale = D ** -0.5
    keep = attn_keep_mask(SEED, SALT, (B, H, Lq, Lk), P_DROP)
    ref = R.attention_ref(q, k, v, H, scale, key_bias=kb, rel_bias=rb, keep=keep, p=P_DROP, dout=dout,
                          want_d_rel_bias=True)
    qd, kd, vd, dod, rbd = (t.to(DEV) for t in (q, k, v, dout, rb))
    kbd = kb.to(DEV) if kb is not None else None
    seed = K.Seed(SEED)
    kw = dict(scale=scale, key_bias=kbd, rel_bias=rbd, dropout_p=P_DROP, seed=seed, salt=SALT)
    o, lse = K.attn_fwd(qd, kd, vd, H, **kw)
    # the call never followed by the entry
    dq0, dk0, dv0 = K.attn_bwd(qd, kd, vd, o, lse, dod, H, **kw)
    delta = torch.full((B, H, Lq), float("nan"), device=DEV)
    dq, dk, dv = K.attn_bwd(qd, kd, vd, o, lse, dod, H, delta=delta, **kw)
    before = [t.clone() for t in (qd, kd, vd, dod, lse, delta, rbd, dq, dk, dv)]
    ds = torch.full((B, H, Lq, Lk), float("nan"), device=DEV)
    out = K.attn_bwd_ds(qd, kd, vd, lse, dod, H, delta, out=ds, **kw)
    ds2 = K.attn_bwd_ds(qd, kd, vd, lse, dod, H, delta, **kw)
    # the keep-bitmask path: forward writes the mask, backward and the entry are handed it
    dm = K.drop_mask_buffer(B, H, Lq, Lk, DEV)
    o_m, lse_m = K.attn_fwd(qd, kd, vd, H, drop_mask=dm, **kw)
    delta_m = torch.empty_like(delta)
    K.attn_bwd(qd, kd, vd, o_m, lse_m, dod, H, delta=delta_m, drop_mask=dm, **kw)
    ds_m = K.attn_bwd_ds(qd, kd, vd, lse_m, dod, H, delta_m, drop_mask=dm, **kw)
    torch.cuda.synchronize()
    assert out is ds and torch.isfinite(ds).all()
    problems = []
    got = dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, d_rel_bias=ds)
    ratios = {}
    for n in ("o", "lse", "dq", "dk", "dv", "d_rel_bias"):
        r, i = R.worst_ratio(n, got[n], ref[n], H, dtype)
        ratios[n] = round(r, 3)
        if not r <= 1.0:
            problems.append(f"{n}: error {r:.3g} x bound at (batch row, head) = {divmod(i, H)}")
    print(f"{dtype} {Lq}x{Lk} D{D} {'mask' if masked else 'nomask'}: error / bound {ratios}")
    if masked:
        dead = (kb != 0)[:, None, None, :].expand(B, H, Lq, Lk)
        if not (dead.any() and bool((ds.cpu()[dead] == 0).all())):
            problems.append("a masked key column is not exactly 0")
    if not _same(ds, ds2):
        problems.append("a repeat call differs")
    if not (_same(lse, lse_m) and _same(delta, delta_m) and _same(ds, ds_m)):
        problems.append("the call with drop_mask differs from the hashed call")
    if not (_same(dq, dq0) and _same(dk, dk0) and _same(dv, dv0)):
        problems.append("dq / dk / dv differ from the call never followed by attn_bwd_ds")
    if not all(_same(a, b) for a, b in zip(before, (qd, kd, vd, dod, lse, delta, rbd, dq, dk, dv))):
        problems.append("attn_bwd_ds changed something besides its output")
    # p = 0: bit for bit the d_rel_bias of attn_bwd
    kw0 = dict(scale=scale, key_bias=kbd, rel_bias=rbd)
    o0, lse0 = K.attn_fwd(qd, kd, vd, H, **kw0)
    want = torch.full((B, H, Lq, Lk), float("nan"), device=DEV)
    delta0 = torch.empty_like(delta)
    K.attn_bwd(qd, kd, vd, o0, lse0, dod, H, d_rel_bias=want, delta=delta0, **kw0)
    got0 = K.attn_bwd_ds(qd, kd, vd, lse0, dod, H, delta0, **kw0)
    torch.cuda.synchronize()
    if not _same(got0, want):
        problems.append("p = 0: differs from d_rel_bias of attn_bwd")
    if _same(got0, ds):
        problems.append("dropout changed nothing")
    assert not problems, (problems, ratios)


def test_attn_bwd_ds_refuses_unsupported():
    Lq, Lk, D = 40, 48, 32
    q, k, v, dout, rb, _ = _inputs("f32", Lq, Lk, D, False)
    qd, kd, vd, dod, rbd = (t.to(DEV) for t in (q, k, v, dout, rb))
    seed = K.Seed(SEED)
    o, lse = K.attn_fwd(qd, kd, vd, H, rel_bias=rbd, dropout_p=P_DROP, seed=seed, salt=SALT)
    delta = torch.empty((B, H, Lq), device=DEV)
    K.attn_bwd(qd, kd, vd, o, lse, dod, H, rel_bias=rbd, dropout_p=P_DROP, seed=seed, salt=SALT, delta=delta)
    ds = torch.zeros(B, H, Lq, Lk, device=DEV)
    shared = rbd[0].contiguous()  # [H, Lq, Lk]: one bias for the whole batch
    with pytest.raises(RuntimeError, match="per-batch rel_bias"):
        K.attn_bwd_ds(qd, kd, vd, lse, dod, H, delta, rel_bias=shared, out=ds)
    with pytest.raises(RuntimeError, match="alias"):
        K.attn_bwd_ds(qd, kd, vd, lse, dod, H, delta, rel_bias=rbd, out=rbd)
    with pytest.raises(RuntimeError, match="seed"):
        K.attn_bwd_ds(qd, kd, vd, lse, dod, H, delta, rel_bias=rbd, dropout_p=P_DROP, out=ds)
    with pytest.raises(ValueError, match="delta"):
        K.attn_bwd_ds(qd, kd, vd, lse, dod, H, delta[:, :, :-1], rel_bias=rbd, out=ds)
    with pytest.raises(ValueError, match="out must be"):
        K.attn_bwd_ds(qd, kd, vd, lse, dod, H, delta, rel_bias=rbd, out=ds[:, :, :, :-1])
    torch.cuda.synchronize()
    assert (ds == 0).all() and torch.equal(rbd.cpu(), rb)
