"""Operator-level tests of the memory-bound training kernels (csrc/misc.hip, csrc/runtime.hip and the
small kernels of csrc/conv.hip) against the plain CPU fp64 references of tests/memory_kernel_refs.py
(proven without a GPU by tests/test_memory_kernels_ref_cpu.py), at the smallest shapes that reach
every code path: scalar and vector forms, partial last blocks and waves, grid-stride loops past the
capped grids, misaligned and sliced buffers.

Tolerances (derived, not tuned):
  * data movement and integer results: bitwise (torch.equal);
  * fp32 -> bf16 without arithmetic: bitwise equal to torch's CPU round-to-nearest-even;
  * fp32 arithmetic: the suite's convention, 3e-5 * scale + 3e-5 * max |ref| (test_kernels_gpu._tol);
  * a bf16 output of an fp32 computation: |got - ref| <= 2^-8 |ref| + 3e-5 * scale per element (one
    rounding to 8 significant bits plus the fp32 error);
  * the GELU derivative: 1.2e-6 absolute (the bound test_gemm_gelu_deriv_pair holds gelu_grad_f to);
  * AdamW parameters: 1e-6 absolute (test_adamw_matches_torch).
"""
import numpy as np
import pytest
import torch

from mmfd import kernels as K
from oracle.dropout_hash import drop_threshold, dropout_hash, keep_mask
from tests import memory_kernel_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
SWEEP = 8192 * 256  # elements one sweep of runtime.hip's capped grid covers (one per thread)
CAP = 16384 * 256   # the same for misc.hip's gridn
_rand = R.rand


def _close(got, ref, scale=1.0, what=""):
    """the bound of the output's dtype (module docstring); `scale`: the magnitude of the operands"""
    ex = R.excess(got, ref, float(scale))
    print(f"{what or 'excess'} [{str(got.dtype).split('.')[-1]}]: {ex:.3e}")
    assert ex <= 0, f"{what}: {ex:.3e} over the {got.dtype} bound"


def _ints(lo, hi, shape, seed):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------------------
# embeddings + LayerNorm (embed_ln_fwd_kernel: a wave per token, 16 strided slots per lane)
# ---------------------------------------------------------------------------------------------
EMB_D = [40, 384, 1000, 1024]  # < one wave's lanes, a multiple of 64, a partial last slot, all 16 slots
EPS = 1e-5


def _emb_inputs(B, L, D, seed=0):
    """tables with a common offset in `word` (sum != its own LayerNorm, so rounding the stored sum
    matters), gamma / beta away from a zero output; explicit position ids with repeated padding
    positions (HF position ids of a sequence with padding_idx 1 inside)"""
    ids = _ints(0, 50, (B, L), seed + 1)
    tts = _ints(0, 2, (B, L), seed + 2)
    padded = ids.clone()
    padded[:, ::3] = 1
    pos_ids = R.position_ids_ref(padded, 1)  # values in [1, L + 1], 1 repeated at the padding
    word = _rand(50, D, seed=seed + 3) + 2.0
    pos = _rand(L + 2, D, seed=seed + 4, scale=0.5)
    typ = _rand(2, D, seed=seed + 5, scale=0.5)
    gamma = 1.0 + 0.1 * _rand(D, seed=seed + 6)
    beta = 0.5 + 0.1 * _rand(D, seed=seed + 7)
    return ids, tts, pos_ids, word, pos, typ, gamma, beta


def _emb_check(got, s64, gamma, beta, dtype, what):
    """got = (sum or None, y, mean or None, rstd or None). With a stored bf16 sum the LayerNorm is
    the LayerNorm of that stored (rounded) sum, which is what the backward re-reads: the stored sum
    is first held to its own bound, then taken as the reference LayerNorm's input. Without a stored
    sum (embed_ln_infer) the LayerNorm is over the unrounded fp32 sum."""
    s, y, mean, rstd = got
    sc = s64.abs().max().item()
    ln_in = s64
    if s is not None:
        _close(s, s64, sc, what + " sum")
        if dtype == torch.bfloat16:
            ln_in = s.double().cpu()
    yr, mr, rr = R.layernorm_ref(ln_in, gamma, beta, EPS)
    _close(y, yr, yr.abs().max().item(), what + " y")
    if mean is not None:
        _close(mean, mr, sc, what + " mean")
        _close(rstd, rr, rr.abs().max().item(), what + " rstd")
    return yr


def _emb_variants(B, L, D, dtype, seed=0):
    ids, tts, pos_ids, word, pos, typ, gamma, beta = _emb_inputs(B, L, D, seed)
    d = lambda t: t.to(DEV)  # noqa: E731
    wd, pd, td, gd, bd = d(word), d(pos), d(typ), d(gamma), d(beta)
    # type table and token types (embed_ln_fwd), positions row % L
    s64 = R.embed_sum_ref(ids, None, tts, word, pos, typ)
    _emb_check(K.embed_ln_fwd(d(ids), d(tts), wd, pd, td, gd, bd, EPS, dtype), s64, gamma, beta, dtype, "fwd")
    # type table without token types: every token takes type row 0
    s64 = R.embed_sum_ref(ids, None, None, word, pos, typ)
    _emb_check(K.embed_ln_fwd(d(ids), None, wd, pd, td, gd, bd, EPS, dtype), s64, gamma, beta, dtype, "fwd tts=None")
    for pids, tag in ((pos_ids, "pos_ids"), (None, "row % L")):
        pdev = d(pids) if pids is not None else None
        # no type table, nothing saved / everything saved
        s64 = R.embed_sum_ref(ids, pids, None, word, pos, None)
        y = K.embed_ln_infer(d(ids), pdev, wd, pd, gd, bd, EPS, dtype)
        _emb_check((None, y, None, None), s64, gamma, beta, dtype, f"infer {tag}")
        _emb_check(K.embed_ln_train(d(ids), pdev, wd, pd, gd, bd, EPS, dtype), s64, gamma, beta, dtype, f"train {tag}")
        # inference with a type table
        s64 = R.embed_sum_ref(ids, pids, tts, word, pos, typ)
        y = K.embed_ln_infer(d(ids), pdev, wd, pd, gd, bd, EPS, dtype, tts=d(tts), typ=td)
        _emb_check((None, y, None, None), s64, gamma, beta, dtype, f"infer typed {tag}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", EMB_D)
def test_embed_ln_variants(dtype, D):
    """B*L = 7: the last block has one live wave"""
    _emb_variants(1, 7, D, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_ln_many_blocks(dtype):
    """B*L = 4*300 + 3 rows (301 blocks, three live waves in the last), L = 401: row % L wraps"""
    _emb_variants(3, 401, 384, dtype, seed=20)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", EMB_D)
def test_embed_ln_dropout_mask_and_scale(dtype, D):
    B, L, p = 1, 7, 0.1
    ids, tts, _, word, pos, typ, gamma, beta = _emb_inputs(B, L, D, seed=40)
    args = [t.to(DEV) for t in (ids, tts, word, pos, typ, gamma, beta)]
    seed = K.Seed(123)
    s0, y0, m0, r0 = K.embed_ln_fwd(*args, EPS, dtype)
    assert (y0 != 0).all()  # precondition: a zero of the dropped output is a dropped element
    yr = _emb_check((s0, y0, m0, r0), R.embed_sum_ref(ids, None, tts, word, pos, typ), gamma, beta, dtype, "p=0")
    patterns = []
    for salt in (K.salt_of("embeddings.dropout"), 7):
        s, y, m, r = K.embed_ln_fwd(*args, EPS, dtype, dropout_p=p, seed=seed, salt=salt)
        keep = torch.from_numpy(keep_mask(123, salt, (B * L, D), p))
        assert torch.equal((y == 0).cpu(), ~keep)
        _close(y, R.dropout_ref(yr, keep, p), yr.abs().max().item() / (1 - p), "dropped y")
        for a, b in ((s, s0), (m, m0), (r, r0)):  # what the backward re-reads does not see the dropout
            assert torch.equal(a, b)
        if dtype == torch.float32:  # the identity the embedding backward relies on (it re-draws the mask)
            assert torch.equal(y, K.dropout(y0, p, seed, salt))
        patterns.append(keep)
    assert not torch.equal(patterns[0], patterns[1])


def test_embed_ln_refuses_wide_rows():
    ids, tts, _, word, pos, typ, gamma, beta = _emb_inputs(1, 7, 1025)
    with pytest.raises(RuntimeError, match="D <= 1024"):  # a host check: nothing launches
        K.embed_ln_fwd(*[t.to(DEV) for t in (ids, tts, word, pos, typ, gamma, beta)], EPS, torch.float32)


# ---------------------------------------------------------------------------------------------
# integer kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [1, 0])
def test_position_ids(pad):
    """B = 257: the second block has one live thread"""
    ids = _ints(0, 6, (257, 9), 50 + pad)
    ids[0] = pad + 1                 # no padding
    ids[1] = pad                     # all padding
    ids[2] = pad + 2; ids[2, 3:6] = pad  # noqa: E702  padding in the middle
    ids[3] = pad + 3; ids[3, 0] = pad    # noqa: E702  padding first
    ids[256] = pad + 1; ids[256, 8] = pad  # noqa: E702  the lone thread of the last block
    out = K.position_ids(ids.to(DEV), pad)
    assert out.dtype == torch.int64 and torch.equal(out.cpu(), R.position_ids_ref(ids, pad))


@pytest.mark.parametrize("H,Lq,Lk", [(3, 5, 7), (5, 920, 920)])
def test_rel_bias(H, Lq, Lk):
    """(5, 920, 920): more elements than the capped grid covers in one sweep"""
    assert (H * Lq * Lk > CAP) == (Lq == 920)
    bucket = _ints(0, 32, (Lq, Lk), 60).int()
    table = _rand(32, H, seed=61)
    out = K.rel_bias(bucket.to(DEV), table.to(DEV))
    assert torch.equal(out.cpu(), R.rel_bias_ref(bucket, table))  # table[bucket].permute(2, 0, 1)


def test_mask_to_bias():
    mask = _ints(0, 3, (3, 50), 62)
    assert torch.equal(K.mask_to_bias(mask.to(DEV), -1e4).cpu(), R.mask_to_bias_ref(mask, -1e4))
    fmin = torch.finfo(torch.float32).min
    assert torch.equal(K.mask_to_bias(mask.to(DEV)).cpu(), R.mask_to_bias_ref(mask, fmin))


# ---------------------------------------------------------------------------------------------
# ViT
# ---------------------------------------------------------------------------------------------
def _patchify_case(px_dev, px, P, dtype):
    out = K.patchify(px_dev, P, dtype)
    assert out.dtype == dtype
    # no arithmetic: bitwise, bf16 = torch's round-to-nearest-even of each pixel
    assert torch.equal(out.cpu(), R.patchify_ref(px, P).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,H,W", [(4, 8, 12), (16, 32, 48),  # vector form
                                   (3, 9, 12), (2, 4, 6)])     # scalar form
def test_patchify(dtype, P, H, W):
    px = _rand(2, 3, H, W, seed=70)
    _patchify_case(px.to(DEV), px, P, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_patchify_misaligned_pixels_take_scalar_form(dtype):
    """P = 4 with pixels that start 4 bytes past a 16-byte boundary"""
    B, C, H, W = 2, 3, 8, 12
    px = _rand(B, C, H, W, seed=71)
    buf = torch.zeros(1 + px.numel(), device=DEV)
    view = buf[1:].view(B, C, H, W)
    view.copy_(px)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    _patchify_case(view, px, 4, dtype)


def test_patchify_vector_form_past_the_grid_cap():
    B, C, H, W = 2, 3, 1676, 1676
    assert B * C * H * W > CAP * 4
    px = _rand(B, C, H, W, seed=72)
    _patchify_case(px.to(DEV), px, 4, torch.float32)


def test_patchify_refuses_indivisible_image():
    with pytest.raises(RuntimeError, match="not divisible"):
        K.patchify(torch.zeros(2, 3, 10, 12, device=DEV), 4, torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [40, 768])
def test_vit_tokens_fwd_bwd(dtype, D):
    B, NP = 5, 6
    patch = _rand(B * NP, D, seed=73).to(dtype)
    cls, pos = _rand(D, seed=74), _rand(NP + 1, D, seed=75)
    out = K.vit_tokens_fwd(patch.to(DEV), B, cls.to(DEV), pos.to(DEV))
    ref = R.vit_tokens_fwd_ref(patch, B, cls, pos)
    _close(out, ref, ref.abs().max().item(), "tokens")
    dout = _rand(B, NP + 1, D, seed=76).to(dtype)
    rpatch, rcls, rpos = R.vit_tokens_bwd_ref(dout)
    for want in (True, False):
        dpatch, dcls, dpos = K.vit_tokens_bwd(dout.to(DEV), want_dpatch=want)
        if want:
            assert torch.equal(dpatch.cpu(), rpatch)  # a copy
        else:
            assert dpatch is None
        assert dcls.dtype == dpos.dtype == torch.float32
        assert torch.equal(dcls, dpos[0])
        _close(dpos, rpos, B * dout.double().abs().max().item(), "dpos")
        _close(dcls, rcls, B * dout.double().abs().max().item(), "dcls")


def test_vit_tokens_fwd_past_the_grid_cap():
    B, NP, D = 28, 196, 768
    assert B * (NP + 1) * D > CAP
    patch, cls, pos = _rand(B * NP, D, seed=77), _rand(D, seed=78), _rand(NP + 1, D, seed=79)
    out = K.vit_tokens_fwd(patch.to(DEV), B, cls.to(DEV), pos.to(DEV))
    ref = R.vit_tokens_fwd_ref(patch, B, cls, pos)
    _close(out, ref, ref.abs().max().item(), "tokens")


# ---------------------------------------------------------------------------------------------
# cast
# ---------------------------------------------------------------------------------------------
def _from_bits(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def _cast_values():
    """48 fp32 values: signed zeros and infinities, exact ties (0x3F808000 rounds to even = down,
    0x3F818000 up) of both signs, the largest finite values (round to +-inf), NaNs (quiet, negative,
    signalling), and randn at three magnitudes"""
    special = _from_bits([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F808000, 0x3F818000, 0xBF808000,
                          0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001])
    return torch.cat([special, _rand(12, seed=80) * 1e-20, _rand(12, seed=81), _rand(11, seed=82) * 1e20])


def _same_bf16(got, x):
    """got == torch's CPU round-to-nearest-even of x bit for bit; NaN by isnan"""
    want = x.to(torch.bfloat16)
    got = got.cpu()
    nan = torch.isnan(x)
    assert got.dtype == torch.bfloat16 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])


def test_cast_f32_to_bf16_every_path_rounds_to_nearest_even():
    v = _cast_values()
    assert v.numel() % 8 == 0
    # vector form: n % 8 == 0, both pointers 16-byte aligned
    xd = v.to(DEV)
    assert xd.data_ptr() % 16 == 0
    _same_bf16(K.cast(xd, torch.bfloat16), v)
    # scalar form from n = 8k + 3 (the same values, three of them again)
    v3 = torch.cat([v, v[4:7]])
    _same_bf16(K.cast(v3.to(DEV), torch.bfloat16), v3)
    # scalar form from an `out` slice at an odd element of a larger buffer (blocks.py casts into
    # slices of a packed buffer): the guard elements on both sides stay
    big = torch.full((v.numel() + 10,), 3.0, device=DEV, dtype=torch.bfloat16)
    out = big[1:1 + v.numel()]
    assert out.data_ptr() % 16 == 2 and K.cast(xd, torch.bfloat16, out=out) is out
    _same_bf16(out, v)
    assert big[0].item() == 3.0 and (big[1 + v.numel():] == 3.0).all()
    # scalar form from an input 4 bytes off alignment
    buf = torch.zeros(1 + v.numel(), device=DEV)
    buf[1:].copy_(v)
    assert buf[1:].data_ptr() % 16 == 4
    _same_bf16(K.cast(buf[1:], torch.bfloat16), v)


def test_cast_f32_denormals():
    """fp32 denormals: the vector and the scalar form return the same bits, and each output is the
    round-to-nearest-even result or a zero of the same sign. Observed on gfx950 (MI355X): round to
    nearest even in both forms, nothing is flushed (0x00008000 ties to 0, 0x00018000 to 0x0002,
    0x007FFFFF rounds up to the smallest normal bf16 0x0080). The observed form is printed."""
    mags = [0x00000001, 0x00008000, 0x00018000, 0x00012345, 0x00400000, 0x007FFFFF, 0x007F8000, 0x007F7FFF]
    x = _from_bits(mags + [m | 0x80000000 for m in mags])
    vec = K.cast(x.to(DEV), torch.bfloat16)
    buf = torch.zeros(1 + x.numel(), device=DEV)
    buf[1:].copy_(x)
    sca = K.cast(buf[1:], torch.bfloat16)
    assert torch.equal(_bits(vec), _bits(sca))
    rne = _bits(x.to(torch.bfloat16))
    zero = torch.where(_bits(x) < 0, -32768, 0).to(torch.int16)  # a zero with the input's sign bit
    got = _bits(vec)
    is_rne, is_zero = got == rne, got == zero
    assert (is_rne | is_zero).all()
    observed = "rne" if is_rne.all() else "flushed" if is_zero.all() else "mixed"
    print("fp32 denormal -> bf16:", observed, [hex(b & 0xFFFF) for b in got.tolist()])


@pytest.mark.parametrize("src,dst", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                     (torch.bfloat16, torch.float32)])
def test_cast_exact_pairs(src, dst):
    """no rounding in these three pairs: bitwise (finite values, signed zeros, infinities)"""
    x = torch.cat([_rand(1000, seed=83), _rand(20, seed=84) * 1e-20, _rand(20, seed=85) * 1e20,
                   torch.tensor([0.0, -0.0, float("inf"), -float("inf")])]).to(src)
    out = K.cast(x.to(DEV), dst)
    assert out.dtype == dst and torch.equal(_bits(out), _bits(x.to(dst)))


@pytest.mark.parametrize("n", [2 ** 24 + 8, SWEEP + 5])
def test_cast_f32_to_bf16_past_one_sweep(n):
    """vector form past 8192*256 threads x 8 elements; scalar form (n % 8 = 5) past 8192*256"""
    assert (n % 8 == 0 and n > SWEEP * 8) or (n % 8 and n > SWEEP)
    x = _rand(n, seed=86)
    out = K.cast(x.to(DEV), torch.bfloat16)
    assert torch.equal(_bits(out), _bits(x.to(torch.bfloat16)))


# ---------------------------------------------------------------------------------------------
# zero fill
# ---------------------------------------------------------------------------------------------
def test_zero_slices_of_a_byte_buffer():
    """the 16-byte body and the byte tail of zero_kernel, aligned and misaligned starts"""
    for off in (0, 1, 8, 15, 16):
        for n in (0, 1, 15, 16, 17, 4099):
            buf = torch.full((off + n + 33,), 0xAB, device=DEV, dtype=torch.uint8)
            K.zero_(buf[off:off + n])
            want = torch.full((off + n + 33,), 0xAB, dtype=torch.uint8)
            want[off:off + n] = 0
            assert torch.equal(buf.cpu(), want), (off, n)


def test_zeros():
    for dtype, shape in ((torch.float32, (3, 5)), (torch.bfloat16, (7,)), (torch.int64, (2, 3, 4)), (torch.float32, (0,))):
        z = K.zeros(shape, dtype=dtype, device=DEV)
        assert z.dtype == dtype and tuple(z.shape) == shape and not z.cpu().view(torch.uint8).any()
    with pytest.raises(ValueError):
        K.zero_(torch.ones(4, 4, device=DEV)[:, :2])


# ---------------------------------------------------------------------------------------------
# axpby / dropout / act_bwd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, SWEEP + 5])
def test_axpby(dtype, n):
    x, y = _rand(n, seed=90).to(dtype), _rand(n, seed=91).to(dtype)
    xd, yd = x.to(DEV), y.to(DEV)
    # y=None ignores b
    _close(K.axpby(1.5, xd, b=7.0), R.axpby_ref(1.5, x), 1.5 * 5, "y=None")
    # b = 0 with y given
    _close(K.axpby(-0.75, xd, b=0.0, y=yd), R.axpby_ref(-0.75, x), 0.75 * 5, "b=0")
    # a = 0
    _close(K.axpby(0.0, xd, b=1.25, y=yd), R.axpby_ref(0.0, x, 1.25, y), 1.25 * 5, "a=0")
    # out aliasing x (fusion.py / dp.py accumulate in place)
    acc = xd.clone()
    assert K.axpby(2.0, acc, b=0.5, y=yd, out=acc) is acc
    _close(acc, R.axpby_ref(2.0, x, 0.5, y), 2.5 * 5, "in place")
    assert torch.equal(xd.cpu(), x) and torch.equal(yd.cpu(), y)  # the operands themselves are only read


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("n", [1000, SWEEP + 5])
def test_dropout(dtype, p, n):
    x = _rand(n, seed=92).to(dtype)
    x[x == 0] = 1.0  # no exact zeros: a zero of the output is a dropped element
    salt = K.salt_of("test.dropout")
    out = K.dropout(x.to(DEV), p, K.Seed(123), salt)
    keep = torch.from_numpy(keep_mask(123, salt, (n,), p))
    assert torch.equal((out == 0).cpu(), ~keep)
    assert p > 0 or keep.all()
    _close(out, R.dropout_ref(x, keep, p), x.double().abs().max().item() / (1 - p), "kept")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout_threshold_is_exclusive(dtype, p):
    """keep <=> hash >= threshold: an element whose hash equals the threshold is kept, one just below
    it is dropped (salts solved for, tests/memory_kernel_refs.py salt_with_hash); the same element
    through act_bwd, which re-draws the mask of a GEMM epilogue"""
    n, idx, thr = 1000, 777, drop_threshold(p)
    x = torch.ones(n, dtype=dtype)
    for target, kept in ((thr, True), (thr - 1, False)):
        if target < 0:
            continue  # p = 0 drops nothing
        salt = R.salt_with_hash(123, idx, target)
        assert int(dropout_hash(123, salt, [idx])[0]) == target
        keep = torch.from_numpy(keep_mask(123, salt, (n,), p))
        assert bool(keep[idx]) == kept
        out = K.dropout(x.to(DEV), p, K.Seed(123), salt)
        assert torch.equal((out == 0).cpu(), ~keep)
        if p > 0:
            out = K.act_bwd(x.to(DEV), None, K.ACT_NONE, dropout_p=p, seed=K.Seed(123), salt=salt)
            assert torch.equal((out == 0).cpu(), ~keep)


def test_dropout_refuses_bad_arguments():
    x = torch.ones(8, device=DEV)
    with pytest.raises(RuntimeError, match="bad p/seed"):
        K.dropout(x, 1.0, K.Seed(123), 0)
    with pytest.raises(RuntimeError, match="bad p/seed"):
        K.dropout(x, 0.1, None, 0)


GELU_TOL = 1.2e-6


def _gelu_aux():
    return torch.cat([torch.linspace(-12, 12, 4001), torch.tensor([0.0, -0.0, 1e-30, -1e-30, 40.0, -40.0]),
                      _rand(1000, seed=93)])


def test_act_bwd_gelu_derivative_fp32():
    """dy = 1: the output is gelu'(aux) itself; 0 / 1 in the tails and never NaN"""
    aux = _gelu_aux()
    out = K.act_bwd(torch.ones(aux.numel(), device=DEV), aux.to(DEV), K.ACT_GELU).cpu()
    err = (out.double() - R.gelu_grad_ref(aux)).abs().max().item()
    print(f"gelu' max abs err {err:.3e}")
    assert not torch.isnan(out).any() and err <= GELU_TOL
    assert out[aux == 40.0].item() == 1.0 and out[aux == -40.0].item() == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["gelu", "relu", "none"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_act_bwd(dtype, act, p):
    if act == "gelu":
        aux = _gelu_aux()
    else:  # exact zeros of both signs: relu'(0) = 0, matching `a > 0`
        aux = torch.cat([_rand(1500, seed=94), torch.zeros(5), -torch.zeros(5)])
    aux = aux.to(dtype)
    n = aux.numel()
    dy = _rand(n, seed=95).to(dtype)
    dy[dy == 0] = 1.0
    code = {"gelu": K.ACT_GELU, "relu": K.ACT_RELU, "none": K.ACT_NONE}[act]
    salt = K.salt_of("test.act_bwd")
    seed = K.Seed(123) if p > 0 else None
    out = K.act_bwd(dy.to(DEV), aux.to(DEV), code, dropout_p=p, seed=seed, salt=salt)
    keep = torch.from_numpy(keep_mask(123, salt, (n,), p)) if p > 0 else None
    z = R.act_bwd_ref(dy, aux, "none", keep, p)  # the gradient before the activation's derivative
    ref = R.act_bwd_ref(dy, aux, act, keep, p)
    got = out.double().cpu()
    assert not torch.isnan(got).any()
    if p > 0:
        assert (got[~keep] == 0).all()
    if act == "relu":
        assert (got[aux.double() <= 0] == 0).all() and (got[(aux.double() > 0) & (z != 0)] != 0).all()
    if dtype == torch.bfloat16:
        _close(out, ref, z.abs().max().item(), act)
    elif p == 0 and act != "gelu":  # a copy or a select: bitwise
        assert torch.equal(out.cpu().double(), ref)
    else:  # the derivative's own bound on top of a few fp32 roundings (dropout scale, products)
        bound = (GELU_TOL if act == "gelu" else 0.0) * z.abs() + 2.0 ** -22 * ref.abs()
        ex = ((got - ref).abs() - bound).max().item()
        print(f"{act} p={p}: excess {ex:.3e}")
        assert ex <= 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_act_bwd_without_activation_reads_no_aux(dtype, p):
    """defect: act_bwd_kernel loaded aux[i] for MMFD_ACT_NONE too, where aux may be null. Without an
    activation the kernel only undoes the dropout: bitwise K.dropout."""
    dy = _rand(SWEEP + 5, seed=96).to(dtype).to(DEV)
    seed, salt = K.Seed(123), K.salt_of("test.act_none")
    out = K.act_bwd(dy, None, K.ACT_NONE, dropout_p=p, seed=seed if p > 0 else None, salt=salt)
    assert torch.equal(out, K.dropout(dy, p, seed, salt))


def test_act_bwd_refuses_missing_operands():
    dy = torch.ones(8, device=DEV)
    for act in (K.ACT_GELU, K.ACT_RELU):
        with pytest.raises(RuntimeError, match="need aux"):
            K.act_bwd(dy, None, act)
    with pytest.raises(RuntimeError, match="bad act"):
        K.act_bwd(dy, dy, K.ACT_TANH)
    with pytest.raises(RuntimeError, match="dropout needs seed"):
        K.act_bwd(dy, dy, K.ACT_GELU, dropout_p=0.1)
    out = torch.empty_like(dy)
    for dyp, outp in ((None, K._ptr(out)), (K._ptr(dy), None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            K._check(K.lib().mmfd_act_bwd(K.F32, 8, dyp, K._ptr(dy), K.ACT_GELU, 0.0, None, 0, outp, K._stream()),
                     "mmfd_act_bwd")


def test_null_required_pointers_are_refused():
    """host-side argument checks (nothing launches): each entry point with one required pointer null"""
    L, st = K.lib(), K._stream()
    f = torch.ones(4 * 3 * 8 * 8, device=DEV)
    i64 = torch.zeros(64, device=DEV, dtype=torch.int64)
    i32 = torch.zeros(64, device=DEV, dtype=torch.int32)
    fp, ip, bp, seed = K._ptr(f), K._ptr(i64), K._ptr(i32), K.Seed(1).ptr()
    calls = {
        "mmfd_axpby": lambda: L.mmfd_axpby(K.F32, 4, 1.0, None, 0.0, None, fp, st),
        "mmfd_axpby out": lambda: L.mmfd_axpby(K.F32, 4, 1.0, fp, 0.0, None, None, st),
        "mmfd_dropout": lambda: L.mmfd_dropout(K.F32, 4, None, fp, 0.1, seed, 0, st),
        "mmfd_dropout out": lambda: L.mmfd_dropout(K.F32, 4, fp, None, 0.1, seed, 0, st),
        "mmfd_vit_tokens_fwd patch": lambda: L.mmfd_vit_tokens_fwd(K.F32, 2, 3, 4, None, fp, fp, fp, st),
        "mmfd_vit_tokens_fwd cls": lambda: L.mmfd_vit_tokens_fwd(K.F32, 2, 3, 4, fp, None, fp, fp, st),
        "mmfd_vit_tokens_fwd out": lambda: L.mmfd_vit_tokens_fwd(K.F32, 2, 3, 4, fp, fp, fp, None, st),
        "mmfd_vit_tokens_bwd dout": lambda: L.mmfd_vit_tokens_bwd(K.F32, 2, 3, 4, None, fp, fp, fp, None, 0, st),
        "mmfd_vit_tokens_bwd dcls": lambda: L.mmfd_vit_tokens_bwd(K.F32, 2, 3, 4, fp, fp, None, fp, None, 0, st),
        "mmfd_vit_tokens_bwd dpos": lambda: L.mmfd_vit_tokens_bwd(K.F32, 2, 3, 4, fp, None, fp, None, None, 0, st),
        "mmfd_patchify pixels": lambda: L.mmfd_patchify(K.F32, 2, 3, 8, 8, 4, None, fp, st),
        "mmfd_patchify out": lambda: L.mmfd_patchify(K.F32, 2, 3, 8, 8, 4, fp, None, st),
        "mmfd_position_ids ids": lambda: L.mmfd_position_ids(4, 8, None, 1, ip, st),
        "mmfd_position_ids out": lambda: L.mmfd_position_ids(4, 8, ip, 1, None, st),
        "mmfd_rel_bias bucket": lambda: L.mmfd_rel_bias(2, 4, 8, None, fp, fp, st),
        "mmfd_rel_bias table": lambda: L.mmfd_rel_bias(2, 4, 8, bp, None, fp, st),
        "mmfd_rel_bias out": lambda: L.mmfd_rel_bias(2, 4, 8, bp, fp, None, st),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="null pointer"):
            K._check(call(), name)
    torch.cuda.synchronize()
    assert (f == 1).all() and not i64.any()


# ---------------------------------------------------------------------------------------------
# sequence mean backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,B,L,D", [(torch.float32, 3, 7, 12), (torch.bfloat16, 3, 7, 12),
                                         (torch.float32, 2, 197, 200), (torch.bfloat16, 2, 197, 200),
                                         (torch.float32, 5, 1100, 768)])
def test_seq_mean_bwd(dtype, B, L, D):
    """a random dout that is a [:, :D] view of a [B, D + 8] buffer (ldo > D); (5, 1100, 768) is past
    the capped grid"""
    assert (B * L * D > CAP) == (L == 1100)
    buf = _rand(B, D + 8, seed=100).to(dtype)
    dx = K.seq_mean_bwd(buf.to(DEV)[:, :D], L)
    assert tuple(dx.shape) == (B, L, D)
    _close(dx, R.seq_mean_bwd_ref(buf[:, :D], L), buf.double().abs().max().item() / L, "dx")


# ---------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------
def _xent_check(loss, dl, rloss, rgrads):
    per_path = rloss[1:].abs().max().item()
    err = (loss.double().cpu() - rloss).abs().max().item()
    print(f"xent loss err {err:.3e} (bound {3e-5 * per_path:.3e})")
    assert err <= 3e-5 * per_path
    for g, r in zip(dl, rgrads):
        assert torch.isfinite(g).all()
        gerr = (g.double().cpu() - r).abs().max().item()
        assert gerr <= 1e-6, gerr


@pytest.mark.parametrize("paths,B,C", [(4, 100, 3), (1, 300, 2), (2, 64, 17)])
def test_xent_rows_past_the_block(paths, B, C):
    """paths * B rows on one block of 256 threads: the first two cases loop"""
    logits = [_rand(B, C, seed=110 + i, scale=3.0) for i in range(paths)]
    labels = _ints(0, C, (B, 4), 111)
    dev = [l.to(DEV) for l in logits]
    loss, dl = K.xent_fwd_bwd(dev, labels.to(DEV))
    _xent_check(loss, dl, *R.xent_ref(logits, labels))
    # a device-side gradient scale: the losses stay, the gradients scale
    sc = torch.full((1,), 0.125, device=DEV)
    loss_s, dl_s = K.xent_fwd_bwd(dev, labels.to(DEV), dloss_scale=sc)
    assert torch.equal(loss_s, loss)
    _xent_check(loss_s, dl_s, *R.xent_ref(logits, labels, dloss_scale=0.125))
    # want_grad=False: the same loss, no gradients
    loss_n, none = K.xent_fwd_bwd(dev, labels.to(DEV), want_grad=False)
    assert none is None and torch.equal(loss_n, loss)


def test_xent_extreme_logits():
    """[1000, 0, -1000] under each of the three labels: losses 0, 1000 and 2000, finite gradients"""
    z = torch.tensor([[1000.0, 0.0, -1000.0]] * 2)
    labels = torch.tensor([[0, 1, 2]] * 2)
    loss, dl = K.xent_fwd_bwd([z.to(DEV)] * 3, labels.to(DEV))
    rloss, rgrads = R.xent_ref([z] * 3, labels)
    assert rloss.tolist() == [3000.0, 0.0, 1000.0, 2000.0]
    _xent_check(loss, dl, rloss, rgrads)
    # the three rows under one path
    z3, l3 = torch.tensor([[1000.0, 0.0, -1000.0]] * 3), torch.tensor([0, 1, 2])
    loss, dl = K.xent_fwd_bwd([z3.to(DEV)], l3.to(DEV))
    _xent_check(loss, dl, *R.xent_ref([z3], l3))


def test_xent_label_columns_and_absent_slots():
    logits = [_rand(6, 3, seed=112), _rand(6, 3, seed=113)]
    labels = _ints(0, 3, (6, 4), 114)
    loss, dl = K.xent_fwd_bwd([l.to(DEV) for l in logits], labels.to(DEV), cols=[1, 3], n_slots=5)
    rloss, rgrads = R.xent_ref(logits, labels, cols=[1, 3], n_slots=5)
    _xent_check(loss, dl, rloss, rgrads)
    assert loss[1].item() == 0.0 and loss[3].item() == 0.0


def test_xent_op_refuses_mismatched_tensors():
    """defect: mmfd::xent took B and C from logits[0] alone"""
    B, C = 6, 3
    a, b = torch.zeros(B, C, device=DEV), torch.zeros(B, C, device=DEV)
    labels = torch.zeros(B, 4, device=DEV, dtype=torch.int64)
    loss = torch.zeros(3, device=DEV)
    op = K._ops().xent
    op([a, b], [0, 1], labels, loss, [torch.empty_like(a), torch.empty_like(b)], None)  # the accepted form
    for bad in (torch.zeros(B + 1, C, device=DEV), torch.zeros(B, C + 1, device=DEV), torch.zeros(B * C, device=DEV)):
        with pytest.raises(RuntimeError, match="logits of path 1"):
            K.xent_fwd_bwd([a, bad], labels)
    for bad in (torch.empty(B, C + 1, device=DEV), torch.empty(B - 1, C, device=DEV), torch.empty(C, B, device=DEV).t(),
                torch.empty(B, C, device=DEV, dtype=torch.bfloat16)):
        with pytest.raises(RuntimeError, match="dlogits of path 1"):
            op([a, b], [0, 1], labels, loss, [torch.empty_like(a), bad], None)
    for bad in (labels.int(), labels[:B - 1], torch.zeros(B + 1, 4, device=DEV, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="labels must be int64"):
            K.xent_fwd_bwd([a, b], bad)


# ---------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------
SENT = 12345.0


class _Arena:
    """buffers carved out of one allocation, three sentinel elements directly after each"""

    def __init__(self, sizes, dtype):
        self.offs, total = [], 0
        for n in sizes:
            self.offs.append((total, n))
            total += n + 3
        self.buf = torch.full((total,), SENT, device=DEV, dtype=dtype)
        self.guard = torch.ones(total, dtype=torch.bool)
        for o, n in self.offs:
            self.guard[o:o + n] = False

    def view(self, i):
        o, n = self.offs[i]
        return self.buf[o:o + n]

    def sentinels_intact(self):
        return bool((self.buf.cpu()[self.guard] == SENT).all())


@pytest.mark.parametrize("wd", [0.01, 0.0])
def test_adamw_table(wd):
    """three tensors (1, 257 and 300001 elements: the last needs the grid-stride loop), a bf16 shadow
    for the second and third, a hand-built pointer table as optim._table builds it"""
    numels = [1, 257, 300001]
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    f32 = _Arena([n for n in numels for _ in range(4)], torch.float32)  # param, grad, exp_avg, exp_avg_sq
    sh = _Arena(numels[1:], torch.bfloat16)
    steps = torch.zeros(3, device=DEV)
    P, G, M, V = ([f32.view(4 * i + k) for i in range(3)] for k in range(4))
    S = [None, sh.view(0), sh.view(1)]
    arr = (K.AdamWTensor * 3)()
    ref = []
    for i, n in enumerate(numels):
        # |p| < 4 throughout: two fp32 roundings of p per step (decay, update), each at most half
        # an ulp = 2^-23 below 4, so a correct kernel stays within 6 * 2^-23 = 7.2e-7 of fp64
        p0 = _rand(n, seed=120 + i).clamp(-3.9, 3.9)
        P[i].copy_(p0); M[i].zero_(); V[i].zero_()  # noqa: E702
        arr[i].param, arr[i].grad = P[i].data_ptr(), G[i].data_ptr()
        arr[i].exp_avg, arr[i].exp_avg_sq = M[i].data_ptr(), V[i].data_ptr()
        arr[i].param_bf16 = S[i].data_ptr() if S[i] is not None else None
        arr[i].step = steps[i:i + 1].data_ptr()
        arr[i].numel = n
        ref.append((p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)))
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    for step in (1, 2, 3):
        for i, n in enumerate(numels):
            g = _rand(n, seed=130 + 10 * step + i) * step
            G[i].copy_(g)
            ref[i] = R.adamw_ref(*ref[i][:1], g, *ref[i][1:], step, lr, b1, b2, eps, wd)
        K.adamw(table, 3, max(numels), lr, b1, b2, eps, wd)
        torch.cuda.synchronize()
        assert steps.tolist() == [float(step)] * 3
        for i in range(3):
            rp, rm, rv = ref[i]
            perr = (P[i].double().cpu() - rp).abs().max().item()
            assert perr <= 1e-6, (step, i, perr)
            _close(M[i], rm, rm.abs().max().item(), f"step {step} exp_avg[{i}]")
            _close(V[i], rv, rv.abs().max().item(), f"step {step} exp_avg_sq[{i}]")
            if S[i] is not None:
                assert torch.equal(_bits(S[i]), _bits(P[i].cpu().to(torch.bfloat16)))
        assert f32.sentinels_intact() and sh.sentinels_intact()


# ---------------------------------------------------------------------------------------------
# convolution helpers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bn", [False, True])
@pytest.mark.parametrize("shape,Kpad", [((5, 3, 7, 7), 152), ((8, 16, 3, 3), None)])
def test_conv_weight_prep(dtype, with_bn, shape, Kpad):
    Cout, Cin, KH, KW = shape
    w = _rand(*shape, seed=140)
    bn = None
    if with_bn:
        var = _rand(Cout, seed=144).abs() + 0.1
        var[1] = 1e-7  # next to 0: eps decides the scale
        bn = (1 + 0.1 * _rand(Cout, seed=141), _rand(Cout, seed=142), _rand(Cout, seed=143), var)
    ow, ob = K.conv_weight_prep(w.to(DEV), dtype, Kpad=Kpad, bn=[t.to(DEV) for t in bn] if bn else None, eps=1e-5)
    rw, rb = R.conv_weight_prep_ref(w, Kpad, bn, 1e-5)
    Kd = KH * KW * Cin
    assert ow.dtype == dtype and tuple(ow.shape) == (Cout, Kpad or Kd) and ob.dtype == torch.float32
    assert (ow[:, Kd:] == 0).all()  # padding columns: exactly 0
    _close(ow, rw, rw.abs().max().item(), "weight")
    if with_bn:
        s = bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)
        _close(ob, rb, (bn[1].double().abs() + (bn[2].double() * s).abs()).max().item(), "bias")
    else:
        assert (ob == 0).all()
        if dtype == torch.float32:  # no scale: a permuted copy
            assert torch.equal(ow.cpu().double(), rw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_global_avgpool_many_slabs_few_positions(dtype):
    """C = 4100: more 64-channel slabs than the 64-block grid and a partial last slab; HW = 3: fewer
    positions than the four waves that split them"""
    N, HW, C = 2, 3, 4100
    x = _rand(N * HW, C, seed=150).to(dtype)
    out = K.global_avgpool(x.to(DEV), N, HW, C)
    assert out.dtype == torch.float32
    _close(out, R.global_avgpool_ref(x, N, HW, C), x.double().abs().max().item(), "avgpool")
