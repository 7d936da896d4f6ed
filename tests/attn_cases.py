"""TEST INFRASTRUCTURE ONLY. The case table of the attention reference tests, shared by the CPU tests
(tests/test_attention_ref_cpu.py: which kernels the table reaches, whether its bounds are attainable)
and the GPU test (tests/test_attention_kernels_gpu.py: every case against tests/attention_refs.py).

A case is a Spec. `plan_args` expands it into the AttnArgs of its launches (attn_args of
tests/test_attn_plan_cpu.py) for mmfd_debug_attn_plan; `make_inputs` expands it into the real tensors,
on the CPU and rounded to the case's dtype.

Batch and heads are B = 2, H = 3 throughout (six heads: a partial last workgroup at four heads per
workgroup, an odd head count everywhere), B = 4 where a bias repeats every 2 batch rows, B = 3 where two
heads per workgroup must not divide B*H. These are the smallest shapes at which the kernels can go
wrong, not the workload's."""
import ctypes
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

from mmfd import kernels as K
from oracle.dropout_hash import attn_keep_mask
from tests.test_attn_plan_cpu import attn_args

Spec = namedtuple("Spec", "dtype mode B H Lq Lk D feature kind")

# (Lq, Lk): heads per workgroup 4 with a ragged 16-row block | 2 | 1 with keys no multiple of 16 or 32 |
# more queries than keys | the split family's limit | the first length it refuses | the resident limit |
# the smallest streaming forward (its backward streams on the keys) | the backward streams on the queries alone
SHAPES = ((13, 29), (40, 50), (70, 100), (130, 65), (208, 208), (209, 209), (256, 256), (24, 257), (257, 40))
DIMS = (16, 32, 48, 64)

# feature -> options. rel: the relative bias's form ("shared" [H,Lq,Lk], "batch" [B,H,Lq,Lk], "mod"
# [2,H,Lq,Lk] read at b % 2); bits: the forward writes the dropout keep-bitmask and the backward reads it
Feat = namedtuple("Feat", "mask p bits rel drel cos planes", defaults=(False, 0.0, False, None, False, False, False))
FEATURES = {
    "plain": Feat(),
    "mask": Feat(mask=True),
    "drop": Feat(p=0.1),
    "drop_mask": Feat(mask=True, p=0.1),
    "bits": Feat(p=0.1, bits=True),
    "bits_mask": Feat(mask=True, p=0.1, bits=True),
    "rel": Feat(rel="shared"),
    "relb_mask": Feat(mask=True, rel="batch"),
    "relm_drop": Feat(p=0.1, rel="mod"),
    "drel": Feat(mask=True, rel="batch", drel=True),
    # beyond the first ten (the full product of tests/test_attention_ref_cpu.py is over those above)
    "rel_bits": Feat(mask=True, p=0.1, bits=True, rel="shared"),
    "cos": Feat(rel="shared", cos=True),
    "cosm_mask": Feat(mask=True, rel="mod", cos=True),
    "planes": Feat(planes=True),
}
FIRST_TEN = tuple(FEATURES)[:10]
RB_MOD = 2
COS_LOGIT_SCALES = (0.5, 2.3, 5.0, -1.0)  # cycled over the heads: 5.0 is past the clamp
COS_MAX_LOG = math.log(100.0)
RAMP_SLOPES = {"ramp0.1": 0.1, "ramp0.4": 0.4}  # log2 units per key
SEED, SALT = 4177, K.salt_of("test.attn.ref")
MIN_LIVE = 5  # live keys of a prefix-masked batch row, at least (see make_inputs): what lead_mask keeps


def spec_id(s):
    mode = "" if s.mode is None else "-" + s.mode
    return f"{s.dtype}{mode}-B{s.B}H{s.H}-{s.Lq}x{s.Lk}-D{s.D}-{s.feature}-{s.kind}"


def batch_of(feature, B=2):
    """B = 4 for a bias that repeats every RB_MOD = 2 batch rows: at B = 2 an [2, H, Lq, Lk] bias is the per-batch form"""
    return 2 * RB_MOD if FEATURES[feature].rel == "mod" else B


# ------------------------------------------------------------------------------------------------------
# plans
# ------------------------------------------------------------------------------------------------------
def plan_args(s):
    """[(bwd, AttnArgs)] of every distinct launch the GPU test makes for the case: forward and (not for
    cosine) backward; a keep-bitmask case also runs its hashed twin. The accumulate flags do not
    change a plan."""
    f = FEATURES[s.feature]
    kw = dict(key_bias=int(f.mask), p=f.p, rel_bias=f.rel or 0,
              rb_mod=RB_MOD if f.rel == "mod" else 0, cos=int(f.cos))
    shape = (s.dtype, s.B, s.H, s.Lq, s.Lk, s.D)
    out = []
    for bits in ((0, 1) if f.bits else (0,)):
        out.append((0, attn_args(0, *shape, drop_mask=bits, o_planes=int(f.planes), **kw)))
        if not f.cos:
            out.append((1, attn_args(1, *shape, drop_mask=bits, d_rel_bias=int(f.drel), dqkv_planes=int(f.planes), **kw)))
    return out


_plan_fn = None


def plan_lines(a, bwd, mode):
    """the lines of mmfd_debug_attn_plan for AttnArgs `a` under the fp32 attention mode `mode`"""
    global _plan_fn
    lib = K.load()
    if _plan_fn is None:
        _plan_fn = lib.mmfd_debug_attn_plan
        _plan_fn.restype = ctypes.c_int
        _plan_fn.argtypes = [ctypes.POINTER(K.AttnArgs), ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]
    buf = ctypes.create_string_buffer(4096)
    old = lib.mmfd_set_fp32_attn_mode(0 if mode == "native" else 1)
    try:
        rc = _plan_fn(ctypes.byref(a), bwd, buf, len(buf))
    finally:
        lib.mmfd_set_fp32_attn_mode(old)
    assert rc == 0, (rc, lib.mmfd_last_error_string().decode())
    return buf.value.decode().splitlines()


def kernels_of(s, mode=None):
    """the kernel instantiations the case launches, in order (mmfd_split3 excluded)"""
    names = []
    for bwd, a in plan_args(s):
        for line in plan_lines(a, bwd, mode or s.mode)[1:]:
            if not line.startswith("mmfd_split3"):
                names.append(line.split(" ")[0])
    return names


# ------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------
def _modes(dtype, B, H, Lq, Lk, D, feature, kind):
    """bf16: one spec. fp32: split and native, or split alone where both modes plan the same kernels."""
    if dtype == "bf16":
        return [Spec(dtype, None, B, H, Lq, Lk, D, feature, kind)]
    s = Spec(dtype, "split", B, H, Lq, Lk, D, feature, kind)
    if kernels_of(s, "split") == kernels_of(s, "native"):
        return [s]
    return [s, s._replace(mode="native")]


def full_product():
    """the nine shapes x D in {16, 32, 48, 64} x the first ten features, both dtypes, both fp32 modes
    where they differ: what the table is trimmed from"""
    return [s for dt in ("f32", "bf16") for Lq, Lk in SHAPES for D in DIMS for f in FIRST_TEN
            for s in _modes(dt, batch_of(f), 3, Lq, Lk, D, f, "randn")]


def build_table():
    t = []

    def add(dtype, Lq, Lk, D, feature, kind="randn", B=2):
        for s in _modes(dtype, batch_of(feature, B), 3, Lq, Lk, D, feature, kind):
            if s not in t:
                t.append(s)

    for dt in ("f32", "bf16"):
        # every shape at the two padded head dims, every feature
        # (dropout without a mask and the keep-bitmask with one: at alternating head dims)
        for i, (Lq, Lk) in enumerate(SHAPES):
            for D in (32, 64):
                for f in FIRST_TEN + ("rel_bits",):
                    if f in ("drop", "bits_mask") and (i + D // 32) % 2:
                        continue
                    add(dt, Lq, Lk, D, f)
        # head dims that are zero-padded to 32 / 64: one shape per family and heads-per-workgroup count
        for Lq, Lk in ((13, 29), (70, 100), (208, 208), (24, 257), (257, 40)):
            for D in (16, 48):
                for f in ("mask", "drop_mask", "bits", "drel"):
                    add(dt, Lq, Lk, D, f)
        # two heads per workgroup with B*H = 9
        for D in (32, 64):
            for f in ("plain", "mask", "rel", "relb_mask"):
                add(dt, 40, 50, D, f, B=3)
    # off-size head dims: fp32 dims that are no multiple of 8 leave the split family even in split mode
    for D, (Lq, Lk), f in ((8, (13, 29), "mask"), (8, (257, 40), "drop_mask"), (24, (70, 100), "bits_mask"),
                           (24, (24, 257), "relb_mask"), (40, (40, 50), "drop"), (40, (208, 208), "drel")):
        add("bf16", Lq, Lk, D, f)
    for D, (Lq, Lk), f in ((12, (13, 29), "drop_mask"), (12, (70, 100), "mask"), (12, (257, 40), "bits"),
                           (36, (40, 50), "mask"), (36, (208, 208), "drop_mask"), (36, (24, 257), "drel")):
        add("f32", Lq, Lk, D, f)
    # rising logits: every resident bf16 forward (fixed modes 0 / 1 / 2, relative bias; 4 / 2 / 1 heads per
    # workgroup) at both slopes, the streaming kernels and fp32 at the steep one
    for kind in RAMP_SLOPES:
        for D in (32, 64):
            for Lq, Lk in ((13, 29), (40, 50), (70, 100), (256, 256)):
                for f in ("plain", "mask", "drop", "rel"):
                    add("bf16", Lq, Lk, D, f, kind)
    for D in (32, 64):
        for Lq, Lk in ((70, 100), (208, 208), (24, 257), (257, 40)):
            for f in ("plain", "drop_mask"):
                add("f32", Lq, Lk, D, f, "ramp0.4")
        add("bf16", 24, 257, D, "drop_mask", "ramp0.4")
        add("bf16", 257, 40, D, "mask", "ramp0.4")
    # key masks that are no prefixes
    for dt in ("f32", "bf16"):
        for (Lq, Lk), D in (((13, 29), 32), ((70, 100), 64), ((208, 208), 32), ((256, 256), 64), ((24, 257), 32),
                            ((257, 40), 64)):
            for f in ("mask", "drop_mask", "bits_mask"):
                add(dt, Lq, Lk, D, f, "lead_mask")
    # cosine attention: bf16 forward on the resident relative-bias kernels
    for D in (16, 32, 64):
        for Lq, Lk in ((13, 29), (40, 50), (70, 100), (256, 256)):
            add("bf16", Lq, Lk, D, "cos")
    add("bf16", 40, 50, 32, "cos", B=3)
    add("bf16", 13, 29, 32, "cosm_mask")
    add("bf16", 70, 100, 64, "cosm_mask")
    # split planes beside the fp32 results: one shape in each family, at D = 32 and D = 64
    for L in (70, 256, 257):
        for D in (32, 64):
            add("f32", L, L, D, "planes")
    return t


_table = None


def table():
    global _table
    if _table is None:
        _table = build_table()
    return _table


# ------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------
def torch_dtype(s):
    return torch.float32 if s.dtype == "f32" else torch.bfloat16


def make_inputs(s):
    """CPU tensors of the case: q [B, Lq, H*D], k, v [B, Lk, H*D], dout rounded to the case's dtype; fp32
    key_bias [B, Lk], rel_bias, cos_logit_scale or None; keep: the oracle's keep mask (bool numpy) or
    None; scale."""
    f = FEATURES[s.feature]
    B, H, Lq, Lk, D = s.B, s.H, s.Lq, s.Lk, s.D
    g = torch.Generator().manual_seed(zlib.crc32(spec_id(s).encode()))
    rn = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    q, k, v, dout = rn(B, Lq, H, D), rn(B, Lk, H, D), rn(B, Lk, H, D), rn(B, Lq, H, D)
    live = None
    if f.mask:
        pos = torch.arange(Lk)[None, :]
        if s.kind == "lead_mask":
            # batch row 0 masks its first Lk//2 + 3 keys (whole leading chunks masked: the real maximum
            # arrives late), row 1 keeps only its first 5 (whole trailing chunks masked)
            assert B == 2
            live = torch.stack([pos[0] >= Lk // 2 + 3, pos[0] < 5])
        else:
            # prefix masks: no batch row fully masked, row 0 never complete. At least MIN_LIVE keys: with
            # one live key every gradient is 0 in exact arithmetic (dS = P (dP - delta), delta = dP), the
            # slice's bound shrinks to atol alone, and delta = rowsum(dO * O) from an O rounded to bf16
            # already misses it — in the CPU emulation as on the GPU
            lens = torch.randint(min(MIN_LIVE, Lk), Lk + 1, (B,), generator=g)
            lens[0] = min(int(lens[0]), Lk - 1)
            live = pos < lens[:, None]
        assert bool(live.any(1).all()) and not bool(live.all())
    else:
        assert s.kind != "lead_mask"
    if s.kind in RAMP_SLOPES:
        # logits that rise along the keys by `slope` log2 units per key: scale * q.k_j ~ 4 r_j. One-sided
        # and anchored at each batch row's last live key: the keys that carry weight have small
        # components (a two-sided ramp, or a prefix mask that cuts a ramp anchored at Lk - 1, makes dq and
        # dk a cancellation of large terms, which no bf16 arithmetic resolves to the bound)
        u = torch.nn.functional.normalize(rn(H, D), dim=-1)
        gain = 2.0 * D ** 0.25
        last = (live.sum(1) - 1 if live is not None else torch.full((B,), Lk - 1)).to(torch.float32)
        j = torch.arange(Lk, dtype=torch.float32)[None, :]
        r = (torch.minimum(j, last[:, None]) - last[:, None]) * (RAMP_SLOPES[s.kind] / (4.0 * math.log2(math.e)))
        q = q + gain * u
        k = k + gain * u * r[:, :, None, None]
    else:
        assert s.kind in ("randn", "lead_mask"), s.kind
    dt = torch_dtype(s)
    q, k, v, dout = (t.reshape(t.shape[0], t.shape[1], H * D).to(dt) for t in (q, k, v, dout))
    key_bias = torch.where(live, 0.0, -10000.0).to(torch.float32) if live is not None else None
    rel_bias = None
    if f.rel:
        assert f.rel != "mod" or (B % RB_MOD == 0 and B > RB_MOD), B
        lead = {"shared": (), "batch": (B,), "mod": (RB_MOD,)}[f.rel]
        rel_bias = rn(*lead, H, Lq, Lk).contiguous()
    cos = None
    if f.cos:
        cos = torch.tensor([COS_LOGIT_SCALES[h % len(COS_LOGIT_SCALES)] for h in range(H)], dtype=torch.float32)
    keep = attn_keep_mask(SEED, SALT, (B, H, Lq, Lk), f.p) if f.p > 0 else None
    return dict(q=q, k=k, v=v, dout=dout, key_bias=key_bias, rel_bias=rel_bias, cos_logit_scale=cos, keep=keep,
                p=f.p, scale=1.0 if f.cos else D ** -0.5, cos_max_log=COS_MAX_LOG if f.cos else None)


def reference(s, x):
    """tests/attention_refs.attention_ref on the inputs `x` of make_inputs"""
    from tests.attention_refs import attention_ref
    f = FEATURES[s.feature]
    return attention_ref(x["q"], x["k"], x["v"], s.H, x["scale"], key_bias=x["key_bias"], rel_bias=x["rel_bias"],
                         keep=x["keep"], p=x["p"], cos_logit_scale=x["cos_logit_scale"], cos_max_log=x["cos_max_log"],
                         dout=None if f.cos else x["dout"], want_d_rel_bias=f.drel)


def pack_keep_bits(keep, Lk):
    """keep mask [..., Lk] (bool) -> the drop_mask words [rows, ceil(Lk/32)] (uint32), bit k % 32 of word k // 32"""
    W = (Lk + 31) // 32
    k = np.zeros(keep.shape[:-1] + (W * 32,), dtype=np.uint64)
    k[..., :Lk] = keep
    k = k.reshape(-1, W, 32)
    return (k << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
