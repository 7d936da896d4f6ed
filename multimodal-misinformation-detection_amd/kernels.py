"""Host bindings of libmmfd_hip.so (the C ABI declared in include/mmfd.h) plus thin torch-tensor
wrappers. PyTorch only provides device memory, the current HIP stream and autograd plumbing; every
computation below is a launch of one of our gfx950 kernels.

Two layers over the same C ABI:
  * the training / retrieval hot path (GEMM, attention, LayerNorm, cross entropy, AdamW, sequence
    mean, cast, cosine scores, top-k) goes through the PyTorch custom ops torch.ops.mmfd.* that
    libmmfd_torch.so registers (csrc/torch_ops.cpp: TORCH_LIBRARY schemas with declared
    mutations, CUDA/HIP dispatch; fake kernels in mmfd/ops.py);
  * the remaining entry points (encoder embeddings, ResNet / Swinv2 / DeBERTa helpers,
    preprocessing) are called through ctypes.

There is no fallback: if either shared library is missing or cannot be loaded, every op raises
`NativeLibraryError` (the product path must never silently run on something else).
"""
from __future__ import annotations

import ctypes
import os
import weakref
import zlib

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMFD_LIB_PATH") or os.path.join(_HERE, "libmmfd_hip.so")  # env override: A/B runs of two builds (tools/ab.sh)
TORCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libmmfd_torch.so")

F32, BF16, F16 = 0, 1, 2
ABI_VERSION = 3  # include/mmfd.h MMFD_ABI_VERSION: the layout of the argument structs below
COS_PAIR, COS_NORMALIZED, COS_ROUND_F16 = 0, 1, 4
MMFD_ERR_INVALID = 1000  # include/mmfd.h: what a failed query function (-1) is reported as
ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_BWD, ACT_RELU_BWD, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4, 5, 6
# GELU whose aux keeps gelu'(pre-activation), and its backward (out *= aux): the training FFNs
ACT_GELU_D, ACT_MUL_AUX = 7, 8


class NativeLibraryError(RuntimeError):
    pass


class EpilogueArgs(ctypes.Structure):
    _fields_ = [
        ("bias", ctypes.c_void_p),
        ("residual", ctypes.c_void_p), ("ldr", ctypes.c_int64),
        ("aux", ctypes.c_void_p), ("ldaux", ctypes.c_int64),
        ("act", ctypes.c_int),
        ("dropout_p", ctypes.c_float),
        ("seed", ctypes.c_void_p),
        ("salt", ctypes.c_uint64),
        ("residual_first", ctypes.c_int),
        ("out_planes", ctypes.c_void_p),
    ]


class _Sized(ctypes.Structure):
    """argument structs that start with `struct_size` (include/mmfd.h, ABI version 2): set on
    construction, so the library can refuse a caller built against another layout"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        if "struct_size" not in kw:
            self.struct_size = ctypes.sizeof(self)


class GemmArgs(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_int64),
        ("dtype", ctypes.c_int), ("trans_a", ctypes.c_int), ("trans_b", ctypes.c_int),
        ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64),
        ("A", ctypes.c_void_p), ("lda", ctypes.c_int64),
        ("B", ctypes.c_void_p), ("ldb", ctypes.c_int64),
        ("C", ctypes.c_void_p), ("ldc", ctypes.c_int64), ("c_dtype", ctypes.c_int),
        ("alpha", ctypes.c_float), ("beta", ctypes.c_float),
        ("ep", EpilogueArgs),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("splits", ctypes.c_int),
        ("a_rowsum", ctypes.c_void_p), ("a_rowsum_beta", ctypes.c_float),
        ("a_planes", ctypes.c_void_p), ("b_planes", ctypes.c_void_p),
        ("a_planes_only", ctypes.c_int), ("b_planes_only", ctypes.c_int),
        ("conv", ctypes.c_void_p),  # const mmfd_conv_geom* (ABI 3): implicit-GEMM convolution
    ]


class ConvGeomArgs(ctypes.Structure):
    """include/mmfd.h mmfd_conv_geom"""
    _fields_ = [("N", ctypes.c_int64), ("H", ctypes.c_int64), ("W", ctypes.c_int64), ("C", ctypes.c_int64),
                ("KH", ctypes.c_int), ("KW", ctypes.c_int), ("stride", ctypes.c_int), ("pad", ctypes.c_int),
                ("Ho", ctypes.c_int64), ("Wo", ctypes.c_int64)]


class AttnArgs(_Sized):
    _fields_ = [
        ("struct_size", ctypes.c_int64),
        ("dtype", ctypes.c_int),
        ("B", ctypes.c_int64), ("H", ctypes.c_int64), ("Lq", ctypes.c_int64), ("Lk", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("scale", ctypes.c_float),
        ("q", ctypes.c_void_p), ("q_sb", ctypes.c_int64), ("q_st", ctypes.c_int64),
        ("k", ctypes.c_void_p), ("k_sb", ctypes.c_int64), ("k_st", ctypes.c_int64),
        ("v", ctypes.c_void_p), ("v_sb", ctypes.c_int64), ("v_st", ctypes.c_int64),
        ("o", ctypes.c_void_p), ("o_sb", ctypes.c_int64), ("o_st", ctypes.c_int64),
        ("lse", ctypes.c_void_p),
        ("key_bias", ctypes.c_void_p),
        ("rel_bias", ctypes.c_void_p),
        ("dropout_p", ctypes.c_float), ("seed", ctypes.c_void_p), ("salt", ctypes.c_uint64),
        ("dout", ctypes.c_void_p), ("do_sb", ctypes.c_int64), ("do_st", ctypes.c_int64),
        ("dq", ctypes.c_void_p), ("dq_sb", ctypes.c_int64), ("dq_st", ctypes.c_int64),
        ("dk", ctypes.c_void_p), ("dk_sb", ctypes.c_int64), ("dk_st", ctypes.c_int64),
        ("dv", ctypes.c_void_p), ("dv_sb", ctypes.c_int64), ("dv_st", ctypes.c_int64),
        ("delta", ctypes.c_void_p),
        ("d_rel_bias", ctypes.c_void_p),
        ("accumulate_dq", ctypes.c_int),
        ("accumulate_dkv", ctypes.c_int),
        ("rel_bias_sb", ctypes.c_int64),
        ("rel_bias_mod", ctypes.c_int64),
        ("cos_logit_scale", ctypes.c_void_p),
        ("cos_max_log", ctypes.c_float),
        ("dqkv_planes", ctypes.c_void_p), ("planes_only", ctypes.c_int),
        ("o_planes", ctypes.c_void_p),
        ("drop_mask", ctypes.c_void_p),
    ]


class AdamWTensor(ctypes.Structure):
    _fields_ = [
        ("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
        ("exp_avg_sq", ctypes.c_void_p), ("param_bf16", ctypes.c_void_p), ("step", ctypes.c_void_p),
        ("numel", ctypes.c_int64),
    ]


_VP, _I64, _I, _F, _U64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint64

# name -> (restype, argtypes); every symbol declared in include/mmfd.h
SIGNATURES = {
    "mmfd_last_error_string": (ctypes.c_char_p, []),
    "mmfd_version": (_I, []),
    "mmfd_dropout_hash": (ctypes.c_uint32, [_U64, _U64, _U64]),
    "mmfd_gemm": (_I, [ctypes.POINTER(GemmArgs), _VP]),
    "mmfd_gemm_workspace_bytes": (_I64, [ctypes.POINTER(GemmArgs)]),
    "mmfd_set_fp32_gemm_mode": (_I, [_I]),
    "mmfd_set_fp32_attn_mode": (_I, [_I]),
    "mmfd_gemm_splits": (_I, [ctypes.POINTER(GemmArgs)]),
    "mmfd_gemm_runs_split": (_I, [ctypes.POINTER(GemmArgs)]),
    "mmfd_set_g4_mode": (_I, [_I]),
    "mmfd_set_g4_persist": (_I, [_I]),
    "mmfd_transpose": (_I, [_I, _I64, _I64, _VP, _I64, _VP, _I64, _VP]),
    "mmfd_set_g4_kmax": (_I64, [_I64]),
    "mmfd_split3": (_I, [_I64, _I64, _VP, _I64, _VP, _VP]),
    "mmfd_layernorm_fwd_split": (_I, [_I64, _I64, _VP, _I64, _VP, _VP, _F, _VP, _I64, _VP, _VP, _VP, _VP]),
    "mmfd_layernorm_bwd_split": (_I, [_I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP,
                                      _F, _VP, _F, _VP, _U64, _VP, _I64, _VP, _VP]),
    "mmfd_colsum": (_I, [_I, _I64, _I64, _VP, _I64, _VP, _F, _VP, _I64, _VP]),
    "mmfd_attn_fwd": (_I, [ctypes.POINTER(AttnArgs), _VP]),
    "mmfd_attn_bwd": (_I, [ctypes.POINTER(AttnArgs), _VP]),
    "mmfd_attn_bwd_ds": (_I, [ctypes.POINTER(AttnArgs), _VP, _VP]),
    "mmfd_layernorm_fwd": (_I, [_I, _I64, _I64, _VP, _I64, _VP, _VP, _F, _VP, _I64, _VP, _VP, _VP]),
    "mmfd_layernorm_bwd": (_I, [_I, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP, _I64,
                                _VP, _VP, _F, _VP, _F, _VP, _U64, _VP, _I64, _VP]),
    "mmfd_seq_mean_fwd": (_I, [_I, _I64, _I64, _I64, _VP, _VP, _I64, _VP]),
    "mmfd_seq_mean_bwd": (_I, [_I, _I64, _I64, _I64, _VP, _I64, _VP, _VP]),
    "mmfd_xent_fwd_bwd": (_I, [_I, _I64, _I64, _VP, _VP, _VP, _I64, _VP, _I, _VP, _VP, _VP]),
    "mmfd_embed_ln_fwd": (_I, [_I, _I64, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _F, _VP, _VP, _VP, _VP,
                               _F, _VP, _U64, _VP]),
    "mmfd_embed_bwd": (_I, [_I, _I64, _I64, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _I64, _VP]),
    "mmfd_embed_bwd_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "mmfd_mask_to_bias": (_I, [_I64, _VP, _VP, _F, _VP]),
    "mmfd_embed_ln_fwd_ex": (_I, [_I, _I64, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _F, _VP, _VP, _VP, _VP,
                                  _F, _VP, _U64, _VP]),
    "mmfd_position_ids": (_I, [_I64, _I64, _VP, _I64, _VP, _VP]),
    "mmfd_conv_weight_prep": (_I, [_I, _I64, _I64, _I64, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _F, _VP, _VP, _VP]),
    "mmfd_im2col_nhwc": (_I, [_I, _I64, _I64, _I64, _I64, _I, _I, _I, _I, _I64, _I64, _I64, _VP, _VP, _VP]),
    "mmfd_im2col_nchw": (_I, [_I, _I64, _I64, _I64, _I64, _I, _I, _I, _I, _I64, _I64, _I64, _VP, _VP, _VP]),
    "mmfd_maxpool_nhwc": (_I, [_I, _I64, _I64, _I64, _I64, _I, _I, _I, _I64, _I64, _VP, _VP, _VP]),
    "mmfd_global_avgpool": (_I, [_I, _I64, _I64, _I64, _VP, _VP, _VP]),
    "mmfd_rel_bias": (_I, [_I64, _I64, _I64, _VP, _VP, _VP, _VP]),
    "mmfd_deberta_rel_bias": (_I, [_I, _I64, _I64, _I64, _VP, _VP, _I64, _VP, _VP, _F, _VP, _VP]),
    "mmfd_deberta_rel_bias_bwd": (_I, [_I, _I64, _I64, _I64, _VP, _VP, _VP, _F, _VP, _VP, _I64, _VP]),
    "mmfd_mask_rows": (_I, [_I, _I64, _I64, _VP, _I64, _VP, _VP]),
    "mmfd_attn_fill_masked_rows": (_I, [_I, _I64, _I64, _I64, _I64, _VP, _I64, _I64, _VP, _I64, _I64, _VP, _VP]),
    "mmfd_attn_fill_masked_rows_bwd": (_I, [_I, _I, _I64, _I64, _I64, _I64, _VP, _I64, _I64, _VP, _I64, _I64, _VP, _VP,
                                            _VP]),
    "mmfd_patchify": (_I, [_I, _I64, _I64, _I64, _I64, _I64, _VP, _VP, _VP]),
    "mmfd_vit_tokens_fwd": (_I, [_I, _I64, _I64, _I64, _VP, _VP, _VP, _VP, _VP]),
    "mmfd_vit_tokens_bwd": (_I, [_I, _I64, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "mmfd_adamw": (_I, [_I, _VP, _I64, _F, _F, _F, _F, _F, _VP]),
    "mmfd_cast": (_I, [_I, _I, _I64, _VP, _VP, _VP]),
    "mmfd_zero": (_I, [_VP, _I64, _VP]),
    "mmfd_axpby": (_I, [_I, _I64, _F, _VP, _F, _VP, _VP, _VP]),
    "mmfd_dropout": (_I, [_I, _I64, _VP, _VP, _F, _VP, _U64, _VP]),
    "mmfd_seed_advance": (_I, [_VP, _VP]),
    "mmfd_act_bwd": (_I, [_I, _I64, _VP, _VP, _I, _F, _VP, _U64, _VP, _VP]),
    "mmfd_cosine_scores": (_I, [_I, _I64, _I64, _I64, _VP, _I64, _VP, _I64, _I, _F, _VP, _I64, _VP]),
    "mmfd_topk_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "mmfd_topk": (_I, [_I64, _I64, _VP, _I64, _I64, _VP, _VP, _VP, _I64, _VP]),
    "mmfd_resize_normalize": (_I, [_I64, _VP, _I64, _I64, _VP, _VP, _I64, _I64, ctypes.POINTER(ctypes.c_float),
                                   ctypes.POINTER(ctypes.c_float), _VP, _VP]),
    "mmfd_layernorm_fwd_res": (_I, [_I, _I64, _I64, _VP, _I64, _VP, _VP, _F, _VP, _I64, _VP, _I64, _VP, _VP, _VP]),
    "mmfd_row_gather": (_I, [_I64, _I64, _I64, _I64, _I64, _VP, _VP, _VP, _VP]),
    "mmfd_swin_cpb": (_I, [_I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mmfd_swin_bias": (_I, [_I64, _I64, _I64, _VP, _VP, _VP, _VP, _VP]),
    "mmfd_swin_qk_norm": (_I, [_I, _I64, _I64, _I64, _VP, _I64, _VP, _F, _VP]),
    "mmfd_swin_qk_norm_train": (_I, [_I, _I64, _I64, _I64, _VP, _I64, _VP, _F, _VP, _VP]),
    "mmfd_swin_qk_norm_bwd_workspace_bytes": (_I64, [_I64, _I64]),
    "mmfd_swin_qk_norm_bwd": (_I, [_I, _I64, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _F, _VP, _VP, _I64, _VP]),
    "mmfd_attn_bwd_bias_sum": (_I, [ctypes.POINTER(AttnArgs), _VP, _VP]),
    "mmfd_swin_bias_bwd": (_I, [_I64, _I64, _I64, _I64, _VP, _VP, _VP, _VP, _VP]),
    "mmfd_swin_cpb_bwd": (_I, [_I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mmfd_attn_decode_splits": (_I, [_I64, _I64, _I64]),
    "mmfd_attn_decode_workspace_bytes": (_I64, [_I64, _I64, _I64, _I64]),
    "mmfd_attn_decode": (_I, [_I, _I64, _I64, _I64, _I64, _F, _VP, _I64, _VP, _I64, _I64, _VP, _I64, _I64, _VP, _I64,
                              _VP, _I64, _VP]),
    "mmfd_attn_decode_grouped": (_I, [_I, _I64, _I64, _I64, _I64, _I64, _F, _VP, _I64, _VP, _I64, _I64, _VP, _I64, _I64, _VP,
                                      _I64, _VP, _I64, _VP]),
    "mmfd_lm_head_argmax_workspace_bytes": (_I64, [_I, _I64, _I64, _I64]),
    "mmfd_lm_head_argmax_slab": (_I64, [_I, _I64, _I64, _I64]),
    "mmfd_lm_head_argmax": (_I, [_I, _I64, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _I64, _VP, _I64, _VP]),
    "mmfd_lm_head_argmax_wide_workspace_bytes": (_I64, [_I, _I64, _I64, _I64]),
    "mmfd_lm_head_argmax_wide": (_I, [_I, _I64, _I64, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _I64, _VP, _I64, _VP]),
    "mmfd_greedy_select": (_I, [_I64, _VP, _VP, _I64, _VP, _I64, _I64, _VP, _I64, _VP]),
    "mmfd_beam_select_slab": (_I64, [_I64]),
    "mmfd_beam_select_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "mmfd_beam_select": (_I, [_I64, _I64, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "mmfd_beam_update": (_I, [_I64, _I64, _I64, _I64, _I64, _I, _I, _I64, _F] + [_VP] * 12 + [_I64, _VP]),
    "mmfd_beam_reorder": (_I, [_I64, _I64, _I64, _I64, _I64, _VP, _VP, _VP, _VP]),
    "mmfd_sample_select_resident_max": (_I64, []),
    "mmfd_sample_select_workspace_bytes": (_I64, [_I64, _I64]),
    "mmfd_sample_select": (_I, [_I64, _I64, _VP, _I64, _F, _I64, _F, _VP, _I64, _VP, _VP, _I64, _VP, _VP, _I64, _VP]),
    "mmfd_row_log_softmax_workspace_bytes": (_I64, [_I64, _I64]),
    "mmfd_row_log_softmax": (_I, [_I64, _I64, _VP, _I64, _VP, _I64, _VP]),
    "mmfd_beam_select_logprobs": (_I, [_I64, _I64, _I64, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _I64, _VP]),
    "mmfd_logits_process": (_I, [_I64, _I64, _VP, _I64, _VP, _I64, _I64, _I, _I64, _F, _I64, _I, _I64, _VP, _I64, _VP]),
    "mmfd_row_argmax": (_I, [_I64, _I64, _VP, _I64, _VP, _VP]),
    "mmfd_vocab_xent_fwd": (_I, [_I64, _I64, _VP, _I64, _VP, _F, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mmfd_vocab_xent_bwd": (_I, [_I, _I64, _I64, _VP, _I64, _VP, _VP, _VP, _F, _VP, _VP, _I64, _VP, _I64, _VP]),
}

_lib = None


def load(path: str = LIB_PATH):
    """Load libmmfd_hip.so (after torch, so the HIP runtime torch already loaded is reused)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeLibraryError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - depends on the box
        raise NativeLibraryError(f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.mmfd_version() != ABI_VERSION:
        raise NativeLibraryError(f"{path} implements ABI version {lib.mmfd_version()}, these bindings version "
                                 f"{ABI_VERSION}: rebuild (python -c 'import __graft_entry__ as g; g.build()')")
    if not os.path.exists(TORCH_LIB_PATH):
        raise NativeLibraryError(f"{TORCH_LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        torch.ops.load_library(TORCH_LIB_PATH)  # registers torch.ops.mmfd.* (needs libmmfd_hip.so loaded)
    except (OSError, RuntimeError) as e:  # pragma: no cover - depends on the box
        raise NativeLibraryError(f"cannot load {TORCH_LIB_PATH}: {e}") from e
    from . import ops  # noqa: F401  (fake kernels of the custom ops)
    _lib = lib
    return lib


def _ops():
    if _lib is None:
        load()
    return torch.ops.mmfd


def _salt(salt):
    """uint64 call-site salt -> the int64 of the op schema (same bits)"""
    salt = int(salt) & 0xFFFFFFFFFFFFFFFF
    return salt - (1 << 64) if salt >= (1 << 63) else salt


def lib():
    return _lib if _lib is not None else load()


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().mmfd_last_error_string().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {dt} (fp32 / bf16)")


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("mmfd kernels need tensors on the GPU (HIP device)")


def salt_of(name: str) -> int:
    """Stable 64-bit call-site id for counter-based dropout."""
    b = name.encode()
    return (zlib.crc32(b) << 32) | zlib.crc32(b[::-1] + b"mmfd")


# ------------------------------------------------------------------------------------------------
# step seed (device resident so that captured graphs see it advance)
# ------------------------------------------------------------------------------------------------
class Seed:
    def __init__(self, value: int = 0, device=None):
        self.t = torch.tensor([value], dtype=torch.int64, device=device or "cuda")

    def ptr(self):
        return _ptr(self.t)

    def advance(self):
        _check(lib().mmfd_seed_advance(self.ptr(), _stream()), "seed_advance")

    def set(self, value: int):
        self.t.fill_(value)

    def fork(self):
        """Snapshot of the current value for one forward/backward pair (the kernels read the seed
        at launch time), then advance this seed for the next forward."""
        s = Seed.__new__(Seed)
        s.t = self.t.clone()
        self.advance()
        return s


# ------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------
def _ld(t: torch.Tensor) -> int:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"operand must be a 2-D row-major view, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0)


_PROBE = None


class GemmProbe:
    """Records HIP events around every MFMA-path GEMM launch while active (bench.py roofline):
    per kernel instantiation, the algorithmic FLOPs (2*M*N*K) and the launch's device time."""

    def __init__(self):
        self.records = []

    def __enter__(self):
        global _PROBE
        _PROBE = self
        return self

    def __exit__(self, *exc):
        global _PROBE
        _PROBE = None

    def summary(self):
        """per kernel instantiation {launches, flops, ms}"""
        torch.cuda.synchronize()
        out = {}
        for key, flops, e0, e1 in self.records:
            ms = e0.elapsed_time(e1)
            d = out.setdefault(key, {"launches": 0, "flops": 0, "ms": 0.0})
            d["launches"] += 1
            d["flops"] += flops
            d["ms"] += ms
        return out


def _x6(a):
    """whether mmfd_gemm runs this fp32 product on split bf16 operands: 0 no, 2 fused-plane kernel,
    1 segmented kernel (the library's own decision, mmfd_gemm_runs_split)"""
    return lib().mmfd_gemm_runs_split(ctypes.byref(a))


_FP32_MODE = None


def set_fp32_gemm_mode(mode):
    """fp32 GEMMs: 'split' (bf16 operand planes, six MFMA products, fp32 accumulation; the default)
    or 'native' (fp32 MFMA). Returns the previous mode name."""
    global _FP32_MODE
    code = {"native": 0, "split": 1}[mode]
    old = lib().mmfd_set_fp32_gemm_mode(code)
    _check(0 if old >= 0 else old, "mmfd_set_fp32_gemm_mode")
    _FP32_MODE = code
    return {0: "native", 1: "split"}[old]


def set_fp32_attn_mode(mode):
    """fp32 attention: 'split' (bf16 operand planes, six MFMA products per product, fp32
    accumulation; the default) or 'native' (fp32 MFMA). Returns the previous mode name."""
    code = {"native": 0, "split": 1}[mode]
    old = lib().mmfd_set_fp32_attn_mode(code)
    _check(0 if old >= 0 else old, "mmfd_set_fp32_attn_mode")
    return {0: "native", 1: "split"}[old]


_G4_MODES = {"off": 0, "on": 1, "gelu": 2}


def set_g4_mode(mode=None, kmax=None):
    """The four-wave bf16 forward GEMM (gemm_g4.hip): 'off', 'on' or 'gelu' (default: the FFN1 GELU
    epilogues too), and the largest K it takes. Returns the previous (mode, kmax); None leaves a
    setting as it is (A/B measurements and tests: set between launches, not per stream)."""
    old = lib().mmfd_set_g4_mode(-1 if mode is None else _G4_MODES[mode])
    _check(0 if old >= 0 else old, "mmfd_set_g4_mode")
    old_k = lib().mmfd_set_g4_kmax(0 if kmax is None else int(kmax))
    return {v: k for k, v in _G4_MODES.items()}[old], int(old_k)


def set_g4_persist(on=None):
    """the four-wave GEMM's persistent grid (default True) or one workgroup per tile; returns the
    previous setting (None only queries)"""
    old = lib().mmfd_set_g4_persist(-1 if on is None else int(bool(on)))
    _check(0 if old >= 0 else old, "mmfd_set_g4_persist")
    return bool(old)


_PLAN_BUF = None


def _gemm_plan(a, whole_workspace=False):
    """the launch plan mmfd_gemm makes for `a` with the workspace it carries, or with the one
    mmfd_gemm_workspace_bytes asks for, as the callers here supply (csrc/gemm.hip
    mmfd_debug_gemm_plan; host arithmetic only): (path, kernel name as GemmProbe keys it), or
    (None, None) when the library refuses the call"""
    global _PLAN_BUF
    if whole_workspace:
        a.workspace_bytes = lib().mmfd_gemm_workspace_bytes(ctypes.byref(a))
        a.workspace = _PLACEHOLDER if a.workspace_bytes > 0 else None
    fn = lib().mmfd_debug_gemm_plan
    if _PLAN_BUF is None:
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(GemmArgs), ctypes.c_char_p, ctypes.c_int64]
        _PLAN_BUF = ctypes.create_string_buffer(2048)
    if fn(ctypes.byref(a), _PLAN_BUF, len(_PLAN_BUF)) != 0 or not _PLAN_BUF.value:
        return None, None
    head, *launches = _PLAN_BUF.value.decode().splitlines()
    main = next(l for l in launches if not l.startswith("split3_kernel"))
    name = main.split(" grid=")[0].split(" tiles=")[0]
    return head.split(" ")[0][len("path="):], name + (" (split-K)" if " ws=0," in head else "")


_PLACEHOLDER = 1 << 20  # a 16-B aligned address for tensors that do not exist yet: a plan never dereferences it


def g4_takes(x2d, W, act, residual=None, dropout_p=0.0):
    """whether the four-wave GEMM runs x2d @ W^T (bf16 nn.Linear forward) with a bias / activation
    epilogue — asked of the library's launch plan; blocks.linear saves the GELU derivative
    (MMFD_ACT_GELU_D) only for products it takes (elsewhere GELU_D runs through a split-K slab and
    the reduce, which costs more than the backward's erf it saves). Epilogues with a residual or
    dropout never save one: False."""
    if residual is not None or dropout_p > 0 or x2d.dtype != W.dtype:
        return False
    a = GemmArgs()
    a.dtype = a.c_dtype = dtype_code(x2d.dtype)
    (a.M, a.K), a.N = x2d.shape, W.shape[0]
    a.A, a.lda, a.B, a.ldb = x2d.data_ptr(), _ld(x2d), W.data_ptr(), _ld(W)
    a.C, a.ldc, a.alpha = _PLACEHOLDER, a.N, 1.0
    a.ep.act = int(act)
    if act in (ACT_GELU_BWD, ACT_RELU_BWD, ACT_GELU_D, ACT_MUL_AUX):
        a.ep.aux, a.ep.ldaux = _PLACEHOLDER, a.N
    return _gemm_plan(a, whole_workspace=True)[0] == "g4"


def g4_mode():
    """(mode, kmax) the library currently uses for the four-wave GEMM"""
    return set_g4_mode()


def fp32_gemm_mode():
    global _FP32_MODE
    if _FP32_MODE is None:  # the library's load-time default (env MMFD_FP32_GEMM)
        old = lib().mmfd_set_fp32_gemm_mode(1)
        lib().mmfd_set_fp32_gemm_mode(old)
        _FP32_MODE = old
    return _FP32_MODE


def gemm(A, B, *, trans_a=False, trans_b=False, out=None, out_dtype=None, alpha=1.0, beta=0.0, bias=None,
         residual=None, act=ACT_NONE, aux=None, dropout_p=0.0, seed=None, salt=0, splits=0, a_rowsum=None,
         a_rowsum_beta=0.0, residual_first=False, a_planes=None, b_planes=None, out_planes=None, write_out=True):
    """C = epilogue(alpha * op(A) @ op(B)) with op(A) = A or A^T ([M,K]) and op(B) = B^T ([N,K] stored,
    nn.Linear weight) when trans_b=False, else B ([K,N] stored). `a_rowsum` (fp32 [M]) additionally
    receives a_rowsum_beta * a_rowsum + sum_k op(A)[m, k] (bias gradient of a weight-gradient GEMM).
    `a_planes` / `b_planes`: split3() of the stored fp32 A / B, reused by the split-operand fp32 GEMM.
    `out_planes` (bf16 [3, M, N], fp32 output only): the output's split planes, written by the
    epilogue; with write_out=False instead of `out` (which then only carries the shape and stays
    unwritten — only for outputs read by split-operand GEMMs alone, see x6_ok)."""
    _require_cuda(A, B, out, bias, residual, aux)
    if A.dtype != B.dtype:
        raise TypeError(f"gemm operands must share a dtype ({A.dtype} vs {B.dtype})")
    if trans_a:
        K, M = A.shape
    else:
        M, K = A.shape
    if trans_b:
        K2, N = B.shape
    else:
        N, K2 = B.shape
    if K != K2:
        raise ValueError(f"gemm inner dims differ: {K} vs {K2}")
    if out is None:
        out = torch.empty((M, N), device=A.device, dtype=out_dtype or A.dtype)
    if tuple(out.shape) != (M, N):
        raise ValueError(f"gemm out shape {tuple(out.shape)} != {(M, N)}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous fp32 vector of length N")
    for t in (residual, aux):
        if t is not None and (t.dtype != out.dtype or tuple(t.shape) != (M, N)):
            raise ValueError("residual/aux must match the output shape and dtype")
    if dropout_p > 0 and seed is None:
        raise ValueError("dropout needs a Seed")
    if a_rowsum is not None:
        if a_rowsum.dtype != torch.float32 or a_rowsum.numel() != M or not a_rowsum.is_contiguous():
            raise ValueError("a_rowsum must be a contiguous fp32 vector of length M")
        _require_cuda(a_rowsum)
    probe = _PROBE
    rec = probe is not None and M >= 16 and N >= 16 and K >= 16 and not torch.cuda.is_current_stream_capturing()
    if rec:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    _ops().gemm(A, B, bool(trans_a), bool(trans_b), out, float(alpha), float(beta), bias, residual,
                bool(residual_first), int(act), aux, float(dropout_p), seed.t if seed is not None else None,
                _salt(salt), int(splits), a_rowsum, float(a_rowsum_beta), a_planes, b_planes, out_planes,
                bool(write_out), bool(getattr(A, "_mmfd_planes_only", False)),
                bool(getattr(B, "_mmfd_planes_only", False)))
    if not write_out:  # the fp32 output stays unwritten: only its planes may be read (checked in mmfd_gemm)
        out._mmfd_planes_only = True
    if rec:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        probe.records.append((_probe_name(A, B, out, trans_a, trans_b, residual, act, beta, splits, alpha=alpha,
                                          residual_first=residual_first, dropout_p=dropout_p, a_rowsum=a_rowsum,
                                          aux=aux, bias=bias), 2 * M * N * K, e0, e1))
    return out


def _probe_name(A, B, out, trans_a, trans_b, residual, act, beta, splits, alpha=1.0, residual_first=False,
                dropout_p=0.0, a_rowsum=None, aux=None, bias=None):
    """the kernel instantiation mmfd_gemm ran for these arguments, read from its launch plan with the
    workspace the library asks for (GemmProbe bookkeeping only)"""
    a = GemmArgs()
    a.dtype, a.c_dtype = dtype_code(A.dtype), dtype_code(out.dtype)
    a.trans_a, a.trans_b = int(bool(trans_a)), int(bool(trans_b))
    a.M, a.K = (A.shape[1], A.shape[0]) if trans_a else A.shape
    a.N = B.shape[1] if trans_b else B.shape[0]
    a.A, a.lda, a.B, a.ldb = A.data_ptr(), _ld(A), B.data_ptr(), _ld(B)
    a.C, a.ldc = out.data_ptr(), _ld(out)
    a.alpha, a.beta, a.splits = float(alpha), float(beta), int(splits)
    a.ep.act, a.ep.residual_first = int(act), int(bool(residual_first))
    if residual is not None:
        a.ep.residual, a.ep.ldr = residual.data_ptr(), _ld(residual)
    if aux is not None:
        a.ep.aux, a.ep.ldaux = aux.data_ptr(), _ld(aux)
    if bias is not None:
        a.ep.bias = bias.data_ptr()
    if dropout_p > 0:
        a.ep.dropout_p, a.ep.seed = float(dropout_p), _PLACEHOLDER
    if a_rowsum is not None:
        a.a_rowsum = a_rowsum.data_ptr()
    return _gemm_plan(a, whole_workspace=True)[1]


def split3(x, out=None):
    """fp32 [rows, cols] (row-major view, cols % 8 == 0) -> bf16 planes [3, rows, cols]: hi = bf16(x),
    mid = bf16(x - hi), lo = bf16(x - hi - mid) — the operand form of the split-operand fp32 GEMM"""
    _require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError("split3 takes a 2-D fp32 tensor")
    if out is None:
        out = torch.empty((3, x.shape[0], x.shape[1]), device=x.device, dtype=torch.bfloat16)
    _ops().split3(x, out)
    return out


def x6_ok(M, N, K, trans_a=False, trans_b=False):
    """whether mmfd_gemm runs this fp32 product (contiguous operands) on split operands — asked of
    the library itself (mmfd_gemm_runs_split: x6_plan + use_g8 + mfma_ok, every env switch
    included), so a producer never skips an fp32 output that a consumer would then read"""
    if fp32_gemm_mode() != 1 or min(M, N, K) < 1:
        return False
    a = GemmArgs()
    a.dtype = a.c_dtype = F32
    a.trans_a, a.trans_b = int(bool(trans_a)), int(bool(trans_b))
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.A = a.B = a.C = 1 << 20  # placeholder 16-B aligned pointers: only the shapes are inspected
    a.lda = M if trans_a else K
    a.ldb = N if trans_b else K
    a.ldc = N
    return lib().mmfd_gemm_runs_split(ctypes.byref(a)) != 0


def gemm_path(dtype, M, N, K, *, trans_a=False, trans_b=False, lda=None, ldb=None, ldc=None, out_dtype=None,
              bias=False, a_rowsum=False):
    """(path, kernel) of mmfd_gemm's launch plan for a product of these shapes and leading dimensions (default:
    contiguous operands) on 16-B aligned operands, with the workspace the library asks for — host arithmetic
    only, as x6_ok; path "simple" is the one-output-per-thread FMA kernel"""
    a = GemmArgs()
    a.dtype, a.c_dtype = dtype_code(dtype), dtype_code(out_dtype or dtype)
    a.trans_a, a.trans_b = int(bool(trans_a)), int(bool(trans_b))
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.A = a.B = a.C = _PLACEHOLDER
    a.lda = int(lda or (M if trans_a else K))
    a.ldb = int(ldb or (N if trans_b else K))
    a.ldc, a.alpha = int(ldc or N), 1.0
    if bias:
        a.ep.bias = _PLACEHOLDER
    if a_rowsum:
        a.a_rowsum = _PLACEHOLDER
    return _gemm_plan(a, whole_workspace=True)


def split_eligible(x):
    """whether GEMMs on fp32 operand `x` run on split planes (mode split, 16-B plane rows)"""
    return (x is not None and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] % 8 == 0
            and x.stride(1) == 1 and fp32_gemm_mode() == 1 and 6 * x.numel() < (1 << 31) - 4096)


def colsum(X, out=None, beta=0.0):
    _require_cuda(X)
    M, N = X.shape
    if out is None:
        out = torch.empty(N, device=X.device, dtype=torch.float32)
    nparts = max(1, min(256, M // 64))
    ws = torch.empty(nparts * N, device=X.device, dtype=torch.float32)
    _check(lib().mmfd_colsum(dtype_code(X.dtype), M, N, _ptr(X), _ld(X), _ptr(out), float(beta), _ptr(ws),
                             ws.numel() * 4, _stream()), "mmfd_colsum")
    return out


def linear(x, w, b=None, **kw):
    """y = x @ w^T + b over the last dim (x: [..., K], w: [N, K])."""
    shp = x.shape
    y = gemm(x.reshape(-1, shp[-1]), w, bias=b, **kw)
    return y.reshape(*shp[:-1], w.shape[0])


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _head_view(t, H, D):
    """t: [B, L, >= H*D] view with unit stride on the last dim -> (ptr, s_b, s_t)."""
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError("attention operands must be [B, L, H*D] views with a contiguous last dim")
    return t.data_ptr(), t.stride(0), t.stride(1)


def drop_mask_buffer(B, H, Lq, Lk, device):
    """the dropout keep-bitmask of one attention call (include/mmfd.h mmfd_attn_args.drop_mask): int32
    words [B*H*Lq*ceil(Lk/32)], written by attn_fwd and read by attn_bwd instead of re-hashing"""
    return torch.empty(B * H * Lq * ((Lk + 31) // 32), device=device, dtype=torch.int32)


def attn_fwd(q, k, v, H, *, out=None, scale=None, key_bias=None, rel_bias=None, dropout_p=0.0, seed=None, salt=0,
             cos_logit_scale=None, cos_max_log=0.0, o_planes=None, drop_mask=None):
    """q: [B, Lq, H*D], k/v: [B, Lk, H*D] (views into fused QKV buffers are fine).
    cos_logit_scale (fp32 [H], bf16 only): Swinv2 cosine attention, q/k normalised in the kernel.
    drop_mask (drop_mask_buffer, with dropout_p > 0): receives the keep-bitmask for attn_bwd.
    Returns (o [B, Lq, H*D], lse [B, H, Lq] fp32)."""
    _require_cuda(q, k, v)
    B, Lq, HD = q.shape
    Lk = k.shape[1]
    D = HD // H
    if out is None:
        out = torch.empty((B, Lq, H * D), device=q.device, dtype=q.dtype)
    lse = torch.empty((B, H, Lq), device=q.device, dtype=torch.float32)
    _head_view(q, H, D), _head_view(k, H, D), _head_view(v, H, D), _head_view(out, H, D)
    rb, rb_sb, rb_mod = _rel_bias_args(rel_bias, B, H, Lq, Lk)
    if cos_logit_scale is not None and (cos_logit_scale.dtype != torch.float32 or not cos_logit_scale.is_contiguous()):
        raise ValueError("cos_logit_scale must be a contiguous fp32 tensor of H values")
    _ops().attn_fwd(q, k, v, out, lse, int(H), float(scale if scale is not None else D ** -0.5), key_bias,
                    rel_bias if rb is not None else None, int(rb_sb), int(rb_mod), float(dropout_p),
                    seed.t if seed is not None else None, _salt(salt), cos_logit_scale, float(cos_max_log), o_planes,
                    drop_mask if dropout_p > 0 else None)
    return out, lse


def _rel_bias_args(rel_bias, B, H, Lq, Lk):
    """(pointer, batch stride, batch modulus) for an additive fp32 bias shared by the batch
    ([H, Lq, Lk], MPNet), per batch row ([B, H, Lq, Lk], DeBERTa) or repeating every M batch rows
    ([M, H, Lq, Lk] with B % M == 0: Swinv2 shifted-window masks, batch = images x M windows)"""
    if rel_bias is None:
        return None, 0, 0
    if rel_bias.dtype != torch.float32 or not rel_bias.is_contiguous():
        raise ValueError("rel_bias must be a contiguous fp32 tensor")
    if tuple(rel_bias.shape) == (H, Lq, Lk):
        return rel_bias.data_ptr(), 0, 0
    if tuple(rel_bias.shape) == (B, H, Lq, Lk):
        return rel_bias.data_ptr(), H * Lq * Lk, 0
    if rel_bias.dim() == 4 and tuple(rel_bias.shape[1:]) == (H, Lq, Lk) and B % rel_bias.shape[0] == 0:
        return rel_bias.data_ptr(), H * Lq * Lk, rel_bias.shape[0]
    raise ValueError(f"rel_bias shape {tuple(rel_bias.shape)} is neither [H,Lq,Lk] nor [M,H,Lq,Lk] with B % M == 0")


def deberta_rel_bias(c2p, p2c, c2p_idx, p2c_idx, B, L, inv_scale, out=None):
    """DeBERTa c2p + p2c bias [B, H, L, L] fp32 from the per-head position scores c2p / p2c
    ([H, B*L, ld]) and the clamped log-bucket indices (int32 [L, L])."""
    _require_cuda(c2p, p2c, c2p_idx, p2c_idx)
    H, _, ld = c2p.shape
    out = out if out is not None else torch.empty((B, H, L, L), device=c2p.device, dtype=torch.float32)
    _check(lib().mmfd_deberta_rel_bias(dtype_code(c2p.dtype), B, H, L, _ptr(c2p), _ptr(p2c), ld, _ptr(c2p_idx),
                                       _ptr(p2c_idx), float(inv_scale), _ptr(out), _stream()), "mmfd_deberta_rel_bias")
    return out


_MONO = {}


def check_rel_index_runs(c2p_idx, p2c_idx):
    """host check behind deberta_rel_bias_bwd: along its second index every row of c2p_idx is
    non-increasing and every row of p2c_idx non-decreasing, so all positions that map to one column
    form ONE contiguous run (the kernel's single-writer sums depend on it). Raises ValueError."""
    c = c2p_idx.detach().cpu().numpy() if isinstance(c2p_idx, torch.Tensor) else c2p_idx
    p = p2c_idx.detach().cpu().numpy() if isinstance(p2c_idx, torch.Tensor) else p2c_idx
    if c.ndim != 2 or p.ndim != 2 or c.shape != p.shape or c.shape[0] != c.shape[1]:
        raise ValueError("deberta_rel_bias_bwd: c2p_idx / p2c_idx must be [L, L]")
    if c.shape[1] > 1 and ((c[:, 1:] > c[:, :-1]).any() or (p[:, 1:] < p[:, :-1]).any()):
        raise ValueError("deberta_rel_bias_bwd: the relative-position indices are not monotone along a row "
                         "(c2p_idx non-increasing, p2c_idx non-decreasing): the run-sum kernel does not apply")
    return int(max(c.max(), p.max())) if c.size else -1, int(min(c.min(), p.min())) if c.size else 0


def verify_rel_indices(c2p_idx, p2c_idx, host=None):
    """(max, min) index of a device index pair after check_rel_index_runs, once per pair (cached by
    tensor identity and version). `host`: the pair's host copies (numpy), for a caller that built the
    device tensors from them — no device read then, so the model registers its cached pair when it
    creates it and a later graph capture finds it verified."""
    key = (c2p_idx.data_ptr(), p2c_idx.data_ptr(), tuple(c2p_idx.shape), c2p_idx._version, p2c_idx._version)
    ent = _MONO.get(key)
    # (an entry counts only for the very tensors it was made for: a freed pair's addresses get reused)
    if ent is not None and ent[1]() is c2p_idx and ent[2]() is p2c_idx:
        return ent[0]
    if host is None and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("deberta_rel_bias_bwd: the index pair must be verified before a graph capture "
                           "(verify_rel_indices outside the capture)")
    rng = check_rel_index_runs(*host) if host is not None else check_rel_index_runs(c2p_idx, p2c_idx)
    if len(_MONO) > 64:
        _MONO.clear()
    _MONO[key] = (rng, weakref.ref(c2p_idx), weakref.ref(p2c_idx))
    return rng


def deberta_rel_bias_bwd(ds, c2p_idx, p2c_idx, B, L, inv_scale, ld, dtype, dc2p=None, dp2c=None):
    """adjoint of deberta_rel_bias: ds fp32 [B, H, L, L] -> (dc2p, dp2c) [H, B*L, ld] in `dtype`.
    The index pair is verified on the host once (cached by tensor identity: the model caches one
    pair per (L, S)): monotone rows (check_rel_index_runs) and values in [0, ld)."""
    _require_cuda(ds, c2p_idx, p2c_idx)
    if ds.dtype != torch.float32 or not ds.is_contiguous() or ds.dim() != 4 or ds.shape[0] != B or ds.shape[2:] != (L, L):
        raise ValueError("deberta_rel_bias_bwd: ds must be a contiguous fp32 [B, H, L, L] tensor")
    for t in (c2p_idx, p2c_idx):
        if t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != (L, L):
            raise ValueError("deberta_rel_bias_bwd: indices must be contiguous int32 [L, L]")
    rng = verify_rel_indices(c2p_idx, p2c_idx)
    if rng[0] >= ld or rng[1] < 0:
        raise ValueError(f"deberta_rel_bias_bwd: indices span [{rng[1]}, {rng[0]}], outside [0, {ld})")
    H = ds.shape[1]
    dc2p = dc2p if dc2p is not None else torch.empty((H, B * L, ld), device=ds.device, dtype=dtype)
    dp2c = dp2c if dp2c is not None else torch.empty((H, B * L, ld), device=ds.device, dtype=dtype)
    for t in (dc2p, dp2c):
        if t.dtype != dtype or tuple(t.shape) != (H, B * L, ld) or not t.is_contiguous():
            raise ValueError("deberta_rel_bias_bwd: dc2p / dp2c must be contiguous [H, B*L, ld] of `dtype`")
    _check(lib().mmfd_deberta_rel_bias_bwd(dtype_code(dtype), B, H, L, _ptr(ds), _ptr(c2p_idx), _ptr(p2c_idx),
                                           float(inv_scale), _ptr(dc2p), _ptr(dp2c), ld, _stream()),
           "mmfd_deberta_rel_bias_bwd")
    return dc2p, dp2c


def attn_fill_masked_rows_bwd(dout, H, mask, dv=None, gsum=None):
    """adjoint of attn_fill_masked_rows in two calls around attn_bwd. Without `dv` (phase 0): returns
    gsum [B, H*Dh] fp32 = (1/L) * the sum of dout over the padded query rows (mask[b, i] == 0), and
    zeroes those rows of dout in place. With `dv` and that `gsum` (phase 1): dv[b, j] += gsum[b] for
    every key j, in place; returns dv."""
    _require_cuda(dout, mask, dv, gsum)
    B, L, HD = dout.shape
    Dh = HD // H
    dop, dosb, dost = _head_view(dout, H, Dh)
    if dv is None:
        m = mask.to(torch.int64).contiguous()
        gsum = torch.empty((B, HD), device=dout.device, dtype=torch.float32)
        _check(lib().mmfd_attn_fill_masked_rows_bwd(dtype_code(dout.dtype), 0, B, H, L, Dh, dop, dosb, dost, None, 0, 0,
                                                    _ptr(m), _ptr(gsum), _stream()), "mmfd_attn_fill_masked_rows_bwd")
        return gsum
    if gsum is None or gsum.dtype != torch.float32 or tuple(gsum.shape) != (B, HD) or not gsum.is_contiguous():
        raise ValueError("attn_fill_masked_rows_bwd: phase 1 needs the gsum [B, H*Dh] of phase 0")
    if dv.dtype != dout.dtype or tuple(dv.shape) != (B, L, HD):
        raise ValueError("attn_fill_masked_rows_bwd: dv must match dout in shape and dtype")
    dvp, dvsb, dvst = _head_view(dv, H, Dh)
    _check(lib().mmfd_attn_fill_masked_rows_bwd(dtype_code(dv.dtype), 1, B, H, L, Dh, None, 0, 0, dvp, dvsb, dvst, None,
                                                _ptr(gsum), _stream()), "mmfd_attn_fill_masked_rows_bwd")
    return dv


def mask_rows(x2d, mask):
    """x[r, :] = 0 where mask[r] == 0 (in place)"""
    _require_cuda(x2d, mask)
    m = mask.reshape(-1).to(torch.int64).contiguous()
    _check(lib().mmfd_mask_rows(dtype_code(x2d.dtype), x2d.shape[0], x2d.shape[1], _ptr(x2d), _ld(x2d), _ptr(m),
                                _stream()), "mmfd_mask_rows")
    return x2d


def attn_fill_masked_rows(v, o, H, mask):
    """o rows of fully masked queries (mask[b, i] == 0) = mean of v over all keys (in place)"""
    _require_cuda(v, o, mask)
    B, L, HD = v.shape
    Dh = HD // H
    m = mask.to(torch.int64).contiguous()
    vp, vsb, vst = _head_view(v, H, Dh)
    op, osb, ost = _head_view(o, H, Dh)
    _check(lib().mmfd_attn_fill_masked_rows(dtype_code(v.dtype), B, H, L, Dh, vp, vsb, vst, op, osb, ost, _ptr(m),
                                            _stream()), "mmfd_attn_fill_masked_rows")
    return o


def attn_bwd(q, k, v, o, lse, dout, H, *, dq=None, dk=None, dv=None, scale=None, key_bias=None, rel_bias=None,
             dropout_p=0.0, seed=None, salt=0, accumulate_dq=False, accumulate_dkv=False, dqkv_planes=None,
             planes_only=False, drop_mask=None, d_rel_bias=None, delta=None):
    """dq, dk, dv (views of one packed [B, L, 3*H*D] buffer when `dqkv_planes` is given: bf16
    [3, B*L, 3*H*D] split planes of that buffer, written by the kernels; planes_only skips the
    fp32 stores — for a gradient read only by split-operand GEMMs, see x6_ok).
    `d_rel_bias` (contiguous fp32 [B, H, Lq, Lk]): receives the gradient with respect to a per-batch
    `rel_bias` [B, H, Lq, Lk] (no dropout; include/mmfd.h mmfd_attn_args.d_rel_bias).
    `delta` (contiguous fp32 [B, H, Lq]): the call's delta workspace, kept by the caller — it holds
    rowsum(dO * O) afterwards, which attn_bwd_bias_sum reads."""
    _require_cuda(q, k, v, o, lse, dout)
    B, Lq, HD = q.shape
    Lk = k.shape[1]
    D = HD // H
    dq = dq if dq is not None else torch.empty_like(q, memory_format=torch.contiguous_format)
    dk = dk if dk is not None else torch.empty((B, Lk, HD), device=q.device, dtype=q.dtype)
    dv = dv if dv is not None else torch.empty((B, Lk, HD), device=q.device, dtype=q.dtype)
    for t in (q, k, v, o, dout, dq, dk, dv):
        _head_view(t, H, D)
    rb, rb_sb, rb_mod = _rel_bias_args(rel_bias, B, H, Lq, Lk)
    _ops().attn_bwd(q, k, v, o, lse, dout, dq, dk, dv, int(H), float(scale if scale is not None else D ** -0.5),
                    key_bias, rel_bias if rb is not None else None, int(rb_sb), int(rb_mod), float(dropout_p),
                    seed.t if seed is not None else None, _salt(salt), bool(accumulate_dq), bool(accumulate_dkv),
                    dqkv_planes, bool(planes_only), drop_mask if dropout_p > 0 else None, d_rel_bias, delta)
    return dq, dk, dv


def attn_bwd_ds(q, k, v, lse, dout, H, delta, *, rel_bias, key_bias=None, scale=None, dropout_p=0.0, seed=None, salt=0,
                drop_mask=None, out=None):
    """The gradient of a per-batch `rel_bias` [B, H, Lq, Lk] with or without attention dropout: fp32
    [B, H, Lq, Lk] = P (M (dO V^T) / (1 - p) - delta) with the forward's keep mask M (include/mmfd.h
    mmfd_attn_bwd_ds). The arguments are those of the preceding attn_bwd call — made without d_rel_bias,
    which refuses dropout — and `delta` the tensor that call was given. Nothing but `out` is written.
    `drop_mask` (the forward's keep-bitmask) is accepted and not read: the kernel re-hashes the same bits.
    With dropout_p = 0 the result is bit for bit attn_bwd's d_rel_bias."""
    _require_cuda(q, k, v, lse, dout, delta, rel_bias, key_bias, out)
    B, Lq, HD = q.shape
    Lk = k.shape[1]
    D = HD // H
    rb, rb_sb, rb_mod = _rel_bias_args(rel_bias, B, H, Lq, Lk)  # (a shared or modulo bias: the library refuses it)
    if rb is None:
        raise ValueError("attn_bwd_ds: no rel_bias")
    if delta.dtype != torch.float32 or not delta.is_contiguous() or delta.numel() != B * H * Lq:
        raise ValueError("attn_bwd_ds: delta must be the contiguous fp32 [B, H, Lq] tensor attn_bwd filled")
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != B * H * Lq:
        raise ValueError("attn_bwd_ds: lse must be contiguous fp32 [B, H, Lq]")
    if key_bias is not None and (key_bias.dtype != torch.float32 or not key_bias.is_contiguous()
                                 or key_bias.numel() != B * Lk):
        raise ValueError("attn_bwd_ds: key_bias must be contiguous fp32 [B, Lk]")
    if tuple(k.shape) != (B, Lk, HD) or tuple(v.shape) != (B, Lk, HD) or tuple(dout.shape) != (B, Lq, HD):
        raise ValueError("attn_bwd_ds: k, v must be [B, Lk, H*D] and dout [B, Lq, H*D]")
    for t in (k, v, dout):
        if t.dtype != q.dtype:
            raise TypeError("attn_bwd_ds: q, k, v, dout must share a dtype")
    if drop_mask is not None and (drop_mask.dtype != torch.int32 or not drop_mask.is_contiguous()
                                  or drop_mask.numel() != B * H * Lq * ((Lk + 31) // 32)):
        raise ValueError("attn_bwd_ds: drop_mask must be the drop_mask_buffer of the forward call")
    if out is None:
        out = torch.empty((B, H, Lq, Lk), device=q.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, H, Lq, Lk):
        raise ValueError(f"attn_bwd_ds: out must be contiguous fp32 {(B, H, Lq, Lk)}")
    a = AttnArgs()
    a.dtype = dtype_code(q.dtype)
    a.B, a.H, a.Lq, a.Lk, a.D = B, H, Lq, Lk, D
    a.scale = float(scale if scale is not None else D ** -0.5)
    a.q, a.q_sb, a.q_st = _head_view(q, H, D)
    a.k, a.k_sb, a.k_st = _head_view(k, H, D)
    a.v, a.v_sb, a.v_st = _head_view(v, H, D)
    a.dout, a.do_sb, a.do_st = _head_view(dout, H, D)
    a.lse, a.delta = lse.data_ptr(), delta.data_ptr()
    a.key_bias = key_bias.data_ptr() if key_bias is not None else None
    a.rel_bias, a.rel_bias_sb, a.rel_bias_mod = rb, rb_sb, rb_mod
    a.dropout_p = float(dropout_p)
    a.seed = seed.t.data_ptr() if seed is not None else None
    a.salt = int(salt) & 0xFFFFFFFFFFFFFFFF
    a.drop_mask = drop_mask.data_ptr() if drop_mask is not None and dropout_p > 0 else None
    _check(lib().mmfd_attn_bwd_ds(ctypes.byref(a), _ptr(out), _stream()), "mmfd_attn_bwd_ds")
    return out


def attn_bwd_bias_sum(q, k, v, o, lse, dout, H, delta, *, rel_bias, rel_bias_mod=None, scale=None, key_bias=None,
                      dropout_p=0.0, cos_logit_scale=None, out=None):
    """The gradient of a `rel_bias` shared by the batch ([H, Lq, Lk]) or read with a batch modulus
    ([M, H, Lq, Lk], B % M == 0): fp32 [M, H, Lq, Lk] (M = 1 for the shared form) = the sum over the batch
    rows b = m (mod M) of P (dP - delta). The arguments are those of the preceding attn_bwd call, `delta`
    the tensor that call was given (include/mmfd.h mmfd_attn_bwd_bias_sum; Lq, Lk <= 256; a per-batch
    bias, dropout and cosine attention are refused). A [B, H, Lq, Lk] bias reads as per-batch, as in
    attn_fwd / attn_bwd (the same numbers either way there); a caller whose modulo bias can have M == B
    (Swinv2 with one image: the batch is its nW windows) says so with `rel_bias_mod` = M, and gets the
    M-row sum of one term each."""
    _require_cuda(q, k, v, o, lse, dout, delta, rel_bias, key_bias)
    B, Lq, HD = q.shape
    Lk = k.shape[1]
    D = HD // H
    rb, rb_sb, rb_mod = _rel_bias_args(rel_bias, B, H, Lq, Lk)
    if rb is None:
        raise ValueError("attn_bwd_bias_sum: no rel_bias")
    if rel_bias_mod is not None:
        if tuple(rel_bias.shape) != (rel_bias_mod, H, Lq, Lk) or B % rel_bias_mod:
            raise ValueError(f"attn_bwd_bias_sum: rel_bias_mod = {rel_bias_mod} needs a [{rel_bias_mod}, H, Lq, Lk] "
                             f"bias and B % {rel_bias_mod} == 0, got {tuple(rel_bias.shape)} with B = {B}")
        rb_sb, rb_mod = H * Lq * Lk, int(rel_bias_mod)
    if delta.dtype != torch.float32 or not delta.is_contiguous() or delta.numel() != B * H * Lq:
        raise ValueError("attn_bwd_bias_sum: delta must be the contiguous fp32 [B, H, Lq] tensor attn_bwd filled")
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != B * H * Lq:
        raise ValueError("attn_bwd_bias_sum: lse must be contiguous fp32 [B, H, Lq]")
    if key_bias is not None and (key_bias.dtype != torch.float32 or not key_bias.is_contiguous()
                                 or key_bias.numel() != B * Lk):
        raise ValueError("attn_bwd_bias_sum: key_bias must be contiguous fp32 [B, Lk]")
    for t in (k, v, o, dout):
        if t.dtype != q.dtype:
            raise TypeError("attn_bwd_bias_sum: q, k, v, o, dout must share a dtype")
    M = rb_mod if rb_mod else (B if rb_sb else 1)  # (a per-batch bias: the library refuses it)
    if out is None:
        out = torch.empty((M, H, Lq, Lk), device=q.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (M, H, Lq, Lk):
        raise ValueError(f"attn_bwd_bias_sum: out must be contiguous fp32 {(M, H, Lq, Lk)}")
    a = AttnArgs()
    a.dtype = dtype_code(q.dtype)
    a.B, a.H, a.Lq, a.Lk, a.D = B, H, Lq, Lk, D
    a.scale = float(scale if scale is not None else D ** -0.5)
    a.q, a.q_sb, a.q_st = _head_view(q, H, D)
    a.k, a.k_sb, a.k_st = _head_view(k, H, D)
    a.v, a.v_sb, a.v_st = _head_view(v, H, D)
    a.o, a.o_sb, a.o_st = _head_view(o, H, D)
    a.dout, a.do_sb, a.do_st = _head_view(dout, H, D)
    a.lse, a.delta = lse.data_ptr(), delta.data_ptr()
    a.key_bias = key_bias.data_ptr() if key_bias is not None else None
    a.rel_bias, a.rel_bias_sb, a.rel_bias_mod = rb, rb_sb, rb_mod
    a.dropout_p = float(dropout_p)
    a.cos_logit_scale = cos_logit_scale.data_ptr() if cos_logit_scale is not None else None
    _check(lib().mmfd_attn_bwd_bias_sum(ctypes.byref(a), _ptr(out), _stream()), "mmfd_attn_bwd_bias_sum")
    return out


# ------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------
def layernorm_fwd(x2d, gamma, beta, eps, out=None, planes=None):
    """y = LayerNorm(x); `planes` (bf16 [3, R, W], fp32 x only): the output's split3 planes, written
    in the same pass"""
    _require_cuda(x2d, gamma, beta)
    R, W = x2d.shape
    y = out if out is not None else torch.empty((R, W), device=x2d.device, dtype=x2d.dtype)
    mean = torch.empty(R, device=x2d.device, dtype=torch.float32)
    rstd = torch.empty(R, device=x2d.device, dtype=torch.float32)
    _ops().layernorm_fwd(x2d, gamma, beta, float(eps), y, mean, rstd, planes)
    return y, mean, rstd


def layernorm_fwd_res(x2d, gamma, beta, eps, res, out=None, stats=False):
    """y = res + LN(x) (Swinv2 res-post-norm); returns y (and mean, rstd when stats=True)"""
    _require_cuda(x2d, gamma, beta, res)
    R, W = x2d.shape
    if tuple(res.shape) != (R, W) or res.dtype != x2d.dtype:
        raise ValueError("layernorm_fwd_res: residual must match x in shape and dtype")
    y = out if out is not None else torch.empty((R, W), device=x2d.device, dtype=x2d.dtype)
    mean = torch.empty(R, device=x2d.device, dtype=torch.float32) if stats else None
    rstd = torch.empty(R, device=x2d.device, dtype=torch.float32) if stats else None
    _check(lib().mmfd_layernorm_fwd_res(dtype_code(x2d.dtype), R, W, _ptr(x2d), _ld(x2d), _ptr(gamma), _ptr(beta),
                                        float(eps), _ptr(res), _ld(res), _ptr(y), _ld(y),
                                        _ptr(mean) if stats else None, _ptr(rstd) if stats else None, _stream()),
           "mmfd_layernorm_fwd_res")
    return (y, mean, rstd) if stats else y


def layernorm_bwd(dy, x, gamma, mean, rstd, *, dx=None, dx_add=None, dgamma=None, dbeta=None, beta_acc=0.0,
                  dx_drop=None, dropout_p=0.0, seed=None, salt=0, planes=None):
    """`planes` (bf16 [3, R, W], fp32 only): split planes of the gradient the next GEMMs read —
    dx_drop when given, else dx — written by the same kernel"""
    _require_cuda(dy, x, gamma, mean, rstd)
    R, W = dy.shape
    dx = dx if dx is not None else torch.empty((R, W), device=dy.device, dtype=dy.dtype)
    _ops().layernorm_bwd(dy, x, gamma, mean, rstd, dx, dx_add, dgamma, dbeta, float(beta_acc), dx_drop,
                         float(dropout_p), seed.t if seed is not None else None, _salt(salt), planes)
    return dx


# ------------------------------------------------------------------------------------------------
# misc
# ------------------------------------------------------------------------------------------------
def seq_mean_fwd(x, out=None):
    B, L, D = x.shape
    out = out if out is not None else torch.empty((B, D), device=x.device, dtype=x.dtype)
    _ops().seq_mean_fwd(x if x.is_contiguous() else x.contiguous(), out)
    return out


def seq_mean_bwd(dout, L, dx=None):
    B, D = dout.shape
    dx = dx if dx is not None else torch.empty((B, L, D), device=dout.device, dtype=dout.dtype)
    _ops().seq_mean_bwd(dout, dx)
    return dx


def xent_fwd_bwd(logits, labels, want_grad=True, dloss_scale=None, cols=None, n_slots=None):
    """logits: list of [B, C] fp32 tensors (present paths), labels: int64 [B, n_cols] (or [B]);
    cols: label column of each path (the reference's path index, train.py:165; default 0..n-1).
    Returns (loss [n_slots] fp32 device tensor: total, then one slot per label column (0 for
    columns without a present path), list of dlogits or None)."""
    n = len(logits)
    B, C = logits[0].shape
    dev = logits[0].device
    cols = list(range(n)) if cols is None else [int(c) for c in cols]
    if len(cols) != n:
        raise ValueError("xent: one label column per path")
    n_slots = n_slots or 1 + max(cols) + 1
    logits = [l.contiguous().float() for l in logits]
    labels = labels.contiguous()
    ld = labels.stride(0) if labels.dim() > 1 else 1
    if max(cols) >= (labels.shape[1] if labels.dim() > 1 else 1):
        raise ValueError(f"xent: label column {max(cols)} outside labels {tuple(labels.shape)}")
    del ld
    loss = torch.empty(n_slots, device=dev, dtype=torch.float32)
    dl = [torch.empty_like(l) for l in logits] if want_grad else None
    _ops().xent(logits, cols, labels, loss, dl if want_grad else [], dloss_scale)
    return loss, dl


def cast(x, dtype, out=None):
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    elif out.dtype != dtype or out.numel() != x.numel() or not out.is_contiguous():
        raise ValueError("cast: out must be a contiguous tensor of the target dtype and size")
    if x.numel():
        _ops().cast(x if x.is_contiguous() else x.contiguous(), out)
    return out


def transpose(x, out=None):
    """out = x^T as a contiguous [cols, rows] tensor (fp32 / bf16, mmfd_transpose)"""
    _require_cuda(x)
    if x.dim() != 2:
        raise ValueError("transpose takes a 2-D tensor")
    rows, cols = x.shape
    if out is None:
        out = torch.empty((cols, rows), device=x.device, dtype=x.dtype)
    if out.dtype != x.dtype or tuple(out.shape) != (cols, rows):
        raise ValueError("transpose: out must be [cols, rows] of the input dtype")
    _check(lib().mmfd_transpose(dtype_code(x.dtype), rows, cols, _ptr(x), _ld(x), _ptr(out), _ld(out), _stream()),
           "mmfd_transpose")
    return out


def zero_(t):
    """t[...] = 0 in place (a contiguous tensor) with mmfd_zero (a zero-fill kernel on the current stream)"""
    if not t.is_contiguous():
        raise ValueError("zero_: contiguous tensors only")
    if t.numel():
        _check(lib().mmfd_zero(_ptr(t), t.numel() * t.element_size(), _stream()), "mmfd_zero")
    return t


def zeros(shape, dtype=torch.float32, device="cuda"):
    """torch.empty + mmfd_zero"""
    return zero_(torch.empty(shape, dtype=dtype, device=device))


def axpby(a, x, b=0.0, y=None, out=None):
    out = out if out is not None else torch.empty_like(x)
    _check(lib().mmfd_axpby(dtype_code(x.dtype), x.numel(), float(a), _ptr(x), float(b), _ptr(y), _ptr(out),
                            _stream()), "mmfd_axpby")
    return out


def dropout(x, p, seed, salt, out=None):
    out = out if out is not None else torch.empty_like(x)
    _check(lib().mmfd_dropout(dtype_code(x.dtype), x.numel(), _ptr(x), _ptr(out), float(p),
                              seed.ptr() if seed is not None else None, int(salt) & 0xFFFFFFFFFFFFFFFF, _stream()),
           "mmfd_dropout")
    return out


def act_bwd(dy, aux, act, dropout_p=0.0, seed=None, salt=0, out=None):
    out = out if out is not None else torch.empty_like(dy)
    _check(lib().mmfd_act_bwd(dtype_code(dy.dtype), dy.numel(), _ptr(dy), _ptr(aux), int(act), float(dropout_p),
                              seed.ptr() if seed is not None else None, int(salt) & 0xFFFFFFFFFFFFFFFF, _ptr(out),
                              _stream()), "mmfd_act_bwd")
    return out


def mask_to_bias(mask, neg=None):
    neg = torch.finfo(torch.float32).min if neg is None else neg
    m = mask.to(torch.int64).contiguous()
    out = torch.empty(m.shape, device=m.device, dtype=torch.float32)
    _check(lib().mmfd_mask_to_bias(m.numel(), _ptr(m), _ptr(out), float(neg), _stream()), "mmfd_mask_to_bias")
    return out


def embed_ln_fwd(ids, tts, word, pos, typ, gamma, beta, eps, dtype, dropout_p=0.0, seed=None, salt=0):
    B, L = ids.shape
    D = word.shape[1]
    dev = ids.device
    s = torch.empty((B * L, D), device=dev, dtype=dtype)
    y = torch.empty((B * L, D), device=dev, dtype=dtype)
    mean = torch.empty(B * L, device=dev, dtype=torch.float32)
    rstd = torch.empty(B * L, device=dev, dtype=torch.float32)
    _check(lib().mmfd_embed_ln_fwd(dtype_code(dtype), B, L, D, _ptr(ids.contiguous()),
                                   _ptr(tts.contiguous()) if tts is not None else None, _ptr(word), _ptr(pos),
                                   _ptr(typ), _ptr(gamma), _ptr(beta), float(eps), _ptr(s), _ptr(y), _ptr(mean),
                                   _ptr(rstd), float(dropout_p), seed.ptr() if seed is not None else None,
                                   int(salt) & 0xFFFFFFFFFFFFFFFF, _stream()), "mmfd_embed_ln_fwd")
    return s, y, mean, rstd


def embed_ln_infer(ids, pos_ids, word, pos, gamma, beta, eps, dtype, tts=None, typ=None):
    """inference embeddings: y = LN(word[id] + pos[pos_id] (+ type[tt])), nothing saved"""
    B, L = ids.shape
    D = word.shape[1]
    y = torch.empty((B * L, D), device=ids.device, dtype=dtype)
    _check(lib().mmfd_embed_ln_fwd_ex(dtype_code(dtype), B, L, D, _ptr(ids.contiguous()),
                                      _ptr(pos_ids.contiguous()) if pos_ids is not None else None,
                                      _ptr(tts.contiguous()) if tts is not None else None, _ptr(word), _ptr(pos),
                                      _ptr(typ) if typ is not None else None, _ptr(gamma), _ptr(beta), float(eps),
                                      None, _ptr(y), None, None, 0.0, None, 0, _stream()), "mmfd_embed_ln_fwd_ex")
    return y


def embed_ln_train(ids, pos_ids, word, pos, gamma, beta, eps, dtype, dropout_p=0.0, seed=None, salt=0):
    """embed_ln_infer that keeps what the LayerNorm backward reads: (sum, y, mean, rstd) with
    sum = word[id] + pos[pos_id] before the LayerNorm (no type table); with dropout_p > 0
    y = dropout(LayerNorm(sum)), element index = the flat index of y (as embed_ln_fwd)"""
    B, L = ids.shape
    D = word.shape[1]
    dev = ids.device
    s = torch.empty((B * L, D), device=dev, dtype=dtype)
    y = torch.empty((B * L, D), device=dev, dtype=dtype)
    mean = torch.empty(B * L, device=dev, dtype=torch.float32)
    rstd = torch.empty(B * L, device=dev, dtype=torch.float32)
    _check(lib().mmfd_embed_ln_fwd_ex(dtype_code(dtype), B, L, D, _ptr(ids.contiguous()),
                                      _ptr(pos_ids.contiguous()) if pos_ids is not None else None, None, _ptr(word),
                                      _ptr(pos), None, _ptr(gamma), _ptr(beta), float(eps), _ptr(s), _ptr(y),
                                      _ptr(mean), _ptr(rstd), float(dropout_p), seed.ptr() if seed is not None else None,
                                      int(salt) & 0xFFFFFFFFFFFFFFFF, _stream()), "mmfd_embed_ln_fwd_ex")
    return s, y, mean, rstd


def position_ids(ids, padding_idx):
    ids = ids.contiguous()
    out = torch.empty_like(ids)
    _check(lib().mmfd_position_ids(ids.shape[0], ids.shape[1], _ptr(ids), int(padding_idx), _ptr(out), _stream()),
           "mmfd_position_ids")
    return out


def rel_bias(bucket, table):
    """bucket int32 [Lq, Lk] (device), table fp32 [nb, H] -> fp32 [H, Lq, Lk]"""
    Lq, Lk = bucket.shape
    H = table.shape[1]
    out = torch.empty((H, Lq, Lk), device=table.device, dtype=torch.float32)
    _check(lib().mmfd_rel_bias(H, Lq, Lk, _ptr(bucket.contiguous()), _ptr(table.contiguous()), _ptr(out), _stream()),
           "mmfd_rel_bias")
    return out


# ---- convolution support (ResNet50 extractor) ------------------------------------------------
def conv_weight_prep(w, dtype, Kpad=None, bn=None, eps=1e-5):
    """fp32 conv weight [Cout, Cin, KH, KW] (+ BatchNorm (gamma, beta, mean, var)) -> GEMM weight
    [Cout, Kpad] in dtype with (kh, kw, c) column order, and the folded fp32 bias [Cout]."""
    Cout, Cin, KH, KW = w.shape
    Kpad = Kpad or KH * KW * Cin
    ow = torch.empty((Cout, Kpad), device=w.device, dtype=dtype)
    ob = torch.empty(Cout, device=w.device, dtype=torch.float32)
    g, b, m, v = bn if bn is not None else (None, None, None, None)
    _check(lib().mmfd_conv_weight_prep(dtype_code(dtype), Cout, Cin, KH, KW, Kpad, _ptr(w.contiguous()),
                                       _ptr(g) if g is not None else None, _ptr(b) if b is not None else None,
                                       _ptr(m) if m is not None else None, _ptr(v) if v is not None else None,
                                       float(eps), _ptr(ow), _ptr(ob), _stream()), "mmfd_conv_weight_prep")
    return ow, ob


def im2col_nhwc(x, N, H, W, C, k, stride, pad, Kpad=None):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    Kpad = Kpad or k * k * C
    out = torch.empty((N * Ho * Wo, Kpad), device=x.device, dtype=x.dtype)
    _check(lib().mmfd_im2col_nhwc(dtype_code(x.dtype), N, H, W, C, k, k, stride, pad, Ho, Wo, Kpad, _ptr(x), _ptr(out),
                                  _stream()), "mmfd_im2col_nhwc")
    return out, Ho, Wo


def im2col_nchw(x, k, stride, pad, Kpad, dtype):
    N, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((N * Ho * Wo, Kpad), device=x.device, dtype=dtype)
    _check(lib().mmfd_im2col_nchw(dtype_code(dtype), N, C, H, W, k, k, stride, pad, Ho, Wo, Kpad,
                                  _ptr(x.contiguous()), _ptr(out), _stream()), "mmfd_im2col_nchw")
    return out, Ho, Wo


def conv_implicit_ok(dtype, C):
    """whether a convolution over C input channels can run as an implicit GEMM (conv2d_nhwc): a
    K-tile / split-operand K-step (64 bf16 / 32 fp32 channels) must not straddle two filter taps"""
    return C % (64 if dtype == torch.bfloat16 else 32) == 0


def conv2d_nhwc(x, N, H, W, C, w, k, stride, pad, bias=None, act=ACT_NONE, residual=None, residual_first=False,
                x_planes=None):
    """Implicit-GEMM convolution (mmfd_gemm_args.conv): x = the NHWC activation as rows [N*H*W, C],
    w = the folded GEMM weight [Cout, k*k*C] with (kh, kw, c) columns (conv_weight_prep), output
    rows [N*Ho*Wo, Cout] = epilogue(conv(x)) — the same products, in the same K order, as
    gemm(im2col_nhwc(x), w) without the im2col matrix (im2im_retrieval.py:14-17, 29-36).
    `x_planes`: split3(x), reused by the split-operand fp32 path when given. Returns (y, Ho, Wo)."""
    _require_cuda(x, w, bias, residual)
    if x.dtype != w.dtype:
        raise TypeError(f"conv operands must share a dtype ({x.dtype} vs {w.dtype})")
    if not conv_implicit_ok(x.dtype, C) or tuple(x.shape) != (N * H * W, C) or not x.is_contiguous():
        raise ValueError(f"conv2d_nhwc: x must be contiguous [N*H*W, C] with C % {64 if x.dtype == torch.bfloat16 else 32} == 0")
    Cout, Kw = w.shape
    if Kw != k * k * C or not w.is_contiguous():
        raise ValueError(f"conv2d_nhwc: w must be contiguous [Cout, {k * k * C}], got {tuple(w.shape)}")
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    M, K = N * Ho * Wo, k * k * C
    out = torch.empty((M, Cout), device=x.device, dtype=x.dtype)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != Cout or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous fp32 vector of length Cout")
    if residual is not None and (residual.dtype != out.dtype or tuple(residual.shape) != (M, Cout)):
        raise ValueError("residual must match the output shape and dtype")
    g = ConvGeomArgs(N=N, H=H, W=W, C=C, KH=k, KW=k, stride=stride, pad=pad, Ho=Ho, Wo=Wo)
    a = GemmArgs()
    a.dtype = a.c_dtype = dtype_code(x.dtype)
    a.M, a.N, a.K = M, Cout, K
    a.A, a.lda, a.B, a.ldb = x.data_ptr(), C, w.data_ptr(), K
    a.C, a.ldc = out.data_ptr(), Cout
    a.alpha = 1.0
    if bias is not None:
        a.ep.bias = bias.data_ptr()
    if residual is not None:
        a.ep.residual, a.ep.ldr = residual.data_ptr(), _ld(residual)
        a.ep.residual_first = int(bool(residual_first))
    a.ep.act = int(act)
    if x_planes is not None:
        if x_planes.dtype != torch.bfloat16 or tuple(x_planes.shape) != (3, N * H * W, C) or not x_planes.is_contiguous():
            raise ValueError("x_planes must be split3(x): contiguous bf16 [3, N*H*W, C]")
        a.a_planes = x_planes.data_ptr()
    a.conv = ctypes.addressof(g)
    need = lib().mmfd_gemm_workspace_bytes(ctypes.byref(a))
    if need < 0:
        raise RuntimeError("mmfd_gemm_workspace_bytes failed: " + lib().mmfd_last_error_string().decode())
    ws = torch.empty(max(need, 1), device=x.device, dtype=torch.uint8) if need > 0 else None
    if ws is not None:
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
    probe = _PROBE
    rec = probe is not None and not torch.cuda.is_current_stream_capturing()
    if rec:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    _check(lib().mmfd_gemm(ctypes.byref(a), _stream()), "mmfd_gemm (conv)")
    if rec:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        name = _gemm_plan(a)[1]
        probe.records.append((name, 2 * M * Cout * K, e0, e1))
    return out, Ho, Wo


def maxpool_nhwc(x, N, H, W, C, k=3, stride=2, pad=1):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((N * Ho * Wo, C), device=x.device, dtype=x.dtype)
    _check(lib().mmfd_maxpool_nhwc(dtype_code(x.dtype), N, H, W, C, k, stride, pad, Ho, Wo, _ptr(x), _ptr(out),
                                   _stream()), "mmfd_maxpool_nhwc")
    return out, Ho, Wo


def global_avgpool(x, N, HW, C):
    out = torch.empty((N, C), device=x.device, dtype=torch.float32)
    _check(lib().mmfd_global_avgpool(dtype_code(x.dtype), N, HW, C, _ptr(x), _ptr(out), _stream()),
           "mmfd_global_avgpool")
    return out


def embed_bwd(ids, tts, dsum, dword, dpos, dtype_emb, padding_idx=-1):
    """deterministic embedding-table gradients (csrc/embed_bwd.hip): sort-by-id word scatter-add"""
    B, L = ids.shape
    D = dsum.shape[-1]
    nws = lib().mmfd_embed_bwd_workspace_bytes(B, L, D)
    if nws < 0:
        raise RuntimeError("mmfd_embed_bwd_workspace_bytes failed")
    ws = torch.empty(max(nws, 1), device=dsum.device, dtype=torch.uint8)
    vocab = dword.shape[0] if dword is not None else 0  # the sort covers the id bits of the vocabulary only
    _check(lib().mmfd_embed_bwd(dtype_code(dsum.dtype), B, L, D, vocab, _ptr(ids), _ptr(tts) if tts is not None else None,
                                _ptr(dsum), _ptr(dword), _ptr(dpos), _ptr(dtype_emb), int(padding_idx), _ptr(ws), nws,
                                _stream()),
           "mmfd_embed_bwd")


def patchify(pixels, P, dtype):
    B, C, Hh, Ww = pixels.shape
    npch = (Hh // P) * (Ww // P)
    out = torch.empty((B * npch, C * P * P), device=pixels.device, dtype=dtype)
    _check(lib().mmfd_patchify(dtype_code(dtype), B, C, Hh, Ww, P, _ptr(pixels.contiguous().float()), _ptr(out),
                               _stream()), "mmfd_patchify")
    return out


def vit_tokens_fwd(patch, B, cls, pos):
    NP = patch.shape[0] // B
    D = patch.shape[1]
    out = torch.empty((B, NP + 1, D), device=patch.device, dtype=patch.dtype)
    _check(lib().mmfd_vit_tokens_fwd(dtype_code(patch.dtype), B, NP, D, _ptr(patch), _ptr(cls), _ptr(pos), _ptr(out),
                                     _stream()), "mmfd_vit_tokens_fwd")
    return out


def vit_tokens_bwd(dout, want_dpatch=True):
    B, T, D = dout.shape
    NP = T - 1
    dpatch = torch.empty((B * NP, D), device=dout.device, dtype=dout.dtype) if want_dpatch else None
    dcls = torch.empty(D, device=dout.device, dtype=torch.float32)
    dpos = torch.empty((T, D), device=dout.device, dtype=torch.float32)
    _check(lib().mmfd_vit_tokens_bwd(dtype_code(dout.dtype), B, NP, D, _ptr(dout.contiguous()), _ptr(dpatch),
                                     _ptr(dcls), _ptr(dpos), None, 0, _stream()), "mmfd_vit_tokens_bwd")
    return dpatch, dcls, dpos


def adamw(table_dev, n, max_numel, lr, beta1, beta2, eps, weight_decay):
    _ops().adamw(table_dev, int(n), int(max_numel), float(lr), float(beta1), float(beta2), float(eps),
                 float(weight_decay))


def dropout_hash(seed: int, salt: int, index: int) -> int:
    return int(lib().mmfd_dropout_hash(seed & 0xFFFFFFFFFFFFFFFF, salt & 0xFFFFFFFFFFFFFFFF, index))


# ------------------------------------------------------------------------------------------------
# retrieval scoring (csrc/retrieval.hip)
# ------------------------------------------------------------------------------------------------
_CORPUS_CODES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def cosine_scores(queries, corpus, mode=COS_PAIR, eps=1e-6, out=None):
    """fp32 [Q, N] cosine scores of fp32 queries [Q, D] against a corpus [N, D] (fp32 / bf16 / fp16)."""
    _require_cuda(queries, corpus, out)
    if queries.dim() == 1:
        queries = queries.unsqueeze(0)
    queries = queries.float().contiguous()
    corpus = corpus.contiguous()
    Q, D = queries.shape
    N = corpus.shape[0]
    if corpus.shape[1] != D:
        raise ValueError(f"query dim {D} != corpus dim {corpus.shape[1]}")
    if corpus.dtype not in _CORPUS_CODES:
        raise TypeError(f"unsupported corpus dtype {corpus.dtype}")
    if out is None:
        out = torch.empty(Q, N, device=corpus.device, dtype=torch.float32)
    _ld(corpus)
    _ops().cosine_scores(queries, corpus, int(mode), float(eps), out)
    return out


def topk(scores, k):
    """Per row of fp32 scores [Q, N]: the k largest, descending, ties -> lower index first.
    Returns (values fp32 [Q, k], indices int64 [Q, k]); missing entries are -inf / -1."""
    _require_cuda(scores)
    Q, N = scores.shape
    val = torch.empty(Q, k, device=scores.device, dtype=torch.float32)
    idx = torch.empty(Q, k, device=scores.device, dtype=torch.int64)
    _ld(scores)
    _ops().topk(scores, int(k), val, idx)
    return val, idx


# -------------------------------------------------------------------------------------------------
# Swinv2 (csrc/swin.hip)
# -------------------------------------------------------------------------------------------------
def row_gather(src, idx, B, rows_out, G=1, out=None):
    """src [B*src_rows, C] -> out [B*rows_out, G*C] with out row (b, r) = concat_g src row
    (b, idx[r*G+g]); idx int32 [rows_out*G] (one image's table, shared by the batch)"""
    _require_cuda(src, idx)
    if idx.dtype != torch.int32 or idx.numel() != rows_out * G:
        raise ValueError("row_gather: idx must be int32 [rows_out*G]")
    if not src.is_contiguous() or src.shape[0] % B:
        raise ValueError("row_gather: src must be contiguous [B*src_rows, C]")
    C = src.shape[1]
    if out is None:
        out = torch.empty((B * rows_out, G * C), device=src.device, dtype=src.dtype)
    _check(lib().mmfd_row_gather(B, rows_out, G, C * src.element_size(), src.shape[0] // B, _ptr(src), _ptr(idx),
                                 _ptr(out), _stream()), "mmfd_row_gather")
    return out


def swin_cpb(coords, w1, b1, w2, out=None):
    """continuous position-bias MLP table [T, H] (fp32) from coords [T, 2], w1 [512, 2], b1 [512], w2 [H, 512]"""
    _require_cuda(coords, w1, b1, w2)
    T, H = coords.shape[0], w2.shape[0]
    if w1.shape != (512, 2) or w2.shape[1] != 512:
        raise ValueError("swin_cpb: the position-bias MLP has 512 hidden units")
    ts = [t.float().contiguous() for t in (coords, w1, b1, w2)]
    if out is None:
        out = torch.empty((T, H), device=coords.device, dtype=torch.float32)
    _check(lib().mmfd_swin_cpb(T, H, *[_ptr(t) for t in ts], _ptr(out), _stream()), "mmfd_swin_cpb")
    return out


def swin_bias(table, rpi, L, mask=None, out=None):
    """[nW, H, L, L] fp32 = 16 sigmoid(table[rpi]) (+ 2 * mask[nW, L, L]); nW = 1 without a mask"""
    _require_cuda(table, rpi)
    H = table.shape[1]
    nW = mask.shape[0] if mask is not None else 1
    if out is None:
        out = torch.empty((nW, H, L, L), device=table.device, dtype=torch.float32)
    _check(lib().mmfd_swin_bias(nW, H, L, _ptr(table), _ptr(rpi), _ptr(mask) if mask is not None else None,
                                _ptr(out), _stream()), "mmfd_swin_bias")
    return out


def swin_qk_norm(qkv, H, d, logit_scale, max_log):
    """in place on packed QKV rows [rows, >= 2*H*d]: cosine-attention q (times the head's clamped
    exp(logit_scale)) and k"""
    _require_cuda(qkv, logit_scale)
    ls = logit_scale.float().contiguous()
    _check(lib().mmfd_swin_qk_norm(dtype_code(qkv.dtype), qkv.shape[0], H, d, _ptr(qkv), _ld(qkv), _ptr(ls),
                                   float(max_log), _stream()), "mmfd_swin_qk_norm")
    return qkv


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous fp32 tensor")
    return t


def swin_qk_norm_train(qkv, H, d, logit_scale, max_log):
    """swin_qk_norm (the same bits) that also returns the inverse norms: (qkv, inv fp32 [rows, 2, H]) with
    inv[r, 0 | 1, h] = 1 / max(|q_h| | |k_h|, 1e-12) — what swin_qk_norm_bwd reads"""
    _require_cuda(qkv, logit_scale)
    ls = _f32c(logit_scale, "logit_scale")
    if ls.numel() != H or qkv.shape[1] < 3 * H * d:
        raise ValueError("swin_qk_norm_train: qkv must be packed [rows, 3*H*d] rows and logit_scale hold H values")
    inv = torch.empty((qkv.shape[0], 2, H), device=qkv.device, dtype=torch.float32)
    _check(lib().mmfd_swin_qk_norm_train(dtype_code(qkv.dtype), qkv.shape[0], H, d, _ptr(qkv), _ld(qkv), _ptr(ls),
                                         float(max_log), _ptr(inv), _stream()), "mmfd_swin_qk_norm_train")
    return qkv, inv


def swin_qk_norm_bwd(dqkv, qkv_norm, inv, H, d, logit_scale, max_log):
    """adjoint of the cosine pass, in place on the q and k thirds of the packed gradient rows `dqkv`
    [rows, 3*H*d] (`qkv_norm`, `inv`: what swin_qk_norm_train left); returns (dqkv, d_logit_scale fp32 [H]),
    the latter exactly 0 for heads whose logit scale is past the clamp"""
    _require_cuda(dqkv, qkv_norm, inv, logit_scale)
    rows = dqkv.shape[0]
    ls = _f32c(logit_scale, "logit_scale")
    if dqkv.dtype != qkv_norm.dtype or qkv_norm.shape[0] != rows or min(dqkv.shape[1], qkv_norm.shape[1]) < 3 * H * d:
        raise ValueError("swin_qk_norm_bwd: dqkv and qkv_norm must be packed [rows, 3*H*d] rows of one dtype")
    if _f32c(inv, "inv").numel() != rows * 2 * H or ls.numel() != H:
        raise ValueError("swin_qk_norm_bwd: inv must be [rows, 2, H] and logit_scale hold H values")
    nws = lib().mmfd_swin_qk_norm_bwd_workspace_bytes(rows, H)
    ws = torch.empty(max(nws // 4, 1), device=dqkv.device, dtype=torch.float32)
    dls = torch.empty(H, device=dqkv.device, dtype=torch.float32)
    _check(lib().mmfd_swin_qk_norm_bwd(dtype_code(dqkv.dtype), rows, H, d, _ptr(dqkv), _ld(dqkv), _ptr(qkv_norm),
                                       _ld(qkv_norm), _ptr(inv), _ptr(ls), float(max_log), _ptr(dls), _ptr(ws), nws,
                                       _stream()), "mmfd_swin_qk_norm_bwd")
    return dqkv, dls


def swin_bias_bwd(d_bias, table, rpi, L):
    """adjoint of swin_bias: d_bias fp32 [nW, H, L, L] -> d_table fp32 [T, H] (the mask takes no gradient)"""
    _require_cuda(d_bias, table, rpi)
    T, H = table.shape
    if _f32c(d_bias, "d_bias").dim() != 4 or tuple(d_bias.shape[1:]) != (H, L, L):
        raise ValueError("swin_bias_bwd: d_bias must be [nW, H, L, L]")
    if rpi.dtype != torch.int32 or rpi.numel() != L * L or not rpi.is_contiguous():
        raise ValueError("swin_bias_bwd: rpi must be contiguous int32 [L*L]")
    out = torch.empty((T, H), device=table.device, dtype=torch.float32)
    _check(lib().mmfd_swin_bias_bwd(d_bias.shape[0], H, L, T, _ptr(d_bias), _ptr(_f32c(table, "table")), _ptr(rpi),
                                    _ptr(out), _stream()), "mmfd_swin_bias_bwd")
    return out


def swin_cpb_bwd(d_table, coords, w1, b1, w2):
    """adjoint of swin_cpb: (d_w1 [512, 2], d_b1 [512], d_w2 [H, 512]) fp32 from d_table [T, H]"""
    _require_cuda(d_table, coords, w1, b1, w2)
    T, H = d_table.shape
    if tuple(w1.shape) != (512, 2) or tuple(w2.shape) != (H, 512) or b1.numel() != 512 or tuple(coords.shape) != (T, 2):
        raise ValueError("swin_cpb_bwd: coords [T, 2], w1 [512, 2], b1 [512], w2 [H, 512], d_table [T, H]")
    for t, n in ((d_table, "d_table"), (coords, "coords"), (w1, "w1"), (b1, "b1"), (w2, "w2")):
        _f32c(t, n)
    dw1, db1, dw2 = (torch.empty(t.shape, device=d_table.device, dtype=torch.float32) for t in (w1, b1, w2))
    _check(lib().mmfd_swin_cpb_bwd(T, H, _ptr(coords), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(d_table), _ptr(dw1),
                                   _ptr(db1), _ptr(dw2), _stream()), "mmfd_swin_cpb_bwd")
    return dw1, db1, dw2


# -------------------------------------------------------------------------------------------------
# greedy decoding (csrc/decode.hip)
# -------------------------------------------------------------------------------------------------
def attn_decode_splits(B, H, Lk):
    """how many waves share the key range of one (b, h) in attn_decode (the library's own rule)"""
    s = lib().mmfd_attn_decode_splits(int(B), int(H), int(Lk))
    _check(0 if s > 0 else MMFD_ERR_INVALID, "mmfd_attn_decode_splits")
    return s


def attn_decode(q, k, v, H, Lk, *, scale=None, out=None, workspace=None, group=1):
    """single-token attention: q [B, H*D], k / v [B, Lmax, H*D] (views into a packed cache are fine), keys
    0 .. Lk-1 only (rows past Lk are never read); returns o [B, H*D]. `workspace`: a uint8 tensor of
    mmfd_attn_decode_workspace_bytes (allocated here when the key range is split and none is given).
    group > 1: k / v hold B / group rows and query row b attends row b // group (the beams of an image)."""
    _require_cuda(q, k, v, out, workspace)
    if q.dim() != 2 or k.dim() != 3 or v.dim() != 3 or q.stride(1) != 1 or k.stride(2) != 1 or v.stride(2) != 1:
        raise ValueError("attn_decode: q [B, H*D] and k / v [B, Lmax, H*D] views with a contiguous last dim")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError("attn_decode: q, k, v must share a dtype")
    B, HD = q.shape
    D = HD // H
    group = int(group)
    if group != 1 and (group < 1 or B % group or k.shape[0] * group != B or v.shape[0] * group != B):
        raise ValueError(f"attn_decode: {B} query rows in groups of {group} need {B // max(group, 1)} rows of k / v")
    if Lk > k.shape[1] or Lk > v.shape[1]:
        raise ValueError(f"attn_decode: Lk = {Lk} exceeds the cache rows ({k.shape[1]})")
    if out is None:
        out = torch.empty((B, HD), device=q.device, dtype=q.dtype)
    elif out.dtype != q.dtype or tuple(out.shape) != (B, HD) or out.stride(1) != 1:
        raise ValueError("attn_decode: out must be a [B, H*D] view of q's dtype with a contiguous last dim")
    need = lib().mmfd_attn_decode_workspace_bytes(B, H, D, int(Lk)) if B and Lk > 0 and D > 0 else 0
    if need > 0 and (workspace is None or workspace.numel() * workspace.element_size() < need):
        workspace = torch.empty(need, device=q.device, dtype=torch.uint8)
    tail = (float(scale if scale is not None else D ** -0.5), _ptr(q), q.stride(0), _ptr(k), k.stride(0), k.stride(1),
            _ptr(v), v.stride(0), v.stride(1), _ptr(out), out.stride(0), _ptr(workspace),
            workspace.numel() * workspace.element_size() if workspace is not None else 0, _stream())
    if group == 1:
        _check(lib().mmfd_attn_decode(dtype_code(q.dtype), B, H, D, int(Lk), *tail), "mmfd_attn_decode")
    else:
        _check(lib().mmfd_attn_decode_grouped(dtype_code(q.dtype), B, group, H, D, int(Lk), *tail),
               "mmfd_attn_decode_grouped")
    return out


def lm_head_slab(dtype, B, V, K):
    """vocabulary rows per workgroup of lm_head_argmax for these shapes"""
    s = lib().mmfd_lm_head_argmax_slab(dtype_code(dtype), int(B), int(V), int(K))
    _check(0 if s > 0 else MMFD_ERR_INVALID, "mmfd_lm_head_argmax_slab")
    return int(s)


def lm_head_argmax(x, W, bias=None, *, out=None, logits=None, workspace=None):
    """argmax_v (x @ W^T + bias) per row without writing the logits: x [B <= 32, K], W [V, K] (row-major
    views, one dtype), bias fp32 [V]. Returns int64 [B]; `logits` (fp32 [B, V] view) also receives them."""
    _require_cuda(x, W, bias, out, logits, workspace)
    if x.dtype != W.dtype:
        raise TypeError(f"lm_head_argmax operands must share a dtype ({x.dtype} vs {W.dtype})")
    B, Kd = x.shape
    V = W.shape[0]
    if W.shape[1] != Kd:
        raise ValueError(f"lm_head_argmax inner dims differ: {Kd} vs {W.shape[1]}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != V or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous fp32 vector of length V")
    if logits is not None and (logits.dtype != torch.float32 or tuple(logits.shape) != (B, V)):
        raise ValueError("logits must be an fp32 [B, V] view")
    if out is None:
        out = torch.empty(B, device=x.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or out.numel() != B or not out.is_contiguous():
        raise ValueError("out must be a contiguous int64 vector of length B")
    code = dtype_code(x.dtype)
    need = lib().mmfd_lm_head_argmax_workspace_bytes(code, B, V, Kd)
    _check(0 if need > 0 else MMFD_ERR_INVALID, "mmfd_lm_head_argmax")
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.uint8)
    _check(lib().mmfd_lm_head_argmax(code, B, V, Kd, _ptr(x), _ld(x), _ptr(W), _ld(W), _ptr(bias), _ptr(out),
                                     _ptr(logits), _ld(logits) if logits is not None else 0, _ptr(workspace),
                                     workspace.numel() * workspace.element_size(), _stream()), "mmfd_lm_head_argmax")
    return out


def lm_head_wide_workspace_bytes(dtype, B, V, K):
    """bytes of workspace lm_head_argmax_wide needs for these shapes"""
    need = lib().mmfd_lm_head_argmax_wide_workspace_bytes(dtype_code(dtype), int(B), int(V), int(K))
    _check(0 if need > 0 else MMFD_ERR_INVALID, "mmfd_lm_head_argmax_wide_workspace_bytes")
    return int(need)


def lm_head_argmax_wide(x, W, bias=None, *, out=None, logits=None, workspace=None):
    """lm_head_argmax for 1 <= B <= 256 rows: 32-row tiles through the same kernel body in one launch, every logit
    bit for bit what lm_head_argmax gives for the row's 32-row block (a short last block zero padded). A
    `workspace` that is given must hold lm_head_wide_workspace_bytes (it is never replaced here)."""
    _require_cuda(x, W, bias, out, logits, workspace)
    if x.dtype != W.dtype:
        raise TypeError(f"lm_head_argmax_wide operands must share a dtype ({x.dtype} vs {W.dtype})")
    B, Kd = x.shape
    V = W.shape[0]
    if W.shape[1] != Kd:
        raise ValueError(f"lm_head_argmax_wide inner dims differ: {Kd} vs {W.shape[1]}")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != V or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous fp32 vector of length V")
    if logits is not None and (logits.dtype != torch.float32 or tuple(logits.shape) != (B, V)):
        raise ValueError("logits must be an fp32 [B, V] view")
    if out is None:
        out = torch.empty(B, device=x.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or out.numel() != B or not out.is_contiguous():
        raise ValueError("out must be a contiguous int64 vector of length B")
    code = dtype_code(x.dtype)
    if workspace is None:
        need = lib().mmfd_lm_head_argmax_wide_workspace_bytes(code, B, V, Kd)
        _check(0 if need > 0 else MMFD_ERR_INVALID, "mmfd_lm_head_argmax_wide")
        workspace = torch.empty(need, device=x.device, dtype=torch.uint8)
    _check(lib().mmfd_lm_head_argmax_wide(code, B, V, Kd, _ptr(x), _ld(x), _ptr(W), _ld(W), _ptr(bias), _ptr(out),
                                          _ptr(logits), _ld(logits) if logits is not None else 0, _ptr(workspace),
                                          workspace.numel() * workspace.element_size(), _stream()),
           "mmfd_lm_head_argmax_wide")
    return out


def greedy_select(argmax, finished, eos, pad, next_tokens, forced=None):
    """one greedy step per row: next_tokens[b] = forced[b] if given, else pad if finished[b], else argmax[b];
    finished[b] |= (token == eos). argmax / forced / next_tokens: int64 [B] views (any stride), finished
    int32 [B] contiguous, updated in place."""
    _require_cuda(argmax, finished, next_tokens, forced)
    B = finished.numel()
    for t in (argmax, forced, next_tokens):
        if t is not None and (t.dtype != torch.int64 or t.dim() != 1 or t.numel() != B):
            raise ValueError("greedy_select: argmax / forced / next_tokens must be int64 [B] views")
    if finished.dtype != torch.int32 or not finished.is_contiguous():
        raise ValueError("greedy_select: finished must be a contiguous int32 [B] tensor")
    if argmax is not None and argmax.stride(0) != 1:
        raise ValueError("greedy_select: argmax must be contiguous")
    _check(lib().mmfd_greedy_select(B, _ptr(argmax), _ptr(forced), forced.stride(0) if forced is not None else 0,
                                    _ptr(finished), int(eos), int(pad), _ptr(next_tokens), next_tokens.stride(0),
                                    _stream()), "mmfd_greedy_select")
    return next_tokens


# ------------------------------------------------------------------------------------------------
# beam search (csrc/beam.hip)
# ------------------------------------------------------------------------------------------------
def beam_select_slab(V):
    """vocabulary entries per workgroup of beam_select"""
    s = lib().mmfd_beam_select_slab(int(V))
    _check(0 if s > 0 else MMFD_ERR_INVALID, "mmfd_beam_select_slab")
    return int(s)


def beam_select_workspace_bytes(B, nb, V):
    n = lib().mmfd_beam_select_workspace_bytes(int(B), int(nb), int(V))
    _check(0 if n > 0 else MMFD_ERR_INVALID, "mmfd_beam_select_workspace_bytes")
    return int(n)


def _i32(t, shape, what):
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int32 tensor of shape {tuple(shape)}")


def _f32(t, shape, what):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous fp32 tensor of shape {tuple(shape)}")


def beam_select(logits, running, nb, *, out=None, workspace=None, logprobs=False):
    """per image the 2 nb best (score, beam, token) of its nb * V candidates, score = log_softmax(logits[row])
    + running[row]: logits fp32 [B * nb, V] (rows may be strided), running fp32 [B * nb]. Returns (score fp32,
    beam int32, token int32), each [B, 2 nb], best first; equal scores go to the lower beam, then the lower
    token, and a NaN is never chosen over a number. logprobs: `logits` holds log-probabilities already
    (row_log_softmax, then logits_process): score = logits[row] + running[row], no normalisation."""
    _require_cuda(logits, running, workspace)
    nb = int(nb)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or nb < 1 or logits.shape[0] % nb:
        raise ValueError("beam_select: logits must be an fp32 [B * nb, V] view with a contiguous last dim")
    R, V = logits.shape
    B = R // nb
    _f32(running, (R,), "beam_select: running")
    if out is None:
        out = (torch.empty(B, 2 * nb, device=logits.device), torch.empty(B, 2 * nb, device=logits.device, dtype=torch.int32),
               torch.empty(B, 2 * nb, device=logits.device, dtype=torch.int32))
    _f32(out[0], (B, 2 * nb), "beam_select: out score")
    _i32(out[1], (B, 2 * nb), "beam_select: out beam")
    _i32(out[2], (B, 2 * nb), "beam_select: out token")
    _require_cuda(*out)
    if workspace is None:
        workspace = torch.empty(beam_select_workspace_bytes(B, nb, V), device=logits.device, dtype=torch.uint8)
    name = "mmfd_beam_select_logprobs" if logprobs else "mmfd_beam_select"
    _check(getattr(lib(), name)(B, nb, V, _ptr(logits), logits.stride(0), _ptr(running), _ptr(out[0]), _ptr(out[1]),
                                _ptr(out[2]), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                _stream()), name)
    return out


def beam_select_logprobs(logprobs, running, nb, *, out=None, workspace=None):
    """beam_select on log-probabilities (processed ones): score = logprobs[row] + running[row]"""
    return beam_select(logprobs, running, nb, out=out, workspace=workspace, logprobs=True)


def row_log_softmax_workspace_bytes(R, V):
    n = lib().mmfd_row_log_softmax_workspace_bytes(int(R), int(V))
    _check(0 if n > 0 else MMFD_ERR_INVALID, "mmfd_row_log_softmax_workspace_bytes")
    return int(n)


def row_log_softmax(logits, *, workspace=None):
    """logits fp32 [R, V] (rows may be strided) <- logits - logsumexp(row), in place: what transformers' beam search
    hands to the logits processors. The log-sum-exp is beam_select's."""
    _require_cuda(logits, workspace)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("row_log_softmax: logits must be an fp32 [R, V] view with a contiguous last dim")
    R, V = logits.shape
    if workspace is None:
        workspace = torch.empty(row_log_softmax_workspace_bytes(R, V), device=logits.device, dtype=torch.uint8)
    _check(lib().mmfd_row_log_softmax(R, V, _ptr(logits), logits.stride(0), _ptr(workspace),
                                      workspace.numel() * workspace.element_size(), _stream()), "mmfd_row_log_softmax")
    return logits


def beam_update(cand, state, t, n_forced, last, eos, length_penalty, early_stopping, next_tokens):
    """one beam step on the device state `state` (dict: run_score, fin_score fp32 [B, nb]; fin_flag, fin_len int32
    [B, nb]; run_seq, fin_seq int32 [B, nb, T]; flags int32 [B, 4]; parent int32 [B * nb]) from the candidates
    `cand` of beam_select: the step that embedded position t chooses position t + 1 (include/mmfd.h
    mmfd_beam_update). next_tokens: int64 [B * nb] view receiving the token of every new beam."""
    B, nb, T = state["run_seq"].shape
    _require_cuda(*cand, next_tokens, *(state[k] for k in ("run_score", "fin_score", "fin_flag", "fin_len", "run_seq",
                                                             "fin_seq", "flags", "parent")))
    _f32(cand[0], (B, 2 * nb), "beam_update: candidate scores")
    _i32(cand[1], (B, 2 * nb), "beam_update: candidate beams")
    _i32(cand[2], (B, 2 * nb), "beam_update: candidate tokens")
    _f32(state["run_score"], (B, nb), "beam_update: run_score")
    _f32(state["fin_score"], (B, nb), "beam_update: fin_score")
    _i32(state["fin_flag"], (B, nb), "beam_update: fin_flag")
    _i32(state["fin_len"], (B, nb), "beam_update: fin_len")
    _i32(state["run_seq"], (B, nb, T), "beam_update: run_seq")
    _i32(state["fin_seq"], (B, nb, T), "beam_update: fin_seq")
    _i32(state["flags"], (B, 4), "beam_update: flags")
    _i32(state["parent"], (B * nb,), "beam_update: parent")
    if next_tokens.dtype != torch.int64 or next_tokens.dim() != 1 or next_tokens.numel() != B * nb:
        raise ValueError("beam_update: next_tokens must be an int64 [B * nb] view")
    gen_len = int(t) + 1 - int(n_forced)
    if gen_len < 1:
        raise ValueError("beam_update: a forced step has no beam update")
    _check(lib().mmfd_beam_update(B, nb, T, int(t), gen_len, int(bool(last)), int(bool(early_stopping)), int(eos),
                                  float(float(gen_len) ** float(length_penalty)), _ptr(cand[0]), _ptr(cand[1]),
                                  _ptr(cand[2]), _ptr(state["run_score"]), _ptr(state["fin_score"]),
                                  _ptr(state["fin_flag"]), _ptr(state["fin_len"]), _ptr(state["run_seq"]),
                                  _ptr(state["fin_seq"]), _ptr(state["flags"]), _ptr(state["parent"]),
                                  _ptr(next_tokens), next_tokens.stride(0), _stream()), "mmfd_beam_update")


def ptr_table(tensors):
    """int64 device tensor of the tensors' addresses (the `src` / `dst` of beam_reorder)"""
    _require_cuda(*tensors)
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=tensors[0].device)


def beam_reorder(src, dst, src_table, dst_table, parent, beam_rows, n_pos):
    """dst[l][r, :n_pos] = src[l][parent[r], :n_pos] for r < beam_rows (the other rows copy themselves), all
    layers in one launch. src / dst: lists of equally shaped contiguous [rows, steps, width] caches whose
    addresses src_table / dst_table (ptr_table) hold; positions at and past n_pos are not touched."""
    _require_cuda(src_table, dst_table, parent)
    a = src[0]
    rows, steps, width = a.shape
    for s, d in zip(src, dst):
        if (s.shape != a.shape or d.shape != a.shape or s.dtype != a.dtype or d.dtype != a.dtype or not s.is_contiguous()
                or not d.is_contiguous() or s.data_ptr() == d.data_ptr()):
            raise ValueError("beam_reorder: src / dst must be distinct contiguous caches of one shape and dtype")
    if len(src) != len(dst) or src_table.numel() != len(src) or dst_table.numel() != len(dst) \
            or src_table.dtype != torch.int64 or dst_table.dtype != torch.int64:
        raise ValueError("beam_reorder: one int64 address per layer")
    if not 0 <= int(n_pos) <= steps:
        raise ValueError(f"beam_reorder: n_pos = {n_pos} exceeds the cache rows ({steps})")
    if parent.dtype != torch.int32 or parent.numel() < int(beam_rows) or not parent.is_contiguous():
        raise ValueError("beam_reorder: parent must be a contiguous int32 vector of at least beam_rows entries")
    es = a.element_size()
    _check(lib().mmfd_beam_reorder(len(src), rows, int(beam_rows), steps * width * es, int(n_pos) * width * es,
                                   _ptr(src_table), _ptr(dst_table), _ptr(parent), _stream()), "mmfd_beam_reorder")


# ------------------------------------------------------------------------------------------------
# sampling (csrc/sample.hip)
# ------------------------------------------------------------------------------------------------
def sample_select_resident_max():
    """the longest row whose keys sample_select keeps in LDS (longer rows re-read the logits on every pass)"""
    return int(lib().mmfd_sample_select_resident_max())


def sample_select_workspace_bytes(R, V):
    n = lib().mmfd_sample_select_workspace_bytes(int(R), int(V))
    _check(0 if n > 0 else MMFD_ERR_INVALID, "mmfd_sample_select_workspace_bytes")
    return int(n)


def check_sampling(temperature, top_k, top_p):
    """the host-side refusal of sampling parameters transformers' warpers refuse too"""
    t, p = float(temperature), float(top_p)
    if not (t > 0.0 and t != float("inf")):
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0 (0: no filter), got {top_k!r}")
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"top_p must lie in [0, 1], got {top_p!r}")
    return t, int(top_k), p


def sample_select(logits, temperature, top_k, top_p, ctl, step, *, out=None, probs=None, kept=None, workspace=None):
    """one sampled token per row of logits fp32 [R, V] (rows may be strided): temperature, top-k and top-p
    filters in transformers' order, softmax, and one draw with u = (hash(seed, step, row0 + r) >> 8) * 2^-24
    (include/mmfd.h mmfd_sample_select). ctl: int64 [2] device tensor {seed, row0}. Returns out int64 [R];
    probs (fp32 [R, >= V] view, optional) receives the filtered distribution, kept (int32 [R], optional) the
    number of entries that survived the filters. Equal logits are ordered by the lower index; a NaN is never
    kept."""
    _require_cuda(logits, ctl, out, probs, kept, workspace)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("sample_select: logits must be an fp32 [R, V] view with a contiguous last dim")
    R, V = logits.shape
    t, k, p = check_sampling(temperature, top_k, top_p)
    if ctl.dtype != torch.int64 or ctl.numel() != 2 or not ctl.is_contiguous():
        raise ValueError("sample_select: ctl must be a contiguous int64 tensor {seed, row0}")
    if int(step) < 0:
        raise ValueError(f"sample_select: step = {step}")
    if out is None:
        out = torch.empty(R, device=logits.device, dtype=torch.int64)
    if out.dtype != torch.int64 or tuple(out.shape) != (R,) or not out.is_contiguous():
        raise ValueError(f"sample_select: out must be a contiguous int64 tensor of shape ({R},)")
    if probs is not None and (probs.dtype != torch.float32 or probs.dim() != 2 or probs.shape[0] != R
                              or probs.shape[1] < V or probs.stride(1) != 1):
        raise ValueError("sample_select: probs must be an fp32 [R, >= V] view with a contiguous last dim")
    if kept is not None:
        _i32(kept, (R,), "sample_select: kept")
    if workspace is None:
        workspace = torch.empty(sample_select_workspace_bytes(R, V), device=logits.device, dtype=torch.uint8)
    _check(lib().mmfd_sample_select(R, V, _ptr(logits), logits.stride(0), t, k, p, _ptr(ctl), int(step), _ptr(out),
                                    _ptr(probs), probs.stride(0) if probs is not None else 0, _ptr(kept),
                                    _ptr(workspace), workspace.numel() * workspace.element_size(), _stream()),
           "mmfd_sample_select")
    return out


# ------------------------------------------------------------------------------------------------
# logits processors (csrc/logits.hip)
# ------------------------------------------------------------------------------------------------
MAX_SUPPRESS = 64      # ids in a suppress list (csrc/logits.hip LGT_MAX_SUPPRESS)
MAX_HISTORY = 1024     # history positions a row may hold (LGT_MAX_LEN)


def _int_arg(v, name, lo=0):
    if isinstance(v, bool) or int(v) != v or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


def check_processors(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, min_new_tokens=0,
                     suppress_tokens=None, vocab_size=None):
    """the host-side refusal of processor arguments transformers' classes refuse too. Returns (penalty, ngram,
    min_length, min_new_tokens, suppress) with suppress a tuple of ints (None -> ())."""
    try:
        p = float(repetition_penalty)
    except (TypeError, ValueError):
        p = float("nan")
    if not (p > 0.0 and p != float("inf")):
        raise ValueError(f"repetition_penalty must be a finite number > 0, got {repetition_penalty!r}")
    n = _int_arg(no_repeat_ngram_size, "no_repeat_ngram_size")
    ml = _int_arg(min_length, "min_length")
    mn = _int_arg(min_new_tokens, "min_new_tokens")
    if suppress_tokens is None:
        sup = ()
    else:
        if isinstance(suppress_tokens, torch.Tensor):
            suppress_tokens = suppress_tokens.reshape(-1).tolist()
        sup = tuple(_int_arg(i, "suppress_tokens entries") for i in suppress_tokens)
        if len(sup) > MAX_SUPPRESS:
            raise ValueError(f"suppress_tokens holds {len(sup)} ids, at most {MAX_SUPPRESS} are supported")
        if vocab_size is not None and any(i >= vocab_size for i in sup):
            raise ValueError(f"suppress_tokens outside [0, {vocab_size})")
    return p, n, ml, mn, sup


def logits_process(scores, history, cur_len, *, repetition_penalty=1.0, no_repeat_ngram_size=0, suppress_eos=False,
                   eos=0, suppress=None, n_suppress=None, history_layout="rows"):
    """transformers' logits processors in place on scores fp32 [R, V] (rows may be strided), from each row's own
    history (include/mmfd.h mmfd_logits_process): the repetition penalty on the scores as passed, then -inf into
    the columns no_repeat_ngram_size bans, into `eos` when suppress_eos, and into the first n_suppress ids of the
    device list `suppress` (int64, at most 64). history: int64 or int32, [R', >= cur_len] with
    history_layout="rows" (row r, position i at history[r, i]) or [>= cur_len, R'] with "steps" (history[i, r]),
    R' >= R, any strides. Greedy decoding and sampling pass the raw logits, beam search row_log_softmax's output."""
    _require_cuda(scores, history, suppress)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError("logits_process: scores must be an fp32 [R, V] view with a contiguous last dim")
    R, V = scores.shape
    p, n, _, _, _ = check_processors(repetition_penalty, no_repeat_ngram_size)
    cur_len = int(cur_len)
    if history.dtype not in (torch.int64, torch.int32) or history.dim() != 2:
        raise ValueError("logits_process: history must be a 2-D int64 or int32 tensor")
    if history_layout not in ("rows", "steps"):
        raise ValueError(f"logits_process: history_layout must be 'rows' or 'steps', got {history_layout!r}")
    rdim, pdim = (0, 1) if history_layout == "rows" else (1, 0)
    if not 1 <= cur_len <= min(history.shape[pdim], MAX_HISTORY) or history.shape[rdim] < R:
        raise ValueError(f"logits_process: history {tuple(history.shape)} ({history_layout}) does not hold {R} rows of "
                         f"cur_len = {cur_len} (1 .. {MAX_HISTORY}) ids")
    if history.stride(rdim) < 0 or history.stride(pdim) < 1:
        raise ValueError("logits_process: history strides must be positive")
    if suppress is None:
        n_sup = 0
    else:
        if suppress.dtype != torch.int64 or suppress.dim() != 1 or not suppress.is_contiguous():
            raise ValueError("logits_process: suppress must be a contiguous int64 vector")
        n_sup = suppress.numel() if n_suppress is None else int(n_suppress)
        if not 0 <= n_sup <= min(suppress.numel(), MAX_SUPPRESS):
            raise ValueError(f"logits_process: {n_sup} suppressed ids (at most {MAX_SUPPRESS}, and the list's length)")
    if suppress_eos and not 0 <= int(eos) < V:
        raise ValueError(f"logits_process: eos = {eos} outside [0, {V})")
    _check(lib().mmfd_logits_process(R, V, _ptr(scores), scores.stride(0), _ptr(history), history.stride(rdim),
                                     history.stride(pdim), history.element_size(), cur_len, p, n,
                                     int(bool(suppress_eos)), int(eos), _ptr(suppress) if n_sup else None, n_sup,
                                     _stream()), "mmfd_logits_process")
    return scores


def row_argmax(scores, *, out=None):
    """argmax per row of scores fp32 [R, V] (rows may be strided): ties to the lowest index, a NaN never over a
    number — lm_head_argmax's order, for scores edited after the LM head wrote them. Returns int64 [R]."""
    _require_cuda(scores, out)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError("row_argmax: scores must be an fp32 [R, V] view with a contiguous last dim")
    R, V = scores.shape
    if out is None:
        out = torch.empty(R, device=scores.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (R,) or not out.is_contiguous():
        raise ValueError(f"row_argmax: out must be a contiguous int64 tensor of shape ({R},)")
    _check(lib().mmfd_row_argmax(R, V, _ptr(scores), scores.stride(0), _ptr(out), _stream()), "mmfd_row_argmax")
    return out


# ------------------------------------------------------------------------------------------------
# vocabulary cross-entropy (csrc/lm_loss.hip): the caption loss of the BLIP text decoder
# ------------------------------------------------------------------------------------------------
IGNORE_INDEX = -100


def check_vocab_labels(labels, V):
    """the host-side refusal of a label that is neither in [0, V) nor IGNORE_INDEX, before anything is
    launched (a device tensor is copied to the host for it: one synchronisation)"""
    lab = labels.detach().cpu()
    bad = (lab != IGNORE_INDEX) & ((lab < 0) | (lab >= V))
    if bool(bad.any()):
        raise ValueError(f"vocab_xent: label {int(lab[bad][0])} is neither in [0, {V}) nor {IGNORE_INDEX}")


def _xent_args(logits, labels):
    _require_cuda(logits, labels)
    if logits.dtype != torch.float32:
        raise ValueError("vocab_xent: logits must be fp32")
    R, V = logits.shape
    ld = _ld(logits)
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.numel() != R or not labels.is_contiguous():
        raise ValueError(f"vocab_xent: labels must be a contiguous int64 vector of {R} entries")
    return R, V, ld


def vocab_xent_fwd(logits, labels, eps=0.0, rows_per_seq=None, check_labels=True):
    """CrossEntropyLoss(label_smoothing=eps, ignore_index=-100) of fp32 logits [R, V] (a row-major view, leading
    dimension >= V) against int64 labels [R]: (loss_rows [R] (0 where ignored), lse [R], lse_lo [R], mean over the
    valid rows (a 0-d tensor; NaN without one), n_valid (int64, 0-d), seq_sums [R / rows_per_seq] or None). All
    fp32 device tensors; nothing visits the host unless `check_labels` (check_vocab_labels). `lse_lo` holds what
    fp32 rounded away from lse (include/mmfd.h); vocab_xent_bwd takes the two together."""
    R, V, ld = _xent_args(logits, labels)
    if check_labels and V >= 1:
        check_vocab_labels(labels, V)
    dev = logits.device
    loss_rows = torch.empty(R, device=dev, dtype=torch.float32)
    lse = torch.empty(R, device=dev, dtype=torch.float32)
    lse_lo = torch.empty(R, device=dev, dtype=torch.float32)
    mean = torch.empty((), device=dev, dtype=torch.float32)
    n_valid = torch.empty((), device=dev, dtype=torch.int64)
    seq = torch.empty(R // rows_per_seq, device=dev, dtype=torch.float32) if rows_per_seq else None
    _check(lib().mmfd_vocab_xent_fwd(R, V, _ptr(logits), ld, _ptr(labels), float(eps), int(rows_per_seq or 0),
                                     _ptr(loss_rows), _ptr(lse), _ptr(lse_lo), _ptr(mean), _ptr(n_valid), _ptr(seq),
                                     _stream()),
           "mmfd_vocab_xent_fwd")
    return loss_rows, lse, lse_lo, mean, n_valid, seq


def vocab_xent_bwd(logits, labels, lse, lse_lo, eps, dtype, *, upstream=None, n_valid=None, rows_per_seq=None, out=None):
    """dlogits [R, V] in `dtype` (fp32 / bf16) of vocab_xent_fwd's loss, from the forward's `lse` and `lse_lo`
    (fp32 [R] each). Mean form: `n_valid` (the forward's device counter) and `upstream` a 1-element fp32 tensor or
    None (= 1); per-sequence form: n_valid None, `upstream` fp32 [R / rows_per_seq] weights. `out`: a row-major
    [R, V] view (leading dimension >= V) to write into; nothing is written past column V."""
    R, V, ld = _xent_args(logits, labels)
    for name, t in (("lse", lse), ("lse_lo", lse_lo)):
        if t is None or t.dtype != torch.float32 or t.dim() != 1 or t.numel() != R or not t.is_contiguous():
            raise ValueError(f"vocab_xent_bwd: {name} must be the forward's contiguous fp32 vector of {R} entries")
    if out is None:
        out = torch.empty((R, V), device=logits.device, dtype=dtype)
    if out.dtype != dtype or out.shape[0] != R or out.shape[1] != V:
        raise ValueError("vocab_xent_bwd: out must be [R, V] of the requested dtype")
    if upstream is not None and (upstream.dtype != torch.float32 or not upstream.is_contiguous()):
        raise ValueError("vocab_xent_bwd: upstream must be a contiguous fp32 tensor")
    if n_valid is None and (upstream is None or not rows_per_seq or upstream.numel() * rows_per_seq != R):
        raise ValueError("vocab_xent_bwd: the per-sequence form needs one upstream weight per rows_per_seq rows")
    if n_valid is not None and (n_valid.dtype != torch.int64 or n_valid.numel() != 1):
        raise ValueError("vocab_xent_bwd: n_valid must be the forward's int64 counter")
    _require_cuda(lse, lse_lo, upstream, n_valid, out)
    _check(lib().mmfd_vocab_xent_bwd(dtype_code(dtype), R, V, _ptr(logits), ld, _ptr(labels), _ptr(lse), _ptr(lse_lo), float(eps),
                                     _ptr(upstream), _ptr(n_valid), int(rows_per_seq or 0), _ptr(out), _ld(out),
                                     _stream()), "mmfd_vocab_xent_bwd")
    return out
