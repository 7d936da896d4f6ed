// Flash-style multi-head attention for gfx950 (head_dim 32 or 64, L <= a few hundred).
//
// Replaces: src/model/layers.py:36-58 (MultiHeadAttention, eager and SDPA branches; no mask) and the
// self-attention of the HF BERT / ViT / MPNet encoders called at train.py:137-143 (key padding mask
// as an additive per-key bias, MPNet relative-position bias as an additive [H][Lq][Lk] bias).
//
// Dropout on P (layers.py:53 / SDPA dropout_p) is counter based: index ((b*H+h)*Lq+q)*Lk+k.
//
// The device code lives in four headers, one per kernel family, all compiled in this one translation
// unit (the compiler's output for a kernel depends on its neighbours in the unit):
//   attn_common.h    AttnP, keep-bitmask / plane stores, pair-hash dropout, LDS images and fragments
//   attn_stream.h    "stream":   64-row blocks through LDS, any length
//   attn_resident.h  "resident": the head's K/V (or Q/dO) staged in LDS once (the v2 kernels)
//   attn_split.h     "split":    fp32 on three bf16 planes per operand (the x6 kernels)
// This file is the host half: switches, argument checks, the launch plan, the C entry points.
#include "attn_common.h"
#include "attn_stream.h"
#include "attn_resident.h"
#include "attn_split.h"
#include <algorithm>
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {

// ---------------------------------------------------------------------------------------------
// load-time switches: the environment is read here, once, and nowhere else
// ---------------------------------------------------------------------------------------------
// A/B switch: MMFD_ATTN_V2_GENERIC=1 (or mmfd_debug_set_attn_v2_generic) runs every v2 call on mode 0
int g_v2_generic = [] {
  const char* v = getenv("MMFD_ATTN_V2_GENERIC");
  return v && atoi(v) != 0 ? 1 : 0;
}();

// A/B switch: MMFD_ATTN_V1=1 sends every call to the streaming v1 kernels
const bool g_attn_v1 = getenv("MMFD_ATTN_V1") != nullptr;

// MMFD_FP32_ATTN (else MMFD_FP32_GEMM) = native / 0: fp32 calls on the fp32 MFMA (mmfd_set_fp32_attn_mode)
int g_fp32_attn_mode = [] {
  const char* v = getenv("MMFD_FP32_ATTN");
  const char* gm = getenv("MMFD_FP32_GEMM");
  const bool native = (v && (!strcmp(v, "native") || !strcmp(v, "0"))) ||
                      (!v && gm && (!strcmp(gm, "native") || !strcmp(gm, "0")));
  return native ? 0 : 1;
}();

// MMFD_X6A_DBG: the x6 phase experiments of AttnP::dbg
const int g_x6a_dbg = getenv("MMFD_X6A_DBG") ? atoi(getenv("MMFD_X6A_DBG")) : 0;

// ---------------------------------------------------------------------------------------------
// argument checks; AttnP from the checked arguments
// ---------------------------------------------------------------------------------------------
int fill(const mmfd_attn_args& a, AttnP& p, bool bwd) {
  MMFD_CHECK_ARG(a.dtype == MMFD_F32 || a.dtype == MMFD_BF16, "attn: bad dtype");
  MMFD_CHECK_ARG(a.D > 0 && a.D <= 64, "attn: head_dim %lld unsupported (<= 64)", (long long)a.D);
  MMFD_CHECK_ARG(a.B >= 0 && a.H > 0 && a.Lq >= 0 && a.Lk > 0, "attn: bad shape");
  MMFD_CHECK_ARG(a.q && a.k && a.v && a.o && a.lse, "attn: null pointer");
  const int epc = a.dtype == MMFD_BF16 ? 8 : 4;
  MMFD_CHECK_ARG(a.D % epc == 0, "attn: head_dim*element_size must be a multiple of 16 bytes");
  auto al = [&](const void* ptr, int64_t sb, int64_t st) {
    return ((uintptr_t)ptr & 15) == 0 && sb % epc == 0 && st % epc == 0;
  };
  MMFD_CHECK_ARG(al(a.q, a.q_sb, a.q_st) && al(a.k, a.k_sb, a.k_st) && al(a.v, a.v_sb, a.v_st),
                 "attn: q/k/v must be 16-B aligned with strides multiple of 16 B");
  MMFD_CHECK_ARG(a.dropout_p <= 0.f || a.seed, "attn: dropout needs seed");
  MMFD_CHECK_ARG(a.dropout_p < 1.f, "attn: dropout p must be < 1");
  if (bwd) {
    MMFD_CHECK_ARG(a.dout && a.dq && a.dk && a.dv && a.delta, "attn_bwd: null pointer");
    MMFD_CHECK_ARG(al(a.dout, a.do_sb, a.do_st), "attn_bwd: dout alignment");
    if (a.d_rel_bias) {  // the gradient of a per-batch bias (attn_bwd_ds_kernel)
      MMFD_CHECK_ARG(a.rel_bias && a.rel_bias_sb == a.H * a.Lq * a.Lk && a.rel_bias_mod == 0,
                     "attn_bwd: d_rel_bias needs a per-batch rel_bias [B][H][Lq][Lk] (rel_bias_sb = H*Lq*Lk, rel_bias_mod = 0)");
      MMFD_CHECK_ARG(a.dropout_p <= 0.f, "attn_bwd: d_rel_bias with attention dropout is not supported");
      MMFD_CHECK_ARG((const float*)a.d_rel_bias != a.rel_bias, "attn_bwd: d_rel_bias must not alias rel_bias");
      MMFD_CHECK_ARG(((uintptr_t)a.d_rel_bias & 15) == 0, "attn_bwd: d_rel_bias must be 16-B aligned");
      MMFD_CHECK_ARG(a.B * a.H <= 65535, "attn_bwd: d_rel_bias needs B*H <= 65535");
    }
    MMFD_CHECK_ARG(a.cos_logit_scale == nullptr, "attn_bwd: cosine attention is inference-only");
  }
  p.B = a.B; p.H = a.H; p.Lq = a.Lq; p.Lk = a.Lk; p.scale = a.scale; p.D = (int)a.D;
  p.q = a.q; p.q_sb = a.q_sb; p.q_st = a.q_st;
  p.k = a.k; p.k_sb = a.k_sb; p.k_st = a.k_st;
  p.v = a.v; p.v_sb = a.v_sb; p.v_st = a.v_st;
  p.o = a.o; p.o_sb = a.o_sb; p.o_st = a.o_st;
  p.lse = a.lse; p.key_bias = a.key_bias; p.rel_bias = a.rel_bias; p.rb_sb = a.rel_bias ? a.rel_bias_sb : 0;
  p.rb_mod = a.rel_bias ? a.rel_bias_mod : 0;
  p.cos_ls = a.cos_logit_scale; p.cos_max_log = a.cos_max_log;
  p.p = a.dropout_p > 0.f ? a.dropout_p : 0.f; p.thr16 = mmfd_drop_threshold16(p.p); p.kp = (a.Lk + 1) / 2;
  p.keep_scale = 1.0f / (1.0f - p.p); p.seed = a.seed; p.salt = a.salt;
  p.dout = a.dout; p.do_sb = a.do_sb; p.do_st = a.do_st;
  p.dq = a.dq; p.dq_sb = a.dq_sb; p.dq_st = a.dq_st;
  p.dk = a.dk; p.dk_sb = a.dk_sb; p.dk_st = a.dk_st;
  p.dv = a.dv; p.dv_sb = a.dv_sb; p.dv_st = a.dv_st;
  p.delta = a.delta;
  p.acc_dq = a.accumulate_dq; p.acc_dkv = a.accumulate_dkv;
  p.idx32 = (uint64_t)a.B * (uint64_t)a.H * (uint64_t)a.Lq * (uint64_t)a.Lk <= (1ull << 32);
  auto al4 = [](const void* ptr, int64_t sb, int64_t st) {
    return ptr && ((uintptr_t)ptr & 15) == 0 && sb % 4 == 0 && st % 4 == 0;
  };
  // (the forward keeps its per-element stores: the 4-column form measured 2-8 % slower there)
  p.vst = a.dtype == MMFD_F32 && bwd && al4(a.dq, a.dq_sb, a.dq_st) && al4(a.dk, a.dk_sb, a.dk_st) &&
          al4(a.dv, a.dv_sb, a.dv_st);
  p.pl = nullptr; p.pl_stride = 0; p.pl_base = nullptr; p.pl_only = 0;
  p.dbg = g_x6a_dbg;
  p.dm = p.p > 0.f ? a.drop_mask : nullptr;
  p.dmw = (int)((a.Lk + 31) / 32);
  p.dm_lds = 0;
  MMFD_CHECK_ARG(!p.dm || ((uintptr_t)p.dm & 3) == 0, "attn: drop_mask must be 4-B aligned");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// the launch plan: everything a call decides before it launches
// ---------------------------------------------------------------------------------------------
enum Family { STREAM, RESIDENT, SPLIT };
const char* const FAMILY_NAME[] = {"stream", "resident", "split"};

// One kernel instantiation: its host handle and, from the same spelling of the template arguments,
// what the plan export prints (bf: the dtype argument, -1 = the kernel has none; then the integer
// arguments). attr_set is the once-flag of this instantiation's dynamic-LDS maximum.
struct Kern { const void* fn; const char* name; int bf; int narg; int arg[4]; bool* attr_set; };
#define KERN_REST(...) (int)std::initializer_list<int>{__VA_ARGS__}.size(), {__VA_ARGS__}, [] { static bool set = false; return &set; }()
#define KERN_TD(name, ...) Kern{(const void*)&name<T, D, ##__VA_ARGS__>, #name, sizeof(T) == 2, KERN_REST(D, ##__VA_ARGS__)}
#define KERN_D(name, ...) Kern{(const void*)&name<D, ##__VA_ARGS__>, #name, -1, KERN_REST(D, ##__VA_ARGS__)}

// lds_max != 0: the maximum the kernel's dynamic-LDS attribute is raised to before its first launch
struct Step { Kern k; dim3 grid; unsigned block; int lds, lds_max; const char* what; };
struct Plan {
  Family family;
  int n;
  Step step[4];
  bool split3;  // mmfd_split3 of the fp32 output follows (the streaming kernels write no planes)
  void add(const Kern& k, dim3 grid, unsigned block, int lds, int lds_max, const char* what) {
    step[n++] = Step{k, grid, block, lds, lds_max, what};
  }
};

// Which family takes the call. The forward and the backward differ on purpose:
//   split   : fp32 in split mode without a relative bias, D <= 64 in 16-B-pair chunks, dropout indices
//             within 32 bits (hash_c1), and the resident rows padded to 16 within X6A_LMAX = 208 — the
//             keys in the forward, keys and queries in the backward
//   resident: forward up to V2_LMAX = 256 keys, any number of queries, and bf16 up to V2_LMAX_FWD = 512
//             keys only when B*H >= 256 — one workgroup per (b, h) fills the chip only with enough
//             heads (a batch-1 pair at L = 512 runs faster on the 64-query-block streaming kernel),
//             and fp32 K/V images of 512 keys would not fit the LDS; backward only up to 256 keys
//             and 256 queries (its dK/dV kernel keeps the head's Q/dO resident)
//   stream  : everything else, and every call under MMFD_ATTN_V1
Family family_of(const mmfd_attn_args& a, bool bwd) {
  if (g_attn_v1) return STREAM;
  const bool bf = a.dtype == MMFD_BF16;
  if (g_fp32_attn_mode == 1 && !bf && !a.rel_bias && !a.cos_logit_scale && a.D % 8 == 0 &&
      v2_pad(a.Lk, 16) <= X6A_LMAX && (!bwd || v2_pad(a.Lq, 16) <= X6A_LMAX) &&
      !(a.dropout_p > 0.f && (uint64_t)a.B * (uint64_t)a.H * (uint64_t)a.Lq * (uint64_t)a.Lk > (1ull << 32)))
    return SPLIT;
  if (bwd) return a.Lk <= V2_LMAX && a.Lq <= V2_LMAX ? RESIDENT : STREAM;
  return a.Lk <= V2_LMAX || (bf && a.Lk <= V2_LMAX_FWD && a.B * a.H >= 256) ? RESIDENT : STREAM;
}

// the fixed v2 mode for these arguments (see V2_RESCALE_TH): 1 plain, 2 hashed dropout with or
// without a key bias (the per-key bias vector is staged either way: 0 for real keys when there is
// none, -inf for the padding — round 6: the fusion head's dropout-only attention had run the
// generic mode at ~50 VALU instructions per MFMA), 0 anything else (relative bias, keep-bitmask,
// a key bias without dropout)
inline int v2_mode(const AttnP& p) {
  if (p.rel_bias || g_v2_generic) return 0;
  if (p.p == 0.f && !p.key_bias) return 1;
  if (p.p > 0.f && !p.dm) return 2;
  return 0;
}

// the relative-bias instantiation carries the extra loads / registers; plain attention (BERT, ViT,
// fusion head) keeps the bias-free one; the fixed modes exist for one head per workgroup only
template <typename T, int D, int HPB>
Kern fwd_v2_kern(const AttnP& p) {
  if (p.rel_bias) return KERN_TD(attn_fwd_v2_kernel, HPB, true, 0);
  if constexpr (HPB == 1) {
    const int mode = v2_mode(p);
    if (mode == 1) return KERN_TD(attn_fwd_v2_kernel, 1, false, 1);
    if (mode == 2) return KERN_TD(attn_fwd_v2_kernel, 1, false, 2);
  }
  return KERN_TD(attn_fwd_v2_kernel, HPB, false, 0);
}

// the dS kernel: the dropout-free instantiation keeps the name it has had in the plan export
// (attn_bwd_ds_kernel<T,D>), the dropout one prints its flag (attn_bwd_ds_kernel<T,D,1>)
template <typename T, int D, bool DROP>
Kern ds_kern() {
  if constexpr (DROP) return KERN_TD(attn_bwd_ds_kernel, true);
  else return Kern{(const void*)&attn_bwd_ds_kernel<T, D, false>, "attn_bwd_ds_kernel", sizeof(T) == 2, KERN_REST(D)};
}

template <typename T, int D, bool REL, int MODE>
void add_bwd_v2(Plan& pl, AttnP& p, const char* what) {
  constexpr int NTH = V2T<T>::DKDV_THREADS;
  const int lq_pad = v2_pad(p.Lq, v2_kc<T>()), lk_pad = v2_pad(p.Lk, v2_kc<T>());
  constexpr int dkdv_max = v2_dkdv_lds<T, D>(V2_LMAX, V2_LMAX / 32);
  // dK/dV stages the head's keep-bitmask rows in LDS when the caller kept them
  p.dm_lds = p.p > 0.f && p.dm && v2_dkdv_lds<T, D>(lq_pad, p.dmw) <= dkdv_max;
  const dim3 heads((unsigned)(p.B * p.H));
  // dQ first: it writes delta = rowsum(dO * O) for dK/dV (no separate delta pass)
  pl.add(KERN_TD(attn_dq_v2_kernel, REL, MODE), heads, V2_THREADS, v2_dq_lds<T, D>(lk_pad), v2_dq_lds<T, D>(V2_LMAX), what);
  pl.add(KERN_TD(attn_dkdv_v2_kernel, NTH, REL, MODE), heads, NTH, v2_dkdv_lds<T, D>(lq_pad, p.dm_lds ? p.dmw : 0),
         dkdv_max, what);
}

// the kernels of one call, in launch order, for the template's (dtype, padded head dim)
template <typename T, int D>
void plan_kernels(Plan& pl, AttnP& p, const mmfd_attn_args& a, bool bwd) {
  const char* what = bwd ? "attn_bwd" : "attn_fwd";
  const int64_t nbh = p.B * p.H;
  const dim3 heads((unsigned)nbh);
  const dim3 qblocks((unsigned)((p.Lq + 63) / 64), (unsigned)nbh), kblocks((unsigned)((p.Lk + 63) / 64), (unsigned)nbh);
  if (pl.family == SPLIT) {
    const int lq16 = v2_pad(p.Lq, 16), lk16 = v2_pad(p.Lk, 16);
    if (!bwd) {
      // dropout as a template argument: a run-time flag let the compiler if-convert the hash into
      // every chunk (its multiplies issued for dropout-free calls too)
      pl.add(p.p > 0.f ? KERN_D(attn_fwd_x6_kernel, true) : KERN_D(attn_fwd_x6_kernel, false), heads, V2_THREADS,
             x6_kv_lds(lk16), X6A_LDS, what);
    } else {
      // dropout in the backward (0 none, 1 hash, 2 keep-bitmask): the forward's keep-bitmask when the
      // caller kept one (dQ reads its row words from memory; dK/dV stages the head's rows in LDS
      // when they fit beside its images, else re-hashes), otherwise the hash again
      const int dqd = p.p <= 0.f ? 0 : !p.dm ? 1 : 2;
      const int dkd = dqd == 2 && x6_dkdv_lds(lq16, lk16, p.dmw) > X6A_LDS_MAX ? 1 : dqd;
      // dQ first: it computes delta = rowsum(dO * O) for dK/dV (no separate delta pass)
      pl.add(dqd == 0 ? KERN_D(attn_dq_x6_kernel, 0) : dqd == 1 ? KERN_D(attn_dq_x6_kernel, 1) : KERN_D(attn_dq_x6_kernel, 2),
             heads, V2_THREADS, x6_kv_lds(lk16), X6A_LDS, what);
      pl.add(dkd == 0 ? KERN_D(attn_dkdv_x6_kernel, 0) : dkd == 1 ? KERN_D(attn_dkdv_x6_kernel, 1) : KERN_D(attn_dkdv_x6_kernel, 2),
             heads, V2_THREADS, x6_dkdv_lds(lq16, lk16, dkd == 2 ? p.dmw : 0), X6A_LDS_MAX, what);
    }
  } else if (pl.family == RESIDENT && !bwd) {
    // short windows: several heads per workgroup so all 8 waves own a 16-query block
    const int hpb = p.Lk <= 64 && p.Lq <= 32 ? 4 : p.Lk <= 64 && p.Lq <= 64 ? 2 : 1;
    const int lmax = hpb > 1 ? 64 : sizeof(T) == 2 ? V2_LMAX_FWD : V2_LMAX;
    pl.add(hpb == 4 ? fwd_v2_kern<T, D, 4>(p) : hpb == 2 ? fwd_v2_kern<T, D, 2>(p) : fwd_v2_kern<T, D, 1>(p),
           dim3((unsigned)((nbh + hpb - 1) / hpb)), V2_THREADS,
           v2_fwd_lds<T, D>(hpb, v2_pad(p.Lk, v2_kc<T>())) + (p.cos_ls ? v2_fwd_cos_lds(hpb, v2_pad(p.Lk, v2_kc<T>())) : 0),
           v2_fwd_lds<T, D>(hpb, lmax) + v2_fwd_cos_lds(hpb, lmax), what);
  } else if (pl.family == RESIDENT) {
    const int mode = v2_mode(p);
    if (p.rel_bias) add_bwd_v2<T, D, true, 0>(pl, p, what);
    else if (mode == 1) add_bwd_v2<T, D, false, 1>(pl, p, what);
    else if (mode == 2) add_bwd_v2<T, D, false, 2>(pl, p, what);
    else add_bwd_v2<T, D, false, 0>(pl, p, what);
  } else if (!bwd) {
    pl.add(KERN_TD(attn_fwd_kernel), qblocks, 256, stream_kv_lds<T, D>(), 0, what);
  } else {
    const int64_t threads = nbh * p.Lq * AT<T, D>::NCH;  // one 16-B chunk of a dO / O row each
    pl.add(KERN_TD(attn_delta_kernel), dim3((unsigned)((threads + 255) / 256)), 256, 0, 0, what);
    pl.add(KERN_TD(attn_bwd_dkdv_kernel), kblocks, 256, stream_dkdv_lds<T, D>(), 0, what);
    pl.add(KERN_TD(attn_bwd_dq_kernel), qblocks, 256, stream_dq_lds<T, D>(), 0, what);
  }
  if (!bwd && p.dm && pl.family == STREAM) {  // the streaming kernels hash without writing the mask: fill it for the backward
    const int64_t words = nbh * p.Lq * p.dmw;
    pl.add(Kern{(const void*)&dm_fill_kernel, "dm_fill_kernel", -1, 0, {}, nullptr},
           dim3((unsigned)std::min<int64_t>((words + 255) / 256, 8192)), 256, 0, 0, "attn_fwd dm_fill");
  }
  if (bwd && a.d_rel_bias)  // after the kernels above: it reads the delta they wrote
    pl.add(ds_kern<T, D, false>(), qblocks, 256, stream_kv_lds<T, D>(), 0, "attn_bwd d_rel_bias");
}

// ---------------------------------------------------------------------------------------------
// mmfd_attn_bwd_ds: dS alone, with or without dropout, after an mmfd_attn_bwd of the same arguments
// ---------------------------------------------------------------------------------------------
// Checks as for d_rel_bias (fill) without what the kernel does not touch (o, dq, dk, dv); the AttnP
// fields attn_bwd_ds_kernel reads, the rest zero.
int make_ds_plan(const mmfd_attn_args* a, const float* ds_out, AttnP& p, Plan& pl) {
  MMFD_CHECK_STRUCT(a, mmfd_attn_args, "mmfd_attn_bwd_ds");
  pl.n = 0;
  pl.split3 = false;
  pl.family = STREAM;
  MMFD_CHECK_ARG(a->dtype == MMFD_F32 || a->dtype == MMFD_BF16, "attn_bwd_ds: bad dtype");
  MMFD_CHECK_ARG(a->D > 0 && a->D <= 64, "attn_bwd_ds: head_dim %lld unsupported (<= 64)", (long long)a->D);
  MMFD_CHECK_ARG(a->B >= 0 && a->H > 0 && a->Lq >= 0 && a->Lk > 0, "attn_bwd_ds: bad shape");
  MMFD_CHECK_ARG(a->q && a->k && a->v && a->dout && a->lse && a->delta && ds_out, "attn_bwd_ds: null pointer");
  const int epc = a->dtype == MMFD_BF16 ? 8 : 4;
  MMFD_CHECK_ARG(a->D % epc == 0, "attn_bwd_ds: head_dim*element_size must be a multiple of 16 bytes");
  auto al = [&](const void* ptr, int64_t sb, int64_t st) {
    return ((uintptr_t)ptr & 15) == 0 && sb % epc == 0 && st % epc == 0;
  };
  MMFD_CHECK_ARG(al(a->q, a->q_sb, a->q_st) && al(a->k, a->k_sb, a->k_st) && al(a->v, a->v_sb, a->v_st) &&
                     al(a->dout, a->do_sb, a->do_st),
                 "attn_bwd_ds: q/k/v/dout must be 16-B aligned with strides multiple of 16 B");
  MMFD_CHECK_ARG(a->rel_bias && a->rel_bias_sb == a->H * a->Lq * a->Lk && a->rel_bias_mod == 0,
                 "attn_bwd_ds: needs a per-batch rel_bias [B][H][Lq][Lk] (rel_bias_sb = H*Lq*Lk, rel_bias_mod = 0)");
  MMFD_CHECK_ARG(a->dropout_p <= 0.f || a->seed, "attn_bwd_ds: dropout needs seed");
  MMFD_CHECK_ARG(a->dropout_p < 1.f, "attn_bwd_ds: dropout p must be < 1");
  MMFD_CHECK_ARG(ds_out != a->rel_bias, "attn_bwd_ds: the output must not alias rel_bias");
  MMFD_CHECK_ARG(((uintptr_t)ds_out & 15) == 0, "attn_bwd_ds: the output must be 16-B aligned");
  MMFD_CHECK_ARG(a->B * a->H <= 65535, "attn_bwd_ds: needs B*H <= 65535");
  MMFD_CHECK_ARG(a->cos_logit_scale == nullptr, "attn_bwd_ds: cosine attention is inference-only");
  MMFD_CHECK_ARG(!a->drop_mask || ((uintptr_t)a->drop_mask & 3) == 0, "attn_bwd_ds: drop_mask must be 4-B aligned");
  p = AttnP{};
  p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.Lk = a->Lk; p.scale = a->scale; p.D = (int)a->D;
  p.q = a->q; p.q_sb = a->q_sb; p.q_st = a->q_st;
  p.k = a->k; p.k_sb = a->k_sb; p.k_st = a->k_st;
  p.v = a->v; p.v_sb = a->v_sb; p.v_st = a->v_st;
  p.dout = a->dout; p.do_sb = a->do_sb; p.do_st = a->do_st;
  p.lse = a->lse; p.delta = a->delta; p.key_bias = a->key_bias;
  p.rel_bias = a->rel_bias; p.rb_sb = a->rel_bias_sb;
  p.p = a->dropout_p > 0.f ? a->dropout_p : 0.f; p.thr16 = mmfd_drop_threshold16(p.p); p.kp = (a->Lk + 1) / 2;
  p.keep_scale = 1.0f / (1.0f - p.p); p.seed = a->seed; p.salt = a->salt;
  p.idx32 = (uint64_t)a->B * (uint64_t)a->H * (uint64_t)a->Lq * (uint64_t)a->Lk <= (1ull << 32);
  p.dmw = (int)((a->Lk + 31) / 32);  // (drop_mask is not read: the kernel re-hashes the same bits)
  if (p.B == 0 || p.Lq == 0) return 0;
  const dim3 qblocks((unsigned)((p.Lq + 63) / 64), (unsigned)(p.B * p.H));
  const bool bf = a->dtype == MMFD_BF16, drop = p.p > 0.f, wide = a->D > 32;
  const char* what = "attn_bwd_ds";
#define DS_ADD(T, D) pl.add(drop ? ds_kern<T, D, true>() : ds_kern<T, D, false>(), qblocks, 256, stream_kv_lds<T, D>(), 0, what)
  if (bf) { if (wide) DS_ADD(bf16, 64); else DS_ADD(bf16, 32); }
  else { if (wide) DS_ADD(float, 64); else DS_ADD(float, 32); }
#undef DS_ADD
  return 0;
}

// check the arguments, fill AttnP (with the host-set flags that steer the kernels: pl / pl_only, vst,
// dm, dm_lds, idx32) and list the launches. An empty call (B = 0 or Lq = 0) gives an empty plan.
int make_plan(const mmfd_attn_args* a, bool bwd, AttnP& p, Plan& pl) {
  MMFD_CHECK_STRUCT(a, mmfd_attn_args, bwd ? "mmfd_attn_bwd" : "mmfd_attn_fwd");
  pl.n = 0;
  pl.split3 = false;
  int rc = fill(*a, p, bwd);
  if (rc) return rc;
  if (p.B == 0 || p.Lq == 0) return 0;
  const bool bf = a->dtype == MMFD_BF16;
  pl.family = family_of(*a, bwd);
  const void* planes = bwd ? a->dqkv_planes : a->o_planes;
  if (!bwd) {
    MMFD_CHECK_ARG(!a->cos_logit_scale || (pl.family == RESIDENT && bf && a->rel_bias),
                   "attn_fwd: cosine attention needs bf16, the resident-K/V kernel (Lk <= 256) and a rel_bias");
    const int64_t W = a->H * a->D;
    MMFD_CHECK_ARG(!planes || (!bf && a->o_st == W && a->o_sb == a->Lq * W && W % 8 == 0),
                   "attn_fwd: o_planes need an fp32 output in one contiguous [B, Lq, H*D] buffer");
  } else if (planes) {
    const int64_t W = 3 * a->H * a->D;
    MMFD_CHECK_ARG(a->dtype == MMFD_F32 && a->Lq == a->Lk && a->dk == (const float*)a->dq + a->H * a->D &&
                       a->dv == (const float*)a->dq + 2 * a->H * a->D && a->dq_st == W && a->dk_st == W &&
                       a->dv_st == W && a->dq_sb == a->Lq * W && a->dk_sb == a->dq_sb && a->dv_sb == a->dq_sb,
                   "attn_bwd: dqkv_planes need fp32 dq | dk | dv packed in one contiguous [B, L, 3*H*D] buffer");
    MMFD_CHECK_ARG(!a->planes_only || (!a->accumulate_dq && !a->accumulate_dkv),
                   "attn_bwd: planes_only excludes accumulate");
  }
  if (planes && pl.family != STREAM) {  // the resident and split kernels write the planes from their stores
    p.pl = (bf16*)planes;
    p.pl_stride = p.B * p.Lq * (bwd ? 3 : 1) * a->H * a->D;
    p.pl_base = (const float*)(bwd ? a->dq : a->o);
    if (bwd) {
      if ((uintptr_t)p.pl & 7) p.vst = 0;
      p.pl_only = a->planes_only;
    }
  }
  pl.split3 = planes && pl.family == STREAM;
  // the one (dtype, head dim) ladder: head dims up to 32 run the D = 32 instantiations, zero-padded
  if (bf) { if (a->D > 32) plan_kernels<bf16, 64>(pl, p, *a, bwd); else plan_kernels<bf16, 32>(pl, p, *a, bwd); }
  else { if (a->D > 32) plan_kernels<float, 64>(pl, p, *a, bwd); else plan_kernels<float, 32>(pl, p, *a, bwd); }
  return 0;
}

int run_plan(const Plan& pl, const AttnP& p, const mmfd_attn_args& a, bool bwd, mmfd_stream_t stream, float* ds) {
  void* args[] = {(void*)&p, (void*)&ds};  // every kernel takes the AttnP; attn_bwd_ds_kernel its output too
  for (int i = 0; i < pl.n; ++i) {
    const Step& st = pl.step[i];
    if (st.lds_max && !*st.k.attr_set) {
      (void)hipFuncSetAttribute(st.k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, st.lds_max);
      *st.k.attr_set = true;
    }
    (void)hipLaunchKernel(st.k.fn, st.grid, dim3(st.block), args, (size_t)st.lds, (hipStream_t)stream);
    if (i + 1 == pl.n || pl.step[i + 1].what != st.what) MMFD_CHECK_LAUNCH(st.what);
  }
  if (!pl.split3) return 0;
  const int64_t W = (bwd ? 3 : 1) * a.H * a.D;
  return mmfd_split3(p.B * p.Lq, W, (const float*)(bwd ? a.dq : a.o), W, bwd ? a.dqkv_planes : a.o_planes, stream);
}

int attn_call(const mmfd_attn_args* a, bool bwd, mmfd_stream_t stream) {
  AttnP p;
  Plan pl;
  int rc = make_plan(a, bwd, p, pl);
  return rc ? rc : run_plan(pl, p, *a, bwd, stream, (float*)a->d_rel_bias);
}

}  // namespace

extern "C" int mmfd_attn_fwd(const mmfd_attn_args* a, mmfd_stream_t stream) { return attn_call(a, false, stream); }
extern "C" int mmfd_attn_bwd(const mmfd_attn_args* a, mmfd_stream_t stream) { return attn_call(a, true, stream); }
extern "C" int mmfd_attn_bwd_ds(const mmfd_attn_args* a, float* ds_out, mmfd_stream_t stream) {
  AttnP p;
  Plan pl;
  int rc = make_ds_plan(a, ds_out, p, pl);
  return rc ? rc : run_plan(pl, p, *a, true, stream, ds_out);
}

// The plan of a call as text, without launching anything or touching HIP (not part of
// include/mmfd.h; the pointers in `a` are never dereferenced). One line "family=<name>", then one
// line per launch in order: the kernel instantiation (bool template arguments as 0 / 1), grid, block,
// dynamic LDS bytes and the names of the host-set AttnP flags that are on (pl, pl_only, vst, dm,
// dm_lds, idx32; pl_stride with pl); "mmfd_split3 rows= W=" when the split follows.
// An empty call writes an empty string. Returns the argument checks' code.
// bwd = 2: the plan of mmfd_attn_bwd_ds for these arguments, with a->d_rel_bias standing for ds_out.
extern "C" int mmfd_debug_attn_plan(const mmfd_attn_args* a, int bwd, char* buf, int64_t bytes) {
  MMFD_CHECK_ARG(buf && bytes > 0, "mmfd_debug_attn_plan: no buffer");
  AttnP p;
  Plan pl;
  buf[0] = 0;
  int rc = bwd == 2 ? make_ds_plan(a, a ? a->d_rel_bias : nullptr, p, pl) : make_plan(a, bwd != 0, p, pl);
  if (rc || pl.n == 0) return rc;
  int64_t at = 0;
  auto put = [&](const char* fmt, auto... v) {
    if (at < bytes) at += snprintf(buf + at, (size_t)(bytes - at), fmt, v...);
  };
  put("family=%s\n", FAMILY_NAME[pl.family]);
  for (int i = 0; i < pl.n; ++i) {
    const Step& st = pl.step[i];
    put("%s", st.k.name);
    for (int j = 0; j < st.k.narg; ++j) {
      if (j == 0) put("%s", st.k.bf < 0 ? "<" : st.k.bf ? "<bf16," : "<float,");
      put(j + 1 < st.k.narg ? "%d," : "%d>", st.k.arg[j]);
    }
    put(" grid=%u,%u,%u block=%u lds=%d%s%s%s%s%s%s", st.grid.x, st.grid.y, st.grid.z, st.block, st.lds,
        p.pl ? " pl" : "", p.pl_only ? " pl_only" : "", p.vst ? " vst" : "", p.dm ? " dm" : "",
        p.dm_lds ? " dm_lds" : "", p.idx32 ? " idx32" : "");
    if (p.pl) put(" pl_stride=%lld", (long long)p.pl_stride);
    put("%s", "\n");
  }
  if (pl.split3) put("mmfd_split3 rows=%lld W=%lld\n", (long long)(p.B * p.Lq), (long long)((bwd ? 3 : 1) * a->H * a->D));
  MMFD_CHECK_ARG(at < bytes, "mmfd_debug_attn_plan: buffer of %lld bytes is too small", (long long)bytes);
  return 0;
}

// A/B switch for the fixed v2 modes (not part of include/mmfd.h): returns the old value
extern "C" int mmfd_debug_set_attn_v2_generic(int on) {
  const int old = g_v2_generic;
  g_v2_generic = on ? 1 : 0;
  return old;
}

extern "C" int mmfd_set_fp32_attn_mode(int mode) {
  MMFD_CHECK_ARG(mode == 0 || mode == 1, "mmfd_set_fp32_attn_mode: mode %d (0 = fp32 MFMA, 1 = split operands)", mode);
  const int old = g_fp32_attn_mode;
  g_fp32_attn_mode = mode;
  return old;
}

#ifdef MMFD_X6A_STAMPS
extern "C" int mmfd_debug_x6a_stamps(void* host_dst, int64_t bytes) {
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(x6a_stamps), (size_t)bytes, 0, hipMemcpyDeviceToHost);
}
#endif
