// The LDS-resident ("v2") attention kernels: forward, dK/dV and dQ with the head's K/V (or Q/dO)
// staged in LDS once; also the staging, cosine-attention and lane-group helpers the split-operand
// kernels of attn_split.h reuse (v2_pad, rows4_max, stage_kbias, LOG2E).
#pragma once
#include "attn_common.h"

namespace {

// =================================================================================================
// v2 kernels (Lq and Lk <= 256; bf16 forward up to 512 keys): one workgroup of 8 waves per (b, h).
// The whole K/V (forward, dQ) or Q/dO (dK/dV) of the head is staged in LDS ONCE and every wave
// sweeps 16-row blocks against it: no per-block restaging and no repeated K/V reads from L2. Rows
// are padded only to one MFMA k-chunk (bf16: 32, fp32: 16), so L = 197 computes on 224 / 208 rows
// instead of the streaming kernels' 256.
// =================================================================================================
constexpr int V2_LMAX = 256;      // backward kernels (Q/dO or K/V images of the head); fp32 forward
constexpr int V2_LMAX_FWD = 512;  // bf16 forward: K/V images of 512 keys (128 KB at D = 64) fit the 160-KB LDS
constexpr int V2_THREADS = 512;   // forward / dQ: 8 waves sharing one K/V image
// dK/dV: bf16 images are small enough for two workgroups per CU; an fp32 head image (up to 128 KB)
// allows one, so it gets 8 waves
template <typename T> struct V2T { static constexpr int DKDV_THREADS = sizeof(T) == 4 ? 512 : 256; };
// row image == transposed image (no second copy): bf16 at D = 64 and every fp32 layout
template <typename T, int D> struct V2 { static constexpr bool DUAL = sizeof(T) == 4 || D == 64; };
// rows per MFMA k-chunk, and 16-row subtiles per chunk
template <typename T> __host__ __device__ constexpr int v2_kc() { return sizeof(T) == 2 ? 32 : 16; }
__host__ __device__ inline int v2_pad(int64_t n, int kc) { return (int)((n + kc - 1) / kc * kc); }

// Head staging: STAGE_BATCH 16-B chunks per thread and source are loaded before the first LDS
// write, so a workgroup waits out one global-load latency per batch instead of one per chunk (the
// one-chunk loop waited vmcnt(0) before every ds_write: 14 serial round trips for a ViT dK/dV head)
constexpr int STAGE_BATCH = 4;

template <typename T, int D, bool TR>
__device__ __forceinline__ int stage_off(int r, int ch) {
  return TR ? (r * AT<T, D>::RB + (tr_chunk<T, D>(r, ch) << 4)) : row_off<T, D>(r, ch);
}

template <typename T, int D, bool TR, int NTH = V2_THREADS>
__device__ __forceinline__ void stage_all(char* lds, const T* __restrict__ base, int64_t st, int64_t nrows,
                                          int nrows_pad, int tid, int dreal) {
  constexpr int NCH = AT<T, D>::NCH, EPC = AT<T, D>::EPC;
  const int total = nrows_pad * NCH;
  for (int c0 = tid; c0 < total; c0 += NTH * STAGE_BATCH) {
    uint4 v[STAGE_BATCH];
#pragma unroll
    for (int j = 0; j < STAGE_BATCH; ++j) {
      const int c = c0 + j * NTH, r = c / NCH, ch = c % NCH;
      v[j] = make_uint4(0, 0, 0, 0);
      if (c < total && r < nrows && ch * EPC < dreal) v[j] = *reinterpret_cast<const uint4*>(base + (int64_t)r * st + ch * EPC);
    }
#pragma unroll
    for (int j = 0; j < STAGE_BATCH; ++j) {
      const int c = c0 + j * NTH;
      if (c < total) *reinterpret_cast<uint4*>(lds + stage_off<T, D, TR>(c / NCH, c % NCH)) = v[j];
    }
  }
}

// two head slices of the same row count (K and V, Q and dO, or one tensor into both layouts),
// every load of a batch of both issued before its writes
template <typename T, int D, bool TRA, bool TRB, int NTH = V2_THREADS>
__device__ __forceinline__ void stage_two(char* lds_a, const T* __restrict__ base_a, int64_t st_a, char* lds_b,
                                          const T* __restrict__ base_b, int64_t st_b, int64_t nrows, int nrows_pad,
                                          int tid, int dreal) {
  constexpr int NCH = AT<T, D>::NCH, EPC = AT<T, D>::EPC;
  const int total = nrows_pad * NCH;
  for (int c0 = tid; c0 < total; c0 += NTH * STAGE_BATCH) {
    uint4 va[STAGE_BATCH], vb[STAGE_BATCH];
#pragma unroll
    for (int j = 0; j < STAGE_BATCH; ++j) {
      const int c = c0 + j * NTH, r = c / NCH, ch = c % NCH;
      va[j] = vb[j] = make_uint4(0, 0, 0, 0);
      if (c < total && r < nrows && ch * EPC < dreal) {
        va[j] = *reinterpret_cast<const uint4*>(base_a + (int64_t)r * st_a + ch * EPC);
        vb[j] = *reinterpret_cast<const uint4*>(base_b + (int64_t)r * st_b + ch * EPC);
      }
    }
#pragma unroll
    for (int j = 0; j < STAGE_BATCH; ++j) {
      const int c = c0 + j * NTH, r = c / NCH, ch = c % NCH;
      if (c < total) {
        *reinterpret_cast<uint4*>(lds_a + stage_off<T, D, TRA>(r, ch)) = va[j];
        *reinterpret_cast<uint4*>(lds_b + stage_off<T, D, TRB>(r, ch)) = vb[j];
      }
    }
  }
}

// K rows staged as they are, and 1 / max(|k|, 1e-12) of each row into kinv (Swinv2 cosine attention:
// the norms scale the fp32 scores, so the MFMA operands stay the exact inputs — normalised rows rounded
// to bf16 cost up to 2^-8 of the logit scale per logit, 0.4 at the clamp of 100): the NCH chunks of a
// row belong to NCH consecutive lanes, so the row's sum of squares is a butterfly over those lanes
template <int D, int NTH>
__device__ __forceinline__ void stage_rows_cos(char* lds, float* kinv, const bf16* __restrict__ base, int64_t st,
                                               int64_t nrows, int nrows_pad, int tid, int dreal) {
  constexpr int NCH = AT<bf16, D>::NCH, EPC = AT<bf16, D>::EPC;
  for (int c = tid; c < nrows_pad * NCH; c += NTH) {
    const int r = c / NCH, ch = c % NCH;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < nrows && ch * EPC < dreal) v = *reinterpret_cast<const uint4*>(base + (int64_t)r * st + ch * EPC);
    const bf16x8 x = __builtin_bit_cast(bf16x8, v);
    float f[EPC], ss = 0.f;
#pragma unroll
    for (int e = 0; e < EPC; ++e) { f[e] = (float)x[e]; ss = fmaf(f[e], f[e], ss); }
#pragma unroll
    for (int o = 1; o < NCH; o <<= 1) ss += __shfl_xor(ss, o, 64);
    if (ch == 0) kinv[r] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    *reinterpret_cast<uint4*>(lds + row_off<bf16, D>(r, ch)) = v;
  }
}

// mult / max(|q|, 1e-12) of the lane's query row from its q fragments (load_row_regs layout: a row's
// chunks sit in lanes li, li+16, li+32, li+48; lane (g, li) owns the scores of query li)
template <int D>
__device__ __forceinline__ float cos_q_scale(const uint4* f, float mult) {
  constexpr int KCH = AT<bf16, D>::KCH;
  float ss = 0.f;
#pragma unroll
  for (int kc = 0; kc < KCH; ++kc) {
    const bf16x8 x = __builtin_bit_cast(bf16x8, f[kc]);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float v = (float)x[e]; ss = fmaf(v, v, ss); }
  }
  ss += __shfl_xor(ss, 16, 64);
  ss += __shfl_xor(ss, 32, 64);
  return mult / fmaxf(sqrtf(ss), 1e-12f);
}

constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

// max / sum over the four lanes li, li+16, li+32, li+48 (the lane groups of one S^T column) by two
// VALU half-swaps (v_permlane16/32_swap) instead of LDS permutes: the same pairs as __shfl_xor 16
// then 32, so a sum rounds identically
__device__ __forceinline__ float rows4_max(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float rows4_sum(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// v2 kernel modes, chosen on the host: 0 = any (dropout, key bias, keep-bitmask, tested at run
// time), 1 = plain (no dropout, no key bias: ViT, the fusion head at eval), 2 = hashed dropout with
// a key bias and no bitmask (BERT training). The fixed modes take the per-subtile branches out of
// the softmax loops, and mode 1 folds the scale into the exponent (exp2(s * c2 - m) as one fma).
// bf16 forward only: the running max is raised only when some lane's chunk max passes it by more
// than 8 (log2 units), so P = exp2(t - m) stays <= 256 and the O / l rescale (and its lane
// broadcasts) is skipped for most chunks; O and l are scaled by the same stale max, so O / l is
// unchanged up to rounding
constexpr float V2_RESCALE_TH = 8.f;

// per-key additive bias in log2 units for the head's batch row: log2e * key_bias (clamped so a
// fully masked row stays finite, as HF's finfo.min mask does) for k < Lk, -inf for padded keys
template <int NTH>
__device__ __forceinline__ void stage_kbias(float* dst, const AttnP& p, int64_t b, int npad, int tid) {
  for (int i = tid; i < npad; i += NTH)
    dst[i] = i < p.Lk ? (p.key_bias ? fmaxf(p.key_bias[b * p.Lk + i] * LOG2E, -1e30f) : 0.f) : -INFINITY;
}

// Dynamic LDS of the three kernels, as each carves its smem (rows padded to the MFMA k-chunk):
//   forward: per head of the workgroup, the K and V images and the per-key bias floats; cosine attention
//            adds, behind all of them, the per-key inverse norms (v2_fwd_cos_lds)
//   dQ     : K and V row images, K transposed unless DUAL, the per-key bias floats
//   dK/dV  : Q and dO as row and (unless DUAL) transposed images; lse, delta and key bias at V2_LMAX
//            floats each; dm_words keep-bitmask words per query row when AttnP::dm_lds
template <typename T, int D> constexpr int v2_fwd_lds(int hpb, int lk_pad) {
  return hpb * (2 * lk_pad * AT<T, D>::RB + lk_pad * 4);
}
constexpr int v2_fwd_cos_lds(int hpb, int lk_pad) { return hpb * lk_pad * 4; }
template <typename T, int D> constexpr int v2_dq_lds(int lk_pad) {
  return (V2<T, D>::DUAL ? 2 : 3) * lk_pad * AT<T, D>::RB + lk_pad * 4;
}
template <typename T, int D> constexpr int v2_dkdv_lds(int lq_pad, int dm_words) {
  return (V2<T, D>::DUAL ? 2 : 4) * lq_pad * AT<T, D>::RB + 3 * V2_LMAX * 4 + lq_pad * dm_words * 4;
}
static_assert(v2_dkdv_lds<float, 64>(V2_LMAX, V2_LMAX / 32) <= 160 * 1024 &&
              v2_dkdv_lds<bf16, 32>(V2_LMAX, V2_LMAX / 32) <= 160 * 1024, "dK/dV LDS");

// bf16 without the relative bias: at most 128 VGPRs (4 waves per SIMD) so that two 8-wave
// workgroups share a CU — the bf16 K/V images allow it, and one VGPR over halves the occupancy
// (ViT fwd +45 %); the REL instantiation needs ~148 and would spill under that bound
template <typename T, int D, int HPB, bool REL, int MODE>
__global__ void __launch_bounds__(V2_THREADS, sizeof(T) == 2 && !REL ? 4 : 1) attn_fwd_v2_kernel(AttnP p) {
  static_assert(MODE == 0 || (HPB == 1 && !REL), "fixed modes: one head per workgroup, no relative bias");
  constexpr bool LAZY = sizeof(T) == 2;
  // K/V of the head resident in LDS; each wave sweeps 16-query blocks with an online softmax (exp2
  // domain) over 64-key chunks (the last one holds only the padded key count's subtiles); key
  // mask/padding come from a per-key bias vector in LDS.
  // HPB > 1 (short windows: Lq <= 64 / 32, Lk <= 64, e.g. Swinv2's 8x8 windows): the 8 waves split
  // into HPB groups, each owning one (b, h) with its own LDS images, so no wave idles on a head
  // that has fewer 16-query blocks than the workgroup has waves.
  using C = AT<T, D>;
  constexpr int KC = v2_kc<T>(), SUBS = KC / 16;
  constexpr int WPH = (V2_THREADS / 64) / HPB;  // waves per head
  constexpr int TPH = V2_THREADS / HPB;         // threads per head
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = wave_all / WPH, wave = wave_all % WPH, htid = tid % TPH;
  const int64_t nbh = p.B * p.H, bh_raw = (int64_t)blockIdx.x * HPB + sub;
  const bool active = bh_raw < nbh;
  const int64_t bh = active ? bh_raw : nbh - 1, b = bh / p.H, h = bh % p.H;
  const int lk_pad = v2_pad(p.Lk, KC);
  char* hbase = smem + sub * (2 * lk_pad * C::RB + lk_pad * 4);
  char* k_img = hbase;
  char* v_img = hbase + lk_pad * C::RB;
  float* kbias = reinterpret_cast<float*>(hbase + 2 * lk_pad * C::RB);
  // cosine only (the launch adds v2_fwd_cos_lds): 1 / |k| per key, behind every head's images
  float* kinv = reinterpret_cast<float*>(smem + v2_fwd_lds<T, D>(HPB, lk_pad)) + sub * lk_pad;
  const T* qb = reinterpret_cast<const T*>(p.q) + b * p.q_sb + h * p.D;
  const T* kb_g = reinterpret_cast<const T*>(p.k) + b * p.k_sb + h * p.D;
  const int nqb = (int)((p.Lq + 15) / 16);
  uint4 qn[C::KCH];  // next query block's fragments, prefetched one block ahead (the first under the staging)
  load_row_regs<T, D>(qn, qb, p.q_st, (int64_t)wave * 16 + li, p.Lq, lane, p.D);
  bool cosine = false;
  if constexpr (sizeof(T) == 2) {
    cosine = REL && p.cos_ls != nullptr;
    if (cosine) stage_rows_cos<D, TPH>(k_img, kinv, kb_g, p.k_st, p.Lk, lk_pad, htid, p.D);
  }
  const T* vb_g = reinterpret_cast<const T*>(p.v) + b * p.v_sb + h * p.D;
  if (!cosine)
    stage_two<T, D, false, true, TPH>(k_img, kb_g, p.k_st, v_img, vb_g, p.v_st, p.Lk, lk_pad, htid, p.D);
  else
    stage_all<T, D, true, TPH>(v_img, vb_g, p.v_st, p.Lk, lk_pad, htid, p.D);
  stage_kbias<TPH>(kbias, p, b, lk_pad, htid);
  __syncthreads();
  if (!active) return;
  const uint64_t seed = p.p > 0.f ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);
  const bool drop = MODE == 0 ? p.p > 0.f : MODE == 2;
  const float c2 = p.scale * LOG2E;
  const float qmult = cosine ? expf(fminf(p.cos_ls[h], p.cos_max_log)) : 1.f;
  const bool rel4 = p.rel_bias && (p.Lk & 3) == 0 && (reinterpret_cast<uintptr_t>(p.rel_bias) & 15) == 0 &&
                    (p.rb_sb & 3) == 0;
  T* ob = reinterpret_cast<T*>(p.o) + b * p.o_sb + h * p.D;
  for (int qbk = wave; qbk < nqb; qbk += WPH) {
    const int64_t q0 = (int64_t)qbk * 16, myq = q0 + li;
    uint4 qf[C::KCH];
#pragma unroll
    for (int kc = 0; kc < C::KCH; ++kc) qf[kc] = qn[kc];
    load_row_regs<T, D>(qn, qb, p.q_st, q0 + WPH * 16 + li, p.Lq, lane, p.D);
    float qscale = 1.f;  // cosine: exp(logit scale) / |q| of this lane's query
    if constexpr (sizeof(T) == 2) {
      if (cosine) qscale = cos_q_scale<D>(qf, qmult);
    }
    const uint64_t hrow = (uint64_t)(bh * p.Lq + myq) * (uint64_t)p.kp;  // pair-index base of this query row
    const uint32_t rowc1 = ((uint32_t)hrow + (uint32_t)(2 * g)) * HASH_C1;
    const float* relrow = REL ? p.rel_bias + rb_off(p, b) + (h * p.Lq + (myq < p.Lq ? myq : 0)) * p.Lk : nullptr;
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[C::DT];
#pragma unroll
    for (int d = 0; d < C::DT; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    // one 64-key chunk with NS 16-key subtiles present (NS < 4 only for the last, padded chunk;
    // NS = 0: that count at run time, `ns_rt`); a compile-time NS keeps every per-subtile branch
    // out of the full chunks. FOLD (mode 1, a full chunk of real keys): the chunk max is taken on
    // the raw scores and the scale goes into the exponent's fma
    auto chunk = [&](int k0, auto nsc, int ns_rt, auto foldc) {
      constexpr int NS = decltype(nsc)::value;
      constexpr bool FOLD = decltype(foldc)::value;
      const int nsub = NS ? NS : ns_rt;
      const char* kc_img = k_img + k0 * C::RB;
      const char* vc_img = v_img + k0 * C::RB;
      f32x4 s[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s[ks] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (sizeof(T) == 4 && nsub == 4) {  // fp32: four interleaved S^T chains, K read one k-chunk ahead
        uint4 fa[4], fb[4], fn[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) { fa[ks] = row_frag<T, D>(kc_img, ks, 0, lane); fb[ks] = qf[0]; }
#pragma unroll
        for (int kc = 0; kc < C::KCH; ++kc) {
          if (kc + 1 < C::KCH) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) fn[ks] = row_frag<T, D>(kc_img, ks, kc + 1, lane);
          }
          Mma<T>::template runN<4>(s, fa, fb);
          if (kc + 1 < C::KCH) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) { fa[ks] = fn[ks]; fb[ks] = qf[kc + 1]; }
          }
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < (NS ? NS : 4); ++ks) {
          if (ks < nsub) {
#pragma unroll
            for (int kc = 0; kc < C::KCH; ++kc) Mma<T>::run(s[ks], row_frag<T, D>(kc_img, ks, kc, lane), qf[kc]);
          }
        }
      }
      float mx = -INFINITY;
      if constexpr (FOLD) {  // c2 > 0: max(s) * c2 == max(s * c2) (rounding is monotone)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[ks][r]);
        mx *= c2;
      } else {
#pragma unroll
      for (int ks = 0; ks < (NS ? NS : 4); ++ks) {
        if (ks >= nsub) continue;
        const float4 kb4 = *reinterpret_cast<const float4*>(kbias + k0 + ks * 16 + 4 * g);
        const float kb[4] = {kb4.x, kb4.y, kb4.z, kb4.w};
        float rb[4] = {0.f, 0.f, 0.f, 0.f};
        const int kk = k0 + ks * 16 + 4 * g;
        if constexpr (REL && sizeof(T) == 2) {
          if (cosine) {  // the scores of raw q . k become cosines times the logit scale
            const float4 ki = *reinterpret_cast<const float4*>(kinv + kk);
            s[ks][0] *= qscale * ki.x; s[ks][1] *= qscale * ki.y; s[ks][2] *= qscale * ki.z; s[ks][3] *= qscale * ki.w;
          }
        }
        if (REL) {  // the 4 keys of a lane are contiguous: one 16-B load per subtile when aligned
          if (rel4) {
            if (kk < p.Lk) {
              const float4 v = *reinterpret_cast<const float4*>(relrow + kk);
              rb[0] = v.x; rb[1] = v.y; rb[2] = v.z; rb[3] = v.w;
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) rb[r] = kk + r < p.Lk ? relrow[kk + r] : 0.f;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t = fmaf(s[ks][r], c2, kb[r]);
          if (REL && kk + r < p.Lk) t = fmaf(rb[r], LOG2E, t);
          s[ks][r] = t;
          mx = fmaxf(mx, t);
        }
      }
      }
      mx = rows4_max(mx);
      // (LAZY: a wave-uniform decision; otherwise every chunk rescales)
      const bool grow = !LAZY || __ballot(mx > m + V2_RESCALE_TH) != 0ull;
      float mnew = m, alpha = 1.f;
      if (grow) {
        mnew = fmaxf(m, mx);
        alpha = __builtin_amdgcn_exp2f(m - mnew);
      }
      float rs = 0.f;
#pragma unroll
      for (int ks = 0; ks < (NS ? NS : 4); ++ks) {
        if (ks >= nsub) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = FOLD ? __builtin_amdgcn_exp2f(fmaf(s[ks][r], c2, -mnew))
                               : __builtin_amdgcn_exp2f(s[ks][r] - mnew);
          rs += e;
          s[ks][r] = e;
        }
        if (drop) {  // one uniform branch per subtile (none in the fixed modes)
          float z[4];
          if (p.idx32) {
            const uint32_t c = rowc1 + (uint32_t)((k0 + ks * 16) >> 1) * HASH_C1;
            keep4_pairs(hash_c1(hkey, c), hash_c1(hkey, c + HASH_C1), p, z);
          } else {
            const uint64_t pi = hrow + (uint64_t)((k0 + ks * 16 + 4 * g) >> 1);
            keep4_pairs(mmfd_hash_k(hkey, pi), mmfd_hash_k(hkey, pi + 1), p, z);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) s[ks][r] *= z[r];
        }
      }
      if (MODE == 0 && p.p > 0.f && p.dm) {
        // the keep-bitmask for the backward, read back from P: a dropped element is 0, a kept one
        // e * keep_scale > 0 unless exp2 underflowed — and then the backward's P of it is 0 too,
        // so recording it as dropped changes no gradient (one register, no hash state kept live)
        uint32_t kbits = 0;
#pragma unroll
        for (int ks = 0; ks < (NS ? NS : 4); ++ks) {
          if (ks >= nsub) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) kbits |= (uint32_t)(s[ks][r] != 0.f) << (ks * 4 + r);
        }
        dm_write64(p, bh, myq, k0, g, kbits);
      }
      lsum = lsum * alpha + rs;  // per-lane partial over this lane's keys; reduced at the end
      m = mnew;
      if (grow) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
          for (int d = 0; d < C::DT; ++d) o[d][r] *= ar;
        }
      }
#pragma unroll
      for (int c = 0; c < (NS ? NS : 4) / SUBS; ++c) {
        if (c * SUBS >= nsub) continue;
        uint4 fa[C::DT], fb[C::DT];
        const uint4 a = pack_acc<T>(s, c);
#pragma unroll
        for (int d = 0; d < C::DT; ++d) { fa[d] = a; fb[d] = tr_frag<T, D>(vc_img, c, d, lane); }
        Mma<T>::template runN<C::DT>(o, fa, fb);
      }
    };
    if constexpr (SUBS == 1) {
      // fp32 (MFMA-bound): one instance with the subtile count at run time — two compile-time
      // instances (full chunk + tail) raised it from 154 to 255 VGPRs and cost 7 % at L = 128
      for (int k0 = 0; k0 < lk_pad; k0 += 64)
        chunk(k0, std::integral_constant<int, 0>{}, min(4, (lk_pad - k0) >> 4), std::false_type{});
    } else {
      // bf16 (VALU-bound): the full chunks free of per-subtile branches (128 VGPRs: two workgroups
      // per CU), the 32-key padded tail as its own instance; mode 1 folds the full chunks of real keys
      int k0 = 0;
      if constexpr (MODE == 1) {
        for (; k0 + 64 <= p.Lk; k0 += 64) chunk(k0, std::integral_constant<int, 4>{}, 4, std::true_type{});
      }
      for (; k0 + 64 <= lk_pad; k0 += 64) chunk(k0, std::integral_constant<int, 4>{}, 4, std::false_type{});
      if (k0 < lk_pad) chunk(k0, std::integral_constant<int, 2>{}, 2, std::false_type{});
    }
    lsum = rows4_sum(lsum);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float lr = __shfl(lsum, 4 * g + r, 64);
      const int64_t q = q0 + 4 * g + r;
      const float inv = 1.0f / lr;
      if (q < p.Lq) {
#pragma unroll
        for (int d = 0; d < C::DT; ++d)
          if (d * 16 + li < p.D) {
            const float val = o[d][r] * inv;
            ob[q * p.o_st + d * 16 + li] = from_f32<T>(val);
            if constexpr (std::is_same<T, float>::value) {
              if (p.pl) plane_put(p, reinterpret_cast<const float*>(ob) + q * p.o_st + d * 16 + li, val);
            }
          }
      }
    }
    if (g == 0 && myq < p.Lq) p.lse[bh * p.Lq + myq] = (m + log2f(lsum)) * LN2;
  }
}

template <typename T, int D, int NTH, bool REL, int MODE>
__global__ void __launch_bounds__(NTH) attn_dkdv_v2_kernel(AttnP p) {
  static_assert(MODE == 0 || !REL, "fixed modes: no relative bias");
  // Q/dO of the head resident in LDS (plus lse, delta in log2 units); each wave owns 16 keys.
  // REL: the additive [H][Lq][Lk] bias (MPNet / DeBERTa) — its loads and batch-modulus address
  // math stay out of the bias-free instantiation (BERT, ViT, fusion head)
  using C = AT<T, D>;
  constexpr int KC = v2_kc<T>(), SUBS = KC / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
  const int lq_pad = v2_pad(p.Lq, KC);
  const int img = lq_pad * C::RB;
  constexpr bool DUAL = V2<T, D>::DUAL;
  char* q_row = smem;
  char* do_row = smem + img;
  char* q_tr = DUAL ? q_row : smem + 2 * img;
  char* do_tr = DUAL ? do_row : smem + 3 * img;
  float* s_lse = reinterpret_cast<float*>(smem + (DUAL ? 2 : 4) * img);
  float* s_delta = s_lse + V2_LMAX;
  float* kbias = s_delta + V2_LMAX;
  uint32_t* s_dm = reinterpret_cast<uint32_t*>(kbias + V2_LMAX);  // dm_lds: the head's keep-bitmask rows
  if (MODE == 0 && p.dm_lds) {
    const uint32_t* src = dm_row(p, bh, 0);
    const int nw = (int)p.Lq * p.dmw;
    for (int i = tid; i < lq_pad * p.dmw; i += NTH) s_dm[i] = i < nw ? src[i] : 0u;
  }
  const T* qb = reinterpret_cast<const T*>(p.q) + b * p.q_sb + h * p.D;
  const T* dob = reinterpret_cast<const T*>(p.dout) + b * p.do_sb + h * p.D;
  const T* kb = reinterpret_cast<const T*>(p.k) + b * p.k_sb + h * p.D;
  const T* vb = reinterpret_cast<const T*>(p.v) + b * p.v_sb + h * p.D;
  // PF (bf16 fixed modes, where the registers allow it): the wave's next key block loaded one block
  // ahead, the first under the staging
  constexpr bool PF = sizeof(T) == 2 && !REL && MODE != 0;
  uint4 kn[C::KCH], vn[C::KCH];
  if constexpr (PF) {
    load_row_regs<T, D>(kn, kb, p.k_st, (int64_t)wave * 16 + li, p.Lk, lane, p.D);
    load_row_regs<T, D>(vn, vb, p.v_st, (int64_t)wave * 16 + li, p.Lk, lane, p.D);
  }
  stage_two<T, D, false, false, NTH>(q_row, qb, p.q_st, do_row, dob, p.do_st, p.Lq, lq_pad, tid, p.D);
  if (!DUAL) stage_two<T, D, true, true, NTH>(q_tr, qb, p.q_st, do_tr, dob, p.do_st, p.Lq, lq_pad, tid, p.D);
  for (int i = tid; i < lq_pad; i += NTH) {
    s_lse[i] = i < p.Lq ? p.lse[bh * p.Lq + i] * LOG2E : INFINITY;
    s_delta[i] = i < p.Lq ? p.delta[bh * p.Lq + i] : 0.f;
  }
  stage_kbias<NTH>(kbias, p, b, (int)((p.Lk + 15) & ~15), tid);
  __syncthreads();
  T* dkb = reinterpret_cast<T*>(p.dk) + b * p.dk_sb + h * p.D;
  T* dvb = reinterpret_cast<T*>(p.dv) + b * p.dv_sb + h * p.D;
  const uint64_t seed = p.p > 0.f ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);
  const bool drop = MODE == 0 ? p.p > 0.f : MODE == 2;
  const float c2 = p.scale * LOG2E;
  const int nkb = (int)((p.Lk + 15) / 16);
  const int nqc = lq_pad / KC;  // query chunks of one MFMA k-chunk
  for (int kbk = wave; kbk < nkb; kbk += NTH / 64) {
    const int64_t k0 = (int64_t)kbk * 16, mykey = k0 + li;
    uint4 kf[C::KCH], vf[C::KCH];
    if constexpr (PF) {
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) { kf[kc] = kn[kc]; vf[kc] = vn[kc]; }
      load_row_regs<T, D>(kn, kb, p.k_st, k0 + NTH / 64 * 16 + li, p.Lk, lane, p.D);
      load_row_regs<T, D>(vn, vb, p.v_st, k0 + NTH / 64 * 16 + li, p.Lk, lane, p.D);
    } else {
      load_row_regs<T, D>(kf, kb, p.k_st, mykey, p.Lk, lane, p.D);
      load_row_regs<T, D>(vf, vb, p.v_st, mykey, p.Lk, lane, p.D);
    }
    // -inf for padded keys -> P = 0 (mode 1: their dK / dV rows are computed but never stored)
    const float kb2 = MODE == 1 ? 0.f : kbias[mykey];
    const uint64_t hcol = (uint64_t)(bh * p.Lq) * (uint64_t)p.kp + (uint64_t)(mykey >> 1);  // pair index, query 0
    const int kodd = (int)(mykey & 1);
    const float* relcol = REL ? p.rel_bias + rb_off(p, b) + h * p.Lq * p.Lk + (mykey < p.Lk ? mykey : 0) : nullptr;
    f32x4 dkv[2 * C::DT];  // dV (even) and dK (odd) of each 16-wide D subtile
#pragma unroll
    for (int i = 0; i < 2 * C::DT; ++i) dkv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Q / dO row fragments of the first query chunk; each iteration prefetches the next chunk's
    uint4 qa[SUBS * C::KCH], da[SUBS * C::KCH];
#pragma unroll
    for (int i = 0; i < SUBS * C::KCH; ++i) {
      qa[i] = row_frag<T, D>(q_row, i / C::KCH, i % C::KCH, lane);
      da[i] = row_frag<T, D>(do_row, i / C::KCH, i % C::KCH, lane);
    }
    for (int qc = 0; qc < nqc; ++qc) {
      // transposed dO / Q fragments of this chunk (B operands of dV / dK), read ahead of the softmax
      uint4 tb[2 * C::DT];
#pragma unroll
      for (int d = 0; d < C::DT; ++d) {
        tb[2 * d] = tr_frag<T, D>(do_tr, qc, d, lane);
        tb[2 * d + 1] = tr_frag<T, D>(q_tr, qc, d, lane);
      }
      f32x4 sd[2 * SUBS];  // S (even) and dP (odd) of each 16-query subtile, interleaved chains
#pragma unroll
      for (int i = 0; i < 2 * SUBS; ++i) sd[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) {
        uint4 fa[2 * SUBS], fb[2 * SUBS];
#pragma unroll
        for (int h2 = 0; h2 < SUBS; ++h2) {
          fa[2 * h2] = qa[h2 * C::KCH + kc]; fb[2 * h2] = kf[kc];
          fa[2 * h2 + 1] = da[h2 * C::KCH + kc]; fb[2 * h2 + 1] = vf[kc];
        }
        Mma<T>::template runN<2 * SUBS>(sd, fa, fb);
      }
      if (qc + 1 < nqc) {
#pragma unroll
        for (int i = 0; i < SUBS * C::KCH; ++i) {
          qa[i] = row_frag<T, D>(q_row, SUBS * (qc + 1) + i / C::KCH, i % C::KCH, lane);
          da[i] = row_frag<T, D>(do_row, SUBS * (qc + 1) + i / C::KCH, i % C::KCH, lane);
        }
      }
      f32x4 pd[SUBS], ds[SUBS];
#pragma unroll
      for (int h2 = 0; h2 < SUBS; ++h2) {
        const int qs = SUBS * qc + h2;
        const f32x4 sv = sd[2 * h2], dp = sd[2 * h2 + 1];
        const float4 l4 = *reinterpret_cast<const float4*>(s_lse + qs * 16 + 4 * g);
        const float4 d4 = *reinterpret_cast<const float4*>(s_delta + qs * 16 + 4 * g);
        const float lq2[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4.x, d4.y, d4.z, d4.w};
        float z[4] = {1.f, 1.f, 1.f, 1.f};
        if (drop) {  // one uniform branch per subtile; the element index advances by Lk per query
          if (MODE == 0 && p.dm_lds) {  // bit mykey of the query rows' words (LDS broadcast reads)
            const uint32_t* col = s_dm + (mykey >> 5);
            const int sh = (int)(mykey & 31);
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = ((col[(qs * 16 + 4 * g + r) * p.dmw] >> sh) & 1u) ? p.keep_scale : 0.f;
          } else if (p.idx32) {
            const uint32_t kpc1 = (uint32_t)p.kp * HASH_C1;
            const uint32_t c = ((uint32_t)hcol + (uint32_t)(qs * 16 + 4 * g + 2 * kodd) * (uint32_t)p.kp) * HASH_C1;
            keep4_col(hash_c1(hkey, c), hash_c1(hkey, c + kpc1), kodd, p, z);
          } else {
            const uint64_t idx = hcol + (uint64_t)(qs * 16 + 4 * g + 2 * kodd) * (uint64_t)p.kp;
            keep4_col(mmfd_hash_k(hkey, idx), mmfd_hash_k(hkey, idx + (uint64_t)p.kp), kodd, p, z);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lq = qs * 16 + 4 * g + r;
          float pr;
          if constexpr (MODE == 1) {  // (lse = +inf on padded queries: P = 0)
            pr = __builtin_amdgcn_exp2f(fmaf(sv[r], c2, -lq2[r]));
          } else {
            float t = fmaf(sv[r], c2, kb2);
            if (REL && lq < p.Lq && mykey < p.Lk) t = fmaf(relcol[(int64_t)lq * p.Lk], LOG2E, t);
            pr = __builtin_amdgcn_exp2f(t - lq2[r]);
          }
          pd[h2][r] = pr * z[r];
          ds[h2][r] = pr * (dp[r] * z[r] - dl[r]);
        }
      }
      const uint4 ap = pack_acc<T>(pd, 0);
      const uint4 as = pack_acc<T>(ds, 0);
      uint4 fa[2 * C::DT];
#pragma unroll
      for (int d = 0; d < C::DT; ++d) { fa[2 * d] = ap; fa[2 * d + 1] = as; }
      Mma<T>::template runN<2 * C::DT>(dkv, fa, tb);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t key = k0 + 4 * g + r;
      if (key < p.Lk) {
#pragma unroll
        for (int d = 0; d < C::DT; ++d) {
          if (d * 16 + li >= p.D) continue;
          T* pk = dkb + key * p.dk_st + d * 16 + li;
          T* pv = dvb + key * p.dv_st + d * 16 + li;
          float vk = dkv[2 * d + 1][r] * p.scale, vv = dkv[2 * d][r];
          if (p.acc_dkv) { vk += to_f32(*pk); vv += to_f32(*pv); }
          if constexpr (std::is_same<T, float>::value) {
            if (p.pl) {
              plane_put(p, pk, vk);
              plane_put(p, pv, vv);
              if (p.pl_only) continue;
            }
          }
          *pk = from_f32<T>(vk);
          *pv = from_f32<T>(vv);
        }
      }
    }
  }
}

template <typename T, int D, bool REL, int MODE>
__global__ void __launch_bounds__(V2_THREADS, sizeof(T) == 2 ? 4 : 1) attn_dq_v2_kernel(AttnP p) {
  static_assert(MODE == 0 || !REL, "fixed modes: no relative bias");
  // K/V of the head resident in LDS; each wave owns 16 queries: dQ = dS K (REL as in dK/dV)
  using C = AT<T, D>;
  constexpr int KC = v2_kc<T>(), SUBS = KC / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
  const int lk_pad = v2_pad(p.Lk, KC);
  const int img = lk_pad * C::RB;
  constexpr bool DUAL = V2<T, D>::DUAL;
  char* k_row = smem;
  char* v_row = smem + img;
  char* k_tr = DUAL ? k_row : smem + 2 * img;
  float* kbias = reinterpret_cast<float*>(smem + (DUAL ? 2 : 3) * img);
  const T* kb = reinterpret_cast<const T*>(p.k) + b * p.k_sb + h * p.D;
  const T* qb = reinterpret_cast<const T*>(p.q) + b * p.q_sb + h * p.D;
  const T* dob = reinterpret_cast<const T*>(p.dout) + b * p.do_sb + h * p.D;
  const T* obq = reinterpret_cast<const T*>(p.o) + b * p.o_sb + h * p.D;
  // PF (bf16 fixed modes, where the registers allow it): the wave's next query block's Q / dO / O
  // rows loaded one block ahead, the first under the staging
  constexpr bool PF = sizeof(T) == 2 && !REL && MODE != 0;
  uint4 qn[C::KCH], dn[C::KCH], on[C::KCH];
  if constexpr (PF) {
    load_row_regs<T, D>(qn, qb, p.q_st, (int64_t)wave * 16 + li, p.Lq, lane, p.D);
    load_row_regs<T, D>(dn, dob, p.do_st, (int64_t)wave * 16 + li, p.Lq, lane, p.D);
    load_row_regs<T, D>(on, obq, p.o_st, (int64_t)wave * 16 + li, p.Lq, lane, p.D);
  }
  stage_two<T, D, false, false>(k_row, kb, p.k_st, v_row, reinterpret_cast<const T*>(p.v) + b * p.v_sb + h * p.D,
                                p.v_st, p.Lk, lk_pad, tid, p.D);
  if (!DUAL) stage_all<T, D, true>(k_tr, kb, p.k_st, p.Lk, lk_pad, tid, p.D);
  stage_kbias<V2_THREADS>(kbias, p, b, lk_pad, tid);
  __syncthreads();
  T* dqb = reinterpret_cast<T*>(p.dq) + b * p.dq_sb + h * p.D;
  const uint64_t seed = p.p > 0.f ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);
  const bool drop = MODE == 0 ? p.p > 0.f : MODE == 2;
  const float c2 = p.scale * LOG2E;
  const int nqb = (int)((p.Lq + 15) / 16);
  const int nkc = lk_pad / KC;
  for (int qbk = wave; qbk < nqb; qbk += V2_THREADS / 64) {
    const int64_t q0 = (int64_t)qbk * 16, myq = q0 + li;
    uint4 qf[C::KCH], dof[C::KCH], of[C::KCH];
    if constexpr (PF) {
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) { qf[kc] = qn[kc]; dof[kc] = dn[kc]; of[kc] = on[kc]; }
      if (qbk + V2_THREADS / 64 < nqb) {
        const int64_t nq = myq + V2_THREADS / 64 * 16;
        load_row_regs<T, D>(qn, qb, p.q_st, nq, p.Lq, lane, p.D);
        load_row_regs<T, D>(dn, dob, p.do_st, nq, p.Lq, lane, p.D);
        load_row_regs<T, D>(on, obq, p.o_st, nq, p.Lq, lane, p.D);
      }
    } else {
      load_row_regs<T, D>(qf, qb, p.q_st, myq, p.Lq, lane, p.D);
      load_row_regs<T, D>(dof, dob, p.do_st, myq, p.Lq, lane, p.D);
      load_row_regs<T, D>(of, obq, p.o_st, myq, p.Lq, lane, p.D);
    }
    const float lse2 = myq < p.Lq ? p.lse[bh * p.Lq + myq] * LOG2E : INFINITY;
    // delta = rowsum(dO * O) from the dO fragments in registers and the O row (this kernel runs
    // before dK/dV and writes delta for it: no separate delta pass)
    float dlt;
    {
      float ds = 0.f;
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) ds += row_chunk_dot<T>(of[kc], dof[kc]);
      ds += __shfl_xor(ds, 16, 64);
      ds += __shfl_xor(ds, 32, 64);
      dlt = myq < p.Lq ? ds : 0.f;
      if (g == 0 && myq < p.Lq) p.delta[bh * p.Lq + myq] = ds;
    }
    const uint64_t hrow = (uint64_t)(bh * p.Lq + myq) * (uint64_t)p.kp;  // pair-index base of this query row
    const float* relrow = REL ? p.rel_bias + rb_off(p, b) + (h * p.Lq + (myq < p.Lq ? myq : 0)) * p.Lk : nullptr;
    const uint32_t* dmrow = MODE == 0 && p.dm ? dm_row(p, bh, myq < p.Lq ? myq : 0) : nullptr;
    f32x4 dq[C::DT];
#pragma unroll
    for (int d = 0; d < C::DT; ++d) dq[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fp32 (MFMA-bound, two waves per SIMD whatever the registers): K / V row fragments of the
    // next key chunk and this chunk's transposed K are read ahead; bf16 reads them where they are
    // used, which keeps the kernel at <= 128 VGPRs and two workgroups per CU (the read-ahead form
    // measured 211 -> 298 us per ViT/BERT call in bf16)
    constexpr bool PF = sizeof(T) == 4;
    uint4 ka[SUBS * C::KCH], va[SUBS * C::KCH];
    if constexpr (PF) {
#pragma unroll
      for (int i = 0; i < SUBS * C::KCH; ++i) {
        ka[i] = row_frag<T, D>(k_row, i / C::KCH, i % C::KCH, lane);
        va[i] = row_frag<T, D>(v_row, i / C::KCH, i % C::KCH, lane);
      }
    }
    for (int kc2 = 0; kc2 < nkc; ++kc2) {
      // the keep word of this chunk's keys (dropout bitmask), loaded ahead of the products
      const uint32_t kw = (MODE == 0 && p.p > 0.f && p.dm) ? dmrow[(SUBS * kc2) >> 1] : 0u;
      uint4 tk[C::DT];  // transposed K fragments (B operand of dQ)
      if constexpr (PF) {
#pragma unroll
        for (int d = 0; d < C::DT; ++d) tk[d] = tr_frag<T, D>(k_tr, kc2, d, lane);
      }
      f32x4 sd[2 * SUBS];
#pragma unroll
      for (int i = 0; i < 2 * SUBS; ++i) sd[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) {
        uint4 fa[2 * SUBS], fb[2 * SUBS];
#pragma unroll
        for (int h2 = 0; h2 < SUBS; ++h2) {
          if constexpr (PF) {
            fa[2 * h2] = ka[h2 * C::KCH + kc];
            fa[2 * h2 + 1] = va[h2 * C::KCH + kc];
          } else {
            fa[2 * h2] = row_frag<T, D>(k_row, SUBS * kc2 + h2, kc, lane);
            fa[2 * h2 + 1] = row_frag<T, D>(v_row, SUBS * kc2 + h2, kc, lane);
          }
          fb[2 * h2] = qf[kc];
          fb[2 * h2 + 1] = dof[kc];
        }
        Mma<T>::template runN<2 * SUBS>(sd, fa, fb);
      }
      if (PF && kc2 + 1 < nkc) {
#pragma unroll
        for (int i = 0; i < SUBS * C::KCH; ++i) {
          ka[i] = row_frag<T, D>(k_row, SUBS * (kc2 + 1) + i / C::KCH, i % C::KCH, lane);
          va[i] = row_frag<T, D>(v_row, SUBS * (kc2 + 1) + i / C::KCH, i % C::KCH, lane);
        }
      }
      f32x4 ds[SUBS];
#pragma unroll
      for (int h2 = 0; h2 < SUBS; ++h2) {
        const int ks = SUBS * kc2 + h2;
        const f32x4 sv = sd[2 * h2], dp = sd[2 * h2 + 1];
        float z[4] = {1.f, 1.f, 1.f, 1.f};
        if (drop) {  // one uniform branch per subtile
          if (MODE == 0 && p.dm) {
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = ((kw >> ((ks & 1) * 16 + 4 * g + r)) & 1u) ? p.keep_scale : 0.f;
          } else if (p.idx32) {
            const uint32_t c = ((uint32_t)hrow + (uint32_t)(ks * 8 + 2 * g)) * HASH_C1;
            keep4_pairs(hash_c1(hkey, c), hash_c1(hkey, c + HASH_C1), p, z);
          } else {
            const uint64_t pi = hrow + (uint64_t)(ks * 8 + 2 * g);
            keep4_pairs(mmfd_hash_k(hkey, pi), mmfd_hash_k(hkey, pi + 1), p, z);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = ks * 16 + 4 * g + r;
          float pr;
          if constexpr (MODE == 1) {
            // padded keys: their K rows are zero, so their dS adds nothing to dQ = dS K
            pr = __builtin_amdgcn_exp2f(fmaf(sv[r], c2, -lse2));
          } else {
            float t = fmaf(sv[r], c2, kbias[ks * 16 + 4 * g + r]);
            if (REL && key < p.Lk) t = fmaf(relrow[key], LOG2E, t);
            pr = __builtin_amdgcn_exp2f(t - lse2);
          }
          ds[h2][r] = pr * (dp[r] * z[r] - dlt);
        }
      }
      const uint4 as = pack_acc<T>(ds, 0);
      uint4 fa[C::DT];
#pragma unroll
      for (int d = 0; d < C::DT; ++d) {
        fa[d] = as;
        if constexpr (!PF) tk[d] = tr_frag<T, D>(k_tr, kc2, d, lane);
      }
      Mma<T>::template runN<C::DT>(dq, fa, tk);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t q = q0 + 4 * g + r;
      if (q < p.Lq) {
#pragma unroll
        for (int d = 0; d < C::DT; ++d) {
          if (d * 16 + li >= p.D) continue;
          T* pq = dqb + q * p.dq_st + d * 16 + li;
          float vq = dq[d][r] * p.scale;
          if (p.acc_dq) vq += to_f32(*pq);
          if constexpr (std::is_same<T, float>::value) {
            if (p.pl) {
              plane_put(p, pq, vq);
              if (p.pl_only) continue;
            }
          }
          *pq = from_f32<T>(vq);
        }
      }
    }
  }
}

}  // namespace
