// What every attention kernel family shares (attention.hip includes the family headers after this
// one): the kernel argument block AttnP, the dropout keep-bitmask and split-plane stores, the
// pair-hash dropout rule, the LDS row / transposed images with their MFMA fragment reads, and the
// additive bias lookups.
#pragma once
#include "common.h"
#include <math.h>
#include <type_traits>

namespace {

struct AttnP {
  int64_t B, H, Lq, Lk;
  int D;  // real head dim (<= the template's padded D; padding columns are zero)
  float scale;
  const void* q; int64_t q_sb, q_st;
  const void* k; int64_t k_sb, k_st;
  const void* v; int64_t v_sb, v_st;
  void* o; int64_t o_sb, o_st;
  float* lse;
  const float* key_bias;
  const float* rel_bias; int64_t rb_sb, rb_mod;
  const float* cos_ls; float cos_max_log;  // Swinv2 cosine attention (REL forward only)
  float p; uint32_t thr16; float keep_scale;
  int64_t kp;  // key pairs per query row, ceil(Lk / 2): attention dropout hashes one index per pair
  const uint64_t* seed; uint64_t salt;
  const void* dout; int64_t do_sb, do_st;
  void* dq; int64_t dq_sb, dq_st;
  void* dk; int64_t dk_sb, dk_st;
  void* dv; int64_t dv_sb, dv_st;
  float* delta;
  int acc_dq, acc_dkv;
  // fp32 backward: split planes of the packed [dq | dk | dv] buffer (base = dq), see mmfd_attn_args
  bf16* pl; int64_t pl_stride; const float* pl_base; int pl_only;
  int idx32;  // every dropout index fits 32 bits (hash_c1)
  int vst;    // x6 backward stores as 4-column groups (16-B fp32, 8-B planes): outputs and planes aligned
  int dbg;  // x6 phase experiments (MMFD_X6A_DBG): 1 = stage zeros, 2 = skip the products
  // dropout keep-bitmask (mmfd_attn_args::drop_mask): forward kernels that hash the mask write it,
  // backward kernels read it instead of re-hashing; dmw = words per query row, dm_lds = the dK/dV
  // kernel stages the head's rows in LDS (room left by its images)
  uint32_t* dm; int dmw; int dm_lds;
};

// word ((b*H + h)*Lq + q)*dmw + k/32 of the keep-bitmask, bit k % 32 = 1 when element (q, k) is kept
__device__ __forceinline__ uint32_t* dm_row(const AttnP& p, int64_t bh, int64_t q) { return p.dm + (bh * p.Lq + q) * p.dmw; }
// forward, S^T layout (lane (g, li): query q0 + li, keys k0 + ks*16 + 4g + r): `kb` holds the lane's
// keep bits of one 64-key chunk at bit ks*4 + r; the four lane groups' bits are merged by shuffles
// into the words k0/32 and k0/32 + 1 of the query's row (all 64 lanes must be active)
__device__ __forceinline__ void dm_write64(const AttnP& p, int64_t bh, int64_t myq, int k0, int g, uint32_t kb) {
  uint32_t w0 = ((kb & 0xFu) << (4 * g)) | (((kb >> 4) & 0xFu) << (16 + 4 * g));
  uint32_t w1 = (((kb >> 8) & 0xFu) << (4 * g)) | (((kb >> 12) & 0xFu) << (16 + 4 * g));
  w0 |= __shfl_xor(w0, 16, 64);
  w0 |= __shfl_xor(w0, 32, 64);
  w1 |= __shfl_xor(w1, 16, 64);
  w1 |= __shfl_xor(w1, 32, 64);
  if (myq < p.Lq) {
    const int w = k0 >> 5;
    uint32_t* row = dm_row(p, bh, myq);
    if (g == 0 && w < p.dmw) row[w] = w0;
    if (g == 1 && w + 1 < p.dmw) row[w + 1] = w1;
  }
}

// one fp32 gradient element into the planes at its offset in the packed buffer
__device__ __forceinline__ void plane_put(const AttnP& p, const float* dst, float v) {
  const int64_t off = dst - p.pl_base;
  const bf16 h = (bf16)v;
  const float r = v - (float)h;
  const bf16 m = (bf16)r;
  p.pl[off] = h;
  p.pl[off + p.pl_stride] = m;
  p.pl[off + 2 * p.pl_stride] = (bf16)(r - (float)m);
}

// Dropout with 32-bit indices (B*H*Lq*Lk <= 2^32: AttnP::idx32, required by the x6 kernels): mmfd_hash_k(key, idx) = mix32(key ^ lo(idx) * C1 ^
// hi(idx) * C2) with hi(idx) = 0, and lo(idx) * C1 (mod 2^32) advances by additions — C1 per key,
// Lk * C1 per query — so an element costs one v_add in place of the 64-bit index arithmetic and
// its two extra 32-bit multiplies (bit-identical masks).
constexpr uint32_t HASH_C1 = 0x9e3779b1u;

// 4x4 transpose across each lane quad (lanes 4j + t): afterwards lane t, register c holds what lane
// c held in register t. A 16x16 MFMA accumulator (lane (g, i): rows 4g + r, column i) becomes
// rows 4g + (i & 3) with 4 consecutive columns 4 (i >> 2) + c per lane — one 16-B fp32 store and
// 8-B plane stores per 4 outputs instead of one 4-B and three 2-B stores per output
__device__ __forceinline__ void quad_tr(float (&x)[4], int t) {
  const bool o1 = t & 1, o2 = t & 2;
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    const float r = __shfl_xor(o1 ? x[j] : x[j + 1], 1, 64);
    if (o1) x[j] = r; else x[j + 1] = r;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float r = __shfl_xor(o2 ? x[j] : x[j + 2], 2, 64);
    if (o2) x[j] = r; else x[j + 2] = r;
  }
}

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// four consecutive fp32 outputs at dst (16-B aligned; AttnP::vst), accumulated onto dst when acc,
// and their split planes when p.pl (the same split3 rule as plane_put)
__device__ __forceinline__ void x6_put4(const AttnP& p, float* dst, const float (&x)[4], bool acc) {
  float4 v = make_float4(x[0], x[1], x[2], x[3]);
  if (acc) {
    const float4 o = *reinterpret_cast<const float4*>(dst);
    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
  }
  if (p.pl) {
    const float e[4] = {v.x, v.y, v.z, v.w};
    bf16x4 h, m, l;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bf16 hu = (bf16)e[u];
      const float r = e[u] - (float)hu;
      const bf16 mu = (bf16)r;
      h[u] = hu;
      m[u] = mu;
      l[u] = (bf16)(r - (float)mu);
    }
    bf16* pp = p.pl + (dst - p.pl_base);
    *reinterpret_cast<uint2*>(pp) = __builtin_bit_cast(uint2, h);
    *reinterpret_cast<uint2*>(pp + p.pl_stride) = __builtin_bit_cast(uint2, m);
    *reinterpret_cast<uint2*>(pp + 2 * p.pl_stride) = __builtin_bit_cast(uint2, l);
    if (p.pl_only) return;
  }
  *reinterpret_cast<float4*>(dst) = v;
}
__device__ __forceinline__ uint32_t hash_c1(uint32_t key, uint32_t idx_c1) { return mmfd_mix32(key ^ idx_c1); }

// Attention dropout draws ONE 32-bit hash per key pair: element (row, k) of the [B*H*Lq][Lk] score
// matrix (row = (b*H + h)*Lq + q) uses h = mmfd_hash_k(key, row * kp + k / 2), kp = ceil(Lk / 2),
// and is kept when its 16-bit half (low for even k, high for odd k) is >= thr16 = round(p * 65536)
// (p = 0.1: thr16 = 6554, a keep probability within 6e-6 of 0.9). oracle/dropout_hash.py
// attn_keep_mask restates it. A lane holding 4 consecutive keys (forward, dQ) hashes twice where it
// hashed four times; a lane holding one key of 4 queries (dK/dV) hashes 2 of the 4 pairs and takes
// the other 2 from its neighbour lane (the pair partner key).
__device__ __forceinline__ bool pair_keep(uint32_t h, int odd, uint32_t thr16) {
  return (odd ? (h >> 16) : (h & 0xffffu)) >= thr16;
}
__device__ __forceinline__ uint32_t attn_hash64(uint32_t hkey, const AttnP& p, int64_t row, int64_t key) {
  return mmfd_hash_k(hkey, (uint64_t)row * (uint64_t)p.kp + (uint64_t)(key >> 1));
}
// keep factors (keep_scale or 0) of 4 consecutive keys starting at an even key, from the pair hashes
// h0 (keys 0, 1) and h1 (keys 2, 3)
__device__ __forceinline__ void keep4_pairs(uint32_t h0, uint32_t h1, const AttnP& p, float (&z)[4]) {
  z[0] = pair_keep(h0, 0, p.thr16) ? p.keep_scale : 0.f;
  z[1] = pair_keep(h0, 1, p.thr16) ? p.keep_scale : 0.f;
  z[2] = pair_keep(h1, 0, p.thr16) ? p.keep_scale : 0.f;
  z[3] = pair_keep(h1, 1, p.thr16) ? p.keep_scale : 0.f;
}
// one key per lane, 4 query rows r: this lane hashed rows (odd ? 2 : 0) -> ha and (odd ? 3 : 1) -> hb
// of its key pair; the partner lane (lane ^ 1, the pair's other key) hashed the other two rows. All
// 64 lanes must be active.
__device__ __forceinline__ void keep4_col(uint32_t ha, uint32_t hb, int odd, const AttnP& p, float (&z)[4]) {
  const uint32_t xa = __shfl_xor(ha, 1, 64), xb = __shfl_xor(hb, 1, 64);
  const uint32_t h[4] = {odd ? xa : ha, odd ? xb : hb, odd ? ha : xa, odd ? hb : xb};
#pragma unroll
  for (int r = 0; r < 4; ++r) z[r] = pair_keep(h[r], odd, p.thr16) ? p.keep_scale : 0.f;
}

template <typename T, int D>
struct AT {
  static constexpr int ESZ = sizeof(T);
  static constexpr int RB = D * ESZ;          // bytes per row
  static constexpr int NCH = RB / 16;         // 16-B chunks per row
  static constexpr int EPC = 16 / ESZ;
  static constexpr int KCH = D / Mma<T>::KC;  // MFMA chunks along D
  static constexpr int TILE = 64 * RB;        // one 64-row image
  static constexpr int DT = D / 16;           // 16-wide output subtiles along D
  static constexpr int PCH = 64 / Mma<T>::KC; // MFMA chunks along a 64-row block
};

// ROW image: 16-B chunk c of row r
template <typename T, int D>
__device__ __forceinline__ int row_off(int r, int c) {
  constexpr int NCH = AT<T, D>::NCH;
  return r * AT<T, D>::RB + ((c ^ (r & (NCH - 1))) << 4);
}
// TR image: 16-B chunk c of row r (layout chosen for the transposed operand reads)
template <typename T, int D>
__device__ __forceinline__ int tr_chunk(int r, int c) {
  if (sizeof(T) == 2) {
    // D = 64 (128-B rows): the ROW swizzle c ^ (r & 7) is also conflict-free for the transposed
    // 8-row reads, so one image serves both kinds of read (DUAL below)
    if (D == 64) return c ^ (r & 7);
    return c ^ (2 * ((r >> 2) & 1));
  }
  // fp32: the ROW swizzle c ^ (r & (NCH-1)) again; the 4-byte transposed reads of rows r+4g
  // (g = 0..3) then land in distinct 4-chunk groups at D = 64 (16 chunks per row)
  return c ^ (r & (AT<T, D>::NCH - 1));
}

// stage 64 rows [row0, row0+64) of a (token-strided) head slice into an image
template <typename T, int D, bool TR>
__device__ __forceinline__ void stage_rows(char* lds, const T* __restrict__ base, int64_t st, int64_t row0,
                                           int64_t nrows, int tid, int dreal) {
  constexpr int NCH = AT<T, D>::NCH, EPC = AT<T, D>::EPC;
  for (int c = tid; c < 64 * NCH; c += 256) {
    const int r = c / NCH, ch = c % NCH;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row0 + r < nrows && ch * EPC < dreal) v = *reinterpret_cast<const uint4*>(base + (row0 + r) * st + ch * EPC);
    const int off = TR ? (r * AT<T, D>::RB + (tr_chunk<T, D>(r, ch) << 4)) : row_off<T, D>(r, ch);
    *reinterpret_cast<uint4*>(lds + off) = v;
  }
}

// A-operand fragment (16 rows starting at sub*16) from a ROW image, MFMA chunk kc along D
template <typename T, int D>
__device__ __forceinline__ uint4 row_frag(const char* lds, int sub, int kc, int lane) {
  const int row = sub * 16 + (lane & 15);
  return lds_read16(lds, row_off<T, D>(row, kc * 4 + (lane >> 4)));
}

// B-operand fragment from a TR image: k = rows of the 64-row block (split order for bf16),
// n = 16 columns starting at dsub*16. chunk c covers rows [c*KC, c*KC+KC).
template <typename T, int D>
__device__ __forceinline__ uint4 tr_frag(const char* lds, int c, int dsub, int lane) {
  const int g = lane >> 4, i = lane & 15;
  constexpr int RB = AT<T, D>::RB;
  if (sizeof(T) == 2) {
    const int q = i >> 2, p = i & 3;
    const int u = dsub * 4 + p;  // 8-B unit (4 bf16)
    uint2 x[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = c * 32 + 16 * h + 4 * g + q;
      const int ch = tr_chunk<T, D>(r, u >> 1);
      x[h] = lds_read_tr16(lds + r * RB + (ch << 4) + ((u & 1) << 3));
    }
    return make_uint4(x[0].x, x[0].y, x[1].x, x[1].y);
  } else {
    const int col = dsub * 16 + i;
    uint32_t v[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int r = c * 16 + 4 * g + s;
      const int ch = tr_chunk<T, D>(r, col >> 2);
      v[s] = *reinterpret_cast<const uint32_t*>(lds + r * RB + (ch << 4) + (col & 3) * 4);
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
  }
}

// pack 16x16 accumulators (rows in split order) into the A fragment of MFMA chunk c
template <typename T>
__device__ __forceinline__ uint4 pack_acc(const f32x4* s, int c) {
  if (sizeof(T) == 2) {
    const f32x4 a = s[2 * c], b = s[2 * c + 1];
    bf16x8 v = {(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
    return __builtin_bit_cast(uint4, v);
  } else {
    const f32x4 a = s[c];
    return make_uint4(__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3]));
  }
}

// dot product of two 16-B chunks of T elements (fp32 sum)
template <typename T>
__device__ __forceinline__ float row_chunk_dot(const uint4& a, const uint4& b) {
  if constexpr (sizeof(T) == 2) {
    const bf16x8 x = __builtin_bit_cast(bf16x8, a), y = __builtin_bit_cast(bf16x8, b);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf((float)x[e], (float)y[e], s);
    return s;
  } else {
    return fmaf(__uint_as_float(a.x), __uint_as_float(b.x),
                fmaf(__uint_as_float(a.y), __uint_as_float(b.y),
                     fmaf(__uint_as_float(a.z), __uint_as_float(b.z), __uint_as_float(a.w) * __uint_as_float(b.w))));
  }
}

// per-lane 16-B operand chunks of one row (query or key) held in registers
template <typename T, int D>
__device__ __forceinline__ void load_row_regs(uint4* f, const T* __restrict__ base, int64_t st,
                                              int64_t row, int64_t nrows, int lane, int dreal) {
  const int g = lane >> 4;
#pragma unroll
  for (int kc = 0; kc < AT<T, D>::KCH; ++kc) {
    f[kc] = make_uint4(0, 0, 0, 0);
    const int col = (kc * 4 + g) * AT<T, D>::EPC;
    if (row < nrows && col < dreal) f[kc] = *reinterpret_cast<const uint4*>(base + row * st + col);
  }
}

// batch offset of rel_bias: b * sb, or (b % mod) * sb when the bias repeats every `mod` batch rows
// (Swinv2 shifted-window masks: one [H][L][L] bias per window position, windows batch-major)
__device__ __forceinline__ int64_t rb_off(const AttnP& p, int64_t b) {
  return (p.rb_mod > 0 ? b % p.rb_mod : b) * p.rb_sb;
}

__device__ __forceinline__ float bias_at(const AttnP& p, int64_t b, int64_t h, int64_t q, int64_t key) {
  float v = 0.f;
  if (p.key_bias) v += p.key_bias[b * p.Lk + key];
  if (p.rel_bias) v += p.rel_bias[rb_off(p, b) + (h * p.Lq + q) * p.Lk + key];
  return v;
}

}  // namespace
