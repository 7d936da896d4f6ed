// The streaming attention kernels: 64-row blocks of K/V (or Q/dO) pass through LDS, any Lq / Lk.
//
// Every product runs on 16x16 MFMAs (bf16: 16x16x32, fp32: 16x16x4). Work split:
//   forward  : workgroup = (b, h, 64 queries), wave = 16 queries; loops over 64-key blocks staged
//              in LDS. S^T = K Q^T puts the query on the lane, so the online-softmax statistics are
//              lane-local (reduced over 4 lanes) and P^T's accumulator is directly the A operand of
//              O = P V (keys in the "split" order {4g..4g+3, 16+4g..16+4g+3}); V is read with the
//              hardware-transposing ds_read_b64_tr_b16.
//   backward : two kernels, no atomics (deterministic): dK/dV per 64-key block looping over query
//              blocks (S = Q K^T puts the key on the lane: P and dS are directly the A operands of
//              dV = P^T dO and dK = dS^T Q), and dQ per 64-query block looping over key blocks
//              (S^T again). delta = rowsum(dO * O) comes from a small kernel first. The gradient of
//              a per-batch additive bias (mmfd_attn_args.d_rel_bias, DeBERTa) is a third kernel of the
//              dQ shape that writes dS itself (attn_bwd_ds_kernel).
#pragma once
#include "attn_common.h"

namespace {

// Dynamic LDS of these kernels in 64-row images (AT::TILE), as each kernel carves its smem: the
// forward and dS hold K and V; dK/dV holds Q and dO as row and transposed images and 2 x 64 floats
// (lse, delta); dQ holds K as row and transposed image and V. The delta kernel uses none.
template <typename T, int D> constexpr int stream_kv_lds() { return 2 * AT<T, D>::TILE; }
template <typename T, int D> constexpr int stream_dkdv_lds() { return 4 * AT<T, D>::TILE + 2 * 64 * 4; }
template <typename T, int D> constexpr int stream_dq_lds() { return 3 * AT<T, D>::TILE; }

// --------------------------------------------------------------------------------------------
// forward
// --------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void __launch_bounds__(256) attn_fwd_kernel(AttnP p) {
  using C = AT<T, D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_img = smem;
  char* v_img = smem + C::TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int64_t bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int64_t q0 = (int64_t)blockIdx.x * 64 + wave * 16;
  const T* qb = reinterpret_cast<const T*>(p.q) + b * p.q_sb + h * p.D;
  const T* kb = reinterpret_cast<const T*>(p.k) + b * p.k_sb + h * p.D;
  const T* vb = reinterpret_cast<const T*>(p.v) + b * p.v_sb + h * p.D;
  const int64_t myq = q0 + li;

  uint4 qf[C::KCH];
  load_row_regs<T, D>(qf, qb, p.q_st, myq, p.Lq, lane, p.D);
  const uint64_t seed = p.p > 0.f ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);

  float m = -INFINITY, lsum = 0.f;
  f32x4 o[C::DT];
#pragma unroll
  for (int d = 0; d < C::DT; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t k0 = 0; k0 < p.Lk; k0 += 64) {
    __syncthreads();
    stage_rows<T, D, false>(k_img, kb, p.k_st, k0, p.Lk, tid, p.D);
    stage_rows<T, D, true>(v_img, vb, p.v_st, k0, p.Lk, tid, p.D);
    __syncthreads();

    f32x4 s[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      s[ks] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) Mma<T>::run(s[ks], row_frag<T, D>(k_img, ks, kc, lane), qf[kc]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t key = k0 + ks * 16 + 4 * g + r;
        float v = s[ks][r] * p.scale;
        if (key >= p.Lk) v = -INFINITY;
        else if (p.key_bias || p.rel_bias) v += bias_at(p, b, h, myq < p.Lq ? myq : 0, key);
        s[ks][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mnew = fmaxf(m, mx);
    const float alpha = __expf(m - mnew);
    float rs = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __expf(s[ks][r] - mnew);
        rs += e;
        float pe = e;
        if (p.p > 0.f) {
          const int64_t key = k0 + ks * 16 + 4 * g + r;
          const uint32_t hsh = attn_hash64(hkey, p, bh * p.Lq + myq, key);
          pe = pair_keep(hsh, (int)(key & 1), p.thr16) ? e * p.keep_scale : 0.f;
        }
        s[ks][r] = pe;
      }
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);
    lsum = lsum * alpha + rs;
    m = mnew;
    // rescale O rows (row = local query 4g+r, whose alpha sits in lane 4g+r)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
      for (int d = 0; d < C::DT; ++d) o[d][r] *= ar;
    }
#pragma unroll
    for (int c = 0; c < C::PCH; ++c) {
      const uint4 a = pack_acc<T>(s, c);
#pragma unroll
      for (int d = 0; d < C::DT; ++d) Mma<T>::run(o[d], a, tr_frag<T, D>(v_img, c, d, lane));
    }
  }

  T* ob = reinterpret_cast<T*>(p.o) + b * p.o_sb + h * p.D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float lr = __shfl(lsum, 4 * g + r, 64);
    const int64_t q = q0 + 4 * g + r;
    const float inv = 1.0f / lr;
    if (q < p.Lq) {
#pragma unroll
      for (int d = 0; d < C::DT; ++d)
        if (d * 16 + li < p.D) ob[q * p.o_st + d * 16 + li] = from_f32<T>(o[d][r] * inv);
    }
  }
  if (g == 0 && myq < p.Lq) p.lse[bh * p.Lq + myq] = m + __logf(lsum);
}

// --------------------------------------------------------------------------------------------
// backward: delta = rowsum(dO * O)
// --------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void attn_delta_kernel(AttnP p) {
  // 8 lanes per (b,h,q) row for D=64 (4 for D=32): each lane a 16-B chunk
  constexpr int LPR = AT<T, D>::NCH;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = gid / LPR;
  const int ch = gid % LPR;
  const int64_t total = p.B * p.H * p.Lq;
  float s = 0.f;
  if (row < total) {
    const int64_t q = row % p.Lq, bh = row / p.Lq, b = bh / p.H, h = bh % p.H;
    if (ch * AT<T, D>::EPC < p.D) {
      const T* o = reinterpret_cast<const T*>(p.o) + b * p.o_sb + q * p.o_st + h * p.D + ch * AT<T, D>::EPC;
      const T* d = reinterpret_cast<const T*>(p.dout) + b * p.do_sb + q * p.do_st + h * p.D + ch * AT<T, D>::EPC;
#pragma unroll
      for (int j = 0; j < AT<T, D>::EPC; ++j) s += to_f32(o[j]) * to_f32(d[j]);
    }
  }
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (row < total && ch == 0) p.delta[row] = s;
}

// --------------------------------------------------------------------------------------------
// backward: dK, dV (workgroup = 64 keys, wave = 16 keys)
// --------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void __launch_bounds__(256) attn_bwd_dkdv_kernel(AttnP p) {
  using C = AT<T, D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* q_row = smem;
  char* q_tr = smem + C::TILE;
  char* do_row = smem + 2 * C::TILE;
  char* do_tr = smem + 3 * C::TILE;
  float* s_lse = reinterpret_cast<float*>(smem + 4 * C::TILE);
  float* s_delta = s_lse + 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int64_t bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int64_t k0 = (int64_t)blockIdx.x * 64 + wave * 16;
  const int64_t mykey = k0 + li;
  const T* qb = reinterpret_cast<const T*>(p.q) + b * p.q_sb + h * p.D;
  const T* kb = reinterpret_cast<const T*>(p.k) + b * p.k_sb + h * p.D;
  const T* vb = reinterpret_cast<const T*>(p.v) + b * p.v_sb + h * p.D;
  const T* dob = reinterpret_cast<const T*>(p.dout) + b * p.do_sb + h * p.D;
  const uint64_t seed = p.p > 0.f ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);

  uint4 kf[C::KCH], vf[C::KCH];
  load_row_regs<T, D>(kf, kb, p.k_st, mykey, p.Lk, lane, p.D);
  load_row_regs<T, D>(vf, vb, p.v_st, mykey, p.Lk, lane, p.D);

  f32x4 dk[C::DT], dv[C::DT];
#pragma unroll
  for (int d = 0; d < C::DT; ++d) { dk[d] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[d] = dk[d]; }

  for (int64_t qs0 = 0; qs0 < p.Lq; qs0 += 64) {
    __syncthreads();
    stage_rows<T, D, false>(q_row, qb, p.q_st, qs0, p.Lq, tid, p.D);
    stage_rows<T, D, true>(q_tr, qb, p.q_st, qs0, p.Lq, tid, p.D);
    stage_rows<T, D, false>(do_row, dob, p.do_st, qs0, p.Lq, tid, p.D);
    stage_rows<T, D, true>(do_tr, dob, p.do_st, qs0, p.Lq, tid, p.D);
    if (tid < 64) {
      const int64_t q = qs0 + tid;
      s_lse[tid] = q < p.Lq ? p.lse[bh * p.Lq + q] : INFINITY;
      s_delta[tid] = q < p.Lq ? p.delta[bh * p.Lq + q] : 0.f;
    }
    __syncthreads();

    f32x4 pd[4], ds[4];
#pragma unroll
    for (int qs = 0; qs < 4; ++qs) {
      f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = sv;
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) {
        Mma<T>::run(sv, row_frag<T, D>(q_row, qs, kc, lane), kf[kc]);
        Mma<T>::run(dp, row_frag<T, D>(do_row, qs, kc, lane), vf[kc]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lq = qs * 16 + 4 * g + r;
        const int64_t q = qs0 + lq;
        float pr = 0.f;
        if (mykey < p.Lk) {
          float sc = sv[r] * p.scale;
          if ((p.key_bias || p.rel_bias) && q < p.Lq) sc += bias_at(p, b, h, q, mykey);
          pr = __expf(sc - s_lse[lq]);
        }
        float z = 1.f;
        if (p.p > 0.f) {
          const uint32_t hsh = attn_hash64(hkey, p, bh * p.Lq + q, mykey);
          z = pair_keep(hsh, (int)(mykey & 1), p.thr16) ? p.keep_scale : 0.f;
        }
        pd[qs][r] = pr * z;
        ds[qs][r] = pr * (dp[r] * z - s_delta[lq]);
      }
    }
#pragma unroll
    for (int c = 0; c < C::PCH; ++c) {
      const uint4 ap = pack_acc<T>(pd, c);
      const uint4 as = pack_acc<T>(ds, c);
#pragma unroll
      for (int d = 0; d < C::DT; ++d) {
        Mma<T>::run(dv[d], ap, tr_frag<T, D>(do_tr, c, d, lane));
        Mma<T>::run(dk[d], as, tr_frag<T, D>(q_tr, c, d, lane));
      }
    }
  }

  T* dkb = reinterpret_cast<T*>(p.dk) + b * p.dk_sb + h * p.D;
  T* dvb = reinterpret_cast<T*>(p.dv) + b * p.dv_sb + h * p.D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t key = k0 + 4 * g + r;
    if (key < p.Lk) {
#pragma unroll
      for (int d = 0; d < C::DT; ++d) {
        if (d * 16 + li >= p.D) continue;
        T* pk = dkb + key * p.dk_st + d * 16 + li;
        T* pv = dvb + key * p.dv_st + d * 16 + li;
        float vk = dk[d][r] * p.scale, vv = dv[d][r];
        if (p.acc_dkv) { vk += to_f32(*pk); vv += to_f32(*pv); }
        *pk = from_f32<T>(vk);
        *pv = from_f32<T>(vv);
      }
    }
  }
}

// --------------------------------------------------------------------------------------------
// backward: dQ (workgroup = 64 queries, wave = 16 queries)
// --------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void __launch_bounds__(256) attn_bwd_dq_kernel(AttnP p) {
  using C = AT<T, D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_row = smem;
  char* k_tr = smem + C::TILE;
  char* v_row = smem + 2 * C::TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int64_t bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int64_t q0 = (int64_t)blockIdx.x * 64 + wave * 16;
  const int64_t myq = q0 + li;
  const T* qb = reinterpret_cast<const T*>(p.q) + b * p.q_sb + h * p.D;
  const T* kb = reinterpret_cast<const T*>(p.k) + b * p.k_sb + h * p.D;
  const T* vb = reinterpret_cast<const T*>(p.v) + b * p.v_sb + h * p.D;
  const T* dob = reinterpret_cast<const T*>(p.dout) + b * p.do_sb + h * p.D;
  const uint64_t seed = p.p > 0.f ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);

  uint4 qf[C::KCH], dof[C::KCH];
  load_row_regs<T, D>(qf, qb, p.q_st, myq, p.Lq, lane, p.D);
  load_row_regs<T, D>(dof, dob, p.do_st, myq, p.Lq, lane, p.D);
  const float lse = myq < p.Lq ? p.lse[bh * p.Lq + myq] : INFINITY;
  const float dlt = myq < p.Lq ? p.delta[bh * p.Lq + myq] : 0.f;

  f32x4 dq[C::DT];
#pragma unroll
  for (int d = 0; d < C::DT; ++d) dq[d] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t k0 = 0; k0 < p.Lk; k0 += 64) {
    __syncthreads();
    stage_rows<T, D, false>(k_row, kb, p.k_st, k0, p.Lk, tid, p.D);
    stage_rows<T, D, true>(k_tr, kb, p.k_st, k0, p.Lk, tid, p.D);
    stage_rows<T, D, false>(v_row, vb, p.v_st, k0, p.Lk, tid, p.D);
    __syncthreads();

    f32x4 ds[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = sv;
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) {
        Mma<T>::run(sv, row_frag<T, D>(k_row, ks, kc, lane), qf[kc]);
        Mma<T>::run(dp, row_frag<T, D>(v_row, ks, kc, lane), dof[kc]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t key = k0 + ks * 16 + 4 * g + r;
        float pr = 0.f;
        if (key < p.Lk) {
          float sc = sv[r] * p.scale;
          if ((p.key_bias || p.rel_bias) && myq < p.Lq) sc += bias_at(p, b, h, myq, key);
          pr = __expf(sc - lse);
        }
        float z = 1.f;
        if (p.p > 0.f) {
          const uint32_t hsh = attn_hash64(hkey, p, bh * p.Lq + myq, key);
          z = pair_keep(hsh, (int)(key & 1), p.thr16) ? p.keep_scale : 0.f;
        }
        ds[ks][r] = pr * (dp[r] * z - dlt);
      }
    }
#pragma unroll
    for (int c = 0; c < C::PCH; ++c) {
      const uint4 as = pack_acc<T>(ds, c);
#pragma unroll
      for (int d = 0; d < C::DT; ++d) Mma<T>::run(dq[d], as, tr_frag<T, D>(k_tr, c, d, lane));
    }
  }

  T* dqb = reinterpret_cast<T*>(p.dq) + b * p.dq_sb + h * p.D;
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
        *pq = from_f32<T>(vq);
      }
    }
  }
}

// --------------------------------------------------------------------------------------------
// backward: dS, the gradient of a per-batch additive rel_bias [B][H][Lq][Lk] (DeBERTa c2p + p2c)
// --------------------------------------------------------------------------------------------
// Workgroup = 64 queries, wave = 16 queries, looping over 64-key blocks staged in LDS exactly like
// attn_bwd_dq_kernel: S^T = K Q^T and dP^T = V dO^T on MFMAs put the query on the lane, so lse and
// delta are lane-local, and a lane holds 4 consecutive keys of its query:
//   dS[q][k] = P (dP - delta),  P = exp(scale q.k + key_bias[k] + rel_bias[q][k] - lse[q])
// (no `scale`: the bias enters S unscaled). It runs after the dQ / dK/dV kernels of the same call
// (mmfd_attn_bwd's d_rel_bias, DROP = false: that entry refuses dropout) or of the preceding call
// (mmfd_attn_bwd_ds, either instantiation) and reads the delta they left; those kernels are
// untouched. Stores are 16-B vector stores when Lk % 4 == 0, else 4-B ones.
//
// DROP: dP = M (dO V^T) / (1 - p) with the keep mask M the forward drew — delta = rowsum(dO * O) =
// rowsum(P * dP) holds under dropout as well, so dS = P (dP - delta) stands. The lane's 4 consecutive
// keys start at a multiple of 4: two key pairs, two hashes (pair_keep). A template argument, not a
// run-time flag: the dropout-free instantiation carries no hash code (see the x6 forward).
//
// Masked keys come out exactly 0: key_bias of a masked key is -FLT_MAX (mmfd_mask_to_bias), which
// absorbs the finite rest of the score, while lse of a row with at least one real key is finite, so
// the exponent is far below DS_EXP_MIN = -104 < ln(2^-150): there exp() rounds to +0 in fp32
// whatever the rounding of the intrinsic, and the kernel returns the literal 0 for such arguments
// instead of calling it. 0 * (dP - delta) is 0 because dP and delta are finite for finite inputs.
// (A row whose keys are ALL masked has lse near -FLT_MAX and uniform P, as in the forward; DeBERTa
// zeroes dO of those rows first, mmfd_attn_fill_masked_rows_bwd, which makes their dS 0 as well.)
constexpr float DS_EXP_MIN = -104.f;

template <typename T, int D, bool DROP>
__global__ void __launch_bounds__(256) attn_bwd_ds_kernel(AttnP p, float* __restrict__ ds_out) {
  using C = AT<T, D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_row = smem;
  char* v_row = smem + C::TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int64_t bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int64_t q0 = (int64_t)blockIdx.x * 64 + wave * 16;
  const int64_t myq = q0 + li;
  const T* qb = reinterpret_cast<const T*>(p.q) + b * p.q_sb + h * p.D;
  const T* kb = reinterpret_cast<const T*>(p.k) + b * p.k_sb + h * p.D;
  const T* vb = reinterpret_cast<const T*>(p.v) + b * p.v_sb + h * p.D;
  const T* dob = reinterpret_cast<const T*>(p.dout) + b * p.do_sb + h * p.D;

  uint4 qf[C::KCH], dof[C::KCH];
  load_row_regs<T, D>(qf, qb, p.q_st, myq, p.Lq, lane, p.D);
  load_row_regs<T, D>(dof, dob, p.do_st, myq, p.Lq, lane, p.D);
  const bool qok = myq < p.Lq;
  const float lse = qok ? p.lse[bh * p.Lq + myq] : INFINITY;
  const float dlt = qok ? p.delta[bh * p.Lq + myq] : 0.f;
  const int64_t rowoff = (bh * p.Lq + (qok ? myq : 0)) * p.Lk;  // [B][H][Lq][Lk] contiguous, as rel_bias
  const float* relrow = p.rel_bias + rowoff;
  float* dsrow = ds_out + rowoff;
  const bool vec4 = (p.Lk & 3) == 0;  // rows then start 16-B aligned (base alignment checked by the host)
  uint32_t hkey = 0u;
  if constexpr (DROP) hkey = mmfd_hash_key(*p.seed, p.salt);

  for (int64_t k0 = 0; k0 < p.Lk; k0 += 64) {
    __syncthreads();
    stage_rows<T, D, false>(k_row, kb, p.k_st, k0, p.Lk, tid, p.D);
    stage_rows<T, D, false>(v_row, vb, p.v_st, k0, p.Lk, tid, p.D);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = sv;
#pragma unroll
      for (int kc = 0; kc < C::KCH; ++kc) {
        Mma<T>::run(sv, row_frag<T, D>(k_row, ks, kc, lane), qf[kc]);
        Mma<T>::run(dp, row_frag<T, D>(v_row, ks, kc, lane), dof[kc]);
      }
      const int64_t key0 = k0 + ks * 16 + 4 * g;
      if (!qok || key0 >= p.Lk) continue;
      float ds[4];
      float z[4] = {1.f, 1.f, 1.f, 1.f};
      if constexpr (DROP) {  // keys key0, key0 + 1 | key0 + 2, key0 + 3 (a pair past Lk is hashed and not used)
        const int64_t row = bh * p.Lq + myq;
        keep4_pairs(attn_hash64(hkey, p, row, key0), attn_hash64(hkey, p, row, key0 + 2), p, z);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t key = key0 + r;
        ds[r] = 0.f;
        if (key < p.Lk) {
          float sc = sv[r] * p.scale + relrow[key];
          if (p.key_bias) sc += p.key_bias[b * p.Lk + key];
          const float x = sc - lse;
          const float pr = x < DS_EXP_MIN ? 0.f : __expf(x);
          if constexpr (DROP) ds[r] = pr * (dp[r] * z[r] - dlt);
          else ds[r] = pr * (dp[r] - dlt);
        }
      }
      if (vec4) {
        *reinterpret_cast<float4*>(dsrow + key0) = make_float4(ds[0], ds[1], ds[2], ds[3]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (key0 + r < p.Lk) dsrow[key0 + r] = ds[r];
      }
    }
  }
}

// the keep-bitmask from the hash, for forward kernels that do not write it (the streaming v1 path)
__global__ void dm_fill_kernel(AttnP p) {
  const int64_t words = p.B * p.H * p.Lq * p.dmw;
  const uint32_t hkey = mmfd_hash_key(*p.seed, p.salt);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / p.dmw, w = i - row * p.dmw;  // row = bh * Lq + q
    uint32_t bits = 0;
    for (int j = 0; j < 32; j += 2) {  // one hash per key pair (k even, k + 1)
      const int64_t k = w * 32 + j;
      if (k >= p.Lk) break;
      const uint32_t hsh = attn_hash64(hkey, p, row, k);
      if (pair_keep(hsh, 0, p.thr16)) bits |= 1u << j;
      if (k + 1 < p.Lk && pair_keep(hsh, 1, p.thr16)) bits |= 1u << (j + 1);
    }
    p.dm[i] = bits;
  }
}

}  // namespace
