// The fp32 split-operand ("x6") attention kernels: forward, dK/dV and dQ on three bf16 planes per
// operand, in the work split of the resident kernels (whose helpers they use).
#pragma once
#include "attn_resident.h"

namespace {

// --------------------------------------------------------------------------------------------
// fp32 attention on split bf16 operands (the fp32 step's attention; mmfd_set_fp32_attn_mode)
// --------------------------------------------------------------------------------------------
// gfx950 has no xf32 MFMA and its fp32 MFMA runs at 1/16 of the bf16 rate. As in gemm256_x6f,
// every fp32 operand is split into three bf16 planes x = hi + mid + lo (the split3 rule; 24
// significand bits, all of x) and each product accumulates the six plane products
//   mid*mid, hi*lo, lo*hi, hi*mid, mid*hi, hi*hi
// on v_mfma_f32_16x16x32_bf16 into fp32 (bf16 x bf16 products are exact; the dropped mid*lo,
// lo*mid, lo*lo are below 2^-24 relative): 6 x 16 cycles per 16x16x32 fp32 product against
// 8 x 32 for the fp32 MFMA. Operands resident in LDS (K/V, or Q/dO) are split while they are
// staged (one fp32 read from HBM, three bf16 plane images of 128-B rows, the bf16 D = 64 swizzle
// that serves both the row and the ds_read_b64_tr_b16 transposed reads); the per-wave register
// operands (the wave's own 16 queries or keys) are split once per block, and the softmax-side
// operands (P, dS) are split in registers right before their products.
//
// Geometry (D = 64 images; any D <= 64 with D % 8 == 0, the zero columns skipped by uniform
// branches): one 8-wave workgroup per (b, h) as the v2 kernels. Two tensors x three planes x
// L16 rows x 128 B must fit the 160-KB LDS: L16 = L padded to 16 rows <= 208 (BERT L = 128, ViT
// L = 197). Rows are padded to 16, not to the 32-row k-chunk: the last chunk of a 16-row remainder
// runs its h = 1 half on a repeat of its h = 0 rows (h1off = 0) against operands that are zero.

// Diagnostic build only (-DMMFD_X6A_STAMPS, tools/x6a_stamps.py): s_memtime per wave at the phase
// boundaries of the split-operand forward into a buffer no computation reads.
#ifdef MMFD_X6A_STAMPS
__device__ uint64_t x6a_stamps[8192 * 8 * 16];
#define X6A_STAMP(k)                                                                               \
  do {                                                                                             \
    const uint64_t t__ = __builtin_amdgcn_s_memtime();                                             \
    if (lane == 0 && blockIdx.x < 8192) x6a_stamps[((int64_t)blockIdx.x * 8 + wave) * 16 + (k)] = t__; \
  } while (0)
#else
#define X6A_STAMP(k) do { } while (0)
#endif
constexpr int X6A_LMAX = 208;
constexpr int X6A_RB = 128;  // bytes per plane row (64 bf16)
constexpr int X6A_LDS = 6 * X6A_LMAX * X6A_RB + 3 * X6A_LMAX * 4;
// Dynamic LDS, as the kernels carve their smem (rows padded to 16): the forward and dQ hold the three
// planes of K and of V and the per-key bias floats (their maximum: X6A_LDS); dK/dV holds the planes
// of Q and of dO, lse and delta per query, the per-key bias, and dm_words keep-bitmask words per
// query row when it stages them (DKD == 2; its maximum: all of the LDS)
constexpr int X6A_LDS_MAX = 160 * 1024;
constexpr int x6_kv_lds(int lk16) { return 6 * lk16 * X6A_RB + lk16 * 4; }
constexpr int x6_dkdv_lds(int lq16, int lk16, int dm_words) {
  return 6 * lq16 * X6A_RB + (2 * lq16 + lk16) * 4 + lq16 * dm_words * 4;
}

__device__ __forceinline__ void split8(const float* x, uint4& hi, uint4& mid, uint4& lo) {
  bf16x8 h, m, l;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const bf16 hu = (bf16)x[u];
    const float r = x[u] - (float)hu;
    const bf16 mu = (bf16)r;
    h[u] = hu;
    m[u] = mu;
    l[u] = (bf16)(r - (float)mu);
  }
  hi = __builtin_bit_cast(uint4, h);
  mid = __builtin_bit_cast(uint4, m);
  lo = __builtin_bit_cast(uint4, l);
}

// acc += (a0 + a1 + a2) (b0 + b1 + b2) over one 32-deep chunk, planes 0/1/2 = hi/mid/lo, small first
__device__ __forceinline__ void mma6(f32x4& acc, const uint4& ah, const uint4& am, const uint4& al, const uint4& bh,
                                     const uint4& bm, const uint4& bl) {
  Mma<bf16>::run(acc, am, bm);
  Mma<bf16>::run(acc, ah, bl);
  Mma<bf16>::run(acc, al, bh);
  Mma<bf16>::run(acc, ah, bm);
  Mma<bf16>::run(acc, am, bh);
  Mma<bf16>::run(acc, ah, bh);
}

// the planes of 16x16 fp32 accumulators (rows in split order) as the A fragment of one 32-key chunk
__device__ __forceinline__ void split_acc(const f32x4& a, const f32x4& b, uint4& hi, uint4& mid, uint4& lo) {
  const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  split8(x, hi, mid, lo);
}

// one fp32 row's MFMA fragments (lane: elements (kc*4 + g)*8 .. +7): loaded raw, split into planes
// f[plane][kc] later (the loads of the next block issue before the current block's products)
template <int KCH> struct X6Row { float4 v[KCH][2]; };
template <int KCH>
__device__ __forceinline__ void x6_row_load(X6Row<KCH>& x, const float* __restrict__ base, int64_t st, int64_t row,
                                            int64_t nrows, int lane, int dreal) {
  const int g = lane >> 4;
#pragma unroll
  for (int kc = 0; kc < KCH; ++kc) {
    const int col = (kc * 4 + g) * 8;
    x.v[kc][0] = x.v[kc][1] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nrows && col < dreal) {
      const float* src = base + row * st + col;
      x.v[kc][0] = *reinterpret_cast<const float4*>(src);
      x.v[kc][1] = *reinterpret_cast<const float4*>(src + 4);
    }
  }
}
template <int KCH>
__device__ __forceinline__ void x6_row_split(uint4 (&f)[3][KCH], const X6Row<KCH>& x) {
#pragma unroll
  for (int kc = 0; kc < KCH; ++kc) {
    const float4 a = x.v[kc][0], b = x.v[kc][1];
    const float e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    split8(e, f[0][kc], f[1][kc], f[2][kc]);
  }
}

// stage two fp32 head slices (rows [0, nrows), zero rows up to nrows_pad) as three plane images
// each: every load of the thread is issued before the first split, so the HBM latency is paid once
// per workgroup rather than once per 16-B chunk (the one-chunk-at-a-time loop took ~16k cycles
// for a 197-row K|V pair, 26 % of the ViT forward workgroup)
template <int D, int NTH>
__device__ __forceinline__ void x6_stage2(char* img_a, const float* __restrict__ base_a, int64_t st_a, char* img_b,
                                          const float* __restrict__ base_b, int64_t st_b, int img, int64_t nrows,
                                          int nrows_pad, int tid, int dreal, int dbg) {
  constexpr int NC = D / 8;
  constexpr int MAXT = (X6A_LMAX * NC + NTH - 1) / NTH;
  const int total = nrows_pad * NC;
  float4 xa[MAXT][2], xb[MAXT][2];
#pragma unroll
  for (int j = 0; j < MAXT; ++j) {
    const int c = tid + j * NTH;
    const int r = c / NC, ch = c % NC;
    xa[j][0] = xa[j][1] = xb[j][0] = xb[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < total && r < nrows && ch * 8 < dreal && !(dbg & 1)) {
      const float* sa = base_a + (int64_t)r * st_a + ch * 8;
      const float* sb = base_b + (int64_t)r * st_b + ch * 8;
      xa[j][0] = *reinterpret_cast<const float4*>(sa);
      xa[j][1] = *reinterpret_cast<const float4*>(sa + 4);
      xb[j][0] = *reinterpret_cast<const float4*>(sb);
      xb[j][1] = *reinterpret_cast<const float4*>(sb + 4);
    }
  }
#pragma unroll
  for (int j = 0; j < MAXT; ++j) {
    const int c = tid + j * NTH;
    if (c < total) {
      const int r = c / NC, ch = c % NC;
      const int off = row_off<bf16, 64>(r, ch);
      uint4 h, m, l;
      {
        const float e[8] = {xa[j][0].x, xa[j][0].y, xa[j][0].z, xa[j][0].w, xa[j][1].x, xa[j][1].y, xa[j][1].z, xa[j][1].w};
        split8(e, h, m, l);
        *reinterpret_cast<uint4*>(img_a + off) = h;
        *reinterpret_cast<uint4*>(img_a + img + off) = m;
        *reinterpret_cast<uint4*>(img_a + 2 * img + off) = l;
      }
      {
        const float e[8] = {xb[j][0].x, xb[j][0].y, xb[j][0].z, xb[j][0].w, xb[j][1].x, xb[j][1].y, xb[j][1].z, xb[j][1].w};
        split8(e, h, m, l);
        *reinterpret_cast<uint4*>(img_b + off) = h;
        *reinterpret_cast<uint4*>(img_b + img + off) = m;
        *reinterpret_cast<uint4*>(img_b + 2 * img + off) = l;
      }
    }
  }
}

// transposed B fragment of one 32-row chunk c (rows in split order) from a plane image; h1off =
// byte distance of the chunk's second 16 rows (16 * 128, or 0 to repeat the first half)
__device__ __forceinline__ uint4 x6_tr_frag(const char* lds, int c, int dsub, int lane, int h1off) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2;
  const int u = dsub * 4 + (i & 3);
  const int r = c * 32 + 4 * g + q;
  const int off = r * X6A_RB + (((u >> 1) ^ (r & 7)) << 4) + ((u & 1) << 3);
  const uint2 x0 = lds_read_tr16(lds + off);
  const uint2 x1 = lds_read_tr16(lds + off + h1off);
  return make_uint4(x0.x, x0.y, x1.x, x1.y);
}

__device__ __forceinline__ void x6_row_frag3(uint4* f, const char* lds, int img, int sub, int kc, int lane) {
  f[0] = row_frag<bf16, 64>(lds, sub, kc, lane);
  f[1] = row_frag<bf16, 64>(lds + img, sub, kc, lane);
  f[2] = row_frag<bf16, 64>(lds + 2 * img, sub, kc, lane);
}
__device__ __forceinline__ void x6_tr_frag3(uint4* f, const char* lds, int img, int c, int d, int lane, int h1off) {
  f[0] = x6_tr_frag(lds, c, d, lane, h1off);
  f[1] = x6_tr_frag(lds + img, c, d, lane, h1off);
  f[2] = x6_tr_frag(lds + 2 * img, c, d, lane, h1off);
}

// Every product phase below is software pipelined by hand: the fragments of step i + 1 are read
// (into the other half of a two-deep register buffer) before step i's six MFMAs issue, and the
// first step of the phase after the softmax is read before the softmax's vector work, so LDS
// latency hides behind MFMAs instead of stalling each group of six (the compiler-scheduled form
// read and waited per group: ViT forward 732 us).

template <int D, bool DROP>
__global__ void __launch_bounds__(V2_THREADS, 1) attn_fwd_x6_kernel(AttnP p) {
  // K/V planes of the head resident; each wave sweeps 16-query blocks with the v2 online softmax
  constexpr int KCH = D / 32, DT = D / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
  X6A_STAMP(0);
  const int lk16 = v2_pad(p.Lk, 16);
  const int img = lk16 * X6A_RB;
  char* k_img = smem;
  char* v_img = smem + 3 * img;
  float* kbias = reinterpret_cast<float*>(smem + 6 * img);
  const float* qb = reinterpret_cast<const float*>(p.q) + b * p.q_sb + h * p.D;
  X6Row<KCH> qn;  // the wave's next query block, raw (one block ahead)
  x6_row_load<KCH>(qn, qb, p.q_st, (int64_t)wave * 16 + li, p.Lq, lane, p.D);
  x6_stage2<D, V2_THREADS>(k_img, reinterpret_cast<const float*>(p.k) + b * p.k_sb + h * p.D, p.k_st, v_img,
                           reinterpret_cast<const float*>(p.v) + b * p.v_sb + h * p.D, p.v_st, img, p.Lk, lk16, tid,
                           p.D, p.dbg);
  stage_kbias<V2_THREADS>(kbias, p, b, lk16, tid);
  __syncthreads();
  X6A_STAMP(1);
  const uint64_t seed = DROP ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);
  const float c2 = p.scale * LOG2E;
  float* ob = reinterpret_cast<float*>(p.o) + b * p.o_sb + h * p.D;
  const int nqb = (int)((p.Lq + 15) / 16);
  // one query block over the 64-key chunks [c0, c1) (online softmax state o, m, lsum)
  const int nfc = lk16 / 64;                       // full 64-key chunks
  const int nchk = nfc + ((lk16 & 63) ? 1 : 0);    // + the padded tail chunk
  auto qrun = [&](int qbk, const uint4 (&qf)[3][KCH], int c0, int c1, f32x4 (&o)[DT], float& m, float& lsum) {
    const int64_t q0 = (int64_t)qbk * 16, myq = q0 + li;
    const uint64_t hrow = (uint64_t)(bh * p.Lq + myq) * (uint64_t)p.kp;  // pair-index base of this query row
    const uint32_t rowc1 = ((uint32_t)hrow + (uint32_t)(2 * g)) * HASH_C1;
    auto chunk = [&](int k0, auto nsc) {
      constexpr int NS = decltype(nsc)::value;  // 16-key subtiles present (4 but in the last chunk)
      constexpr int NC = (NS + 1) / 2;           // 32-key chunks of P V
      const char* kc_img = k_img + k0 * X6A_RB;
      const char* vc_img = v_img + k0 * X6A_RB;
      f32x4 s[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s[ks] = f32x4{0.f, 0.f, 0.f, 0.f};
      {  // S^T = K Q^T, steps (kc, ks)
        constexpr int N = KCH * NS;
        uint4 f[2][3];
        x6_row_frag3(f[0], kc_img, img, 0, 0, lane);
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (i + 1 < N) x6_row_frag3(f[(i + 1) & 1], kc_img, img, (i + 1) % NS, (i + 1) / NS, lane);
          const int kc = i / NS, ks = i % NS;
          mma6(s[ks], f[i & 1][0], f[i & 1][1], f[i & 1][2], qf[0][kc], qf[1][kc], qf[2][kc]);
        }
      }
      // P V steps (c, d); an odd last subtile pairs with zero P (s[NS] stays 0) over repeated V rows
      constexpr int NV = NC * DT;
      auto ld_v = [&](int i, uint4* f) {
        const int c = i / DT, d = i % DT;
        x6_tr_frag3(f, vc_img, img, c, d, lane, (2 * c + 1 < NS) ? 16 * X6A_RB : 0);
      };
      uint4 vf[2][3];
      ld_v(0, vf[0]);
      float mx = -INFINITY;
#pragma unroll
      for (int ks = 0; ks < NS; ++ks) {
        const float4 kb4 = *reinterpret_cast<const float4*>(kbias + k0 + ks * 16 + 4 * g);
        const float kb[4] = {kb4.x, kb4.y, kb4.z, kb4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t = fmaf(s[ks][r], c2, kb[r]);
          s[ks][r] = t;
          mx = fmaxf(mx, t);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(m, mx);
      const float alpha = __builtin_amdgcn_exp2f(m - mnew);
      float rs = 0.f;
#pragma unroll
      for (int ks = 0; ks < NS; ++ks) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(s[ks][r] - mnew);
          rs += e;
          s[ks][r] = e;
        }
      }
      if constexpr (DROP) {
        const uint32_t cc = rowc1 + (uint32_t)(k0 >> 1) * HASH_C1;
        uint32_t kbits = 0;
#pragma unroll
        for (int ks = 0; ks < NS; ++ks) {
          const uint32_t h0 = hash_c1(hkey, cc + (uint32_t)(ks * 8) * HASH_C1);
          const uint32_t h1 = hash_c1(hkey, cc + (uint32_t)(ks * 8 + 1) * HASH_C1);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool kp = pair_keep(r < 2 ? h0 : h1, r & 1, p.thr16);
            s[ks][r] = kp ? s[ks][r] * p.keep_scale : 0.f;
            kbits |= (uint32_t)kp << (ks * 4 + r);
          }
        }
        if (p.dm) dm_write64(p, bh, myq, k0, g, kbits);  // the backward kernels read it
      }
      lsum = lsum * alpha + rs;
      m = mnew;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ar = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
        for (int d = 0; d < DT; ++d) o[d][r] *= ar;
      }
      uint4 pp[NC][3];
#pragma unroll
      for (int c = 0; c < NC; ++c) split_acc(s[2 * c], s[2 * c + 1], pp[c][0], pp[c][1], pp[c][2]);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (i + 1 < NV) ld_v(i + 1, vf[(i + 1) & 1]);
        const int c = i / DT, d = i % DT;
        mma6(o[d], pp[c][0], pp[c][1], pp[c][2], vf[i & 1][0], vf[i & 1][1], vf[i & 1][2]);
      }
    };
    const int ce = c1 < nfc ? c1 : nfc;
    for (int c = c0; c < ce; ++c) chunk(c * 64, std::integral_constant<int, 4>{});
    if (c1 > nfc) {
      const int k0 = nfc * 64;
      switch ((lk16 - k0) >> 4) {
        case 1: chunk(k0, std::integral_constant<int, 1>{}); break;
        case 2: chunk(k0, std::integral_constant<int, 2>{}); break;
        case 3: chunk(k0, std::integral_constant<int, 3>{}); break;
        default: break;
      }
    }
  };
  // normalise and store one query block (lsum already summed over the four lane groups)
  auto qfin = [&](int qbk, const f32x4 (&o)[DT], float m, float lsum) {
    const int64_t q0 = (int64_t)qbk * 16, myq = q0 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float lr = __shfl(lsum, 4 * g + r, 64);
      const int64_t q = q0 + 4 * g + r;
      const float inv = 1.0f / lr;
      if (q < p.Lq) {
#pragma unroll
        for (int d = 0; d < DT; ++d)
          if (d * 16 + li < p.D) {
            const float val = o[d][r] * inv;
            ob[q * p.o_st + d * 16 + li] = val;
            if (p.pl) plane_put(p, ob + q * p.o_st + d * 16 + li, val);
          }
      }
    }
    if (g == 0 && myq < p.Lq) p.lse[bh * p.Lq + myq] = (m + log2f(lsum)) * LN2;
  };
  if (p.dbg & 2) return;
  // the last query block halved over the key chunks between two SIMD pairs when the blocks do not
  // spread evenly (ViT: 13 blocks), as in dK/dV; the halves' softmax states merge in LDS
  const int R = nqb - V2_THREADS / 64;
  const bool split = R >= 1 && R <= V2_THREADS / 64 && (R & 3) == 1 && nchk >= 2;
  const int nwhole = split ? nqb - 1 : nqb;
  for (int qbk = wave; qbk < nwhole; qbk += V2_THREADS / 64) {
    uint4 qf[3][KCH];
    x6_row_split<KCH>(qf, qn);
    if (qbk + V2_THREADS / 64 < nwhole)
      x6_row_load<KCH>(qn, qb, p.q_st, (int64_t)(qbk + V2_THREADS / 64) * 16 + li, p.Lq, lane, p.D);
    if (qbk == wave) X6A_STAMP(2);
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    qrun(qbk, qf, 0, nchk, o, m, lsum);
    if (qbk == wave) X6A_STAMP(7);
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    qfin(qbk, o, m, lsum);
    if (qbk == wave) X6A_STAMP(8);
  }
  if (split) {
    const int sb = nqb - 1, hc = nchk / 2;
    const bool own = wave == R - 1, part = wave == R;
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (own || part) {
      X6Row<KCH> qr;
      x6_row_load<KCH>(qr, qb, p.q_st, (int64_t)sb * 16 + li, p.Lq, lane, p.D);
      uint4 qf[3][KCH];
      x6_row_split<KCH>(qf, qr);
      qrun(sb, qf, own ? 0 : hc, own ? hc : nchk, o, m, lsum);
      lsum += __shfl_xor(lsum, 16, 64);
      lsum += __shfl_xor(lsum, 32, 64);
    }
    __syncthreads();  // every wave is done with the K / V images: reuse them for the exchange
    f32x4* xo = reinterpret_cast<f32x4*>(smem);
    float* xm = reinterpret_cast<float*>(smem + DT * 64 * 16);
    if (part) {
#pragma unroll
      for (int d = 0; d < DT; ++d) xo[d * 64 + lane] = o[d];
      xm[lane] = m;
      xm[64 + lane] = lsum;
    }
    __syncthreads();
    if (own) {  // merge: m = max, each half's sums rescaled by exp2(m_half - m)
      const float mb = xm[lane], lb = xm[64 + lane];
      const float mm = fmaxf(m, mb);
      const float aa = __builtin_amdgcn_exp2f(m - mm), ab = __builtin_amdgcn_exp2f(mb - mm);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ra = __shfl(aa, 4 * g + r, 64), rb = __shfl(ab, 4 * g + r, 64);
#pragma unroll
        for (int d = 0; d < DT; ++d) o[d][r] = o[d][r] * ra + xo[d * 64 + lane][r] * rb;
      }
      qfin(sb, o, mm, lsum * aa + lb * ab);
    }
  }
  X6A_STAMP(9);
}

// DROP (dK/dV, dQ): 0 = none, 1 = re-hash the forward's mask, 2 = read the forward's keep-bitmask
template <int D, int DROP>
__global__ void __launch_bounds__(V2_THREADS, 1) attn_dkdv_x6_kernel(AttnP p) {
  // Q/dO planes of the head resident (+ lse, delta, key bias); each wave owns 16 keys
  constexpr int KCH = D / 32, DT = D / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
  const int lq16 = v2_pad(p.Lq, 16), lk16 = v2_pad(p.Lk, 16);
  const int img = lq16 * X6A_RB;
  char* q_img = smem;
  char* do_img = smem + 3 * img;
  float* s_lse = reinterpret_cast<float*>(smem + 6 * img);
  float* s_delta = s_lse + lq16;
  float* kbias = s_delta + lq16;
  uint32_t* s_dm = reinterpret_cast<uint32_t*>(kbias + lk16);  // DROP == 2: the head's keep-bitmask rows
  const float* kb = reinterpret_cast<const float*>(p.k) + b * p.k_sb + h * p.D;
  const float* vb = reinterpret_cast<const float*>(p.v) + b * p.v_sb + h * p.D;
  if constexpr (DROP == 2) {
    const uint32_t* src = dm_row(p, bh, 0);
    const int nw = (int)p.Lq * p.dmw;
    for (int i = tid; i < lq16 * p.dmw; i += V2_THREADS) s_dm[i] = i < nw ? src[i] : 0u;
  }
  X6Row<KCH> kn, vn;  // the wave's first key block, raw (loaded with the staging)
  x6_row_load<KCH>(kn, kb, p.k_st, (int64_t)wave * 16 + li, p.Lk, lane, p.D);
  x6_row_load<KCH>(vn, vb, p.v_st, (int64_t)wave * 16 + li, p.Lk, lane, p.D);
  x6_stage2<D, V2_THREADS>(q_img, reinterpret_cast<const float*>(p.q) + b * p.q_sb + h * p.D, p.q_st, do_img,
                           reinterpret_cast<const float*>(p.dout) + b * p.do_sb + h * p.D, p.do_st, img, p.Lq, lq16,
                           tid, p.D, p.dbg);
  for (int i = tid; i < lq16; i += V2_THREADS) {
    s_lse[i] = i < p.Lq ? p.lse[bh * p.Lq + i] * LOG2E : INFINITY;
    s_delta[i] = i < p.Lq ? p.delta[bh * p.Lq + i] : 0.f;
  }
  stage_kbias<V2_THREADS>(kbias, p, b, lk16, tid);
  __syncthreads();
  float* dkb = reinterpret_cast<float*>(p.dk) + b * p.dk_sb + h * p.D;
  float* dvb = reinterpret_cast<float*>(p.dv) + b * p.dv_sb + h * p.D;
  const uint64_t seed = DROP ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);
  const float c2 = p.scale * LOG2E;
  const int nkb = lk16 / 16;
  // one key block; called for the first block on the rows loaded with the staging and then on
  // fresh loads (a loop over both would keep the prefetched rows live across the back edge)
  // dK / dV of one key block over the query chunks [qa, qb) into dkv (dV even, dK odd per 16-wide
  // D subtile)
  auto kblock = [&](int kbk, const X6Row<KCH>& kr, const X6Row<KCH>& vr, int qa, int qb, f32x4 (&dkv)[2 * DT]) {
    const int64_t k0 = (int64_t)kbk * 16, mykey = k0 + li;
    uint4 kf[3][KCH], vf[3][KCH];
    x6_row_split<KCH>(kf, kr);
    x6_row_split<KCH>(vf, vr);
    const float kb2 = kbias[mykey];  // -inf for padded keys -> P = 0
    const uint64_t hcol = (uint64_t)(bh * p.Lq) * (uint64_t)p.kp + (uint64_t)(mykey >> 1);  // pair index, query 0
    const int kodd = (int)(mykey & 1);
    const uint32_t kpc1 = (uint32_t)p.kp * HASH_C1;
    const uint32_t colc1 = (uint32_t)hcol * HASH_C1 + (uint32_t)(4 * g + 2 * kodd) * kpc1;
    auto chunk = [&](int qc, auto nsc) {
      constexpr int NS = decltype(nsc)::value;  // 16-query subtiles of this 32-query chunk
      f32x4 sd[4];  // S (even) and dP (odd) per subtile
#pragma unroll
      for (int i = 0; i < 4; ++i) sd[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      {  // S = Q K^T and dP = dO V^T, steps (kc, h2)
        constexpr int N = KCH * NS;
        uint4 f[2][6];
        auto ld = [&](int i, uint4* fr) {
          const int sub = 2 * qc + i % NS, kc = i / NS;
          x6_row_frag3(fr, q_img, img, sub, kc, lane);
          x6_row_frag3(fr + 3, do_img, img, sub, kc, lane);
        };
        ld(0, f[0]);
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (i + 1 < N) ld(i + 1, f[(i + 1) & 1]);
          const int kc = i / NS, h2 = i % NS;
          const uint4* fr = f[i & 1];
          mma6(sd[2 * h2], fr[0], fr[1], fr[2], kf[0][kc], kf[1][kc], kf[2][kc]);
          mma6(sd[2 * h2 + 1], fr[3], fr[4], fr[5], vf[0][kc], vf[1][kc], vf[2][kc]);
        }
      }
      constexpr int h1off = NS == 2 ? 16 * X6A_RB : 0;
      uint4 tb[2][6];  // transposed dO / Q planes of one D subtile (B operands of dV / dK)
      auto ldt = [&](int d, uint4* fr) {
        x6_tr_frag3(fr, do_img, img, qc, d, lane, h1off);
        x6_tr_frag3(fr + 3, q_img, img, qc, d, lane, h1off);
      };
      ldt(0, tb[0]);
      f32x4 pd[2], ds[2];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) { pd[h2] = f32x4{0.f, 0.f, 0.f, 0.f}; ds[h2] = pd[h2]; }
      float z[NS][4];
#pragma unroll
      for (int h2 = 0; h2 < NS; ++h2)
#pragma unroll
        for (int r = 0; r < 4; ++r) z[h2][r] = 1.f;
      if constexpr (DROP == 1) {  // the element index advances by Lk per query
#pragma unroll
        for (int h2 = 0; h2 < NS; ++h2) {
          const uint32_t e = colc1 + (uint32_t)((2 * qc + h2) * 16) * kpc1;
          keep4_col(hash_c1(hkey, e), hash_c1(hkey, e + kpc1), kodd, p, z[h2]);
        }
      } else if constexpr (DROP == 2) {  // bit mykey of the query rows' words (LDS broadcast reads)
        const uint32_t* col = s_dm + (mykey >> 5);
        const int sh = (int)(mykey & 31);
#pragma unroll
        for (int h2 = 0; h2 < NS; ++h2)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            z[h2][r] = ((col[((2 * qc + h2) * 16 + 4 * g + r) * p.dmw] >> sh) & 1u) ? p.keep_scale : 0.f;
      }
#pragma unroll
      for (int h2 = 0; h2 < NS; ++h2) {
        const int qs = 2 * qc + h2;
        const f32x4 sv = sd[2 * h2], dp = sd[2 * h2 + 1];
        const float4 l4 = *reinterpret_cast<const float4*>(s_lse + qs * 16 + 4 * g);
        const float4 d4 = *reinterpret_cast<const float4*>(s_delta + qs * 16 + 4 * g);
        const float lq2[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = __builtin_amdgcn_exp2f(fmaf(sv[r], c2, kb2) - lq2[r]);
          pd[h2][r] = pr * z[h2][r];
          ds[h2][r] = pr * (dp[r] * z[h2][r] - dl[r]);
        }
      }
      uint4 ph, pm, pl, sh, sm, sl;
      split_acc(pd[0], pd[1], ph, pm, pl);
      split_acc(ds[0], ds[1], sh, sm, sl);
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        if (d + 1 < DT) ldt(d + 1, tb[(d + 1) & 1]);
        const uint4* fr = tb[d & 1];
        mma6(dkv[2 * d], ph, pm, pl, fr[0], fr[1], fr[2]);
        mma6(dkv[2 * d + 1], sh, sm, sl, fr[3], fr[4], fr[5]);
      }
    };
    const int nfull = lq16 / 32;
    const int qe = qb < nfull ? qb : nfull;
    for (int qc = qa; qc < qe; ++qc) chunk(qc, std::integral_constant<int, 2>{});
    if (qb > nfull) chunk(nfull, std::integral_constant<int, 1>{});
  };
  auto kstore = [&](int kbk, const f32x4 (&dkv)[2 * DT]) {
    const int64_t k0 = (int64_t)kbk * 16;
    if (p.vst) {  // (uniform) quad transposes, then 4-column stores
      const int t = li & 3, c4 = 4 * (li >> 2);
      const int64_t key = k0 + 4 * g + t;
      float* krow = dkb + key * p.dk_st + c4;
      float* vrow = dvb + key * p.dv_st + c4;
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        float xk[4] = {dkv[2 * d + 1][0] * p.scale, dkv[2 * d + 1][1] * p.scale, dkv[2 * d + 1][2] * p.scale,
                       dkv[2 * d + 1][3] * p.scale};
        float xv[4] = {dkv[2 * d][0], dkv[2 * d][1], dkv[2 * d][2], dkv[2 * d][3]};
        quad_tr(xk, t);
        quad_tr(xv, t);
        if (key < p.Lk && d * 16 + c4 < p.D) {
          x6_put4(p, krow + d * 16, xk, p.acc_dkv);
          x6_put4(p, vrow + d * 16, xv, p.acc_dkv);
        }
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t key = k0 + 4 * g + r;
      if (key < p.Lk) {
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (d * 16 + li >= p.D) continue;
          float* pk = dkb + key * p.dk_st + d * 16 + li;
          float* pv = dvb + key * p.dv_st + d * 16 + li;
          float vk = dkv[2 * d + 1][r] * p.scale, vv = dkv[2 * d][r];
          if (p.acc_dkv) { vk += *pk; vv += *pv; }
          if (p.pl) {
            plane_put(p, pk, vk);
            plane_put(p, pv, vv);
            if (p.pl_only) continue;
          }
          *pk = vk;
          *pv = vv;
        }
      }
    }
  };
  if (p.dbg & 2) return;
  // 8 waves share the key blocks round robin; waves w and w + 4 share a SIMD, so with R = nkb - 8
  // extra blocks and R % 4 == 1 (ViT: 13 blocks) one SIMD pair would carry one block more than the
  // others. The last block is then halved over the query chunks between waves R - 1 and R (two
  // SIMD pairs), whose partial sums meet in LDS once every wave is done with the Q / dO images.
  const int nch = lq16 / 32 + ((lq16 & 16) ? 1 : 0);
  const int R = nkb - V2_THREADS / 64;
  const bool split = R >= 1 && R <= V2_THREADS / 64 && (R & 3) == 1 && nch >= 2;
  const int nwhole = split ? nkb - 1 : nkb;
  if (wave < nwhole) {
    f32x4 dkv[2 * DT];
#pragma unroll
    for (int i = 0; i < 2 * DT; ++i) dkv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    kblock(wave, kn, vn, 0, nch, dkv);
    kstore(wave, dkv);
  }
  for (int kbk = wave + V2_THREADS / 64; kbk < nwhole; kbk += V2_THREADS / 64) {
    X6Row<KCH> kr, vr;
    x6_row_load<KCH>(kr, kb, p.k_st, (int64_t)kbk * 16 + li, p.Lk, lane, p.D);
    x6_row_load<KCH>(vr, vb, p.v_st, (int64_t)kbk * 16 + li, p.Lk, lane, p.D);
    f32x4 dkv[2 * DT];
#pragma unroll
    for (int i = 0; i < 2 * DT; ++i) dkv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    kblock(kbk, kr, vr, 0, nch, dkv);
    kstore(kbk, dkv);
  }
  if (split) {
    const int sb = nkb - 1, hc = nch / 2;
    const bool own = wave == R - 1, part = wave == R;
    f32x4 dkv[2 * DT];
#pragma unroll
    for (int i = 0; i < 2 * DT; ++i) dkv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (own || part) {
      X6Row<KCH> kr, vr;
      x6_row_load<KCH>(kr, kb, p.k_st, (int64_t)sb * 16 + li, p.Lk, lane, p.D);
      x6_row_load<KCH>(vr, vb, p.v_st, (int64_t)sb * 16 + li, p.Lk, lane, p.D);
      kblock(sb, kr, vr, own ? 0 : hc, own ? hc : nch, dkv);
    }
    __syncthreads();  // every wave is done with the Q / dO images: reuse them for the exchange
    f32x4* xch = reinterpret_cast<f32x4*>(smem);
    if (part) {
#pragma unroll
      for (int i = 0; i < 2 * DT; ++i) xch[i * 64 + lane] = dkv[i];
    }
    __syncthreads();
    if (own) {
#pragma unroll
      for (int i = 0; i < 2 * DT; ++i) dkv[i] += xch[i * 64 + lane];
      kstore(sb, dkv);
    }
  }
}

template <int D, int DROP>
__global__ void __launch_bounds__(V2_THREADS, 1) attn_dq_x6_kernel(AttnP p) {
  // K/V planes of the head resident; each wave owns 16 queries: dQ = dS K
  constexpr int KCH = D / 32, DT = D / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
  const int lk16 = v2_pad(p.Lk, 16);
  const int img = lk16 * X6A_RB;
  char* k_img = smem;
  char* v_img = smem + 3 * img;
  float* kbias = reinterpret_cast<float*>(smem + 6 * img);
  const float* qb = reinterpret_cast<const float*>(p.q) + b * p.q_sb + h * p.D;
  const float* dob = reinterpret_cast<const float*>(p.dout) + b * p.do_sb + h * p.D;
  const float* obp = reinterpret_cast<const float*>(p.o) + b * p.o_sb + h * p.D;
  X6Row<KCH> qn, don, on;  // the wave's first query block, raw (loaded with the staging)
  x6_row_load<KCH>(qn, qb, p.q_st, (int64_t)wave * 16 + li, p.Lq, lane, p.D);
  x6_row_load<KCH>(don, dob, p.do_st, (int64_t)wave * 16 + li, p.Lq, lane, p.D);
  x6_row_load<KCH>(on, obp, p.o_st, (int64_t)wave * 16 + li, p.Lq, lane, p.D);
  x6_stage2<D, V2_THREADS>(k_img, reinterpret_cast<const float*>(p.k) + b * p.k_sb + h * p.D, p.k_st, v_img,
                           reinterpret_cast<const float*>(p.v) + b * p.v_sb + h * p.D, p.v_st, img, p.Lk, lk16, tid,
                           p.D, p.dbg);
  stage_kbias<V2_THREADS>(kbias, p, b, lk16, tid);
  __syncthreads();
  float* dqb = reinterpret_cast<float*>(p.dq) + b * p.dq_sb + h * p.D;
  const uint64_t seed = DROP ? *p.seed : 0ull;
  const uint32_t hkey = mmfd_hash_key(seed, p.salt);
  const float c2 = p.scale * LOG2E;
  const int nqb = (int)((p.Lq + 15) / 16);
  // dQ of one query block over the key chunks [ka, kb2e) into dq (as kblock in dK/dV)
  // delta = rowsum(dO * O) of the block's queries is computed here from the rows the wave loads
  // anyway (no separate delta pass: the dQ kernel runs first and writes it for dK/dV)
  auto qblock = [&](int qbk, const X6Row<KCH>& qr, const X6Row<KCH>& dr, const X6Row<KCH>& orow, bool wdelta,
                    int ka, int kb2e, f32x4 (&dq)[DT]) {
    const int64_t q0 = (int64_t)qbk * 16, myq = q0 + li;
    uint4 qf[3][KCH], dof[3][KCH];
    x6_row_split<KCH>(qf, qr);
    x6_row_split<KCH>(dof, dr);
    const float lse2 = myq < p.Lq ? p.lse[bh * p.Lq + myq] * LOG2E : INFINITY;
    float dsum = 0.f;
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const float4 a = orow.v[kc][hh], c = dr.v[kc][hh];
        dsum = fmaf(a.x, c.x, fmaf(a.y, c.y, fmaf(a.z, c.z, fmaf(a.w, c.w, dsum))));
      }
    dsum += __shfl_xor(dsum, 16, 64);
    dsum += __shfl_xor(dsum, 32, 64);
    const float dlt = myq < p.Lq ? dsum : 0.f;
    if (wdelta && g == 0 && myq < p.Lq) p.delta[bh * p.Lq + myq] = dsum;
    const uint64_t hrow = (uint64_t)(bh * p.Lq + myq) * (uint64_t)p.kp;  // pair-index base of this query row
    const uint32_t rowc1 = ((uint32_t)hrow + (uint32_t)(2 * g)) * HASH_C1;
    const uint32_t* dmrow = DROP == 2 ? dm_row(p, bh, myq < p.Lq ? myq : 0) : nullptr;
    auto chunk = [&](int kc2, auto nsc) {
      constexpr int NS = decltype(nsc)::value;  // 16-key subtiles of this 32-key chunk
      uint32_t kw = 0;  // DROP == 2: the chunk's keep word (32 keys), loaded ahead of the products
      if constexpr (DROP == 2) kw = dmrow[kc2];
      f32x4 sd[4];  // S^T (even) and dP^T (odd) per subtile
#pragma unroll
      for (int i = 0; i < 4; ++i) sd[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      {  // S^T = K Q^T and dP^T = V dO^T, steps (kc, h2)
        constexpr int N = KCH * NS;
        uint4 f[2][6];
        auto ld = [&](int i, uint4* fr) {
          const int sub = 2 * kc2 + i % NS, kc = i / NS;
          x6_row_frag3(fr, k_img, img, sub, kc, lane);
          x6_row_frag3(fr + 3, v_img, img, sub, kc, lane);
        };
        ld(0, f[0]);
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (i + 1 < N) ld(i + 1, f[(i + 1) & 1]);
          const int kc = i / NS, h2 = i % NS;
          const uint4* fr = f[i & 1];
          mma6(sd[2 * h2], fr[0], fr[1], fr[2], qf[0][kc], qf[1][kc], qf[2][kc]);
          mma6(sd[2 * h2 + 1], fr[3], fr[4], fr[5], dof[0][kc], dof[1][kc], dof[2][kc]);
        }
      }
      constexpr int h1off = NS == 2 ? 16 * X6A_RB : 0;
      uint4 tk[2][3];  // transposed K planes of one D subtile (B operand of dQ)
      x6_tr_frag3(tk[0], k_img, img, kc2, 0, lane, h1off);
      f32x4 ds[2];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) ds[h2] = f32x4{0.f, 0.f, 0.f, 0.f};
      float z[NS][4];
#pragma unroll
      for (int h2 = 0; h2 < NS; ++h2)
#pragma unroll
        for (int r = 0; r < 4; ++r) z[h2][r] = 1.f;
      if constexpr (DROP == 1) {
#pragma unroll
        for (int h2 = 0; h2 < NS; ++h2) {
          const uint32_t e = rowc1 + (uint32_t)((2 * kc2 + h2) * 8) * HASH_C1;
          keep4_pairs(hash_c1(hkey, e), hash_c1(hkey, e + HASH_C1), p, z[h2]);
        }
      } else if constexpr (DROP == 2) {
#pragma unroll
        for (int h2 = 0; h2 < NS; ++h2)
#pragma unroll
          for (int r = 0; r < 4; ++r) z[h2][r] = ((kw >> (h2 * 16 + 4 * g + r)) & 1u) ? p.keep_scale : 0.f;
      }
#pragma unroll
      for (int h2 = 0; h2 < NS; ++h2) {
        const int ks = 2 * kc2 + h2;
        const f32x4 sv = sd[2 * h2], dp = sd[2 * h2 + 1];
        const float4 kb4 = *reinterpret_cast<const float4*>(kbias + ks * 16 + 4 * g);
        const float kbr[4] = {kb4.x, kb4.y, kb4.z, kb4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = __builtin_amdgcn_exp2f(fmaf(sv[r], c2, kbr[r]) - lse2);
          ds[h2][r] = pr * (dp[r] * z[h2][r] - dlt);
        }
      }
      uint4 sh, sm, sl;
      split_acc(ds[0], ds[1], sh, sm, sl);
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        if (d + 1 < DT) x6_tr_frag3(tk[(d + 1) & 1], k_img, img, kc2, d + 1, lane, h1off);
        const uint4* fr = tk[d & 1];
        mma6(dq[d], sh, sm, sl, fr[0], fr[1], fr[2]);
      }
    };
    const int nfull = lk16 / 32;
    const int ke = kb2e < nfull ? kb2e : nfull;
    for (int kc2 = ka; kc2 < ke; ++kc2) chunk(kc2, std::integral_constant<int, 2>{});
    if (kb2e > nfull) chunk(nfull, std::integral_constant<int, 1>{});
  };
  auto qstore = [&](int qbk, const f32x4 (&dq)[DT]) {
    const int64_t q0 = (int64_t)qbk * 16;
    if (p.vst) {  // (uniform) quad transposes, then 4-column stores
      const int t = li & 3, c4 = 4 * (li >> 2);
      const int64_t q = q0 + 4 * g + t;
      float* qrow = dqb + q * p.dq_st + c4;
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        float x[4] = {dq[d][0] * p.scale, dq[d][1] * p.scale, dq[d][2] * p.scale, dq[d][3] * p.scale};
        quad_tr(x, t);
        if (q < p.Lq && d * 16 + c4 < p.D) x6_put4(p, qrow + d * 16, x, p.acc_dq);
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t q = q0 + 4 * g + r;
      if (q < p.Lq) {
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (d * 16 + li >= p.D) continue;
          float* pq = dqb + q * p.dq_st + d * 16 + li;
          float vq = dq[d][r] * p.scale;
          if (p.acc_dq) vq += *pq;
          if (p.pl) {
            plane_put(p, pq, vq);
            if (p.pl_only) continue;
          }
          *pq = vq;
        }
      }
    }
  };
  if (p.dbg & 2) return;
  // the last query block halved over the key chunks between two SIMD pairs, as in dK/dV
  const int nch = lk16 / 32 + ((lk16 & 16) ? 1 : 0);
  const int R = nqb - V2_THREADS / 64;
  const bool split = R >= 1 && R <= V2_THREADS / 64 && (R & 3) == 1 && nch >= 2;
  const int nwhole = split ? nqb - 1 : nqb;
  if (wave < nwhole) {
    f32x4 dq[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) dq[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    qblock(wave, qn, don, on, true, 0, nch, dq);
    qstore(wave, dq);
  }
  for (int qbk = wave + V2_THREADS / 64; qbk < nwhole; qbk += V2_THREADS / 64) {
    X6Row<KCH> qr, dr, orr;
    x6_row_load<KCH>(qr, qb, p.q_st, (int64_t)qbk * 16 + li, p.Lq, lane, p.D);
    x6_row_load<KCH>(dr, dob, p.do_st, (int64_t)qbk * 16 + li, p.Lq, lane, p.D);
    x6_row_load<KCH>(orr, obp, p.o_st, (int64_t)qbk * 16 + li, p.Lq, lane, p.D);
    f32x4 dq[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) dq[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    qblock(qbk, qr, dr, orr, true, 0, nch, dq);
    qstore(qbk, dq);
  }
  if (split) {
    const int sb = nqb - 1, hc = nch / 2;
    const bool own = wave == R - 1, part = wave == R;
    f32x4 dq[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) dq[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (own || part) {
      X6Row<KCH> qr, dr, orr;
      x6_row_load<KCH>(qr, qb, p.q_st, (int64_t)sb * 16 + li, p.Lq, lane, p.D);
      x6_row_load<KCH>(dr, dob, p.do_st, (int64_t)sb * 16 + li, p.Lq, lane, p.D);
      x6_row_load<KCH>(orr, obp, p.o_st, (int64_t)sb * 16 + li, p.Lq, lane, p.D);
      qblock(sb, qr, dr, orr, own, own ? 0 : hc, own ? hc : nch, dq);
    }
    __syncthreads();  // every wave is done with the K / V images: reuse them for the exchange
    f32x4* xch = reinterpret_cast<f32x4*>(smem);
    if (part) {
#pragma unroll
      for (int d = 0; d < DT; ++d) xch[d * 64 + lane] = dq[d];
    }
    __syncthreads();
    if (own) {
#pragma unroll
      for (int d = 0; d < DT; ++d) dq[d] += xch[d * 64 + lane];
      qstore(sb, dq);
    }
  }
}
}  // namespace
