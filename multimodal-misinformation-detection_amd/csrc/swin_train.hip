// Swinv2 fine-tuning (Swinv2Config(trainable=True), train.py --train_image_encoder): the backward
// pieces the shared kernels do not have. Under grad a block's attention runs as packed QKV GEMM ->
// cosine pass on the packed rows (training form: keeps the inverse norms) -> plain attention with
// scale 1 and the block's bias, so dQ / dK / dV come from mmfd_attn_bwd; what this file adds:
//   swin_qk_norm_train   : mmfd_swin_qk_norm's arithmetic (same bits) + inv[row][q|k][h] = 1 / max(|.|, 1e-12)
//   swin_qk_norm_bwd     : adjoint of the cosine pass in place on the packed gradient rows, and the
//                          logit-scale gradient through per-block partials summed in a fixed order
//   attn_bwd_bias_sum    : dB[m][h][i][j] = sum_{b = m (mod M)} P (dP - delta), the gradient of a bias
//                          shared by the batch (M = 1) or read with rel_bias_mod = M; MFMA
//                          recomputation shaped like attn_bwd_ds_kernel inside a loop over the batch
//                          rows of one bias row, the [64 queries][Lk <= 256] tile kept in registers
//   swin_bias_bwd        : dB -> dtable through 16 sigmoid(table[rpi]) (the shift mask is a constant)
//   swin_cpb_bwd         : dtable -> dW1, db1, dW2 of the position-bias MLP
// Every kernel is deterministic: no floating-point atomics, sums in a fixed order.
// (This translation unit is separate from attention.hip on purpose: DESIGN §3.)
#include "attn_common.h"

namespace {

// sum over the 256 threads of a block, the same value in every thread; fixed order
__device__ __forceinline__ float block_sum256(float v, float* red4) {
  v = wave_sum(v);
  __syncthreads();  // red4 may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// ---------------------------------------------------------------------------------------------
// cosine pass, training form: one thread per (row, head, q|k) as swin_qk_norm_kernel
// ---------------------------------------------------------------------------------------------
template <typename T, int d>
__global__ void __launch_bounds__(256) swin_qk_norm_train_kernel(int64_t rows, int H, T* __restrict__ qkv, int64_t ld,
                                                                 const float* __restrict__ logit_scale, float max_log,
                                                                 float* __restrict__ inv) {
  constexpr int N = 16 / sizeof(T);
  const int64_t total = rows * H * 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int which = (int)(t % 2);          // 0 = q, 1 = k
  const int h = (int)((t / 2) % H);
  const int64_t row = t / (2 * H);
  T* p = qkv + row * ld + (int64_t)which * H * d + (int64_t)h * d;
  constexpr int nch = d / N;
  float v[d];
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < nch; ++c) {
    const uint4 raw = reinterpret_cast<const uint4*>(p)[c];
    const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
    for (int j = 0; j < N; ++j) { v[c * N + j] = to_f32(e[j]); ss = fmaf(v[c * N + j], v[c * N + j], ss); }
  }
  float s = 1.f / fmaxf(sqrtf(ss), 1e-12f);
  inv[(row * 2 + which) * H + h] = s;
  const float mult = which == 0 ? expf(fminf(logit_scale[h], max_log)) : 1.f;
#pragma unroll
  for (int c = 0; c < nch; ++c) {
    uint4 raw;
    T* e = reinterpret_cast<T*>(&raw);
#pragma unroll
    for (int j = 0; j < N; ++j) e[j] = from_f32<T>((v[c * N + j] * s) * mult);
    reinterpret_cast<uint4*>(p)[c] = raw;
  }
}

// With qh = q / |q|, s = exp(min(ls_h, c)), qn = s qh (the saved operand) and g = dL/dqn:
//   dq = (s / |q|) (g - qh (qh . g)) = inv (s g - qn (qn . g) / s)        |q| >= 1e-12
//   dq = (s / 1e-12) g                                                     below (F.normalize's clamp)
//   d ls_h = [ls_h <= c] sum_rows g . qn                                   (k: s = 1, no logit scale)
// part[block][h] = the block's share of sum g . qn, summed over its threads in thread order.
template <typename T, int d>
__global__ void __launch_bounds__(256) swin_qk_norm_bwd_kernel(int64_t rows, int H, T* __restrict__ dqkv, int64_t ldg,
                                                               const T* __restrict__ qkvn, int64_t ldn,
                                                               const float* __restrict__ inv,
                                                               const float* __restrict__ logit_scale, float max_log,
                                                               float* __restrict__ part) {
  constexpr int N = 16 / sizeof(T);
  constexpr int nch = d / N;
  __shared__ float gq[256];
  const int64_t total = rows * H * 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float dot = 0.f;
  if (t < total) {
    const int which = (int)(t % 2);
    const int h = (int)((t / 2) % H);
    const int64_t row = t / (2 * H);
    const int64_t col = (int64_t)which * H * d + (int64_t)h * d;
    T* pg = dqkv + row * ldg + col;
    const T* pn = qkvn + row * ldn + col;
    float g[d];
#pragma unroll
    for (int c = 0; c < nch; ++c) {
      const uint4 rg = reinterpret_cast<const uint4*>(pg)[c];
      const uint4 rn = reinterpret_cast<const uint4*>(pn)[c];
      const T* eg = reinterpret_cast<const T*>(&rg);
      const T* en = reinterpret_cast<const T*>(&rn);
#pragma unroll
      for (int j = 0; j < N; ++j) { g[c * N + j] = to_f32(eg[j]); dot = fmaf(g[c * N + j], to_f32(en[j]), dot); }
    }
    const float iv = inv[(row * 2 + which) * H + h];
    const float s = which == 0 ? expf(fminf(logit_scale[h], max_log)) : 1.f;
    const bool clamped = iv >= 1.f / 1e-12f;
    const float a = iv * s;                         // s / max(|q|, 1e-12)
    const float bq = clamped ? 0.f : iv * dot / s;  // (qn . g) / (s |q|)
#pragma unroll
    for (int c = 0; c < nch; ++c) {
      const uint4 rn = reinterpret_cast<const uint4*>(pn)[c];
      const T* en = reinterpret_cast<const T*>(&rn);
      uint4 raw;
      T* e = reinterpret_cast<T*>(&raw);
#pragma unroll
      for (int j = 0; j < N; ++j) e[j] = from_f32<T>(fmaf(-bq, to_f32(en[j]), a * g[c * N + j]));
      reinterpret_cast<uint4*>(pg)[c] = raw;
    }
    if (which != 0) dot = 0.f;
  }
  gq[threadIdx.x] = dot;
  __syncthreads();
  if ((int)threadIdx.x < H) {
    // element i of this block is (row, head, q|k) number t0 + i: q entries are the even ones
    const int64_t t0 = (int64_t)blockIdx.x * 256;
    const int h0 = (int)((t0 / 2) % H);
    float s = 0.f;
    for (int e = 0; e < 128; ++e)
      if ((h0 + e) % H == (int)threadIdx.x) s += gq[2 * e];  // (entries past `total` hold 0)
    part[(int64_t)blockIdx.x * H + threadIdx.x] = s;
  }
}

// dls[h] = [ls_h <= max_log] * sum_p part[p][h]: one block per head, strided partial sums then a tree
__global__ void __launch_bounds__(256) swin_logit_scale_reduce_kernel(int64_t nparts, int H, const float* __restrict__ part,
                                                                      const float* __restrict__ logit_scale, float max_log,
                                                                      float* __restrict__ dls) {
  __shared__ float red4[4];
  const int h = blockIdx.x;
  float s = 0.f;
  for (int64_t p = threadIdx.x; p < nparts; p += 256) s += part[p * H + h];
  s = block_sum256(s, red4);
  if (threadIdx.x == 0) dls[h] = logit_scale[h] <= max_log ? s : 0.f;
}

// ---------------------------------------------------------------------------------------------
// gradient of a batch-shared / modulo bias
// ---------------------------------------------------------------------------------------------
struct BiasSumP {
  int64_t B, H, Lq, Lk, M;
  int D;
  float scale;
  const void* q; int64_t q_sb, q_st;
  const void* k; int64_t k_sb, k_st;
  const void* v; int64_t v_sb, v_st;
  const void* dout; int64_t do_sb, do_st;
  const float* lse;
  const float* delta;
  const float* key_bias;
  const float* rel_bias; int64_t rb_sb;  // bias row m at rel_bias + m * rb_sb (0 when M = 1)
};

// below this exponent exp() is +0 in fp32 whatever the intrinsic's rounding (as attn_bwd_ds_kernel)
constexpr float BS_EXP_MIN = -104.f;

// Workgroup = 64 queries of bias row (m, h), wave = 16 queries; for every batch row b = m, m + M, ...
// the 64-key blocks of K and V go through LDS and S^T = K Q^T, dP^T = V dO^T run on MFMAs with the
// query on the lane (lse, delta lane-local; a lane holds keys 4g .. 4g+3 of each 16-key sub-block).
// NKB = ceil(Lk / 64) <= 4 key blocks: the lane's 16 * NKB terms stay in registers over the loop.
template <typename T, int D, int NKB>
__global__ void __launch_bounds__(256) attn_bwd_bias_sum_kernel(BiasSumP p, float* __restrict__ out) {
  using C = AT<T, D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_row = smem;
  char* v_row = smem + C::TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int64_t mh = blockIdx.y, m = mh / p.H, h = mh % p.H;
  const int64_t q0 = (int64_t)blockIdx.x * 64 + wave * 16;
  const int64_t myq = q0 + li;
  const bool qok = myq < p.Lq;
  const float* relrow = p.rel_bias + m * p.rb_sb + (h * p.Lq + (qok ? myq : 0)) * p.Lk;

  float acc[NKB][4][4];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[kb][ks][r] = 0.f;

  for (int64_t b = m; b < p.B; b += p.M) {
    const int64_t bh = b * p.H + h;
    const T* qb = reinterpret_cast<const T*>(p.q) + b * p.q_sb + h * p.D;
    const T* kb_ = reinterpret_cast<const T*>(p.k) + b * p.k_sb + h * p.D;
    const T* vb = reinterpret_cast<const T*>(p.v) + b * p.v_sb + h * p.D;
    const T* dob = reinterpret_cast<const T*>(p.dout) + b * p.do_sb + h * p.D;
    uint4 qf[C::KCH], dof[C::KCH];
    load_row_regs<T, D>(qf, qb, p.q_st, myq, p.Lq, lane, p.D);
    load_row_regs<T, D>(dof, dob, p.do_st, myq, p.Lq, lane, p.D);
    const float lse = qok ? p.lse[bh * p.Lq + myq] : INFINITY;
    const float dlt = qok ? p.delta[bh * p.Lq + myq] : 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const int64_t k0 = (int64_t)kb * 64;
      __syncthreads();
      stage_rows<T, D, false>(k_row, kb_, p.k_st, k0, p.Lk, tid, p.D);
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
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t key = key0 + r;
          if (qok && key < p.Lk) {
            float sc = sv[r] * p.scale + relrow[key];
            if (p.key_bias) sc += p.key_bias[b * p.Lk + key];
            const float x = sc - lse;
            const float pr = x < BS_EXP_MIN ? 0.f : __expf(x);
            acc[kb][ks][r] += pr * (dp[r] - dlt);
          }
        }
      }
    }
  }

  if (!qok) return;
  float* orow = out + (mh * p.Lq + myq) * p.Lk;  // [M][H][Lq][Lk] contiguous
  const bool vec4 = (p.Lk & 3) == 0;             // rows then start 16-B aligned (base checked by the host)
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int64_t key0 = (int64_t)kb * 64 + ks * 16 + 4 * g;
      if (key0 >= p.Lk) continue;
      if (vec4) {
        *reinterpret_cast<float4*>(orow + key0) = make_float4(acc[kb][ks][0], acc[kb][ks][1], acc[kb][ks][2], acc[kb][ks][3]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (key0 + r < p.Lk) orow[key0 + r] = acc[kb][ks][r];
      }
    }
}

template <typename T, int D>
int launch_bias_sum(const BiasSumP& p, float* out, hipStream_t s) {
  const dim3 grid((unsigned)((p.Lq + 63) / 64), (unsigned)(p.M * p.H));
  const int lds = 2 * AT<T, D>::TILE;
  const int nkb = (int)((p.Lk + 63) / 64);
#define BS(N) hipLaunchKernelGGL((attn_bwd_bias_sum_kernel<T, D, N>), grid, dim3(256), lds, s, p, out)
  if (nkb == 1) BS(1); else if (nkb == 2) BS(2); else if (nkb == 3) BS(3); else BS(4);
#undef BS
  MMFD_CHECK_LAUNCH("attn_bwd_bias_sum");
  return 0;
}

// ---------------------------------------------------------------------------------------------
// position bias: dB -> dtable -> MLP gradients
// ---------------------------------------------------------------------------------------------
// one block per (table row r, head h): the (i, j) with rpi[i][j] == r, all windows, then 16 sigmoid'
__global__ void __launch_bounds__(256) swin_bias_bwd_kernel(int64_t nW, int64_t H, int64_t LL, const float* __restrict__ db,
                                                            const float* __restrict__ table, const int32_t* __restrict__ rpi,
                                                            float* __restrict__ dtable) {
  __shared__ float red4[4];
  const int r = blockIdx.x;
  const int64_t h = blockIdx.y;
  float s = 0.f;
  for (int64_t ij = threadIdx.x; ij < LL; ij += 256) {
    if (rpi[ij] != r) continue;
    for (int64_t w = 0; w < nW; ++w) s += db[(w * H + h) * LL + ij];
  }
  s = block_sum256(s, red4);
  if (threadIdx.x == 0) {
    const float sg = 1.f / (1.f + expf(-table[(int64_t)r * H + h]));
    dtable[(int64_t)r * H + h] = 16.f * sg * (1.f - sg) * s;
  }
}

// one workgroup, thread k = hidden unit k: the hidden value is recomputed per table row (as
// swin_cpb_kernel computes it) and the three gradients accumulate in registers over the rows
__global__ void __launch_bounds__(512) swin_cpb_bwd_kernel(int T, int H, const float* __restrict__ coords,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ dtable,
                                                           float* __restrict__ dw1, float* __restrict__ db1,
                                                           float* __restrict__ dw2) {
  const int k = threadIdx.x;
  const float w10 = w1[2 * k], w11 = w1[2 * k + 1], bk = b1[k];
  float w2k[32], g2[32];
#pragma unroll
  for (int h = 0; h < 32; ++h) {
    w2k[h] = h < H ? w2[h * 512 + k] : 0.f;
    g2[h] = 0.f;
  }
  float g10 = 0.f, g11 = 0.f, gb = 0.f;
  for (int t = 0; t < T; ++t) {
    const float c0 = coords[2 * t], c1 = coords[2 * t + 1];
    const float pre = fmaf(w10, c0, fmaf(w11, c1, bk));
    const float hk = fmaxf(pre, 0.f);
    float dh = 0.f;
#pragma unroll
    for (int h = 0; h < 32; ++h) {
      if (h < H) {
        const float dt = dtable[t * H + h];
        g2[h] = fmaf(dt, hk, g2[h]);
        dh = fmaf(dt, w2k[h], dh);
      }
    }
    if (pre > 0.f) {
      g10 = fmaf(dh, c0, g10);
      g11 = fmaf(dh, c1, g11);
      gb += dh;
    }
  }
  dw1[2 * k] = g10;
  dw1[2 * k + 1] = g11;
  db1[k] = gb;
#pragma unroll
  for (int h = 0; h < 32; ++h)
    if (h < H) dw2[h * 512 + k] = g2[h];
}

}  // namespace

extern "C" int mmfd_swin_qk_norm_train(int dtype, int64_t rows, int64_t H, int64_t d, void* qkv, int64_t ld,
                                       const float* logit_scale, float max_log, float* inv_norm,
                                       mmfd_stream_t stream) {
  MMFD_CHECK_ARG(dtype == MMFD_F32 || dtype == MMFD_BF16, "swin_qk_norm_train: bad dtype");
  const int esz = dtype == MMFD_BF16 ? 2 : 4;
  MMFD_CHECK_ARG(d == 32 || d == 64, "swin_qk_norm_train: head dim %lld unsupported (32 or 64, as the backward)", (long long)d);
  MMFD_CHECK_ARG(rows >= 0 && H > 0 && ld >= 2 * H * d, "swin_qk_norm_train: bad shape");
  MMFD_CHECK_ARG(((uintptr_t)qkv & 15) == 0 && (ld * esz) % 16 == 0, "swin_qk_norm_train: 16-B aligned rows");
  MMFD_CHECK_ARG(qkv && logit_scale && inv_norm, "swin_qk_norm_train: null pointer");
  const int64_t total = rows * H * 2;
  if (total == 0) return 0;
  MMFD_CHECK_ARG((total + 255) / 256 <= 0x7fffffff, "swin_qk_norm_train: too many rows");
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
#define QKN(T, D) hipLaunchKernelGGL((swin_qk_norm_train_kernel<T, D>), grid, dim3(256), 0, s, rows, (int)H, (T*)qkv, ld, logit_scale, max_log, inv_norm)
  if (dtype == MMFD_BF16) { if (d == 32) QKN(bf16, 32); else QKN(bf16, 64); }
  else { if (d == 32) QKN(float, 32); else QKN(float, 64); }
#undef QKN
  MMFD_CHECK_LAUNCH("swin_qk_norm_train");
  return 0;
}

extern "C" int64_t mmfd_swin_qk_norm_bwd_workspace_bytes(int64_t rows, int64_t H) {
  if (rows < 0 || H <= 0) return -1;
  return ((rows * H * 2 + 255) / 256) * H * 4;
}

extern "C" int mmfd_swin_qk_norm_bwd(int dtype, int64_t rows, int64_t H, int64_t d, void* dqkv, int64_t ldg,
                                     const void* qkv_norm, int64_t ldn, const float* inv_norm,
                                     const float* logit_scale, float max_log, float* d_logit_scale, void* workspace,
                                     int64_t workspace_bytes, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(dtype == MMFD_F32 || dtype == MMFD_BF16, "swin_qk_norm_bwd: bad dtype");
  const int esz = dtype == MMFD_BF16 ? 2 : 4;
  MMFD_CHECK_ARG(d == 32 || d == 64, "swin_qk_norm_bwd: head dim %lld unsupported (32 or 64)", (long long)d);
  MMFD_CHECK_ARG(rows >= 0 && H > 0 && H <= 256 && ldg >= 2 * H * d && ldn >= 2 * H * d, "swin_qk_norm_bwd: bad shape");
  MMFD_CHECK_ARG(((uintptr_t)dqkv & 15) == 0 && (ldg * esz) % 16 == 0 && ((uintptr_t)qkv_norm & 15) == 0 &&
                     (ldn * esz) % 16 == 0, "swin_qk_norm_bwd: 16-B aligned rows");
  MMFD_CHECK_ARG(dqkv && qkv_norm && inv_norm && logit_scale && d_logit_scale, "swin_qk_norm_bwd: null pointer");
  MMFD_CHECK_ARG(dqkv != qkv_norm, "swin_qk_norm_bwd: the gradient must not alias the saved operands");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = rows * H * 2;
  const int64_t nblk = (total + 255) / 256;
  MMFD_CHECK_ARG(nblk <= 0x7fffffff, "swin_qk_norm_bwd: too many rows");
  MMFD_CHECK_ARG(nblk == 0 || (workspace && workspace_bytes >= nblk * H * 4),
                 "swin_qk_norm_bwd: workspace of %lld bytes needed", (long long)(nblk * H * 4));
  if (nblk > 0) {
    const dim3 grid((unsigned)nblk);
#define QKB(T, D) hipLaunchKernelGGL((swin_qk_norm_bwd_kernel<T, D>), grid, dim3(256), 0, s, rows, (int)H, (T*)dqkv, ldg, (const T*)qkv_norm, ldn, inv_norm, logit_scale, max_log, (float*)workspace)
    if (dtype == MMFD_BF16) { if (d == 32) QKB(bf16, 32); else QKB(bf16, 64); }
    else { if (d == 32) QKB(float, 32); else QKB(float, 64); }
#undef QKB
    MMFD_CHECK_LAUNCH("swin_qk_norm_bwd");
  }
  hipLaunchKernelGGL(swin_logit_scale_reduce_kernel, dim3((unsigned)H), dim3(256), 0, s, nblk, (int)H,
                     (const float*)workspace, logit_scale, max_log, d_logit_scale);
  MMFD_CHECK_LAUNCH("swin_qk_norm_bwd reduce");
  return 0;
}

extern "C" int mmfd_attn_bwd_bias_sum(const mmfd_attn_args* a, float* d_bias, mmfd_stream_t stream) {
  MMFD_CHECK_STRUCT(a, mmfd_attn_args, "mmfd_attn_bwd_bias_sum");
  MMFD_CHECK_ARG(a->dtype == MMFD_F32 || a->dtype == MMFD_BF16, "attn_bwd_bias_sum: bad dtype");
  MMFD_CHECK_ARG(a->D > 0 && a->D <= 64, "attn_bwd_bias_sum: head_dim %lld unsupported (<= 64)", (long long)a->D);
  MMFD_CHECK_ARG(a->B >= 0 && a->H > 0 && a->Lq >= 0 && a->Lk > 0, "attn_bwd_bias_sum: bad shape");
  MMFD_CHECK_ARG(a->Lq <= 256 && a->Lk <= 256, "attn_bwd_bias_sum: Lq = %lld, Lk = %lld not covered (<= 256)",
                 (long long)a->Lq, (long long)a->Lk);
  MMFD_CHECK_ARG(a->q && a->k && a->v && a->dout && a->lse && a->delta && d_bias, "attn_bwd_bias_sum: null pointer");
  const int epc = a->dtype == MMFD_BF16 ? 8 : 4;
  MMFD_CHECK_ARG(a->D % epc == 0, "attn_bwd_bias_sum: head_dim*element_size must be a multiple of 16 bytes");
  auto al = [&](const void* ptr, int64_t sb, int64_t st) {
    return ((uintptr_t)ptr & 15) == 0 && sb % epc == 0 && st % epc == 0;
  };
  MMFD_CHECK_ARG(al(a->q, a->q_sb, a->q_st) && al(a->k, a->k_sb, a->k_st) && al(a->v, a->v_sb, a->v_st) &&
                     al(a->dout, a->do_sb, a->do_st),
                 "attn_bwd_bias_sum: q/k/v/dout must be 16-B aligned with strides multiple of 16 B");
  MMFD_CHECK_ARG(a->rel_bias, "attn_bwd_bias_sum: no rel_bias to differentiate");
  MMFD_CHECK_ARG(a->rel_bias_sb == 0 || a->rel_bias_mod > 0,
                 "attn_bwd_bias_sum: a per-batch rel_bias takes mmfd_attn_args.d_rel_bias of mmfd_attn_bwd; this entry "
                 "point sums over the batch rows of a shared (rel_bias_sb = 0) or modulo (rel_bias_mod > 0) bias");
  const int64_t M = a->rel_bias_sb == 0 ? 1 : a->rel_bias_mod;
  MMFD_CHECK_ARG(a->rel_bias_sb == 0 || a->rel_bias_sb == a->H * a->Lq * a->Lk,
                 "attn_bwd_bias_sum: a modulo bias must be contiguous [M][H][Lq][Lk]");
  MMFD_CHECK_ARG(a->B % M == 0, "attn_bwd_bias_sum: B = %lld is no multiple of rel_bias_mod = %lld", (long long)a->B,
                 (long long)M);
  MMFD_CHECK_ARG(a->dropout_p <= 0.f, "attn_bwd_bias_sum: attention dropout is not supported");
  MMFD_CHECK_ARG(a->cos_logit_scale == nullptr, "attn_bwd_bias_sum: cosine attention is inference-only");
  MMFD_CHECK_ARG(d_bias != a->rel_bias, "attn_bwd_bias_sum: the output must not alias rel_bias");
  MMFD_CHECK_ARG(((uintptr_t)d_bias & 15) == 0, "attn_bwd_bias_sum: the output must be 16-B aligned");
  MMFD_CHECK_ARG(M * a->H <= 65535, "attn_bwd_bias_sum: needs M*H <= 65535");
  hipStream_t s = (hipStream_t)stream;
  if (a->Lq == 0) return 0;
  if (a->B == 0) return mmfd_zero(d_bias, M * a->H * a->Lq * a->Lk * 4, stream);
  BiasSumP p;
  p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.Lk = a->Lk; p.M = M; p.D = (int)a->D; p.scale = a->scale;
  p.q = a->q; p.q_sb = a->q_sb; p.q_st = a->q_st;
  p.k = a->k; p.k_sb = a->k_sb; p.k_st = a->k_st;
  p.v = a->v; p.v_sb = a->v_sb; p.v_st = a->v_st;
  p.dout = a->dout; p.do_sb = a->do_sb; p.do_st = a->do_st;
  p.lse = a->lse; p.delta = a->delta; p.key_bias = a->key_bias;
  p.rel_bias = a->rel_bias; p.rb_sb = a->rel_bias_sb;
  if (a->dtype == MMFD_BF16) return a->D > 32 ? launch_bias_sum<bf16, 64>(p, d_bias, s) : launch_bias_sum<bf16, 32>(p, d_bias, s);
  return a->D > 32 ? launch_bias_sum<float, 64>(p, d_bias, s) : launch_bias_sum<float, 32>(p, d_bias, s);
}

extern "C" int mmfd_swin_bias_bwd(int64_t nW, int64_t H, int64_t L, int64_t T, const float* d_bias, const float* table,
                                  const int32_t* rpi, float* d_table, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(nW > 0 && H > 0 && H <= 65535 && L > 0 && T > 0, "swin_bias_bwd: bad shape");
  MMFD_CHECK_ARG(d_bias && table && rpi && d_table, "swin_bias_bwd: null pointer");
  hipLaunchKernelGGL(swin_bias_bwd_kernel, dim3((unsigned)T, (unsigned)H), dim3(256), 0, (hipStream_t)stream, nW, H,
                     L * L, d_bias, table, rpi, d_table);
  MMFD_CHECK_LAUNCH("swin_bias_bwd");
  return 0;
}

extern "C" int mmfd_swin_cpb_bwd(int64_t T, int64_t H, const float* coords, const float* w1, const float* b1,
                                 const float* w2, const float* d_table, float* d_w1, float* d_b1, float* d_w2,
                                 mmfd_stream_t stream) {
  MMFD_CHECK_ARG(H > 0 && H <= 32 && T > 0 && T <= 0x7fffffff / 32, "swin_cpb_bwd: 1 <= H <= 32 heads");
  MMFD_CHECK_ARG(coords && w1 && b1 && w2 && d_table && d_w1 && d_b1 && d_w2, "swin_cpb_bwd: null pointer");
  hipLaunchKernelGGL(swin_cpb_bwd_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, (int)T, (int)H, coords, w1, b1, w2,
                     d_table, d_w1, d_b1, d_w2);
  MMFD_CHECK_LAUNCH("swin_cpb_bwd");
  return 0;
}
