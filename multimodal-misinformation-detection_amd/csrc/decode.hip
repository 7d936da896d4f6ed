// Greedy autoregressive decoding (BLIP captioning, mmfd/blip.py): the three kernels a one-token-per-step
// decoder needs beside the GEMMs, LayerNorm and embeddings it shares with the encoders.
//
//   mmfd_attn_decode     one query token per (b, h) against Lk cached keys: keys across the lanes of a wave,
//                        16-byte loads, the dot products over D in registers, softmax statistics by wave
//                        shuffles, no MFMA; the key range is split over waves when B*H alone leaves the
//                        chip idle, and a second kernel combines the splits.
//                        mmfd_attn_decode_grouped: the same with `group` query rows per row of k / v (the beams
//                        of an image, csrc/beam.hip).
//   mmfd_lm_head_argmax  argmax_v (x . W[v] + bias[v]) for B <= 32 rows without the [B, V] logits ever
//                        being written: each workgroup streams one slab of vocabulary rows once for all B
//                        rows and leaves one (max, index) per row; a second kernel reduces those.
//                        mmfd_lm_head_argmax_wide: up to 256 rows, a grid of slabs x 32-row tiles of the same body.
//   mmfd_greedy_select   the greedy rule per row (forced token, pad after eos, finished flag).
//
// Nothing here hands data between workgroups inside a launch: every phase is its own kernel on the stream.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

// sum of N per-lane values over the 64 lanes of a wave, N a power of two <= 64: lane l returns the total of
// element l & (N - 1). While more lanes than values remain the steps are plain butterflies; after that each
// step halves the values a lane keeps (it sends the half its partner keeps), N - 1 shuffles instead of 6 N.
// (the lane distance OFF is a template argument so that every array index is a constant: the sums stay in
// registers)
template <int N, int OFF> __device__ __forceinline__ void reduce_scatter_step(float (&a)[N], int lane) {
  if constexpr (OFF >= N) {
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] += __shfl_xor(a[i], OFF, 64);
  } else {
    const bool up = (lane & OFF) != 0;
#pragma unroll
    for (int i = 0; i < OFF; ++i) {
      const float send = up ? a[i] : a[i + OFF];
      const float keep = up ? a[i + OFF] : a[i];
      a[i] = keep + __shfl_xor(send, OFF, 64);
    }
  }
  if constexpr (OFF > 1) reduce_scatter_step<N, OFF / 2>(a, lane);
}
template <int N> __device__ __forceinline__ float reduce_scatter(float (&a)[N], int lane) {
  reduce_scatter_step<N, 32>(a, lane);
  return a[0];
}

// one 16-byte chunk of a row -> fp32 (4 fp32 or 8 bf16 elements)
template <typename T> struct Chunk;
template <> struct Chunk<float> {
  static constexpr int E = 4;
  __device__ __forceinline__ static void load(const float* p, float (&f)[4]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y); f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
  }
};
template <> struct Chunk<bf16> {
  static constexpr int E = 8;
  __device__ __forceinline__ static void load(const bf16* p, float (&f)[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
    f[4] = __uint_as_float(u.z << 16); f[5] = __uint_as_float(u.z & 0xffff0000u);
    f[6] = __uint_as_float(u.w << 16); f[7] = __uint_as_float(u.w & 0xffff0000u);
  }
};

// ---------------------------------------------------------------------------------------------
// single-token attention
// ---------------------------------------------------------------------------------------------
struct DecodeParams {
  const void* q; const void* k; const void* v; void* o; float* ws;
  int64_t q_sb, k_sb, k_st, v_sb, v_st, o_sb;
  int B, H, Lk, S, chunk;   // S splits of `chunk` keys (a multiple of 64) each
  int group;                // query rows per row of k / v (GROUPED kernels only; beam search: the beams of an image)
  float scale_log2;         // scale * log2(e): the softmax runs on exp2
};

constexpr int DEC_WAVES = 4;  // independent (b, h, split) items per 256-thread workgroup

// one wave per (b, h, split): lane l takes keys k0 + l, k0 + l + 64, ... with its own running (max, sum,
// accumulator); the lanes are merged once at the end. S == 1 writes o, else the unnormalised partial
// {max, sum, acc[D]} goes to ws[(b*H + h)*S + split].
// GROUPED: query row b reads the keys and values of row b / group (the instantiation without it is the code it was).
template <typename T, int D, bool GROUPED = false>
__global__ __launch_bounds__(64 * DEC_WAVES) void attn_decode_kernel(DecodeParams p) {
  constexpr int E = Chunk<T>::E;
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * DEC_WAVES + (threadIdx.x >> 6);
  if (item >= (int64_t)p.B * p.H * p.S) return;  // (no barrier below: a wave may leave alone)
  const int split = (int)(item % p.S);
  const int64_t bh = item / p.S;
  const int b = (int)(bh / p.H), h = (int)(bh % p.H);
  const int k0 = split * p.chunk, k1 = min(p.Lk, k0 + p.chunk);

  float qf[D];
  const T* qp = (const T*)p.q + b * p.q_sb + (int64_t)h * D;
#pragma unroll
  for (int c = 0; c < D / E; ++c) {
    float f[E];
    Chunk<T>::load(qp + c * E, f);
#pragma unroll
    for (int e = 0; e < E; ++e) qf[c * E + e] = f[e] * p.scale_log2;
  }
  float acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int kv_row = GROUPED ? b / p.group : b;
  const T* kb = (const T*)p.k + kv_row * p.k_sb + (int64_t)h * D;
  const T* vb = (const T*)p.v + kv_row * p.v_sb + (int64_t)h * D;
  for (int key = k0 + lane; key < k1; key += 64) {  // rows at and past Lk are never read
    const T* kr = kb + (int64_t)key * p.k_st;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int c = 0; c < D / E; ++c) {
      float f[E];
      Chunk<T>::load(kr + c * E, f);
#pragma unroll
      for (int e = 0; e < E; e += 2) {
        s0 = fmaf(qf[c * E + e], f[e], s0);
        s1 = fmaf(qf[c * E + e + 1], f[e + 1], s1);
      }
    }
    const float s = s0 + s1;
    const float mn = fmaxf(m, s);
    const float corr = exp2f(m - mn);  // m = -inf on the first key: 0
    const float pr = exp2f(s - mn);
    l = fmaf(l, corr, pr);
    m = mn;
    const T* vr = vb + (int64_t)key * p.v_st;
#pragma unroll
    for (int c = 0; c < D / E; ++c) {
      float f[E];
      Chunk<T>::load(vr + c * E, f);
#pragma unroll
      for (int e = 0; e < E; ++e) acc[c * E + e] = fmaf(acc[c * E + e], corr, pr * f[e]);
    }
  }
  const float M = wave_max(m);
  const float f = (m == -INFINITY) ? 0.f : exp2f(m - M);  // a lane without keys contributes nothing
  const float L = wave_sum(l * f);
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] *= f;
  const float tot = reduce_scatter<D>(acc, lane);  // lane d (D = 32: lanes d and d + 32) holds element d
  if (lane < D) {
    if (p.S == 1) {
      ((T*)p.o)[b * p.o_sb + (int64_t)h * D + lane] = from_f32<T>(tot / L);
    } else {
      float* w = p.ws + item * (D + 2);
      if (lane == 0) { w[0] = M; w[1] = L; }
      w[2 + lane] = tot;
    }
  }
}

// o[b][h*D + d] = sum_s acc_s[d] 2^(M_s - M) / sum_s L_s 2^(M_s - M): one thread per output element
template <typename T> __global__ void attn_decode_combine_kernel(DecodeParams p, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)p.B * p.H * D) return;
  const int d = (int)(i % D);
  const int64_t bh = i / D;
  const float* w = p.ws + bh * p.S * (D + 2);
  float M = -INFINITY;
  for (int s = 0; s < p.S; ++s) M = fmaxf(M, w[s * (D + 2)]);
  float L = 0.f, a = 0.f;
  for (int s = 0; s < p.S; ++s) {
    const float f = exp2f(w[s * (D + 2)] - M);
    L = fmaf(w[s * (D + 2) + 1], f, L);
    a = fmaf(w[s * (D + 2) + 2 + d], f, a);
  }
  const int b = (int)(bh / p.H), h = (int)(bh % p.H);
  ((T*)p.o)[b * p.o_sb + (int64_t)h * D + d] = from_f32<T>(a / L);
}

// The split rule: one wave covers 64 keys per step, so a (b, h) has ceil(Lk / 64) steps to hand out; they are
// spread over as many waves as it takes to put about one wave on every SIMD of the chip (256 CUs x 4), and
// never over more than DEC_MAX_SPLITS (the combine reads every split per output element).
constexpr int DEC_TARGET_WAVES = 1024, DEC_MAX_SPLITS = 32;
void decode_plan(int64_t B, int64_t H, int64_t Lk, int& S, int& chunk) {
  const int64_t steps = (Lk + 63) / 64;
  const int64_t want = std::max<int64_t>(1, DEC_TARGET_WAVES / std::max<int64_t>(1, B * H));
  const int64_t s = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(steps, want), DEC_MAX_SPLITS));
  const int64_t per = (steps + s - 1) / s;  // steps per split
  chunk = (int)(per * 64);
  S = (int)((steps + per - 1) / per);
}

// ---------------------------------------------------------------------------------------------
// LM head + argmax
// ---------------------------------------------------------------------------------------------
constexpr int LMH_WAVES = 8;  // waves per workgroup (512 threads)

struct LmhPlan { int BT, R, NJ, G, slab; int64_t lds; };

// BT: batch rows padded to {4, 8, 16, 32}; NJ: 16-byte chunks of a row per lane; R: vocabulary rows a wave
// takes per step (BT*R <= 64 sums and at most 64 weight registers per lane); G workgroups of `slab`
// consecutive vocabulary rows.
constexpr int lmh_rows(int E, int BT, int NJ) {
  const int r = NJ * E <= 16 ? 4 : NJ * E <= 24 ? 2 : 1;
  return r * BT <= 64 ? r : 64 / BT;
}
bool lmh_plan(int dtype, int64_t B, int64_t V, int64_t K, LmhPlan& pl) {
  const int E = dtype == MMFD_BF16 ? 8 : 4;
  if (B < 1 || B > 32 || V < 1 || K < E || K % E) return false;
  pl.BT = B <= 4 ? 4 : B <= 8 ? 8 : B <= 16 ? 16 : 32;
  const int64_t nch = K / E;
  pl.NJ = (int)((nch + 63) / 64);
  if (pl.NJ > 4) return false;
  pl.R = lmh_rows(E, pl.BT, pl.NJ);
  pl.lds = (int64_t)pl.BT * pl.NJ * 64 * E * 4;  // x as fp32, zero padded
  const int64_t gmax = pl.lds <= 72 * 1024 ? 512 : 256;  // two workgroups per CU where LDS lets them
  const int64_t per_step = (int64_t)LMH_WAVES * pl.R;
  int64_t G = std::max<int64_t>(1, std::min<int64_t>(gmax, (V + per_step - 1) / per_step));
  int64_t slab = (V + G - 1) / G;
  slab = (slab + pl.R - 1) / pl.R * pl.R;
  pl.slab = (int)slab;
  pl.G = (int)((V + slab - 1) / slab);
  return true;
}

__device__ __forceinline__ bool lmh_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// One workgroup's share: slab blockIdx.x of the vocabulary against the B <= BT rows of x. The (max, index) of row
// b goes to pval / pidx[blockIdx.x * pld + b]. Both kernels below are this body: the logit of a row is the same
// bits whichever of them computed it.
template <typename T, int BT, int NJ>
__device__ __forceinline__ void lm_head_tile(const T* __restrict__ x, int64_t ldx, const T* __restrict__ W, int64_t ldw,
                                             const float* __restrict__ bias, int B, int V, int K, int slab,
                                             float* __restrict__ logits, int64_t ldl, float* __restrict__ pval,
                                             int* __restrict__ pidx, int64_t pld) {
  constexpr int E = Chunk<T>::E, Q = E / 4, R = lmh_rows(E, BT, NJ), N = BT * R;
  static_assert(N <= 64, "one (row, batch) sum per lane after the reduce");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xs = reinterpret_cast<float*>(smem);  // [BT][NJ][Q][64 lanes][4]: every 16-byte read lane-contiguous
  __shared__ float sval[LMH_WAVES][N];
  __shared__ int sidx[LMH_WAVES][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = K / E;
  const int row_lo = blockIdx.x * slab, row_hi = min(V, row_lo + slab);

  for (int i = threadIdx.x; i < BT * NJ * 64 * E; i += 64 * LMH_WAVES) {
    const int b = i / (NJ * 64 * E), kk = i % (NJ * 64 * E);
    const int c = kk / E, e = kk % E;
    const float val = (b < B && kk < K) ? to_f32(x[b * ldx + kk]) : 0.f;
    xs[(((b * NJ + c / 64) * Q + e / 4) * 64 + (c % 64)) * 4 + (e % 4)] = val;
  }
  __syncthreads();

  const int slot = lane & (N - 1);          // the sum this lane holds after the reduce: row slot / BT, batch slot % BT
  const int my_r = slot / BT, my_b = slot % BT;
  float best = -INFINITY;
  int besti = INT_MAX;
  for (int r0 = row_lo + wave * R; r0 < row_hi; r0 += LMH_WAVES * R) {
    float w[R][NJ][E];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        if (r0 + r < row_hi && c < nch) {
          Chunk<T>::load(W + (int64_t)(r0 + r) * ldw + (int64_t)c * E, w[r][j]);
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) w[r][j][e] = 0.f;
        }
      }
    float acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.f;
#pragma unroll
    for (int b = 0; b < BT; ++b) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int qd = 0; qd < Q; ++qd) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(&xs[(((b * NJ + j) * Q + qd) * 64 + lane) * 4]);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            float a = acc[r * BT + b];
            a = fmaf(xv[0], w[r][j][qd * 4 + 0], a);
            a = fmaf(xv[1], w[r][j][qd * 4 + 1], a);
            a = fmaf(xv[2], w[r][j][qd * 4 + 2], a);
            a = fmaf(xv[3], w[r][j][qd * 4 + 3], a);
            acc[r * BT + b] = a;
          }
        }
      // the loop is unrolled for constant register indices; without this fence the scheduler hoists the LDS
      // reads of every batch row to the top and spills (two rows of reads stay in flight)
      if (b % 2 == 1) __builtin_amdgcn_sched_barrier(0);
    }
    float v = reduce_scatter<N>(acc, lane);
    const int row = r0 + my_r;
    if (lane < N && row < row_hi && my_b < B) {
      v += bias ? bias[row] : 0.f;
      if (logits) logits[my_b * ldl + row] = v;
      if (lmh_better(v, row, best, besti)) { best = v; besti = row; }
    }
  }
  if (lane < N) { sval[wave][lane] = best; sidx[wave][lane] = besti; }
  __syncthreads();
  if (threadIdx.x < B) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int wv = 0; wv < LMH_WAVES; ++wv)
      for (int r = 0; r < R; ++r) {
        const float v = sval[wv][r * BT + threadIdx.x];
        const int i = sidx[wv][r * BT + threadIdx.x];
        if (lmh_better(v, i, bv, bi)) { bv = v; bi = i; }
      }
    pval[(int64_t)blockIdx.x * pld + threadIdx.x] = bv;
    pidx[(int64_t)blockIdx.x * pld + threadIdx.x] = bi;
  }
}

template <typename T, int BT, int NJ>
__global__ __launch_bounds__(64 * LMH_WAVES) void lm_head_kernel(const T* __restrict__ x, int64_t ldx,
                                                                  const T* __restrict__ W, int64_t ldw,
                                                                  const float* __restrict__ bias, int B, int V, int K,
                                                                  int slab, float* __restrict__ logits, int64_t ldl,
                                                                  float* __restrict__ pval, int* __restrict__ pidx) {
  lm_head_tile<T, BT, NJ>(x, ldx, W, ldw, bias, B, V, K, slab, logits, ldl, pval, pidx, B);
}

// B <= 256 rows in tiles of LMH_TILE: workgroup (g, t) is lm_head_tile on slab g and rows 32 t .. 32 t + 31 (the
// last tile zero padded, as the narrow kernel pads a short batch), so W is read once per row tile; the partials
// lie [G][B] as the narrow kernel leaves them and lm_head_final_kernel reduces them unchanged.
constexpr int LMH_TILE = 32, LMH_WIDE_ROWS = 256;
template <typename T, int NJ>
__global__ __launch_bounds__(64 * LMH_WAVES) void lm_head_wide_kernel(const T* __restrict__ x, int64_t ldx,
                                                                       const T* __restrict__ W, int64_t ldw,
                                                                       const float* __restrict__ bias, int B, int V,
                                                                       int K, int slab, float* __restrict__ logits,
                                                                       int64_t ldl, float* __restrict__ pval,
                                                                       int* __restrict__ pidx) {
  const int b0 = blockIdx.y * LMH_TILE;
  lm_head_tile<T, LMH_TILE, NJ>(x + b0 * ldx, ldx, W, ldw, bias, min(LMH_TILE, B - b0), V, K, slab,
                                logits ? logits + b0 * ldl : nullptr, ldl, pval + b0, pidx + b0, B);
}

// one wave per batch row over the G per-workgroup partials: the largest value, ties to the lowest index; a
// NaN never compares larger, so it is never chosen over a number (a row of nothing but NaN gives token 0)
__global__ __launch_bounds__(64) void lm_head_final_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                           int G, int B, int64_t* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float bv = -INFINITY;
  int bi = INT_MAX;
  for (int g = lane; g < G; g += 64) {
    const float v = pval[(int64_t)g * B + b];
    const int i = pidx[(int64_t)g * B + b];
    if (lmh_better(v, i, bv, bi)) { bv = v; bi = i; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (lmh_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) out[b] = bi == INT_MAX ? 0 : bi;
}

template <typename T, int BT, int NJ>
int lmh_launch(const LmhPlan& pl, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* bias, int64_t B,
               int64_t V, int64_t K, float* logits, int64_t ldl, float* pval, int* pidx, hipStream_t s) {
  auto kern = &lm_head_kernel<T, BT, NJ>;
  if (pl.lds > 48 * 1024 &&  // (per device and cheap: set whenever the launch needs it)
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)pl.lds) != hipSuccess)
    return mmfd_set_error(MMFD_ERR_UNSUPPORTED, "mmfd_lm_head_argmax: cannot reserve %lld bytes of LDS",
                          (long long)pl.lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)pl.G), dim3(64 * LMH_WAVES), (size_t)pl.lds, s, (const T*)x, ldx, (const T*)W,
                     ldw, bias, (int)B, (int)V, (int)K, pl.slab, logits, ldl, pval, pidx);
  return 0;
}

template <typename T, int BT>
int lmh_launch_nj(const LmhPlan& pl, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* bias, int64_t B,
                  int64_t V, int64_t K, float* logits, int64_t ldl, float* pval, int* pidx, hipStream_t s) {
  switch (pl.NJ) {
    case 1: return lmh_launch<T, BT, 1>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    case 2: return lmh_launch<T, BT, 2>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    case 3: return lmh_launch<T, BT, 3>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    default: return lmh_launch<T, BT, 4>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
  }
}

template <typename T>
int lmh_launch_bt(const LmhPlan& pl, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* bias, int64_t B,
                  int64_t V, int64_t K, float* logits, int64_t ldl, float* pval, int* pidx, hipStream_t s) {
  switch (pl.BT) {
    case 4: return lmh_launch_nj<T, 4>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    case 8: return lmh_launch_nj<T, 8>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    case 16: return lmh_launch_nj<T, 16>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    default: return lmh_launch_nj<T, 32>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
  }
}

template <typename T, int NJ>
int lmh_wide_launch(const LmhPlan& pl, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* bias,
                    int64_t B, int64_t V, int64_t K, float* logits, int64_t ldl, float* pval, int* pidx, hipStream_t s) {
  auto kern = &lm_head_wide_kernel<T, NJ>;
  if (pl.lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)pl.lds) != hipSuccess)
    return mmfd_set_error(MMFD_ERR_UNSUPPORTED, "mmfd_lm_head_argmax_wide: cannot reserve %lld bytes of LDS",
                          (long long)pl.lds);
  const dim3 grid((unsigned)pl.G, (unsigned)((B + LMH_TILE - 1) / LMH_TILE));
  hipLaunchKernelGGL(kern, grid, dim3(64 * LMH_WAVES), (size_t)pl.lds, s, (const T*)x, ldx, (const T*)W, ldw, bias,
                     (int)B, (int)V, (int)K, pl.slab, logits, ldl, pval, pidx);
  return 0;
}

template <typename T>
int lmh_wide_launch_nj(const LmhPlan& pl, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* bias,
                       int64_t B, int64_t V, int64_t K, float* logits, int64_t ldl, float* pval, int* pidx,
                       hipStream_t s) {
  switch (pl.NJ) {
    case 1: return lmh_wide_launch<T, 1>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    case 2: return lmh_wide_launch<T, 2>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    case 3: return lmh_wide_launch<T, 3>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
    default: return lmh_wide_launch<T, 4>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
  }
}

// the wide kernel's plan is the narrow kernel's at a full row tile: the same slabs, so the same workgroup
// computes a vocabulary row however many rows the call holds
// (a tile of x lies in LDS as fp32, 64 lanes x 16 bytes per chunk: beside the 4 KiB of per-wave partials that is
// within the 160 KiB of a workgroup up to 1024 elements per row in either dtype, as at 32 rows of the narrow kernel)
constexpr int64_t LMH_WIDE_MAX_K = 1024;
bool lmh_wide_plan(int dtype, int64_t B, int64_t V, int64_t K, LmhPlan& pl) {
  return B >= 1 && B <= LMH_WIDE_ROWS && K <= LMH_WIDE_MAX_K && lmh_plan(dtype, LMH_TILE, V, K, pl) &&
         pl.lds + 4096 <= 160 * 1024;
}

// ---------------------------------------------------------------------------------------------
// greedy select
// ---------------------------------------------------------------------------------------------
__global__ void greedy_select_kernel(int B, const int64_t* __restrict__ argmax, const int64_t* __restrict__ forced,
                                     int64_t forced_ld, int* __restrict__ finished, int64_t eos, int64_t pad,
                                     int64_t* __restrict__ next, int64_t next_ld) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int was = finished[b];
  const int64_t tok = forced ? forced[b * forced_ld] : (was ? pad : argmax[b]);
  next[b * next_ld] = tok;
  finished[b] = (was || tok == eos) ? 1 : 0;
}

}  // namespace

extern "C" int mmfd_attn_decode_splits(int64_t B, int64_t H, int64_t Lk) {
  if (B < 1 || H < 1 || Lk < 1) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_attn_decode_splits: bad shape");
    return -1;
  }
  int S, chunk;
  decode_plan(B, H, Lk, S, chunk);
  return S;
}

extern "C" int64_t mmfd_attn_decode_workspace_bytes(int64_t B, int64_t H, int64_t D, int64_t Lk) {
  if (B < 1 || H < 1 || Lk < 1 || D < 1) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_attn_decode_workspace_bytes: bad shape");
    return -1;
  }
  int S, chunk;
  decode_plan(B, H, Lk, S, chunk);
  return S > 1 ? B * H * S * (D + 2) * (int64_t)sizeof(float) : 0;
}

namespace {
int attn_decode_impl(int dtype, int64_t B, int64_t group, int64_t H, int64_t D, int64_t Lk, float scale, const void* q,
                     int64_t q_sb, const void* k, int64_t k_sb, int64_t k_st, const void* v, int64_t v_sb,
                     int64_t v_st, void* o, int64_t o_sb, void* workspace, int64_t workspace_bytes,
                     mmfd_stream_t stream) {
  MMFD_CHECK_ARG(dtype == MMFD_F32 || dtype == MMFD_BF16, "mmfd_attn_decode: bad dtype");
  MMFD_CHECK_ARG(D == 32 || D == 64, "mmfd_attn_decode: head_dim %lld unsupported (32 or 64)", (long long)D);
  MMFD_CHECK_ARG(B >= 0 && H > 0 && B * H < (1 << 24), "mmfd_attn_decode: bad shape");
  MMFD_CHECK_ARG(Lk > 0 && Lk < (1 << 30), "mmfd_attn_decode: Lk = %lld (at least one key)", (long long)Lk);
  MMFD_CHECK_ARG(q && k && v && o, "mmfd_attn_decode: null pointer");
  const int64_t epc = dtype == MMFD_BF16 ? 8 : 4;  // elements per 16 bytes
  auto al = [&](const void* ptr, int64_t s0, int64_t s1) {
    return ((uintptr_t)ptr & 15) == 0 && s0 % epc == 0 && s1 % epc == 0;
  };
  MMFD_CHECK_ARG(al(q, q_sb, 0) && al(k, k_sb, k_st) && al(v, v_sb, v_st),
                 "mmfd_attn_decode: q/k/v pointers and strides must be 16-byte aligned");
  if (B == 0) return 0;
  DecodeParams p;
  p.q = q; p.k = k; p.v = v; p.o = o; p.ws = (float*)workspace;
  p.q_sb = q_sb; p.k_sb = k_sb; p.k_st = k_st; p.v_sb = v_sb; p.v_st = v_st; p.o_sb = o_sb;
  p.B = (int)B; p.H = (int)H; p.Lk = (int)Lk; p.group = (int)group;
  decode_plan(B, H, Lk, p.S, p.chunk);
  p.scale_log2 = scale * 1.4426950408889634f;
  if (p.S > 1) {
    const int64_t need = B * H * p.S * (D + 2) * (int64_t)sizeof(float);
    MMFD_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                   "mmfd_attn_decode: %d splits need a workspace of %lld bytes (mmfd_attn_decode_workspace_bytes)",
                   p.S, (long long)need);
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t items = B * H * p.S;
  const dim3 grid((unsigned)((items + DEC_WAVES - 1) / DEC_WAVES)), block(64 * DEC_WAVES);
  if (group > 1) {
    if (dtype == MMFD_F32) {
      if (D == 64) hipLaunchKernelGGL((attn_decode_kernel<float, 64, true>), grid, block, 0, s, p);
      else hipLaunchKernelGGL((attn_decode_kernel<float, 32, true>), grid, block, 0, s, p);
    } else {
      if (D == 64) hipLaunchKernelGGL((attn_decode_kernel<bf16, 64, true>), grid, block, 0, s, p);
      else hipLaunchKernelGGL((attn_decode_kernel<bf16, 32, true>), grid, block, 0, s, p);
    }
  } else if (dtype == MMFD_F32) {
    if (D == 64) hipLaunchKernelGGL((attn_decode_kernel<float, 64>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((attn_decode_kernel<float, 32>), grid, block, 0, s, p);
  } else {
    if (D == 64) hipLaunchKernelGGL((attn_decode_kernel<bf16, 64>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((attn_decode_kernel<bf16, 32>), grid, block, 0, s, p);
  }
  MMFD_CHECK_LAUNCH("mmfd_attn_decode");
  if (p.S > 1) {
    const int64_t n = B * H * D;
    const dim3 g2((unsigned)((n + 255) / 256));
    if (dtype == MMFD_F32) hipLaunchKernelGGL(attn_decode_combine_kernel<float>, g2, dim3(256), 0, s, p, (int)D);
    else hipLaunchKernelGGL(attn_decode_combine_kernel<bf16>, g2, dim3(256), 0, s, p, (int)D);
    MMFD_CHECK_LAUNCH("mmfd_attn_decode (combine)");
  }
  return 0;
}
}  // namespace

extern "C" int mmfd_attn_decode(int dtype, int64_t B, int64_t H, int64_t D, int64_t Lk, float scale, const void* q,
                                int64_t q_sb, const void* k, int64_t k_sb, int64_t k_st, const void* v, int64_t v_sb,
                                int64_t v_st, void* o, int64_t o_sb, void* workspace, int64_t workspace_bytes,
                                mmfd_stream_t stream) {
  return attn_decode_impl(dtype, B, 1, H, D, Lk, scale, q, q_sb, k, k_sb, k_st, v, v_sb, v_st, o, o_sb, workspace,
                          workspace_bytes, stream);
}

extern "C" int mmfd_attn_decode_grouped(int dtype, int64_t B, int64_t group, int64_t H, int64_t D, int64_t Lk,
                                        float scale, const void* q, int64_t q_sb, const void* k, int64_t k_sb,
                                        int64_t k_st, const void* v, int64_t v_sb, int64_t v_st, void* o, int64_t o_sb,
                                        void* workspace, int64_t workspace_bytes, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(group >= 1 && group <= 64 && B % group == 0,
                 "mmfd_attn_decode_grouped: %lld query rows in groups of %lld", (long long)B, (long long)group);
  return attn_decode_impl(dtype, B, group, H, D, Lk, scale, q, q_sb, k, k_sb, k_st, v, v_sb, v_st, o, o_sb, workspace,
                          workspace_bytes, stream);
}

extern "C" int64_t mmfd_lm_head_argmax_workspace_bytes(int dtype, int64_t B, int64_t V, int64_t K) {
  LmhPlan pl;
  if (!lmh_plan(dtype, B, V, K, pl)) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_lm_head_argmax_workspace_bytes: unsupported shape");
    return -1;
  }
  return (int64_t)pl.G * B * 8;
}

extern "C" int64_t mmfd_lm_head_argmax_slab(int dtype, int64_t B, int64_t V, int64_t K) {
  LmhPlan pl;
  if (!lmh_plan(dtype, B, V, K, pl)) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_lm_head_argmax_slab: unsupported shape");
    return -1;
  }
  return pl.slab;
}

extern "C" int mmfd_lm_head_argmax(int dtype, int64_t B, int64_t V, int64_t K, const void* x, int64_t ldx, const void* W,
                                   int64_t ldw, const float* bias, int64_t* out_idx, float* logits, int64_t ldl,
                                   void* workspace, int64_t workspace_bytes, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(dtype == MMFD_F32 || dtype == MMFD_BF16, "mmfd_lm_head_argmax: bad dtype");
  MMFD_CHECK_ARG(B >= 1 && B <= 32, "mmfd_lm_head_argmax: B = %lld (1 .. 32 rows)", (long long)B);
  MMFD_CHECK_ARG(V >= 1 && V < (1 << 30), "mmfd_lm_head_argmax: V = %lld", (long long)V);
  const int64_t epc = dtype == MMFD_BF16 ? 8 : 4;
  LmhPlan pl;
  MMFD_CHECK_ARG(lmh_plan(dtype, B, V, K, pl), "mmfd_lm_head_argmax: K = %lld must be a multiple of %lld and <= %lld",
                 (long long)K, (long long)epc, (long long)(256 * epc));
  MMFD_CHECK_ARG(x && W && out_idx, "mmfd_lm_head_argmax: null pointer");
  MMFD_CHECK_ARG(ldx >= K && ldw >= K && (!logits || ldl >= V), "mmfd_lm_head_argmax: leading dimension too small");
  MMFD_CHECK_ARG(((uintptr_t)W & 15) == 0 && ldw % epc == 0, "mmfd_lm_head_argmax: W rows must be 16-byte aligned");
  const int64_t need = (int64_t)pl.G * B * 8;
  MMFD_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                 "mmfd_lm_head_argmax: needs a workspace of %lld bytes (mmfd_lm_head_argmax_workspace_bytes)",
                 (long long)need);
  float* pval = (float*)workspace;
  int* pidx = (int*)(pval + (int64_t)pl.G * B);
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == MMFD_F32
                     ? lmh_launch_bt<float>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s)
                     : lmh_launch_bt<bf16>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
  if (rc) return rc;
  MMFD_CHECK_LAUNCH("mmfd_lm_head_argmax");
  hipLaunchKernelGGL(lm_head_final_kernel, dim3((unsigned)B), dim3(64), 0, s, pval, pidx, pl.G, (int)B, out_idx);
  MMFD_CHECK_LAUNCH("mmfd_lm_head_argmax (final)");
  return 0;
}

extern "C" int64_t mmfd_lm_head_argmax_wide_workspace_bytes(int dtype, int64_t B, int64_t V, int64_t K) {
  LmhPlan pl;
  if ((dtype != MMFD_F32 && dtype != MMFD_BF16) || !lmh_wide_plan(dtype, B, V, K, pl)) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_lm_head_argmax_wide_workspace_bytes: unsupported shape");
    return -1;
  }
  return (int64_t)pl.G * B * 8;
}

extern "C" int mmfd_lm_head_argmax_wide(int dtype, int64_t B, int64_t V, int64_t K, const void* x, int64_t ldx,
                                        const void* W, int64_t ldw, const float* bias, int64_t* out_idx, float* logits,
                                        int64_t ldl, void* workspace, int64_t workspace_bytes, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(dtype == MMFD_F32 || dtype == MMFD_BF16, "mmfd_lm_head_argmax_wide: bad dtype");
  MMFD_CHECK_ARG(B >= 1 && B <= LMH_WIDE_ROWS, "mmfd_lm_head_argmax_wide: B = %lld (1 .. %d rows)", (long long)B,
                 LMH_WIDE_ROWS);
  MMFD_CHECK_ARG(V >= 1 && V < (1 << 30), "mmfd_lm_head_argmax_wide: V = %lld", (long long)V);
  const int64_t epc = dtype == MMFD_BF16 ? 8 : 4;
  LmhPlan pl;
  MMFD_CHECK_ARG(lmh_wide_plan(dtype, B, V, K, pl),
                 "mmfd_lm_head_argmax_wide: K = %lld must be a multiple of %lld and <= %lld (a 32-row tile of x lies "
                 "in LDS as fp32)", (long long)K, (long long)epc, (long long)LMH_WIDE_MAX_K);
  MMFD_CHECK_ARG(x && W && out_idx, "mmfd_lm_head_argmax_wide: null pointer");
  MMFD_CHECK_ARG(ldx >= K && ldw >= K && (!logits || ldl >= V), "mmfd_lm_head_argmax_wide: leading dimension too small");
  MMFD_CHECK_ARG(((uintptr_t)W & 15) == 0 && ldw % epc == 0, "mmfd_lm_head_argmax_wide: W rows must be 16-byte aligned");
  const int64_t need = (int64_t)pl.G * B * 8;
  MMFD_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                 "mmfd_lm_head_argmax_wide: needs a workspace of %lld bytes (mmfd_lm_head_argmax_wide_workspace_bytes)",
                 (long long)need);
  float* pval = (float*)workspace;
  int* pidx = (int*)(pval + (int64_t)pl.G * B);
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == MMFD_F32
                     ? lmh_wide_launch_nj<float>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s)
                     : lmh_wide_launch_nj<bf16>(pl, x, ldx, W, ldw, bias, B, V, K, logits, ldl, pval, pidx, s);
  if (rc) return rc;
  MMFD_CHECK_LAUNCH("mmfd_lm_head_argmax_wide");
  hipLaunchKernelGGL(lm_head_final_kernel, dim3((unsigned)B), dim3(64), 0, s, pval, pidx, pl.G, (int)B, out_idx);
  MMFD_CHECK_LAUNCH("mmfd_lm_head_argmax_wide (final)");
  return 0;
}

extern "C" int mmfd_greedy_select(int64_t B, const int64_t* argmax, const int64_t* forced, int64_t forced_ld,
                                  int32_t* finished, int64_t eos, int64_t pad, int64_t* next, int64_t next_ld,
                                  mmfd_stream_t stream) {
  MMFD_CHECK_ARG(B >= 0 && B < (1 << 24), "mmfd_greedy_select: bad B");
  MMFD_CHECK_ARG((argmax || forced) && finished && next, "mmfd_greedy_select: null pointer");
  if (B == 0) return 0;
  hipLaunchKernelGGL(greedy_select_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (int)B,
                     argmax, forced, forced_ld, (int*)finished, eos, pad, next, next_ld);
  MMFD_CHECK_LAUNCH("mmfd_greedy_select");
  return 0;
}
