// Vocabulary cross-entropy of the BLIP text decoder's language-model loss (mmfd.blip, forward(labels=)):
// torch's CrossEntropyLoss(label_smoothing = eps, ignore_index = -100) over materialised fp32 logits [R][V],
// forward (per-row loss and log-sum-exp, then a fixed-order reduction) and backward (dlogits in the compute
// dtype). Both passes are memory bound: one workgroup per row streams the row once with 16-byte loads —
// R*V*4 bytes read by the forward, R*V*(4 + esz) bytes moved by the backward — and every reduction runs in a
// fixed order, so the same inputs give the same bits.
#include <float.h>

#include "common.h"

namespace {
constexpr int NT = 256;  // threads of a row's workgroup (4 waves)

__device__ __forceinline__ bool label_valid(int64_t y, int64_t V) { return y >= 0 && y < V; }

// running (max, sum of exp(z - max)) of a softmax row: merge of two partial results. An empty partial is
// (-FLT_MAX, 0): finite, so max - max is never inf - inf. The exponentials are fp32 (the largest is exp(0) = 1,
// exact); their sum is kept in double, so the log-sum-exp carries no accumulation error of its own
__device__ __forceinline__ void ms_merge(float& m, double& s, float m2, double s2) {
  const float mn = fmaxf(m, m2);
  s = s * exp((double)m - (double)mn) + s2 * exp((double)m2 - (double)mn);
  m = mn;
}
__device__ __forceinline__ void ms_add4(float& m, double& s, float a, float b, float c, float d) {
  const float mx = fmaxf(fmaxf(a, b), fmaxf(c, d));
  if (mx > m) {
    s *= exp((double)m - (double)mx);
    m = mx;
  }
  s += ((double)expf(a - m) + (double)expf(b - m)) + ((double)expf(c - m) + (double)expf(d - m));
}
__device__ __forceinline__ void ms_add1(float& m, double& s, float a) {
  if (a > m) {
    s *= exp((double)m - (double)a);
    m = a;
  }
  s += (double)expf(a - m);
}

// loss_r = lse_r - (1 - eps) z_r[y_r] - (eps / V) sum_v z_r[v]; 0 for an ignored row (its lse is still written)
template <bool VEC>
__global__ __launch_bounds__(NT) void vocab_xent_fwd_kernel(int64_t V, const float* __restrict__ logits, int64_t ldl,
                                                           const int64_t* __restrict__ labels, float eps,
                                                           float* __restrict__ loss_rows, float* __restrict__ lse_out,
                                                           float* __restrict__ lse_lo) {
  const int64_t r = blockIdx.x;
  const float* __restrict__ z = logits + r * ldl;
  const int t = threadIdx.x;
  float m = -FLT_MAX;
  double s = 0.0;
  double zs = 0.0;  // sum of the row's logits (label smoothing only)
  const bool smooth = eps != 0.f;
  int64_t done = 0;
  if (VEC) {
    const int64_t n4 = V >> 2;
    const f32x4* __restrict__ z4 = reinterpret_cast<const f32x4*>(z);
    for (int64_t c = t; c < n4; c += NT) {
      const f32x4 a = z4[c];
      ms_add4(m, s, a.x, a.y, a.z, a.w);
      if (smooth) zs += (double)((a.x + a.y) + (a.z + a.w));
    }
    done = n4 << 2;
  }
  for (int64_t v = done + t; v < V; v += NT) {  // the scalar tail, or the whole row without 16-byte alignment
    const float a = z[v];
    ms_add1(m, s, a);
    if (smooth) zs += (double)a;
  }
  // wave butterfly: every lane ends with the same (m, s, zs), the operations being commutative
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const double s2 = __shfl_xor(s, o, 64);
    ms_merge(m, s, m2, s2);
    zs += __shfl_xor(zs, o, 64);
  }
  __shared__ float sm[NT / 64];
  __shared__ double ss[NT / 64], sz[NT / 64];
  if ((t & 63) == 0) {
    sm[t >> 6] = m;
    ss[t >> 6] = s;
    sz[t >> 6] = zs;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < NT / 64; ++w) {
      ms_merge(m, s, sm[w], ss[w]);
      zs += sz[w];
    }
    const double lse = (double)m + log(s);
    lse_out[r] = (float)lse;
    if (lse_lo) lse_lo[r] = (float)(lse - (double)(float)lse);
    const int64_t y = labels[r];
    float loss = 0.f;
    if (label_valid(y, V)) {
      double l = lse - (1.0 - (double)eps) * (double)z[y];
      if (smooth) l -= (double)eps / (double)V * zs;
      loss = (float)l;
    }
    loss_rows[r] = loss;
  }
}

// one workgroup, fixed order: mean over the valid rows (0 valid rows: 0 / 0 = NaN, as torch), their number, and
// the sums of every run of rows_per_seq rows
__global__ __launch_bounds__(NT) void vocab_xent_reduce_kernel(int64_t R, int64_t V, int64_t rows_per_seq,
                                                              const int64_t* __restrict__ labels,
                                                              const float* __restrict__ loss_rows, float* __restrict__ mean,
                                                              int64_t* __restrict__ n_valid, float* __restrict__ seq_sums) {
  const int t = threadIdx.x;
  double acc = 0.0;
  long long cnt = 0;
  for (int64_t r = t; r < R; r += NT) {
    acc += (double)loss_rows[r];
    cnt += label_valid(labels[r], V) ? 1 : 0;
  }
  __shared__ double sa[NT];
  __shared__ long long sc[NT];
  sa[t] = acc;
  sc[t] = cnt;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (t < o) {
      sa[t] += sa[t + o];
      sc[t] += sc[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (mean) *mean = (float)(sa[0] / (double)sc[0]);
    if (n_valid) *n_valid = (int64_t)sc[0];
  }
  if (seq_sums) {
    const int64_t B = R / rows_per_seq;
    for (int64_t b = t; b < B; b += NT) {
      double a = 0.0;
      for (int64_t j = 0; j < rows_per_seq; ++j) a += (double)loss_rows[b * rows_per_seq + j];
      seq_sums[b] = (float)a;
    }
  }
}

template <typename T> struct out_chunk;  // 16 bytes of the output row
template <> struct out_chunk<float> {
  static constexpr int E = 4;
  __device__ __forceinline__ static void store(float* p, const float* v) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  }
};
template <> struct out_chunk<bf16> {
  static constexpr int E = 8;
  __device__ __forceinline__ static void store(bf16* p, const float* v) {
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (bf16)v[i];
    *reinterpret_cast<bf16x8*>(p) = o;
  }
};

// dlogits[r][v] = g_r (exp(z - lse_r) - (1 - eps) [v == y_r] - eps / V); an ignored row is written as exact zeros
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void vocab_xent_bwd_kernel(int64_t V, const float* __restrict__ logits, int64_t ldl,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ lse,
                                                           const float* __restrict__ lse_lo, float eps,
                                                           const float* __restrict__ upstream,
                                                           const int64_t* __restrict__ n_valid, int64_t rows_per_seq,
                                                           T* __restrict__ dlogits, int64_t ldd) {
  constexpr int E = out_chunk<T>::E;
  const int64_t r = blockIdx.x;
  const float* __restrict__ z = logits + r * ldl;
  T* __restrict__ d = dlogits + r * ldd;
  const int t = threadIdx.x;
  const int64_t y = labels[r];
  const bool valid = label_valid(y, V);
  float g = 0.f;
  if (valid) g = n_valid ? (upstream ? upstream[0] : 1.f) / (float)n_valid[0] : upstream[r / rows_per_seq];
  // z - lse in double from the two-float lse: near the row's largest probabilities z - lse is small, and rounding
  // lse itself to fp32 first would leave its whole ulp (of a value near 10) in their exponent
  const double L = (double)lse[r] + (lse_lo ? (double)lse_lo[r] : 0.0);
  const float keep = 1.f - eps, ev = eps / (float)V;
  int64_t done = 0;
  if (VEC) {
    const int64_t nc = V / E;
    for (int64_t c = t; c < nc; c += NT) {
      float v[E];
      if (valid) {
#pragma unroll
        for (int h = 0; h < E / 4; ++h) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(z + c * E + 4 * h);
          v[4 * h] = a.x, v[4 * h + 1] = a.y, v[4 * h + 2] = a.z, v[4 * h + 3] = a.w;
        }
#pragma unroll
        for (int i = 0; i < E; ++i) {
          float p = expf((float)((double)v[i] - L));
          if (c * E + i == y) p -= keep;
          v[i] = g * (p - ev);
        }
      } else {
#pragma unroll
        for (int i = 0; i < E; ++i) v[i] = 0.f;
      }
      out_chunk<T>::store(d + c * E, v);
    }
    done = nc * E;
  }
  for (int64_t c = done + t; c < V; c += NT) {
    float p = 0.f;
    if (valid) {
      p = expf((float)((double)z[c] - L));
      if (c == y) p -= keep;
      p = g * (p - ev);
    }
    d[c] = from_f32<T>(p);
  }
}
}  // namespace

extern "C" int mmfd_vocab_xent_fwd(int64_t R, int64_t V, const float* logits, int64_t ldl, const int64_t* labels, float eps,
                                   int64_t rows_per_seq, float* loss_rows, float* lse, float* lse_lo, float* mean,
                                   int64_t* n_valid, float* seq_sums, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(R >= 1 && R <= 0x7fffffffLL, "mmfd_vocab_xent_fwd: R = %lld outside [1, 2^31)", (long long)R);
  MMFD_CHECK_ARG(V >= 1, "mmfd_vocab_xent_fwd: V = %lld must be >= 1", (long long)V);
  MMFD_CHECK_ARG(ldl >= V, "mmfd_vocab_xent_fwd: leading dimension %lld < V = %lld", (long long)ldl, (long long)V);
  MMFD_CHECK_ARG(eps >= 0.f && eps <= 1.f, "mmfd_vocab_xent_fwd: smoothing %g outside [0, 1]", (double)eps);
  MMFD_CHECK_ARG(logits && labels && loss_rows && lse, "mmfd_vocab_xent_fwd: NULL logits / labels / loss_rows / lse");
  MMFD_CHECK_ARG((uintptr_t)logits % 16 == 0, "mmfd_vocab_xent_fwd: logits must be 16-byte aligned");
  MMFD_CHECK_ARG((uintptr_t)labels % 8 == 0 && (uintptr_t)loss_rows % 4 == 0 && (uintptr_t)lse % 4 == 0 &&
                     (uintptr_t)lse_lo % 4 == 0 && (uintptr_t)mean % 4 == 0 && (uintptr_t)n_valid % 8 == 0 && (uintptr_t)seq_sums % 4 == 0,
                 "mmfd_vocab_xent_fwd: labels / outputs are not aligned to their element size");
  MMFD_CHECK_ARG(!seq_sums || (rows_per_seq >= 1 && R % rows_per_seq == 0),
                 "mmfd_vocab_xent_fwd: rows_per_seq = %lld does not divide R = %lld", (long long)rows_per_seq, (long long)R);
  hipStream_t s = (hipStream_t)stream;
  if (ldl % 4 == 0)
    hipLaunchKernelGGL((vocab_xent_fwd_kernel<true>), dim3((unsigned)R), dim3(NT), 0, s, V, logits, ldl, labels, eps, loss_rows, lse,
                       lse_lo);
  else
    hipLaunchKernelGGL((vocab_xent_fwd_kernel<false>), dim3((unsigned)R), dim3(NT), 0, s, V, logits, ldl, labels, eps, loss_rows, lse,
                       lse_lo);
  MMFD_CHECK_LAUNCH("mmfd_vocab_xent_fwd");
  if (mean || n_valid || seq_sums) {
    hipLaunchKernelGGL(vocab_xent_reduce_kernel, dim3(1), dim3(NT), 0, s, R, V, rows_per_seq, labels, loss_rows, mean, n_valid,
                       seq_sums);
    MMFD_CHECK_LAUNCH("mmfd_vocab_xent_fwd (reduce)");
  }
  return 0;
}

extern "C" int mmfd_vocab_xent_bwd(int out_dtype, int64_t R, int64_t V, const float* logits, int64_t ldl,
                                   const int64_t* labels, const float* lse, const float* lse_lo, float eps,
                                   const float* upstream, const int64_t* n_valid, int64_t rows_per_seq, void* dlogits, int64_t ldd,
                                   mmfd_stream_t stream) {
  MMFD_CHECK_ARG(out_dtype == MMFD_F32 || out_dtype == MMFD_BF16, "mmfd_vocab_xent_bwd: bad dtype %d", out_dtype);
  MMFD_CHECK_ARG(R >= 1 && R <= 0x7fffffffLL, "mmfd_vocab_xent_bwd: R = %lld outside [1, 2^31)", (long long)R);
  MMFD_CHECK_ARG(V >= 1, "mmfd_vocab_xent_bwd: V = %lld must be >= 1", (long long)V);
  MMFD_CHECK_ARG(ldl >= V && ldd >= V, "mmfd_vocab_xent_bwd: leading dimensions %lld / %lld < V = %lld", (long long)ldl,
                 (long long)ldd, (long long)V);
  MMFD_CHECK_ARG(eps >= 0.f && eps <= 1.f, "mmfd_vocab_xent_bwd: smoothing %g outside [0, 1]", (double)eps);
  MMFD_CHECK_ARG(logits && labels && lse && dlogits, "mmfd_vocab_xent_bwd: NULL logits / labels / lse / dlogits");
  MMFD_CHECK_ARG(n_valid || (upstream && rows_per_seq >= 1 && R % rows_per_seq == 0),
                 "mmfd_vocab_xent_bwd: the per-sequence form needs upstream weights and rows_per_seq dividing R");
  MMFD_CHECK_ARG((uintptr_t)logits % 16 == 0 && (uintptr_t)dlogits % 16 == 0,
                 "mmfd_vocab_xent_bwd: logits and dlogits must be 16-byte aligned");
  MMFD_CHECK_ARG((uintptr_t)labels % 8 == 0 && (uintptr_t)lse % 4 == 0 && (uintptr_t)lse_lo % 4 == 0 &&
                     (uintptr_t)upstream % 4 == 0 &&
                     (uintptr_t)n_valid % 8 == 0,
                 "mmfd_vocab_xent_bwd: labels / lse / upstream / n_valid are not aligned to their element size");
  hipStream_t s = (hipStream_t)stream;
  const bool bf = out_dtype == MMFD_BF16;
  const bool vec = ldl % 4 == 0 && ldd % (bf ? 8 : 4) == 0;
#define LAUNCH(T, VEC)                                                                                              \
  hipLaunchKernelGGL((vocab_xent_bwd_kernel<T, VEC>), dim3((unsigned)R), dim3(NT), 0, s, V, logits, ldl, labels, lse, lse_lo, \
                     eps, upstream, n_valid, rows_per_seq, (T*)dlogits, ldd)
  if (bf) {
    if (vec) LAUNCH(bf16, true); else LAUNCH(bf16, false);
  } else {
    if (vec) LAUNCH(float, true); else LAUNCH(float, false);
  }
#undef LAUNCH
  MMFD_CHECK_LAUNCH("mmfd_vocab_xent_bwd");
  return 0;
}
