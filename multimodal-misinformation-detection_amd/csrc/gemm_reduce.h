// The extended epilogue (GELU_D / MUL_AUX / tanh / sigmoid) with the kernels that run it: the two
// split-K reduces and the plain FMA GEMM. Device code only, included by gemm.hip alone.
#pragma once
#include "gemm_tiles.h"

namespace {

// The epilogue activations MMFD_ACT_GELU_D (GELU, aux <- gelu'(z)) and MMFD_ACT_MUL_AUX (z *= aux)
// run in the four-wave kernel's register epilogue (gemm_g4.hip, the bf16 training FFN), and
// everywhere else in the split-K reduce / simple kernels only: a product with one of them that the
// four-wave kernel does not take writes its raw fp32 sums to a workspace slab (one split at least)
// and the reduce applies the whole epilogue. The tile kernels' shared epilogues (gemm_tiles.h) keep
// their round-5 code — the two extra activations inlined there made every GEMM's epilogue slower
// (config-5 extract −4 %, profiles/r06t_extract_regression.log).
// The forward-only tanh / sigmoid (the cross-encoder's pooler and score) go the same way: the tile
// kernels' epilogues carry only NONE / GELU / ReLU and their backward forms.
__device__ __host__ __forceinline__ bool act_ext(int act) {
  return act == MMFD_ACT_GELU_D || act == MMFD_ACT_MUL_AUX || act == MMFD_ACT_TANH || act == MMFD_ACT_SIGMOID;
}

// epilogue_store (gemm_tiles.h) with the two extra activations: bias, [residual first], the
// activation, then the unchanged tail (dropout, residual, beta, store / planes)
template <typename TC>
__device__ __forceinline__ void epilogue_store_x(const EpiArgs& e, TC* C, int64_t ldc, int64_t N, int64_t row,
                                                 int64_t col, float z, uint32_t hkey) {
  if (!act_ext(e.act)) return epilogue_store<TC>(e, C, ldc, N, row, col, z, hkey);
  if (e.bias) z += e.bias[col];
  if (e.res_first && e.residual) z += to_f32(reinterpret_cast<const TC*>(e.residual)[row * e.ldr + col]);
  TC* ax = reinterpret_cast<TC*>(e.aux) + row * e.ldaux + col;
  if (e.act == MMFD_ACT_GELU_D) {
    float d;
    z = gelu_and_grad_f(z, d);
    if (e.aux) *ax = from_f32<TC>(d);
  } else if (e.act == MMFD_ACT_MUL_AUX) {
    z *= to_f32(*ax);
  } else {
    z = act_tail_f(e.act, z);
  }
  EpiArgs t = e;
  t.act = MMFD_ACT_NONE; t.bias = nullptr;
  if (e.res_first) t.residual = nullptr;
  epilogue_store<TC>(t, C, ldc, N, row, col, z, hkey);
}

template <typename TC>
__device__ __forceinline__ void epilogue_store8_x(const EpiArgs& e, TC* C, int64_t ldc, int64_t N, int64_t row,
                                                  int64_t col, float (&z)[8], uint32_t hkey) {
  if (!act_ext(e.act)) return epilogue_store8<TC>(e, C, ldc, N, row, col, z, hkey);
  if (e.bias) {
    const float4 b0 = *reinterpret_cast<const float4*>(e.bias + col), b1 = *reinterpret_cast<const float4*>(e.bias + col + 4);
    z[0] += b0.x; z[1] += b0.y; z[2] += b0.z; z[3] += b0.w; z[4] += b1.x; z[5] += b1.y; z[6] += b1.z; z[7] += b1.w;
  }
  if (e.res_first && e.residual) {
    float r[8];
    V8<TC>::load(reinterpret_cast<const TC*>(e.residual) + row * e.ldr + col, r);
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] += r[q];
  }
  TC* ax = reinterpret_cast<TC*>(e.aux) + row * e.ldaux + col;
  if (e.act == MMFD_ACT_GELU_D) {
    float d[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = gelu_and_grad_f(z[q], d[q]);
    if (e.aux) V8<TC>::store(ax, d);
  } else if (e.act == MMFD_ACT_MUL_AUX) {
    float a[8];
    V8<TC>::load(ax, a);
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] *= a[q];
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) z[q] = act_tail_f(e.act, z[q]);
  }
  EpiArgs t = e;
  t.act = MMFD_ACT_NONE; t.bias = nullptr;
  if (e.res_first) t.residual = nullptr;
  epilogue_store8<TC>(t, C, ldc, N, row, col, z, hkey);
}

// split-K reduce, one output per thread (outputs that are not 16-B vectorisable; else splitk_reduce8_kernel)
template <typename TC>
__global__ void splitk_reduce_kernel(const float* __restrict__ ws, int splits, TC* __restrict__ C,
                                     int64_t ldc, int64_t M, int64_t N, EpiArgs e, const float* __restrict__ rs_part,
                                     int rs_nparts,
                                     float* __restrict__ rs_out, float rs_beta) {
  const uint32_t seed = (e.p > 0.0f) ? mmfd_hash_key(*e.seed, e.salt) : 0u;  // dropout hash key
  const int64_t total = M * N;
  if (rs_part) {  // the fused row sums' per-split partials (G8 split-K), summed in split order
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
      float t = 0.f;
      for (int s = 0; s < rs_nparts; ++s) t += rs_part[(int64_t)s * M + m];
      rs_out[m] = (rs_beta != 0.f ? rs_beta * rs_out[m] : 0.f) + t;
    }
  }
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    float z = 0.f;
    for (int s = 0; s < splits; ++s) z += ws[(int64_t)s * total + idx];
    epilogue_store_x<TC>(e, C, ldc, N, idx / N, idx % N, z, seed);
  }
}

// split-K reduce for 16-B-aligned outputs with N % 8 == 0: 8 consecutive outputs per thread group,
// the splits cut into P contiguous ranges summed by P threads (each in split order) and combined
// through LDS in range order — deterministic, and P x the threads of one-thread-per-8-outputs: a
// weight gradient's 768 x 768 output is 73,728 groups, 288 busy blocks on 256 CUs at P = 1 (the
// slab reads ran at ~1 TB/s), 2,304 at P = 8
template <typename TC, int P>
__global__ void __launch_bounds__(256) splitk_reduce8_kernel(const float* __restrict__ ws, int splits,
                                                             TC* __restrict__ C, int64_t ldc, int64_t M, int64_t N,
                                                             EpiArgs e, const float* __restrict__ rs_part,
                                                             int rs_nparts, float* __restrict__ rs_out, float rs_beta) {
  constexpr int G = 256 / P;  // output groups per block pass
  __shared__ float red[P > 1 ? P - 1 : 1][G][9];
  const uint32_t seed = (e.p > 0.0f) ? mmfd_hash_key(*e.seed, e.salt) : 0u;  // dropout hash key
  const int64_t total = M * N, groups = total / 8;
  if (rs_part) {  // the fused row sums' per-split partials (G8 split-K), summed in split order
    for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
      float t = 0.f;
      for (int s = 0; s < rs_nparts; ++s) t += rs_part[(int64_t)s * M + m];
      rs_out[m] = (rs_beta != 0.f ? rs_beta * rs_out[m] : 0.f) + t;
    }
  }
  const int gi = threadIdx.x % G, pi = threadIdx.x / G;
  const int per = (splits + P - 1) / P;
  const int s0 = pi * per, s1 = min(splits, s0 + per);
  for (int64_t gb = (int64_t)blockIdx.x * G; gb < groups; gb += (int64_t)gridDim.x * G) {
    const int64_t g = gb + gi;
    float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (g < groups) {
      const float* base = ws + g * 8;
      int s = s0;
      for (; s + 4 <= s1; s += 4) {  // four slabs' loads in flight before their adds (split order)
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float* q = base + (int64_t)(s + u) * total;
          a[u] = *reinterpret_cast<const float4*>(q);
          b[u] = *reinterpret_cast<const float4*>(q + 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          z[0] += a[u].x; z[1] += a[u].y; z[2] += a[u].z; z[3] += a[u].w;
          z[4] += b[u].x; z[5] += b[u].y; z[6] += b[u].z; z[7] += b[u].w;
        }
      }
      for (; s < s1; ++s) {
        const float* q = base + (int64_t)s * total;
        const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
        z[0] += a.x; z[1] += a.y; z[2] += a.z; z[3] += a.w; z[4] += b.x; z[5] += b.y; z[6] += b.z; z[7] += b.w;
      }
    }
    if constexpr (P > 1) {
      if (pi > 0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) red[pi - 1][gi][u] = z[u];
      }
      __syncthreads();
      if (pi == 0) {
#pragma unroll
        for (int q = 0; q < P - 1; ++q)
#pragma unroll
          for (int u = 0; u < 8; ++u) z[u] += red[q][gi][u];
      }
      __syncthreads();
    }
    if (pi == 0 && g < groups) epilogue_store8_x<TC>(e, C, ldc, N, (g * 8) / N, (g * 8) % N, z, seed);
  }
}

// Plain FMA GEMM for shapes the MFMA path cannot take (tiny / unaligned: classifier heads).
template <typename T, typename TC>
__global__ void gemm_simple_kernel(const T* __restrict__ A, int64_t lda, int ta, const T* __restrict__ B,
                                   int64_t ldb, int tb, TC* __restrict__ C, int64_t ldc, int64_t M,
                                   int64_t N, int64_t K, float alpha, EpiArgs e) {
  const uint32_t seed = (e.p > 0.0f) ? mmfd_hash_key(*e.seed, e.salt) : 0u;  // dropout hash key
  const int64_t total = M * N;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = idx / N, n = idx % N;
    float s = 0.f;
    for (int64_t k = 0; k < K; ++k) {
      const float a = to_f32(ta ? A[k * lda + m] : A[m * lda + k]);
      const float b = to_f32(tb ? B[k * ldb + n] : B[n * ldb + k]);
      s = fmaf(a, b, s);
    }
    epilogue_store_x<TC>(e, C, ldc, N, m, n, alpha * s, seed);
  }
}

}  // namespace
