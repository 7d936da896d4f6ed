// split3 (fp32 operand -> three bf16 planes), the column-sum partial kernels and the shared reduce of
// per-block partials (mmfd_reduce_partials_kernel, also launched by the LayerNorm backward). Device
// code only, included by gemm.hip alone: these kernels are built with that unit's flags.
#pragma once
#include "common.h"

namespace {

// fp32 operand -> three bf16 planes (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid),
// each difference exact in fp32): stored rows x cols (ld) -> planes [3][rows][cols]; 8 columns per
// thread (two 16-B loads, one 16-B store per plane), cols % 8 == 0
__global__ void __launch_bounds__(256) split3_kernel(const float* __restrict__ X, int64_t ldx, int64_t rows,
                                                     int64_t cols, bf16* __restrict__ P, int64_t plane) {
  // one 8-column chunk of one row per thread, grid-stride over all chunks (narrow rows — 768
  // columns = 96 chunks — keep every lane busy)
  const uint32_t c8 = (uint32_t)(cols / 8);
  const uint32_t total = (uint32_t)(rows * c8);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t r = i / c8;
    const int64_t c = (int64_t)(i - r * c8) * 8;
    const float* src = X + (int64_t)r * ldx + c;
    const float4 x0 = *reinterpret_cast<const float4*>(src);
    const float4 x1 = *reinterpret_cast<const float4*>(src + 4);
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    bf16x8 h, m, l;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bf16 hu = (bf16)x[u];
      const float r1 = x[u] - (float)hu;
      const bf16 mu = (bf16)r1;
      h[u] = hu;
      m[u] = mu;
      l[u] = (bf16)(r1 - (float)mu);
    }
    bf16* d = P + (int64_t)r * cols + c;
    *reinterpret_cast<uint4*>(d) = __builtin_bit_cast(uint4, h);
    *reinterpret_cast<uint4*>(d + plane) = __builtin_bit_cast(uint4, m);
    *reinterpret_cast<uint4*>(d + 2 * plane) = __builtin_bit_cast(uint4, l);
  }
}

// pass 1 (vector path): block = 4 waves x 64 lanes; a lane owns one 16-B chunk of columns, the 4
// waves stride over the block's row slab; the waves' partials are combined in LDS.
template <typename T>
__global__ void __launch_bounds__(256) colsum_partial_vec_kernel(const T* __restrict__ X, int64_t ldx, int64_t M,
                                                                 int64_t N, int64_t rows_per_block,
                                                                 float* __restrict__ part) {
  constexpr int EPC = 16 / sizeof(T);
  __shared__ float red[4][64 * EPC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col = ((int64_t)blockIdx.x * 64 + lane) * EPC;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  float acc[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
  if (col < N) {
    for (int64_t r = r0 + wave; r < r1; r += 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(X + r * ldx + col);
      const T* t = reinterpret_cast<const T*>(&v);
#pragma unroll
      for (int e = 0; e < EPC; ++e) acc[e] += to_f32(t[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < EPC; ++e) red[wave][lane * EPC + e] = acc[e];
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * EPC; i += 256) {
    const int64_t c = (int64_t)blockIdx.x * 64 * EPC + i;
    if (c < N) part[(int64_t)blockIdx.y * N + c] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
  }
}
template <typename T>
__global__ void colsum_partial_kernel(const T* __restrict__ X, int64_t ldx, int64_t M, int64_t N,
                                      int64_t rows_per_block, float* __restrict__ part) {
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= N) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  float s = 0.f;
  for (int64_t r = r0; r < r1; ++r) s += to_f32(X[r * ldx + col]);
  part[(int64_t)blockIdx.y * N + col] = s;
}

}  // namespace

// pass 2, shared with the LayerNorm backward: out[c] = beta*out[c] + sum_p part[p*stride + c];
// block = 64 columns x 16 waves splitting the partials (4 independent loads in flight per lane),
// combined through LDS in a fixed order (deterministic).
__global__ void __launch_bounds__(1024) mmfd_reduce_partials_kernel(const float* __restrict__ part, int nparts,
                                                                    int64_t stride, int64_t N, float* __restrict__ out,
                                                                    float beta) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + lane;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < N) {
    int p = wave;
    for (; p + 48 < nparts; p += 64) {
      s0 += part[(int64_t)p * stride + col];
      s1 += part[(int64_t)(p + 16) * stride + col];
      s2 += part[(int64_t)(p + 32) * stride + col];
      s3 += part[(int64_t)(p + 48) * stride + col];
    }
    for (; p < nparts; p += 16) s0 += part[(int64_t)p * stride + col];
  }
  red[wave][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (wave == 0 && col < N) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w][lane];
    out[col] = (beta != 0.f ? beta * out[col] : 0.f) + t;
  }
}
