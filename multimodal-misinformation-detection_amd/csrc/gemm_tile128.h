// The 256x128 tile kernel (gemm_mfma_body) and its three __global__ wrappers: the plain GEMM, the
// 256x64 tile for N <= 64 and the implicit-GEMM convolution. Device code only, included by gemm.hip alone.
#pragma once
#include "gemm_tiles.h"

namespace {

// CONV: implicit-GEMM convolution (ConvGeom): A is the NHWC activation and its fill gathers the
// im2col rows per K-tile (ConvFill); TA = 0 only. The body is shared by gemm_mfma_kernel and
// conv_mfma_kernel (two kernel names, so the plain GEMM's name in traces stays what it was).
// BNT: the tile's N width — 128, or 64 for N <= 64 (the ResNet stem / layer1 convolutions: a 128-wide
// tile spent half its MFMAs on zero columns); BNT = 64 takes K-contiguous B only (TB = 0)
template <typename T, int TA, int TB, typename TC, bool CONV, int BNT = BN>
__device__ __forceinline__ void
gemm_mfma_body(const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb,
               TC* __restrict__ C, int64_t ldc, float* __restrict__ ws, int64_t M, int64_t N,
               int64_t K, float alpha, int tiles_per_split, const EpiArgs& e, const ConvGeom& cg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(BNT == BN || (BNT == 64 && TB == 0), "the 64-wide tile takes K-contiguous B only");
  constexpr int BBYTES = BNT * ROWB, SBYTES = A_BYTES + BBYTES;  // B image, one stage
  constexpr int WNS = BNT / 32;                     // 16-column subtiles per wave (2 wave columns)
  constexpr int APIECES = A_BYTES / 1024 / NWAVES;  // 4 pieces per wave
  constexpr int BPIECES = BBYTES / 1024 / NWAVES;   // 2 (1 for BNT = 64) pieces per wave
  constexpr int PIECES = APIECES + BPIECES;         // DMA instructions per wave per tile

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int gx = gridDim.x, gy = gridDim.y;
  const int lin = blockIdx.y * gx + blockIdx.x;
  const int tile = xcd_remap(lin, gx * gy);
  const int tm = tile / gx, tn = tile % gx;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BNT;

  const int nkt_total = (int)((K + GT<T>::BK - 1) / GT<T>::BK);
  const int kt0 = blockIdx.z * tiles_per_split;
  const int nk = min(nkt_total, kt0 + tiles_per_split) - kt0;

  f32x4 acc[4][WNS];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < WNS; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t a_bytes = CONV ? cg.H * cg.W * cg.C * (M / (cg.Ho * cg.Wo)) * (int64_t)sizeof(T)
                               : (TA == 0 ? M : K) * lda * (int64_t)sizeof(T);
  const __amdgpu_buffer_rsrc_t rsa = make_rsrc(A, a_bytes);
  const __amdgpu_buffer_rsrc_t rsb = make_rsrc(B, (TB == 0 ? N : K) * ldb * (int64_t)sizeof(T));
  std::conditional_t<CONV, ConvFill<T, APIECES>, Fill<T, TA, BM, APIECES>> fa;
  Fill<T, TB, BNT, BPIECES> fb;
  if constexpr (CONV) fa.init(cg, m0, M, wave, lane);
  else fa.init(lda, m0, M, wave, lane);
  fb.init(ldb, n0, N, wave, lane);

  auto issue = [&](int t) {
    const int64_t k0 = (int64_t)(kt0 + t) * GT<T>::BK;
    const bool tail = k0 + GT<T>::BK > K;
    char* st = smem + (t % NSTAGE) * SBYTES;
    if constexpr (CONV) fa.issue(rsa, st, cg, k0, K, wave);
    else fa.issue(rsa, st, (uint32_t)(k0 * (TA == 0 ? 1 : lda) * (int64_t)sizeof(T)), tail, k0, K, wave, lane);
    fb.issue(rsb, st + A_BYTES, (uint32_t)(k0 * (TB == 0 ? 1 : ldb) * (int64_t)sizeof(T)), tail, k0, K, wave, lane);
  };

  if (nk > 0) issue(0);
  if (nk > 1) issue(1);
  for (int t = 0; t < nk; ++t) {
    // tile t landed (keep tile t+1 in flight); the barrier also retires every wave's reads of the
    // stage about to be refilled (tile t-1)
    if (t + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 2 < nk) issue(t + 2);
    const char* la = smem + (t % NSTAGE) * SBYTES;
    const char* lb = la + A_BYTES;
#pragma unroll
    for (int kc = 0; kc < GT<T>::KCH; ++kc) {
      uint4 xa[4], xb[WNS];
#pragma unroll
      for (int i = 0; i < 4; ++i) xa[i] = load_frag<T, TA, BM>(la, wm * 4 + i, kc, lane);
#pragma unroll
      for (int j = 0; j < WNS; ++j) xb[j] = load_frag<T, TB, BNT>(lb, wn * WNS + j, kc, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WNS; ++j) Mma<T>::run(acc[i][j], xa[i], xb[j]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- epilogue: stage the 256x128 fp32 tile through LDS in four 64-row quarters (one wave row
  // each), then every thread handles 4 consecutive columns of a row (coalesced stores).
  constexpr int LDC = BNT + 4;
  float* ct = reinterpret_cast<float*>(smem);
  const int g = lane >> 4, ci = lane & 15;
  const uint32_t seed = (!ws && e.p > 0.0f) ? mmfd_hash_key(*e.seed, e.salt) : 0u;  // dropout hash key
  float* slab = ws ? ws + (int64_t)blockIdx.z * M * N : nullptr;
#pragma unroll
  for (int qtr = 0; qtr < 4; ++qtr) {
    if (wm == qtr) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < WNS; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) ct[(i * 16 + 4 * g + r) * LDC + wn * (BNT / 2) + j * 16 + ci] = acc[i][j][r];
    }
    __syncthreads();
    // 64 rows x BNT/8 groups of 8 columns
    for (int idx = tid; idx < 64 * (BNT / 8); idx += NT) {
      const int lr = idx / (BNT / 8), c8 = (idx % (BNT / 8)) * 8;
      const int64_t row = m0 + qtr * 64 + lr;
      const int64_t col = n0 + c8;
      if (row >= M || col >= N) continue;
      const float* src = ct + lr * LDC + c8;
      const float4 a4 = *reinterpret_cast<const float4*>(src), b4 = *reinterpret_cast<const float4*>(src + 4);
      float vv[8] = {alpha * a4.x, alpha * a4.y, alpha * a4.z, alpha * a4.w,
                     alpha * b4.x, alpha * b4.y, alpha * b4.z, alpha * b4.w};
      const bool full = col + 8 <= N;
      if (slab) {
        if (full && (N % 4) == 0) {
          *reinterpret_cast<float4*>(slab + row * N + col) = make_float4(vv[0], vv[1], vv[2], vv[3]);
          *reinterpret_cast<float4*>(slab + row * N + col + 4) = make_float4(vv[4], vv[5], vv[6], vv[7]);
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q)
            if (col + q < N) slab[row * N + col + q] = vv[q];
        }
      } else if (full && e.vec) {
        epilogue_store8<TC>(e, C, ldc, N, row, col, vv, seed);
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (col + q < N) epilogue_store<TC>(e, C, ldc, N, row, col + q, vv[q], seed);
      }
    }
    __syncthreads();
  }
}


template <typename T, int TA, int TB, typename TC>
__global__ void __launch_bounds__(NT, 1)
gemm_mfma_kernel(const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb,
                 TC* __restrict__ C, int64_t ldc, float* __restrict__ ws, int64_t M, int64_t N,
                 int64_t K, float alpha, int tiles_per_split, EpiArgs e) {
  gemm_mfma_body<T, TA, TB, TC, false>(A, lda, B, ldb, C, ldc, ws, M, N, K, alpha, tiles_per_split, e, ConvGeom{});
}
// the 256x64 tile for N <= 64 with K-contiguous B
template <typename T, int TA, typename TC>
__global__ void __launch_bounds__(NT, 1)
gemm_mfma_n64_kernel(const T* __restrict__ A, int64_t lda, const T* __restrict__ B, int64_t ldb,
                     TC* __restrict__ C, int64_t ldc, float* __restrict__ ws, int64_t M, int64_t N,
                     int64_t K, float alpha, int tiles_per_split, EpiArgs e) {
  gemm_mfma_body<T, TA, 0, TC, false, 64>(A, lda, B, ldb, C, ldc, ws, M, N, K, alpha, tiles_per_split, e, ConvGeom{});
}
// implicit-GEMM convolution on the 256x128 kernel (mmfd_gemm_args.conv): A = the NHWC activation
template <typename T, typename TC, int BNT>
__global__ void __launch_bounds__(NT, 1)
conv_mfma_kernel(const T* __restrict__ X, const T* __restrict__ B, int64_t ldb, TC* __restrict__ C, int64_t ldc,
                 float* __restrict__ ws, int64_t M, int64_t N, int64_t K, float alpha, int tiles_per_split, EpiArgs e,
                 ConvGeom cg) {
  gemm_mfma_body<T, 0, 0, TC, true, BNT>(X, cg.C, B, ldb, C, ldc, ws, M, N, K, alpha, tiles_per_split, e, cg);
}

}  // namespace
