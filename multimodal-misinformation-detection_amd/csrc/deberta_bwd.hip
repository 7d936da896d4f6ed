// DeBERTa-v3 training helpers: the adjoints of mmfd_deberta_rel_bias and mmfd_attn_fill_masked_rows
// (misc.hip; transformers modeling_deberta_v2.py disentangled_attention_bias :276-346 and the
// masked_fill + softmax semantics of a fully padded query row :252-256).
//
// mmfd_deberta_rel_bias_bwd: the forward gathers out[b][h][i][j] = inv * c2p[h][b*L+i][c2p_idx[i][j]] +
// inv * p2c[h][b*L+j][p2c_idx[j][i]], so the adjoint scatters dS back:
//   dc2p[h][b*L+i][s] = inv * sum_{j : c2p_idx[i][j] == s} ds[b][h][i][j]
//   dp2c[h][b*L+j][s] = inv * sum_{i : p2c_idx[j][i] == s} ds[b][h][i][j]
// Both index maps are monotone along the summed index (log-bucket relative positions; the Python
// wrapper checks it once per (L, S) on the host), so every output element is the sum of ONE
// contiguous run: the thread at the start of a run sums it in index order and is the only writer
// of that element — deterministic, no atomics. A workgroup owns 16 "owner" rows (queries i for
// dc2p, keys j for dp2c) of one (b, h) with their whole fp32 output rows [16][ld] in LDS, and
// streams the summed index in chunks of 64 through an LDS tile, so global reads of dS stay
// row-contiguous in both halves (dp2c reads 16 consecutive keys of 64 query rows and sums down the
// tile's columns). A run cut by a chunk boundary continues from the value in LDS, which keeps the
// summation order strictly ascending.
#include "common.h"
#include <algorithm>

namespace {
inline unsigned gridn(int64_t n, int per) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 16384));
}

constexpr int RBB_OWN = 16, RBB_CH = 64;

template <typename T, bool P2C>
__global__ void __launch_bounds__(256) deberta_rel_bias_bwd_kernel(int64_t B, int64_t H, int64_t L,
                                                                   const float* __restrict__ ds,
                                                                   const int32_t* __restrict__ idx, float inv_scale,
                                                                   T* __restrict__ out, int ld) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* acc = reinterpret_cast<float*>(smem);        // [RBB_OWN][ld]
  float* tile = acc + RBB_OWN * ld;                    // [RBB_OWN][RBB_CH + 1]
  constexpr int TS = RBB_CH + 1;
  const int t = threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * RBB_OWN;
  const int64_t bh = blockIdx.y, b = bh / H, h = bh % H;
  const float* dsb = ds + bh * L * L;
  for (int e = t; e < RBB_OWN * ld; e += 256) acc[e] = 0.f;
  for (int64_t c0 = 0; c0 < L; c0 += RBB_CH) {
    __syncthreads();  // the previous chunk's readers are done with the tile (and acc is zeroed)
    if (P2C) {  // owner = key j (16 consecutive floats of a dS row), streamed = query i
      const int o = t % RBB_OWN;
#pragma unroll
      for (int k = 0; k < RBB_CH / (256 / RBB_OWN); ++k) {
        const int c = t / RBB_OWN + k * (256 / RBB_OWN);
        const int64_t i = c0 + c, j = o0 + o;
        tile[o * TS + c] = (i < L && j < L) ? dsb[i * L + j] : 0.f;
      }
    } else {    // owner = query i (one dS row), streamed = key j
      const int c = t % RBB_CH;
#pragma unroll
      for (int k = 0; k < RBB_OWN / (256 / RBB_CH); ++k) {
        const int o = t / RBB_CH + k * (256 / RBB_CH);
        const int64_t i = o0 + o, j = c0 + c;
        tile[o * TS + c] = (i < L && j < L) ? dsb[i * L + j] : 0.f;
      }
    }
    __syncthreads();
    // 16 x 64 (owner, streamed) pairs, 4 per thread: the start of a run inside this chunk sums it
#pragma unroll
    for (int k = 0; k < RBB_OWN * RBB_CH / 256; ++k) {
      const int e = t + k * 256, o = e / RBB_CH, c = e % RBB_CH;
      const int64_t own = o0 + o, pos = c0 + c;
      if (own >= L || pos >= L) continue;
      const int32_t* row = idx + own * L;
      const int32_t s = row[pos];
      if (c > 0 && row[pos - 1] == s) continue;       // not a run start
      if ((uint32_t)s >= (uint32_t)ld) continue;      // (indices are < ld: checked by the caller)
      float a = acc[o * ld + s];
      for (int u = c; u < RBB_CH && c0 + u < L && row[c0 + u] == s; ++u) a += tile[o * TS + u];
      acc[o * ld + s] = a;
    }
  }
  __syncthreads();
  for (int e = t; e < RBB_OWN * ld; e += 256) {
    const int o = e / ld, s = e % ld;
    const int64_t own = o0 + o;
    if (own < L) out[((h * B + b) * L + own) * ld + s] = from_f32<T>(acc[e] * inv_scale);
  }
}

// Fully padded query rows (mask[b][i] == 0) of the forward are o[b][i] = mean_j v[b][j] over all L
// keys. Phase 0, before mmfd_attn_bwd: gsum[b][h*Dh + d] = (1/L) * sum_{i padded} dO[b][i][h][d]
// (fp32, fixed order) and those dO rows are zeroed, so the attention backward sees no gradient
// for them. One block per (b, h), as the forward.
template <typename T>
__global__ void __launch_bounds__(256) fill_masked_rows_bwd_reduce_kernel(int64_t H, int64_t L, int64_t Dh,
                                                                          T* __restrict__ dout, int64_t do_sb,
                                                                          int64_t do_st,
                                                                          const int64_t* __restrict__ mask,
                                                                          float* __restrict__ gsum) {
  const int64_t b = blockIdx.x / H, h = blockIdx.x % H;
  __shared__ float part[4][64];
  const int d = threadIdx.x & 63, rg = threadIdx.x >> 6;
  float s = 0.f;
  if (d < Dh)
    for (int64_t i = rg; i < L; i += 4)
      if (mask[b * L + i] == 0) {
        T* p = dout + b * do_sb + i * do_st + h * Dh + d;
        s += to_f32(*p);
        *p = from_f32<T>(0.f);
      }
  part[rg][d] = s;
  __syncthreads();
  if (rg == 0 && d < Dh)
    gsum[(b * H + h) * Dh + d] = (part[0][d] + part[1][d] + part[2][d] + part[3][d]) / (float)L;
}

// Phase 1, after mmfd_attn_bwd: dv[b][j][h][:] += gsum[b][h][:] for every key j, padded keys included
template <typename T>
__global__ void fill_masked_rows_bwd_add_kernel(int64_t B, int64_t H, int64_t L, int64_t Dh, T* __restrict__ dv,
                                                int64_t dv_sb, int64_t dv_st, const float* __restrict__ gsum) {
  const int64_t W = H * Dh, total = B * L * W;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = e % W, r = e / W, b = r / L, j = r % L;
    T* p = dv + b * dv_sb + j * dv_st + c;
    *p = from_f32<T>(to_f32(*p) + gsum[b * W + c]);
  }
}

}  // namespace

extern "C" int mmfd_deberta_rel_bias_bwd(int dtype, int64_t B, int64_t H, int64_t L, const float* ds,
                                         const int32_t* c2p_idx, const int32_t* p2c_idx, float inv_scale, void* dc2p,
                                         void* dp2c, int64_t ld, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(B >= 0 && H > 0 && L >= 0 && ld > 0, "deberta_rel_bias_bwd: bad shape");
  MMFD_CHECK_ARG(dtype == MMFD_F32 || dtype == MMFD_BF16, "deberta_rel_bias_bwd: bad dtype");
  if (B * H * L == 0) return 0;
  MMFD_CHECK_ARG(ds && c2p_idx && p2c_idx && dc2p && dp2c, "deberta_rel_bias_bwd: null pointer");
  MMFD_CHECK_ARG(B * H < 65536 && L < (1 << 20), "deberta_rel_bias_bwd: grid too large");
  const int64_t lds = (RBB_OWN * ld + RBB_OWN * (RBB_CH + 1)) * 4;
  MMFD_CHECK_ARG(lds <= 64 * 1024, "deberta_rel_bias_bwd: ld %lld too wide (16 output rows must fit 64 KB of LDS)",
                 (long long)ld);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((L + RBB_OWN - 1) / RBB_OWN), (unsigned)(B * H));
  if (dtype == MMFD_BF16) {
    hipLaunchKernelGGL((deberta_rel_bias_bwd_kernel<bf16, false>), grid, dim3(256), lds, s, B, H, L, ds, c2p_idx,
                       inv_scale, (bf16*)dc2p, (int)ld);
    hipLaunchKernelGGL((deberta_rel_bias_bwd_kernel<bf16, true>), grid, dim3(256), lds, s, B, H, L, ds, p2c_idx,
                       inv_scale, (bf16*)dp2c, (int)ld);
  } else {
    hipLaunchKernelGGL((deberta_rel_bias_bwd_kernel<float, false>), grid, dim3(256), lds, s, B, H, L, ds, c2p_idx,
                       inv_scale, (float*)dc2p, (int)ld);
    hipLaunchKernelGGL((deberta_rel_bias_bwd_kernel<float, true>), grid, dim3(256), lds, s, B, H, L, ds, p2c_idx,
                       inv_scale, (float*)dp2c, (int)ld);
  }
  MMFD_CHECK_LAUNCH("deberta_rel_bias_bwd");
  return 0;
}

extern "C" int mmfd_attn_fill_masked_rows_bwd(int dtype, int phase, int64_t B, int64_t H, int64_t L, int64_t Dh,
                                              void* dout, int64_t do_sb, int64_t do_st, void* dv, int64_t dv_sb,
                                              int64_t dv_st, const int64_t* mask, float* gsum,
                                              mmfd_stream_t stream) {
  MMFD_CHECK_ARG(B >= 0 && H > 0 && L >= 0 && Dh > 0 && Dh <= 64, "attn_fill_masked_rows_bwd: bad shape (Dh <= 64)");
  MMFD_CHECK_ARG(dtype == MMFD_F32 || dtype == MMFD_BF16, "attn_fill_masked_rows_bwd: bad dtype");
  MMFD_CHECK_ARG(phase == 0 || phase == 1, "attn_fill_masked_rows_bwd: phase %d (0 = reduce and zero, 1 = add)", phase);
  if (B * L == 0) return 0;
  MMFD_CHECK_ARG(gsum, "attn_fill_masked_rows_bwd: null gsum");
  hipStream_t s = (hipStream_t)stream;
  if (phase == 0) {
    MMFD_CHECK_ARG(dout && mask, "attn_fill_masked_rows_bwd: null pointer");
    MMFD_CHECK_ARG(B * H < (1ll << 31), "attn_fill_masked_rows_bwd: grid too large");
    if (dtype == MMFD_BF16)
      hipLaunchKernelGGL((fill_masked_rows_bwd_reduce_kernel<bf16>), dim3((unsigned)(B * H)), dim3(256), 0, s, H, L, Dh,
                         (bf16*)dout, do_sb, do_st, mask, gsum);
    else
      hipLaunchKernelGGL((fill_masked_rows_bwd_reduce_kernel<float>), dim3((unsigned)(B * H)), dim3(256), 0, s, H, L, Dh,
                         (float*)dout, do_sb, do_st, mask, gsum);
  } else {
    MMFD_CHECK_ARG(dv, "attn_fill_masked_rows_bwd: null pointer");
    const unsigned grid = gridn(B * L * H * Dh, 256);
    if (dtype == MMFD_BF16)
      hipLaunchKernelGGL((fill_masked_rows_bwd_add_kernel<bf16>), dim3(grid), dim3(256), 0, s, B, H, L, Dh, (bf16*)dv,
                         dv_sb, dv_st, gsum);
    else
      hipLaunchKernelGGL((fill_masked_rows_bwd_add_kernel<float>), dim3(grid), dim3(256), 0, s, B, H, L, Dh, (float*)dv,
                         dv_sb, dv_st, gsum);
  }
  MMFD_CHECK_LAUNCH("attn_fill_masked_rows_bwd");
  return 0;
}
