// Logits processors for the one-token-per-step decoder (BLIP captioning, mmfd/blip.py): the edits transformers'
// `generate` makes to a row of scores before it selects — RepetitionPenaltyLogitsProcessor,
// NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor / MinNewTokensLengthLogitsProcessor and
// SuppressTokensLogitsProcessor (generation/logits_process.py) — applied on the device from the row's own
// history, and the row argmax the greedy step takes afterwards.
//
//   mmfd_logits_process  in place on fp32 scores [R][ldl], one workgroup per row. The row's history (cur_len ids,
//                        int64 or int32, any row / position stride) is staged in LDS once. Then
//     penalty  every id of the history, once: the lane of an id's FIRST occurrence reads the column, forms
//              s < 0 ? s * p : s / p (an IEEE division) and writes it back; the lanes of later occurrences do
//              nothing. No other lane touches that column before the barrier that follows, so the value is the
//              one transformers' gather-then-scatter leaves, whatever the order the lanes run in.
//     bans     -inf into: the last id of every window of n ids whose first n - 1 equal the history's last n - 1
//              (n <= cur_len; the window that would start at the suffix itself does not exist yet), eos when the
//              caller says so, and the ids of a device list. Several lanes may write the same -inf.
//              An id outside [0, V) touches nothing. At most cur_len + 1 + 64 columns of a row are touched and
//              nothing else of it is read.
//   mmfd_row_argmax      one workgroup per row: the largest number, ties to the lowest index, a NaN never over a
//                        number (the order of mmfd_lm_head_argmax; -inf counts as a number, a row of nothing but
//                        NaN gives 0).
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int LGT_THREADS = 256;
constexpr int LGT_MAX_LEN = 1024;      // history positions staged in LDS (8 KiB)
constexpr int LGT_MAX_SUPPRESS = 64;
constexpr int ARG_THREADS = 1024, ARG_WAVES = ARG_THREADS / 64;

struct LogitsParams {
  float* scores; int64_t ldl;
  const void* hist; int64_t hist_row, hist_pos;
  const int64_t* suppress;
  int hist_wide;  // 1: int64 ids, 0: int32
  int V, cur_len, ngram, n_suppress;
  int eos;        // < 0: not suppressed at this step
  int penalise;
  float penalty;
};

__global__ __launch_bounds__(LGT_THREADS) void logits_process_kernel(LogitsParams p) {
  __shared__ int64_t ids[LGT_MAX_LEN];
  const int tid = threadIdx.x, n = p.cur_len;
  const int64_t V = p.V;
  float* x = p.scores + (int64_t)blockIdx.x * p.ldl;
  for (int i = tid; i < n; i += LGT_THREADS) {
    const int64_t at = (int64_t)blockIdx.x * p.hist_row + (int64_t)i * p.hist_pos;
    ids[i] = p.hist_wide ? static_cast<const int64_t*>(p.hist)[at] : (int64_t) static_cast<const int32_t*>(p.hist)[at];
  }
  __syncthreads();
  if (p.penalise) {
    for (int i = tid; i < n; i += LGT_THREADS) {
      const int64_t id = ids[i];
      if (id < 0 || id >= V) continue;
      bool first = true;
      for (int j = 0; j < i; ++j)
        if (ids[j] == id) {
          first = false;
          break;
        }
      if (first) {
        const float s = x[id];
        x[id] = s < 0.f ? s * p.penalty : __fdiv_rn(s, p.penalty);
      }
    }
    __syncthreads();  // a banned column is banned after it was penalised, never before
  }
  const float ninf = -INFINITY;
  const int g = p.ngram;
  if (g > 0 && g <= n) {
    const int tail = n - (g - 1);  // the history's last g - 1 ids
    for (int i = tid; i + g <= n; i += LGT_THREADS) {
      bool same = true;
      for (int k = 0; k < g - 1; ++k)
        if (ids[i + k] != ids[tail + k]) {
          same = false;
          break;
        }
      const int64_t id = ids[i + g - 1];
      if (same && id >= 0 && id < V) x[id] = ninf;
    }
  }
  if (tid == 0 && p.eos >= 0 && p.eos < V) x[p.eos] = ninf;
  for (int i = tid; i < p.n_suppress; i += LGT_THREADS) {
    const int64_t id = p.suppress[i];
    if (id >= 0 && id < V) x[id] = ninf;
  }
}

// the candidates' order of beam.hip as one 64-bit key: the score's bits mapped monotonically (NaN -> 0, -0 -> +0)
// above ~index, so the unsigned maximum is the largest number at its lowest index
__device__ __forceinline__ uint64_t arg_key(float v, int index) {
  uint32_t k = 0u;
  if (v == v) {
    v += 0.0f;
    const uint32_t u = __float_as_uint(v);
    k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((uint64_t)k << 32) | (uint64_t)(0xffffffffu - (uint32_t)index);
}
__device__ __forceinline__ uint64_t u64_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

__global__ __launch_bounds__(ARG_THREADS) void row_argmax_kernel(const float* __restrict__ scores, int64_t ldl, int V,
                                                                 int64_t* __restrict__ out) {
  __shared__ uint64_t sh[ARG_WAVES];
  const int tid = threadIdx.x;
  const float* x = scores + (int64_t)blockIdx.x * ldl;
  // scalar entries up to the first 16-byte boundary, 16-byte loads, a scalar tail
  const int head = min(V, (int)((4u - (uint32_t)(((uintptr_t)x >> 2) & 3u)) & 3u));
  const int nv = (V - head) >> 2;
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  uint64_t best = 0ull;
  if (tid < head) best = arg_key(x[tid], tid);
#pragma unroll 4
  for (int i = tid; i < nv; i += ARG_THREADS) {
    const float4 v = xv[i];
    const int at = head + 4 * i;
    best = u64_max(best, u64_max(u64_max(arg_key(v.x, at), arg_key(v.y, at + 1)),
                                 u64_max(arg_key(v.z, at + 2), arg_key(v.w, at + 3))));
  }
  for (int i = head + 4 * nv + tid; i < V; i += ARG_THREADS) best = u64_max(best, arg_key(x[i], i));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = u64_max(best, (uint64_t)__shfl_xor((unsigned long long)best, o, 64));
  if ((tid & 63) == 0) sh[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < ARG_WAVES; ++w) best = u64_max(best, sh[w]);
    out[blockIdx.x] = (int64_t)(0xffffffffu - (uint32_t)best);  // (V >= 1: some entry always set a key)
  }
}

}  // namespace

extern "C" int mmfd_logits_process(int64_t R, int64_t V, float* scores, int64_t ldl, const void* history,
                                   int64_t hist_row_stride, int64_t hist_pos_stride, int hist_elem_bytes,
                                   int64_t cur_len, float penalty, int64_t ngram, int suppress_eos, int64_t eos,
                                   const int64_t* suppress, int64_t n_suppress, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(R >= 1 && R <= INT_MAX, "mmfd_logits_process: R = %lld rows", (long long)R);
  MMFD_CHECK_ARG(V >= 1 && V < (1 << 30), "mmfd_logits_process: V = %lld", (long long)V);
  MMFD_CHECK_ARG(scores && history, "mmfd_logits_process: null pointer");
  MMFD_CHECK_ARG(ldl >= V, "mmfd_logits_process: leading dimension too small");
  MMFD_CHECK_ARG(hist_elem_bytes == 8 || hist_elem_bytes == 4,
                 "mmfd_logits_process: the history holds int64 (8) or int32 (4) ids, got %d bytes", hist_elem_bytes);
  MMFD_CHECK_ARG(hist_row_stride >= 0 && hist_pos_stride >= 1, "mmfd_logits_process: bad history strides");
  MMFD_CHECK_ARG(cur_len >= 1 && cur_len <= LGT_MAX_LEN, "mmfd_logits_process: cur_len = %lld (1 .. %d)",
                 (long long)cur_len, LGT_MAX_LEN);
  MMFD_CHECK_ARG(penalty > 0.f && std::isfinite(penalty), "mmfd_logits_process: repetition_penalty must be finite and > 0");
  MMFD_CHECK_ARG(ngram >= 0, "mmfd_logits_process: no_repeat_ngram_size = %lld (0: off)", (long long)ngram);
  MMFD_CHECK_ARG(!suppress_eos || (eos >= 0 && eos < V), "mmfd_logits_process: eos = %lld outside [0, V)", (long long)eos);
  MMFD_CHECK_ARG(n_suppress >= 0 && n_suppress <= LGT_MAX_SUPPRESS && (n_suppress == 0 || suppress),
                 "mmfd_logits_process: %lld suppressed ids (0 .. %d, with their list)", (long long)n_suppress,
                 LGT_MAX_SUPPRESS);
  LogitsParams p;
  p.scores = scores; p.ldl = ldl;
  p.hist = history; p.hist_row = hist_row_stride; p.hist_pos = hist_pos_stride; p.hist_wide = hist_elem_bytes == 8;
  p.suppress = suppress; p.n_suppress = (int)n_suppress;
  p.V = (int)V; p.cur_len = (int)cur_len;
  p.ngram = (int)(ngram > cur_len ? 0 : ngram);  // (no window of more ids than the history holds)
  p.eos = suppress_eos ? (int)eos : -1;
  p.penalise = penalty != 1.0f; p.penalty = penalty;
  hipLaunchKernelGGL(logits_process_kernel, dim3((unsigned)R), dim3(LGT_THREADS), 0, (hipStream_t)stream, p);
  MMFD_CHECK_LAUNCH("mmfd_logits_process");
  return 0;
}

extern "C" int mmfd_row_argmax(int64_t R, int64_t V, const float* scores, int64_t ldl, int64_t* out_idx,
                               mmfd_stream_t stream) {
  MMFD_CHECK_ARG(R >= 1 && R <= INT_MAX, "mmfd_row_argmax: R = %lld rows", (long long)R);
  MMFD_CHECK_ARG(V >= 1 && V < (1 << 30), "mmfd_row_argmax: V = %lld", (long long)V);
  MMFD_CHECK_ARG(scores && out_idx, "mmfd_row_argmax: null pointer");
  MMFD_CHECK_ARG(ldl >= V, "mmfd_row_argmax: leading dimension too small");
  MMFD_CHECK_ARG(((uintptr_t)scores & 3) == 0, "mmfd_row_argmax: scores must be 4-byte aligned");
  hipLaunchKernelGGL(row_argmax_kernel, dim3((unsigned)R), dim3(ARG_THREADS), 0, (hipStream_t)stream, scores, ldl,
                     (int)V, out_idx);
  MMFD_CHECK_LAUNCH("mmfd_row_argmax");
  return 0;
}
