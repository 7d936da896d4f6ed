// Beam search for the one-token-per-step decoder (BLIP captioning, mmfd/blip.py): what a beam step needs
// beside the greedy decoder's kernels (decode.hip). transformers' GenerationMixin._beam_search is the rule.
//
//   mmfd_beam_select    per image the 2 nb best (score, beam, token) of the nb * V candidates, score =
//                       log_softmax(logits[row])[token] + running[row]. Three kernels: (a) every workgroup
//                       leaves the {max, sum exp} of one slab of one row; (b) every workgroup combines its
//                       row's partials into the log-sum-exp, scores its slab and leaves the slab's 2 nb best;
//                       (c) one workgroup per image merges the lists of its nb rows.
//   mmfd_row_log_softmax, mmfd_beam_select_logprobs   the same selection cut in two for the logits processors
//                       (logits.hip), which transformers applies to log_softmax(logits) of every running beam
//                       before the running score is added: (a) and an in-place x - lse over the same slabs with
//                       the same log-sum-exp, then — after the edits — (b) without a second normalisation and (c).
//                       An unedited entry scores bit for bit what mmfd_beam_select gives it.
//   mmfd_beam_update    one workgroup per image: the next running beams, the finished hypotheses, the early-stop
//                       heuristic, the parent row of every beam and the token the next step embeds.
//   mmfd_beam_reorder   the self-attention caches of all layers gathered by parent row into a second set of
//                       buffers (one launch; never reads what it wrote).
//
// Order among candidates: a larger score first, equal scores by the lower flat index (beam * V + token), a NaN
// after every number (NaNs among themselves by index). A candidate is one 64-bit key — the score's bits
// mapped monotonically into the high word (NaN -> 0), ~index in the low word — so "the best candidate after
// the previous winner" is a plain unsigned maximum over keys below the previous key: the selections need no
// marks and no sorting network. Nothing hands data between workgroups inside a launch.
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int BEAM_THREADS = 256, BEAM_WAVES = BEAM_THREADS / 64;
constexpr int BEAM_MAX_NB = 8, BEAM_MAX_SLAB = 1024, BEAM_PER_THREAD = BEAM_MAX_SLAB / BEAM_THREADS;
constexpr int BEAM_MAX_T = 512;

// slab: vocabulary entries per workgroup of kernels (a) and (b): a quarter of the row in multiples of 64,
// at most 1024 (four values per thread, held in registers between the passes)
int beam_slab(int64_t V) {
  const int64_t q = ((V + 3) / 4 + 63) / 64 * 64;
  return (int)(q < 64 ? 64 : q > BEAM_MAX_SLAB ? BEAM_MAX_SLAB : q);
}

__device__ __forceinline__ uint32_t beam_float_key(float v) {
  if (v != v) return 0u;
  v += 0.0f;  // -0 -> +0: they compare equal, so they share a key
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // -inf -> 0x007fffff: above the NaN key
}
__device__ __forceinline__ float beam_key_float(uint32_t k) {
  if (k == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ uint64_t beam_key(float v, uint32_t index) {
  return ((uint64_t)beam_float_key(v) << 32) | (uint64_t)(0xffffffffu - index);
}
__device__ __forceinline__ uint32_t beam_key_index(uint64_t k) { return 0xffffffffu - (uint32_t)k; }

// workgroup reductions over BEAM_THREADS threads; `sh` holds BEAM_WAVES values and is free again on return
__device__ __forceinline__ uint64_t wg_max_u64(uint64_t v, uint64_t* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t other = __shfl_xor((unsigned long long)v, o, 64);
    v = other > v ? other : v;
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t r = sh[0];
#pragma unroll
  for (int w = 1; w < BEAM_WAVES; ++w) r = sh[w] > r ? sh[w] : r;
  __syncthreads();
  return r;
}
template <bool MAX> __device__ __forceinline__ float wg_reduce_f(float v, float* sh) {
  v = MAX ? wave_max(v) : wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int w = 1; w < BEAM_WAVES; ++w) r = MAX ? fmaxf(r, sh[w]) : r + sh[w];
  __syncthreads();
  return r;
}

// (a) grid (S, R): {max, sum exp(x - max)} over the numbers of one slab of one row (a NaN logit is left out: it
// can never be selected, and it does not take the row's other candidates with it)
__global__ __launch_bounds__(BEAM_THREADS) void beam_partial_kernel(const float* __restrict__ logits, int64_t ldl,
                                                                     int V, int slab, float* __restrict__ pm,
                                                                     float* __restrict__ ps) {
  __shared__ float sh[BEAM_WAVES];
  const int row = blockIdx.y, S = gridDim.x;
  const int lo = blockIdx.x * slab, hi = min(V, lo + slab);
  const float* x = logits + (int64_t)row * ldl;
  float v[BEAM_PER_THREAD];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < BEAM_PER_THREAD; ++j) {
    const int i = lo + threadIdx.x + j * BEAM_THREADS;
    v[j] = i < hi ? x[i] : __uint_as_float(0x7fc00000u);
    if (v[j] == v[j]) m = fmaxf(m, v[j]);
  }
  m = wg_reduce_f<true>(m, sh);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < BEAM_PER_THREAD; ++j)
    if (v[j] == v[j] && v[j] != -INFINITY) s += expf(v[j] - m);
  s = wg_reduce_f<false>(s, sh);
  if (threadIdx.x == 0) {
    pm[(int64_t)row * S + blockIdx.x] = m;
    ps[(int64_t)row * S + blockIdx.x] = s;
  }
}

// the row's log-sum-exp from its S partials: every thread of every workgroup of the row adds them in the same
// order, so the whole row is scored against one value
__device__ __forceinline__ float beam_row_lse(const float* __restrict__ pm, const float* __restrict__ ps, int row,
                                              int S) {
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, pm[(int64_t)row * S + s]);
  float sum = 0.f;
  for (int s = 0; s < S; ++s) {
    const float m = pm[(int64_t)row * S + s];
    if (m != -INFINITY) sum += ps[(int64_t)row * S + s] * expf(m - M);
  }
  return M + logf(sum);
}

// (b) grid (S, R): keys[(row * S + slab) * K + k], k < K = 2 nb: the slab's best scores in order (index = token);
// 0 where the slab has fewer than K entries. LOGP: the row holds log-probabilities already (processed ones):
// score = x + running, and pm / ps are not read
template <bool LOGP>
__global__ __launch_bounds__(BEAM_THREADS) void beam_slab_topk_kernel(const float* __restrict__ logits, int64_t ldl,
                                                                       const float* __restrict__ running, int V,
                                                                       int slab, int K, const float* __restrict__ pm,
                                                                       const float* __restrict__ ps,
                                                                       uint64_t* __restrict__ keys) {
  __shared__ uint64_t sh[BEAM_WAVES];
  const int row = blockIdx.y, S = gridDim.x;
  const int lo = blockIdx.x * slab, hi = min(V, lo + slab);
  const float lse = LOGP ? 0.f : beam_row_lse(pm, ps, row, S);
  const float run = running[row];
  const float* x = logits + (int64_t)row * ldl;
  uint64_t key[BEAM_PER_THREAD];
#pragma unroll
  for (int j = 0; j < BEAM_PER_THREAD; ++j) {
    const int i = lo + threadIdx.x + j * BEAM_THREADS;
    key[j] = i < hi ? beam_key(LOGP ? x[i] + run : (x[i] - lse) + run, (uint32_t)i) : 0ull;
  }
  uint64_t prev = ~0ull;
  for (int k = 0; k < K; ++k) {
    uint64_t best = 0ull;
#pragma unroll
    for (int j = 0; j < BEAM_PER_THREAD; ++j)
      if (key[j] < prev && key[j] > best) best = key[j];
    best = wg_max_u64(best, sh);
    if (threadIdx.x == 0) keys[((int64_t)row * S + blockIdx.x) * K + k] = best;
    prev = best;  // (0 once the slab is used up: nothing lies below it)
  }
}

// grid (S, R): x <- x - logsumexp(row) in place over one slab of one row, the value (b) scores against (a NaN
// stays a NaN, -inf stays -inf). Reads only the partials of (a) beside its own slab.
__global__ __launch_bounds__(BEAM_THREADS) void beam_normalize_kernel(float* __restrict__ logits, int64_t ldl, int V,
                                                                       int slab, const float* __restrict__ pm,
                                                                       const float* __restrict__ ps) {
  const int row = blockIdx.y, S = gridDim.x;
  const int lo = blockIdx.x * slab, hi = min(V, lo + slab);
  const float lse = beam_row_lse(pm, ps, row, S);
  float* x = logits + (int64_t)row * ldl;
  for (int i = lo + threadIdx.x; i < hi; i += BEAM_THREADS) x[i] = x[i] - lse;
}

// (c) one workgroup per image over the nb * S * K keys of its rows, re-keyed by the flat index beam * V + token
__global__ __launch_bounds__(BEAM_THREADS) void beam_merge_kernel(const uint64_t* __restrict__ keys, int nb, int S,
                                                                   int K, int V, float* __restrict__ out_score,
                                                                   int32_t* __restrict__ out_beam,
                                                                   int32_t* __restrict__ out_token) {
  __shared__ uint64_t sh[BEAM_WAVES];
  const int b = blockIdx.x;
  const int per_row = S * K, n = nb * per_row;
  const uint64_t* src = keys + (int64_t)b * n;
  uint64_t prev = ~0ull;
  for (int k = 0; k < K; ++k) {
    uint64_t best = 0ull;
    for (int i = threadIdx.x; i < n; i += BEAM_THREADS) {
      const uint64_t raw = src[i];
      if (raw == 0ull) continue;
      const uint32_t flat = (uint32_t)(i / per_row) * (uint32_t)V + beam_key_index(raw);
      const uint64_t c = (raw & 0xffffffff00000000ull) | (uint64_t)(0xffffffffu - flat);
      if (c < prev && c > best) best = c;
    }
    best = wg_max_u64(best, sh);
    if (threadIdx.x == 0) {
      // (V >= 2 nb, so an image always has K candidates; an empty slot would still name row 0, token 0)
      const uint32_t flat = best ? beam_key_index(best) : 0u;
      out_score[(int64_t)b * K + k] = beam_key_float((uint32_t)(best >> 32));
      out_beam[(int64_t)b * K + k] = (int32_t)(flat / (uint32_t)V);
      out_token[(int64_t)b * K + k] = (int32_t)(flat % (uint32_t)V);
    }
    prev = best;
  }
}

// ---------------------------------------------------------------------------------------------
// beam update
// ---------------------------------------------------------------------------------------------
struct BeamUpdateParams {
  const float* c_score; const int32_t* c_beam; const int32_t* c_token;
  float* run_score; float* fin_score; int32_t* fin_flag; int32_t* fin_len;
  int32_t* run_seq; int32_t* fin_seq; int32_t* flags; int32_t* parent; int64_t* next; int64_t next_ld;
  int nb, T, t, gen_len, last, early, eos;
  float len_div;
};

// k best of n values in the candidates' order (larger first, ties to the lower index, NaN last): order[j]
__device__ void beam_small_topk(const float* v, int n, int k, int* order) {
  uint64_t prev = ~0ull;
  for (int j = 0; j < k; ++j) {
    uint64_t best = 0ull;
    for (int i = 0; i < n; ++i) {
      const uint64_t c = beam_key(v[i], (uint32_t)i);
      if (c < prev && c > best) best = c;
    }
    order[j] = (int)beam_key_index(best);
    prev = best;
  }
}

// transformers' steps d - g for one image (generation/utils.py _beam_search): thread 0 decides, all threads
// move the sequences. Every fp32 operation is the one torch performs, in its order.
__global__ __launch_bounds__(BEAM_THREADS) void beam_update_kernel(BeamUpdateParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* old_run = reinterpret_cast<int32_t*>(smem);   // [nb][T]
  int32_t* old_fin = old_run + p.nb * p.T;               // [nb][T]
  __shared__ int run_src[BEAM_MAX_NB], fin_src[BEAM_MAX_NB], c_beam[2 * BEAM_MAX_NB], c_tok[2 * BEAM_MAX_NB];
  const int b = blockIdx.x, nb = p.nb, K = 2 * nb, T = p.T;
  const int64_t seq0 = (int64_t)b * nb * T;
  for (int i = threadIdx.x; i < nb * T; i += BEAM_THREADS) {
    old_run[i] = p.run_seq[seq0 + i];
    old_fin[i] = p.fin_seq[seq0 + i];
  }
  if (threadIdx.x == 0) {
    const float NEG = -1.0e9f;
    float cs[2 * BEAM_MAX_NB], rl[2 * BEAM_MAX_NB], merged[3 * BEAM_MAX_NB];
    int hit[2 * BEAM_MAX_NB], mflag[3 * BEAM_MAX_NB], mlen[3 * BEAM_MAX_NB];
    bool all_hit = true, full = true;
    for (int j = 0; j < nb; ++j) {
      merged[j] = p.fin_score[b * nb + j];
      mflag[j] = p.fin_flag[b * nb + j];
      mlen[j] = p.fin_len[b * nb + j];
      full = full && mflag[j] != 0;
    }
    full = full && p.early != 0;
    const bool unsat = p.flags[b * 4 + 0] != 0;
    for (int c = 0; c < K; ++c) {
      cs[c] = p.c_score[b * K + c];
      // (the selection never names a beam or token out of range; a caller's own candidates are clamped)
      c_beam[c] = min(max(p.c_beam[b * K + c], 0), nb - 1);
      c_tok[c] = p.c_token[b * K + c];
      hit[c] = (c_tok[c] == p.eos || p.last) ? 1 : 0;
      all_hit = all_hit && hit[c];
      rl[c] = hit[c] ? cs[c] + NEG : cs[c];
      const bool did = hit[c] && c < nb;
      float s = cs[c] / p.len_div;
      if (full) s += NEG;
      if (!unsat) s += NEG;
      if (!did) s += NEG;
      merged[nb + c] = s;
      mflag[nb + c] = did ? 1 : 0;
      mlen[nb + c] = p.gen_len;
    }
    beam_small_topk(rl, K, nb, run_src);
    beam_small_topk(merged, 3 * nb, nb, fin_src);
    float new_fin[BEAM_MAX_NB];
    bool all_fin = true;
    float worst = INFINITY;
    for (int j = 0; j < nb; ++j) {
      const int c = run_src[j];
      p.run_score[b * nb + j] = rl[c];
      p.parent[b * nb + j] = b * nb + c_beam[c];
      p.next[(int64_t)(b * nb + j) * p.next_ld] = c_tok[c];
      new_fin[j] = merged[fin_src[j]];
      // torch.min propagates a NaN
      worst = (new_fin[j] != new_fin[j] || worst != worst) ? __uint_as_float(0x7fc00000u) : fminf(worst, new_fin[j]);
    }
    const float best_possible = rl[run_src[0]] / p.len_div;
    bool improve = false;
    for (int j = 0; j < nb; ++j) {
      const int m = fin_src[j];
      p.fin_score[b * nb + j] = new_fin[j];
      p.fin_flag[b * nb + j] = mflag[m];
      p.fin_len[b * nb + j] = mlen[m];
      all_fin = all_fin && mflag[m] != 0;
      improve = improve || best_possible > (mflag[m] ? worst : NEG);
    }
    p.flags[b * 4 + 0] = (unsat && improve) ? 1 : 0;
    p.flags[b * 4 + 1] = all_fin ? 1 : 0;
    p.flags[b * 4 + 2] = all_hit ? 1 : 0;
  }
  __syncthreads();
  const int pos = p.t + 1;
  for (int i = threadIdx.x; i < nb * T; i += BEAM_THREADS) {
    const int j = i / T, q = i % T;
    const int c = run_src[j];
    p.run_seq[seq0 + i] = q == pos ? c_tok[c] : old_run[c_beam[c] * T + q];
    const int m = fin_src[j];
    int32_t v;
    if (m < nb) v = old_fin[m * T + q];
    else v = q == pos ? c_tok[m - nb] : old_run[c_beam[m - nb] * T + q];
    p.fin_seq[seq0 + i] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// cache reorder
// ---------------------------------------------------------------------------------------------
// grid (chunks, rows, layers): dst[layer] row r <- src[layer] row parent[r], the first `bytes` bytes of the row
// (positions 0 .. t are contiguous in a [rows, steps, 2E] cache); rows past n_beam_rows copy themselves
__global__ __launch_bounds__(BEAM_THREADS) void beam_reorder_kernel(const char* const* __restrict__ src,
                                                                     char* const* __restrict__ dst,
                                                                     const int32_t* __restrict__ parent,
                                                                     int n_beam_rows, int64_t row_stride,
                                                                     int64_t bytes) {
  const int r = blockIdx.y, layer = blockIdx.z;
  int from = r;
  if (r < n_beam_rows) {
    const int pr = parent[r];
    if (pr >= 0 && pr < n_beam_rows) from = pr;  // (a parent out of range is never followed)
  }
  const uint4* s = reinterpret_cast<const uint4*>(src[layer] + (int64_t)from * row_stride);
  uint4* d = reinterpret_cast<uint4*>(dst[layer] + (int64_t)r * row_stride);
  const int64_t n = bytes / 16;
  for (int64_t i = (int64_t)blockIdx.x * BEAM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BEAM_THREADS)
    d[i] = s[i];
}

bool beam_select_shape_ok(int64_t B, int64_t nb, int64_t V) {
  return B >= 1 && nb >= 1 && nb <= BEAM_MAX_NB && B * nb <= 65535 && V >= 2 * nb && V <= (1 << 20);
}

}  // namespace

extern "C" int64_t mmfd_beam_select_slab(int64_t V) {
  if (V < 1 || V > (1 << 20)) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_beam_select_slab: V = %lld (1 .. 2^20)", (long long)V);
    return -1;
  }
  return beam_slab(V);
}

extern "C" int64_t mmfd_beam_select_workspace_bytes(int64_t B, int64_t nb, int64_t V) {
  if (!beam_select_shape_ok(B, nb, V)) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_beam_select_workspace_bytes: unsupported shape");
    return -1;
  }
  const int64_t slab = beam_slab(V), S = (V + slab - 1) / slab, R = B * nb;
  return R * S * 8 + R * S * 2 * nb * 8;  // {max, sum} and 2 nb keys per (row, slab)
}

namespace {

int beam_select_run(const char* name, bool logp, int64_t B, int64_t nb, int64_t V, const float* logits, int64_t ldl,
                    const float* running, float* out_score, int32_t* out_beam, int32_t* out_token, void* workspace,
                    int64_t workspace_bytes, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(nb >= 1 && nb <= BEAM_MAX_NB, "%s: num_beams = %lld (1 .. %d)", name, (long long)nb, BEAM_MAX_NB);
  MMFD_CHECK_ARG(B >= 1 && B * nb <= 65535, "%s: B = %lld", name, (long long)B);
  MMFD_CHECK_ARG(V >= 2 * nb && V <= (1 << 20), "%s: V = %lld (2 num_beams .. 2^20)", name, (long long)V);
  MMFD_CHECK_ARG(logits && running && out_score && out_beam && out_token, "%s: null pointer", name);
  MMFD_CHECK_ARG(ldl >= V, "%s: leading dimension too small", name);
  const int64_t need = mmfd_beam_select_workspace_bytes(B, nb, V);
  MMFD_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
                 "%s: needs an 8-byte aligned workspace of %lld bytes (mmfd_beam_select_workspace_bytes)", name,
                 (long long)need);
  const int slab = beam_slab(V);
  const int64_t S = (V + slab - 1) / slab, R = B * nb;
  uint64_t* keys = (uint64_t*)workspace;           // [R][S][2 nb]
  float* pm = (float*)(keys + R * S * 2 * nb);     // [R][S]
  float* ps = pm + R * S;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)S, (unsigned)R), block(BEAM_THREADS);
  if (!logp) {
    hipLaunchKernelGGL(beam_partial_kernel, grid, block, 0, s, logits, ldl, (int)V, slab, pm, ps);
    MMFD_CHECK_LAUNCH("mmfd_beam_select (partials)");
    hipLaunchKernelGGL(beam_slab_topk_kernel<false>, grid, block, 0, s, logits, ldl, running, (int)V, slab,
                       (int)(2 * nb), pm, ps, keys);
  } else {
    hipLaunchKernelGGL(beam_slab_topk_kernel<true>, grid, block, 0, s, logits, ldl, running, (int)V, slab,
                       (int)(2 * nb), pm, ps, keys);
  }
  MMFD_CHECK_LAUNCH("mmfd_beam_select (slabs)");
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)B), block, 0, s, keys, (int)nb, (int)S, (int)(2 * nb), (int)V,
                     out_score, out_beam, out_token);
  MMFD_CHECK_LAUNCH("mmfd_beam_select (merge)");
  return 0;
}

}  // namespace

extern "C" int mmfd_beam_select(int64_t B, int64_t nb, int64_t V, const float* logits, int64_t ldl,
                                const float* running, float* out_score, int32_t* out_beam, int32_t* out_token,
                                void* workspace, int64_t workspace_bytes, mmfd_stream_t stream) {
  return beam_select_run("mmfd_beam_select", false, B, nb, V, logits, ldl, running, out_score, out_beam, out_token,
                         workspace, workspace_bytes, stream);
}

extern "C" int mmfd_beam_select_logprobs(int64_t B, int64_t nb, int64_t V, const float* logprobs, int64_t ldl,
                                         const float* running, float* out_score, int32_t* out_beam,
                                         int32_t* out_token, void* workspace, int64_t workspace_bytes,
                                         mmfd_stream_t stream) {
  return beam_select_run("mmfd_beam_select_logprobs", true, B, nb, V, logprobs, ldl, running, out_score, out_beam,
                         out_token, workspace, workspace_bytes, stream);
}

extern "C" int64_t mmfd_row_log_softmax_workspace_bytes(int64_t R, int64_t V) {
  if (R < 1 || R > 65535 || V < 1 || V > (1 << 20)) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_row_log_softmax_workspace_bytes: R = %lld (1 .. 65535), V = %lld (1 .. 2^20)",
                   (long long)R, (long long)V);
    return -1;
  }
  const int64_t slab = beam_slab(V), S = (V + slab - 1) / slab;
  return R * S * 8;  // {max, sum} per (row, slab)
}

extern "C" int mmfd_row_log_softmax(int64_t R, int64_t V, float* logits, int64_t ldl, void* workspace,
                                    int64_t workspace_bytes, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(R >= 1 && R <= 65535, "mmfd_row_log_softmax: R = %lld rows (1 .. 65535)", (long long)R);
  MMFD_CHECK_ARG(V >= 1 && V <= (1 << 20), "mmfd_row_log_softmax: V = %lld (1 .. 2^20)", (long long)V);
  MMFD_CHECK_ARG(logits, "mmfd_row_log_softmax: null pointer");
  MMFD_CHECK_ARG(ldl >= V, "mmfd_row_log_softmax: leading dimension too small");
  const int64_t need = mmfd_row_log_softmax_workspace_bytes(R, V);
  MMFD_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
                 "mmfd_row_log_softmax: needs a 4-byte aligned workspace of %lld bytes "
                 "(mmfd_row_log_softmax_workspace_bytes)", (long long)need);
  const int slab = beam_slab(V);
  const int64_t S = (V + slab - 1) / slab;
  float* pm = (float*)workspace;  // [R][S]
  float* ps = pm + R * S;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)S, (unsigned)R), block(BEAM_THREADS);
  hipLaunchKernelGGL(beam_partial_kernel, grid, block, 0, s, logits, ldl, (int)V, slab, pm, ps);
  MMFD_CHECK_LAUNCH("mmfd_row_log_softmax (partials)");
  hipLaunchKernelGGL(beam_normalize_kernel, grid, block, 0, s, logits, ldl, (int)V, slab, pm, ps);
  MMFD_CHECK_LAUNCH("mmfd_row_log_softmax (normalise)");
  return 0;
}

extern "C" int mmfd_beam_update(int64_t B, int64_t nb, int64_t T, int64_t t, int64_t gen_len, int last,
                                int early_stopping, int64_t eos, float len_div, const float* cand_score,
                                const int32_t* cand_beam, const int32_t* cand_token, float* run_score,
                                float* fin_score, int32_t* fin_flag, int32_t* fin_len, int32_t* run_seq,
                                int32_t* fin_seq, int32_t* flags, int32_t* parent, int64_t* next, int64_t next_ld,
                                mmfd_stream_t stream) {
  MMFD_CHECK_ARG(nb >= 1 && nb <= BEAM_MAX_NB, "mmfd_beam_update: num_beams = %lld (1 .. %d)", (long long)nb,
                 BEAM_MAX_NB);
  MMFD_CHECK_ARG(B >= 1 && B * nb <= 65535, "mmfd_beam_update: B = %lld", (long long)B);
  MMFD_CHECK_ARG(T >= 2 && T <= BEAM_MAX_T, "mmfd_beam_update: T = %lld positions (2 .. %d)", (long long)T, BEAM_MAX_T);
  MMFD_CHECK_ARG(t >= 0 && t + 1 < T, "mmfd_beam_update: step %lld writes position %lld of %lld", (long long)t,
                 (long long)(t + 1), (long long)T);
  MMFD_CHECK_ARG(gen_len >= 1 && gen_len <= t + 1, "mmfd_beam_update: generated length %lld at step %lld",
                 (long long)gen_len, (long long)t);
  MMFD_CHECK_ARG(len_div > 0.f && len_div == len_div, "mmfd_beam_update: length divisor must be positive");
  MMFD_CHECK_ARG(eos >= 0 && eos <= INT_MAX, "mmfd_beam_update: bad eos");
  MMFD_CHECK_ARG(cand_score && cand_beam && cand_token && run_score && fin_score && fin_flag && fin_len && run_seq &&
                     fin_seq && flags && parent && next,
                 "mmfd_beam_update: null pointer");
  MMFD_CHECK_ARG(next_ld >= 1, "mmfd_beam_update: bad stride");
  BeamUpdateParams p;
  p.c_score = cand_score; p.c_beam = cand_beam; p.c_token = cand_token;
  p.run_score = run_score; p.fin_score = fin_score; p.fin_flag = fin_flag; p.fin_len = fin_len;
  p.run_seq = run_seq; p.fin_seq = fin_seq; p.flags = flags; p.parent = parent; p.next = next; p.next_ld = next_ld;
  p.nb = (int)nb; p.T = (int)T; p.t = (int)t; p.gen_len = (int)gen_len; p.last = last ? 1 : 0;
  p.early = early_stopping ? 1 : 0; p.eos = (int)eos; p.len_div = len_div;
  const size_t lds = (size_t)2 * nb * T * sizeof(int32_t);  // <= 32 KiB
  hipLaunchKernelGGL(beam_update_kernel, dim3((unsigned)B), dim3(BEAM_THREADS), lds, (hipStream_t)stream, p);
  MMFD_CHECK_LAUNCH("mmfd_beam_update");
  return 0;
}

extern "C" int mmfd_beam_reorder(int64_t layers, int64_t rows, int64_t beam_rows, int64_t row_stride_bytes,
                                 int64_t bytes, const void* const* src, void* const* dst, const int32_t* parent,
                                 mmfd_stream_t stream) {
  MMFD_CHECK_ARG(layers >= 1 && layers <= 65535 && rows >= 1 && rows <= 65535, "mmfd_beam_reorder: bad shape");
  MMFD_CHECK_ARG(beam_rows >= 0 && beam_rows <= rows, "mmfd_beam_reorder: %lld beam rows of %lld", (long long)beam_rows,
                 (long long)rows);
  MMFD_CHECK_ARG(bytes >= 0 && bytes <= row_stride_bytes && bytes % 16 == 0 && row_stride_bytes % 16 == 0,
                 "mmfd_beam_reorder: the copied bytes and the row stride must be multiples of 16, bytes <= stride");
  MMFD_CHECK_ARG(src && dst && parent, "mmfd_beam_reorder: null pointer");
  if (bytes == 0) return 0;
  const int64_t chunks = (bytes / 16 + BEAM_THREADS - 1) / BEAM_THREADS;
  const dim3 grid((unsigned)(chunks < 64 ? chunks : 64), (unsigned)rows, (unsigned)layers);
  hipLaunchKernelGGL(beam_reorder_kernel, grid, dim3(BEAM_THREADS), 0, (hipStream_t)stream, (const char* const*)src,
                     (char* const*)dst, parent, (int)beam_rows, row_stride_bytes, bytes);
  MMFD_CHECK_LAUNCH("mmfd_beam_reorder");
  return 0;
}
