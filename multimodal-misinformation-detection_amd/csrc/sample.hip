// Sampling for the one-token-per-step decoder (BLIP captioning, mmfd/blip.py): the selection a sampling step
// needs in place of the argmax. transformers' GenerationMixin._sample with do_sample=True is the rule:
// TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (min_tokens_to_keep = 1), softmax, one draw.
//
//   mmfd_sample_select   one workgroup of 1024 threads per row. The row becomes order-preserving 32-bit keys
//                        (the beam kernels' mapping of s = logit / temperature; NaN -> 0), staged once in LDS
//                        when the row fits (V <= mmfd_sample_select_resident_max), else recomputed from the
//                        logits on every pass. The masses are INTEGERS, w = round(exp(s - max) * 2^40): every
//                        histogram, reduction and prefix is a sum of integers, so it does not depend on the order
//                        in which LDS atomics arrive and the same inputs give the same bits.
//     top-k    the k-th largest key by a radix select over four 8-bit digits with count histograms.
//     top-p    the same descent with mass histograms: the smallest key x whose mass strictly above is below
//              P = ceil(top_p * S) (at least 1: the first entry always stays); of the entries equal to x the
//              c = ceil((P - mass above) / w(x)) lowest indices stay (found by the index-ordered walk below).
//     draw     u = (mmfd_hash(seed, step, row0 + r) >> 8) * 2^-24; the token is the lowest kept index whose
//              inclusive prefix mass exceeds floor(u * S_k) (a 24 x 64 bit product), found from per-wave
//              contiguous index ranges, the waves' totals, and two wave scans inside the range that holds it
//              (over per-lane contiguous runs, then over the entries of the run that holds it).
//
// Order among entries: the larger s first, equal s by the lower index; a NaN is never kept, -inf has mass 0 and
// is never kept either (a filtered entry and a -inf one are the same thing to the softmax).
#include <cmath>

#include "common.h"

namespace {

constexpr int SMP_THREADS = 1024, SMP_WAVES = SMP_THREADS / 64;
constexpr int SMP_STAGE = 8;                   // slices whose loads the staging pass keeps in flight
constexpr int SMP_REP = 8;                     // histogram copies (lane & 7): logits crowd into a few top digits
constexpr int SMP_RESIDENT_MAX = 32768;        // keys staged in LDS up to this V (128 KiB of the CU's 160)
constexpr int SMP_MAX_V = 1 << 20;             // V * 2^40 < 2^63
constexpr uint32_t SMP_KEY_FLOOR = 0x00800000u;  // the key of -FLT_MAX: below it only -inf (0x007fffff) and NaN (0)
constexpr uint64_t SMP_ONE = 1ull << 40;

__device__ __forceinline__ uint32_t smp_float_key(float v) {
  if (v != v) return 0u;
  v += 0.0f;  // -0 -> +0
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float smp_key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// exp(x) for x <= 0 to about 1.5 ulp: x log2(e) as an unevaluated sum t + lo (log2(e) split into two floats, the
// product's rounding error recovered by an FMA), 2^t by the hardware (1 ulp), the rest by its first-order term
__device__ __forceinline__ float smp_exp(float x) {
  const float t = x * 1.44269502e+00f;
  const float lo = fmaf(x, 1.44269502e+00f, -t) + x * 1.92596303e-08f;
  const float e = __builtin_amdgcn_exp2f(t);
  return fmaf(e, lo * 6.93147182e-01f, e);
}

struct SampleParams {
  const float* logits; int64_t ldl;
  const int64_t* ctl; int64_t step;
  int64_t* out_token; float* probs; int64_t ldp; int32_t* kept;
  int V, top_k;
  float temperature, top_p;
};

struct SampleShared {
  unsigned long long hist[256 * SMP_REP];
  unsigned long long hsum[256];
  unsigned long long tot[SMP_WAVES], cnt[SMP_WAVES];
  unsigned long long sel_above, sel_p, sel_mass;
  uint32_t sel_digit, red[SMP_WAVES];
  int found;
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

template <bool RES> struct Row {
  const float* x;
  const uint32_t* keys;  // LDS
  float temperature;
  __device__ __forceinline__ uint32_t key_of(float v) const {
    return smp_float_key(temperature == 1.0f ? v : __fdiv_rn(v, temperature));
  }
  __device__ __forceinline__ uint32_t make(int i) const { return key_of(x[i]); }
  __device__ __forceinline__ uint32_t key(int i) const { return RES ? keys[i] : make(i); }
};

// every wave owns one contiguous index range [w * seg, (w + 1) * seg), seg a multiple of 64, and visits it in
// slices of 64 consecutive entries (one per lane): coalesced, and in index order within the wave
#define SMP_FOR_SLICES(base) \
  for (int base = wave * seg, end__ = min(V, (wave + 1) * seg); base < end__; base += 64)

// The radix descent. weight(key) is an integer mass per entry; returns the smallest key x (among entries of
// non-zero weight) whose weight strictly above, `above`, is below P. P is p.x of the caller, or, FROM_TOTAL,
// max(1, ceil(frac * total weight)) (returned in P). The caller guarantees P >= 1 and a non-zero total.
// equal_out: the weight of all entries equal to x together.
template <bool RES, bool FROM_TOTAL, typename W>
__device__ uint32_t smp_descend(SampleShared& sh, const Row<RES>& row, int V, int seg, W weight,
                                unsigned long long& P, float frac, unsigned long long& above_out,
                                unsigned long long& equal_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t prefix = 0;
  unsigned long long above = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 256 * SMP_REP; i += SMP_THREADS) sh.hist[i] = 0ull;
    __syncthreads();
    SMP_FOR_SLICES(base) {
      const int i = base + lane;
      if (i < V) {
        const uint32_t k = row.key(i);
        if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) {
          const unsigned long long w = weight(k);
          if (w) atomicAdd(&sh.hist[((k >> shift) & 255u) * SMP_REP + (lane & (SMP_REP - 1))], w);
        }
      }
    }
    __syncthreads();
    if (tid < 256) {
      unsigned long long h = 0;
#pragma unroll
      for (int r = 0; r < SMP_REP; ++r) h += sh.hist[tid * SMP_REP + r];
      sh.hsum[tid] = h;
    }
    __syncthreads();
    if (wave == 0) {
      // lane l holds digits 255 - 4l .. 252 - 4l, the largest first
      unsigned long long h[4], mine = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = sh.hsum[255 - 4 * lane - j];
        mine += h[j];
      }
      const unsigned long long incl = wave_incl_scan_u64(mine, lane);
      unsigned long long Pl = P;
      if (FROM_TOTAL && pass == 0) {
        const unsigned long long total = __shfl(incl, 63, 64);
        const double pd = ceil((double)frac * (double)total);
        Pl = pd < 1.0 ? 1ull : (unsigned long long)pd;
      }
      unsigned long long run = above + (incl - mine), best_above = 0, best_mass = 0;
      int best = -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (h[j] != 0 && run < Pl) {
          best = 255 - 4 * lane - j;
          best_above = run;
          best_mass = h[j];
        }
        run += h[j];
      }
      // the lowest digit that qualifies: the qualifying digits are the top non-empty ones, so it lies in the
      // highest lane that has one
      const unsigned long long has = __ballot(best >= 0);
      const int owner = has ? 63 - __builtin_clzll(has) : 0;
      if (lane == owner) {
        sh.sel_digit = (uint32_t)(best < 0 ? 0 : best);
        sh.sel_above = best_above;
        sh.sel_mass = best_mass;
        sh.sel_p = Pl;
      }
    }
    __syncthreads();
    prefix |= sh.sel_digit << shift;
    above = sh.sel_above;
    P = sh.sel_p;
  }
  above_out = above;
  equal_out = sh.sel_mass;  // (not written again before the next descent's third barrier)
  return prefix;
}

// The index-ordered walk: the lowest index whose inclusive prefix of weight(key, index) exceeds target, or V when
// the whole row's weight does not. total_out / count_out: the row's weight and its number of non-zero entries.
template <bool RES, typename W>
__device__ int smp_find_prefix(SampleShared& sh, const Row<RES>& row, int V, int seg, W weight,
                               unsigned long long target, bool target_is_fraction, uint32_t u24,
                               unsigned long long& total_out, unsigned long long& count_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long mine = 0, n = 0;
  SMP_FOR_SLICES(base) {
    const int i = base + lane;
    if (i < V) {
      const unsigned long long w = weight(row.key(i), i, n);
      mine += w;
    }
  }
  mine = wave_sum_u64(mine);
  n = wave_sum_u64(n);
  if (lane == 0) {
    sh.tot[wave] = mine;
    sh.cnt[wave] = n;
    if (wave == 0) sh.found = V;
  }
  __syncthreads();
  unsigned long long before = 0, total = 0, count = 0;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) {
    if (w < wave) before += sh.tot[w];
    total += sh.tot[w];
    count += sh.cnt[w];
  }
  total_out = total;
  count_out = count;
  if (target_is_fraction) {
    // floor(u * total), u = u24 * 2^-24: a 24 x 64 bit product (below `total`, so an index is always found)
    const unsigned long long hi = __umul64hi((unsigned long long)u24, total), lo = (unsigned long long)u24 * total;
    target = (hi << 40) | (lo >> 24);
  }
  if (before <= target && target < before + mine) {  // wave-uniform: this wave's range holds the target
    // two levels, one wave scan each: every lane sums a contiguous run of q = seg / 64 entries and the scan of
    // the runs' sums names the run; then the run's entries go one per lane (64 at a time when q > 64)
    unsigned long long dummy = 0, run_sum = 0;
    const int q = seg >> 6, w0 = wave * seg;
    for (int j = 0, i = w0 + lane * q; j < q && i < V; ++j, ++i) run_sum += weight(row.key(i), i, dummy);
    const unsigned long long incl = wave_incl_scan_u64(run_sum, lane);
    const unsigned long long hit = __ballot(before + incl > target);  // non-zero: integer sums, the same total
    const int src = hit ? __builtin_ctzll(hit) : 63;
    unsigned long long acc = before + __shfl(incl - run_sum, src, 64);
    const int run_lo = w0 + src * q;
    for (int c = 0; c < q; c += 64) {
      const int j = c + lane, i = run_lo + j;
      const unsigned long long w = (j < q && i < V) ? weight(row.key(i), i, dummy) : 0ull;
      const unsigned long long incl2 = wave_incl_scan_u64(w, lane);
      const unsigned long long hit2 = __ballot(acc + incl2 > target);
      if (hit2) {
        if (lane == 0) sh.found = run_lo + c + __builtin_ctzll(hit2);
        break;
      }
      acc += __shfl(incl2, 63, 64);
    }
  }
  __syncthreads();
  const int found = sh.found;
  __syncthreads();
  return found;
}

template <bool RES>
__global__ __launch_bounds__(SMP_THREADS) void sample_select_kernel(SampleParams p) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smp_keys[];
  __shared__ SampleShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x, V = p.V;
  const int seg = ((V + SMP_WAVES - 1) / SMP_WAVES + 63) / 64 * 64;
  Row<RES> row;
  row.x = p.logits + (int64_t)r * p.ldl;
  row.keys = smp_keys;
  row.temperature = p.temperature;

  // keys (staged when resident) and the largest of them
  // (eight slices per trip, their loads issued together; worth about 1 us of the kernel's 32 at V = 30,524)
  uint32_t kmax = 0;
  for (int base = wave * seg, end = min(V, (wave + 1) * seg); base < end; base += 64 * SMP_STAGE) {
    float v[SMP_STAGE];
#pragma unroll
    for (int u = 0; u < SMP_STAGE; ++u) {
      const int i = base + u * 64 + lane;
      v[u] = i < end ? row.x[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SMP_STAGE; ++u) {
      const int i = base + u * 64 + lane;
      if (i < end) {
        const uint32_t k = row.key_of(v[u]);
        if (RES) smp_keys[i] = k;
        kmax = max(kmax, k);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
  if (lane == 0) sh.red[wave] = kmax;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) kmax = max(kmax, sh.red[w]);
  float* prow = p.probs ? p.probs + (int64_t)r * p.ldp : nullptr;
  if (kmax < SMP_KEY_FLOOR) {  // no number in the row
    if (prow)
      for (int i = tid; i < V; i += SMP_THREADS) prow[i] = 0.f;
    if (tid == 0) {
      p.out_token[r] = 0;
      if (p.kept) p.kept[r] = 0;
    }
    return;
  }
  const float m = smp_key_float(kmax);

  // top-k: the k-th largest key, duplicates (and NaNs, below every number) counted
  uint32_t lo = SMP_KEY_FLOOR;
  if (p.top_k > 0 && p.top_k < V) {
    unsigned long long P = (unsigned long long)p.top_k, above, equal;
    const uint32_t tau = smp_descend<RES, false>(sh, row, V, seg, [](uint32_t) { return 1ull; }, P, 0.f, above, equal);
    lo = max(lo, tau);
  }
  auto mass = [=](uint32_t k) -> unsigned long long {
    if (k < lo) return 0ull;
    if (k == kmax) return SMP_ONE;
    const float d = smp_key_float(k) - m;
    if (!(d > -64.f)) return 0ull;  // below 2^-41 anyway; also m = +inf
    return (unsigned long long)rintf(ldexpf(smp_exp(d), 40));
  };

  // top-p: the boundary key x, and the last index kept among the entries equal to it
  uint32_t x = 0;
  int cut = V;
  const bool nucleus = p.top_p < 1.0f;
  if (nucleus) {
    unsigned long long P = 0, above, equal;
    x = smp_descend<RES, true>(sh, row, V, seg, mass, P, p.top_p, above, equal);
    const unsigned long long wx = mass(x);  // > 0: the descent only enters digits of non-zero mass
    // of the equal / wx entries at x, c = ceil((P - above) / wx) >= 1 stay; all of them (one entry, mostly) when
    // P - above > equal - wx
    if (P - above + wx <= equal) {
      const unsigned long long c = (P - above + wx - 1) / wx;
      unsigned long long t_, c_;
      cut = smp_find_prefix<RES>(sh, row, V, seg,
                                 [=](uint32_t k, int, unsigned long long&) { return k == x ? 1ull : 0ull; }, c - 1,
                                 false, 0u, t_, c_);
    }
  }
  auto keep = [=](uint32_t k, int i) { return k >= lo && (!nucleus || k > x || (k == x && i <= cut)); };

  // the draw
  const uint64_t seed = (uint64_t)p.ctl[0], idx = (uint64_t)(p.ctl[1] + r);
  const uint32_t u24 = mmfd_hash(seed, (uint64_t)p.step, idx) >> 8;
  unsigned long long Sk, nkept;
  const int token = smp_find_prefix<RES>(sh, row, V, seg,
                                         [=](uint32_t k, int i, unsigned long long& n) {
                                           if (!keep(k, i)) return 0ull;
                                           ++n;
                                           return mass(k);
                                         },
                                         0ull, true, u24, Sk, nkept);
  if (tid == 0) {
    p.out_token[r] = token < V ? token : 0;  // (token < V always: floor(u S_k) < S_k)
    if (p.kept) p.kept[r] = (int32_t)nkept;
  }
  if (prow) {
    const float inv = (float)(1.0 / (double)Sk);
    SMP_FOR_SLICES(base) {
      const int i = base + lane;
      if (i < V) {
        const uint32_t k = row.key(i);
        prow[i] = keep(k, i) ? (float)mass(k) * inv : 0.f;
      }
    }
  }
}

}  // namespace

extern "C" int64_t mmfd_sample_select_resident_max(void) { return SMP_RESIDENT_MAX; }

extern "C" int64_t mmfd_sample_select_workspace_bytes(int64_t R, int64_t V) {
  if (R < 1 || R > 65535 || V < 1 || V > SMP_MAX_V) {
    mmfd_set_error(MMFD_ERR_INVALID, "mmfd_sample_select_workspace_bytes: R = %lld (1 .. 65535), V = %lld (1 .. 2^20)",
                   (long long)R, (long long)V);
    return -1;
  }
  return 16;  // nothing passes between workgroups; a caller may always hand over the bytes asked for
}

extern "C" int mmfd_sample_select(int64_t R, int64_t V, const float* logits, int64_t ldl, float temperature,
                                  int64_t top_k, float top_p, const int64_t* ctl, int64_t step, int64_t* out_token,
                                  float* probs, int64_t ldp, int32_t* kept, void* workspace, int64_t workspace_bytes,
                                  mmfd_stream_t stream) {
  MMFD_CHECK_ARG(R >= 1 && R <= 65535, "mmfd_sample_select: R = %lld rows (1 .. 65535)", (long long)R);
  MMFD_CHECK_ARG(V >= 1 && V <= SMP_MAX_V, "mmfd_sample_select: V = %lld (1 .. 2^20)", (long long)V);
  MMFD_CHECK_ARG(logits && ctl && out_token, "mmfd_sample_select: null pointer");
  MMFD_CHECK_ARG(ldl >= V, "mmfd_sample_select: leading dimension of the logits too small");
  MMFD_CHECK_ARG(!probs || ldp >= V, "mmfd_sample_select: leading dimension of probs too small");
  MMFD_CHECK_ARG(std::isfinite(temperature) && temperature > 0.f, "mmfd_sample_select: temperature must be finite and > 0");
  MMFD_CHECK_ARG(top_k >= 0, "mmfd_sample_select: top_k = %lld (0: no filter)", (long long)top_k);
  MMFD_CHECK_ARG(top_p >= 0.f && top_p <= 1.f, "mmfd_sample_select: top_p must lie in [0, 1]");
  MMFD_CHECK_ARG(step >= 0, "mmfd_sample_select: step = %lld", (long long)step);
  const int64_t need = mmfd_sample_select_workspace_bytes(R, V);
  MMFD_CHECK_ARG(workspace && workspace_bytes >= need,
                 "mmfd_sample_select: needs a workspace of %lld bytes (mmfd_sample_select_workspace_bytes)",
                 (long long)need);
  SampleParams p;
  p.logits = logits; p.ldl = ldl; p.ctl = ctl; p.step = step;
  p.out_token = out_token; p.probs = probs; p.ldp = ldp; p.kept = kept;
  p.V = (int)V; p.top_k = (int)(top_k < V ? top_k : 0);
  p.temperature = temperature; p.top_p = top_p;
  hipStream_t s = (hipStream_t)stream;
  if (V <= SMP_RESIDENT_MAX) {
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_select_kernel<true>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 SMP_RESIDENT_MAX * 4) == hipSuccess;
    (void)attr;
    hipLaunchKernelGGL(sample_select_kernel<true>, dim3((unsigned)R), dim3(SMP_THREADS), (size_t)V * 4, s, p);
  } else {
    hipLaunchKernelGGL(sample_select_kernel<false>, dim3((unsigned)R), dim3(SMP_THREADS), 0, s, p);
  }
  MMFD_CHECK_LAUNCH("mmfd_sample_select");
  return 0;
}
