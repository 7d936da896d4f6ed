// MFMA GEMM with fused epilogue for gfx950: the host half — switches, argument checks, the launch
// plan, the C entry points.
//
// The device code of this translation unit lives in headers, all compiled here and nowhere else
// (the compiler's output for a kernel depends on the unit's flags and neighbours):
//   gemm_tiles.h    epilogue arguments and stores, LDS operand images, LDS-DMA fills, MFMA fragments
//   gemm_tile128.h  the 256x128 tile kernel: gemm_mfma_kernel, gemm_mfma_n64_kernel, conv_mfma_kernel
//   gemm256.h       the 256x256 tile kernel (its bf16-output instantiations; shared with gemm_f32out.hip)
//   gemm_reduce.h   the extended epilogue, both split-K reduces, the plain FMA kernel
//   gemm_colsum.h   split3, the column sums, mmfd_reduce_partials_kernel
// Three more units hold kernels under flags of their own (Makefile) and export only launchers that
// take what the plan decided: gemm_f32out.hip, gemm_x6f.hip, gemm_g4.hip (generated).
//
// Operand layouts (template TA / TB):
//   0 = "K-contiguous" (A[m][k], or B[n][k] = nn.Linear weight): LDS image [128 rows][128 B],
//       16-B chunk c of row r stored at chunk c ^ (r & 7) (conflict-free ds_read_b128);
//   1 = "MN-contiguous" (A[k][m] or B[k][n]): LDS image [BK rows][128 elements]; bf16 fragments
//       come from ds_read_b64_tr_b16 (hardware transpose), fp32 fragments from 4 ds_read_b32.
// The three nn.Linear products are (TA,TB) = (0,0) forward, (0,1) grad-input, (1,1) grad-weight.
#include "common.h"
#include <algorithm>
#include <type_traits>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gemm_tiles.h"
#include "gemm_tile128.h"
#include "gemm256.h"
#include "gemm_reduce.h"
#include "gemm_colsum.h"

// ---------------------------------------------------------------------------------------------
// load-time switches: the environment is read here, once, and nowhere else
// ---------------------------------------------------------------------------------------------
namespace mmfd_gemmx {
// MMFD_X6_SEGMENTED: the segmented K loop (gemm256_kernel<X6>, kept for A/B measurements) instead of the
// fused planes (gemm256_x6f_kernel). MMFD_FP32_GEMM = native / 0: fp32 x fp32 -> fp32 on the fp32 MFMA,
// else on split operands (six bf16 MFMA products per fp32 product, see gemm256_kernel's X6 note; about
// 1.6x the fp32 MFMA rate at the encoder shapes)
GemmSwitches g_gemm_sw = [] {
  auto set = [](const char* name) { return getenv(name) != nullptr ? 1 : 0; };
  const char *gm = getenv("MMFD_G8_GROUP_M"), *v = getenv("MMFD_FP32_GEMM");
  return GemmSwitches{set("MMFD_GEMM_V1"), set("MMFD_GEMM_F32_V1"), set("MMFD_GEMM_NARROW_G8"), set("MMFD_X6_SEGMENTED"),
                      gm ? std::max(1, atoi(gm)) : 1, (v && (!strcmp(v, "native") || !strcmp(v, "0"))) ? 0 : 1};
}();
}  // namespace mmfd_gemmx

#ifdef MMFD_G8_STAMPS
extern "C" int mmfd_debug_g8_stamps(void* host_dst, int64_t bytes) {
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g8_stamps), (size_t)bytes, 0, hipMemcpyDeviceToHost);
}
#endif

namespace {
using mmfd_gemmx::g_gemm_sw;

void launch_split3(const float* X, int64_t ldx, int64_t rows, int64_t cols, bf16* P, hipStream_t s) {
  const int64_t chunks = rows * (cols / 8);
  const unsigned blocks = (unsigned)std::min<int64_t>((chunks + 255) / 256, 8192);
  hipLaunchKernelGGL(split3_kernel, dim3(blocks), dim3(256), 0, s, X, ldx, rows, cols, P, rows * cols);
}

// ---------------------------------------------------------------------------------------------
// what a product is eligible for
// ---------------------------------------------------------------------------------------------
bool x6_fused() { return !g_gemm_sw.x6_segmented; }

bool use_g8(const mmfd_gemm_args& a) {
  // tall GEMMs with N <= 128 or K < 64 (Swinv2 stage-1 out-projection / FFN2 at N = 128, its 4x4
  // patch embedding at K = 48): the 256x256 tile is half padding / all prologue, and the 256x128
  // kernel measured 20-35 % faster per launch (45 vs 66 us, 85 vs 107 us, 36 vs 55 us)
  if (!g_gemm_sw.narrow_g8 && a.M >= 4096 && (a.N <= 128 || a.K < 64)) return false;
  if (g_gemm_sw.v1) return false;
  if (a.dtype == MMFD_BF16) return true;
  // fp32 operands (the parity / headline mode): the 256x256 tile halves the B-panel traffic per
  // MFMA of the 256x128 kernel; fp32 C only (a bf16 C from fp32 operands stays on the 256x128 kernel)
  return a.dtype == MMFD_F32 && a.c_dtype == MMFD_F32 && !g_gemm_sw.f32_v1;
}

bool mfma_ok(const mmfd_gemm_args& a) {
  const int epc = (a.dtype == MMFD_BF16) ? 8 : 4;
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (a.conv) {  // implicit convolution: checked by conv_geom(); B as below
    const int64_t esz = a.dtype == MMFD_BF16 ? 2 : 4;
    const int64_t bbytes = (a.trans_b ? a.K : a.N) * a.ldb * esz;
    return al16(a.B) && a.ldb % epc == 0 && (a.trans_b ? a.N : a.K) % epc == 0 && a.N >= 16 &&
           bbytes < (1ll << 31) - 4096;
  }
  if (!al16(a.A) || !al16(a.B)) return false;
  if (a.lda % epc || a.ldb % epc) return false;
  const int64_t a_ext = a.trans_a ? a.M : a.K;  // contiguous extent
  const int64_t b_ext = a.trans_b ? a.N : a.K;
  if (a_ext % epc || b_ext % epc) return false;
  if (a.M < 16 || a.N < 16 || a.K < 16) return false;
  const int64_t esz = a.dtype == MMFD_BF16 ? 2 : 4;
  const int64_t abytes = (a.trans_a ? a.K : a.M) * a.lda * esz, bbytes = (a.trans_b ? a.K : a.N) * a.ldb * esz;
  if (abytes >= (1ll << 31) - 4096 || bbytes >= (1ll << 31) - 4096) return false;  // 32-bit buffer offsets
  return true;
}

// K units a split-K launch divides: 32-deep steps of all six products (fused planes), the six
// segments' 64-deep tiles (segmented), else the kernel's K-tiles
int64_t k_units(const mmfd_gemm_args& a, bool x6) {
  if (x6) return x6_fused() ? (a.K + 31) / 32 : 6 * ((a.K + 63) / 64);
  const int T = a.dtype == MMFD_BF16 ? 64 : 32;
  return (a.K + T - 1) / T;
}

int choose_splits(const mmfd_gemm_args& a, int64_t nkt, bool g8, bool x6) {
  const bool xf = x6 && x6_fused();
  int splits = 1;
  if (g8) {
    // one 256x256 block per CU: pick the split count that minimises rounds-of-256 per unit of work
    const int64_t tiles = ((a.M + G8_BM - 1) / G8_BM) * ((a.N + G8_BN - 1) / G8_BN);
    if (a.splits > 0) splits = a.splits;
    else if (nkt >= 16 && tiles < 256) {
      // modelled time (us): rounds of 256 blocks x (K-tiles per block x ~1.8 us + ~3 us block
      // overhead) + the fp32 slab round trip (written by the blocks, read by the reduce) at ~5 TB/s
      double best = 1e30;
      // (up to one round of blocks: the fusion head's 256x256 weight gradients over 32k-50k rows are
      // a single tile, and 32 splits left 224 CUs idle for ~180 us per launch)
      const int smax = (int)std::min<int64_t>(std::max<int64_t>(32, 256 / tiles), nkt / 8);
      // one 256x256 K-tile (bf16 / fp32 MFMA rate; a fused split-operand step = 3 bf16 K-tiles of MFMA)
      const double kt_us = xf ? 3.6 : (a.dtype == MMFD_BF16 || x6) ? 1.8 : 7.0;
      for (int sp = 1; sp <= smax; ++sp) {
        const double rounds = (double)((tiles * sp + 255) / 256);
        const double kts = (double)((nkt + sp - 1) / sp);
        double cost = rounds * (kts * kt_us + 3.0);
        if (sp > 1) cost += (double)sp * a.M * a.N * 8.0 / 5.0e6 + 4.0;
        if (cost < best) { best = cost; splits = sp; }
      }
    }
  } else if (a.splits > 0) splits = a.splits;
  else if (((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN) < 200 && nkt >= 16) {
    const int64_t tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    splits = (int)((384 + tiles - 1) / tiles);
    splits = (int)std::min<int64_t>(splits, nkt / 8);
    splits = std::min(splits, 16);
    if (splits < 1) splits = 1;
  }
  if (splits > nkt) splits = (int)nkt;
  if (splits < 1) splits = 1;
  return splits;
}

// split-operand eligibility: fp32 in / fp32 out on the 256x256 path, stored column counts a
// multiple of 8 (16-B plane rows), three planes of each operand < 2 GB (32-bit buffer offsets), and
// K a whole number of 64-row tiles when an operand is MN-contiguous (its K rows are plane rows:
// a partial tile would read into the next plane)
struct X6Plan { bool on; int64_t rows_a, cols_a, rows_b, cols_b, pa, pb; };
X6Plan x6_plan(const mmfd_gemm_args& a, bool g8) {
  X6Plan p{};
  if (g_gemm_sw.fp32_mode != 1 || a.dtype != MMFD_F32 || a.c_dtype != MMFD_F32 || !g8) return p;
  p.rows_a = a.trans_a ? a.K : a.M; p.cols_a = a.trans_a ? a.M : a.K;
  if (a.conv) {  // the planes of the NHWC activation, not of the (never written) im2col matrix
    p.rows_a = a.conv->N * a.conv->H * a.conv->W; p.cols_a = a.conv->C;
  }
  p.rows_b = a.trans_b ? a.K : a.N; p.cols_b = a.trans_b ? a.N : a.K;
  if (p.cols_a % 8 || p.cols_b % 8) return p;
  if ((a.trans_a || a.trans_b) && a.K % (x6_fused() ? 32 : 64)) return p;
  p.pa = p.rows_a * p.cols_a * 2; p.pb = p.rows_b * p.cols_b * 2;
  if (3 * p.pa >= (1ll << 31) - 4096 || 3 * p.pb >= (1ll << 31) - 4096) return p;
  p.on = true;
  return p;
}
int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// extra workspace for the fused row sums: per-split partials (G8) or the colsum partials (others)
int64_t rowsum_ws_bytes(const mmfd_gemm_args& a, int splits, bool g8) {
  if (!a.a_rowsum) return 0;
  if (g8) {  // per-(split, column tile) partials (gemm256_kernel rs_mode 3)
    const int64_t parts = (int64_t)splits * ((a.N + G8_BN - 1) / G8_BN);
    return parts > 1 ? parts * a.M * 4 : 0;
  }
  const int64_t nparts = std::min<int64_t>(256, std::max<int64_t>(1, a.K / 64));
  return nparts * a.M * 4;
}

// the implicit-convolution geometry of `a` (on = 0 without one), or an error string
const char* conv_geom(const mmfd_gemm_args& a, ConvGeom& g) {
  g = ConvGeom{};
  if (!a.conv) return nullptr;
  const mmfd_conv_geom& c = *a.conv;
  const int64_t kstep = a.dtype == MMFD_BF16 ? 64 : 32;  // K per K-tile / split-operand K-step
  if (a.trans_a) return "conv needs trans_a = 0";
  if (a.trans_b) return "conv needs trans_b = 0";  // only K-contiguous-B conv kernels exist
  if (c.N <= 0 || c.H <= 0 || c.W <= 0 || c.C <= 0 || c.KH <= 0 || c.KW <= 0 || c.stride <= 0 || c.pad < 0)
    return "conv: bad geometry";
  if (c.Ho != (c.H + 2 * c.pad - c.KH) / c.stride + 1 || c.Wo != (c.W + 2 * c.pad - c.KW) / c.stride + 1)
    return "conv: Ho / Wo do not match H, W, KH, KW, stride, pad";
  if (a.M != c.N * c.Ho * c.Wo || a.K != (int64_t)c.KH * c.KW * c.C) return "conv: M != N*Ho*Wo or K != KH*KW*C";
  if (c.C % kstep) return "conv: C must be a multiple of 32 (fp32) / 64 (bf16)";
  if (((uintptr_t)a.A & 15) != 0) return "conv: x must be 16-B aligned";
  if (a.a_rowsum || a.a_planes_only) return "conv: no a_rowsum / a_planes_only";
  const int64_t esz = a.dtype == MMFD_BF16 ? 2 : 4;
  if (c.N * c.H * c.W * c.C * esz >= (1ll << 31) - 4096) return "conv: activation >= 2 GB";
  g.on = 1; g.KW = c.KW; g.stride = c.stride; g.pad = c.pad;
  g.H = c.H; g.W = c.W; g.C = c.C; g.Ho = c.Ho; g.Wo = c.Wo;
  return nullptr;
}

EpiArgs make_epi(const mmfd_gemm_args& a) {
  EpiArgs e;
  e.bias = a.ep.bias; e.residual = a.ep.residual; e.ldr = a.ep.ldr; e.aux = a.ep.aux;
  e.ldaux = a.ep.ldaux; e.act = a.ep.act; e.p = a.ep.dropout_p > 0.f ? a.ep.dropout_p : 0.f;
  e.thr = mmfd_drop_threshold(e.p); e.keep_scale = 1.0f / (1.0f - e.p);
  e.seed = a.ep.seed; e.salt = a.ep.salt; e.beta = a.beta; e.res_first = a.ep.residual_first ? 1 : 0;
  e.pl = a.c_dtype == MMFD_F32 ? (bf16*)a.ep.out_planes : nullptr;
  e.pl_stride = a.M * a.N;
  e.c_out = (a.C != nullptr) ? 1 : 0;
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  bool v = (a.C == nullptr || al(a.C)) && (a.ldc % 8) == 0;
  if (a.ep.residual) v = v && al(a.ep.residual) && (a.ep.ldr % 8) == 0;
  if (a.ep.aux) v = v && al(a.ep.aux) && (a.ep.ldaux % 8) == 0;
  if (a.ep.bias) v = v && al(a.ep.bias);
  e.vec = v ? 1 : 0;
  return e;
}

// ---------------------------------------------------------------------------------------------
// the launch plan: everything a call decides before it launches
// ---------------------------------------------------------------------------------------------
enum Path { P_EMPTY, P_SIMPLE, P_T128, P_T128_CONV, P_G8, P_G8_X6SEG, P_X6F, P_X6F_CONV, P_G4 };
const char* const PATH_NAME[] = {"empty", "simple", "tile128", "tile128_conv", "tile256", "tile256_x6seg",
                                 "x6f", "x6f_conv", "g4"};
enum Reduce { R_NONE, R_VEC8, R_SCALAR, R_PARTIALS };

// What a product gets before the workspace at hand is looked at; the three queries answer from it.
struct Choice {
  bool mfma, g8;    // an MFMA path takes it (else the plain FMA kernel); on the 256x256 kernels
  X6Plan xp;        // xp.on: it runs on split operands
  int nkt, splits;  // K units in all, split count
  int g4;           // the four-wave kernel's epilogue mode, -1 when it does not take the product
  bool xs;          // the epilogue runs in the reduce only: raw sums go to a slab even at one split
  int64_t total;    // workspace bytes: slabs, row-sum partials, 256-aligned planes
};

struct GemmPlan {
  Path path;
  Choice c;  // as launched (the workspace may have ruled out split operands or shrunk the splits); c.total as asked
  bool pre;  // 256x256 bf16 output: one prefetched epilogue operand stream
  bool n64;  // 256x128 families: the 64-wide tile
  EpiArgs e;
  ConvGeom cg;
  G8Launch L;  // grid, epilogue form, units per split, rs_mode, plane leading dims, X6Args; run_plan sets the pointers
  int lds, persist;
  // workspace layout, byte offsets into a.workspace (-1: no such region; the planes' regions are split3's outputs)
  int64_t slab_off, rs_off, a_planes_off, b_planes_off;
  int rs_nparts;
  Reduce reduce;
  int P, reduce_blocks;
  bool colsum;  // row sums of op(A) off the 256x256 kernels: mmfd_colsum (trans_a only, else refused late)
  int64_t colsum_off, colsum_bytes;
};

// c.g4 and c.xs for c.splits. The four-wave kernel takes one-split bf16 -> bf16 products of the 256x256
// path that pass g4_epi. MMFD_ACT_GELU_D / MUL_AUX / TANH / SIGMOID need a slab (the reduce runs the
// epilogue) unless that kernel or the split-operand kernel's ext instantiation takes the product: GELU_D /
// MUL_AUX without dropout, one split, and every tile on the epilogue's fast path (full 256x256 tiles,
// 16-B aligned operands: its per-element path for partial tiles is the shared one, without the two)
void route(const mmfd_gemm_args& a, const EpiArgs& e, Choice& c) {
  const int act = a.ep.act;
  const bool one = c.splits == 1, bb = a.dtype == MMFD_BF16 && a.c_dtype == MMFD_BF16;
  c.g4 = (one && c.g8 && bb && !a.conv) ? mmfd_gemmx::g4_epi(a, e, 1) : -1;
  const bool ext = one && (act == MMFD_ACT_GELU_D || act == MMFD_ACT_MUL_AUX) && a.ep.dropout_p <= 0.f && !a.conv &&
                   c.xp.on && x6_fused() && a.M % 256 == 0 && a.N % 256 == 0 && e.vec;
  c.xs = act_ext(act) && c.g4 < 0 && !ext;
}

Choice choose(const mmfd_gemm_args& a, const EpiArgs& e, bool split_operands) {
  // (off the MFMA paths: one split, no four-wave kernel, the colsum fallback's partials)
  Choice c{mfma_ok(a), use_g8(a), X6Plan{}, 0, 1, -1, false, rowsum_ws_bytes(a, 1, false)};
  if (!c.mfma) return c;
  if (split_operands) c.xp = x6_plan(a, c.g8);
  c.nkt = (int)k_units(a, c.xp.on);
  c.splits = choose_splits(a, c.nkt, c.g8, c.xp.on);
  route(a, e, c);
  const int64_t mn4 = a.M * a.N * 4;
  c.total = (c.splits > 1 ? c.splits * mn4 : c.xs ? mn4 : 0) + rowsum_ws_bytes(a, c.splits, c.g8);
  if (c.xp.on)  // + the bf16 planes of the operands not handed over already split
    c.total = align256(c.total) + (a.a_planes ? 0 : align256(3 * c.xp.pa)) + (a.b_planes ? 0 : 3 * c.xp.pb);
  return c;
}

// Checks the arguments and decides the call for the workspace it carries; touches no HIP call.
int make_plan(const mmfd_gemm_args& a, GemmPlan& p) {
  p = GemmPlan{};
  p.slab_off = p.rs_off = p.a_planes_off = p.b_planes_off = -1;
  const int act = a.ep.act;
  MMFD_CHECK_ARG(a.dtype == MMFD_F32 || a.dtype == MMFD_BF16, "mmfd_gemm: bad dtype %d", a.dtype);
  MMFD_CHECK_ARG(a.c_dtype == MMFD_F32 || a.c_dtype == MMFD_BF16, "mmfd_gemm: bad c_dtype %d", a.c_dtype);
  MMFD_CHECK_ARG(a.M >= 0 && a.N >= 0 && a.K >= 0, "mmfd_gemm: negative shape");
  MMFD_CHECK_ARG(a.C != nullptr || (a.ep.out_planes != nullptr && a.c_dtype == MMFD_F32 && a.beta == 0.f),
                 "mmfd_gemm: null C (allowed only with fp32 out_planes and beta = 0)");
  MMFD_CHECK_ARG(a.ep.out_planes == nullptr || (a.N % 8 == 0 && ((uintptr_t)a.ep.out_planes & 15) == 0),
                 "mmfd_gemm: out_planes need N %% 8 == 0 and 16-B alignment");
  MMFD_CHECK_ARG(a.ldc >= a.N, "mmfd_gemm: ldc %lld < N %lld", (long long)a.ldc, (long long)a.N);
  MMFD_CHECK_ARG(act >= 0 && act <= MMFD_ACT_MUL_AUX, "mmfd_gemm: bad act %d", act);
  const bool bwd_act = act == MMFD_ACT_GELU_BWD || act == MMFD_ACT_RELU_BWD || act == MMFD_ACT_MUL_AUX;
  MMFD_CHECK_ARG(!bwd_act || a.ep.aux != nullptr, "mmfd_gemm: backward act needs aux");
  MMFD_CHECK_ARG(a.ep.dropout_p <= 0.f || a.ep.seed != nullptr, "mmfd_gemm: dropout needs seed");
  MMFD_CHECK_ARG(a.ep.dropout_p < 1.f, "mmfd_gemm: dropout p must be < 1");
  if (a.M == 0 || a.N == 0) return 0;
  MMFD_CHECK_ARG(a.K == 0 || (a.A && a.B), "mmfd_gemm: null operand");
  const EpiArgs& e = p.e = make_epi(a);
  Choice& c = p.c = choose(a, e, true);
  if (const char* why = conv_geom(a, p.cg)) return mmfd_set_error(MMFD_ERR_INVALID, "mmfd_gemm: %s", why);
  if (p.cg.on && !c.mfma)
    return mmfd_set_error(MMFD_ERR_UNSUPPORTED, "mmfd_gemm: conv with an unaligned / oversized B operand");
  // split operands only with the whole workspace they ask for (none when both operands come split and there
  // is no split-K), else the fp32 MFMA path; an operand whose fp32 copy was never written can only be read
  // through its planes: refuse every path that would read the fp32 copy (the simple kernel included)
  const int64_t total = c.total, mn4 = a.M * a.N * 4;
  if (c.xp.on && total > 0 && (!a.workspace || a.workspace_bytes < total)) c = choose(a, e, false);
  c.total = total;
  if ((a.a_planes_only || a.b_planes_only) && !c.xp.on)
    return mmfd_set_error(MMFD_ERR_UNSUPPORTED, "mmfd_gemm: an operand exists only as split planes, but this "
                          "product (M %lld N %lld K %lld) does not run on split operands", (long long)a.M,
                          (long long)a.N, (long long)a.K);
  G8Launch& L = p.L;
  L.lda = a.lda; L.ldb = a.ldb; L.x6 = X6Args{1, 0, 0};
  if (!c.mfma) {  // the plain FMA kernel (tiny / unaligned shapes: classifier heads)
    p.path = P_SIMPLE;
    L.grid = dim3((unsigned)std::min<int64_t>((a.M * a.N + 255) / 256, 4096));
    p.colsum = a.a_rowsum != nullptr;
    p.colsum_bytes = a.workspace_bytes;
    return 0;
  }
  const bool x6 = c.xp.on, xf = x6 && x6_fused(), g8 = c.g8;
  int splits = c.splits;
  if (!x6 && splits > 1 && (!a.workspace || a.workspace_bytes < splits * mn4 + rowsum_ws_bytes(a, splits, g8))) {
    // shrink to the slabs (each with its row-sum partial) that the workspace holds
    const int64_t fit = a.workspace ? a.workspace_bytes / (mn4 + (a.a_rowsum ? a.M * 4 : 0)) : 1;
    splits = fit > 1 ? (int)std::min<int64_t>(splits, std::min<int64_t>(fit, 32)) : 1;
  }
  L.tps = (c.nkt + splits - 1) / splits;
  splits = (c.nkt + L.tps - 1) / L.tps;
  if (splits != c.splits) {
    c.splits = splits;
    route(a, e, c);
  }
  if (c.xs) {
    MMFD_CHECK_ARG(!a.a_rowsum, "mmfd_gemm: act %d with a_rowsum is not supported", act);
    MMFD_CHECK_ARG(a.workspace && a.workspace_bytes >= splits * mn4,
                   "mmfd_gemm: act %d on this product needs a workspace of %lld bytes (mmfd_gemm_workspace_bytes)",
                   act, (long long)(splits * mn4));
  }
  // the layout: slabs first, the row-sum partials after them ([splits][column tiles][M] when the workspace
  // holds them: rs_mode 3; else the first column tile sums alone, per split or direct), then the planes
  const bool slabs = splits > 1 || c.xs;
  const int64_t slab_bytes = slabs ? splits * mn4 : 0, gxt = (a.N + G8_BN - 1) / G8_BN;
  if (slabs) p.slab_off = 0;
  p.rs_nparts = splits;
  if (a.a_rowsum && g8) {
    const bool rs3 = splits * gxt > 1 && a.workspace && a.workspace_bytes >= slab_bytes + splits * gxt * a.M * 4;
    L.rs_mode = rs3 ? 3 : (splits > 1 ? 2 : 1);
    if (rs3) p.rs_nparts = (int)(splits * gxt);
    if (L.rs_mode >= 2) p.rs_off = slab_bytes;
  }
  if (x6) {  // the planes' leading dim = the stored column count
    int64_t at = align256(slab_bytes + rowsum_ws_bytes(a, splits, true));
    if (!a.a_planes) { p.a_planes_off = at; at += align256(3 * c.xp.pa); }
    if (!a.b_planes) p.b_planes_off = at;
    L.lda = a.trans_a ? a.M : a.K; L.ldb = a.trans_b ? a.N : a.K;
    L.x6 = X6Args{xf ? c.nkt : (int)((a.K + 63) / 64), (uint32_t)c.xp.pa, (uint32_t)c.xp.pb};
  }
  // the kernel (with split-K slabs the tile kernel runs no epilogue at all: the reduce does)
  const bool lean = slabs || (act == MMFD_ACT_NONE && e.p <= 0.f);
  L.form = lean ? mmfd_gemmx::G8_LEAN : mmfd_gemmx::G8_ACT;
  p.lds = G8_LDS;
  L.grid = dim3((unsigned)gxt, (unsigned)((a.M + G8_BM - 1) / G8_BM), (unsigned)splits);  // (G8_BM == BM)
  if (xf) {
    p.path = p.cg.on ? P_X6F_CONV : P_X6F;
    if (!p.cg.on && !lean && (act == MMFD_ACT_GELU_D || act == MMFD_ACT_MUL_AUX)) L.form = mmfd_gemmx::G8_EXT;
  } else if (x6) {
    if (p.cg.on) return mmfd_set_error(MMFD_ERR_UNSUPPORTED, "mmfd_gemm: conv on the segmented split-operand kernel");
    p.path = P_G8_X6SEG;
  } else if (p.cg.on || !g8) {  // the 256x128 kernel; a convolution gathers its A rows per K-tile
    p.path = p.cg.on ? P_T128_CONV : P_T128;
    p.n64 = a.N <= 64 && (p.cg.on || !a.trans_b);  // the 256x64 tile (no zero half-tile of B)
    const int bnt = p.n64 ? 64 : BN;
    p.lds = NSTAGE * (A_BYTES + bnt * ROWB);
    L.grid.x = (unsigned)((a.N + bnt - 1) / bnt);
  } else if (c.g4 >= 0) {
    p.path = P_G4;
    p.persist = mmfd_gemmx::g_g4_persist;
  } else {
    p.path = P_G8;  // PRE: exactly one bf16 epilogue operand stream
    p.pre = a.c_dtype == MMFD_BF16 && (e.residual ? 1 : 0) + (bwd_act ? 1 : 0) + (e.beta != 0.f ? 1 : 0) == 1 && !slabs && e.vec;
  }
  // follow-ups
  if (slabs && e.vec && a.N % 8 == 0) {
    // split ranges per group: up to 8, while the threads stay under ~2^19 (2,048 per CU)
    const int64_t groups = a.M * a.N / 8;
    p.reduce = R_VEC8;
    p.P = 1;
    while (p.P < 8 && 2 * p.P <= splits && groups * p.P < ((int64_t)1 << 19)) p.P *= 2;
    const int G = 256 / p.P;
    p.reduce_blocks = (int)std::min<int64_t>(std::max<int64_t>((groups + G - 1) / G, (a.M + 255) / 256), 16384);
  } else if (slabs) {
    p.reduce = R_SCALAR;
    p.reduce_blocks = (int)std::min<int64_t>((a.M * a.N + 255) / 256, 8192);
  } else if (L.rs_mode == 3) {  // no split-K: only the column tiles' row-sum partials to reduce
    p.reduce = R_PARTIALS;
    p.reduce_blocks = (int)((a.M + 63) / 64);
  }
  p.colsum = a.a_rowsum && !g8;
  p.colsum_off = slab_bytes;
  p.colsum_bytes = a.workspace_bytes - slab_bytes;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// launching a plan: one ladder from (T, TC, TA, TB, variant) to the kernel per family
// ---------------------------------------------------------------------------------------------
template <int V> using IC = std::integral_constant<int, V>;
template <typename F> void by_layout(const mmfd_gemm_args& a, F f) {
  if (!a.trans_a && !a.trans_b) f(IC<0>{}, IC<0>{});
  else if (!a.trans_a) f(IC<0>{}, IC<1>{});
  else if (!a.trans_b) f(IC<1>{}, IC<0>{});
  else f(IC<1>{}, IC<1>{});
}
#define BY_TYPES(F, ...)                                                                                      \
  if (a.dtype == MMFD_BF16) { if (a.c_dtype == MMFD_BF16) F<bf16, bf16>(__VA_ARGS__); else F<bf16, float>(__VA_ARGS__); } \
  else { if (a.c_dtype == MMFD_BF16) F<float, bf16>(__VA_ARGS__); else F<float, float>(__VA_ARGS__); }

// the plain FMA kernel and the 256x128 kernels of one (T, TC)
template <typename T, typename TC>
void launch_t128(const mmfd_gemm_args& a, const GemmPlan& p, float* ws, hipStream_t s) {
  // (T128_GO leaves the argument list open: a convolution appends its geometry)
#define T128_GO(KERNEL, LDS, ...)                                                                        \
  lds_max<&KERNEL>(LDS);                                                                                 \
  hipLaunchKernelGGL((KERNEL), p.L.grid, dim3(NT), LDS, s, (const T*)a.A, __VA_ARGS__, (TC*)a.C, a.ldc, ws, a.M, a.N, \
                     a.K, a.alpha, p.L.tps, p.e
  if (p.path == P_SIMPLE)
    hipLaunchKernelGGL((gemm_simple_kernel<T, TC>), p.L.grid, dim3(256), 0, s, (const T*)a.A, a.lda, a.trans_a,
                       (const T*)a.B, a.ldb, a.trans_b, (TC*)a.C, a.ldc, a.M, a.N, a.K, a.alpha, p.e);
  else if (p.path == P_T128_CONV && p.n64) { T128_GO((conv_mfma_kernel<T, TC, 64>), p.lds, (const T*)a.B, a.ldb), p.cg); }
  else if (p.path == P_T128_CONV) { T128_GO((conv_mfma_kernel<T, TC, BN>), p.lds, (const T*)a.B, a.ldb), p.cg); }
  else by_layout(a, [&](auto ta, auto tb) {
    constexpr int TA = decltype(ta)::value, TB = decltype(tb)::value;
    if constexpr (TB == 0) {
      if (p.n64) { T128_GO((gemm_mfma_n64_kernel<T, TA, TC>), p.lds, a.lda, (const T*)a.B, a.ldb)); return; }
    }
    T128_GO((gemm_mfma_kernel<T, TA, TB, TC>), LDS_BYTES, a.lda, (const T*)a.B, a.ldb));
  });
#undef T128_GO
}

// the split-K reduce of one TC; it also reduces the row sums' partials (rs_mode 2 / 3)
template <typename T, typename TC>
void launch_reduce(const mmfd_gemm_args& a, const GemmPlan& p, float* ws, const float* rsp, hipStream_t s) {
#define REDUCE_GO(KERNEL)                                                                                 \
  hipLaunchKernelGGL((KERNEL), dim3(p.reduce_blocks), dim3(256), 0, s, ws, p.c.splits, (TC*)a.C, a.ldc, a.M, a.N, \
                     p.e, rsp, p.rs_nparts, a.a_rowsum, a.a_rowsum_beta)
  if (p.reduce == R_SCALAR) REDUCE_GO((splitk_reduce_kernel<TC>));
  else if (p.P == 8) REDUCE_GO((splitk_reduce8_kernel<TC, 8>));
  else if (p.P == 4) REDUCE_GO((splitk_reduce8_kernel<TC, 4>));
  else if (p.P == 2) REDUCE_GO((splitk_reduce8_kernel<TC, 2>));
  else REDUCE_GO((splitk_reduce8_kernel<TC, 1>));
#undef REDUCE_GO
}

int run_plan(const GemmPlan& p, const mmfd_gemm_args& a, hipStream_t s) {
  if (p.path == P_EMPTY) return 0;
  char* const wsb = (char*)a.workspace;
  float* const ws = p.slab_off >= 0 ? (float*)(wsb + p.slab_off) : nullptr;
  float* const rs_part = p.rs_off >= 0 ? (float*)(wsb + p.rs_off) : nullptr;
  const EpiArgs& e = p.e;
  const X6Plan& xp = p.c.xp;
  G8Launch L = p.L;
  L.ws = ws;
  L.rs_out = rs_part ? rs_part : a.a_rowsum;
  L.A = !xp.on ? a.A : a.a_planes ? a.a_planes : wsb + p.a_planes_off;
  L.B = !xp.on ? a.B : a.b_planes ? a.b_planes : wsb + p.b_planes_off;
  if (p.a_planes_off >= 0)
    launch_split3((const float*)a.A, p.cg.on ? p.cg.C : a.lda, xp.rows_a, xp.cols_a, (bf16*)L.A, s);
  if (p.b_planes_off >= 0) launch_split3((const float*)a.B, a.ldb, xp.rows_b, xp.cols_b, (bf16*)L.B, s);
  if (xp.on) MMFD_CHECK_LAUNCH("split3");

  switch (p.path) {
    case P_G8:  // fp32-output instantiations live in gemm_f32out.hip (built without SLP vectorisation)
      by_layout(a, [&](auto ta, auto tb) {
        constexpr int TA = decltype(ta)::value, TB = decltype(tb)::value;
        if (a.c_dtype == MMFD_BF16 && p.pre) launch_g8_v<bf16, TA, TB, bf16, true, false>(a, e, L, s);
        else if (a.c_dtype == MMFD_BF16) launch_g8_v<bf16, TA, TB, bf16, false, false>(a, e, L, s);
        else if (a.dtype == MMFD_BF16) mmfd_gemmx::launch_g8_f32out<bf16, TA, TB, false>(a, e, L, s);
        else mmfd_gemmx::launch_g8_f32out<float, TA, TB, false>(a, e, L, s);
      });
      break;
    case P_G8_X6SEG:
      by_layout(a, [&](auto ta, auto tb) { mmfd_gemmx::launch_g8_f32out<bf16, decltype(ta)::value, decltype(tb)::value, true>(a, e, L, s); });
      break;
    case P_X6F:
      by_layout(a, [&](auto ta, auto tb) { mmfd_gemmx::launch_x6f<decltype(ta)::value, decltype(tb)::value>(a, e, L, s); });
      break;
    case P_X6F_CONV: mmfd_gemmx::launch_conv_x6f(a, e, L, p.cg, s); break;
    case P_G4: {  // persistent: one workgroup per CU (looked up here, so the plan is the same without a device)
      const int64_t tiles = (a.M / 256) * (a.N / 256);
      mmfd_gemmx::launch_g4(a, e, p.c.g4, p.persist ? std::min<int64_t>(tiles, mmfd_gemmx::g4_cus()) : tiles, s);
      break;
    }
    default: BY_TYPES(launch_t128, a, p, ws, s); break;
  }
  MMFD_CHECK_LAUNCH(p.path == P_SIMPLE ? "gemm_simple" : "gemm_mfma");

  if (p.reduce == R_PARTIALS) {
    hipLaunchKernelGGL(mmfd_reduce_partials_kernel, dim3((unsigned)p.reduce_blocks), dim3(1024), 0, s,
                       (const float*)rs_part, p.rs_nparts, a.M, a.M, a.a_rowsum, a.a_rowsum_beta);
    MMFD_CHECK_LAUNCH("rowsum_reduce");
  } else if (p.reduce != R_NONE) {
    BY_TYPES(launch_reduce, a, p, ws, rs_part, s);
    MMFD_CHECK_LAUNCH("splitk_reduce");
  }
  if (!p.colsum) return 0;
  // row sums of op(A) off the 256x256 kernels: with trans_a, op(A) rows are the columns of the stored [K][M]
  // matrix, i.e. mmfd_colsum
  if (!a.trans_a)
    return mmfd_set_error(MMFD_ERR_UNSUPPORTED, "mmfd_gemm: a_rowsum without trans_a needs the bf16 MFMA path");
  return mmfd_colsum(a.dtype, a.K, a.M, a.A, a.lda, a.a_rowsum, a.a_rowsum_beta, wsb + p.colsum_off, p.colsum_bytes, s);
}

// The queries answer for a caller that supplies the whole workspace; they refuse nothing but arguments of
// another ABI layout (struct_size): -1, error string set.
bool query(const mmfd_gemm_args* a, const char* what, Choice& c) {
  if (!a || a->struct_size != (int64_t)sizeof(mmfd_gemm_args)) {
    mmfd_set_error(MMFD_ERR_INVALID, "%s: mmfd_gemm_args.struct_size = %lld, this library expects %lld (ABI version %d)",
                   what, a ? (long long)a->struct_size : 0ll, (long long)sizeof(mmfd_gemm_args), MMFD_ABI_VERSION);
    return false;
  }
  c = choose(*a, make_epi(*a), true);
  return true;
}

}  // namespace

extern "C" int64_t mmfd_gemm_workspace_bytes(const mmfd_gemm_args* a) {
  Choice c;
  return query(a, "mmfd_gemm_workspace_bytes", c) ? c.total : -1;
}

extern "C" int mmfd_gemm_splits(const mmfd_gemm_args* a) {
  Choice c;
  return query(a, "mmfd_gemm_splits", c) ? c.splits : -1;
}

extern "C" int mmfd_gemm_runs_split(const mmfd_gemm_args* a) {
  Choice c;
  return query(a, "mmfd_gemm_runs_split", c) ? (c.xp.on ? (x6_fused() ? 2 : 1) : 0) : -1;
}

extern "C" int mmfd_set_fp32_gemm_mode(int mode) {
  MMFD_CHECK_ARG(mode == 0 || mode == 1, "mmfd_set_fp32_gemm_mode: mode %d (0 = fp32 MFMA, 1 = split operands)", mode);
  const int old = g_gemm_sw.fp32_mode;
  g_gemm_sw.fp32_mode = mode;
  return old;
}

// A/B switches by their environment names (not part of include/mmfd.h; tests reach both sides of a
// switch in one process): sets it (MMFD_G8_GROUP_M: at least 1; the others 0 / 1) and returns the old
// value, -1 for an unknown name
extern "C" int mmfd_debug_set_gemm_switch(const char* name, int value) {
  const char* const names[] = {"MMFD_GEMM_V1", "MMFD_GEMM_F32_V1", "MMFD_GEMM_NARROW_G8", "MMFD_X6_SEGMENTED", "MMFD_G8_GROUP_M"};
  int* const fields[] = {&g_gemm_sw.v1, &g_gemm_sw.f32_v1, &g_gemm_sw.narrow_g8, &g_gemm_sw.x6_segmented, &g_gemm_sw.group_m};
  for (int i = 0; i < 5; ++i) {
    if (!name || strcmp(name, names[i])) continue;
    const int old = *fields[i];
    *fields[i] = i == 4 ? std::max(1, value) : (value != 0);
    return old;
  }
  mmfd_set_error(MMFD_ERR_INVALID, "mmfd_debug_set_gemm_switch: unknown switch %s", name ? name : "(null)");
  return -1;
}

extern "C" int mmfd_gemm(const mmfd_gemm_args* ap, mmfd_stream_t stream) {
  MMFD_CHECK_STRUCT(ap, mmfd_gemm_args, "mmfd_gemm");
  GemmPlan p;
  const int rc = make_plan(*ap, p);
  return rc ? rc : run_plan(p, *ap, (hipStream_t)stream);
}

// The plan of a call as text, for the workspace the arguments carry, without launching anything or
// touching HIP (not part of include/mmfd.h; the pointers in `a` are never dereferenced). A header line
//   path= splits= units= rs=<rs_mode>,<rs_nparts> flags=<vec>,<c_out>,<planes written>
//   ws=<slabs>,<row-sum partials>,<A planes>,<B planes>,<total>
// (workspace byte offsets, -1 = no such region; the total is what mmfd_gemm_workspace_bytes answers)
// then one line per launch in order, the kernel named as rocprof demangles it, with grid=, block=,
// lds= (the four-wave kernel: tiles= persist= for its grid); "mmfd_colsum ws_off= ws_bytes=" for the
// column-sum fallback. An empty call writes an empty string. Returns the call's refusal code.
extern "C" int mmfd_debug_gemm_plan(const mmfd_gemm_args* a, char* buf, int64_t bytes) {
  MMFD_CHECK_ARG(buf && bytes > 0, "mmfd_debug_gemm_plan: no buffer");
  buf[0] = 0;
  MMFD_CHECK_STRUCT(a, mmfd_gemm_args, "mmfd_gemm");
  GemmPlan p;
  int rc = make_plan(*a, p);
  if (rc || p.path == P_EMPTY) return rc;
  int64_t at = 0;
  auto put = [&](const char* fmt, auto... v) {
    if (at < bytes) at += snprintf(buf + at, (size_t)(bytes - at), fmt, v...);
  };
  auto launch = [&](dim3 g, int block, int lds) { put(" grid=%u,%u,%u block=%d lds=%d\n", g.x, g.y, g.z, block, lds); };
  const char* const t = a->dtype == MMFD_BF16 ? "__bf16" : "float";
  const char* const tc = a->c_dtype == MMFD_BF16 ? "__bf16" : "float";
  const char* const form = p.L.form == mmfd_gemmx::G8_LEAN ? "" : p.L.form == mmfd_gemmx::G8_ACT ? "_act" : "_ext";
  const int ta = a->trans_a ? 1 : 0, tb = a->trans_b ? 1 : 0;
  const X6Plan& xp = p.c.xp;
  put("path=%s splits=%d units=%d rs=%d,%d flags=%d,%d,%d ws=%lld,%lld,%lld,%lld,%lld\n", PATH_NAME[p.path],
      p.c.splits, p.L.tps, p.L.rs_mode, p.rs_nparts, p.e.vec, p.e.c_out, p.e.pl ? 1 : 0, (long long)p.slab_off,
      (long long)p.rs_off, (long long)p.a_planes_off, (long long)p.b_planes_off, (long long)p.c.total);
  auto split3 = [&](int64_t rows, int64_t cols) {
    put("%s", "split3_kernel");
    launch(dim3((unsigned)std::min<int64_t>((rows * (cols / 8) + 255) / 256, 8192)), 256, 0);
  };
  if (p.a_planes_off >= 0) split3(xp.rows_a, xp.cols_a);
  if (p.b_planes_off >= 0) split3(xp.rows_b, xp.cols_b);
  switch (p.path) {
    case P_SIMPLE: put("gemm_simple_kernel<%s, %s>", t, tc); launch(p.L.grid, 256, 0); break;
    case P_T128:
      if (p.n64) put("gemm_mfma_n64_kernel<%s, %d, %s>", t, ta, tc);
      else put("gemm_mfma_kernel<%s, %d, %d, %s>", t, ta, tb, tc);
      launch(p.L.grid, NT, p.lds);
      break;
    case P_T128_CONV: put("conv_mfma_kernel<%s, %s, %d>", t, tc, p.n64 ? 64 : BN); launch(p.L.grid, NT, p.lds); break;
    case P_G8:
    case P_G8_X6SEG:
      put("gemm256%s_kernel<%s, %d, %d, %s, %s, %s>", form, p.path == P_G8_X6SEG ? "__bf16" : t, ta, tb, tc,
          p.pre ? "true" : "false", p.path == P_G8_X6SEG ? "true" : "false");
      launch(p.L.grid, NT, p.lds);
      break;
    case P_X6F: put("gemm256_x6f%s_kernel<%d, %d>", form, ta, tb); launch(p.L.grid, NT, p.lds); break;
    case P_X6F_CONV: put("%s", "conv_x6f_kernel"); launch(p.L.grid, NT, p.lds); break;
    case P_G4:
      put("gemm_g4_kernel<%d> tiles=%lld persist=%d block=256 lds=0\n", p.c.g4, (long long)((a->M / 256) * (a->N / 256)),
          p.persist);
      break;
    case P_EMPTY: break;
  }
  if (p.reduce == R_VEC8) { put("splitk_reduce8_kernel<%s, %d>", tc, p.P); launch(dim3(p.reduce_blocks), 256, 0); }
  else if (p.reduce == R_SCALAR) { put("splitk_reduce_kernel<%s>", tc); launch(dim3(p.reduce_blocks), 256, 0); }
  else if (p.reduce == R_PARTIALS) { put("%s", "mmfd_reduce_partials_kernel"); launch(dim3(p.reduce_blocks), 1024, 0); }
  if (p.colsum && !a->trans_a)
    rc = mmfd_set_error(MMFD_ERR_UNSUPPORTED, "mmfd_gemm: a_rowsum without trans_a needs the bf16 MFMA path");
  else if (p.colsum)
    put("mmfd_colsum ws_off=%lld ws_bytes=%lld\n", (long long)p.colsum_off, (long long)p.colsum_bytes);
  MMFD_CHECK_ARG(at < bytes, "mmfd_debug_gemm_plan: buffer of %lld bytes is too small", (long long)bytes);
  return rc;
}

extern "C" int mmfd_split3(int64_t rows, int64_t cols, const float* x, int64_t ld, void* planes, mmfd_stream_t stream) {
  MMFD_CHECK_ARG(rows >= 0 && cols >= 0 && ld >= cols, "mmfd_split3: bad shape");
  MMFD_CHECK_ARG(cols % 8 == 0 && ld % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)planes & 15) == 0,
                 "mmfd_split3: cols must be a multiple of 8 and rows 16-B aligned");
  MMFD_CHECK_ARG(rows * (cols / 8) < (1ll << 32) && rows * ld < (1ll << 31), "mmfd_split3: matrix too large");
  if (rows == 0 || cols == 0) return 0;
  launch_split3(x, ld, rows, cols, (bf16*)planes, (hipStream_t)stream);
  MMFD_CHECK_LAUNCH("split3");
  return 0;
}

// column sums (bias gradients), deterministic two-pass: per-block partials (gemm_colsum.h), then
// mmfd_reduce_partials_kernel
extern "C" int mmfd_colsum(int dtype, int64_t M, int64_t N, const void* X, int64_t ldx, float* out,
                           float beta, void* workspace, int64_t workspace_bytes, mmfd_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  MMFD_CHECK_ARG(dtype == MMFD_F32 || dtype == MMFD_BF16, "mmfd_colsum: bad dtype");
  if (N == 0) return 0;
  int nparts = (int)std::min<int64_t>(256, std::max<int64_t>(1, M / 64));
  if (workspace_bytes < (int64_t)nparts * N * 4) nparts = (int)(workspace_bytes / (N * 4));
  MMFD_CHECK_ARG(nparts >= 1 && workspace, "mmfd_colsum: workspace too small");
  const int64_t rpb = (M + nparts - 1) / nparts;
  const int epc = dtype == MMFD_BF16 ? 8 : 4;
  const bool vec = (N % epc) == 0 && (ldx % epc) == 0 && ((uintptr_t)X & 15) == 0;
  const dim3 g1((unsigned)(vec ? (N / epc + 63) / 64 : (N + 255) / 256), (unsigned)nparts);
  auto pass1 = [&](auto t) {
    using T = decltype(t);
    if (vec) hipLaunchKernelGGL((colsum_partial_vec_kernel<T>), g1, dim3(256), 0, s, (const T*)X, ldx, M, N, rpb, (float*)workspace);
    else hipLaunchKernelGGL((colsum_partial_kernel<T>), g1, dim3(256), 0, s, (const T*)X, ldx, M, N, rpb, (float*)workspace);
  };
  if (dtype == MMFD_BF16) pass1(bf16{}); else pass1(float{});
  hipLaunchKernelGGL(mmfd_reduce_partials_kernel, dim3((unsigned)((N + 63) / 64)), dim3(1024), 0, s,
                     (const float*)workspace, nparts, N, N, out, beta);
  MMFD_CHECK_LAUNCH("colsum");
  return 0;
}
