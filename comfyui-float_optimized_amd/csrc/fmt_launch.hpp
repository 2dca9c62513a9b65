// From a GemmArgs to a launch: the FMT's kernel instantiation lists, the raising of their dynamic-LDS limits, the tiling
// choices, and the launchers of the GEMM families (generic, wide, LDS-DMA, persistent projection, row-blocked), LayerNorm,
// and attention.  Knows nothing of struct float_fmt: launchers that read a handle's workspace get it
// through FmtLaunch.  Included by fmt_api.hip only, after the kernel headers (the one translation unit that holds the FMT
// kernels' instantiations).
#pragma once
#include <type_traits>

#include "fmt_weights.hpp"

namespace {

constexpr int kLdsMax = 160 * 1024;  // gfx950: 160 KiB of LDS per workgroup
constexpr int kWtRows = 256;  // LayerNorm / attention launches of at most this many rows store write-through (common.hpp, FMT_WT)

typedef void (*GemmKernel)(GemmArgs);
// fmt_gemm_kernel: the members of GemmHead as scalar parameters, then the tail (fmt_gemm_launch passes them)
typedef void (*GemmHeadKernel)(const u16*, const u16*, int, int, int, int, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, GemmTail);

// dynamic LDS above the 64 KiB default, once per process and kernel
template <class K>
void raise_lds(K kern, int bytes) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
    (void)hipGetLastError();
}

// A run-time value as a template argument: f(std::integral_constant<int, V>) for the V among Vs that equals v (false: none does)
template <int... Vs, class F>
bool with_const(int v, F&& f) {
  return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// What the launchers that read a handle's workspace are given: the handle's switches, the stream, the range counter of the
// 16-bit activation stores, and the buffers and sizes of the block chain.
struct FmtLaunch {
  const FmtTune& tn;
  hipStream_t s;
  unsigned long long* sat;
  float *xres, *slab;  // residual stream [Mpad][D]; split-K partial sums [8][Mpad][D]
  u16 *h16, *qkv16, *att16;
  int D, ntok, Ntot, Mpad, heads, attn_window;
};

// ---- the instantiation lists: prime_kernels and the launchers both walk them, so a tiling is added by one line here ----

// fmt_gemm_kernel, f(kernel, row tiles, column tiles, waves splitting K per workgroup, dynamic LDS).  Split tilings (a
// quarter/third/half of the CFG rows per workgroup) carry every epilogue and 4/8/16 K-splitting waves; full-height tilings (LDS
// bound) only the two epilogues that need them: EPI_CFG (all CFG rows of a token in one workgroup) and EPI_F32.  A listed tiling
// may need more LDS than a workgroup has (launch_gemm refuses it).
template <int MTW, int NT>
struct Tile {};
template <class T, int EPI, int NW, class F, int... MTW, int... NT>
void gemm_tiles(F& f, Tile<MTW, NT>...) {
  (f(fmt_gemm_kernel<T, MTW, NT, NW, EPI>, MTW, NT, NW, NW * MTW * 16 * NT * 16 * (int)sizeof(float)), ...);
}
template <class T, int EPI, int NW, class F>
void gemm_split_tiles(F& f) {
  gemm_tiles<T, EPI, NW>(f, Tile<3, 1>{}, Tile<3, 2>{}, Tile<3, 4>{}, Tile<5, 1>{}, Tile<5, 2>{}, Tile<5, 4>{}, Tile<4, 1>{},
                         Tile<4, 2>{}, Tile<6, 2>{}, Tile<2, 1>{}, Tile<1, 1>{});
}
template <class T, int EPI, class F>
void for_each_gemm(F&& f) {
  if constexpr (T::is32) {
    // the fp32 verification mode runs a handful of 16-column tilings (pick_tiling32): speed is not its point
    gemm_tiles<T, EPI, 4>(f, Tile<1, 1>{}, Tile<2, 1>{}, Tile<3, 1>{}, Tile<4, 1>{}, Tile<5, 1>{});
    if constexpr (EPI == EPI_CFG) gemm_tiles<T, EPI, 8>(f, Tile<1, 1>{}, Tile<3, 1>{}, Tile<4, 1>{});
  } else {
    gemm_split_tiles<T, EPI, 4>(f);
    gemm_split_tiles<T, EPI, 8>(f);
    gemm_split_tiles<T, EPI, 16>(f);
    if constexpr (EPI == EPI_F32 || EPI == EPI_CFG) {
      gemm_tiles<T, EPI, 4>(f, Tile<12, 2>{}, Tile<15, 2>{}, Tile<12, 1>{}, Tile<15, 1>{});
      gemm_tiles<T, EPI, 8>(f, Tile<12, 1>{}, Tile<15, 1>{});
    }
  }
}
// fmt_gemm_wide_kernel, f(kernel, row tiles, k-blocks per LDS chunk, waves, dynamic LDS)
template <int MTW, int KCH, int NWV>
struct WideTile {};
template <class T, class F, int... MTW, int... KCH, int... NWV>
void wide_tiles(F& f, WideTile<MTW, KCH, NWV>...) {
  (f(fmt_gemm_wide_kernel<T, MTW, KCH, NWV>, MTW, KCH, NWV, 2 * MTW * KCH * 1024), ...);
}
template <class T, class F>
void for_each_wide(F&& f) {  // 8 waves: two per SIMD, rows split over the wave pairs
  wide_tiles<T>(f, WideTile<4, 4, 4>{}, WideTile<5, 4, 4>{}, WideTile<6, 4, 4>{}, WideTile<6, 2, 4>{}, WideTile<12, 2, 4>{},
                WideTile<12, 4, 4>{}, WideTile<12, 2, 8>{}, WideTile<12, 4, 8>{});
}
// fmt_gemm_dma_kernel, f(kernel, wave columns, ring stages, wave rows half a step apart, dynamic LDS)
template <class T, int NWC, int NS, int STG, class F>
void dma_tile(F& f) {
  f(fmt_gemm_dma_kernel<T, NWC, NS, STG>, NWC, NS, STG, NS * (12 + 5 * NWC) * 1024);
}
template <class T, class F>
void for_each_dma(F&& f) {
  dma_tile<T, 4, 4, 0>(f);
  dma_tile<T, 4, 4, 1>(f);
}
// fmt_gemm_rbs_kernel, f(kernel, shape, rows, columns, k-blocks per stage, dynamic LDS);
// tile shapes built: 0 = 96 x 64 (two workgroups per CU), 1 = 96 x 128, 2 = 192 x 128 (ring of 3)
template <class T, int EPI, int MI, int NJ, int KPS, int NS, class F>
void rbs_tile(F& f, int shape) {
  f(fmt_gemm_rbs_kernel<T, MI, NJ, KPS, NS, EPI>, shape, 32 * MI, 32 * NJ, KPS, fmt_rb_smem(MI, NJ, KPS, NS));
}
template <class T, int EPI, class F>
void for_each_rbs(F&& f) {
  rbs_tile<T, EPI, 3, 2, 2, 4>(f, 0);
  rbs_tile<T, EPI, 3, 4, 2, 4>(f, 1);
  rbs_tile<T, EPI, 6, 4, 2, 3>(f, 2);
}

// the persistent projection kernel: one workgroup per CU (fmt_gemm_big4_kernel)
constexpr int kBigSmem = 4 * 28 * 1024 + 4 * 4096;

template <class T>
void prime_kernels() {
  auto raise = [](auto kern, int, int, int, int smem) {
    if (smem <= kLdsMax) raise_lds(kern, smem);
  };
  for_each_gemm<T, EPI_F32>(raise);
  for_each_gemm<T, EPI_T16>(raise);
  for_each_gemm<T, EPI_SILU_P16>(raise);
  for_each_gemm<T, EPI_GELU_P16>(raise);
  for_each_gemm<T, EPI_GATE_RES>(raise);
  for_each_gemm<T, EPI_XEMBED>(raise);
  for_each_gemm<T, EPI_CFG>(raise);
  for_each_gemm<T, EPI_PARTIAL>(raise);
  for_each_gemm<T, EPI_GELUERF_P16>(raise);
  if constexpr (!T::is32) {
    auto raise_rb = [](GemmKernel kern, int, int, int, int, int smem) { raise_lds(kern, smem); };
    raise_lds(fmt_gemm_big4_kernel<T, 4>, kBigSmem);
    for_each_dma<T>(raise);
    for_each_wide<T>(raise);
    for_each_rbs<T, EPI_T16>(raise_rb);
    for_each_rbs<T, EPI_GELU_P16>(raise_rb);
    for_each_rbs<T, EPI_PARTIAL>(raise_rb);
  }
}

// ---- launchers of the GEMM families ----

// Wide-N path (fused adaLN projection): LDS-staged A, 128 columns per workgroup (FmtTune::wide_variant picks the kernel).
template <class T>
int launch_wide_tile(GemmArgs g, int mtw, int kch, int nwv, hipStream_t s) {
  GemmKernel kern = nullptr;
  int smem = 0;
  for_each_wide<T>([&](GemmKernel k, int m, int c, int w, int bytes) {
    if (m == mtw && c == kch && w == nwv) kern = k, smem = bytes;
  });
  FH_REQUIRE(kern, "no wide GEMM tiling (%d row tiles, %d k-blocks per chunk, %d waves)", mtw, kch, nwv);
  const int mt_total = (g.M + 15) / 16;
  g.mblk = (mt_total + mtw - 1) / mtw;
  g.ksplit = 1;
  const dim3 grid((g.N / 128) * g.mblk * (g.zcount > 1 ? g.zcount : 1));
  fh_launch_prof(2, kern, grid, dim3(nwv * 64), smem, s, g);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}
// 192 x 320 tiles with both operands by LDS-DMA (fmt_gemm_dma_kernel): 8 waves, ring of 4 stages, one workgroup per CU; N in
// blocks of 320 columns and an even number (>= 4) of k-blocks.  Measured per launch of the hoisted projection (50 x 180 rows,
// 0.944 TFLOP), rocprofv3, bitwise the same numbers in every form:
//   register-staged 192 x 128 tile (variant 2)                                   1376 us  (686 TFLOP/s)
//   LDS-DMA tile, waves in lock step, stores straight from the accumulators      1260
//   + output through LDS (whole lines per store)                                 1150
//   + 2 column blocks per XCD group instead of 4 (FLOAT_FMT_ZGROUP)              1045     (variant 6)
//   + wave rows half a step apart (variant 7, the default)                       1021     (924 TFLOP/s, 37 % of the MFMA peak)
//   the same with the DMA pieces issued between the MFMA rows                    1115
// Not faster: 4 waves / 160 columns / ring of 3 with two workgroups per CU (1458), fragment reads spread between the MFMA rows
// (1172), a staggered start of the first workgroup generation, non-temporal stores.  In-kernel clocks (s_memtime /
// s_memrealtime) put a 32-step tile at ~49 000 clocks at 2.1 GHz, of which the bare barrier skeleton is a third.
template <class T>
int launch_dma(GemmArgs g, int nwc, int ns, int stg, hipStream_t s) {
  GemmKernel kern = nullptr;
  int smem = 0;
  for_each_dma<T>([&](GemmKernel k, int c, int n, int st, int bytes) {
    if (c == nwc && n == ns && st == stg) kern = k, smem = bytes;
  });
  FH_REQUIRE(kern, "no LDS-DMA GEMM tile (%d wave columns, ring of %d, stagger %d)", nwc, ns, stg);
  g.mblk = ((g.M + 15) / 16 + 11) / 12;
  const dim3 grid((g.N / (80 * nwc)) * g.mblk * (g.zcount > 1 ? g.zcount : 1));
  fh_launch_prof(2, kern, grid, dim3(nwc * 128), smem, s, g);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}
bool dma_shape_ok(const GemmArgs& g, int bn) { return g.N % bn == 0 && g.K % 64 == 0 && g.K >= 128; }

// The hoisted projection of a whole batch of evaluations on DENSE rows: the persistent one-wave-per-SIMD kernel
// (fmt_big_kernels.hpp), one workgroup per CU.  N in column blocks of 256, eight of them per XCD group; an even number (>= 4) of
// k-blocks (the K loop is unrolled by two behind four peeled steps).  Bitwise the numbers of fmt_gemm_dma_kernel.
// FLOAT_FMT_BIG=0 keeps the one-tile-per-workgroup kernels on rows padded per evaluation (the A/B switch).
constexpr int kBigMinRows = 1536;  // below 8 row blocks the padded layout's kernels stay (a single evaluation: 180 rows)
bool big_shape_ok(const FmtTune& tn, int rows_total, int N, int K, int n_cu) {
  return tn.big && rows_total >= kBigMinRows && N % 2048 == 0 && K % 64 == 0 && K >= 128 && n_cu >= 8;
}
template <class T>
int launch_big4(const u16* A, const FmtLin& L, float* out, int rows_total, int ldo, int n_cu, hipStream_t s) {
  if constexpr (T::is32) {
    fh_set_error("the fp32 verification mode has no persistent projection kernel");
    return FLOAT_E_INVALID;
  } else {
    BigArgs g{A, L.W, L.b, out, rows_total, L.N, L.K, ldo, (rows_total + 191) / 192, L.N / 256};
    const dim3 grid((unsigned)((n_cu / 8) * 8));
    fh_launch_prof(2, fmt_gemm_big4_kernel<T, 4>, grid, dim3(256), kBigSmem, s, g);
    FH_CHECK_HIP(hipGetLastError());
    return FLOAT_OK;
  }
}

template <class T>
int launch_wide(const GemmArgs& g, int variant, hipStream_t s) {
  const int mt = (g.M + 15) / 16;
  if ((variant == 6 || variant == 7) && mt > 4 && dma_shape_ok(g, 320)) return launch_dma<T>(g, 4, 4, variant == 7 ? 1 : 0, s);
  if (mt <= 4) return launch_wide_tile<T>(g, 4, 4, 4, s);
  // 192-row blocks also for the stacked clips of a batch (mt > 12): the last block reads up to 11 row tiles past the batch (the
  // operand buffers are padded for it, the rows are never stored); 80-row blocks ran the batched projection at 240 TFLOP/s
  // against 700 for 192-row ones
  if (variant == 6 || variant == 7) variant = 2;  // shapes the LDS-DMA tile does not take
  static const int by_variant[6][3] = {{6, 4, 4}, {6, 2, 4}, {12, 2, 4}, {12, 4, 4}, {12, 2, 8}, {12, 4, 8}};
  if (mt <= 12 || variant == 2 || variant >= 4) {
    const int* t = by_variant[variant >= 1 && variant <= 5 ? variant : 0];
    return launch_wide_tile<T>(g, t[0], t[1], t[2], s);
  }
  return launch_wide_tile<T>(g, 5, 4, 4, s);
}

// The weight-streaming GEMM (fmt_gemm_kernel) with `mtw` x `nt` tiles and `nw` K-splitting waves per workgroup
template <class T, int EPI>
int launch_gemm(GemmArgs g, int mtw, int nt, int nw, hipStream_t s) {
  FH_REQUIRE(g.N % (nt * 16) == 0 && g.K % (32 * nw * ((EPI == EPI_PARTIAL && g.ksplit > 1) ? g.ksplit : 1)) == 0,
             "gemm shape N=%d K=%d not tileable by %d columns / %d waves", g.N, g.K, nt * 16, nw);
  GemmHeadKernel kern = nullptr;
  int smem = 0;
  for_each_gemm<T, EPI>([&](GemmHeadKernel k, int m, int n, int w, int bytes) {
    if (m == mtw && n == nt && w == nw) kern = k, smem = bytes;
  });
  FH_REQUIRE(kern, "no GEMM tiling (%d x %d tiles, %d waves) for epilogue %d", mtw, nt, nw, EPI);
  FH_REQUIRE(smem <= kLdsMax, "GEMM tiling %dx%d tiles with %d waves needs %d B of LDS", mtw, nt, nw, smem);
  const int mt_total = (g.M + 15) / 16;
  g.mblk = (mt_total + mtw - 1) / mtw;
  if (EPI != EPI_PARTIAL || g.ksplit < 1) g.ksplit = 1;
  dim3 grid((g.N / (nt * 16)) * g.mblk * g.ksplit);
  FH_REQUIRE(grid.x < kFmtDivMax, "GEMM grid of %u workgroups is beyond the block decode's range", grid.x);
  fmt_gemm_head(g, nt * 16, EPI == EPI_PARTIAL);
  fmt_gemm_launch(0, kern, grid, dim3(nw * 64), smem, s, g);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// ---- stacked clips (>= kRbMinRows rows): the row-blocked LDS-DMA tile (fmt_rb_kernels.hpp) for qkv / proj / fc1 / fc2
template <class T, int EPI>
int launch_rbs(GemmArgs g, int shape, hipStream_t s) {
  if constexpr (T::is32) {
    fh_set_error("the fp32 verification mode has no row-blocked tiling");
    return FLOAT_E_INVALID;
  } else {
    GemmKernel kern = nullptr;
    int rows = 0, bn = 0, kps = 0, smem = 0;
    const int want = (shape == 0 || shape == 1) ? shape : 2;
    for_each_rbs<T, EPI>([&](GemmKernel k, int sh, int r, int c, int kp, int bytes) {
      if (sh == want) kern = k, rows = r, bn = c, kps = kp, smem = bytes;
    });
    if (EPI != EPI_PARTIAL || g.ksplit < 1) g.ksplit = 1;
    FH_REQUIRE(g.N % bn == 0 && (g.K / 32) % (g.ksplit * kps) == 0 && g.K / 32 / g.ksplit / kps >= 1,
               "row-blocked GEMM: N=%d K=%d not tileable by %d columns / %d K slices of %d-k-block stages", g.N, g.K, bn, g.ksplit, kps);
    g.mblk = (g.M + rows - 1) / rows;
    g.touch.W = nullptr;
    const dim3 grid((unsigned)((g.N / bn) * g.mblk * g.ksplit));
    fh_launch_prof(3, kern, grid, dim3(512), smem, s, g);
    FH_CHECK_HIP(hipGetLastError());
    return FLOAT_OK;
  }
}
// Which tile, per layer and row count (tools/probes/gemm_lab.hip on MI355X, us per launch incl. the launch boundary, weights
// rotating over 8 buffers; 48 x 64 tiling -> best row-blocked tile):
//   rows    qkv (3072 x 1024)     proj (1024 x 1024)      fc1 (4096 x 1024)      fc2 (1024 x 4096, 4 K slices)
//    360     9.7 ->  6.7 (96x64)   5.1 (kept)             10.9 ->  8.0 (96x64)   10.9 ->  8.3 (96x64)
//    720    14.4 ->  9.9 (96x128)  6.6 ->  6.4 (96x64 /2) 18.8 -> 13.2 (96x128)  19.0 -> 12.8 (96x128)
//   1440    24.4 -> 16.4 (96x64)  11.6 ->  9.8 (96x64 /2) 33.1 -> 22.5 (192x128) 34.1 -> 20.9 (192x128)
//   2880    53.7 -> 31.7 (192x128) 22.2 -> 15.7 (192x128 /2) 74.5 -> 43.3 (192x128) 71.8 -> 39.1 (192x128)
// FLOAT_FMT_RB=0 keeps the 48 x 64 tiling (the A/B switch); FLOAT_FMT_RB_QKV / _PROJ / _FC1 / _FC2 = "shape[,ksplit]" override.
constexpr int kRbMinRows = 300;
struct RbPlan {
  int shape = -1, ksplit = 1;  // shape < 0: the weight-streaming tiling
};
RbPlan pick_rb(const FmtTune& tn, int layer, int M) {
  RbPlan p;
  if (!tn.rb || M < kRbMinRows) return p;
  const int tier = M < 540 ? 0 : (M < 1100 ? 1 : (M < 2200 ? 2 : 3));
  static const int shapes[4][4] = {/* qkv */ {0, 1, 0, 2}, /* proj */ {-1, 0, 0, 2}, /* fc1 */ {0, 1, 2, 2}, /* fc2 */ {0, 1, 2, 2}};
  p.shape = shapes[layer][tier];
  // fc2: 4 K slices fill the CUs up to 1440 rows; from 2200 rows on 2 slices do (15 x 8 tiles x 2) and halve the fp32 slabs the
  // next LayerNorm folds (16 clips: 415.7 vs 438.6 ms per 250 evaluations; 8 clips the other way round: 251.6 vs 241.9)
  p.ksplit = layer == RB_PROJ ? 2 : (layer == RB_FC2 ? (tier == 3 ? 2 : 4) : 1);
  const FmtTune::Rb& o = tn.rb_layer[layer];
  if (o.n >= 1) {
    p.shape = o.shape;
    const int ks = o.ksplit;
    if (o.n >= 2 && (layer == RB_PROJ || layer == RB_FC2) && (ks == 1 || ks == 2 || ks == 4 || ks == 8)) p.ksplit = ks;
  }
  return p;
}

// Tiling choice: split the rows over row blocks so that narrow layers still fill the 256 CUs, and
// split K over as many waves as keeps >= 4 k-steps per wave (one prefetch round per wave).
struct Tiling {
  int mtw, nt, nw;
};
int pick_nw(int K, int forced) {
  const int KB = K / 32;
  if (forced && KB % forced == 0) return forced;
  if (KB >= 128 && KB % 16 == 0) return 16;
  if (KB >= 32 && KB % 8 == 0) return 8;
  return 4;
}
Tiling pick_tiling(const FmtTune& tn, int M, int N, int K, bool need_full_rows) {
  const int mt = (M + 15) / 16;
  if (need_full_rows) {
    if (mt <= 4) return {4, 1, pick_nw(K, 0)};
    // 16 columns per workgroup: twice the workgroups of the 32-column tile; 8 K-splitting waves keep twice
    // the operand bytes in flight (each of the 32 workgroups streams the whole 393 KB activation operand)
    return {mt <= 12 ? 12 : 15, 1, (tn.full_nw == 8 && (K / 32) % 8 == 0) ? 8 : 4};
  }
  int split = mt <= 4 ? 4 : (mt <= 12 ? 3 : 5);
  if (mt <= 2) split = mt;
  const int blocks = (mt + split - 1) / split;
  const bool wide = N >= 16384;  // the fused adaLN projection
  if (mt >= 12) {  // tuning overrides only apply to the CFG-batched shapes (buffers hold 240 rows)
    const int* o = tn.plan + (wide ? 3 : 0);
    if (o[0]) {
      int nw = o[0] >= 12 ? 4 : pick_nw(K, o[2]);
      while (nw > 4 && nw * o[0] * 16 * o[1] * 16 * 4 > kLdsMax) nw >>= 1;
      return {o[0], o[1], nw};
    }
  }
  if (wide) return {mt <= 4 ? 4 : 6, 2, std::min(8, pick_nw(K, 0))};
  // stacked clips (float_fmt_sample_batch, more than 15 row tiles): the one-clip tile (48 x 64) with 4 K-splitting waves, so that
  // two or three workgroups share a CU (49 KB of LDS each instead of 98).  Measured per 250 evaluations, B = 2 / 4 clips:
  // 120.7 / 184.5 ms against 136.4 / 200.6 with the 80-row tiles this function would pick below, 130.1 / 208.1 with 8 waves
  // (one clip: 85.0).  Operands come straight from L2 per workgroup, so the traffic grows with rows x column blocks: the
  // batched chain wants an LDS-staged large-tile kernel like fmt_gemm_wide_kernel with these epilogues.
  if (mt > 15 && N % 64 == 0) return {3, 4, 4};
  // column tiles per workgroup: the widest (<= 4) that still gives >= ~200 workgroups, so that each CU
  // runs ONE workgroup (two back-to-back workgroups per CU double the latency chain of the layer)
  int nt = 1;
  if (mt >= 5) {
    if ((N / 64) * blocks >= 192 && N % 64 == 0) nt = 4;
    else if ((N / 32) * blocks >= 192 && N % 32 == 0) nt = 2;
  } else if ((N / 16) * blocks > 512) {
    nt = 2;
  }
  return {split, nt, pick_nw(K, 0)};
}
// fp32 verification mode: 16 columns per workgroup, 4 K-splitting waves, the row split of the 16-bit tilings capped at 5 tiles
Tiling pick_tiling32(int M) {
  const int mt = (M + 15) / 16;
  return {mt <= 5 ? mt : (mt <= 12 ? 3 : 5), 1, 4};
}

GemmArgs base_args(const u16* A, const Lin& L, int M) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A, g.W = L.W, g.bias = L.b;
  g.K = L.K, g.N = L.N, g.M = M;
  return g;
}

// plan: a per-layer tiling override of the one-clip chain (FmtTune::plan_layer, tuning aid)
template <class T, int EPI>
int run_gemm(const FmtTune& tn, GemmArgs g, hipStream_t s, bool need_full_rows = false, const LayerPlan* plan = nullptr) {
  if constexpr (T::is32) {
    FH_REQUIRE(!need_full_rows, "the fp32 mode has no all-rows CFG epilogue tiling (token-blocked head only)");
    const Tiling t = pick_tiling32(g.M);
    g.touch.W = nullptr;
    return launch_gemm<T, EPI>(g, t.mtw, t.nt, t.nw, s);
  }
  if (plan && plan->on() && (g.M + 15) / 16 <= 15) {
    g.touch.W = nullptr;  // the touch descriptors follow the default block decode
    return launch_gemm<T, EPI>(g, plan->v[0], plan->v[1], plan->v[2], s);
  }
  const Tiling t = pick_tiling(tn, g.M, g.N, g.K, need_full_rows);
  return launch_gemm<T, EPI>(g, t.mtw, t.nt, t.nw, s);
}

// Split-K GEMM whose gated residual add happens in the next LayerNorm launch (EPI_PARTIAL + LnRed): `ks` K slices, slice z
// written to slab[z] ([Mpad][N] fp32), and the fold handed to that LayerNorm.
struct PendingRed {
  int ks = 0;
  LnRed red{};
};
void to_slab(GemmArgs& g, float* slab, int Mpad, int ks) {
  g.ksplit = ks, g.out_f32 = slab, g.ldo = g.N, g.slab_stride = (size_t)Mpad * g.N;
}
PendingRed pending_red(float* slab, int Mpad, int D, const float* bias, const float* gate, int ks) {
  return PendingRed{ks, LnRed{slab, (size_t)Mpad * D, bias, gate}};
}
// The tiling is the one a GEMM with ksplit * N columns and K / ksplit would get: same workgroup
// count, a fraction of the activation bytes per workgroup (FmtTune::fc2_split, proj_split).
template <class T>
int run_gemm_partial(const FmtLaunch& cx, GemmArgs g, int ksplit, const LayerPlan* plan = nullptr) {
  to_slab(g, cx.slab, cx.Mpad, ksplit);
  if (plan && plan->on() && !T::is32 && (g.M + 15) / 16 <= 15) {
    g.touch.W = nullptr;
    return launch_gemm<T, EPI_PARTIAL>(g, plan->v[0], plan->v[1], plan->v[2], cx.s);
  }
  Tiling t = T::is32 ? pick_tiling32(g.M) : pick_tiling(cx.tn, g.M, g.N * ksplit, g.K / ksplit, false);
  while (t.nt > 1 && g.N % (t.nt * 16)) t.nt >>= 1;
  if (T::is32) g.touch.W = nullptr;
  return launch_gemm<T, EPI_PARTIAL>(g, t.mtw, t.nt, t.nw, cx.s);
}

int log2_exact(unsigned v) {  // log2 of a power of two, else -1
  int n = 0;
  while ((1u << n) < v) ++n;
  return (1u << n) == v ? n : -1;
}

// Touch descriptor for the weights of GEMM `L` as it will be launched for M rows (ksplit = 0: plain GEMM, else EPI_PARTIAL
// with that many K slices), to be executed by `lanes` threads per XCD with at most `per_lane` lines each; W = nullptr when the
// GEMM's block decode is not the XCD-affine one or the lanes cannot cover it.  Who pulls whose weights: FmtTune::touch.
TouchSpec make_touch(const FmtTune& tn, const Lin& L, int M, int ksplit, unsigned lanes, unsigned per_lane, int force_nt = 0) {
  TouchSpec t{};
  Tiling tl = ksplit ? pick_tiling(tn, M, L.N * ksplit, L.K / ksplit, false) : pick_tiling(tn, M, L.N, L.K, false);
  if (force_nt) tl.nt = force_nt;
  if (ksplit)
    while (tl.nt > 1 && L.N % (tl.nt * 16)) tl.nt >>= 1;
  const int ks = ksplit ? ksplit : 1;
  if (L.N % (tl.nt * 16) || L.K % (32 * ks) || 8 % ks) return t;
  const int nbn = L.N / (tl.nt * 16);
  if ((nbn * ks) % 8) return t;
  const unsigned P = 8 / ks, run_lines = (unsigned)(L.K / 32 / ks) * 8u;
  if (log2_exact(run_lines) < 0 || log2_exact((unsigned)tl.nt) < 0) return t;
  t.run_shift = (unsigned)log2_exact(run_lines);
  t.nt_shift = (unsigned)log2_exact((unsigned)tl.nt);
  t.p_shift = (unsigned)log2_exact(P);
  t.tile_bytes = (unsigned)(L.K / 32) * 1024u;
  t.total = ((unsigned)nbn / P) * (unsigned)tl.nt * run_lines;
  if ((size_t)t.total > (size_t)lanes * per_lane) return t;
  t.W = reinterpret_cast<const char*>(L.W);
  return t;
}

// The same for a row-blocked GEMM (fmt_gemm_rbs_kernel, no K split): only the FIRST stages of every weight column tile - what
// each of its workgroups waits for before it can start (1.5 of fc1's 10 us at 720 rows: every CU asks for cold lines at once).
// Its block decode puts column block bx on XCD bx % 8, like the 48 x 64 tiling's.  kb = k-blocks to pull (FmtTune::rb_touch, 0 = off).
TouchSpec make_touch_rb(const Lin& L, int shape, int kb, unsigned lanes, unsigned per_lane) {
  TouchSpec t{};
  const int ct = shape == 0 ? 4 : 8;  // 16-column tiles per column block: 96 x 64 | 96 x 128, 192 x 128
  if (kb <= 0 || (kb & (kb - 1)) || L.N % (ct * 16) || (L.N / (ct * 16)) % 8 || L.K / 32 < kb) return t;
  const unsigned run_lines = (unsigned)kb * 8u;  // a k-block of a column tile is 1 KiB = 8 lines, consecutive k-blocks are consecutive
  t.run_shift = (unsigned)log2_exact(run_lines);  // kb and ct are powers of two
  t.nt_shift = (unsigned)log2_exact((unsigned)ct);
  t.p_shift = 3;
  t.tile_bytes = (unsigned)(L.K / 32) * 1024u;
  t.total = (unsigned)(L.N / (ct * 16) / 8) * (unsigned)ct * run_lines;
  if ((size_t)t.total > (size_t)lanes * per_lane) return t;
  t.W = reinterpret_cast<const char*>(L.W);
  return t;
}

// threads per XCD of the launch run_gemm makes for a plain (M, N, K) GEMM
unsigned gemm_lanes_per_xcd(const FmtTune& tn, int M, int N, int K) {
  const Tiling t = pick_tiling(tn, M, N, K, false);
  const int mblk = ((M + 15) / 16 + t.mtw - 1) / t.mtw;
  return (unsigned)((N / (t.nt * 16)) * mblk / 8) * (unsigned)(t.nw * 64);
}

// ---- LayerNorm, attention ----

// LayerNorm + modulation of the M rows of xres -> `out` (default h16), after folding the split-K slabs `pend` describes (which
// it clears); `next`: the GEMM whose weights the workgroups touch meanwhile under touch bits 1 | touch_bit (rb_shape >= 0: as a
// row-blocked launch of that tile shape).
template <class T>
int launch_lnmod(const FmtLaunch& cx, int M, const float* shift, const float* scale, PendingRed* pend = nullptr,
                 const Lin* next = nullptr, u16* out = nullptr, int perm = 0, int touch_bit = 1, int rb_shape = -1) {
  // one row (wave) per workgroup: 180 single-wave workgroups spread over 180 CUs (4 rows per workgroup: +0.4 %)
  const int rpw = cx.tn.ln_rows;
  // rpw == 1: the kernel maps ids to rows in groups of 8 rows per XCD -> 64 row slots per group of 64 ids
  dim3 grid(rpw == 1 ? ((M + 63) / 64) * 64 : (M + rpw - 1) / rpw), block(64 * rpw);
  const int ks = pend ? pend->ks : 0;
  const bool wt = M <= kWtRows;  // write-through outputs for one clip's rows only (common.hpp, FMT_WT)
  LnRed red{};
  if (ks) red = pend->red;
  TouchSpec pf{};
  if (next && (cx.tn.touch & (1 | touch_bit)) && rpw == 1 && !T::is32)
    pf = rb_shape >= 0 ? make_touch_rb(*next, rb_shape, cx.tn.rb_touch, (grid.x / 8) * 64, 6)
                       : make_touch(cx.tn, *next, M, 0, (grid.x / 8) * 64, 6);
  decltype(&fmt_lnmod_kernel<T, 1, 0, false, false>) kern = nullptr;
  with_const<1, 2, 4, 8>(cx.D / 256, [&](auto NV) {
    with_const<0, 1, 2, 4, 8>((ks == 0 || ks == 1 || ks == 2 || ks == 4) ? ks : 8, [&](auto KS) {
      with_const<0, 1>(pf.W != nullptr, [&](auto TOUCH) {
        with_const<0, 1>(wt, [&](auto WT) {
          kern = fmt_lnmod_kernel<T, decltype(NV)::value, decltype(KS)::value, decltype(TOUCH)::value != 0, decltype(WT)::value != 0>;
        });
      });
    });
  });
  FH_REQUIRE(kern, "dim_h %d unsupported (must be 256*{1,2,4,8})", cx.D);
  FH_REQUIRE(red.slab_stride <= 0xffffffffull, "split-K slab of %zu elements is beyond the LayerNorm kernel's 32-bit stride", red.slab_stride);
  hipLaunchKernelGGL(kern, grid, block, 0, cx.s, cx.xres, shift, scale, red.slab, red.gate, M, cx.Ntot, rpw, (unsigned)red.slab_stride,
                     out ? out : cx.h16, red.bias, pf, cx.ntok, perm, cx.sat);
  if (pend) pend->ks = 0;
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// Banded attention over the M rows of qkv16 -> att16 (packed operand of attn.proj); `pull`: the GEMM whose weights the
// workgroups touch meanwhile (TouchSpec), or nullptr.
template <class T>
void launch_attn(const FmtLaunch& cx, int M, const Lin* pull) {
  // queries per workgroup / lanes per query (FLOAT_FMT_ATTN): one 8-row output group per workgroup, 8 dims per lane by default
  const int qpw = cx.tn.attn_qpw, lpq = cx.tn.attn_lpq;
  dim3 grid(cx.heads, (M + qpw - 1) / qpw), block(qpw * lpq);
  TouchSpec pf{};
  if (pull && !T::is32) pf = make_touch(cx.tn, *pull, M, 0, (grid.x * grid.y / 8) * block.x, 2);
  decltype(&fmt_attn_kernel<T, 8, false, false>) kern = nullptr;
  with_const<16, 8>(lpq == 16 ? 16 : 8, [&](auto LPQ) {
    with_const<0, 1>(pf.W != nullptr, [&](auto TOUCH) {
      with_const<0, 1>(M <= kWtRows, [&](auto WT) {
        kern = fmt_attn_kernel<T, decltype(LPQ)::value, decltype(TOUCH)::value != 0, decltype(WT)::value != 0>;
      });
    });
  });
  const FmtDiv nd = fmt_make_div((unsigned)cx.ntok);
  hipLaunchKernelGGL(kern, grid, block, 0, cx.s, cx.qkv16, cx.att16, 3 * cx.D, cx.ntok, M, cx.D, cx.attn_window, (int)block.x, nd.mul, nd.sh,
                     (int)grid.x, (int)grid.y, cx.sat, pf);
}

}  // namespace
