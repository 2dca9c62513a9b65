// HIP kernels of the Flow-Matching-Transformer evaluation (reference FMT.py:277-401).
//
// Shapes: M = Bc * n_tok rows (Bc = 1/3/4 CFG rows x 60 tokens), so every linear layer is a
// weight-streaming GEMM with a short M.  Both operands live in HBM in MFMA-FRAGMENT-MAJOR order:
//   packed[tile16][kb][lane(64)][8]   tile16 = row/16 (A) or n/16 (W), kb = k/32,
//                                     lane = (row%16) + 16*((k/8)%4), 8 consecutive k per lane
// so the 16-byte-per-lane operand of v_mfma_f32_16x16x32 for one (tile, kb) is ONE contiguous 1 KiB
// wave load (8 full 128-B lines) and consecutive k-steps are consecutive KiBs - no LDS staging, no
// strided rows hitting one L2 channel.  A workgroup owns MTW row tiles x NT column tiles; its 4 waves
// split K, partial sums meet in LDS, and the epilogue (bias / SiLU / GELU / gate*residual / CFG+Euler)
// is applied once per output element in a fixed order -> bitwise reproducible, no atomics.  Weights
// are read from HBM once (non-temporal); workgroups that share a weight column block differ only in
// blockIdx.y, i.e. by a multiple of gridDim.x (a multiple of 8), so they sit on one XCD's L2.
#pragma once
#include "common.hpp"
#include "fmt_pack.hpp"

// k-steps of operands in flight per wave.  With 4 k-blocks per wave (K = 1024 over 8 waves) PF = 4 puts the whole
// K slice in flight at once: one memory round trip instead of two for the 48x64 tilings (7 fragments per k-step,
// 112 operand registers + 48 accumulators still fit two waves per SIMD)
template <class T, int MTW, int NT>
constexpr int fmt_gemm_pf() {
  return T::is32 ? 1 : ((MTW + NT <= 7) ? 4 : ((MTW + NT <= 8) ? 3 : 2));
}
// The instantiations that carry the straight-line form of the body (FLAT below) beside the general one: the tilings of the
// one-clip step chain - qkv / fc1 / fc2 (48 x 64, 8 waves), proj and the head (48 x 16, 8 waves), x-embed (64 x 16, 4 waves).
// Every other tiling keeps the general form alone: the straight-line form's registers would cost the small ones a wave per SIMD.
template <class T, int MTW, int NT, int NW, int EPI>
constexpr bool fmt_gemm_has_flat() {
  if (T::is32) return false;
  if (EPI == EPI_XEMBED) return MTW == 4 && NT == 1 && NW == 4;
  return NW == 8 && MTW == 3 && (NT == 4 || EPI == EPI_GATE_RES || EPI == EPI_CFG);
}

// The kernel's body as a device function (fmt_gemm_kernel picks its FLAT or its general form).
// FLAT: the wave's K slice is exactly the PF k-steps in flight (every GEMM of the one-clip chain: K = 1024 over 8 waves, fc2 with
// its K slices).  The body is then straight-line code from the first operand load to the last MFMA - every load of the prologue
// is issued by every lane, none is issued in the K loop - and the compiler's s_waitcnt vmcnt in front of k-step p counts exactly
// the loads behind that step's operands: the later steps, the epilogue operands and the touched lines stay in flight under the
// MFMAs.  With the run-time trip counts of the general form it must assume the youngest load is the one it waits for, which
// makes every wave wait for its whole K slice AND the touched HBM lines in front of its first MFMA.  The straight-line form
// retires the touch behind its last store; everything else - the exchange through LDS, the epilogues - is the general form's.
template <class T, int MTW, int NT, int NW, int EPI, bool FLAT = false>
__device__ __forceinline__ void fmt_gemm_body(const GemmArgs& g) {
  const unsigned bid = blockIdx.x, nblk = gridDim.x;
  constexpr int BN = NT * 16;
  constexpr int ROWS = MTW * 16;
  constexpr bool WT = NW >= 8;  // the single-clip tilings (stacked clips split K over 4 waves): see common.hpp, FMT_WT
  constexpr int NTHR = NW * 64;
  constexpr int PF = fmt_gemm_pf<T, MTW, NT>();
  typedef typename T::elem E;
  typedef typename T::pack8 P8;
  extern __shared__ __attribute__((aligned(16))) float red[];  // [NW][ROWS][BN]
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  // 1-D grid of (column blocks) x (row blocks) x (K slices): fmt_decode.hpp.  Everything up to the first operand load reads the
  // head of the argument block only (GemmHead, preloaded into SGPRs for fmt_gemm_kernel); the tail is first read behind them.
  const GemmBlock blk = fmt_block_decode(g.dec, (unsigned)g.mblk, bid, EPI == EPI_PARTIAL);
  const int bx = blk.bx, by = blk.by, ks = blk.ks;
  const int nb0 = bx * NT;
  const int mt0 = by * MTW;
  const int n0 = nb0 * 16, m0 = mt0 * 16;

  f32x4 acc[MTW][NT];
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KB = g.K >> 5;
  const int KBs = (EPI == EPI_PARTIAL) ? g.kbs : KB;  // k-blocks of this workgroup's K slice
  const int KBw = FLAT ? PF : (int)((unsigned)KBs / NW);  // k-blocks per wave
  const E* Ap = reinterpret_cast<const E*>(g.A) + ((size_t)mt0 * KB + ks * KBs + w * KBw) * 512 + lane * 8;
  const E* Wp = reinterpret_cast<const E*>(g.W) + ((size_t)nb0 * KB + ks * KBs + w * KBw) * 512 + lane * 8;
  const size_t tstride = (size_t)KB * 512;

  P8 a[PF][MTW], b[PF][NT];
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    if (FLAT || p < KBw) {
#pragma unroll
      for (int j = 0; j < NT; ++j) b[p][j] = T::load8_nt(Wp + j * tstride + (size_t)p * 512);
#pragma unroll
      for (int i = 0; i < MTW; ++i) a[p][i] = T::load8(Ap + i * tstride + (size_t)p * 512);
    }
  }
  // EPI_GATE_RES with one epilogue item per thread: fetch residual and gate now, not after the K loop (behind the operand
  // loads: their addresses are the first thing that needs the tail of the argument block)
  constexpr bool kEarlyRes = (EPI == EPI_GATE_RES) && (MTW * 16 * (NT * 2) <= NW * 64);
  float4 res_pf[2], gate_pf[2];
  if constexpr (kEarlyRes) {
    const int r = threadIdx.x / (NT * 2), cg = threadIdx.x % (NT * 2);
    int row = m0 + r;
    const int nb = n0 + cg * 8;
    if constexpr (FLAT) row = min(m0 + min(r, ROWS - 1), g.M - 1);  // a thread without an item fetches a row that exists: no branch
    if (FLAT || (r < ROWS && row < g.M)) {
      const float* o = g.out_f32 + (size_t)row * g.ldo + nb;
      const float* gt = g.gate + (size_t)row * g.ldg + nb;
      res_pf[0] = fh_load_f4(o);
      res_pf[1] = fh_load_f4(o + 4);
      gate_pf[0] = fh_load_f4_stream(gt);
      gate_pf[1] = fh_load_f4_stream(gt + 4);
    }
  }
  // only the epilogue kinds whose launches are given a TouchSpec carry the code (2 registers, a branch)
  constexpr bool kTouch = (EPI == EPI_GELU_P16 || EPI == EPI_T16 || EPI == EPI_GATE_RES || EPI == EPI_PARTIAL);
  unsigned touched[2] = {0u, 0u};
  if constexpr (kTouch && FLAT) {
    __builtin_amdgcn_sched_barrier(0);  // behind the operand loads
    fmt_touch_always(g.touch, Wp, bid & 7, (bid >> 3) * NTHR + threadIdx.x, (nblk >> 3) * NTHR, touched);
  } else if constexpr (kTouch) {
    if (g.touch.W) fmt_touch(g.touch, bid & 7, (bid >> 3) * NTHR + threadIdx.x, (nblk >> 3) * NTHR, touched);
  }
  if constexpr (FLAT) {
    // (the scheduler may not move a load down into the MFMAs to save registers, nor a k-step up across a wait)
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < MTW; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = T::mfma(a[p][i], b[p][j], acc[i][j]);
    }
    __builtin_amdgcn_sched_barrier(0);
  } else
  for (int kb0 = 0; kb0 < KBw; kb0 += PF) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int kb = kb0 + p;
      if (kb < KBw) {
#pragma unroll
        for (int i = 0; i < MTW; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[i][j] = T::mfma(a[p][i], b[p][j], acc[i][j]);
        if (kb + PF < KBw) {
#pragma unroll
          for (int j = 0; j < NT; ++j)
            b[p][j] = T::load8_nt(Wp + j * tstride + (size_t)(kb + PF) * 512);
#pragma unroll
          for (int i = 0; i < MTW; ++i) a[p][i] = T::load8(Ap + i * tstride + (size_t)(kb + PF) * 512);
        }
      }
    }
  }

  // (the general form has waited for the touched lines in its K loop already; holding their registers to the end would cost
  // the 16-wave tilings spills and the smallest ones a wave)
  if constexpr (kTouch && !FLAT) {
    if (g.touch.W) fmt_touch_retire(touched);
  }
  // C/D map of mfma_f32_16x16x32: col = lane & 15, row = (lane >> 4) * 4 + reg
  float* my = red + w * (ROWS * BN);
#pragma unroll
  for (int i = 0; i < MTW; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) my[(i * 16 + q * 4 + r) * BN + j * 16 + r16] = acc[i][j][r];
  __syncthreads();

  constexpr int S = ROWS * BN;
  constexpr int CG = BN / 8;  // 8-column groups per row
  unsigned rm = 0u;           // range tracker of this thread's 16-bit stores (fh_range_flush)
  auto slab_sum = [&](int o) {
    float a = red[o];
#pragma unroll
    for (int ww = 1; ww < NW; ++ww) a += red[ww * S + o];
    return a;
  };
  if constexpr (EPI == EPI_CFG) {
    // rows of the tile: b * ntok + i (one clip, all rows in the workgroup), or b * 16 + i % 16 of (token block, clip) pair `by`
    // (g.tokblk: by = token block * nclip + clip).  Combine the CFG rows of token i, then (optionally) Euler.
    const int nclip = g.nclip > 1 ? g.nclip : 1;
    const int tb = g.tokblk ? by / nclip : 0, q = g.tokblk ? by - tb * nclip : 0;
    const int ni = g.tokblk ? 16 : g.ntok, i0 = tb * 16, rstride = g.tokblk ? 16 : g.ntok;
    float* const vout_q = g.vout ? g.vout + (size_t)q * g.ntok * g.N : nullptr;
    float* const xcur_q = g.xcur ? g.xcur + (size_t)q * (g.ntok - g.n_prev) * g.N : nullptr;
    for (int idx = threadIdx.x; idx < ni * BN; idx += NTHR) {
      const int il = idx / BN, i = i0 + il, c = idx % BN, n = n0 + c;
      if (i >= g.ntok) break;
      const float bias = g.bias[n];
      float v[4];
#pragma unroll
      for (int b2 = 0; b2 < 4; ++b2) {
        if (b2 < g.bc) {
          const int o = (b2 * rstride + il) * BN + c;
          v[b2] = slab_sum(o) + bias;
        } else {
          v[b2] = 0.f;
        }
      }
      float out;
      if (g.bc == 1) {
        out = v[0];
      } else if (g.bc == 3) {  // [uncond | all | audio-only]
        out = v[0] + g.a_cfg * (v[2] - v[0]) + g.e_cfg * (v[1] - v[2]);
      } else {  // [null-ref | uncond | all | audio-only]
        out = v[0] + g.r_cfg * (v[1] - v[0]) + g.a_cfg * (v[3] - v[1]) + g.e_cfg * (v[2] - v[3]);
      }
      if (vout_q) vout_q[(size_t)i * g.N + n] = out;
      if (xcur_q && i >= g.n_prev) {
        const size_t xo = (size_t)(i - g.n_prev) * g.N + n;
        const float xn = xcur_q[xo] + g.dt * out;  // x_{k+1} = x_k + dt * v  (fixed-grid Euler)
        xcur_q[xo] = xn;
        reinterpret_cast<E*>(g.xin16)[fmt_pack_off(q * g.ntok + i, n, g.ldx)] = fh_cvt<T>(xn, rm);
      }
    }
  } else {
    for (int idx = threadIdx.x; idx < ROWS * CG; idx += NTHR) {
      const int r = idx / CG, cg = idx % CG;
      const int row = m0 + r, nb = n0 + cg * 8;
      if (row >= g.M) continue;
      float v[8];
      {
        const float* p0 = red + r * BN + cg * 8;
#pragma unroll
        for (int e = 0; e < 8; e += 4) {
          float4 a4 = *reinterpret_cast<const float4*>(p0 + e);
#pragma unroll
          for (int ww = 1; ww < NW; ++ww) {
            const float4 t4 = *reinterpret_cast<const float4*>(p0 + ww * S + e);
            a4.x += t4.x;
            a4.y += t4.y;
            a4.z += t4.z;
            a4.w += t4.w;
          }
          float4 bb = float4{0.f, 0.f, 0.f, 0.f};
          if constexpr (EPI != EPI_PARTIAL) bb = *reinterpret_cast<const float4*>(g.bias + nb + e);
          v[e + 0] = a4.x + bb.x;
          v[e + 1] = a4.y + bb.y;
          v[e + 2] = a4.z + bb.z;
          v[e + 3] = a4.w + bb.w;
        }
      }
      if constexpr (EPI == EPI_F32 || EPI == EPI_PARTIAL) {
        float* o = g.out_f32 + (size_t)ks * g.slab_stride + (size_t)row * g.ldo + nb;
        fh_store_f4_wt<4, WT>(o, float4{v[0], v[1], v[2], v[3]});
        fh_store_f4_wt<4, WT>(o + 4, float4{v[4], v[5], v[6], v[7]});
      } else if constexpr (EPI == EPI_T16 || EPI == EPI_SILU_P16 || EPI == EPI_GELU_P16 || EPI == EPI_GELUERF_P16) {
        P8 u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float x = v[i];
          if constexpr (EPI == EPI_SILU_P16) x = fh_silu(x);
          if constexpr (EPI == EPI_GELU_P16) x = fh_gelu_tanh(x);
          if constexpr (EPI == EPI_GELUERF_P16) x = fh_gelu_erf(x);
          T::set(u, i, x);
        }
        fh_track_pack<T>(rm, u);
        E* const o16 = reinterpret_cast<E*>(g.out16);
        if constexpr (EPI == EPI_T16) T::template store8_wt<8, WT>(o16 + (size_t)row * g.ldo16 + nb, u);
        else T::template store8_wt<8, WT>(o16 + fmt_pack_off(row, nb, g.ldo16), u);
      } else if constexpr (EPI == EPI_GATE_RES) {
        float* o = g.out_f32 + (size_t)row * g.ldo + nb;
        const float* gt = g.gate + (size_t)row * g.ldg + nb;
#pragma unroll
        for (int e = 0; e < 8; e += 4) {
          float4 x, gg;
          if constexpr (kEarlyRes) {
            x = res_pf[e / 4];
            gg = gate_pf[e / 4];
          } else {
            x = fh_load_f4(o + e);
            gg = fh_load_f4_stream(gt + e);
          }
          x.x += gg.x * v[e + 0];
          x.y += gg.y * v[e + 1];
          x.z += gg.z * v[e + 2];
          x.w += gg.w * v[e + 3];
          fh_store_f4_wt<16, WT>(o + e, x);
        }
      } else if constexpr (EPI == EPI_XEMBED) {
        // input row = clip * ntok + token (the CFG rows of a clip share x); output rows (clip * bc + b2) * ntok + token
        const int q = row / g.ntok, tok = row - q * g.ntok;
        const float* ps = g.pos + (size_t)tok * g.N + nb;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += ps[i];
        for (int b2 = 0; b2 < g.bc; ++b2) {
          float* o = g.out_f32 + (size_t)((q * g.bc + b2) * g.ntok + tok) * g.ldo + nb;
          fh_store_f4_wt<32, WT>(o, float4{v[0], v[1], v[2], v[3]});
          fh_store_f4_wt<32, WT>(o + 4, float4{v[4], v[5], v[6], v[7]});
        }
      }
    }
  }
  if constexpr (EPI == EPI_CFG || EPI == EPI_T16 || EPI == EPI_SILU_P16 || EPI == EPI_GELU_P16 || EPI == EPI_GELUERF_P16) fh_range_flush<T>(g.sat, rm);
  // straight-line form: behind the last store - the touched lines come from HBM and are the wave's youngest loads, and nothing
  // reads their registers
  if constexpr (kTouch && FLAT) fmt_touch_retire_last(touched);
}

template <class T, int MTW, int NT, int NW, int EPI>
__global__ __launch_bounds__(NW * 64) void fmt_gemm_kernel(const u16* A, const u16* W, int K, int kbs, int ksplit, int mblk,
                                                           unsigned mblk_mul, unsigned nbx, unsigned nbx_mul, unsigned nbn,
                                                           unsigned nbn_mul, unsigned bits, GemmTail t) {
  // GemmHead member by member: scalar parameters are preloaded, a by-value struct never is (and it ends the preloaded run)
  GemmArgs g;
  static_cast<GemmHead&>(g) = GemmHead{A, W, K, kbs, ksplit, mblk, GemmDecode{mblk_mul, nbx, nbx_mul, nbn, nbn_mul, bits}};
  static_cast<GemmTail&>(g) = t;
  // the straight-line form where the tiling carries it and the K slice is its PF k-steps per wave: a uniform branch on two
  // preloaded scalars
  if constexpr (fmt_gemm_has_flat<T, MTW, NT, NW, EPI>()) {
    if ((EPI == EPI_PARTIAL ? kbs : (K >> 5)) == NW * fmt_gemm_pf<T, MTW, NT>()) {
      fmt_gemm_body<T, MTW, NT, NW, EPI, true>(g);
      return;
    }
  }
  fmt_gemm_body<T, MTW, NT, NW, EPI>(g);
}
// the host's side of that parameter list: launches fmt_gemm_kernel<...> `kern` with the head's members and the tail of `g`
// (whose head fmt_gemm_head has completed); `prof` as fh_launch_prof
template <class K>
void fmt_gemm_launch(int prof, K kern, dim3 grid, dim3 block, size_t smem, hipStream_t s, const GemmArgs& g) {
  const GemmTail& t = g;
  fh_launch_prof(prof, kern, grid, block, smem, s, g.A, g.W, g.K, g.kbs, g.ksplit, g.mblk, g.dec.mblk_mul, g.dec.nbx, g.dec.nbx_mul,
                 g.dec.nbn, g.dec.nbn_mul, g.dec.bits, t);
}

// Wide-N variant for the fused adaLN projection (N = depth*6D + 2D = 51 200, K = D): here re-reading
// the activations per 32-column slab dominates the L2->CU traffic (r01 PMC: 1.8 TB/s of HBM+write
// traffic, waves 85 % stalled), so A goes through LDS ONCE per workgroup and serves 128 columns:
//   * the fragment-major HBM image of A is exactly the LDS image a wave wants (1 KiB per fragment,
//     lane-linear: conflict-free ds_read_b128); chunks of 4 k-blocks are double-buffered through
//     registers so the loads of chunk c+1 fly while chunk c is multiplied;
//   * the 4 waves own 32 columns each for the whole K (no K split, no LDS reduction); weights stream
//     straight to registers, non-temporal;
//   * operands are swapped (D = W_tile * A_tile^T) so a lane holds 4 consecutive columns of one row and
//     the fp32 result is stored as float4.
// NWV = 8: two waves per SIMD - waves 0..3 own the upper half of the row tiles, waves 4..7 the lower half, both halves the
// same four 32-column slices (each weight fragment is then loaded by two waves, from L2; the LDS reads per MFMA do not change).
// (Round 2 also ran this body with the step chain's epilogues for stacked clips - 96 / 192-row tiles, EPI_T16 / EPI_GELU_P16 /
// EPI_PARTIAL - and it was slower than the 48 x 64 tiling at 360-720 rows: 167 / 194 ms per batch of 2 / 4 clips against
// 118 / 181; removed in round 3, DESIGN.md "Negative results".)
template <class T, int MTW, int KCH /* k-blocks (of 32) per LDS chunk */, int NWV = 4>
__global__ __launch_bounds__(NWV * 64) void fmt_gemm_wide_kernel(GemmArgs g) {
  constexpr int EPI = EPI_F32;
  constexpr int NF = MTW * KCH;            // 1-KiB A fragments per chunk
  constexpr int NFW = (NF + NWV - 1) / NWV;  // fragments staged by one wave
  constexpr int WR = NWV / 4, MTR = MTW / WR;  // row halves, row tiles per wave
  static_assert(MTW % WR == 0, "row tiles must split evenly over the wave rows");
  extern __shared__ __attribute__((aligned(16))) unsigned char sA[];  // [2][MTW][KCH][1 KiB]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wc = w & 3, wr = w >> 2;
  const int r16 = lane & 15, q = lane >> 4;
  const int nbn = g.N >> 7;
  const int nbx = (EPI == EPI_PARTIAL) ? nbn * g.ksplit : nbn;  // (column block, K slice) pairs
  int bx, by, bz = 0, ks = 0;
  {
    const int id = blockIdx.x;
    const int nz = g.zcount > 1 ? g.zcount : 1;
    if (nz > 1 && (nbx & 7) == 0 && g.zgroup > 1) {
      // Batched over the Euler steps of a window (the hoisted adaLN projection): ids congruent mod 8 share an XCD's L2.
      // An XCD walks groups of `zgroup` column blocks; inside a group the step runs slowest and the column blocks fastest, so
      // the ~32 workgroups in flight on the XCD are (32 / zgroup) steps x zgroup column blocks: the group's weight slabs
      // (262 KB each) stay in L2 for the whole group and every activation tile (393 KB) is fetched from the Infinity Cache
      // once per group instead of once per column block.  The last group of an XCD may be narrower.
      const int slot = id >> 3, G = g.zgroup, ncx = nbx >> 3, rows = g.mblk * nz;
      const int full = ncx / G, per_grp = G * rows;
      int grp = slot / per_grp, rem = slot - grp * per_grp, gw = G;
      if (grp >= full) {
        grp = full;
        rem = slot - full * per_grp;
        gw = ncx - full * G;
      }
      const int zy = rem / gw;
      bz = zy / g.mblk;
      by = zy - bz * g.mblk;
      bx = (grp * G + (rem - zy * gw)) * 8 + (id & 7);
    } else if ((nbx & 7) == 0) {
      const int slot = id >> 3, zy = slot % (g.mblk * nz);
      bz = zy / g.mblk;
      by = zy - bz * g.mblk;
      bx = (slot / (g.mblk * nz)) * 8 + (id & 7);
    } else {
      bx = id % nbx;
      const int zy = id / nbx;
      bz = zy / g.mblk;
      by = zy - bz * g.mblk;
    }
    if constexpr (EPI == EPI_PARTIAL) {
      if ((nbx & 7) == 0 && (8 % g.ksplit) == 0) {
        const int P = 8 / g.ksplit, x = bx & 7;
        ks = x / P;
        bx = (bx >> 3) * P + (x % P);
      } else {
        ks = bx / nbn;
        bx = bx % nbn;
      }
    }
  }
  const int mt0 = by * MTW;
  const int nb0 = bx * 8 + wc * 2;  // this wave's two 16-column tiles
  const int KB = g.K >> 5;
  const int KBs = (EPI == EPI_PARTIAL) ? KB / g.ksplit : KB;  // k-blocks of this workgroup's K slice
  const int nchunk = KBs / KCH;
  const size_t tstride = (size_t)KB * 512;
  const u16* Wp = g.W + (size_t)nb0 * tstride + (size_t)ks * KBs * 512 + lane * 8;
  const u16* Ag = g.A + (size_t)bz * g.a_zstride + (size_t)mt0 * tstride + (size_t)ks * KBs * 512 + lane * 8;
  float* const outz = g.out_f32 + (size_t)bz * g.o_zstride + (size_t)ks * g.slab_stride;

  f32x4 acc[MTR][2];
#pragma unroll
  for (int i = 0; i < MTR; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Register-staged software pipeline (all ordinary loads, so hipcc's counted vmcnt waits keep the next
  // chunk in flight): while chunk c is multiplied out of LDS buffer c&1 and the b registers, the A
  // fragments and the weights of chunk c+1 are already on their way.
  u32x4 an[NFW], bn[KCH][2], bc[KCH][2];
  auto issue = [&](int c) {
    const int kc = c * KCH;
#pragma unroll
    for (int f = 0; f < NFW; ++f) {
      const int fi = f * NWV + w;
      if (fi < NF) {
        const int i = fi / KCH, kk = fi % KCH;
        an[f] = *reinterpret_cast<const u32x4*>(Ag + i * tstride + (size_t)(kc + kk) * 512);
      }
    }
#pragma unroll
    for (int kk = 0; kk < KCH; ++kk) {
      bn[kk][0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(Wp + (size_t)(kc + kk) * 512));
      bn[kk][1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(Wp + tstride + (size_t)(kc + kk) * 512));
    }
  };
  auto commit = [&](int buf) {  // registers -> LDS buffer `buf`, weights -> current set
#pragma unroll
    for (int f = 0; f < NFW; ++f) {
      const int fi = f * NWV + w;
      if (fi < NF) *reinterpret_cast<u32x4*>(sA + (buf * NF + fi) * 1024 + lane * 16) = an[f];
    }
#pragma unroll
    for (int kk = 0; kk < KCH; ++kk) {
      bc[kk][0] = bn[kk][0];
      bc[kk][1] = bn[kk][1];
    }
  };
  issue(0);
  commit(0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunk) issue(c + 1);
#pragma unroll
    for (int kk = 0; kk < KCH; ++kk) {
#pragma unroll
      for (int i = 0; i < MTR; ++i) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(sA + (buf * NF + (wr * MTR + i) * KCH + kk) * 1024 + lane * 16);
        acc[i][0] = T::mfma(bc[kk][0], a, acc[i][0]);
        acc[i][1] = T::mfma(bc[kk][1], a, acc[i][1]);
      }
    }
    if (c + 1 < nchunk) {
      commit(buf ^ 1);  // the other buffer was last read in iteration c-1, and a barrier has passed since
      __syncthreads();
    }
  }
  // D[n = q*4 + reg][m = r16]: lane -> row m0 + i*16 + r16, columns n0 + j*16 + q*4 .. +3
#pragma unroll
  for (int i = 0; i < MTR; ++i) {
    const int row = (mt0 + wr * MTR + i) * 16 + r16;
    if (row >= g.M) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = (nb0 + j) * 16 + q * 4;
      float4 o = float4{acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if constexpr (EPI != EPI_PARTIAL) {
        const float4 bb = *reinterpret_cast<const float4*>(g.bias + n);
        o.x += bb.x;
        o.y += bb.y;
        o.z += bb.z;
        o.w += bb.w;
      }
      if constexpr (EPI == EPI_F32 || EPI == EPI_PARTIAL) {
        *reinterpret_cast<float4*>(outz + (size_t)row * g.ldo + n) = o;
      } else if constexpr (EPI == EPI_T16) {
        T::store4(g.out16 + (size_t)row * g.ldo16 + n, o.x, o.y, o.z, o.w);
      } else {
        static_assert(EPI == EPI_GELU_P16, "epilogue not built for the wide GEMM");
        T::store4(g.out16 + fmt_pack_off(row, n, g.ldo16), fh_gelu_tanh(o.x), fh_gelu_tanh(o.y), fh_gelu_tanh(o.z), fh_gelu_tanh(o.w));
      }
    }
  }
}

// The hoisted adaLN projection on a 192 x 320 tile, 8 waves, both operands by LDS-DMA (fmt_gemm_dma_kernel).
// fmt_gemm_wide_kernel above tops out near 680 TFLOP/s: four waves with 2 column tiles each read one LDS fragment per two
// MFMAs (LDS-read-bound), stage through registers, and need 2-3 co-resident workgroups to hide their own barriers.  Here:
//   * the tile is 12 row tiles x 20 column tiles (51 200 = 160 x 320), waves laid out 2 x 4, each 6 x 5 tiles: 11 fragment
//     reads per 30 MFMAs; 12 + 20 = 32 fragments of 1 KiB per k-block, i.e. exactly 4 LDS-DMA instructions per wave and stage
//     (the fragment-major HBM images are lane-linear, so the LDS image needs no swizzle and every ds_read_b128 is conflict-free);
//   * a ring of 4 stages (128 KiB), three k-blocks in flight behind a COUNTED vmcnt and ONE raw s_barrier per k-block; the
//     fragments of k-block s+1 are read into a second register set while the MFMAs of k-block s run (LDS reads by inline asm:
//     hipcc would otherwise drain the DMA queue before every ds_read).
// Hazards: stage s+4 overwrites the buffer of stage s, whose fragments every wave has in registers (lgkmcnt(0)) before it
// arrives at the barrier of step s; a stage is read one barrier after the wait that retires this wave's share of it.
template <int OFF>
__device__ __forceinline__ u32x4 fh_ds_read128(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int N>
__device__ __forceinline__ void fh_wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <class T, int NWC /* wave columns: 4 -> 8 waves, 320-column tile (2 -> 4 waves, 160 columns) */, int NS /* ring stages */,
          int STG /* 1: the two wave rows run half a step apart (see DMA_STEP_STG) */>
__global__ __launch_bounds__(NWC * 128) void fmt_gemm_dma_kernel(GemmArgs g) {
  constexpr int RT = 12, CT = 5 * NWC, NF = RT + CT, NW = 2 * NWC, STAGE = NF * 1024;
  constexpr int IMAX = (NF + NW - 1) / NW, ILO = NF / NW, NHI = NF % NW;  // DMA instructions per wave and stage: IMAX for waves < NHI
  static_assert(NS >= 3 && NS <= 4, "ring of 3 or 4 stages");
  extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];  // [NS][NF fragments][1 KiB]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w / NWC, wc = w % NWC;
  const int r16 = lane & 15, q = lane >> 4;
  const int nbx = g.N / (CT * 16);
  int bx, by, bz;
  {
    // same walk as fmt_gemm_wide_kernel: an XCD (ids congruent mod 8) takes groups of `zgroup` column blocks, the step slowest
    const int id = blockIdx.x, nz = g.zcount > 1 ? g.zcount : 1;
    if ((nbx & 7) == 0 && g.zgroup > 1) {
      const int slot = id >> 3, G = g.zgroup, ncx = nbx >> 3, rows = g.mblk * nz;
      const int full = ncx / G, per_grp = G * rows;
      int grp = slot / per_grp, rem = slot - grp * per_grp, gw = G;
      if (grp >= full) {
        grp = full;
        rem = slot - full * per_grp;
        gw = ncx - full * G;
      }
      const int zy = rem / gw;
      bz = zy / g.mblk;
      by = zy - bz * g.mblk;
      bx = (grp * G + (rem - zy * gw)) * 8 + (id & 7);
    } else {
      bx = id % nbx;
      const int zy = id / nbx;
      bz = zy / g.mblk;
      by = zy - bz * g.mblk;
    }
  }
  const int KB = g.K >> 5;
  const size_t tstride = (size_t)KB * 512;
  // this wave's fragments of a stage: fi = w + NW * i; fi < 12: row tile fi of A, else column tile fi - 12 of W
  const u16* src[IMAX];
#pragma unroll
  for (int i = 0; i < IMAX; ++i) {
    const int fi = min(w + NW * i, NF - 1);
    src[i] = (fi < RT ? g.A + (size_t)bz * g.a_zstride + (size_t)(by * RT + fi) * tstride
                      : g.W + (size_t)(bx * CT + fi - RT) * tstride) + lane * 8;
  }
  auto issue = [&](int s) {
    unsigned char* dst = ring + (s % NS) * STAGE + w * 1024;
#pragma unroll
    for (int i = 0; i < IMAX; ++i)
      if (i < ILO || w < NHI)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[i] + (size_t)s * 512),
                                         (__attribute__((address_space(3))) void*)(dst + i * NW * 1024), 16, 0, 0);
  };
  // wait until at most K of this wave's stages are still in flight (waves < NHI issue one more instruction per stage)
#define DMA_WAIT(K)                                   \
  do {                                                \
    if (NHI == 0 || w < NHI) fh_wait_vmcnt<(K)*IMAX>(); \
    else fh_wait_vmcnt<(K)*ILO>();                    \
  } while (0)
  const unsigned abase = (unsigned)(lane * 16 + wr * 6 * 1024), bbase = (unsigned)(lane * 16 + (RT + wc * 5) * 1024);

  f32x4 acc[6][5];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 a0[6], b0[5], a1[6], b1[5];

#define DMA_READ(S, AR, BR)                                        \
  do {                                                             \
    const unsigned so = (unsigned)(((S) % NS) * STAGE);            \
    AR[0] = fh_ds_read128<0>(abase + so);                          \
    AR[1] = fh_ds_read128<1024>(abase + so);                       \
    AR[2] = fh_ds_read128<2048>(abase + so);                       \
    AR[3] = fh_ds_read128<3072>(abase + so);                       \
    AR[4] = fh_ds_read128<4096>(abase + so);                       \
    AR[5] = fh_ds_read128<5120>(abase + so);                       \
    BR[0] = fh_ds_read128<0>(bbase + so);                          \
    BR[1] = fh_ds_read128<1024>(bbase + so);                       \
    BR[2] = fh_ds_read128<2048>(bbase + so);                       \
    BR[3] = fh_ds_read128<3072>(bbase + so);                       \
    BR[4] = fh_ds_read128<4096>(bbase + so);                       \
  } while (0)
  // step s: stage s+1 has landed everywhere after the barrier; stage s+NS goes into the buffer of stage s, whose fragments every
  // wave holds in registers since before it arrived at this barrier; the reads of s+1 fly under the MFMAs of s
#define DMA_STEP(S, AC, BC, AN, BN)                                                            \
  do {                                                                                         \
    const int s_ = (S);                                                                        \
    if (s_ + 1 < KB) {                                                                         \
      const int rem = KB - 2 - s_; /* stages issued beyond s+1 */                              \
      if (NS == 4 && rem >= 2) DMA_WAIT(2);                                                    \
      else if (rem >= 1) DMA_WAIT(1);                                                          \
      else DMA_WAIT(0);                                                                        \
    }                                                                                          \
    __builtin_amdgcn_s_barrier();                                                              \
    if (s_ + NS < KB) issue(s_ + NS);                                                          \
    if (s_ + 1 < KB) DMA_READ(s_ + 1, AN, BN);                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                         \
    _Pragma("unroll") for (int i = 0; i < 6; ++i)                                              \
      _Pragma("unroll") for (int j = 0; j < 5; ++j) acc[i][j] = T::mfma(BC[j], AC[i], acc[i][j]); \
    __builtin_amdgcn_sched_barrier(0);                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                         \
    __builtin_amdgcn_sched_barrier(0);                                                         \
  } while (0)

  // Staggered form (STG = 1; 1021 vs 1045 us per launch of the hoisted projection).  In lock step all 8 waves read fragments at
  // the same time and multiply at the same time, and ablation builds showed the LDS time and the MFMA time of a step adding up
  // rather than overlapping.  Here the wave rows run half a step apart: a step is [barrier A | DMA issue + fragment reads of s+1, waited for |
  // barrier B | MFMAs of s], and row 1 executes one extra barrier first - while row 0 multiplies, row 1 (the other wave of
  // each SIMD) reads, and vice versa.  Row 0 reads stage s+1 one barrier before row 1 does, so a wave of row 0 waits for its
  // share of stage s+1 before its barrier A, a wave of row 1 for its share of stage s+2 before its barrier B (the same global
  // barrier).  Stage s+NS is issued after both rows have read stage s.  Row 0 runs one extra barrier at the end: every wave
  // executes 2 KB + 2 barriers.
#define DMA_WAIT_UPTO(K)                      \
  do {                                        \
    const int k_ = (K);                       \
    if (NS == 4 && k_ >= 2) DMA_WAIT(2);      \
    else if (k_ >= 1) DMA_WAIT(1);            \
    else DMA_WAIT(0);                         \
  } while (0)
#define DMA_STEP_STG(S, AC, BC, AN, BN)                                                        \
  do {                                                                                         \
    const int s_ = (S);                                                                        \
    if (!g1 && s_ + 1 < KB) DMA_WAIT_UPTO(KB - 2 - s_);                                        \
    __builtin_amdgcn_s_barrier();                                                              \
    if (s_ + NS < KB) issue(s_ + NS);                                                          \
    if (s_ + 1 < KB) DMA_READ(s_ + 1, AN, BN);                                                 \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                         \
    __builtin_amdgcn_sched_barrier(0);                                                         \
    if (g1 && s_ + 2 < KB) {                                                                   \
      DMA_WAIT_UPTO(KB - 3 - s_);                                                              \
    }                                                                                          \
    __builtin_amdgcn_s_barrier();                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                         \
    _Pragma("unroll") for (int i = 0; i < 6; ++i)                                              \
      _Pragma("unroll") for (int j = 0; j < 5; ++j) acc[i][j] = T::mfma(BC[j], AC[i], acc[i][j]); \
    __builtin_amdgcn_sched_barrier(0);                                                         \
  } while (0)

  const bool g1 = wr == 1;
#ifdef DMA_CLK
  const unsigned long long c0 = clock64(), w0 = wall_clock64();
#endif
#pragma unroll
  for (int s = 0; s < NS; ++s) issue(s);
  if constexpr (STG) DMA_WAIT(NS - 2);  // stages 0 and 1: row 0 reads stage 1 right after the first barrier of the loop
  else DMA_WAIT(NS - 1);
  __builtin_amdgcn_s_barrier();
  DMA_READ(0, a0, b0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (STG) {
    if (g1) __builtin_amdgcn_s_barrier();
    for (int s = 0; s < KB; s += 2) {
      DMA_STEP_STG(s, a0, b0, a1, b1);
      DMA_STEP_STG(s + 1, a1, b1, a0, b0);
    }
    if (!g1) __builtin_amdgcn_s_barrier();
  } else {
    for (int s = 0; s < KB; s += 2) {
      DMA_STEP(s, a0, b0, a1, b1);
      DMA_STEP(s + 1, a1, b1, a0, b0);
    }
  }
#ifdef DMA_CLK
  if ((blockIdx.x == 3000 || blockIdx.x == 6001) && threadIdx.x == 0) {
    const unsigned long long c1 = clock64(), w1 = wall_clock64();
    printf("tile loop: %llu core clocks, %llu wall ticks\n", c1 - c0, w1 - w0);
  }
#endif
#undef DMA_STEP_STG
#undef DMA_WAIT_UPTO
#undef DMA_STEP
#undef DMA_READ
#undef DMA_WAIT
  // D[n = q*4 + reg][m = r16]: lane -> one row, 4 consecutive columns per (i, j)
  float* const outz = g.out_f32 + (size_t)bz * g.o_zstride;
  // Through LDS (the ring is idle: nobody reads it after the barrier of the last step), 96 rows per pass, so that a store
  // instruction writes 1 KiB of one output row - 8 whole lines - instead of 16 half lines 205 KB apart (straight from the
  // accumulators the launch took 1260 us instead of 1150).  Row stride OW + 4
  // floats: the 16 rows of a lane group then fall on the 16 different 16-byte bank slots.
  constexpr int OW = CT * 16, OSTR = OW + 4, C4 = OW / 4, NTHR = NW * 64;
  static_assert(96 * OSTR * 4 <= NS * STAGE, "output staging does not fit the ring");
  float* const so = reinterpret_cast<float*>(ring);
  float4 bb[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) bb[j] = *reinterpret_cast<const float4*>(g.bias + (bx * CT + wc * 5 + j) * 16 + q * 4);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if (wr == p) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j)
          *reinterpret_cast<float4*>(so + (i * 16 + r16) * OSTR + (wc * 5 + j) * 16 + q * 4) =
              float4{acc[i][j][0] + bb[j].x, acc[i][j][1] + bb[j].y, acc[i][j][2] + bb[j].z, acc[i][j][3] + bb[j].w};
    }
    __syncthreads();
    {
#pragma unroll
      for (int k = 0; k < (96 * C4) / NTHR; ++k) {
        const int idx = k * NTHR + threadIdx.x, rl = idx / C4, c4 = idx - rl * C4;
        const int row = by * (RT * 16) + p * 96 + rl;
        if (row < g.M)
          *reinterpret_cast<float4*>(outz + (size_t)row * g.ldo + bx * OW + c4 * 4) = *reinterpret_cast<const float4*>(so + rl * OSTR + c4 * 4);
      }
    }
    if (p == 0) __syncthreads();
  }
}

// LayerNorm (no affine, biased variance, eps 1e-6) + framewise modulate, one wave per token row
// (FMT.py:157,168-169,174-175,197).  out = T( (x-mu)*rstd * (1 + scale[row]) + shift[row] ), written in
// the packed A-operand order of the consuming GEMM (K = D).
// KS > 0: the residual update of the preceding split-K GEMM (EPI_PARTIAL) is folded in first,
//   x[row] += gate[row] * (bias + slab[0][row] + ... + slab[KS-1][row])      (fixed order: bitwise reproducible)
// and the new residual row is written back, so the gated add costs no launch and no extra round trip:
// every operand of the row is requested before the first one is used.
struct LnRed {
  const float* slab;   // [KS][rows][D] partial sums of the GEMM
  size_t slab_stride;
  const float* bias;   // [D]
  const float* gate;   // row stride ldm (a column block of the modulation matrix)
};

constexpr int kLnTouch = 6;  // lines per lane: 192 single-wave workgroups cover 8 XCDs x 1 MB (fc1) with 6

// Body: `wpb` waves per workgroup (1 = one row per workgroup, the XCD-grouped mapping).
template <class T, int NV, int KS, bool TOUCH, bool WT>
__device__ __forceinline__ void fmt_lnmod_body(float* __restrict__ x, int M, const float* __restrict__ shift,
                                               const float* __restrict__ scale, int ldm, u16* __restrict__ out, const LnRed& red,
                                               const TouchSpec& pf, int ntok, int perm, unsigned long long* sat, const int wpb) {
  constexpr int D = NV * 256;
  const unsigned bid = blockIdx.x, nblk = gridDim.x;
  const int lane = threadIdx.x & 63;
  int row = bid * wpb + (threadIdx.x >> 6);
  unsigned touched[kLnTouch] = {};
  const bool touch = TOUCH && wpb == 1;
  // (`pf` and `nblk` belong to the tail of fmt_lnmod_kernel's parameters: nothing of them is needed before the row's loads)
  auto touch_lines = [&]() { fmt_touch(pf, bid & 7, (bid >> 3) * 64 + lane, (nblk >> 3) * 64, touched); };
  if (wpb == 1) {
    // One row per workgroup: a 128-byte line of the packed output holds the 16-byte pieces of 8 consecutive rows, so give
    // those 8 rows to workgroups of ONE XCD (ids congruent mod 8 share an XCD's L2, where the pieces merge into full lines
    // before they are written back; ablation: the stores cost 1 of the kernel's 4.7 us when 8 XCDs each owned a piece).
    const int x = bid & 7, j = bid >> 3;
    row = (((j >> 3) * 8 + x) << 3) + (j & 7);
  }
  if (row >= M) {
    if (touch) {
      touch_lines();
      fmt_touch_retire(touched);
    }
    return;
  }
  float* xr = x + (size_t)row * D;
#ifdef FMT_DIAG_HOTMOD  // timing-only build (WRONG results): every row reads the modulation row 0 - what the fp32 slab's reads cost
  const size_t mrow = 0;
#else
  const size_t mrow = (size_t)row;
#endif
  const float* sh = shift + mrow * ldm;
  const float* sc = scale + mrow * ldm;
  float4 v[NV], a[NV], b[NV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 256 + lane * 4;
    v[i] = fh_load_f4(xr + c);
    a[i] = fh_load_f4_stream(sh + c);
    b[i] = fh_load_f4_stream(sc + c);
  }
  if (KS == 0 && touch) touch_lines();  // behind the row's own loads (in-order retirement)
  if constexpr (KS > 0) {
    float4 p[KS][NV], gt[NV], bi[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 256 + lane * 4;
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        const float* ps = red.slab + k * red.slab_stride + (size_t)row * D + c;
        p[k][i] = fh_load_f4_stream(ps);  // the slab's only read
      }
      gt[i] = fh_load_f4_stream(red.gate + mrow * ldm + c);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) bi[i] = *reinterpret_cast<const float4*>(red.bias + i * 256 + lane * 4);  // tail (fmt_lnmod_kernel)
    if (touch) touch_lines();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float4 t = p[0][i];
#pragma unroll
      for (int k = 1; k < KS; ++k) {
        t.x += p[k][i].x;
        t.y += p[k][i].y;
        t.z += p[k][i].z;
        t.w += p[k][i].w;
      }
      v[i].x += gt[i].x * (t.x + bi[i].x);
      v[i].y += gt[i].y * (t.y + bi[i].y);
      v[i].z += gt[i].z * (t.z + bi[i].z);
      v[i].w += gt[i].w * (t.w + bi[i].w);
      fh_store_f4_wt<1, WT>(xr + i * 256 + lane * 4, v[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mu = wave_sum(s) * (1.f / D);
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float d0 = v[i].x - mu, d1 = v[i].y - mu, d2 = v[i].z - mu, d3 = v[i].w - mu;
    s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const float rstd = rsqrtf(wave_sum(s2) * (1.f / D) + 1e-6f);
  // perm = (clips * bc) * 16: token-blocked output rows for the CFG head GEMM (GemmArgs::tokblk); b counts the
  // (clip, CFG row) sequences, so a token block holds clip-major, CFG-row-minor row tiles
  unsigned rm = 0u;
  int orow = row;
  if (perm) {
    const int b = row / ntok, i = row - b * ntok;
    orow = (i >> 4) * perm + b * 16 + (i & 15);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 256 + lane * 4;
    fh_store4_wt<T, 1, WT>(reinterpret_cast<typename T::elem*>(out) + fmt_pack_off(orow, c, D / 32),
              (v[i].x - mu) * rstd * (1.f + b[i].x) + a[i].x, (v[i].y - mu) * rstd * (1.f + b[i].y) + a[i].y,
              (v[i].z - mu) * rstd * (1.f + b[i].z) + a[i].z, (v[i].w - mu) * rstd * (1.f + b[i].w) + a[i].w, rm);
  }
  fh_range_flush<T>(sat, rm);
  if (touch) fmt_touch_retire(touched);
}

template <class T, int NV, int KS, bool TOUCH, bool WT>
__global__ __launch_bounds__(256) void fmt_lnmod_kernel(float* __restrict__ x, const float* __restrict__ shift,
                                                        const float* __restrict__ scale, const float* __restrict__ slab,
                                                        const float* __restrict__ gate, int M, int ldm, int wpb, unsigned slab_stride,
                                                        u16* __restrict__ out, const float* __restrict__ red_bias, TouchSpec pf,
                                                        int ntok, int perm, unsigned long long* sat) {
  // The first 14 dwords - every pointer and size behind the addresses of the row's loads and of the slabs folded into it, the
  // rows per workgroup included (blockDim would be a load from the kernarg segment) - are preloaded into SGPRs at dispatch; the
  // output, the fold's bias, the touch and the permutation come behind and are first read once those loads are in flight.
  const LnRed red{slab, (size_t)slab_stride, red_bias, gate};
  fmt_lnmod_body<T, NV, KS, TOUCH, WT>(x, M, shift, scale, ldm, out, red, pf, ntok, perm, sat, wpb);
}

// Banded attention (FMT.py:71-88 with the mask of FMT.py:15-19): query i sees keys |i-j| <= window.
// LPQ lanes per query, 128/LPQ head dims each; a workgroup is a run of blockDim.x/LPQ queries of one (cfg row, head)
// (blockIdx.y = run), so the 24 (row, head) pairs spread over many CUs - with one 512-thread workgroup per pair only 24 CUs
// pulled q/k/v and the kernel took 5.2 us; single-wave workgroups of 8 queries take 4.1 us.  With at most 2*window+1 keys
// per query this is 0.3 % of the evaluation's flops - MFMA/LDS tiling would only add latency - so q/k/v come straight from
// L2.  For window <= 2 every load of the query's band is issued before the first use (one memory round trip); wider
// windows loop.  Output is written in the packed A-operand order of the proj GEMM (K = D).
// Body: head `h`, run `run` of `qpw` queries (nthr = qpw * LPQ threads take part), `lin` of `nwg` workgroups for the touch.
template <class T, int LPQ, bool TOUCH, bool WT>
__device__ __forceinline__ void fmt_attn_body(const u16* __restrict__ qkv, int ld, u16* __restrict__ out, int ntok, int M, int D,
                                              int window, const FmtDiv ntok_div, const TouchSpec& pf, unsigned long long* sat,
                                              const int h, const int run, const int nthr, const unsigned lin, const unsigned nwg) {
  constexpr int HD = 128, PD = HD / LPQ, NU = PD / 8;
  // blockIdx.x = head, blockIdx.y = run of blockDim.x / LPQ consecutive ROWS of the (cfg rows x tokens) batch: with 8 rows per
  // workgroup the run is one 8-row group of the packed output, whose 128-byte lines then come whole from a single wave
  const int row_ = run * (nthr / LPQ) + threadIdx.x / LPQ, part = threadIdx.x % LPQ;
  unsigned touched[2] = {0u, 0u};
  // issued BEHIND the wave's own q / k / v loads (memory operations retire in order: in front of them, the wave would wait
  // for the touched HBM lines before it could use operands that come from the Infinity Cache)
  auto touch = [&]() {
    if constexpr (TOUCH) {
      fmt_touch(pf, lin & 7, (lin >> 3) * nthr + threadIdx.x, (nwg >> 3) * nthr, touched);
    }
  };
  if (row_ >= M) {  // whole LPQ-lane groups leave together
    touch();
    if constexpr (TOUCH) fmt_touch_retire(touched);
    return;
  }
  const int b = (int)fmt_div((unsigned)row_, ntok_div), qi = row_ - b * ntok;  // row_ / ntok, the host's constant
  const int d0 = h * HD + part * PD;
  const float scale = rsqrtf((float)HD);
  typedef typename T::elem E;
  typedef typename T::pack8 P8;
  const E* base = reinterpret_cast<const E*>(qkv) + (size_t)(b * ntok) * ld + d0;
  float qf[PD], o[PD];
  P8 qq[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) qq[u] = T::load8(base + (size_t)qi * ld + u * 8);
  // converted behind the first k / v loads of either branch below: in front of the branch the conversion made the wave wait for
  // q (a whole memory round trip) before it asked for k and v
  auto scale_q = [&]() {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[u * 8 + j] = T::get(qq[u], j) * scale;
    }
  };
#pragma unroll
  for (int i = 0; i < PD; ++i) o[i] = 0.f;
  float m = -INFINITY, l = 0.f;
  auto score = [&](const P8* k) {  // depends on q and k only
    float dot = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
      for (int j = 0; j < 8; ++j) dot += qf[u * 8 + j] * T::get(k[u], j);
    }
    return group_sum<LPQ>(dot);  // the query's LPQ lanes are one aligned group of a DPP row and leave together (above)
  };
  auto fold = [&](float dot, const P8* v) {
    const float mn = fmaxf(m, dot);
    const float alpha = __expf(m - mn), p = __expf(dot - mn);
    l = l * alpha + p;
    m = mn;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[u * 8 + j] = o[u * 8 + j] * alpha + p * T::get(v[u], j);
    }
  };
  if (window <= 2) {
    P8 kk[5][NU], vv[5][NU];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int kj = min(max(qi + t - 2, 0), ntok - 1);
      const E* kp = base + (size_t)kj * ld + D;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        kk[t][u] = T::load8(kp + u * 8);
        vv[t][u] = T::load8(kp + D + u * 8);
      }
    }
    touch();
    scale_q();
    // (the five scores formed in front of the first fold, so that their reductions overlap: measured, not faster - DESIGN.md §7)
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int kj = qi + t - 2;
      const float dot = score(kk[t]);
      if (kj >= 0 && kj < ntok && (t - 2 >= -window) && (t - 2 <= window)) fold(dot, vv[t]);
    }
  } else {
    touch();
    scale_q();
    for (int kj = qi - window; kj <= qi + window; ++kj) {
      const int kc = min(max(kj, 0), ntok - 1);
      const E* kp = base + (size_t)kc * ld + D;
      P8 k[NU], v[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        k[u] = T::load8(kp + u * 8);
        v[u] = T::load8(kp + D + u * 8);
      }
      const float dot = score(k);
      if (kj >= 0 && kj < ntok) fold(dot, v);
    }
  }
  const float inv = 1.f / l;
  const int row = b * ntok + qi;
  unsigned rm = 0u;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    P8 uo;
#pragma unroll
    for (int j = 0; j < 8; ++j) T::set(uo, j, o[u * 8 + j] * inv);
    fh_track_pack<T>(rm, uo);
    T::template store8_wt<2, WT>(reinterpret_cast<E*>(out) + fmt_pack_off(row, d0 + u * 8, D / 32), uo);
  }
  fh_range_flush<T>(sat, rm);
  if constexpr (TOUCH) fmt_touch_retire(touched);
}

template <class T, int LPQ, bool TOUCH, bool WT>
__global__ __launch_bounds__(512) void fmt_attn_kernel(const u16* __restrict__ qkv, u16* __restrict__ out, int ld, int ntok, int M,
                                                       int D, int window, int nthr, unsigned ntok_mul, unsigned ntok_sh, int heads,
                                                       int nrun, unsigned long long* sat, TouchSpec pf) {
  // 14 preloaded dwords in front of the TouchSpec: the launch's block and grid sizes are among them (blockDim / gridDim would
  // be loads from the kernarg segment), so the q / k / v loads are issued without a scalar-memory round trip in front of them
  fmt_attn_body<T, LPQ, TOUCH, WT>(qkv, ld, out, ntok, M, D, window, FmtDiv{ntok_mul, ntok_sh}, pf, sat, blockIdx.x, blockIdx.y,
                                   nthr, blockIdx.x + (unsigned)heads * blockIdx.y, (unsigned)(heads * nrun));
}

// Test hook (float_fmt_debug request 5): the cross-lane reductions of common.hpp on caller data, one wave per 64-lane vector.
// out[vec][k][form][lane], k = wave sum, wave max, 16-, 8-, 4-lane group sum; form 0 = DPP / lane swap, 1 = __shfl_xor.
constexpr int kXlaneProbeVecs = 64, kXlaneProbeSums = 5;
__global__ __launch_bounds__(64) void fmt_xlane_probe_kernel(const float* __restrict__ in, float* __restrict__ out) {
  const int lane = threadIdx.x;
  const float v = in[blockIdx.x * 64 + lane];
  float* o = out + (size_t)blockIdx.x * kXlaneProbeSums * 2 * 64 + lane;
  o[0 * 64] = wave_sum(v), o[1 * 64] = wave_sum_shfl(v);
  o[2 * 64] = wave_max(v), o[3 * 64] = wave_max_shfl(v);
  o[4 * 64] = group_sum<16>(v), o[5 * 64] = group_sum_shfl<16>(v);
  o[6 * 64] = group_sum<8>(v), o[7 * 64] = group_sum_shfl<8>(v);
  o[8 * 64] = group_sum<4>(v), o[9 * 64] = group_sum_shfl<4>(v);
}

// Condition rows for c_embedder: [wr | wa | we | 0-pad] per (cfg row b, token i) with the CFG nulling
// pattern given as bit masks over b (FMT.py:322-333, 360-373, 382-392).
template <class T>
__global__ void fmt_build_cond_kernel(u16* __restrict__ out, int ld, int bc, int ntok, int n_prev, int dim_w, int dim_a,
                                      int dim_e, const float* __restrict__ wr, const float* __restrict__ wa,
                                      const float* __restrict__ prev_wa, const float* __restrict__ we, int we_len,
                                      const float* __restrict__ prev_we, unsigned wr_mask, unsigned wa_mask,
                                      unsigned we_mask, unsigned long long* sat) {
  // row = (clip * bc + b) * ntok + i; per-clip tensors are stacked: wr (clips, dim_w), wa (clips, n_cur, dim_a),
  // prev_wa (clips, n_prev, dim_a), we (clips, we_len, dim_e), prev_we (clips, n_prev, dim_e)
  const int row = blockIdx.x;
  const int s = row / ntok, i = row % ntok, q = s / bc, b = s - q * bc, n_cur = ntok - n_prev;
  const bool on_r = (wr_mask >> b) & 1, on_a = (wa_mask >> b) & 1, on_e = (we_mask >> b) & 1;
  wr += (size_t)q * dim_w;
  wa += (size_t)q * n_cur * dim_a;
  prev_wa += (size_t)q * n_prev * dim_a;
  we += (size_t)q * we_len * dim_e;
  if (prev_we) prev_we += (size_t)q * n_prev * dim_e;
  unsigned rm = 0u;
  for (int c = threadIdx.x; c < ld; c += blockDim.x) {
    float v = 0.f;
    if (c < dim_w) {
      v = on_r ? wr[c] : 0.f;
    } else if (c < dim_w + dim_a) {
      const int k = c - dim_w;
      // prev_wa is replicated UN-nulled into every CFG row; only the current window is nulled
      // (prev_wa_cat = [prev_wa]*3, FMT.py:366 vs audio_cat, FMT.py:360)
      if (i < n_prev) v = prev_wa[i * dim_a + k];
      else if (on_a) v = wa[(i - n_prev) * dim_a + k];
    } else if (c < dim_w + dim_a + dim_e) {
      const int k = c - dim_w - dim_a;
      if (on_e) {
        if (we_len == 1) v = we[k];
        else v = (i < n_prev) ? prev_we[i * dim_e + k] : we[(i - n_prev) * dim_e + k];
      }
    }
    reinterpret_cast<typename T::elem*>(out)[fmt_pack_off(row, c, ld / 32)] = fh_cvt<T>(v, rm);
  }
  fh_range_flush<T>(sat, rm);
}

// Sinusoidal timestep features [cos(t f_k) | sin(t f_k)], k < 128 (FMT.py:118-123), one row per evaluation of a window.
// The evaluation times are formed here: grid point i of torch.linspace(0, 1, nfe) in fp32 (symmetric around the midpoint:
// i * step below it, 1 - (nfe-1-i) * step above), and for a Runge-Kutta scheme with `stages` stages per step
// t = g_i + c_j (g_{i+1} - g_i) for evaluation s = i * stages + j.  nfe == 0: the single explicit time t0 (float_fmt_eval).
// Separately rounded multiplies and adds (no fma contraction): the times must equal the host's / torch's bit for bit.
__device__ __forceinline__ float fmt_linspace01(int i, int n) {
  if (n <= 1) return 0.f;
  const float step = __fdiv_rn(1.0f, (float)(n - 1));
  return (i < n / 2) ? __fmul_rn(step, (float)i) : __fsub_rn(1.0f, __fmul_rn(step, (float)(n - 1 - i)));
}
template <class T>
__global__ void fmt_tsin_kernel(u16* __restrict__ out, const float* __restrict__ freqs, int n_steps, float t0, int nfe,
                                int stages, float c0, float c1, float c2, float c3) {
  const int s = blockIdx.x;
  if (s >= n_steps) return;
  float t = t0;
  if (nfe > 0) {
    const int i = s / stages, j = s - i * stages;
    const float gi = fmt_linspace01(i, nfe);
    t = gi;
    if (j > 0) {
      const float cj = j == 1 ? c1 : (j == 2 ? c2 : c3);
      t = __fadd_rn(gi, __fmul_rn(__fsub_rn(fmt_linspace01(i + 1, nfe), gi), cj));
    }
  }
  (void)c0;
  const int k = threadIdx.x;  // 0..255
  const float arg = t * freqs[k & 127];
  reinterpret_cast<typename T::elem*>(out)[fmt_pack_off(s, k, 8)] = T::from_float(k < 128 ? cosf(arg) : sinf(arg));
}

// sc16[row] = T(silu(t_emb + c_cond[row]))   (c = t + c_embedder(.), FMT.py:335; SiLU of FMT.py:164,187)
// written packed: the A operand of the fused adaLN projection.  8 columns per thread.
template <class T>
__global__ void fmt_silu_c_kernel(u16* __restrict__ out, const float* __restrict__ temb, const float* __restrict__ ccond,
                                  int M, int D, size_t step_stride, int dense_rows, unsigned long long* sat) {
  // blockIdx.y = Euler step: all steps of a window are produced by one launch when they fit.  dense_rows = 0: one packed image
  // per step, step_stride elements apart; dense_rows = M: ONE packed image whose row z * M + r is row r of step z (fmt_gemm_big4_kernel)
  const int idx = (blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (idx >= M * D) return;
  const int c = idx % D, row = idx / D + (int)blockIdx.y * dense_rows;
  typename T::elem* const o = reinterpret_cast<typename T::elem*>(out) + (dense_rows ? (size_t)0 : (size_t)blockIdx.y * step_stride);
  temb += (size_t)blockIdx.y * D;
  typename T::pack8 u;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 a = *reinterpret_cast<const float4*>(ccond + idx + 4 * h);
    const float4 t = *reinterpret_cast<const float4*>(temb + c + 4 * h);
    T::set(u, 4 * h + 0, fh_silu(a.x + t.x));
    T::set(u, 4 * h + 1, fh_silu(a.y + t.y));
    T::set(u, 4 * h + 2, fh_silu(a.z + t.z));
    T::set(u, 4 * h + 3, fh_silu(a.w + t.w));
  }
  unsigned rm = 0u;
  fh_track_pack<T>(rm, u);
  fh_range_flush<T>(sat, rm);
  T::store8(o + fmt_pack_off(row, c, D / 32), u);
}

// Euler state and x_embedder input rows for a new window, per clip q: xcur[q] = x0[q]; xin16 rows q * ntok + i = [prev_x[q] ; x0[q]].
template <class T>
__global__ void fmt_init_x_kernel(float* __restrict__ xcur, u16* __restrict__ xin16, int ldx, const float* __restrict__ x0,
                                  const float* __restrict__ prev_x, int n_prev, int n_cur, int dim_w, int nclip,
                                  unsigned long long* sat) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int ntok = n_prev + n_cur;
  if (idx >= nclip * ntok * dim_w) return;
  const int q = idx / (ntok * dim_w), r = idx - q * ntok * dim_w;
  const int i = r / dim_w, c = r % dim_w;
  float v;
  if (i < n_prev) {
    v = prev_x[((size_t)q * n_prev + i) * dim_w + c];
  } else {
    v = x0[((size_t)q * n_cur + (i - n_prev)) * dim_w + c];
    xcur[((size_t)q * n_cur + (i - n_prev)) * dim_w + c] = v;
  }
  unsigned rm = 0u;
  reinterpret_cast<typename T::elem*>(xin16)[fmt_pack_off(q * ntok + i, c, ldx)] = fh_cvt<T>(v, rm);
  fh_range_flush<T>(sat, rm);
}

// Explicit Runge-Kutta glue for the non-Euler fixed-grid solvers: y = xcur + sum_m coef[m] * k_m over the
// current-window rows of every clip (coef already includes dt).  final = 0: y is the next stage's input (packed 16-bit
// rows of the x_embedder operand); final = 1: y becomes the new state and the next step's stage-0 input.
// kbuf: [stage][clip][ntok][W] with stage stride kstride.
template <class T>
__global__ void fmt_rk_combine_kernel(float* __restrict__ xcur, const float* __restrict__ kbuf, size_t kstride, int nk, float c0,
                                      float c1, float c2, float c3, int final, u16* __restrict__ xin16, int ldx, int n_prev,
                                      int n_cur, int W, int nclip, unsigned long long* sat) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nclip * n_cur * W) return;
  const int q = idx / (n_cur * W), r = idx - q * n_cur * W;
  const int i = r / W, c = r % W, ntok = n_prev + n_cur;
  const float cf[4] = {c0, c1, c2, c3};
  float y = xcur[idx];
  for (int m = 0; m < nk; ++m) y += cf[m] * kbuf[(size_t)m * kstride + ((size_t)q * ntok + n_prev + i) * W + c];
  if (final) xcur[idx] = y;
  unsigned rm = 0u;
  reinterpret_cast<typename T::elem*>(xin16)[fmt_pack_off(q * ntok + n_prev + i, c, ldx)] = fh_cvt<T>(y, rm);
  fh_range_flush<T>(sat, rm);
}

// Window slice with replicate padding along time (FLOAT.py:224-227), per clip: dst[q][i] = src[q][min(t0+i, T-1)].
__global__ void fmt_slice_pad_kernel(float* __restrict__ dst, const float* __restrict__ src, int t0, int T, int n, int dim,
                                     int nclip) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nclip * n * dim) return;
  const int q = idx / (n * dim), r = idx - q * n * dim;
  const int i = r / dim, c = r % dim;
  const int t = min(t0 + i, T - 1);
  dst[idx] = src[((size_t)q * T + t) * dim + c];
}

// AR hand-off (FLOAT.py:217-222; nodes_adv.py:682-686), per clip: dst[q] = the last n_prev rows of src[q] (n_cur rows).
__global__ void fmt_tail_kernel(float* __restrict__ dst, const float* __restrict__ src, int n_prev, int n_cur, int dim, int nclip) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nclip * n_prev * dim) return;
  const int q = idx / (n_prev * dim), r = idx - q * n_prev * dim;
  dst[idx] = src[((size_t)q * n_cur + (n_cur - n_prev)) * dim + r];
}

// Ragged jobs (float_fmt_sample_begin_ragged): clips of their own lengths, each behind its own device pointer.  The table of a
// launch travels BY VALUE in the kernel arguments (192 bytes), so no host table is read by the stream and a caller's capture
// records the pointers themselves; slot q of the launch is blockIdx.y, so the table is indexed uniformly per workgroup.
constexpr int kFmtMaxClips = 16;  // the operator's clip limit (float_fmt_cfg_t::max_batch)
template <class P>
struct FmtClipTab {
  P p[kFmtMaxClips];
  int T[kFmtMaxClips];  // rows behind p[q]
};

// Ragged counterpart of fmt_slice_pad_kernel: dst[q][i] = src.p[q][min(t0 + i, src.T[q] - 1)] for i < n, per clip q < gridDim.y
// (replicate padding along time, FLOAT.py:224-227).  n = 1, t0 = 0 stages one row per clip (wr, a static we) in slot order.
__global__ void fmt_gather_pad_kernel(float* __restrict__ dst, const FmtClipTab<const float*> src, int t0, int n, int dim) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  if (r >= n * dim) return;
  const int i = r / dim, c = r - i * dim;
  const int t = min(t0 + i, src.T[q] - 1);
  dst[(size_t)q * n * dim + r] = src.p[q][(size_t)t * dim + c];
}

// Ragged counterpart of the r_d copy: dst.p[q][t0 + i] = src[q][i] for the rows i < n with t0 + i < dst.T[q] (trim to T,
// FLOAT.py:252): the padded rows of a clip's last window never leave the workspace.
__global__ void fmt_scatter_trim_kernel(const FmtClipTab<float*> dst, const float* __restrict__ src, int t0, int n, int dim) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  if (r >= n * dim) return;
  const int i = r / dim, c = r - i * dim;
  if (t0 + i >= dst.T[q]) return;
  dst.p[q][(size_t)(t0 + i) * dim + c] = src[(size_t)q * n * dim + r];
}

// (the test hook's conversion kernels fmt_dbg_to16_kernel / fmt_dbg_unpack_kernel live in fmt_pack.hpp: the audio hook shares them)

// Device-side copies / fills of the sampling calls.  Kernels, not hipMemcpyAsync / hipMemsetAsync: when the caller captures the
// stream those become memcpy / memset NODES, and replays of such a graph were not reproducible on ROCm 7.2 (the r_d copy of
// window k raced with window k+1's writes to the Euler state: the first 16 frames of a window differed from replay to replay);
// kernel nodes of one captured stream keep their order.  rows x width floats, pitches in floats; src == nullptr fills zeros.
__global__ void fmt_copy_kernel(float* __restrict__ dst, size_t dpitch, const float* __restrict__ src, size_t spitch, int width, int rows) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * width) return;
  const int r = idx / width, c = idx - r * width;
  dst[(size_t)r * dpitch + c] = src ? src[(size_t)r * spitch + c] : 0.f;
}
