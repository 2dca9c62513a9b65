// HIP kernels of the motion pass of the encoder: EncoderApp + Encoder.fc over a block of stacked driving frames (reference
// encoder.py:262-277: `h_motion_target = fc(net_app(input_target))`), one lambda row per frame, no skip features.  Activations
// are [frame][y][x][channel] in the operand type T (16-bit in production, fp32 in the verification mode: the same kernels on
// T::elem / T::pack8), accumulation is fp32.  conv1 of every ResBlock runs the decoder's LDS-tiled 3x3 kernels, which take a
// frame count as they are (encm_api.hip); what is here is the rest of the chain.
//
// Frame independence: every reduction below has a K-order that depends on the frame's own pixels only (chunks of 32 input
// channels in rising order, taps row-major inside a chunk, a fixed lane / wave order where lanes or waves split K), so row t
// of the result does not depend, by a bit, on the number of frames, the block size or the frame's neighbours in a workgroup.
#pragma once
#include "common.hpp"
#include "enc_fir.hpp"

// ------------------------------------------------------------------------------------------
// convs.0 on 8-bit frames: (q / 127.5 - 1) (generate.py:37 of the reference, in fp32) -> EqualConv2d 1x1 (3 -> C) +
// FusedLeakyReLU.  frames [npix][3] uint8 (npix = frames x S x S), out [npix][C].  One thread = one pixel x 8 channels.
template <class T>
__global__ __launch_bounds__(256) void encm_first_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ w /*[C][3] scaled*/,
                                                         const float* __restrict__ bias, typename T::elem* __restrict__ out, size_t npix,
                                                         int C, unsigned long long* sat) {
  const int c8 = C >> 3;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= npix * c8) return;
  const int cg = (int)(idx % c8);
  const size_t p = idx / c8;
  const uint8_t* px = frames + p * 3;
  const float r = (float)px[0] / 127.5f - 1.0f, g = (float)px[1] / 127.5f - 1.0f, b = (float)px[2] / 127.5f - 1.0f;
  typename T::pack8 o;
  unsigned rm = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = cg * 8 + i;
    fh_set<T>(o, i, fh_lrelu_s2(w[c * 3 + 0] * r + w[c * 3 + 1] * g + w[c * 3 + 2] * b + bias[c]), rm);
  }
  fh_range_flush<T>(sat, rm);
  T::store8(out + p * C + cg * 8, o);
}

// ------------------------------------------------------------------------------------------
// The tail of a ResBlock in one launch (encoder.py:183-199):
//   y = (act(conv2_3x3_s2(Blur_pad2(t1)) + bias) + skip_1x1_s2(Blur_pad1(x))) / sqrt(2),  R x R -> R/2 x R/2.
// A workgroup owns 64 output pixels x BN = NT*16 output channels: NF whole output tiles of TO x TO pixels (TO = 8 where the
// output is at least 8 px wide: NF = 1 tile of one frame; below that TO = the whole output and the 64 rows of M hold NF
// different FRAMES, each staged behind its own zero border, so a halo never reads the neighbouring frame).  Per chunk of 32
// input channels:
//   1. the raw halo tile of t1 ((2 TO + 4)^2 pixels per tile, zeros outside the frame) and the chunk's weight slabs
//      ([9][BN] rows of conv2, [BN] rows of the skip conv) go to LDS;
//   2. the 4 x 4 FIR (the handle's EncFir: the checkpoint's taps, flipped) runs in LDS: (2 TO + 1)^2 blurred pixels per
//      tile, rounded to T exactly where the unfused chain stored the blurred map;
//   3. the raw tile of x ((2 TO + 2)^2) replaces t1's, and its FIR is evaluated at the TO^2 even positions only - the 1x1
//      stride-2 conv reads nothing else;
//   4. 9 MFMA steps of conv2 over the blurred tile (A fragment of tap (ty, tx): blurred pixel (2 oy + ty, 2 ox + tx)) and
//      one of the skip conv, into separate accumulators (the activation applies to conv2 alone).
// Neither blurred map exists in HBM.  The weight slabs are staged once per workgroup and chunk and serve all NF frames.
// LDS rows are 32 channels; the 16-byte (pack8) slot of a row is XOR-ed with (column >> 1) & 3 of the blurred tile (stride-2
// fragment reads) or (row >> 1) & 3 (weights, skip tile), as the decoder's tiles are.
// Budget (16-bit, NT = 4): raw 25.6 KB (TO = 8) .. 65.5 KB (16 frames of 4 px), blurred 18.5 .. 25.6 KB, skip tile 4 KB,
// weights 36.9 + 4 KB: 89 .. 135 KB of the CU's 160.  Registers: 2 x NT accumulators (32 VGPRs) + fragments.
struct EncmTailArgs {
  const void* T1;     // [F][R][R][C] conv1's output
  const void* X;      // [F][R][R][C] the block's input
  const void* W2;     // [9][Cout][C]
  const void* Ws;     // [Cout][C]
  const float* bias;  // [Cout] of conv2's FusedLeakyReLU
  void* Y;            // [F][R/2][R/2][Cout]
  int F, R, C, Cout;
  int lto, lnf;       // log2 of the output tile edge TO and of the tiles (frames) per workgroup NF; NF * TO^2 <= 64
  int tiles;          // output tiles per frame edge = (R/2) >> lto
  EncFir fir2, firs;
  unsigned long long* sat;
};

// bytes of dynamic LDS of encm_tail_kernel<T, NT>
template <class T, int NT>
constexpr size_t encm_tail_lds(int lto, int lnf) {
  const size_t TO = (size_t)1 << lto, NF = (size_t)1 << lnf, RB = 32 * T::EB;
  return (NF * (2 * TO + 4) * (2 * TO + 4) + NF * (2 * TO + 1) * (2 * TO + 1) + 64 + 10 * NT * 16) * RB;
}

template <class T, int NT>
__global__ __launch_bounds__(256) void encm_tail_kernel(EncmTailArgs g) {
  typedef typename T::elem E;
  typedef typename T::pack8 P8;
  constexpr int RB = 32 * T::EB, CB = 8 * T::EB, BN = NT * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int TO = 1 << g.lto, NF = 1 << g.lnf;
  const int RS = 2 * TO + 4, XS = 2 * TO + 2, BS = 2 * TO + 1;
  const int nraw = NF * RS * RS, nxraw = NF * XS * XS, nbl = NF * BS * BS, nsk = NF * TO * TO;
  unsigned char* const sR = smem;                   // raw tiles of t1, then of x
  unsigned char* const sBl = sR + (size_t)nraw * RB;  // blurred t1 tiles
  unsigned char* const sSb = sBl + (size_t)nbl * RB;  // blurred x at the even positions, [64] rows
  unsigned char* const sW = sSb + 64 * RB;           // [9][BN] rows
  unsigned char* const sWs = sW + 9 * BN * RB;       // [BN] rows
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const E* const T1 = reinterpret_cast<const E*>(g.T1);
  const E* const X = reinterpret_cast<const E*>(g.X);
  const E* const W2 = reinterpret_cast<const E*>(g.W2);
  const E* const Ws = reinterpret_cast<const E*>(g.Ws);

  int bid = blockIdx.x;
  const int tx0 = bid % g.tiles;
  bid /= g.tiles;
  const int ty0 = bid % g.tiles;
  const int f0 = (bid / g.tiles) * NF;  // first frame of the workgroup
  const int n0 = blockIdx.y * BN;
  const int oy0 = ty0 * TO, ox0 = tx0 * TO;  // output origin of the tile
  const int R = g.R, C = g.C, Ro = R >> 1;

  // this lane's row of M: tile (frame) fl, output pixel (oy, ox) of the tile
  const int m = w * 16 + r16;
  const bool mvalid = m < nsk && f0 + (m >> (2 * g.lto)) < g.F;
  const int mfl = mvalid ? m >> (2 * g.lto) : 0, moy = mvalid ? (m >> g.lto) & (TO - 1) : 0, mox = mvalid ? m & (TO - 1) : 0;
  const int abase = (mfl * BS + 2 * moy) * BS + 2 * mox;  // blurred pixel of tap (0, 0)
  const int msk = mvalid ? m : 0;

  f32x4 acc[NT], accs[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = accs[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  unsigned rm = 0u;

  for (int c0 = 0; c0 < C; c0 += 32) {
    __syncthreads();  // the MFMAs of the previous chunk are done with every tile
    // 1. raw halo of t1: tile pixel (hy, hx) = frame pixel (2 oy0 - 2 + hy, 2 ox0 - 2 + hx); the weight slabs
    for (int e = tid; e < nraw * 4; e += 256) {
      const int p = e >> 2, ch = e & 3;
      const int fl = p / (RS * RS), rem = p - fl * RS * RS;
      const int hy = rem / RS, hx = rem - hy * RS;
      const int f = f0 + fl, iy = 2 * oy0 - 2 + hy, ix = 2 * ox0 - 2 + hx;
      P8 v = T::zero8();
      if (f < g.F && iy >= 0 && iy < R && ix >= 0 && ix < R) v = T::load8(T1 + (((size_t)f * R + iy) * R + ix) * C + c0 + ch * 8);
      *reinterpret_cast<P8*>(sR + (size_t)e * CB) = v;
    }
    for (int e = tid; e < 10 * BN * 4; e += 256) {
      const int row = e >> 2, ch = e & 3;  // row = tap * BN + n; rows 9 BN .. are the skip conv's
      const int tap = row / BN, n = row - tap * BN;
      const E* src = tap < 9 ? W2 + ((size_t)tap * g.Cout + n0 + n) * C : Ws + (size_t)(n0 + n) * C;
      *reinterpret_cast<P8*>(sW + (size_t)row * RB + (ch ^ ((row >> 1) & 3)) * CB) = T::load8(src + c0 + ch * 8);
    }
    __syncthreads();
    // 2. Blur pad (2, 2): blurred (by, bx) of the tile = sum_ab k[a][b] raw(by + a, bx + b)
    for (int e = tid; e < nbl * 4; e += 256) {
      const int p = e >> 2, ch = e & 3;
      const int fl = p / (BS * BS), rem = p - fl * BS * BS;
      const int by = rem / BS, bx = rem - by * BS;
      float s[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) s[i] = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const P8 u = *reinterpret_cast<const P8*>(sR + (size_t)(((fl * RS + by + a) * RS + bx + b) * 4 + ch) * CB);
          const float kk = g.fir2.k[a * 4 + b];
#pragma unroll
          for (int i = 0; i < 8; ++i) s[i] += kk * T::get(u, i);
        }
      P8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) fh_set<T>(o, i, s[i], rm);
      *reinterpret_cast<P8*>(sBl + (size_t)p * RB + (ch ^ ((bx >> 1) & 3)) * CB) = o;
    }
    __syncthreads();
    // 3. raw halo of x: tile pixel (hy, hx) = frame pixel (2 oy0 - 1 + hy, 2 ox0 - 1 + hx); Blur pad (1, 1) at the even positions
    for (int e = tid; e < nxraw * 4; e += 256) {
      const int p = e >> 2, ch = e & 3;
      const int fl = p / (XS * XS), rem = p - fl * XS * XS;
      const int hy = rem / XS, hx = rem - hy * XS;
      const int f = f0 + fl, iy = 2 * oy0 - 1 + hy, ix = 2 * ox0 - 1 + hx;
      P8 v = T::zero8();
      if (f < g.F && iy >= 0 && iy < R && ix >= 0 && ix < R) v = T::load8(X + (((size_t)f * R + iy) * R + ix) * C + c0 + ch * 8);
      *reinterpret_cast<P8*>(sR + (size_t)e * CB) = v;
    }
    __syncthreads();
    for (int e = tid; e < nsk * 4; e += 256) {
      const int p = e >> 2, ch = e & 3;  // p = row of M
      const int fl = p >> (2 * g.lto), oy = (p >> g.lto) & (TO - 1), ox = p & (TO - 1);
      float s[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) s[i] = 0.f;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const P8 u = *reinterpret_cast<const P8*>(sR + (size_t)(((fl * XS + 2 * oy + a) * XS + 2 * ox + b) * 4 + ch) * CB);
          const float kk = g.firs.k[a * 4 + b];
#pragma unroll
          for (int i = 0; i < 8; ++i) s[i] += kk * T::get(u, i);
        }
      P8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) fh_set<T>(o, i, s[i], rm);
      *reinterpret_cast<P8*>(sSb + (size_t)p * RB + (ch ^ ((p >> 1) & 3)) * CB) = o;
    }
    __syncthreads();
    // 4. conv2's nine taps and the skip conv
    const unsigned brow = (unsigned)(r16 * RB + (q ^ ((r16 >> 1) & 3)) * CB);
#pragma unroll
    for (int ty = 0; ty < 3; ++ty)
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) {
        const int col = 2 * mox + tx;
        const P8 a = *reinterpret_cast<const P8*>(sBl + (size_t)(abase + ty * BS + tx) * RB + (q ^ ((col >> 1) & 3)) * CB);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const P8 b = *reinterpret_cast<const P8*>(sW + (size_t)((ty * 3 + tx) * BN + j * 16) * RB + brow);
          acc[j] = T::mfma(b, a, acc[j]);  // D = W (16 channels x K) * X^T: a lane ends with 4 consecutive channels of one pixel
        }
      }
    {
      const P8 a = *reinterpret_cast<const P8*>(sSb + (size_t)msk * RB + (q ^ ((msk >> 1) & 3)) * CB);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const P8 b = *reinterpret_cast<const P8*>(sWs + (size_t)(j * 16) * RB + brow);
        accs[j] = T::mfma(b, a, accs[j]);
      }
    }
  }

  if (mvalid) {
    const float inv_s2 = 0.70710678118654752f;
    E* yp = reinterpret_cast<E*>(g.Y) + (((size_t)(f0 + mfl) * Ro + oy0 + moy) * Ro + ox0 + mox) * g.Cout;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int co = n0 + j * 16 + q * 4;
      const float4 bb = *reinterpret_cast<const float4*>(g.bias + co);
      fh_store4<T>(yp + co, (fh_lrelu_s2(acc[j][0] + bb.x) + accs[j][0]) * inv_s2, (fh_lrelu_s2(acc[j][1] + bb.y) + accs[j][1]) * inv_s2,
                   (fh_lrelu_s2(acc[j][2] + bb.z) + accs[j][2]) * inv_s2, (fh_lrelu_s2(acc[j][3] + bb.w) + accs[j][3]) * inv_s2, rm);
    }
  }
  fh_range_flush<T>(g.sat, rm);
}

// ------------------------------------------------------------------------------------------
// EqualConv2d(C, dim, 4, padding 0) on the 4 x 4 maps of F frames as ONE GEMM: row f of X is the frame's [16][C] map, K = 16 C
// (tap-major, as the packed weights [16][dim][C] are), s[f][n] fp32.  A workgroup owns 16 frames x 16 outputs; its four waves
// split K by taps (wave w: taps 4w .. 4w + 3) and wave 0 adds the partial tiles in wave order through LDS.
template <class T>
__global__ __launch_bounds__(256) void encm_last_kernel(const typename T::elem* __restrict__ X, const typename T::elem* __restrict__ W,
                                                        float* __restrict__ s, int F, int C, int dim) {
  typedef typename T::pack8 P8;
  __shared__ f32x4 red[3][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * 16, f = blockIdx.y * 16 + r16;
  const bool fvalid = f < F;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nchunk = C >> 5;
  for (int t = 4 * w; t < 4 * w + 4; ++t) {
    const typename T::elem* xa = X + ((size_t)(fvalid ? f : 0) * 16 + t) * C + q * 8;
    const typename T::elem* wb = W + ((size_t)t * dim + n0 + r16) * C + q * 8;
    for (int c = 0; c < nchunk; c += 4) {
      P8 a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool live = c + u < nchunk;
        a[u] = (fvalid && live) ? T::load8(xa + (c + u) * 32) : T::zero8();
        b[u] = live ? T::load8(wb + (c + u) * 32) : T::zero8();
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = T::mfma(b[u], a[u], acc);
    }
  }
  if (w > 0) red[w - 1][lane] = acc;
  __syncthreads();
  if (w == 0 && fvalid) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const f32x4 o = red[i][lane];
      acc[0] += o[0], acc[1] += o[1], acc[2] += o[2], acc[3] += o[3];
    }
    *reinterpret_cast<float4*>(s + (size_t)f * dim + n0 + q * 4) = float4{acc[0], acc[1], acc[2], acc[3]};
  }
}

// ------------------------------------------------------------------------------------------
// One EqualLinear of Encoder.fc for F rows: y[f][n] = alpha * sum_k x[f][k] W[n][k] + b[n], fp32.  A wave owns output n of up
// to 8 rows: a weight is read once for all of them; per row the sum is enc_linear_kernel's (lane-strided, then the butterfly).
__global__ __launch_bounds__(256) void encm_fc_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
                                                      float alpha, float* __restrict__ y, int F, int N, int K, int ldy) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int f0 = blockIdx.y * 8;
  if (n >= N) return;
  float s[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) s[r] = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float wv = W[(size_t)n * K + k];
#pragma unroll
    for (int r = 0; r < 8; ++r) s[r] += x[(size_t)min(f0 + r, F - 1) * K + k] * wv;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const float t = wave_sum(s[r]);
    if (lane == 0 && f0 + r < F) y[(size_t)(f0 + r) * ldy + n] = alpha * t + b[n];
  }
}

// ------------------------------------------------------------------------------------------
// Driving rows (Synthesis.forward, styledecoder.py:497-508; Direction is linear, :434-444).  mode 0, absolute:
// r_d[t] = lam[t] Q^T; mode 1, relative: r_d[t] = ((lam[t] - lam_start) + lam_source) Q^T.  fp32, one thread per output,
// terms in rising j.
__global__ __launch_bounds__(256) void encm_rows_kernel(const float* __restrict__ lam, const float* __restrict__ lam_source,
                                                        const float* __restrict__ lam_start, const float* __restrict__ Q /*[dim][dm]*/,
                                                        float* __restrict__ r_d, int T, int dim, int dm, int mode) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)T * dim) return;
  const int i = (int)(idx % dim);
  const size_t t = idx / dim;
  float s = 0.f;
  for (int j = 0; j < dm; ++j) {
    float c = lam[t * dm + j];
    if (mode) c = (c - lam_start[j]) + lam_source[j];
    s = fmaf(c, Q[(size_t)i * dm + j], s);
  }
  r_d[idx] = s;
}
