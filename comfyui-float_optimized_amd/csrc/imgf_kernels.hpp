// Kernels of float_img_front (include/float_hip.h): RGBA conversion, zero-bordered window, exact area / linear resize, 8-bit
// rounding and normalisation of a node's IMAGE input in HBM.  Two launches, no atomics, integers from the quantiser on:
//   imgf_rows_kernel  grid (dst_w tiles, source rows of the window).  A workgroup stages the span of one source row that its
//                     kImgfTile output columns read: every pixel is loaded once (a float4 per RGBA pixel, lanes along the
//                     row), quantised and converted to RGB as it arrives, and kept as one packed dword in LDS; then lane d
//                     walks the taps of output column d and writes the three int32 row sums (at most 255 P) into `work`
//                     as (source row, dst_w, 3).  Pixels outside the image are never staged: they are the zero border.
//   imgf_cols_kernel  grid (dst_w tiles, dst_h).  Lane (dy, dx) adds the row sums of its cell in 64 bits, divides once with a
//                     tie-to-even test and writes planar fp32 (q / 127.5 - 1) or interleaved uint8.
// Lanes read the LDS at a stride of about P / Q dwords, so even factors conflict (8-way at 8 : 1); left as it is: one
// ds_read_b32 per source pixel at 8 cycles is still four pixels per clock and CU, ten times what HBM delivers (16 bytes a
// pixel).  The fp32 expressions (quantiser, blend, normalisation) are written with plain operators under
// `#pragma clang fp contract(off)`: hipcc's __fmul_rn / __fadd_rn are the plain operators too and would contract with their
// neighbours, the pragma is what keeps every operation rounded on its own; fp32 division is correctly rounded by default.
#pragma once
#include "common.hpp"

constexpr int kImgfTile = 256;  // output columns per workgroup = threads per workgroup

struct ImgfAxis {
  int P, Q;  // scale P / Q (reduced): destination cell d covers [d P, (d + 1) P) in units of 1 / Q of a sample
  int n;     // extent of the window
  int off;   // the window's first sample in source coordinates (may be negative)
  int src;   // extent of the source
  int dst;   // extent of the destination
};

struct ImgfPlan {
  ImgfAxis x, y;
  int channels, rgba_mode, linear, out_mode;
  int bkg[3];
  int row_lo, rows;  // the source rows inside the window: [row_lo, row_lo + rows); row r is row r - row_lo of `work`
  int lds_px;        // packed pixels of LDS the launch asked for
};

// clip(x * 255.0, 0, 255) in fp32, truncated; NaN -> 0
__device__ __forceinline__ int imgf_quant(float x) {
#pragma clang fp contract(off)
  const float t = x * 255.0f;
  return t > 0.f ? (t < 255.f ? (int)t : 255) : 0;
}

// rgb * (a / 255) + bkg * (1 - a / 255), every operation rounded to fp32, clipped and truncated
__device__ __forceinline__ int imgf_blend(int c, int a, int bk) {
#pragma clang fp contract(off)
  const float af = (float)a / 255.0f;
  const float om = 1.0f - af;
  const float fg = (float)c * af;
  const float bg = (float)bk * om;
  const float v = fg + bg;
  return v > 0.f ? (v < 255.f ? (int)v : 255) : 0;
}

__device__ __forceinline__ unsigned imgf_pixel(const float* __restrict__ img, size_t px, const ImgfPlan& p) {
  int r, g, b;
  if (p.channels == 4) {
    const float4 v = fh_load_f4_stream(img + px * 4);
    r = imgf_quant(v.x), g = imgf_quant(v.y), b = imgf_quant(v.z);
    if (p.rgba_mode != FLOAT_IMG_RGBA_DISCARD) {
      const int a = imgf_quant(v.w);
      if (p.rgba_mode == FLOAT_IMG_RGBA_BLEND) {
        r = imgf_blend(r, a, p.bkg[0]), g = imgf_blend(g, a, p.bkg[1]), b = imgf_blend(b, a, p.bkg[2]);
      } else if (a == 0) {
        r = p.bkg[0], g = p.bkg[1], b = p.bkg[2];
      }
    }
  } else {
    const float* q = img + px * 3;
    r = imgf_quant(q[0]), g = imgf_quant(q[1]), b = imgf_quant(q[2]);
  }
  return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// the taps of destination index d on one axis: window samples lo ... hi (inclusive)
__device__ __forceinline__ void imgf_span(const ImgfAxis& a, int linear, int d, int* lo, int* hi) {
  const int c0 = d * a.P;
  if (linear) {
    const int sx = min(c0 / a.Q, a.n - 1);
    *lo = sx, *hi = min(sx + 1, a.n - 1);
  } else {
    const int c1 = min(c0 + a.P, a.n * a.Q);
    *lo = c0 / a.Q, *hi = (c1 + a.Q - 1) / a.Q - 1;
  }
}

// linear rule: taps (sx, P - f) and (min(sx + 1, n - 1), f)
__device__ __forceinline__ void imgf_linear_taps(const ImgfAxis& a, int d, int* s0, int* s1, int* f) {
  int sx = (d * a.P) / a.Q;
  const int num = (d + 1) * a.P - (sx + 1) * a.Q;
  int fr = num <= 0 ? 0 : num % a.P;
  if (sx >= a.n - 1) sx = a.n - 1, fr = 0;
  *s0 = sx, *s1 = min(sx + 1, a.n - 1), *f = fr;
}

// dynamic LDS: p.lds_px packed pixels (imgf_api.hip sizes it for the widest tile)
__global__ __launch_bounds__(kImgfTile) void imgf_rows_kernel(const float* __restrict__ img, int* __restrict__ work, const ImgfPlan p) {
  extern __shared__ __attribute__((aligned(16))) unsigned imgf_px[];
  const int tid = threadIdx.x;
  const int row = p.row_lo + blockIdx.y;  // a source row inside the image and the window
  const int d0 = blockIdx.x * kImgfTile, d1 = min(d0 + kImgfTile, p.x.dst) - 1;
  int first, last, t;
  imgf_span(p.x, p.linear, d0, &first, &t);
  imgf_span(p.x, p.linear, d1, &t, &last);
  const int s_lo = max(0, p.x.off + first);                                         // source columns staged: [s_lo, s_lo + n_stage)
  // 0 when the tile lies wholly left or right of the image: it reads the border only, nothing is staged and no tap passes the
  // unsigned tests below
  const int n_stage = max(0, min(min(p.x.src, p.x.off + last + 1) - s_lo, p.lds_px));
  const size_t row_px = (size_t)row * p.x.src;
  for (int k = tid; k < n_stage; k += kImgfTile) imgf_px[k] = imgf_pixel(img, row_px + s_lo + k, p);
  __syncthreads();
  const int d = d0 + tid;
  if (d > d1) return;
  // window sample i sits at LDS index i + sh; anything outside [0, n_stage) is the zero border
  const int sh = p.x.off - s_lo;
  int r = 0, g = 0, b = 0;
  if (p.linear) {
    int s0, s1, f;
    imgf_linear_taps(p.x, d, &s0, &s1, &f);
    const unsigned k0 = (unsigned)(s0 + sh), k1 = (unsigned)(s1 + sh);
    const unsigned v0 = k0 < (unsigned)n_stage ? imgf_px[k0] : 0u, v1 = k1 < (unsigned)n_stage ? imgf_px[k1] : 0u;
    const int w0 = p.x.P - f;
    r = (int)(v0 & 255u) * w0 + (int)(v1 & 255u) * f;
    g = (int)((v0 >> 8) & 255u) * w0 + (int)((v1 >> 8) & 255u) * f;
    b = (int)(v0 >> 16) * w0 + (int)(v1 >> 16) * f;
  } else {
    const int c0 = d * p.x.P, c1 = min(c0 + p.x.P, p.x.n * p.x.Q);
    int i = c0 / p.x.Q;
    for (int pos = i * p.x.Q; pos < c1; pos += p.x.Q, ++i) {
      const unsigned k = (unsigned)(i + sh);
      if (k >= (unsigned)n_stage) continue;
      const unsigned v = imgf_px[k];
      const int w = min(pos + p.x.Q, c1) - max(pos, c0);
      r += (int)(v & 255u) * w, g += (int)((v >> 8) & 255u) * w, b += (int)(v >> 16) * w;
    }
  }
  int* o = work + ((size_t)blockIdx.y * p.x.dst + d) * 3;
  o[0] = r, o[1] = g, o[2] = b;
}

// S / D rounded half to even (0 <= S <= 255 D, 1 <= D <= 2^30)
__device__ __forceinline__ int imgf_round_div(long long S, long long D) {
  const long long q = S / D, r2 = 2 * (S - q * D);
  return (int)q + ((r2 > D || (r2 == D && (q & 1))) ? 1 : 0);
}

__global__ __launch_bounds__(kImgfTile) void imgf_cols_kernel(const int* __restrict__ work, void* __restrict__ out, const ImgfPlan p) {
  const int dx = blockIdx.x * kImgfTile + threadIdx.x, dy = blockIdx.y;
  if (dx >= p.x.dst) return;
  long long S[3] = {0, 0, 0}, D;
  const int* col = work + (size_t)dx * 3;
  const size_t pitch = (size_t)p.x.dst * 3;
  if (p.linear) {
    int s0, s1, f;
    imgf_linear_taps(p.y, dy, &s0, &s1, &f);
    const int rr[2] = {s0 + p.y.off - p.row_lo, s1 + p.y.off - p.row_lo}, ww[2] = {p.y.P - f, f};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if ((unsigned)rr[t] >= (unsigned)p.rows) continue;  // a row of the zero border
      const int* w = col + (size_t)rr[t] * pitch;
#pragma unroll
      for (int c = 0; c < 3; ++c) S[c] += (long long)w[c] * ww[t];
    }
    D = (long long)p.x.P * p.y.P;
  } else {
    const int c0 = dy * p.y.P, c1 = min(c0 + p.y.P, p.y.n * p.y.Q);
    int i = c0 / p.y.Q;
    for (int pos = i * p.y.Q; pos < c1; pos += p.y.Q, ++i) {
      const int rr = i + p.y.off - p.row_lo;
      if ((unsigned)rr >= (unsigned)p.rows) continue;
      const int wy = min(pos + p.y.Q, c1) - max(pos, c0);
      const int* w = col + (size_t)rr * pitch;
#pragma unroll
      for (int c = 0; c < 3; ++c) S[c] += (long long)w[c] * wy;
    }
    const int x0 = dx * p.x.P;
    D = (long long)(min(x0 + p.x.P, p.x.n * p.x.Q) - x0) * (c1 - c0);
  }
  const size_t at = (size_t)dy * p.x.dst + dx, plane = (size_t)p.y.dst * p.x.dst;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int q = imgf_round_div(S[c], D);
    if (p.out_mode == FLOAT_IMG_OUT_HWC_U8) {
      ((unsigned char*)out)[at * 3 + c] = (unsigned char)q;
    } else {
#pragma clang fp contract(off)
      const float v = (float)q / 127.5f;
      ((float*)out)[c * plane + at] = v - 1.0f;
    }
  }
}
