// The image front end's rule as device functions, shared by its kernels (imgf_kernels.hpp: one image, two launches) and by the
// frame-stacked kernel (imgv_kernels.hpp): the axis plan, the fp32 quantiser and blend, a pixel as one packed dword, the taps of a
// destination index under the area and the linear rule, and the division with the tie to even.  The rule itself is written out
// above float_img_front in include/float_hip.h.
#pragma once
#include "common.hpp"

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

// S / D rounded half to even (0 <= S <= 255 D, 1 <= D <= 2^30)
__device__ __forceinline__ int imgf_round_div(long long S, long long D) {
  const long long q = S / D, r2 = 2 * (S - q * D);
  return (int)q + ((r2 > D || (r2 == D && (q & 1))) ? 1 : 0);
}
