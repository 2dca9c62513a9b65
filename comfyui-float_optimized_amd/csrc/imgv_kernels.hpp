// Kernel of float_img_front_frames (include/float_hip.h): the image front end over a stack of frames, one window PER FRAME, in
// one launch per kImgvBlock frames and without any HBM scratch.  The rule is float_img_front's (imgf_kernels.hpp: quantiser,
// RGBA conversion, zero-bordered window, integer area / linear resize, tie to even; imgf_rule.hpp); what is new is how the work is cut:
//   grid (dst_w / 64, dst_h / 32, frames of the block), 256 threads = 4 waves.  A workgroup owns a 64 x 32 output tile of one
//   frame; lane = output column, and wave w owns the band of kImgvBand = 8 output rows w of the tile.  The frame's plan (P / Q
//   per axis, the rule, the tile's and the lane's tap bounds) is formed once, from that frame's rect in the kernel arguments.
//   A wave walks the source rows of its band once, top to bottom.  For each row it stages the span the tile's 64 columns read -
//   lanes along the row, a float4 per fp32 RGBA pixel, a dword per 8-bit RGBA pixel, two aligned dwords funnel-shifted per
//   8-bit RGB pixel; quantised and converted to RGB as it arrives, one packed dword per pixel - into its OWN slice of the LDS,
//   then lane d walks the taps of column d (int32 sums, at most 255 P) and folds them, times the row's vertical weight, into
//   the 64-bit totals it keeps IN REGISTERS for the output row being formed; a source row that ends one cell and begins the
//   next (the only way a row touches two cells under the area rule) is folded into both before the next row is staged.  A
//   finished row is divided once (imgf_round_div) and stored as interleaved uint8.  Under the linear rule the two tapped rows'
//   sums are kept in registers and reused by the next output row, so a source row is staged once per band there too.
//   Nothing is shared between waves: no __syncthreads, no totals in LDS, no atomics; the four waves are at different source
//   rows at any time, so one wave's loads are in flight while another runs its horizontal pass.  The price is the seam: the
//   source row under the border between two bands (non-integer ratios only) is staged by both neighbours, 1 row in about
//   8 P / Q, and the second read comes from the cache, not from HBM.  Rows and columns outside the image are never loaded.
// LDS: a wave's slice is stage_px dwords (the widest span of the block's frames, 64 P / Q + 2, at most kImgvStage = 4096, so
//   at most 64 KiB per workgroup and usually 1 - 3 KiB); a span wider than the slice (beyond 63 : 1) is walked in chunks.  The
//   stores are unit stride; the reads have a stride of about P / Q dwords across lanes, so even factors conflict (8-way at
//   8 : 1), as in imgf_rows_kernel and for the same reason left alone: one ds_read_b32 per source pixel is far above what HBM
//   delivers.  Expected limiter: the HBM read of the windows, 12 or 16 bytes per fp32 pixel (3 or 4 per 8-bit pixel).
// The arithmetic is exact integer arithmetic behind an fp32 quantiser: matrix instructions have no place here.  fp32
//   expressions live in imgf_quant / imgf_blend, under `#pragma clang fp contract(off)`.  This translation unit is compiled
//   with packed fp32 instructions turned off (FLAGS_imgv_api, as the motion pass): the quantiser of a float4 is four independent
//   multiplications that the compiler would otherwise pair into v_pk_mul_f32, and the result has to be the definition's bit for
//   bit on every pixel; the scalar form costs nothing next to the loads.  imgf_api is left as it has been built and tested.
// How a source row's span gets into the slice is a source policy (ImgvSrcF32, ImgvSrcU8 below; ImgySrc in imgy_kernels.hpp for
//   YUV 4:2:0): a template parameter of the kernel, so that the area and linear loops exist once.
#pragma once
#include "imgf_rule.hpp"

constexpr int kImgvBlock = 16;    // frames per launch: their rects travel in the kernel arguments (16 x 16 bytes)
constexpr int kImgvCols = 64;     // output columns of a tile = lanes of a wave
constexpr int kImgvWaves = 4;
constexpr int kImgvBand = 8;      // output rows of a wave
constexpr int kImgvRows = kImgvWaves * kImgvBand;
constexpr int kImgvStage = 4096;  // packed pixels of a wave's LDS slice, at most

struct ImgvArgs {
  const void* frames;        // the block's first frame
  unsigned char* out;        // the block's first output frame
  unsigned long long bytes;  // of the block's source frames (the bounds of the 8-bit RGB dword loads)
  int src_h, src_w, dst_h, dst_w;
  int channels, rgba_mode, bkg[3];
  int scale_num, scale_den;  // the shared scale (reduced), or 0, 0: rect_w / dst_w and rect_h / dst_h per frame
  int stage_px;              // dwords of a wave's LDS slice
  int rect[kImgvBlock][4];   // x, y, w, h per frame
};

// an 8-bit pixel -> the packed RGB dword (the RGBA conversion of imgf_pixel on bytes that are q already)
__device__ __forceinline__ unsigned imgv_pack_u8(int r, int g, int b, int a, const ImgfPlan& p) {
  if (p.channels == 4 && p.rgba_mode != FLOAT_IMG_RGBA_DISCARD) {
    if (p.rgba_mode == FLOAT_IMG_RGBA_BLEND) {
      r = imgf_blend(r, a, p.bkg[0]), g = imgf_blend(g, a, p.bkg[1]), b = imgf_blend(b, a, p.bkg[2]);
    } else if (a == 0) {
      r = p.bkg[0], g = p.bkg[1], b = p.bkg[2];
    }
  }
  return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// pixel `px` of the frame at `img`, 4 bytes at a time.  RGBA: its dword.  RGB: the two aligned dwords that hold its three
// bytes, funnel-shifted - where both lie inside [safe_lo, safe_hi), the aligned part of the block; the first and last bytes of
// an unaligned block are read as bytes.
__device__ __forceinline__ unsigned imgv_pixel_u8(const unsigned char* __restrict__ img, size_t px, const ImgfPlan& p, uintptr_t safe_lo,
                                                   uintptr_t safe_hi) {
  if (p.channels == 4) {
    const unsigned v = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(img) + px);
    return imgv_pack_u8((int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u), (int)(v >> 24), p);
  }
  const uintptr_t at = (uintptr_t)img + px * 3, al = at & ~(uintptr_t)3;
  if (al >= safe_lo && al + 8 <= safe_hi) {
    const unsigned lo = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(al));
    const unsigned hi = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(al) + 1);
    return (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * (unsigned)(at & 3))) & 0xffffffu;
  }
  const unsigned char* q = reinterpret_cast<const unsigned char*>(at);
  return (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
}

// what lane d reads of a staged row: its taps on the x axis, in window samples
struct ImgvTaps {
  int c0, c1;      // area: the cell [c0, c1) in units of 1 / Q
  int lo, hi;      // area: samples lo ... hi; linear: the two taps
  int w_lo, w_hi;  // linear: their weights P - f and f
};

// A source policy says how one source row's span becomes packed RGB dwords in the wave's LDS slice; everything after that - the
// taps, the sums, the totals - is the same code for every source.  A policy has: Args, the kernel's argument struct, and
// common(args), the ImgvArgs in it; slice(args), the dwords of LDS a wave owns (its first stage_px are the RGB slice, the rest
// the policy's own); first_col(c), the first source column that is staged for a span that begins at c (a policy may begin
// earlier, inside the image); a constructor (args, frame of the block, plan, the wave's own LDS); and stage(px, lane, row, col0,
// n), which writes pixels col0 ... col0 + n - 1 of source row `row` (all inside the image) to px[0 ... n - 1].  stage may keep
// state between rows (imgy_kernels.hpp keeps chroma rows); the wave-level barrier after it is the caller's.
struct ImgvSrcF32 {
  using Args = ImgvArgs;
  __device__ static const ImgvArgs& common(const Args& a) { return a; }
  __device__ static int slice(const Args& a) { return a.stage_px; }
  __device__ static int first_col(int c) { return c; }
  const float* frame;
  const ImgfPlan& p;
  __device__ ImgvSrcF32(const Args& a, int fr, const ImgfPlan& plan, unsigned*)
      : frame((const float*)a.frames + (size_t)fr * a.src_h * a.src_w * a.channels), p(plan) {}
  __device__ __forceinline__ void stage(unsigned* px, int lane, int row, int col0, int n) {
    const size_t at = (size_t)row * p.x.src + col0;
    for (int k = lane; k < n; k += kImgvCols) px[k] = imgf_pixel(frame, at + k, p);
  }
};

struct ImgvSrcU8 {
  using Args = ImgvArgs;
  __device__ static const ImgvArgs& common(const Args& a) { return a; }
  __device__ static int slice(const Args& a) { return a.stage_px; }
  __device__ static int first_col(int c) { return c; }
  const unsigned char* frame;
  const ImgfPlan& p;
  uintptr_t safe_lo, safe_hi;  // the aligned part of the block's frames
  __device__ ImgvSrcU8(const Args& a, int fr, const ImgfPlan& plan, unsigned*)
      : frame((const unsigned char*)a.frames + (size_t)fr * a.src_h * a.src_w * a.channels),
        p(plan),
        safe_lo(((uintptr_t)a.frames + 3) & ~(uintptr_t)3),
        safe_hi(((uintptr_t)a.frames + a.bytes) & ~(uintptr_t)3) {}
  __device__ __forceinline__ void stage(unsigned* px, int lane, int row, int col0, int n) {
    const size_t at = (size_t)row * p.x.src + col0;
    for (int k = lane; k < n; k += kImgvCols) px[k] = imgv_pixel_u8(frame, at + k, p, safe_lo, safe_hi);
  }
};

// Stages the tile's span of window row `i` (wave-uniform) chunk by chunk into `px` and returns lane d's three int32 sums in h.
// s_lo, n_tot: the source columns of the span that lie in the image, [s_lo, s_lo + n_tot).
template <class Src>
__device__ __forceinline__ void imgv_row_sums(Src& src, unsigned* px, int lane, int i, const ImgfPlan& p, const ImgvTaps& t, int s_lo,
                                              int n_tot, int stage_px, int h[3]) {
  h[0] = h[1] = h[2] = 0;
  const int row = p.y.off + i;
  if ((unsigned)row >= (unsigned)p.y.src) return;  // a row of the zero border: nothing is loaded
  for (int k0 = 0; k0 < n_tot; k0 += stage_px) {
    const int n_stage = min(stage_px, n_tot - k0);
    src.stage(px, lane, row, s_lo + k0, n_stage);
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    // window sample s sits at px[s + sh]; anything outside [0, n_stage) is the zero border or another chunk
    const int sh = p.x.off - s_lo - k0;
    if (p.linear) {
      const unsigned ka = (unsigned)(t.lo + sh), kb = (unsigned)(t.hi + sh);
      const unsigned va = ka < (unsigned)n_stage ? px[ka] : 0u, vb = kb < (unsigned)n_stage ? px[kb] : 0u;
      h[0] += (int)(va & 255u) * t.w_lo + (int)(vb & 255u) * t.w_hi;
      h[1] += (int)((va >> 8) & 255u) * t.w_lo + (int)((vb >> 8) & 255u) * t.w_hi;
      h[2] += (int)(va >> 16) * t.w_lo + (int)(vb >> 16) * t.w_hi;
    } else {
      const int sa = max(t.lo, -sh), sb = min(t.hi, n_stage - 1 - sh);
      for (int s = sa; s <= sb; ++s) {
        const unsigned v = px[s + sh];
        const int pos = s * p.x.Q;
        const int w = min(pos + p.x.Q, t.c1) - max(pos, t.c0);
        h[0] += (int)(v & 255u) * w, h[1] += (int)((v >> 8) & 255u) * w, h[2] += (int)(v >> 16) * w;
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next chunk, or the next row, overwrites the slice
    __threadfence_block();
  }
}

// dynamic LDS: kImgvWaves slices of Src::slice(args) dwords
template <class Src>
__global__ __launch_bounds__(kImgvCols* kImgvWaves) void imgv_frames_kernel(const typename Src::Args args) {
  const ImgvArgs& a = Src::common(args);
  extern __shared__ __attribute__((aligned(16))) unsigned imgv_lds[];
  const int lane = threadIdx.x & (kImgvCols - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kImgvCols);
  const int fr = blockIdx.z;
  const int oy_lo = blockIdx.y * kImgvRows + wave * kImgvBand, oy_hi = min(oy_lo + kImgvBand, a.dst_h);
  if (oy_lo >= oy_hi) return;  // wave-uniform, and no barrier of the workgroup follows
  unsigned* px = imgv_lds + (size_t)wave * Src::slice(args);

  // the frame's plan
  ImgfPlan p{};
  p.x.off = a.rect[fr][0], p.y.off = a.rect[fr][1], p.x.n = a.rect[fr][2], p.y.n = a.rect[fr][3];
  p.x.src = a.src_w, p.y.src = a.src_h, p.x.dst = a.dst_w, p.y.dst = a.dst_h;
  p.x.P = a.scale_num ? a.scale_num : p.x.n, p.x.Q = a.scale_num ? a.scale_den : p.x.dst;
  p.y.P = a.scale_num ? a.scale_num : p.y.n, p.y.Q = a.scale_num ? a.scale_den : p.y.dst;
  p.channels = a.channels, p.rgba_mode = a.rgba_mode;
  p.bkg[0] = a.bkg[0], p.bkg[1] = a.bkg[1], p.bkg[2] = a.bkg[2];
  p.linear = (p.x.P < p.x.Q || p.y.P < p.y.Q) ? 1 : 0;

  // the tile's span of a row and the lane's taps in it
  const int d0 = blockIdx.x * kImgvCols, d1 = min(d0 + kImgvCols, p.x.dst) - 1, d = d0 + lane;
  int first, last, tmp;
  imgf_span(p.x, p.linear, d0, &first, &tmp);
  imgf_span(p.x, p.linear, d1, &tmp, &last);
  const int s_lo = Src::first_col(max(0, p.x.off + first));
  const int n_tot = max(0, min(p.x.src, p.x.off + last + 1) - s_lo);  // 0: the tile reads the border only
  ImgvTaps t{};
  long long len_x = (long long)p.x.P;  // the divisor's x factor
  if (d <= d1) {
    if (p.linear) {
      int f;
      imgf_linear_taps(p.x, d, &t.lo, &t.hi, &f);
      t.w_lo = p.x.P - f, t.w_hi = f;
    } else {
      t.c0 = d * p.x.P, t.c1 = min(t.c0 + p.x.P, p.x.n * p.x.Q);
      t.lo = t.c0 / p.x.Q, t.hi = (t.c1 + p.x.Q - 1) / p.x.Q - 1;
      len_x = t.c1 - t.c0;
    }
  } else {
    t.lo = 0, t.hi = -1;  // no column: no taps (linear: both weights are 0)
  }

  Src src(args, fr, p, px + a.stage_px);
  unsigned char* out = a.out + ((size_t)fr * a.dst_h * a.dst_w + d) * 3;
  auto finish = [&](int oy, const long long S[3], long long D) {
    if (d > d1) return;
    unsigned char* o = out + (size_t)oy * a.dst_w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned char)imgf_round_div(S[c], D);
  };

  int h[3];
  if (p.linear) {
    int ia = -1, ib = -1, ha[3] = {0, 0, 0}, hb[3] = {0, 0, 0};  // the two rows whose sums are at hand
    for (int oy = oy_lo; oy < oy_hi; ++oy) {
      int s0, s1, f;
      imgf_linear_taps(p.y, oy, &s0, &s1, &f);
      if (s0 != ia) {
        if (s0 == ib) {
          ha[0] = hb[0], ha[1] = hb[1], ha[2] = hb[2];
        } else {
          imgv_row_sums(src, px, lane, s0, p, t, s_lo, n_tot, a.stage_px, ha);
        }
        ia = s0;
      }
      if (s1 == ia) {
        hb[0] = ha[0], hb[1] = ha[1], hb[2] = ha[2];
      } else if (s1 != ib) {
        imgv_row_sums(src, px, lane, s1, p, t, s_lo, n_tot, a.stage_px, hb);
      }
      ib = s1;
      long long S[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) S[c] = (long long)ha[c] * (p.y.P - f) + (long long)hb[c] * f;
      finish(oy, S, (long long)p.x.P * p.y.P);
    }
    return;
  }

  // area rule: window rows from the first one of the band's first cell; row i covers [i Q, (i + 1) Q)
  int oy = oy_lo;
  int c0 = oy * p.y.P, c1 = min(c0 + p.y.P, p.y.n * p.y.Q);
  long long S[3] = {0, 0, 0};
  for (int i = c0 / p.y.Q; oy < oy_hi; ++i) {
    imgv_row_sums(src, px, lane, i, p, t, s_lo, n_tot, a.stage_px, h);
    const int pos = i * p.y.Q;
    while (oy < oy_hi) {
      const int wy = min(pos + p.y.Q, c1) - max(pos, c0);
#pragma unroll
      for (int c = 0; c < 3; ++c) S[c] += (long long)h[c] * wy;
      if (pos + p.y.Q < c1) break;  // the cell goes on in the next row
      finish(oy, S, len_x * (c1 - c0));
      S[0] = S[1] = S[2] = 0;
      ++oy;
      c0 = oy * p.y.P, c1 = min(c0 + p.y.P, p.y.n * p.y.Q);
      if (pos + p.y.Q <= c0) break;  // the row ended with the cell
    }
  }
}
