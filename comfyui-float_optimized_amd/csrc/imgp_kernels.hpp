// Kernel of float_img_paste (include/float_hip.h): the generated 8-bit frames back in the source portrait, in HBM.  One launch,
// no LDS, no scratch, no atomics; integers throughout, bitwise host_models.paste_rgb8.
//   imgp_paste_kernel  Every output frame is a flat stream of N = 3 H W bytes that starts at out + f N (formed in 64 bits; N
//                      itself is below 2^31 at the 16384-px limit).  3 W and N are no multiples of 4 in general, so a frame is cut
//                      where its ADDRESS is dword-aligned: a head of (4 - address) & 3 bytes, whole aligned dwords, a tail of at
//                      most 3 bytes.  A workgroup owns kImgpSpan consecutive dwords of one frame; lane t stores dword
//                      it * 256 + t of them, so a wave's store covers 256 contiguous aligned bytes.  Head and tail are byte stores
//                      by six lanes of the frame's first workgroup.  Byte i of a frame is channel i % 3 of pixel i / 3: the lane
//                      divides once for its first byte and steps (c, x, y) for the other three.  The source is read as one
//                      unaligned dword at the same byte offset i (the copy outside the box: 3 B read, 3 B written per pixel);
//                      inside rect & image the lane evaluates the resize rule of the image front end on the frame - the taps
//                      come straight from global memory, the frame fits L2 - then the feather weight and the blend, once per
//                      pixel and channel.
//                      Block order: frame-major and XCD-affine as in dec_flowlast_kernel - the spans are padded to a multiple of
//                      8 and all frames of a span run back to back on ids congruent mod 8, so a span of the source is fetched
//                      into one L2 once for the whole clip (a speed assumption only).
// Accumulator width, from host_models._area_axis / _linear_axis at the limits of the entry (frame sides <= 1024, box sides <=
// 16384): the scale of an axis is P / Q = frame / box reduced, so P <= 1024 and Q <= 16384.  Area rule (P >= Q on both axes): a
// weight is an overlap length <= Q, a cell's weights sum to its length <= P, so S = sum(v wx wy) <= 255 Px Py <= 255 * 2^20 <
// 2^28 and D = len_x len_y <= 2^20.  Linear rule: the weights of an axis are P - f and f, S <= 255 Px Py and D = Px Py, the same
// bounds.  Positions: d P, (d + 1) P, (sx + 1) Q and n Q are at most 16384 * 1024 = 2^24.  The tie test doubles a remainder < D.
// The feather numerator is 255 (d + 1) <= 255 * 2^14 < 2^22, the blend a face + (255 - a) src + 127 <= 255^2 + 127.  Everything
// fits 32 bits: the only 64-bit values in the kernel are the frame bases and the products of imgp_div below.
//
// Kernel of float_img_paste_i420: the same pasted frames leaving as planar YUV 4:2:0, bitwise host_models.paste_i420.  One launch,
// no LDS, no scratch, no atomics.
//   imgp_paste_i420_kernel  An output frame is 3 H W / 2 bytes at out + f * that (formed in 64 bits): the Y plane H x W, then U and V
//                      at H/2 x W/2.  A lane owns a cell of 2 rows x 4 columns: it forms the eight pasted RGB pixels with imgp_setup /
//                      imgp_face / imgp_blend - the very bytes float_img_paste stores - and from them eight Y samples and the two
//                      2 x 2 chroma blocks of the cell, so a block that straddles the box edge or the feather mixes pasted and
//                      source PIXELS, as the definition does; chroma is never blended.  A workgroup owns 256 consecutive cells in
//                      row-major cell order (block order: frame-major and XCD-affine, as above), so a wave stores 256 contiguous Y
//                      bytes per row.
//                      FAST (W % 4 == 0 and out 4-byte aligned, chosen on the host per launch): every frame, the Y plane and its
//                      rows are dword-aligned and the chroma planes and rows 2-byte aligned (H W / 4 may be odd in dwords, never in
//                      16-bit words), so a lane stores one dword of Y per row, 16 bits of U and 16 bits of V, and reads the source
//                      as three unaligned dwords per row (12 bytes that end inside the row).
//                      Otherwise (W % 4 == 2: rows 2-byte aligned, the last cell of a row has two columns, H W / 4 can be odd and V
//                      then starts at an odd address; or a misaligned out) every load of the source and every store is a byte.
// Accumulator width: the RGB in front of the conversion is the kernel's above, 0 ... 255.  Y = 66 R + 129 G + 25 B + 128 <= 56228
// < 2^16; a chroma mean is (c00 + c01 + c10 + c11 + 2) >> 2 with a sum <= 1022; the U / V numerators lie in [-28432, 28688].  They
// are signed 32-bit ints and >> is the arithmetic shift (floor), as in host_models.rgb8_to_i420.  Cell and pixel indices are below
// H W <= 2^28 and a source offset 3 (y W + x) below 3 * 2^28, in unsigned 32 bits; the frame bases are 64-bit.
#pragma once
#include "common.hpp"

constexpr int kImgpThreads = 256;
constexpr int kImgpIters = 4;                           // dwords per lane
constexpr int kImgpSpan = kImgpThreads * kImgpIters;    // dwords per workgroup

// Every divisor of the kernel is the same for all lanes (Q of an axis, Px Py, feather + 1, the source's width), and every dividend
// is below 2^28, so a division is one 32 x 32 -> 64-bit multiply and a shift (Granlund & Montgomery): with l = ceil(log2 D),
// k = 28 + l and M = floor(2^k / D) + 1, 2^k <= M D <= 2^k + 2^l, hence n / D == (n M) >> k for 0 <= n < 2^28; M <= 2^29 + 1.
struct ImgpDiv {
  unsigned M, k;
};
inline ImgpDiv imgp_make_div(unsigned D) {
  unsigned l = 0;
  while ((1u << l) < D) ++l;
  ImgpDiv d;
  d.k = 28u + l;
  d.M = (unsigned)((1ull << d.k) / D + 1ull);
  return d;
}
__device__ __forceinline__ unsigned imgp_div(unsigned n, const ImgpDiv& d) { return (unsigned)(((unsigned long long)n * d.M) >> d.k); }

struct ImgpAxis {
  ImgpDiv dq;    // / Q
  int P, Q;      // scale P / Q (reduced) = frame extent / box extent: box cell d covers [d P, (d + 1) P) in units of 1 / Q of a sample
  int n;         // extent of the frame
  int off, ext;  // the box in source coordinates: cells off ... off + ext - 1
  int lo, hi;    // box & image: [lo, hi), empty when hi <= lo
  int open_lo, open_hi;  // that side of the box lies strictly inside the image: it feathers
};

struct ImgpPlan {
  ImgpAxis x, y;
  int linear, feather;
  int D;             // Px Py: the divisor of every cell under both rules (box extent * P == frame extent * Q: no cell is clipped)
  ImgpDiv dD, df, dw;  // / D, / (feather + 1), / src_w
  int src_w;
  int n_frames;
  unsigned frame_bytes;  // 3 H W of the source = bytes of an output frame
  unsigned in_bytes;     // 3 h w of a generated frame
  unsigned spans;        // workgroups per frame, a multiple of 8
};

// the launch's plan from the entry's (checked) arguments
inline ImgpPlan imgp_make_plan(int src_h, int src_w, int fr_h, int fr_w, int rect_x, int rect_y, int rect_w, int rect_h, int feather) {
  ImgpPlan p{};
  p.x.n = fr_w, p.x.off = rect_x, p.x.ext = rect_w;
  p.y.n = fr_h, p.y.off = rect_y, p.y.ext = rect_h;
  const int src_ext[2] = {src_w, src_h};
  ImgpAxis* axes[2] = {&p.x, &p.y};
  for (int k = 0; k < 2; ++k) {
    ImgpAxis* a = axes[k];
    int g = a->n, r = a->ext;
    while (r) {  // gcd
      const int t = g % r;
      g = r, r = t;
    }
    a->P = a->n / g, a->Q = a->ext / g;
    a->dq = imgp_make_div((unsigned)a->Q);
    a->lo = std::max(0, a->off), a->hi = std::min(src_ext[k], a->off + a->ext);
    a->open_lo = a->off > 0, a->open_hi = a->off + a->ext < src_ext[k];
  }
  if (p.x.hi <= p.x.lo || p.y.hi <= p.y.lo) p.x.lo = p.x.hi = p.y.lo = p.y.hi = 0;  // the box misses the image: a copy of the source
  p.linear = (p.x.P < p.x.Q || p.y.P < p.y.Q) ? 1 : 0;
  p.feather = feather;
  p.D = p.x.P * p.y.P;
  p.dD = imgp_make_div((unsigned)p.D), p.df = imgp_make_div((unsigned)feather + 1u), p.dw = imgp_make_div((unsigned)src_w);
  p.src_w = src_w;
  p.frame_bytes = 3u * (unsigned)src_h * (unsigned)src_w;  // <= 3 * 2^28
  p.in_bytes = 3u * (unsigned)fr_h * (unsigned)fr_w;
  const unsigned spans = (p.frame_bytes / 4u + kImgpSpan - 1) / kImgpSpan;
  p.spans = std::max(8u, (spans + 7u) & ~7u);
  return p;
}

// S / D rounded half to even (0 <= S <= 255 D, 1 <= D <= 2^20)
__device__ __forceinline__ unsigned imgp_round_div(unsigned S, unsigned D, const ImgpDiv& dD) {
  const unsigned q = imgp_div(S, dD), r2 = 2u * (S - q * D);
  return q + ((r2 > D || (r2 == D && (q & 1u))) ? 1u : 0u);
}

// linear rule: taps (s0, P - f) and (s1, f).  num = (d + 1) P - (sx + 1) Q < P because (sx + 1) Q > d P, so num mod P is num.
__device__ __forceinline__ void imgp_linear_taps(const ImgpAxis& a, int d, int* s0, int* s1, int* f) {
  int sx = (int)imgp_div((unsigned)(d * a.P), a.dq);
  int fr = max((d + 1) * a.P - (sx + 1) * a.Q, 0);
  if (sx >= a.n - 1) sx = a.n - 1, fr = 0;
  *s0 = sx, *s1 = min(sx + 1, a.n - 1), *f = fr;
}

// what one pixel of the box needs, whatever the channel
struct ImgpPixel {
  int inside;  // the pixel lies in box & image
  int alpha;   // 0 ... 255
  // linear: taps x0 / x1 with weights wx0 / wx1, rows y0 / y1 with wy0 / wy1; area: the cell [cx0, cx1) x [cy0, cy1)
  int x0, x1, wx0, wx1, y0, y1, wy0, wy1;
  int cx0, cx1, cy0, cy1;
};

__device__ __forceinline__ void imgp_setup(const ImgpPlan& p, int x, int y, ImgpPixel* px) {
  px->inside = (x >= p.x.lo && x < p.x.hi && y >= p.y.lo && y < p.y.hi) ? 1 : 0;
  if (!px->inside) return;
  const int u = x - p.x.off, v = y - p.y.off;
  int d = 1 << 30;
  if (p.x.open_lo) d = min(d, u);
  if (p.x.open_hi) d = min(d, p.x.ext - 1 - u);
  if (p.y.open_lo) d = min(d, v);
  if (p.y.open_hi) d = min(d, p.y.ext - 1 - v);
  px->alpha = (p.feather == 0 || d >= p.feather) ? 255 : min(255, (int)imgp_div((unsigned)(255 * (d + 1)), p.df));  // d >= feather gives >= 255
  if (p.linear) {
    int f;
    imgp_linear_taps(p.x, u, &px->x0, &px->x1, &f);
    px->wx0 = p.x.P - f, px->wx1 = f;
    imgp_linear_taps(p.y, v, &px->y0, &px->y1, &f);
    px->wy0 = p.y.P - f, px->wy1 = f;
  } else {
    px->cx0 = u * p.x.P, px->cx1 = min(px->cx0 + p.x.P, p.x.n * p.x.Q);
    px->cy0 = v * p.y.P, px->cy1 = min(px->cy0 + p.y.P, p.y.n * p.y.Q);
    px->x0 = (int)imgp_div((unsigned)px->cx0, p.x.dq), px->y0 = (int)imgp_div((unsigned)px->cy0, p.y.dq);  // first tap of the cell on each axis
  }
}

// channel c of the resized frame at a pixel of the box, 0 ... 255
__device__ __forceinline__ unsigned imgp_face(const unsigned char* __restrict__ fr, const ImgpPlan& p, const ImgpPixel& px, int c) {
  const int pitch = p.x.n * 3;
  if (p.linear) {
    const unsigned char* r0 = fr + px.y0 * pitch + c;
    const unsigned char* r1 = fr + px.y1 * pitch + c;
    const unsigned S = ((unsigned)r0[px.x0 * 3] * px.wx0 + (unsigned)r0[px.x1 * 3] * px.wx1) * px.wy0 +
                       ((unsigned)r1[px.x0 * 3] * px.wx0 + (unsigned)r1[px.x1 * 3] * px.wx1) * px.wy1;
    return imgp_round_div(S, (unsigned)p.D, p.dD);
  }
  unsigned S = 0;
  int i = px.y0;
  for (int py = i * p.y.Q; py < px.cy1; py += p.y.Q, ++i) {  // i < n: cy1 <= n Q
    const unsigned wy = (unsigned)(min(py + p.y.Q, px.cy1) - max(py, px.cy0));
    const unsigned char* r = fr + i * pitch + c;
    unsigned row = 0;
    int j = px.x0;
    for (int qx = j * p.x.Q; qx < px.cx1; qx += p.x.Q, ++j) row += (unsigned)r[j * 3] * (unsigned)(min(qx + p.x.Q, px.cx1) - max(qx, px.cx0));
    S += row * wy;
  }
  return imgp_round_div(S, (unsigned)p.D, p.dD);  // (cx1 - cx0) (cy1 - cy0) == Px Py: no cell is clipped
}

__device__ __forceinline__ unsigned imgp_blend(unsigned face, unsigned s, int a) {
  return (a * face + (255 - a) * s + 127u) / 255u;
}

// bytes [i0, i0 + n) of a frame, n <= 4, packed little-endian; sv holds the source's bytes at the same offsets
__device__ __forceinline__ unsigned imgp_bytes(const unsigned char* __restrict__ fr, const ImgpPlan& p, unsigned i0, int n, unsigned sv) {
  const unsigned pix = i0 / 3u;
  int c = (int)(i0 - pix * 3u);
  int y = (int)imgp_div(pix, p.dw), x = (int)(pix - (unsigned)y * (unsigned)p.src_w);
  if (p.x.hi <= p.x.lo || y >= p.y.hi || y + 1 < p.y.lo) return sv;  // four bytes touch at most rows y and y + 1
  ImgpPixel px;
  imgp_setup(p, x, y, &px);
  unsigned v = sv;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < n && px.inside) {
      const unsigned s = (sv >> (8 * k)) & 255u;
      const unsigned o = px.alpha == 0 ? s : imgp_blend(imgp_face(fr, p, px, c), s, px.alpha);
      v = (v & ~(255u << (8 * k))) | (o << (8 * k));
    }
    if (++c == 3 && k < 3) {
      c = 0;
      if (++x == p.src_w) x = 0, ++y;
      imgp_setup(p, x, y, &px);
    }
  }
  return v;
}

__device__ __forceinline__ unsigned imgp_load_u32(const unsigned char* q) {  // any alignment
  unsigned v;
  __builtin_memcpy(&v, q, 4);
  return v;
}

__global__ __launch_bounds__(kImgpThreads) void imgp_paste_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ frames,
                                                                  unsigned char* __restrict__ out, const ImgpPlan p) {
  // block -> (frame, span): all frames of a span back to back on ids congruent mod 8
  const unsigned slot = blockIdx.x >> 3;
  const unsigned f = slot % (unsigned)p.n_frames;
  const unsigned span = (slot / (unsigned)p.n_frames) * 8u + (blockIdx.x & 7u);
  const unsigned N = p.frame_bytes;
  unsigned char* o = out + (size_t)f * N;
  const unsigned char* fr = frames + (size_t)f * p.in_bytes;
  const unsigned head = min(N, (unsigned)((4u - ((unsigned)(uintptr_t)o & 3u)) & 3u));
  const unsigned nd = (N - head) >> 2, tail = N - head - 4u * nd;
  if (span == 0 && threadIdx.x < 6) {  // lanes 0 ... 2: the head, lanes 3 ... 5: the tail
    const unsigned t = threadIdx.x;
    const bool is_head = t < 3;
    const unsigned k = is_head ? t : t - 3;
    if (k < (is_head ? head : tail)) {
      const unsigned i = is_head ? k : head + 4u * nd + k;
      o[i] = (unsigned char)imgp_bytes(fr, p, i, 1, (unsigned)src[i]);
    }
  }
#pragma unroll
  for (int it = 0; it < kImgpIters; ++it) {
    const unsigned k = span * (unsigned)kImgpSpan + (unsigned)(it * kImgpThreads) + threadIdx.x;
    if (k >= nd) break;
    const unsigned i0 = head + 4u * k;  // i0 + 3 < N
    *reinterpret_cast<unsigned*>(o + i0) = imgp_bytes(fr, p, i0, 4, imgp_load_u32(src + i0));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// float_img_paste_i420: the pasted frames as planar YUV 4:2:0
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kImgpCellW = 4;  // a lane's cell: 2 rows x 4 columns = one dword of Y per row, two chroma samples per plane

// what the I420 kernel needs besides the plan (ImgpPlan is the RGB kernel's and stays as it is)
struct ImgpYuv {
  ImgpDiv dcx;       // / cells_x
  unsigned cells_x;  // cells per pair of rows: ceil(W / 4); the last one has two columns when W % 4 == 2
  unsigned cells;    // cells per frame: (H / 2) cells_x <= 2^25
  unsigned spans;    // workgroups per frame, a multiple of 8
  unsigned y_bytes;  // H W
  unsigned c_bytes;  // (H / 2) (W / 2): a frame is y_bytes + 2 c_bytes
};

inline ImgpYuv imgp_make_yuv(int src_h, int src_w) {  // both even
  ImgpYuv q{};
  q.cells_x = ((unsigned)src_w + kImgpCellW - 1) / kImgpCellW;
  q.dcx = imgp_make_div(q.cells_x);
  q.cells = (unsigned)(src_h / 2) * q.cells_x;
  const unsigned spans = (q.cells + kImgpThreads - 1) / kImgpThreads;
  q.spans = std::max(8u, (spans + 7u) & ~7u);
  q.y_bytes = (unsigned)src_h * (unsigned)src_w;
  q.c_bytes = (unsigned)(src_h / 2) * (unsigned)(src_w / 2);
  return q;
}

// The conversion is fh_yuv_plane (common.hpp) on the rows of matrix M (0 / 2 / 4 / 6): host_models.rgb8_to_i420.  M is a template
// parameter here, not a kernel argument as in the decoder's kernels: the FAST instantiation sits at 80 VGPRs, six waves per SIMD,
// and the table in SGPRs cost it the 81st (the compiler keeps coefficients in VGPRs across the cell's loops) and with it a wave;
// folded into the instructions, M = 0 compiles to the registers it had.
template <bool FAST, int M>
__global__ __launch_bounds__(kImgpThreads) void imgp_paste_i420_kernel(const unsigned char* __restrict__ src, const unsigned char* __restrict__ frames,
                                                                       unsigned char* __restrict__ out, const ImgpPlan p, const ImgpYuv q) {
  constexpr FhYuv t = fh_yuv_pack(kFhYuvRows[M >> 1]);
  // block -> (frame, span): all frames of a span back to back on ids congruent mod 8
  const unsigned slot = blockIdx.x >> 3;
  const unsigned f = slot % (unsigned)p.n_frames;
  const unsigned span = (slot / (unsigned)p.n_frames) * 8u + (blockIdx.x & 7u);
  const unsigned k = span * (unsigned)kImgpThreads + threadIdx.x;
  if (k >= q.cells) return;
  const unsigned cy = imgp_div(k, q.dcx), cx = k - cy * q.cells_x;
  const unsigned W = (unsigned)p.src_w, x0 = cx * kImgpCellW, y0 = 2u * cy;
  const int ncol = FAST ? kImgpCellW : min(kImgpCellW, (int)(W - x0));  // 4, or 2 in the last cell of a row with W % 4 == 2
  const unsigned char* fr = frames + (size_t)f * p.in_bytes;
  unsigned char* o = out + (size_t)f * ((size_t)q.y_bytes + 2u * (size_t)q.c_bytes);
  unsigned m[3] = {0u, 0u, 0u};  // per channel: the sum of the cell's left 2 x 2 block in bits 0 ... 15, of its right one in 16 ... 31 (<= 1020 each)
  for (int r = 0; r < 2; ++r) {
    const unsigned row = (y0 + (unsigned)r) * W + x0;  // pixel index of the row's first sample, < 2^28
    const unsigned char* s = src + 3u * row;
    unsigned a, b, c;  // the row's 3 ncol source bytes, little-endian
    if (FAST) {
      a = imgp_load_u32(s), b = imgp_load_u32(s + 4), c = imgp_load_u32(s + 8);
    } else {
      unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 3 * kImgpCellW; ++i)
        if (i < 3 * ncol) w[i >> 2] |= (unsigned)s[i] << (8 * (i & 3));
      a = w[0], b = w[1], c = w[2];
    }
    unsigned yw = 0;
    for (int col = 0; col < ncol; ++col) {
      unsigned rgb[3] = {a & 255u, (a >> 8) & 255u, (a >> 16) & 255u};
      a = (a >> 24) | (b << 8), b = (b >> 24) | (c << 8), c >>= 24;  // the next pixel's bytes move down
      ImgpPixel px;
      imgp_setup(p, (int)x0 + col, (int)y0 + r, &px);
      if (px.inside && px.alpha != 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb[ch] = imgp_blend(imgp_face(fr, p, px, ch), rgb[ch], px.alpha);
      }
      yw |= fh_yuv_plane(t, 0, (int)rgb[0], (int)rgb[1], (int)rgb[2]) << (8 * col);
      const int sh = 16 * (col >> 1);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) m[ch] += rgb[ch] << sh;
    }
    unsigned char* yo = o + row;
    if (FAST) {
      *reinterpret_cast<unsigned*>(yo) = yw;  // out, y_bytes + 2 c_bytes and W are multiples of 4
    } else {
      for (int col = 0; col < ncol; ++col) yo[col] = (unsigned char)(yw >> (8 * col));
    }
  }
  unsigned uv[2];  // U | V << 8 of the left and the right block
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    const int mr = (int)(((m[0] >> (16 * blk)) & 0xffffu) + 2u) >> 2, mg = (int)(((m[1] >> (16 * blk)) & 0xffffu) + 2u) >> 2,
              mb = (int)(((m[2] >> (16 * blk)) & 0xffffu) + 2u) >> 2;
    uv[blk] = fh_yuv_plane(t, 1, mr, mg, mb) | (fh_yuv_plane(t, 2, mr, mg, mb) << 8);
  }
  const unsigned at = cy * (W >> 1) + (x0 >> 1);  // < c_bytes
  unsigned char* uo = o + q.y_bytes + at;
  unsigned char* vo = uo + q.c_bytes;
  if (FAST) {  // W / 2 and x0 / 2 are even, c_bytes is even: 2-byte aligned
    *reinterpret_cast<unsigned short*>(uo) = (unsigned short)((uv[0] & 255u) | ((uv[1] & 255u) << 8));
    *reinterpret_cast<unsigned short*>(vo) = (unsigned short)((uv[0] >> 8) | (uv[1] & 0xff00u));
  } else {
    uo[0] = (unsigned char)uv[0], vo[0] = (unsigned char)(uv[0] >> 8);
    if (ncol == kImgpCellW) uo[1] = (unsigned char)uv[1], vo[1] = (unsigned char)(uv[1] >> 8);
  }
}
