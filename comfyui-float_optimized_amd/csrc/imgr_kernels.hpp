// Kernels of float_img_resample (include/float_hip.h): bicubic / Lanczos resampling of 8-bit RGB frames in HBM by Pillow's
// fixed-point rule, bitwise host_models.resample_rgb8.  Two launches, no LDS, no atomics, no float: the filter was evaluated on the
// host (float_img_resample_plan) and arrives as a table of int32 per output index of an axis,
//     row i of a table:  xmin, n, k[0 ... ksize - 1]        (2 + ksize ints; k[x] = 0 for x >= n)
// and one sample of a pass is clamp((2^21 + sum_{x < n} k[x] in[xmin + x]) >> 22, 0, 255) with >> the arithmetic shift.
//   imgr_horizontal_kernel  grid (cells of a row / 128, rows, frames).  A lane forms a cell of four neighbouring output pixels of
//                      one row, 12 bytes: per pixel it reads that pixel's table row once - xmin, n and each k[x] serve all three
//                      channels - and the n input pixels as bytes.  Neighbouring lanes read overlapping taps of one input row;
//                      they come from L1/L2.
//   imgr_vertical_kernel    grid (cells of a row / 128, output rows, frames).  The output row is the block's y index, so its table
//                      row is the same for every lane: the compiler reads it with scalar loads, once per wave.  A lane reads 12
//                      bytes of each of the n input rows (three dwords of any alignment where the 12 bytes lie inside the row,
//                      else bytes) and forms the same four pixels of the output row.  tab == nullptr is the copy (n = 1, k =
//                      2^22, row y): what is left when both axes keep their size.
//   FAST (chosen on the host per launch): the destination's base, row pitch and frame pitch are multiples of 4 and every cell may
//                      store 12 bytes, so a lane stores three dwords and a wave 768 contiguous bytes.  The intermediate between
//                      the passes is laid out for it (rows padded to whole cells; the padding is stored as zeros and never
//                      leaves).  Otherwise - `out` with a width that is no multiple of 4, or misaligned - a lane stores its
//                      3 * columns bytes one by one.  The bytes stored are the same.
// Accumulator width: float_img_resample_plan refuses a table row with 255 sum|k| + 2^21 >= 2^31 (none occurs: sum|k| stays near
// 2^22 times the filter's L1 norm, below 1.5), so every partial sum fits int32 in any order.  Offsets inside a frame are below
// 3 * 2^28 (sides <= 16384) and are formed in 32 bits; frame bases and table rows are formed in 64 bits.
#pragma once
#include "common.hpp"

constexpr int kImgrThreads = 128;
constexpr int kImgrCellW = 4;    // pixels per lane: 12 bytes, three dwords
constexpr int kImgrBits = 22;    // coefficients are in units of 2^-22
constexpr int kImgrMaxKsize = 255;
constexpr int kImgrMaxSide = 16384;

struct ImgrPass {
  long long in_frame;   // bytes between input frames
  long long out_frame;  // bytes between output frames
  unsigned in_off;      // byte offset, inside a frame, of the first sample the pass reads (its first row and column)
  unsigned in_pitch;    // bytes per input row
  unsigned out_pitch;   // bytes per output row
  int in_first;         // vertical pass: the input row that sits at in_off (a table holds rows of the whole frame)
  int in_cols;          // vertical pass: columns from in_off on that may be read in every row
  int width;            // output columns
  int cells_x;          // ceil(width / 4)
  int ksize;            // a table row is 2 + ksize ints
};

__device__ __forceinline__ unsigned imgr_load_u32(const unsigned char* q) {  // any alignment
  unsigned v;
  __builtin_memcpy(&v, q, 4);
  return v;
}

// clamp((a >> 22), 0, 255), written as a clamp of the sum followed by the shift of a non-negative value.  The direct form is
// matched by the compiler to v_ashr_pk_u8_i32 (two clamped shifts packed into 16 bits), and the bytes this kernel then assembled
// from its result carried bits of the destination register's earlier content in their upper half (seen on the MI355X with 1 x 1
// frames, where every sample is a known constant); this form compiles to v_med3_i32 and v_lshrrev_b32.
__device__ __forceinline__ unsigned imgr_clip8(int a) {
  return (unsigned)min(max(a, 0), (255 << kImgrBits) | ((1 << kImgrBits) - 1)) >> kImgrBits;
}

// the 3 * ncol bytes of a cell, packed little-endian in v[0 ... 2]
template <bool FAST>
__device__ __forceinline__ void imgr_store(unsigned char* o, const unsigned* v, int ncol) {
  if (FAST) {
    unsigned* d = reinterpret_cast<unsigned*>(o);
    d[0] = v[0], d[1] = v[1], d[2] = v[2];
  } else {
#pragma unroll
    for (int b = 0; b < 3 * kImgrCellW; ++b)
      if (b < 3 * ncol) o[b] = (unsigned char)(v[b >> 2] >> (8 * (b & 3)));
  }
}

template <bool FAST>
__global__ __launch_bounds__(kImgrThreads) void imgr_horizontal_kernel(const unsigned char* __restrict__ in, const int* __restrict__ tab,
                                                                       unsigned char* __restrict__ out, const ImgrPass p) {
  const int cx = (int)(blockIdx.x * kImgrThreads + threadIdx.x);
  if (cx >= p.cells_x) return;
  const unsigned r = blockIdx.y;
  const unsigned char* row = in + (size_t)blockIdx.z * (size_t)p.in_frame + p.in_off + (size_t)r * p.in_pitch;
  unsigned char* o = out + (size_t)blockIdx.z * (size_t)p.out_frame + (size_t)r * p.out_pitch + 3u * kImgrCellW * (unsigned)cx;
  const int x0 = cx * kImgrCellW;
  unsigned v[3] = {0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < kImgrCellW; ++i) {
    if (x0 + i < p.width) {
      const int* t = tab + (size_t)(x0 + i) * (size_t)(2 + p.ksize);
      const int n = t[1];
      const unsigned char* s = row + 3 * t[0];
      int a0 = 1 << (kImgrBits - 1), a1 = a0, a2 = a0;
      for (int j = 0; j < n; ++j) {
        const int k = t[2 + j];
        a0 += k * (int)s[3 * j], a1 += k * (int)s[3 * j + 1], a2 += k * (int)s[3 * j + 2];
      }
      const unsigned px[3] = {imgr_clip8(a0), imgr_clip8(a1), imgr_clip8(a2)};
#pragma unroll
      for (int c = 0; c < 3; ++c) v[(3 * i + c) >> 2] |= px[c] << (8 * ((3 * i + c) & 3));
    }
  }
  imgr_store<FAST>(o, v, min(kImgrCellW, p.width - x0));
}

template <bool FAST>
__global__ __launch_bounds__(kImgrThreads) void imgr_vertical_kernel(const unsigned char* __restrict__ in, const int* __restrict__ tab,
                                                                     unsigned char* __restrict__ out, const ImgrPass p) {
  const int cx = (int)(blockIdx.x * kImgrThreads + threadIdx.x);
  if (cx >= p.cells_x) return;
  const unsigned y = blockIdx.y;
  const int* t = tab ? tab + (size_t)y * (size_t)(2 + p.ksize) : nullptr;  // the same for every lane
  const int first = t ? t[0] - p.in_first : (int)y;
  const int n = t ? t[1] : 1;
  const int x0 = cx * kImgrCellW;
  const int ncol = min(kImgrCellW, p.width - x0);
  const bool whole = x0 + kImgrCellW <= p.in_cols;  // 12 bytes from here lie inside every input row
  const unsigned char* s = in + (size_t)blockIdx.z * (size_t)p.in_frame + p.in_off + (size_t)first * p.in_pitch + 3u * kImgrCellW * (unsigned)cx;
  int acc[3 * kImgrCellW];
#pragma unroll
  for (int b = 0; b < 3 * kImgrCellW; ++b) acc[b] = 1 << (kImgrBits - 1);
  for (int j = 0; j < n; ++j, s += p.in_pitch) {
    const int k = t ? t[2 + j] : 1 << kImgrBits;
    unsigned w[3] = {0u, 0u, 0u};
    if (whole) {
      w[0] = imgr_load_u32(s), w[1] = imgr_load_u32(s + 4), w[2] = imgr_load_u32(s + 8);
    } else {
#pragma unroll
      for (int b = 0; b < 3 * kImgrCellW; ++b)
        if (b < 3 * ncol) w[b >> 2] |= (unsigned)s[b] << (8 * (b & 3));
    }
#pragma unroll
    for (int b = 0; b < 3 * kImgrCellW; ++b) acc[b] += k * (int)((w[b >> 2] >> (8 * (b & 3))) & 255u);
  }
  unsigned v[3] = {0u, 0u, 0u};
#pragma unroll
  for (int b = 0; b < 3 * kImgrCellW; ++b) v[b >> 2] |= imgr_clip8(acc[b]) << (8 * (b & 3));
  unsigned char* o = out + (size_t)blockIdx.z * (size_t)p.out_frame + (size_t)y * p.out_pitch + 3u * kImgrCellW * (unsigned)cx;
  imgr_store<FAST>(o, v, ncol);
}
