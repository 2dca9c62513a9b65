// Kernels of float_jpg_encode (include/float_hip.h): baseline JPEG files (4:2:0, one interleaved scan, the standard Huffman tables)
// from 8-bit RGB frames in HBM.  All of it is integer arithmetic and bitwise the definition host_models.jpeg_encode_rgb8.  Three
// launches per group of kJpgGroup frames:
//   jpg_code_kernel     grid (restart intervals, frames of the group), 256 threads: one workgroup codes one restart interval,
//                       kJpgChunkMcus MCUs at a time.  Per pass: (1) a lane converts 2 x 2 pixels (three 2-byte loads per row) to
//                       Y / Cb / Cr, subsamples the chroma and stores level-shifted int16 samples per 8 x 8 block in LDS; (2) a lane
//                       per (block, column) runs DCT pass 1 in place, (3) a lane per (block, row) pass 2 and the quantiser (an
//                       integer division by 8 q) and stores the coefficients in zigzag order; (4) one lane per block adds up the
//                       block's bits - the DC predictor is the previous block of the component, across passes the one kept in LDS -
//                       and a workgroup scan gives every block its bit offset; (5) every lane ORs its codes into an LDS bit
//                       buffer (ds_or_b32: neighbouring blocks share words); (6) the whole bytes of the buffer are stuffed (a lane
//                       per run of bytes counts its 0xFF, a second scan places it) and appended to the interval's slot in `work`;
//                       the bits of the last, incomplete byte open the next pass's buffer.  The last pass pads with 1-bits.
//                       Blocks are kJpgBlkStride = 66 int16 apart, so the one-lane-per-block walks hit 64 different banks.
//                       With restart = 0 a frame is ONE interval, hence one workgroup walking the frame pass by pass: supported
//                       for completeness, not meant to be fast.
//   jpg_offsets_kernel  one workgroup: exclusive scan over the group's interval lengths plus header, RSTk markers and EOI -> the
//                       files' offsets (continuing from the previous group's last one) and every interval's place in `out`.
//   jpg_pack_kernel     grid as jpg_code_kernel: header (first interval) or RSTk, the interval's bytes, EOI (last interval) into
//                       `out`; a byte at or beyond out_cap is not written.
// jpg_code_kernel<PAD>: <false> is the kernel of frames made of whole MCUs at an even address, stage (1) as stated.  <true>
// (float_jpg_encode_padded, any sides from 1 x 1 on, any address) differs in stage (1) ONLY: the MCU grid is ceil(h / 16) x
// ceil(w / 16) and a lane's four pixels sit at rows min(py + dy, h - 1) and columns min(px + dx, w - 1) - the last row and column
// replicated into the partial MCUs, on RGB, in front of the conversion - read with single-byte loads, since 3 w and 3 h w may be
// odd.  No read leaves a frame's h w 3 bytes.  Stages (2) - (6) and the two other kernels see whole MCUs either way.
// The Huffman code tables, the quantiser tables and the header bytes are built on the host inside the call and reach the kernels
// as KERNEL ARGUMENTS (JpgTables, 2432 bytes; JpgHeader, 644 bytes): no device table, no copy.  wave64 throughout.
#pragma once
#include "common.hpp"

constexpr int kJpgThreads = 256;
constexpr int kJpgGroup = 16;                                  // frames coded per group: what bounds `work`
constexpr int kJpgChunkMcus = 16;                              // MCUs of one pass
constexpr int kJpgChunkBlocks = kJpgChunkMcus * 6;             // 96: at most one lane per block in the coding steps
constexpr int kJpgBlkStride = 66;                              // int16 per block in LDS (64 + 2: 33 dwords, bank-conflict free)
constexpr int kJpgBlockBytes = 208;                            // bound of a block's code: 64 coefficients x 26 bits (DC 9 + 11, AC 16 + 10)
constexpr int kJpgBitWords = kJpgChunkBlocks * kJpgBlockBytes / 4 + 2;  // a pass's bits, the carried byte and one word of spill
constexpr int kJpgHeaderMax = 640;                             // SOI ... SOS is 623 bytes, 629 with DRI

struct JpgTables {
  uint32_t dc[2][16];   // [luma, chroma][category] = code << 8 | length
  uint32_t ac[2][256];  // [luma, chroma][run << 4 | category]
  uint16_t q[2][64];    // quantiser steps, row-major
};
struct JpgHeader {
  uint8_t bytes[kJpgHeaderMax];
  int len;
};
struct JpgPlan {
  int h, w, mcw;        // frame sides, MCUs per row
  int nmcu, span, n_int;  // MCUs per frame, MCUs per restart interval, intervals per frame
  int frame0, frames;   // the group: frames [frame0, frame0 + frames) of the call
  int hdr_len;
  unsigned long long slot_bytes;
};

__device__ const unsigned char kJpgNatToZz[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                                  41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                                  46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// rint(2^14 A), A the orthonormal 8-point DCT-II matrix; indices are compile-time constants after unrolling
__device__ __forceinline__ constexpr int jpg_m(int k, int n) {
  constexpr int M[8][8] = {{5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793},       {8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035},
                           {7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568},   {6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811},
                           {5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793},   {4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551},
                           {3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135},   {1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598}};
  return M[k][n];
}

// Exclusive scan of one int per thread over the 256 threads of a workgroup; *total = the sum.  s_w: 4 ints of LDS.
__device__ __forceinline__ int jpg_wg_scan(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < kJpgThreads / 64; ++i) {
    const int t = s_w[i];
    if (i < wave) base += t;
    sum += t;
  }
  __syncthreads();  // s_w may be written again
  *total = sum;
  return base + inc - v;
}

// OR the n (1 ... 32) low bits of v into the bit stream at bit p (big-endian within the words), p += n
__device__ __forceinline__ void jpg_put(uint32_t* bits, uint32_t& p, uint32_t v, int n) {
  const uint32_t w = p >> 5, o = p & 31;
  const unsigned long long x = (unsigned long long)v << (64 - (int)o - n);
  atomicOr(&bits[w], (uint32_t)(x >> 32));
  if ((uint32_t)x) atomicOr(&bits[w + 1], (uint32_t)x);
  p += n;
}

__device__ __forceinline__ int jpg_category(int v) { return 32 - __clz(v < 0 ? -v : v); }  // 0 for 0
__device__ __forceinline__ uint32_t jpg_amplitude(int v, int cat) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u); }

// One block's codes: EMIT = false adds up the bits (returned), EMIT = true ORs them into `bits` from bit p on.
template <bool EMIT>
__device__ __forceinline__ int jpg_block(const int16_t* c, int prev_dc, const uint32_t* dc_tab, const uint32_t* ac_tab, uint32_t* bits, uint32_t p) {
  int len = 0;
  const int diff = (int)c[0] - prev_dc;
  {
    const int cat = jpg_category(diff);
    const uint32_t e = dc_tab[cat];
    if constexpr (EMIT) jpg_put(bits, p, ((e >> 8) << cat) | jpg_amplitude(diff, cat), (int)(e & 255u) + cat);
    else len += (int)(e & 255u) + cat;
  }
  const uint32_t zrl = ac_tab[0xF0], eob = ac_tab[0];
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = c[k];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {
      if constexpr (EMIT) jpg_put(bits, p, zrl >> 8, (int)(zrl & 255u));
      else len += (int)(zrl & 255u);
      run -= 16;
    }
    const int cat = jpg_category(v);
    const uint32_t e = ac_tab[(run << 4) | cat];
    if constexpr (EMIT) jpg_put(bits, p, ((e >> 8) << cat) | jpg_amplitude(v, cat), (int)(e & 255u) + cat);
    else len += (int)(e & 255u) + cat;
    run = 0;
  }
  if (run > 0) {
    if constexpr (EMIT) jpg_put(bits, p, eob >> 8, (int)(eob & 255u));
    else len += (int)(eob & 255u);
  }
  return len;
}

// PAD = false: both sides are multiples of 16 and rgb is 2-byte aligned.  PAD = true: any sides and any address; p.mcw and p.nmcu
// count the partial MCUs too.
template <bool PAD>
__global__ __launch_bounds__(kJpgThreads) void jpg_code_kernel(const uint8_t* __restrict__ rgb, JpgPlan p, JpgTables tb, int* __restrict__ lens,
                                                               uint8_t* __restrict__ slots) {
  __shared__ int16_t s_smp[kJpgChunkBlocks * kJpgBlkStride];   // samples, then pass 1's result, per block row-major
  __shared__ int16_t s_coef[kJpgChunkBlocks * kJpgBlkStride];  // quantised coefficients per block in zigzag order
  __shared__ uint32_t s_bits[kJpgBitWords];
  __shared__ uint32_t s_tab[sizeof(JpgTables) / 4];
  __shared__ int s_w[kJpgThreads / 64];
  __shared__ int s_pred[3];
  const int tid = threadIdx.x;
  const int iv = blockIdx.x, fr = blockIdx.y;
  const uint32_t* tbw = reinterpret_cast<const uint32_t*>(&tb);
  for (int i = tid; i < (int)(sizeof(JpgTables) / 4); i += kJpgThreads) s_tab[i] = tbw[i];
  if (tid < 3) s_pred[tid] = 0;
  const uint32_t* s_dc = s_tab;                                      // [2][16]
  const uint32_t* s_ac = s_tab + 32;                                 // [2][256]
  const uint16_t* s_q = reinterpret_cast<const uint16_t*>(s_tab + 32 + 512);  // [2][64]

  const int first = iv * p.span;
  const int count = min(p.span, p.nmcu - first);
  const uint8_t* img = rgb + (size_t)(p.frame0 + fr) * ((size_t)p.h * p.w * 3);
  uint8_t* slot = slots + ((size_t)fr * p.n_int + iv) * p.slot_bytes;
  uint32_t carry_bits = 0, carry_byte = 0;
  size_t outpos = 0;
  __syncthreads();

  for (int m0 = 0; m0 < count; m0 += kJpgChunkMcus) {
    const int nm = min(kJpgChunkMcus, count - m0);
    const int nblk = nm * 6;
    const bool last = m0 + nm >= count;
    // (1) colour conversion and chroma subsampling: one lane per 2 x 2 pixels
    for (int q = tid; q < nm * 64; q += kJpgThreads) {
      const int m = q >> 6, qy = (q >> 3) & 7, qx = q & 7;
      const int g = first + m0 + m;
      const int py = (g / p.mcw) * 16 + 2 * qy, px = (g % p.mcw) * 16 + 2 * qx;
      int cb = 2, cr = 2;
      int16_t* yb = s_smp + (m * 6 + (qy >> 2) * 2 + (qx >> 2)) * kJpgBlkStride + ((2 * qy) & 7) * 8 + ((2 * qx) & 7);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        int r0, g0, b0, r1, g1, b1;
        if constexpr (!PAD) {
          const unsigned short* s = reinterpret_cast<const unsigned short*>(img + ((size_t)(py + dy) * p.w + px) * 3);
          const unsigned a = s[0], b = s[1], c = s[2];
          r0 = a & 255, g0 = a >> 8, b0 = b & 255, r1 = b >> 8, g1 = c & 255, b1 = c >> 8;
        } else {  // the last row and column fill the partial MCUs; 3 w and 3 h w may be odd: byte loads
          const uint8_t* row = img + (size_t)min(py + dy, p.h - 1) * p.w * 3;
          const uint8_t *s0 = row + (size_t)min(px, p.w - 1) * 3, *s1 = row + (size_t)min(px + 1, p.w - 1) * 3;
          r0 = s0[0], g0 = s0[1], b0 = s0[2], r1 = s1[0], g1 = s1[1], b1 = s1[2];
        }
        yb[dy * 8] = (int16_t)(((19595 * r0 + 38470 * g0 + 7471 * b0 + 32768) >> 16) - 128);
        yb[dy * 8 + 1] = (int16_t)(((19595 * r1 + 38470 * g1 + 7471 * b1 + 32768) >> 16) - 128);
        cb += ((-11059 * r0 - 21709 * g0 + 32768 * b0 + (128 << 16) + 32767) >> 16) + ((-11059 * r1 - 21709 * g1 + 32768 * b1 + (128 << 16) + 32767) >> 16);
        cr += ((32768 * r0 - 27439 * g0 - 5329 * b0 + (128 << 16) + 32767) >> 16) + ((32768 * r1 - 27439 * g1 - 5329 * b1 + (128 << 16) + 32767) >> 16);
      }
      s_smp[(m * 6 + 4) * kJpgBlkStride + qy * 8 + qx] = (int16_t)((cb >> 2) - 128);
      s_smp[(m * 6 + 5) * kJpgBlkStride + qy * 8 + qx] = (int16_t)((cr >> 2) - 128);
    }
    __syncthreads();
    // (2) DCT pass 1 down the columns, in place: t = (M X + 2^10) >> 11, |t| < 2^13
    for (int it = tid; it < nblk * 8; it += kJpgThreads) {
      int16_t* col = s_smp + (it >> 3) * kJpgBlkStride + (it & 7);
      int x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = col[j * 8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        int acc = 1 << 10;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += jpg_m(k, j) * x[j];
        col[k * 8] = (int16_t)(acc >> 11);
      }
    }
    __syncthreads();
    // (3) pass 2 along the rows, F8 = (t M^T + 2^13) >> 14, and the quantiser c = sign(F8) ((|F8| + 4 q) / (8 q))
    for (int it = tid; it < nblk * 8; it += kJpgThreads) {
      const int b = it >> 3, k = it & 7;
      const int16_t* row = s_smp + b * kJpgBlkStride + k * 8;
      const uint16_t* q = s_q + ((b % 6) >= 4 ? 64 : 0) + k * 8;
      int16_t* dst = s_coef + b * kJpgBlkStride;
      int t[8];
#pragma unroll
      for (int n = 0; n < 8; ++n) t[n] = row[n];
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        int acc = 1 << 13;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc += t[n] * jpg_m(l, n);
        const int f8 = acc >> 14;
        const unsigned qq = q[l];
        const int mag = (int)(((unsigned)(f8 < 0 ? -f8 : f8) + 4u * qq) / (8u * qq));
        dst[kJpgNatToZz[k * 8 + l]] = (int16_t)(f8 < 0 ? -mag : mag);
      }
    }
    __syncthreads();
    // (4) bits per block and their offsets
    const int j = tid % 6, tsel = j >= 4 ? 1 : 0;
    const int16_t* mine = s_coef + (tid < nblk ? tid : 0) * kJpgBlkStride;
    int prev = 0;
    if (tid < nblk) {
      if (j >= 1 && j <= 3) prev = mine[-kJpgBlkStride];
      else if (j == 0) prev = tid >= 6 ? mine[-3 * kJpgBlkStride] : s_pred[0];
      else prev = tid >= 6 ? mine[-6 * kJpgBlkStride] : s_pred[j - 3];
    }
    const int len = tid < nblk ? jpg_block<false>(mine, prev, s_dc + tsel * 16, s_ac + tsel * 256, nullptr, 0) : 0;
    int sum;
    const int off = jpg_wg_scan(len, s_w, &sum);
    const uint32_t total_bits = carry_bits + (uint32_t)sum;
    // (5) the bit buffer: zeroed but for the bits carried over, then every block's codes
    for (uint32_t i = 1 + tid; i <= (total_bits >> 5) + 1; i += kJpgThreads) s_bits[i] = 0;
    if (tid == 0) s_bits[0] = carry_byte << 24;
    __syncthreads();
    if (tid < nblk) jpg_block<true>(mine, prev, s_dc + tsel * 16, s_ac + tsel * 256, s_bits, carry_bits + (uint32_t)off);
    const uint32_t pad = last ? (0u - total_bits) & 7u : 0u;
    if (tid == 0 && pad) {
      uint32_t pp = total_bits;
      jpg_put(s_bits, pp, (1u << pad) - 1u, (int)pad);
    }
    __syncthreads();
    // (6) byte stuffing into the slot
    const int nbytes = (int)((total_bits + pad) >> 3);
    const int per = (nbytes + kJpgThreads - 1) / kJpgThreads;
    const int a = min(tid * per, nbytes), e = min(a + per, nbytes);
    int ff = 0;
    for (int i = a; i < e; ++i) ff += ((s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u;
    int ff_total;
    const int ff_before = jpg_wg_scan(ff, s_w, &ff_total);
    uint8_t* o = slot + outpos + a + ff_before;
    for (int i = a; i < e; ++i) {
      const uint32_t v = (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
      *o++ = (uint8_t)v;
      if (v == 255u) *o++ = 0;
    }
    outpos += (size_t)nbytes + ff_total;
    carry_bits = (total_bits + pad) & 7u;
    carry_byte = carry_bits ? (s_bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u : 0u;
    if (tid == 0) {
      s_pred[0] = s_coef[(nblk - 3) * kJpgBlkStride];
      s_pred[1] = s_coef[(nblk - 2) * kJpgBlkStride];
      s_pred[2] = s_coef[(nblk - 1) * kJpgBlkStride];
    }
    __syncthreads();  // s_bits, s_coef and s_pred are read before the next pass writes them
  }
  if (tid == 0) lens[fr * p.n_int + iv] = (int)outpos;
}

// what interval `iv` of a frame adds to the file: the header or a restart marker in front, its bytes, EOI behind the last one
__device__ __forceinline__ long long jpg_piece(const JpgPlan& p, int iv, int len) {
  return (long long)len + (iv == 0 ? p.hdr_len : 2) + (iv == p.n_int - 1 ? 2 : 0);
}

__global__ __launch_bounds__(kJpgThreads) void jpg_offsets_kernel(JpgPlan p, const int* __restrict__ lens, long long* __restrict__ dst,
                                                                  long long* __restrict__ offsets) {
  __shared__ long long s_sum[kJpgThreads];
  const int tid = threadIdx.x;
  const int items = p.frames * p.n_int;
  const int per = (items + kJpgThreads - 1) / kJpgThreads;
  const int a = min(tid * per, items), e = min(a + per, items);
  const long long base = p.frame0 == 0 ? 0 : offsets[p.frame0];  // the previous group's launch wrote it
  long long sum = 0;
  for (int i = a; i < e; ++i) sum += jpg_piece(p, i % p.n_int, lens[i]);
  s_sum[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    long long run = base;
    for (int i = 0; i < kJpgThreads; ++i) {
      const long long t = s_sum[i];
      s_sum[i] = run;
      run += t;
    }
    offsets[p.frame0 + p.frames] = run;
  }
  __syncthreads();
  long long run = s_sum[tid];
  for (int i = a; i < e; ++i) {
    const int iv = i % p.n_int;
    if (iv == 0) offsets[p.frame0 + i / p.n_int] = run;
    dst[i] = run + (iv == 0 ? p.hdr_len : 2);
    run += jpg_piece(p, iv, lens[i]);
  }
}

__global__ __launch_bounds__(kJpgThreads) void jpg_pack_kernel(JpgPlan p, JpgHeader hd, const int* __restrict__ lens, const long long* __restrict__ dst,
                                                               const uint8_t* __restrict__ slots, uint8_t* __restrict__ out, unsigned long long out_cap) {
  const int tid = threadIdx.x;
  const int iv = blockIdx.x, fr = blockIdx.y;
  const int item = fr * p.n_int + iv;
  const int len = lens[item];
  const unsigned long long at = (unsigned long long)dst[item];
  const uint8_t* slot = slots + (size_t)item * p.slot_bytes;
  if (iv == 0) {
    for (int i = tid; i < p.hdr_len; i += kJpgThreads)
      if (at - p.hdr_len + i < out_cap) out[at - p.hdr_len + i] = hd.bytes[i];
  } else if (tid < 2) {
    if (at - 2 + tid < out_cap) out[at - 2 + tid] = tid == 0 ? (uint8_t)0xFF : (uint8_t)(0xD0 + ((iv - 1) & 7));
  }
  for (int i = tid; i < len; i += kJpgThreads)
    if (at + i < out_cap) out[at + i] = slot[i];
  if (iv == p.n_int - 1 && tid < 2) {
    if (at + len + tid < out_cap) out[at + len + tid] = tid == 0 ? (uint8_t)0xFF : (uint8_t)0xD9;
  }
}
