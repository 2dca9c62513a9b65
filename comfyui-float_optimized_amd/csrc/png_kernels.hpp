// Kernels of float_png_encode (include/float_hip.h): lossless PNG files (8 bits, colour type 2, one IDAT) from 8-bit RGB frames in
// HBM.  All of it is integer arithmetic and bitwise the definition host_models.png_encode_rgb8.  A frame's filtered scanlines
// are cut into bands of `band` rows; a band is one dynamic-Huffman deflate block of literals in one of 8 fixed code tables
// followed by an empty stored block (a sync flush), so the bands are independent, byte-aligned pieces.  Three launches per
// group of kPngGroup frames:
//   png_code_kernel     grid (bands, frames of the group), 256 threads: one workgroup codes one band.  (1) A wave per row adds up
//                       the five filters' costs, sum of min(v, 256 - v), lane-parallel over the row's bytes, reduces them
//                       across its lanes and takes the cheapest (ties: the smallest type); it then counts the row's filtered
//                       bytes into its OWN 256-bin histogram in LDS (ds_add_u32; one histogram per wave keeps a run of equal
//                       residuals from serialising four waves on one address).  (2) A lane per byte value prices the 8 tables,
//                       bits(k) = sum of hist[v] T_k[v]; the cheapest goes to LDS.  (3) The band is coded kPngChunk bytes at a
//                       time: the filtered bytes are staged in LDS (a lane per byte, the filter recomputed from the raw
//                       neighbours), a lane takes 16 consecutive bytes, adds up their code lengths, a workgroup scan gives its
//                       bit position, and it ORs its codes into an LDS bit buffer a dword at a time (ds_or_b32: neighbouring
//                       lanes share the first and the last word).  The whole bytes go to the band's slot in `work`; the bits of
//                       the last, incomplete byte open the next pass's buffer.  The first pass starts behind the 1106-bit block
//                       header, the last one appends end-of-block and the flush.  Along the way: the band's Adler pair (the sum
//                       of its bytes, and the sum weighted by the distance to the band's end, both mod 65521) and the CRC-32
//                       of its coded bytes - a lane's run by the byte table, runs and passes joined by png_crc_shift.
//   png_offsets_kernel  one workgroup: exclusive scan over the group's band lengths plus the 43 bytes in front of a frame's first
//                       band and the 25 behind its last -> the files' offsets (continuing the previous group's) and every band's
//                       place in `out`; per frame the Adler-32 (bands joined in order), the CRC-32 of the zlib stream - every
//                       band's CRC times x^(8 bytes behind it), XORed - and the IDAT chunk's CRC.
//   png_pack_kernel     grid as png_code_kernel: signature, IHDR, IDAT head and 78 01 (first band), the band's bytes, the final
//                       stored block, Adler-32, the IDAT CRC and IEND (last band) into `out`; a byte at or beyond out_cap is
//                       not written.
// The code-length tables are stated once, below, as hex digits; the canonical codes (bit-reversed for deflate's LSB-first
// packing), the CRC byte table and the powers x^(8 2^k) are computed from them at compile time into __device__ constants: no
// table is built or copied at run time.  wave64 throughout.
#pragma once
#include "common.hpp"

constexpr int kPngThreads = 256;
constexpr int kPngGroup = 16;          // frames coded per group: what bounds `work`
constexpr int kPngMaxSide = 16384;
constexpr int kPngBandBytes = 65536;   // the most filter-plus-row bytes of a band
constexpr int kPngPer = 16;            // consecutive bytes a lane codes in one pass
constexpr int kPngChunk = kPngThreads * kPngPer;  // bytes of one pass
constexpr int kPngHeaderBits = 1106;   // 17 + 19 x 3 + 258 x 4
constexpr int kPngHeadBytes = 43;      // signature 8, IHDR 25, IDAT length and type 8, 78 01
constexpr int kPngTailBytes = 25;      // 01 00 00 FF FF, Adler-32, IDAT CRC, IEND 12
constexpr int kPngBitWords = (kPngHeaderBits + kPngChunk * 15 + 7 + 15 + 3 + 7 + 32) / 32 + 2;  // a pass at 15 bits per byte
constexpr uint32_t kPngCrcPoly = 0xEDB88320u;  // reflected: bit 31 is x^0

// T_k[0 ... 256] as hex digits: byte values 0 ... 255, then end-of-block (host_models._PNG_LENGTHS states the same digits)
constexpr const char* kPngLengthDigits[8] = {
    "137abbbbbbbbbbbbbccccccccccccccccccccccccccccccccccccccccccccccccccccccccccccbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbb"
    "bbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbba72b",
    "13579acccccdddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddd"
    "dddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddccccca8652d",
    "233556789aabcccccccdddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddd"
    "dddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddcccccccbaa98765433d",
    "3344555667788999aabbbcccccccddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddd"
    "ddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddccccccbbbbaa999887766554443d",
    "44445555666667777888889999aaaabbbbbbcccccccccdddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddd"
    "dddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddddcccccccccbbbbbaaaaa9999888887777666665555444d",
    "555555556666666677777777888888888999999999aaaaaaaaaabbbbbbbbbbbccccccccccccccccccdddddddddddddddddddddddddddddddddddddddddddddddd"
    "dddddddddddddddddddddddddddddddddddddddddddddddccccccccccccccccccbbbbbbbbbbbaaaaaaaaaa99999999988888888877777777666666665555555d",
    "6666666666666667777777777777777788888888888888888999999999999999999aaaaaaaaaaaaaaaaaaabbbbbbbbbbbbbbbbbbbbbcccccccccccccccccccccd"
    "ccccccccccccccccccccbbbbbbbbbbbbbbbbbbbbbbaaaaaaaaaaaaaaaaaaa999999999999999998888888888888888887777777777777777666666666666666d",
    "888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888889"
    "88888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888889",
};

struct PngLengths {
  uint8_t len[8][257];
};
struct PngCodes {
  uint32_t e[8][257];  // length << 16 | code, bit-reversed
};
struct PngCrc {
  uint32_t byte[256];  // the byte-at-a-time table
  uint32_t pow8[32];   // x^(8 2^k) mod P
};

constexpr PngLengths png_make_lengths() {
  PngLengths t{};
  for (int k = 0; k < 8; ++k)
    for (int s = 0; s < 257; ++s) {
      const char c = kPngLengthDigits[k][s];
      t.len[k][s] = (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10);
    }
  return t;
}
constexpr bool png_lengths_complete(const PngLengths& t) {
  for (int k = 0; k < 8; ++k) {
    unsigned kraft = 0;
    for (int s = 0; s < 257; ++s) {
      if (t.len[k][s] < 1 || t.len[k][s] > 15) return false;
      kraft += 1u << (15 - t.len[k][s]);
    }
    if (kraft != 1u << 15 || kPngLengthDigits[k][257] != 0) return false;
  }
  return true;
}
constexpr PngCodes png_make_codes() {  // RFC 1951 3.2.2: the codes of one length count up in symbol order, and double to the next
  const PngLengths t = png_make_lengths();
  PngCodes c{};
  for (int k = 0; k < 8; ++k) {
    uint32_t count[16] = {}, next[16] = {};
    for (int s = 0; s < 257; ++s) ++count[t.len[k][s]];
    for (int n = 1; n <= 15; ++n) next[n] = (next[n - 1] + count[n - 1]) << 1;
    for (int s = 0; s < 257; ++s) {
      const int n = t.len[k][s];
      const uint32_t code = next[n]++;
      uint32_t rev = 0;
      for (int b = 0; b < n; ++b) rev |= ((code >> b) & 1u) << (n - 1 - b);
      c.e[k][s] = ((uint32_t)n << 16) | rev;
    }
  }
  return c;
}
// a(x) b(x) mod P, both reflected: what zlib's crc32_combine multiplies with
__host__ __device__ constexpr uint32_t png_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? kPngCrcPoly : 0u);
  }
  return p;
}
constexpr PngCrc png_make_crc() {
  PngCrc t{};
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ ((c & 1u) ? kPngCrcPoly : 0u);
    t.byte[i] = c;
  }
  uint32_t p = 0x00800000u;  // x^8
  for (int k = 0; k < 32; ++k) {
    t.pow8[k] = p;
    p = png_crc_mul(p, p);
  }
  return t;
}
constexpr uint32_t png_crc_bytes(const PngCrc& t, const uint8_t* d, int n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) c = t.byte[(c ^ d[i]) & 255u] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

constexpr PngLengths kPngLengths = png_make_lengths();
static_assert(png_lengths_complete(kPngLengths), "a code-length table is not complete, or a length is outside 1 ... 15");
constexpr PngCrc kPngCrcHost = png_make_crc();
constexpr uint8_t kPngZlibHead[2] = {0x78, 0x01};
constexpr uint8_t kPngIdat[4] = {'I', 'D', 'A', 'T'};
constexpr uint32_t kPngCrcZlibHead = png_crc_bytes(kPngCrcHost, kPngZlibHead, 2);
constexpr uint32_t kPngCrcIdat = png_crc_bytes(kPngCrcHost, kPngIdat, 4);

__device__ const PngCodes kPngCodes = png_make_codes();
__device__ const PngCrc kPngCrc = png_make_crc();

struct PngPlan {
  int h, w, band, nb;   // frame sides, rows per band, bands per frame
  int stride;           // bytes of a filtered row: 1 + 3 w
  int frame0, frames;   // the group: frames [frame0, frame0 + frames) of the call
  unsigned long long slot_bytes;
  uint8_t head[33];     // signature and IHDR
};

// crc (of a piece A) -> the part of crc(A | B) that A gives when n bytes follow: crc times x^(8 n); crc(A | B) is that XOR crc(B)
__device__ __forceinline__ uint32_t png_crc_shift(uint32_t crc, unsigned long long n) {
  for (int k = 0; n != 0 && crc != 0; ++k, n >>= 1)
    if (n & 1ull) crc = png_crc_mul(kPngCrc.pow8[k], crc);
  return crc;
}

// Exclusive scan of one int per thread over the 256 threads of a workgroup; *total = the sum.  s_w: 4 ints of LDS.
__device__ __forceinline__ int png_wg_scan(int v, int* s_w, int* total) {
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
  for (int i = 0; i < kPngThreads / 64; ++i) {
    const int t = s_w[i];
    if (i < wave) base += t;
    sum += t;
  }
  __syncthreads();  // s_w may be written again
  *total = sum;
  return base + inc - v;
}

__device__ __forceinline__ uint32_t png_wave_add(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t png_wave_xor(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
  return v;
}

// OR the n (1 ... 32) low bits of v into the bit stream at bit p, LSB first as deflate packs
__device__ __forceinline__ void png_put(uint32_t* bits, uint32_t p, uint32_t v, int n) {
  const unsigned long long x = (unsigned long long)v << (p & 31u);
  atomicOr(&bits[p >> 5], (uint32_t)x);
  if ((uint32_t)(x >> 32)) atomicOr(&bits[(p >> 5) + 1], (uint32_t)(x >> 32));
}

// the PNG specification's filters with bpp = 3: x the byte, a the one 3 to the left, b the one above, c the one above a
__device__ __forceinline__ int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int png_filtered(int f, int x, int a, int b, int c) {
  const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
  return (x - pred) & 255;
}
// the four raw bytes the filters of byte i of row y read; the row above row 0 and the pixel left of pixel 0 are zero
__device__ __forceinline__ void png_neighbours(const uint8_t* __restrict__ cur, int i, int y, int rowbytes, int& x, int& a, int& b, int& c) {
  x = cur[i];
  a = i >= 3 ? cur[i - 3] : 0;
  b = y > 0 ? cur[i - rowbytes] : 0;
  c = (y > 0 && i >= 3) ? cur[i - rowbytes - 3] : 0;
}
__device__ __forceinline__ uint32_t png_byte_of(const uint32_t* bits, int i) { return (bits[i >> 2] >> (8 * (i & 3))) & 255u; }

__global__ __launch_bounds__(kPngThreads) void png_code_kernel(const uint8_t* __restrict__ rgb, PngPlan p, int* __restrict__ lens,
                                                               uint32_t* __restrict__ band_crc, uint32_t* __restrict__ ad1,
                                                               uint32_t* __restrict__ ad2, uint8_t* __restrict__ slots) {
  __shared__ uint32_t s_hist[kPngThreads / 64][256];
  __shared__ uint32_t s_code[257];
  __shared__ uint32_t s_crct[256];
  __shared__ uint32_t s_bits[kPngBitWords];
  __shared__ uint32_t s_red[kPngThreads / 64][8];
  __shared__ int s_w[kPngThreads / 64];
  __shared__ __align__(16) uint8_t s_stage[kPngChunk];
  __shared__ uint8_t s_filt[kPngMaxSide];  // the filter type of every row of the band
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bd = blockIdx.x, fr = blockIdx.y;
  const int rowbytes = 3 * p.w;
  const int row0 = bd * p.band;
  const int rows = min(p.band, p.h - row0);
  const int N = rows * p.stride;
  const uint8_t* img = rgb + (size_t)(p.frame0 + fr) * ((size_t)p.h * rowbytes);
  uint8_t* slot = slots + ((size_t)fr * p.nb + bd) * p.slot_bytes;

  for (int i = tid; i < (kPngThreads / 64) * 256; i += kPngThreads) (&s_hist[0][0])[i] = 0;
  s_crct[tid] = kPngCrc.byte[tid];
  __syncthreads();
  // (1) the filter of every row and the histogram of the filtered bytes: a wave per row
  for (int r = wave; r < rows; r += kPngThreads / 64) {
    const int y = row0 + r;
    const uint8_t* cur = img + (size_t)y * rowbytes;
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < rowbytes; i += 64) {
      int x, a, b, c;
      png_neighbours(cur, i, y, rowbytes, x, a, b, c);
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        const int v = png_filtered(f, x, a, b, c);
        cost[f] += (uint32_t)min(v, 256 - v);
      }
    }
    int best = 0;
    uint32_t best_cost = png_wave_add(cost[0]);
#pragma unroll
    for (int f = 1; f < 5; ++f) {
      const uint32_t t = png_wave_add(cost[f]);
      if (t < best_cost) best_cost = t, best = f;
    }
    if (lane == 0) {
      s_filt[r] = (uint8_t)best;
      atomicAdd(&s_hist[wave][best], 1u);
    }
    for (int i = lane; i < rowbytes; i += 64) {
      int x, a, b, c;
      png_neighbours(cur, i, y, rowbytes, x, a, b, c);
      atomicAdd(&s_hist[wave][png_filtered(best, x, a, b, c)], 1u);
    }
  }
  __syncthreads();
  // (2) the table: bits(k) = sum of hist[v] T_k[v], a lane per byte value
  {
    uint32_t hv = 0;
#pragma unroll
    for (int i = 0; i < kPngThreads / 64; ++i) hv += s_hist[i][tid];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t t = png_wave_add(hv * (kPngCodes.e[k][tid] >> 16));
      if (lane == 0) s_red[wave][k] = t;
    }
  }
  __syncthreads();
  int table = 0;
  {
    uint32_t best_bits = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      uint32_t t = 0;
#pragma unroll
      for (int i = 0; i < kPngThreads / 64; ++i) t += s_red[i][k];
      if (t < best_bits) best_bits = t, table = k;
    }
  }
  for (int i = tid; i < 257; i += kPngThreads) s_code[i] = kPngCodes.e[table][i];
  __syncthreads();
  const uint32_t eob = s_code[256];

  // (3) the band's bits, kPngChunk bytes per pass
  uint32_t carry_bits = 0, carry_byte = 0, crc_all = 0, sum_a = 0, sum_b = 0;
  size_t outpos = 0;
  for (int c0 = 0; c0 < N; c0 += kPngChunk) {
    const int n = min(kPngChunk, N - c0);
    const bool first = c0 == 0, last = c0 + n >= N;
    for (int j = tid; j < n; j += kPngThreads) {
      const int g = c0 + j;
      const int r = g / p.stride, col = g - r * p.stride;
      const int f = s_filt[r];
      int v = f;
      if (col > 0) {
        int x, a, b, c;
        png_neighbours(img + (size_t)(row0 + r) * rowbytes, col - 1, row0 + r, rowbytes, x, a, b, c);
        v = png_filtered(f, x, a, b, c);
      }
      s_stage[j] = (uint8_t)v;
    }
    __syncthreads();
    const int j0 = tid * kPngPer;
    const int cnt = max(0, min(kPngPer, n - j0));
    int len = 0;
    {
      uint32_t a1 = 0, b1 = 0;
      for (int i = 0; i < cnt; ++i) {
        const uint32_t v = s_stage[j0 + i];
        len += (int)(s_code[v] >> 16);
        a1 += v;
        b1 += (uint32_t)(cnt - i) * v;
      }
      // Adler: byte i of the band counts N - i times in s2; a1 <= 4080 and the bytes behind this run <= 65536
      const uint32_t behind = (uint32_t)(N - (c0 + j0 + cnt));
      sum_a += a1;
      sum_b = (sum_b + b1 + a1 * (cnt > 0 ? behind : 0u)) % 65521u;
    }
    int sum;
    const int off = png_wg_scan(len, s_w, &sum);
    const uint32_t base = carry_bits + (first ? (uint32_t)kPngHeaderBits : 0u);
    const uint32_t total = base + (uint32_t)sum;
    // behind the last code: end-of-block, 000 (a stored block, not final), zeros to the byte boundary, 00 00 FF FF
    const uint32_t fin = last ? ((total + (eob >> 16) + 3u + 7u) & ~7u) + 32u : total;
    for (uint32_t i = tid; i <= (fin >> 5) + 1; i += kPngThreads) s_bits[i] = i == 0 ? carry_byte : 0u;
    __syncthreads();
    if (first) {
      // BFINAL 0, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15; the code-length code in its order 16 17 18 0 8 ...: 0 0 0, then 4 sixteen
      // times; the 257 lengths and one distance length 0 as 4-bit codes (symbol n has code n, sent MSB first)
      if (tid == 0) png_put(s_bits, 0, 0x1E004u, 17);
      if (tid >= 3 && tid < 19) png_put(s_bits, 17u + 3u * tid, 4u, 3);
      for (int i = tid; i < 258; i += kPngThreads) {
        const uint32_t l = i < 257 ? s_code[i] >> 16 : 0u;
        const uint32_t rev = ((l & 1u) << 3) | ((l & 2u) << 1) | ((l & 4u) >> 1) | ((l & 8u) >> 3);
        if (rev) png_put(s_bits, 74u + 4u * i, rev, 4);
      }
    }
    if (cnt > 0) {
      const uint32_t at = base + (uint32_t)off;
      uint32_t w = at >> 5, fill = at & 31u;
      unsigned long long acc = 0;
      for (int i = 0; i < cnt; ++i) {
        const uint32_t e = s_code[s_stage[j0 + i]];
        acc |= (unsigned long long)(e & 0xFFFFu) << fill;
        fill += e >> 16;
        if (fill >= 32u) {
          atomicOr(&s_bits[w++], (uint32_t)acc);
          acc >>= 32;
          fill -= 32u;
        }
      }
      if ((uint32_t)acc) atomicOr(&s_bits[w], (uint32_t)acc);
    }
    if (last && tid == 0) {
      png_put(s_bits, total, eob & 0xFFFFu, (int)(eob >> 16));
      png_put(s_bits, fin - 16u, 0xFFFFu, 16);
    }
    __syncthreads();
    // the whole bytes: their CRC (a run per lane, joined by the bytes behind it) and their copy into the slot
    const int nbytes = (int)(fin >> 3);
    {
      const int per = (nbytes + kPngThreads - 1) / kPngThreads;
      const int a = min(tid * per, nbytes), e = min(a + per, nbytes);
      uint32_t c = 0xFFFFFFFFu;
      for (int i = a; i < e; ++i) c = s_crct[(c ^ png_byte_of(s_bits, i)) & 255u] ^ (c >> 8);
      c = png_wave_xor(png_crc_shift(~c, (unsigned long long)(nbytes - e)));
      if (lane == 0) s_red[wave][0] = c;
    }
    for (int i = tid; i < nbytes; i += kPngThreads) slot[outpos + i] = (uint8_t)png_byte_of(s_bits, i);
    outpos += (size_t)nbytes;
    carry_bits = fin & 7u;
    carry_byte = carry_bits ? png_byte_of(s_bits, nbytes) : 0u;
    __syncthreads();  // s_bits and s_stage are read before the next pass writes them
    if (tid == 0) {
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < kPngThreads / 64; ++i) c ^= s_red[i][0];
      crc_all = png_crc_shift(crc_all, (unsigned long long)nbytes) ^ c;
    }
  }
  sum_a = png_wave_add(sum_a);
  sum_b = png_wave_add(sum_b);
  if (lane == 0) s_red[wave][1] = sum_a, s_red[wave][2] = sum_b;
  __syncthreads();
  if (tid == 0) {
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < kPngThreads / 64; ++i) a += s_red[i][1], b += s_red[i][2];
    const int item = fr * p.nb + bd;
    lens[item] = (int)outpos;
    band_crc[item] = crc_all;
    ad1[item] = a % 65521u;
    ad2[item] = b % 65521u;
  }
}

// what band `bd` of a frame adds to the file
__device__ __forceinline__ long long png_piece(const PngPlan& p, int bd, int len) {
  return (long long)len + (bd == 0 ? kPngHeadBytes : 0) + (bd == p.nb - 1 ? kPngTailBytes : 0);
}

// meta: 4 words per frame of the group - the IDAT length, the Adler-32, the CRC-32 of the zlib stream, the IDAT chunk's CRC
__global__ __launch_bounds__(kPngThreads) void png_offsets_kernel(PngPlan p, const int* __restrict__ lens, const uint32_t* __restrict__ band_crc,
                                                                  const uint32_t* __restrict__ ad1, const uint32_t* __restrict__ ad2,
                                                                  long long* __restrict__ dst, uint32_t* __restrict__ meta,
                                                                  long long* __restrict__ offsets, uint32_t* __restrict__ crcs) {
  __shared__ long long s_sum[kPngThreads];
  __shared__ long long s_start[kPngGroup + 1];
  __shared__ uint32_t s_crc[kPngGroup];
  const int tid = threadIdx.x;
  const int items = p.frames * p.nb;
  const int per = (items + kPngThreads - 1) / kPngThreads;
  const int a = min(tid * per, items), e = min(a + per, items);
  const long long base = p.frame0 == 0 ? 0 : offsets[p.frame0];  // the previous group's launch wrote it
  long long sum = 0;
  for (int i = a; i < e; ++i) sum += png_piece(p, i % p.nb, lens[i]);
  s_sum[tid] = sum;
  if (tid < kPngGroup) s_crc[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    long long run = base;
    for (int i = 0; i < kPngThreads; ++i) {
      const long long t = s_sum[i];
      s_sum[i] = run;
      run += t;
    }
    offsets[p.frame0 + p.frames] = run;
    s_start[p.frames] = run;
  }
  __syncthreads();
  long long run = s_sum[tid];
  for (int i = a; i < e; ++i) {
    const int bd = i % p.nb;
    if (bd == 0) offsets[p.frame0 + i / p.nb] = run, s_start[i / p.nb] = run;
    dst[i] = run + (bd == 0 ? kPngHeadBytes : 0);
    run += png_piece(p, bd, lens[i]);
  }
  __syncthreads();
  // a band's share of the zlib stream's CRC: its own CRC times x^(8 bytes between its end and the stream's)
  for (int i = a; i < e; ++i) {
    const long long zend = s_start[i / p.nb + 1] - 16;  // the IDAT CRC and IEND follow the stream
    atomicXor(&s_crc[i / p.nb], png_crc_shift(band_crc[i], (unsigned long long)(zend - (dst[i] + lens[i]))));
  }
  __syncthreads();
  if (tid < p.frames) {
    uint32_t s1 = 1, s2 = 0;
    for (int bd = 0; bd < p.nb; ++bd) {  // Adler-32 of A | B from A's (s1, s2) and B's sums: s2 grows by len(B) s1
      const int i = tid * p.nb + bd;
      const unsigned long long n = (unsigned long long)min(p.band, p.h - bd * p.band) * p.stride;
      s2 = (uint32_t)((s2 + (n % 65521u) * s1 + ad2[i]) % 65521u);
      s1 = (s1 + ad1[i]) % 65521u;
    }
    const uint32_t adler = (s2 << 16) | s1;
    const unsigned long long zlen = (unsigned long long)(s_start[tid + 1] - s_start[tid]) - (kPngHeadBytes - 2) - 16;
    const uint8_t tail[9] = {1, 0, 0, 255, 255, (uint8_t)(adler >> 24), (uint8_t)(adler >> 16), (uint8_t)(adler >> 8), (uint8_t)adler};
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < 9; ++i) c = kPngCrc.byte[(c ^ tail[i]) & 255u] ^ (c >> 8);
    const uint32_t zcrc = png_crc_shift(kPngCrcZlibHead, zlen - 2) ^ s_crc[tid] ^ ~c;
    uint32_t* m = meta + 4 * tid;
    m[0] = (uint32_t)zlen, m[1] = adler, m[2] = zcrc, m[3] = png_crc_shift(kPngCrcIdat, zlen) ^ zcrc;
    if (crcs) crcs[p.frame0 + tid] = zcrc;
  }
}

__global__ __launch_bounds__(kPngThreads) void png_pack_kernel(PngPlan p, const int* __restrict__ lens, const long long* __restrict__ dst,
                                                               const uint32_t* __restrict__ meta, const uint8_t* __restrict__ slots,
                                                               uint8_t* __restrict__ out, unsigned long long out_cap) {
  const int tid = threadIdx.x;
  const int bd = blockIdx.x, fr = blockIdx.y;
  const int item = fr * p.nb + bd;
  const int len = lens[item];
  const unsigned long long at = (unsigned long long)dst[item];
  const uint8_t* slot = slots + (size_t)item * p.slot_bytes;
  const uint32_t* m = meta + 4 * fr;
  if (bd == 0 && tid < kPngHeadBytes) {
    const uint32_t zlen = m[0];
    const uint8_t v = tid < 33 ? p.head[tid] : tid < 37 ? (uint8_t)(zlen >> (8 * (36 - tid))) : tid == 37 ? 'I' : tid == 38 ? 'D' : tid == 39 ? 'A'
                    : tid == 40 ? 'T' : tid == 41 ? 0x78 : 0x01;
    if (at - kPngHeadBytes + tid < out_cap) out[at - kPngHeadBytes + tid] = v;
  }
  for (int i = tid; i < len; i += kPngThreads)
    if (at + i < out_cap) out[at + i] = slot[i];
  if (bd == p.nb - 1 && tid < kPngTailBytes) {
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    const uint8_t stored[5] = {1, 0, 0, 255, 255};
    const uint8_t v = tid < 5 ? stored[tid] : tid < 9 ? (uint8_t)(m[1] >> (8 * (8 - tid))) : tid < 13 ? (uint8_t)(m[3] >> (8 * (12 - tid))) : iend[tid - 13];
    if (at + len + tid < out_cap) out[at + len + tid] = v;
  }
}
