// The JPEG decoder's rule as host-and-device inline code, shared by its kernels (jpgd_kernels.hpp) and by the host path
// (jpgd_plan.hpp: float_jpg_decode_host and the stand-alone tools/probes/jpgd_host.cpp): the plan's layout, the bit reader, the
// Huffman symbol decode, one block's coefficients, the two IDCT passes, chroma upsampling and the colour conversion.  The rule
// itself is written out in host_models.jpeg_decode_rgb8.  Plain C++ plus stdint: a host compiler without HIP takes it as it is.
// All arithmetic is int32 with wrap-around, spelled in uint32_t where a signed overflow or a shift of a negative could occur.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPGD_HD __host__ __device__ __forceinline__
#else
#define JPGD_HD inline
#endif

// ---------------------------------------------------------------- the plan: int32 words
// header, then one frame record per frame, then the distinct table sets
enum {
  JPGD_P_MAGIC = 0,  // kJpgdMagic
  JPGD_P_INTS,       // words in use
  JPGD_P_N,          // frames
  JPGD_P_H,
  JPGD_P_W,
  JPGD_P_NCOMP,  // 1 or 3
  JPGD_P_HS,     // luma sampling: 1 | 2
  JPGD_P_VS,
  JPGD_P_MCUX,  // MCUs per row, rows of MCUs
  JPGD_P_MCUY,
  JPGD_P_BPM,      // blocks per MCU
  JPGD_P_NSETS,    // distinct table sets
  JPGD_P_MAXINT,   // the most intervals of a frame
  JPGD_P_GROUP,    // frames that share `work`
  JPGD_P_FRAMES,   // word index of frame record 0
  JPGD_P_SETS,     // word index of table set 0
  JPGD_P_HEADER = 16
};
// scan bytes [SCAN0, SCAN1) of the file; MCUs per interval; ROUTE: 0 = one lane per restart interval, above 0 the sync route (below)
// with that many bytes as its shortest subsequence, below 0 the split route (further below) with minus that many
enum { JPGD_F_SCAN0 = 0, JPGD_F_SCAN1, JPGD_F_SPAN, JPGD_F_NINT, JPGD_F_SET, JPGD_F_ROUTE, JPGD_F_INTS = 8 };
constexpr int32_t kJpgdMagic = 0x4A504744;
// a Huffman table: look[512] uint16 (length << 8 | symbol of every 9-bit prefix, 0: longer or none), maxcode[18], valoff[18], vals[256] uint8
constexpr int kJpgdHuffLook = 0, kJpgdHuffMax = 256, kJpgdHuffOff = 274, kJpgdHuffVals = 292, kJpgdHuffInts = 356;
// a table set: per component c the quantiser (64 uint16, natural order) at 32 c, then the tables DC c, AC c at kJpgdSetHuff + (2 c + class) kJpgdHuffInts
constexpr int kJpgdSetHuff = 96, kJpgdSetInts = kJpgdSetHuff + 6 * kJpgdHuffInts;
constexpr int JPGD_ST_BAD_CODE = 1, JPGD_ST_RESTARTS = 2, JPGD_ST_PAST_END = 4;  // the bits of a frame's status word

struct JpgdHuff {
  const uint16_t* look;
  const int32_t* maxcode;
  const int32_t* valoff;
  const uint8_t* vals;
};
JPGD_HD JpgdHuff jpgd_huff(const int32_t* set, int comp, int cls) {
  const int32_t* t = set + kJpgdSetHuff + (2 * comp + cls) * kJpgdHuffInts;
  return JpgdHuff{(const uint16_t*)(t + kJpgdHuffLook), t + kJpgdHuffMax, t + kJpgdHuffOff, (const uint8_t*)(t + kJpgdHuffVals)};
}

JPGD_HD int jpgd_natural(int k) {  // zigzag position -> row-major index
  constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k];
}

// ---------------------------------------------------------------- bit reader over bytes [p, end): unstuffs 0xFF 0x00, zeros past the end
struct JpgdBits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc;   // the low n bits are unread
  int n;
  uint32_t over;  // zero bytes supplied past the end
};
JPGD_HD void jpgd_bits_open(JpgdBits& b, const uint8_t* p, const uint8_t* end) { b.p = p, b.end = end, b.acc = 0, b.n = 0, b.over = 0; }
JPGD_HD void jpgd_fill(JpgdBits& b) {  // at least 57 unread bits afterwards
  while (b.n <= 56) {
    uint32_t v = 0;
    if (b.p < b.end) {
      v = *b.p++;
      if (v == 0xFF && b.p < b.end && *b.p == 0) ++b.p;
    } else {
      ++b.over;
    }
    b.acc = (b.acc << 8) | v;
    b.n += 8;
  }
}
template <class B>
JPGD_HD uint32_t jpgd_peek(const B& b, int k) { return (uint32_t)(b.acc >> (b.n - k)) & ((1u << k) - 1u); }  // 1 <= k <= 16 <= n
JPGD_HD bool jpgd_past_end(const JpgdBits& b) { return (uint64_t)b.over * 8 > (uint64_t)b.n; }  // a supplied zero bit was consumed

// The same reader over bytes that hold no stuffing any more (the sync route's copy of a scan): a position is one integer, a bit
// offset.  u[at] is the next byte to load, zeros from u[len] on.
struct JpgdRaw {
  const uint8_t* u;
  uint32_t at, len;
  uint64_t acc;
  int n;
};
JPGD_HD void jpgd_raw_open(JpgdRaw& b, const uint8_t* u, uint32_t len, uint32_t bit) {
  b.u = u, b.len = len, b.at = bit >> 3, b.acc = 0, b.n = 0;
  if (bit & 7u) b.acc = b.at < len ? u[b.at] : 0u, ++b.at, b.n = 8 - (int)(bit & 7u);  // the byte's read bits stay above the low n
}
JPGD_HD void jpgd_fill(JpgdRaw& b) {
  while (b.n <= 56) {
    const uint32_t v = b.at < b.len ? b.u[b.at] : 0u;
    ++b.at;
    b.acc = (b.acc << 8) | v;
    b.n += 8;
  }
}
JPGD_HD uint32_t jpgd_raw_pos(const JpgdRaw& b) { return 8u * b.at - (uint32_t)b.n; }  // the next unread bit
JPGD_HD bool jpgd_past_end(const JpgdRaw& b) { return 8ull * b.at - (uint64_t)b.n > 8ull * b.len; }  // JpgdBits' rule: over = at - len

// one symbol (needs 16 unread bits); -1 for a code that matches none
template <class B>
JPGD_HD int jpgd_symbol(B& b, const JpgdHuff& t) {
  const uint32_t e = t.look[jpgd_peek(b, 9)];
  if (e) {
    b.n -= (int)(e >> 8);
    return (int)(e & 255);
  }
  int l = 10;
  while (l <= 16 && (int32_t)jpgd_peek(b, l) > t.maxcode[l]) ++l;
  if (l > 16) return -1;
  const int sym = t.vals[((int32_t)jpgd_peek(b, l) + t.valoff[l]) & 255];
  b.n -= l;
  return sym;
}
// s more bits (s <= 15, after jpgd_symbol's 16 of one fill) as the signed value of category s
template <class B>
JPGD_HD int32_t jpgd_extend(B& b, int s) {
  if (s == 0) return 0;
  const int32_t r = (int32_t)jpgd_peek(b, s);
  b.n -= s;
  return r >= (1 << (s - 1)) ? r : r - (1 << s) + 1;
}

// One block: 64 coefficients in natural order into coef[0 ... 63] (zeroed by the caller), NOT dequantised - a 16-bit table entry
// times a coefficient needs the int32 the IDCT multiplies in.  false: a bad code or an overflowing run.
template <class B, class P>
JPGD_HD bool jpgd_block(B& b, const JpgdHuff& dc, const JpgdHuff& ac, int32_t& pred, P coef) {
  jpgd_fill(b);
  int s = jpgd_symbol(b, dc);
  if (s < 0) return false;
  pred = (int32_t)((uint32_t)pred + (uint32_t)jpgd_extend(b, s & 15));
  coef[0] = (int16_t)(uint16_t)((uint32_t)pred & 0xFFFFu);
  for (int k = 1; k < 64;) {
    jpgd_fill(b);
    const int rs = jpgd_symbol(b, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;
      if (k + 16 > 64) return false;
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return false;
    coef[jpgd_natural(k)] = (int16_t)jpgd_extend(b, s);
    ++k;
  }
  return true;
}

// ---------------------------------------------------------------- the sync route: one scan without restart markers, many lanes
// The scan's one segment is copied without its stuffing and cut into n_sub subsequences of S bytes; lane i OWNS the blocks whose
// first bit lies in subsequence i and decodes an owned block to its end.  Between blocks the decoder's state is (p, j): the
// bit offset of the next block and that block's index inside the MCU; kJpgdDead for p says that a bad code was met.  Lanes
// guess an entry state, decode, and decode again from their predecessor's exit until no exit changes: Huffman streams fall
// into step, and lane i's entry is the serial chain's after round i at the latest.  A dead exit may be a wrong guess's: lane i
// takes it over in round i, when it is final, and keeps its own entry until then.
constexpr uint32_t kJpgdDead = 0xFFFFFFFFu;
constexpr int kJpgdSyncLanes = 1024;        // subsequences of a scan, at most
constexpr int kJpgdSyncBytes = 64;          // the default shortest subsequence
constexpr int kJpgdSyncMaxBytes = 65536;    // the longest a caller may ask for
constexpr int32_t kJpgdSyncScan = 1 << 28;  // scans from here on stay on the interval route: a bit offset is a uint32_t
// the lane table in `work`: a header, then per lane (entry p, entry j, first block, pred[3])
enum { JPGD_T_LEN = 0, JPGD_T_S, JPGD_T_NSUB, JPGD_T_ZERO, JPGD_T_ROUNDS, JPGD_T_HEADER = 8, JPGD_T_LANE = 6 };
constexpr int kJpgdTableInts = JPGD_T_HEADER + kJpgdSyncLanes * JPGD_T_LANE;

JPGD_HD uint32_t jpgd_sync_sub(uint32_t len, uint32_t sync_bytes) {  // S
  const uint32_t s = (len + kJpgdSyncLanes - 1) / kJpgdSyncLanes;
  return s > sync_bytes ? s : sync_bytes;
}
JPGD_HD uint32_t jpgd_sync_lanes(uint32_t len, uint32_t S) { return len ? (len + S - 1) / S : 1u; }  // n_sub <= kJpgdSyncLanes
JPGD_HD uint32_t jpgd_sync_end(uint32_t i, uint32_t S, uint32_t len) { return 8u * ((i + 1) * S < len ? (i + 1) * S : len); }  // lane i's last bit + 1

struct JpgdNoCoef {  // a block that is decoded and not kept
  struct Sink {
    JPGD_HD void operator=(int16_t) {}
  };
  JPGD_HD Sink operator[](int) const { return Sink(); }
};
struct JpgdRun {
  uint32_t p;     // in: the entry's bit offset.  out: where the first block starts that is not this run's, or kJpgdDead
  int32_t j;      // ... and that block's index inside the MCU
  uint32_t n;     // out: blocks decoded well
  int32_t dc[3];  // in: the predictions.  out: after the last block (from 0: the wrap-around sums of the DC differences)
};
// The blocks from state (x.p, x.j) that start before bit `end` - all of them for `tail`, which reads zero bits from the end
// of the data on - and at most `room` blocks.  block(b, component, prediction, k) decodes the run's k-th block.
template <class F>
JPGD_HD void jpgd_sync_run(JpgdRaw& b, const uint8_t* u, uint32_t len, uint32_t end, bool tail, uint32_t room, int hv, int bpm, JpgdRun& x, F&& block) {
  x.n = 0;
  if (x.p == kJpgdDead) {
    x.j = 0;
    return;
  }
  jpgd_raw_open(b, u, len, x.p);
  while ((x.p < end || tail) && x.n < room) {
    const int c = x.j < hv ? 0 : x.j - hv + 1;
    int32_t& pr = c == 0 ? x.dc[0] : c == 1 ? x.dc[1] : x.dc[2];
    if (!block(b, c, pr, x.n)) {
      x.p = kJpgdDead, x.j = 0;
      return;
    }
    ++x.n;
    x.j = x.j + 1 == bpm ? 0 : x.j + 1;
    x.p = jpgd_raw_pos(b);
  }
}

// ---------------------------------------------------------------- the split route: a scan WITH restart markers, many lanes
// A restart marker is a point where the serial state is known: a byte boundary, block 0 of an MCU, predictions 0.  So every
// interval's segment is copied without its stuffing into one buffer per frame, interval k becomes jpgd_split_lanes(len_k, S)
// subsequences of S = jpgd_split_sub(...) bytes - the frame's kJpgdSyncLanes lanes dealt out by length -, and the sync route's
// relaxation runs inside each interval: positions are bit offsets from the interval's first byte, the interval's first lane
// enters at the true (0, 0), a lane takes its predecessor's exit inside its interval only, and block counts and DC sums are
// prefixed per interval.  An interval without a segment (too few markers) has no lane and keeps its zeros.  The frame's ROUTE
// word is minus the shortest subsequence.
constexpr int kJpgdSplitIntervals = kJpgdSyncLanes / 2;  // frames with more intervals stay on the interval route
// the table in `work`: the sync route's header, then per lane (entry p, entry j, first block inside the interval, pred[3],
// interval, lane inside the interval), then per interval (first byte in the copy, bytes, lanes, first block to zero inside it)
enum { JPGD_X_LANE = 8, JPGD_X_INT = 4 };
constexpr int kJpgdSplitLaneAt = JPGD_T_HEADER, kJpgdSplitIntAt = kJpgdSplitLaneAt + kJpgdSyncLanes * JPGD_X_LANE;
constexpr int kJpgdSplitTableInts = kJpgdSplitIntAt + kJpgdSplitIntervals * JPGD_X_INT;

// S: `present` <= kJpgdSplitIntervals intervals have a segment, `total` bytes in all.  Every such interval gets a lane, the
// bytes share the rest: sum of jpgd_split_lanes <= present + total / S <= kJpgdSyncLanes.
JPGD_HD uint32_t jpgd_split_sub(uint32_t total, uint32_t present, uint32_t sync_bytes) {
  const uint32_t room = (uint32_t)kJpgdSyncLanes - present, s = (total + room - 1) / room;
  return s > sync_bytes ? s : sync_bytes;
}
JPGD_HD uint32_t jpgd_split_lanes(uint32_t len, uint32_t S) { return len ? (len + S - 1) / S : 1u; }
// the blocks of interval k: `span` MCUs, fewer in the frame's last
JPGD_HD uint32_t jpgd_split_blocks(int k, int span, int nmcu, int bpm) {
  const long long m0 = (long long)k * span, m1 = m0 + span < nmcu ? m0 + span : nmcu;
  return (uint32_t)((m1 - m0) * bpm);
}

// ---------------------------------------------------------------- jidctint.c ("islow"): one 8-point pass
JPGD_HD int32_t jpgd_mul(int32_t a, int32_t c) { return (int32_t)((uint32_t)a * (uint32_t)c); }
JPGD_HD int32_t jpgd_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
JPGD_HD int32_t jpgd_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
JPGD_HD int32_t jpgd_shl13(int32_t a) { return (int32_t)((uint32_t)a << 13); }
// v[0 ... 7] in place; SHIFT 11 for pass 1 (down a column of dequantised coefficients), 18 for pass 2 (along a row of pass 1)
template <int SHIFT>
JPGD_HD void jpgd_idct8(int32_t* v) {
  const int32_t i0 = v[0], i1 = v[1], i2 = v[2], i3 = v[3], i4 = v[4], i5 = v[5], i6 = v[6], i7 = v[7];
  int32_t z1 = jpgd_mul(jpgd_add(i2, i6), 4433);
  int32_t t2 = jpgd_add(z1, jpgd_mul(i6, -15137));
  int32_t t3 = jpgd_add(z1, jpgd_mul(i2, 6270));
  int32_t t0 = jpgd_shl13(jpgd_add(i0, i4));
  int32_t t1 = jpgd_shl13(jpgd_sub(i0, i4));
  const int32_t t10 = jpgd_add(t0, t3), t13 = jpgd_sub(t0, t3), t11 = jpgd_add(t1, t2), t12 = jpgd_sub(t1, t2);
  z1 = jpgd_add(i7, i1);
  int32_t z2 = jpgd_add(i5, i3), z3 = jpgd_add(i7, i3), z4 = jpgd_add(i5, i1);
  const int32_t z5 = jpgd_mul(jpgd_add(z3, z4), 9633);
  t0 = jpgd_mul(i7, 2446), t1 = jpgd_mul(i5, 16819), t2 = jpgd_mul(i3, 25172), t3 = jpgd_mul(i1, 12299);
  z1 = jpgd_mul(z1, -7373), z2 = jpgd_mul(z2, -20995);
  z3 = jpgd_add(jpgd_mul(z3, -16069), z5), z4 = jpgd_add(jpgd_mul(z4, -3196), z5);
  t0 = jpgd_add(t0, jpgd_add(z1, z3)), t1 = jpgd_add(t1, jpgd_add(z2, z4));
  t2 = jpgd_add(t2, jpgd_add(z2, z3)), t3 = jpgd_add(t3, jpgd_add(z1, z4));
  constexpr int32_t rnd = 1 << (SHIFT - 1);
  v[0] = jpgd_add(jpgd_add(t10, t3), rnd) >> SHIFT, v[7] = jpgd_add(jpgd_sub(t10, t3), rnd) >> SHIFT;
  v[1] = jpgd_add(jpgd_add(t11, t2), rnd) >> SHIFT, v[6] = jpgd_add(jpgd_sub(t11, t2), rnd) >> SHIFT;
  v[2] = jpgd_add(jpgd_add(t12, t1), rnd) >> SHIFT, v[5] = jpgd_add(jpgd_sub(t12, t1), rnd) >> SHIFT;
  v[3] = jpgd_add(jpgd_add(t13, t0), rnd) >> SHIFT, v[4] = jpgd_add(jpgd_sub(t13, t0), rnd) >> SHIFT;
}
JPGD_HD int32_t jpgd_clamp8(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
JPGD_HD uint8_t jpgd_sample(int32_t pass2) { return (uint8_t)jpgd_clamp8(jpgd_add(pass2, 128)); }  // range limit around +128

// ---------------------------------------------------------------- chroma at full resolution and the colour conversion
// The planes hold whole blocks; (cw, ch) is the chroma plane's true size, which neighbours are clamped to.  hs, vs: 1 | 2.
JPGD_HD int32_t jpgd_chroma(const uint8_t* plane, int stride, int cw, int ch, int hs, int vs, int x, int y) {
  const int cy = vs == 2 ? y >> 1 : y, cx = hs == 2 ? x >> 1 : x;
  const uint8_t* row = plane + (size_t)cy * stride;
  if (hs == 1 || cw <= 2) return row[cx];  // replication (vs == 2 comes with hs == 2 only)
  const int nx = (x & 1) ? (cx + 1 < cw ? cx + 1 : cw - 1) : (cx > 0 ? cx - 1 : 0);
  if (vs == 1) return (3 * row[cx] + row[nx] + ((x & 1) ? 2 : 1)) >> 2;
  const int ny = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
  const uint8_t* far = plane + (size_t)ny * stride;
  const int32_t s_this = 3 * row[cx] + far[cx], s_next = 3 * row[nx] + far[nx];
  return (3 * s_this + s_next + ((x & 1) ? 7 : 8)) >> 4;
}
JPGD_HD void jpgd_rgb(int32_t y, int32_t cb, int32_t cr, uint8_t* rgb) {
  cb -= 128, cr -= 128;
  rgb[0] = (uint8_t)jpgd_clamp8(y + ((91881 * cr + 32768) >> 16));
  rgb[1] = (uint8_t)jpgd_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = (uint8_t)jpgd_clamp8(y + ((116130 * cb + 32768) >> 16));
}
