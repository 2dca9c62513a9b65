// Host-only half of the JPEG decoder: the header parser and the plan builder behind float_jpg_decode_plan, the layout of `work`,
// and the host path of the rule (float_jpg_decode_host, tools/probes/jpgd_host.cpp).  Plain C++: no HIP call, no GPU.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jpgd_rule.hpp"

constexpr int32_t kJpgdMaxSide = 16384;
constexpr int kJpgdGroup = 16;                        // frames that share `work`, at most
constexpr unsigned long long kJpgdGroupBytes = 1ull << 30;  // ... and as few as keep a group's work below this (one frame always goes)

struct JpgdTable {  // a DHT table as the file has it
  bool have = false;
  uint8_t bits[16];
  uint8_t vals[256];
  int n = 0;
};
struct JpgdFile {
  int h = 0, w = 0, ncomp = 0, hs = 1, vs = 1, restart = 0;
  long long scan0 = 0, scan1 = 0;
  int32_t set[kJpgdSetInts];  // the resolved tables of the components
};

inline int jpgd_fail(char* err, size_t errn, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err, errn, fmt, ap);
  va_end(ap);
  return 1;
}

// BITS / HUFFVAL -> the decoder's form; false for over-subscribed lengths
inline bool jpgd_derive(const JpgdTable& t, int32_t* out) {
  // the lengths are checked BEFORE any table is written: with every code of length l below 2^l, a look-ahead index
  // (code << (9 - l)) | fill stays below 512
  for (int l = 1, c = 0, n = 0; l <= 16; ++l, c <<= 1)
    if ((c += t.bits[l - 1]) > (1 << l) || (n += t.bits[l - 1]) > 256) return false;  // ... and vals[] holds 256
  memset(out, 0, kJpgdHuffInts * sizeof(int32_t));
  uint16_t* look = (uint16_t*)(out + kJpgdHuffLook);
  int32_t* maxcode = out + kJpgdHuffMax;
  int32_t* valoff = out + kJpgdHuffOff;
  memcpy(out + kJpgdHuffVals, t.vals, 256);
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    maxcode[l] = -1;
    if (t.bits[l - 1]) {
      valoff[l] = k - code;
      for (int i = 0; i < t.bits[l - 1]; ++i, ++code, ++k)
        if (l <= 9)
          for (int f = 0; f < (1 << (9 - l)); ++f) look[(code << (9 - l)) | f] = (uint16_t)((l << 8) | t.vals[k]);
      maxcode[l] = code - 1;
    }
    if (code > (1 << l)) return false;
    code <<= 1;
  }
  maxcode[0] = -1, maxcode[17] = 0xFFFFF;
  return true;
}

// One file's header -> JpgdFile; 1 with the reason in err.  Every refusal of host_models.jpeg_parse_header, in its words.
inline int jpgd_parse(const uint8_t* d, long long n, JpgdFile* f, char* err, size_t errn) {
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return jpgd_fail(err, errn, "no SOI marker at the start of the file");
  std::vector<uint16_t> qt(4 * 64);
  bool have_q[4] = {false, false, false, false}, have_sof = false;
  std::vector<JpgdTable> huff(8);  // class * 4 + id
  int comp_id[3] = {0, 0, 0}, comp_q[3] = {0, 0, 0};
  static const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  long long pos = 2;
  for (;;) {
    if (pos + 2 > n) return jpgd_fail(err, errn, "the header runs past the end of the file (truncated header)");
    if (d[pos] != 0xFF) return jpgd_fail(err, errn, "no marker at byte %lld of the header", pos);
    const int m = d[pos + 1];
    if (m == 0xFF) {
      ++pos;
      continue;
    }
    pos += 2;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9) return jpgd_fail(err, errn, "EOI before any scan");
    if (pos + 2 > n) return jpgd_fail(err, errn, "the header runs past the end of the file (truncated header)");
    const long long len = (d[pos] << 8) | d[pos + 1];
    if (len < 2 || pos + len > n) return jpgd_fail(err, errn, "the header runs past the end of the file (truncated header)");
    const uint8_t* s = d + pos + 2;
    const int sl = (int)len - 2;
    pos += len;
    if (m == 0xC2) return jpgd_fail(err, errn, "progressive (SOF2) is not baseline");
    if (m == 0xC1) return jpgd_fail(err, errn, "extended sequential (SOF1) is not baseline");
    if (m == 0xC3 || m == 0xC7) return jpgd_fail(err, errn, "lossless (SOF%d) is not baseline", m - 0xC0);
    if (m == 0xC5 || m == 0xC6) return jpgd_fail(err, errn, "differential (SOF%d) is not baseline", m - 0xC0);
    if (m == 0xCC || (m >= 0xC9 && m <= 0xCF)) return jpgd_fail(err, errn, "arithmetic coding (marker 0x%02X)", m);
    if (m == 0xDB) {
      for (int at = 0; at < sl;) {
        const int pq = s[at] >> 4, tq = s[at] & 15, size = 64 * (pq ? 2 : 1);
        if (pq > 1 || tq > 3 || at + 1 + size > sl) return jpgd_fail(err, errn, "bad DQT segment");
        for (int i = 0; i < 64; ++i) qt[tq * 64 + zz[i]] = pq ? (uint16_t)((s[at + 1 + 2 * i] << 8) | s[at + 2 + 2 * i]) : s[at + 1 + i];
        have_q[tq] = true;
        at += 1 + size;
      }
    } else if (m == 0xC4) {
      for (int at = 0; at < sl;) {
        if (at + 17 > sl) return jpgd_fail(err, errn, "bad DHT segment");
        const int tc = s[at] >> 4, th = s[at] & 15;
        int cnt = 0;
        for (int i = 0; i < 16; ++i) cnt += s[at + 1 + i];
        if (tc > 1 || th > 3 || cnt > 256 || at + 17 + cnt > sl) return jpgd_fail(err, errn, "bad DHT segment");
        JpgdTable& t = huff[tc * 4 + th];
        t.have = true, t.n = cnt;
        memcpy(t.bits, s + at + 1, 16);
        memset(t.vals, 0, 256);
        memcpy(t.vals, s + at + 17, cnt);
        int32_t tmp[kJpgdHuffInts];
        if (!jpgd_derive(t, tmp)) return jpgd_fail(err, errn, "bad DHT segment (over-subscribed code lengths)");
        if (tc == 0)
          for (int i = 0; i < cnt; ++i)
            if (t.vals[i] > 15) return jpgd_fail(err, errn, "bad DHT segment (DC category above 15)");
        at += 17 + cnt;
      }
    } else if (m == 0xC0) {
      if (have_sof || sl < 6 || sl != 6 + 3 * s[5]) return jpgd_fail(err, errn, "bad or repeated SOF0 segment");
      if (s[0] != 8) return jpgd_fail(err, errn, "%d-bit samples (8-bit only)", s[0]);
      f->h = (s[1] << 8) | s[2], f->w = (s[3] << 8) | s[4], f->ncomp = s[5];
      if (f->ncomp != 1 && f->ncomp != 3) return jpgd_fail(err, errn, "%d components (1 or 3 only)", f->ncomp);
      if (f->h < 1 || f->h > kJpgdMaxSide || f->w < 1 || f->w > kJpgdMaxSide)
        return jpgd_fail(err, errn, "sides %d x %d outside 1 ... %d", f->h, f->w, kJpgdMaxSide);
      for (int i = 0; i < f->ncomp; ++i) {
        comp_id[i] = s[6 + 3 * i], comp_q[i] = s[8 + 3 * i];
        const int hv = s[7 + 3 * i];
        if (comp_q[i] > 3) return jpgd_fail(err, errn, "bad SOF0 segment (quantiser table id)");
        if (f->ncomp == 3 && (i == 0 ? (hv != 0x11 && hv != 0x21 && hv != 0x22) : hv != 0x11))
          return jpgd_fail(err, errn, "sampling factors %dx%d of component %d (4:4:4, 4:2:2 as 2x1 and 4:2:0 as 2x2 only)", hv >> 4, hv & 15, i);
        if (f->ncomp == 3 && i == 0) f->hs = hv >> 4, f->vs = hv & 15;
      }
      have_sof = true;
    } else if (m == 0xDD) {
      if (sl != 2) return jpgd_fail(err, errn, "bad DRI segment");
      f->restart = (s[0] << 8) | s[1];
    } else if (m == 0xDA) {
      if (!have_sof) return jpgd_fail(err, errn, "SOS before SOF0");
      if (sl < 1 || sl != 4 + 2 * s[0]) return jpgd_fail(err, errn, "bad SOS segment");
      if (s[0] != f->ncomp) return jpgd_fail(err, errn, "a scan of %d of %d components (multiple scans)", s[0], f->ncomp);
      memset(f->set, 0, sizeof(f->set));
      for (int i = 0; i < f->ncomp; ++i) {
        if (s[1 + 2 * i] != comp_id[i]) return jpgd_fail(err, errn, "the scan's components are not in the frame's order");
        const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
        if (!have_q[comp_q[i]]) return jpgd_fail(err, errn, "missing quantisation table %d", comp_q[i]);
        if (td > 3 || ta > 3 || !huff[td].have || !huff[4 + ta].have) return jpgd_fail(err, errn, "missing Huffman table (DC %d / AC %d)", td, ta);
        memcpy((uint16_t*)(f->set + 32 * i), &qt[comp_q[i] * 64], 128);
        jpgd_derive(huff[td], f->set + kJpgdSetHuff + (2 * i) * kJpgdHuffInts);
        jpgd_derive(huff[4 + ta], f->set + kJpgdSetHuff + (2 * i + 1) * kJpgdHuffInts);
      }
      const uint8_t* e = s + 1 + 2 * f->ncomp;
      if (e[0] != 0 || e[1] != 63 || e[2] != 0) return jpgd_fail(err, errn, "spectral selection or successive approximation in SOS (not baseline)");
      break;
    }
  }
  f->scan0 = pos;
  long long at = pos;
  for (;; ++at) {  // the first 0xFF followed by anything but 0x00, RSTn or 0xFF ends the scan
    const uint8_t* q = at < n ? (const uint8_t*)memchr(d + at, 0xFF, (size_t)(n - at)) : nullptr;
    if (!q || q + 1 >= d + n) {
      at = n;
      break;
    }
    at = q - d;
    const int c = q[1];
    if (c != 0 && c != 0xFF && !(c >= 0xD0 && c <= 0xD7)) break;
  }
  f->scan1 = at;
  while (at + 4 <= n && d[at] == 0xFF && d[at + 1] != 0xD9) {  // what follows the scan: another scan is refused
    if (d[at + 1] == 0xDA) return jpgd_fail(err, errn, "a second SOS (multiple scans)");
    at += 2 + ((d[at + 2] << 8) | d[at + 3]);
  }
  return 0;
}

inline size_t jpgd_plan_ints(int32_t n_frames) {  // room for every frame with a table set of its own
  return n_frames < 1 ? 0 : (size_t)JPGD_P_HEADER + (size_t)n_frames * (JPGD_F_INTS + kJpgdSetInts);
}

// ---------------------------------------------------------------- `work`: per frame of a group, every part 16-byte aligned
struct JpgdWork {
  size_t seg, coef, plane[3], frame;  // byte offsets inside a frame's share, and its size
  int pw, ph, cw, ch;                 // the planes' allocated sizes: whole blocks
  long long nblocks;
  size_t unst, table;  // with a frame on the sync or the split route: the longest such scan without its stuffing, the lane table
  int sync_lanes;      // the most lanes a frame on the sync route can need: the stuffed length bounds the true one.  0: no such frame
  int split_lanes;     // the same for the split route, whose table is the longer one
};
inline size_t jpgd_align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline JpgdWork jpgd_work(const int32_t* plan) {
  JpgdWork k{};
  const int mcux = plan[JPGD_P_MCUX], mcuy = plan[JPGD_P_MCUY];
  k.pw = mcux * 8 * plan[JPGD_P_HS], k.ph = mcuy * 8 * plan[JPGD_P_VS], k.cw = mcux * 8, k.ch = mcuy * 8;
  k.nblocks = (long long)mcux * mcuy * plan[JPGD_P_BPM];
  k.seg = 0;
  k.coef = jpgd_align16((size_t)plan[JPGD_P_MAXINT] * 2 * sizeof(int32_t));
  k.plane[0] = k.coef + (size_t)k.nblocks * 128;
  k.plane[1] = k.plane[0] + jpgd_align16((size_t)k.pw * k.ph);
  k.plane[2] = k.plane[1] + (plan[JPGD_P_NCOMP] == 3 ? jpgd_align16((size_t)k.cw * k.ch) : 0);
  k.frame = k.plane[2] + (plan[JPGD_P_NCOMP] == 3 ? jpgd_align16((size_t)k.cw * k.ch) : 0);
  long long scan = 0;
  for (int i = 0; i < plan[JPGD_P_N]; ++i) {
    const int32_t* r = plan + plan[JPGD_P_FRAMES] + i * JPGD_F_INTS;
    if (!r[JPGD_F_ROUTE]) continue;
    const long long bytes = r[JPGD_F_SCAN1] - r[JPGD_F_SCAN0];
    scan = std::max(scan, bytes);
    if (r[JPGD_F_ROUTE] > 0)
      k.sync_lanes = (int)std::max<long long>(k.sync_lanes, std::min<long long>(kJpgdSyncLanes, std::max<long long>(1, (bytes + r[JPGD_F_ROUTE] - 1) / r[JPGD_F_ROUTE])));
    else  // a lane per interval and the bytes' share: jpgd_split_sub
      k.split_lanes = (int)std::max<long long>(k.split_lanes, std::min<long long>(kJpgdSyncLanes, r[JPGD_F_NINT] + (bytes - r[JPGD_F_ROUTE] - 1) / -r[JPGD_F_ROUTE]));
  }
  if (k.sync_lanes || k.split_lanes) {
    k.unst = k.frame;
    k.table = k.unst + jpgd_align16((size_t)scan);
    k.frame = k.table + jpgd_align16((k.split_lanes ? kJpgdSplitTableInts : kJpgdTableInts) * sizeof(int32_t));
  }
  return k;
}
inline bool jpgd_plan_ok(const int32_t* plan) { return plan && plan[JPGD_P_MAGIC] == kJpgdMagic && plan[JPGD_P_N] >= 1; }

// n files in host memory -> the plan.  1 with the reason (and the frame) in err.  entropy: 0 every frame on the interval route,
// 1 the sync route for every frame with one interval, 2 for those whose scan has at least kJpgdSyncLanes kJpgdSyncBytes bytes,
// 3 the split route for every frame with at most kJpgdSplitIntervals intervals; sync_bytes: the shortest subsequence (0: kJpgdSyncBytes).
inline int jpgd_build_plan(const uint8_t* files, const int64_t* offsets, int32_t n, int32_t* plan, size_t plan_ints, char* err, size_t errn,
                           int32_t entropy = 0, int32_t sync_bytes = 0) {
  if (entropy < 0 || entropy > 3) return jpgd_fail(err, errn, "entropy (%d) must be 0 (interval), 1 (sync), 2 (auto) or 3 (split)", entropy);
  if (sync_bytes < 0 || sync_bytes > kJpgdSyncMaxBytes) return jpgd_fail(err, errn, "sync_bytes (%d) must be 0 (the default, %d) or 1 ... %d", sync_bytes, kJpgdSyncBytes, kJpgdSyncMaxBytes);
  if (plan_ints < jpgd_plan_ints(n)) return jpgd_fail(err, errn, "plan_ints %zu < float_jpg_decode_plan_ints(%d) = %zu", plan_ints, n, jpgd_plan_ints(n));
  memset(plan, 0, JPGD_P_HEADER * sizeof(int32_t));
  const int frames_at = JPGD_P_HEADER, sets_at = JPGD_P_HEADER + n * JPGD_F_INTS;
  int nsets = 0, maxint = 1;
  std::vector<JpgdFile> one(1);
  JpgdFile& f = one[0];
  for (int i = 0; i < n; ++i) {
    const long long len = offsets[i + 1] - offsets[i];
    if (offsets[i] < 0 || len < 0 || len >= (1ll << 31)) return jpgd_fail(err, errn, "frame %d: offsets must ascend, files stay below 2 GiB", i);
    f = JpgdFile();
    char why[200];
    if (jpgd_parse(files + offsets[i], len, &f, why, sizeof(why))) return jpgd_fail(err, errn, "frame %d: %s", i, why);
    if (i == 0) {
      plan[JPGD_P_H] = f.h, plan[JPGD_P_W] = f.w, plan[JPGD_P_NCOMP] = f.ncomp, plan[JPGD_P_HS] = f.hs, plan[JPGD_P_VS] = f.vs;
      plan[JPGD_P_MCUX] = (f.w + 8 * f.hs - 1) / (8 * f.hs), plan[JPGD_P_MCUY] = (f.h + 8 * f.vs - 1) / (8 * f.vs);
      plan[JPGD_P_BPM] = f.hs * f.vs + f.ncomp - 1;
    } else if (f.h != plan[JPGD_P_H] || f.w != plan[JPGD_P_W] || f.ncomp != plan[JPGD_P_NCOMP] || f.hs != plan[JPGD_P_HS] || f.vs != plan[JPGD_P_VS]) {
      return jpgd_fail(err, errn, "frame %d is %d x %d with %d components sampled %dx%d, frame 0 is %d x %d with %d sampled %dx%d: one call, one geometry", i,
                       f.h, f.w, f.ncomp, f.hs, f.vs, plan[JPGD_P_H], plan[JPGD_P_W], plan[JPGD_P_NCOMP], plan[JPGD_P_HS], plan[JPGD_P_VS]);
    }
    const int nmcu = plan[JPGD_P_MCUX] * plan[JPGD_P_MCUY];
    const int span = f.restart > 0 && f.restart < nmcu ? f.restart : nmcu;
    int set = 0;
    while (set < nsets && memcmp(plan + sets_at + set * kJpgdSetInts, f.set, sizeof(f.set))) ++set;
    if (set == nsets) memcpy(plan + sets_at + (nsets++) * kJpgdSetInts, f.set, sizeof(f.set));
    int32_t* r = plan + frames_at + i * JPGD_F_INTS;
    memset(r, 0, JPGD_F_INTS * sizeof(int32_t));
    r[JPGD_F_SCAN0] = (int32_t)f.scan0, r[JPGD_F_SCAN1] = (int32_t)f.scan1, r[JPGD_F_SPAN] = span, r[JPGD_F_NINT] = (nmcu + span - 1) / span;
    r[JPGD_F_SET] = set;
    const long long scan = f.scan1 - f.scan0;
    if (entropy == 3) {
      if (r[JPGD_F_NINT] <= kJpgdSplitIntervals && scan < kJpgdSyncScan) r[JPGD_F_ROUTE] = -(sync_bytes ? sync_bytes : kJpgdSyncBytes);
    } else if (entropy && r[JPGD_F_NINT] == 1 && scan < kJpgdSyncScan && (entropy == 1 || scan >= kJpgdSyncLanes * kJpgdSyncBytes)) {
      r[JPGD_F_ROUTE] = sync_bytes ? sync_bytes : kJpgdSyncBytes;
    }
    maxint = std::max(maxint, r[JPGD_F_NINT]);
  }
  plan[JPGD_P_MAGIC] = kJpgdMagic, plan[JPGD_P_N] = n, plan[JPGD_P_NSETS] = nsets, plan[JPGD_P_MAXINT] = maxint;
  plan[JPGD_P_FRAMES] = frames_at, plan[JPGD_P_SETS] = sets_at, plan[JPGD_P_INTS] = sets_at + nsets * kJpgdSetInts;
  const unsigned long long per = jpgd_work(plan).frame;
  plan[JPGD_P_GROUP] = (int32_t)std::max<unsigned long long>(1, std::min<unsigned long long>(kJpgdGroup, kJpgdGroupBytes / per));
  return 0;
}

// ---------------------------------------------------------------- the host path: frame i of the plan through the rule header
// The sync route over the segment [p, end), the kernels' steps with the lanes as a plain loop: unstuff, relax until no exit
// changes (n_sub rounds at most), prefix, write.  coef: nblocks zeroed blocks.  Returns the BAD_CODE and PAST_END bits.
inline void jpgd_host_unstuff(const uint8_t* p, const uint8_t* end, std::vector<uint8_t>& u) {
  for (const uint8_t* q = p; q < end; ++q)
    if (!(*q == 0 && q > p && q[-1] == 0xFF)) u.push_back(*q);
}
// one chain: `len` bytes without stuffing as nsub subsequences of S bytes, nblocks blocks from coef on
inline int jpgd_host_lanes(const uint8_t* u, uint32_t len, uint32_t S, uint32_t nsub, const int32_t* set, int hv, int bpm, long long nblocks, int16_t* coef) {
  std::vector<JpgdRun> entry(nsub), exit(nsub);
  const auto skip = [&](JpgdRaw& b, int c, int32_t& pred, uint32_t) { return jpgd_block(b, jpgd_huff(set, c, 0), jpgd_huff(set, c, 1), pred, JpgdNoCoef()); };
  JpgdRaw b;
  for (uint32_t r = 0; r < nsub; ++r) {
    bool changed = false;
    for (uint32_t i = nsub; i-- > 0;) {  // downwards: lane i reads the exit that lane i - 1 had BEFORE this round
      if (r == 0) entry[i] = JpgdRun{8u * i * S, 0, 0u, {0, 0, 0}};
      else if (i == 0 || (exit[i - 1].p == entry[i].p && exit[i - 1].j == entry[i].j)) continue;
      else if (exit[i - 1].p == kJpgdDead && r < i) {  // not final before round i: the lane keeps its entry, the loop goes on
        changed = true;
        continue;
      } else entry[i].p = exit[i - 1].p, entry[i].j = exit[i - 1].j;
      JpgdRun x = entry[i];
      jpgd_sync_run(b, u, len, jpgd_sync_end(i, S, len), false, 0xFFFFFFFFu, hv, bpm, x, skip);
      changed = changed || r == 0 || x.p != exit[i].p || x.j != exit[i].j;
      exit[i] = x;
    }
    if (!changed) break;
  }
  int st = 0;
  long long first = 0;
  int32_t pred[3] = {0, 0, 0};
  for (uint32_t i = 0; i < nsub && first < nblocks && entry[i].p != kJpgdDead; ++i) {  // a dead entry: the chain ended, the rest keeps its zeros
    JpgdRun x{entry[i].p, entry[i].j, 0u, {pred[0], pred[1], pred[2]}};
    bool bad = false;
    jpgd_sync_run(b, u, len, jpgd_sync_end(i, S, len), i == nsub - 1, (uint32_t)(nblocks - first), hv, bpm, x, [&](JpgdRaw& bits, int c, int32_t& pr, uint32_t k) {
      int16_t* blk = coef + (size_t)(first + k) * 64;
      if (jpgd_block(bits, jpgd_huff(set, c, 0), jpgd_huff(set, c, 1), pr, blk)) return true;
      memset(blk, 0, 128);
      bad = true;
      return false;
    });
    if (bad) st |= JPGD_ST_BAD_CODE;
    if (jpgd_past_end(b)) st |= JPGD_ST_PAST_END;
    // the prefix of the kernels, taken from the relaxation's record and not from this run, as the table is
    first += exit[i].n;
    for (int c = 0; c < 3; ++c) pred[c] = jpgd_add(pred[c], exit[i].dc[c]);
    if (bad) break;
  }
  return st;
}
inline int jpgd_host_sync(const uint8_t* p, const uint8_t* end, const int32_t* set, int hv, int bpm, uint32_t sync_bytes, long long nblocks, int16_t* coef) {
  std::vector<uint8_t> u;
  jpgd_host_unstuff(p, end, u);
  const uint32_t len = (uint32_t)u.size(), S = jpgd_sync_sub(len, sync_bytes);
  return jpgd_host_lanes(u.data(), len, S, jpgd_sync_lanes(len, S), set, hv, bpm, nblocks, coef);
}
// The split route over the interval table seg[2 n_int] (-1: no segment): every segment into one copy, the lanes dealt out by
// jpgd_split_sub, then interval by interval a chain of its own - the kernels relax all intervals in the same rounds.
inline int jpgd_host_split(const uint8_t* file, const int32_t* seg, int n_int, int span, int nmcu, const int32_t* set, int hv, int bpm, uint32_t sync_bytes,
                           int16_t* coef) {
  std::vector<uint8_t> u;
  std::vector<uint32_t> start((size_t)n_int + 1, 0);
  uint32_t present = 0;
  for (int k = 0; k < n_int; ++k) {
    if (seg[2 * k] >= 0) jpgd_host_unstuff(file + seg[2 * k], file + seg[2 * k + 1], u), ++present;
    start[k + 1] = (uint32_t)u.size();
  }
  const uint32_t S = jpgd_split_sub((uint32_t)u.size(), present, sync_bytes);
  int st = 0;
  for (int k = 0; k < n_int; ++k) {
    if (seg[2 * k] < 0) continue;
    const uint32_t len = start[k + 1] - start[k];
    st |= jpgd_host_lanes(u.data() + start[k], len, S, jpgd_split_lanes(len, S), set, hv, bpm, jpgd_split_blocks(k, span, nmcu, bpm),
                          coef + (size_t)k * span * bpm * 64);
  }
  return st;
}

// rgb: h w 3 bytes.  scratch comes from the heap; the stages and their order are the kernels'.
inline void jpgd_host_frame(const uint8_t* files, const int64_t* offsets, const int32_t* plan, int i, uint8_t* rgb, int32_t* status) {
  const int32_t* fr = plan + plan[JPGD_P_FRAMES] + i * JPGD_F_INTS;
  const int32_t* set = plan + plan[JPGD_P_SETS] + fr[JPGD_F_SET] * kJpgdSetInts;
  const uint8_t* file = files + offsets[i];
  const JpgdWork k = jpgd_work(plan);
  const int H = plan[JPGD_P_H], W = plan[JPGD_P_W], nc = plan[JPGD_P_NCOMP], hs = plan[JPGD_P_HS], vs = plan[JPGD_P_VS];
  const int mcux = plan[JPGD_P_MCUX], bpm = plan[JPGD_P_BPM], nmcu = mcux * plan[JPGD_P_MCUY], n_int = fr[JPGD_F_NINT], span = fr[JPGD_F_SPAN];
  int st = 0;
  // restart scan
  std::vector<int32_t> seg((size_t)2 * n_int, -1);
  int cnt = 0;
  seg[0] = fr[JPGD_F_SCAN0];
  for (int p = fr[JPGD_F_SCAN0]; p + 1 < fr[JPGD_F_SCAN1]; ++p)
    if (file[p] == 0xFF && (file[p + 1] & 0xF8) == 0xD0) {
      if (cnt < n_int) seg[2 * cnt + 1] = p;
      if (cnt + 1 < n_int) seg[2 * cnt + 2] = p + 2;
      ++cnt;
    }
  if (cnt < n_int) seg[2 * cnt + 1] = fr[JPGD_F_SCAN1];
  if (cnt != n_int - 1) st |= JPGD_ST_RESTARTS;
  // entropy decode
  std::vector<int16_t> coef((size_t)k.nblocks * 64, 0);
  if (fr[JPGD_F_ROUTE] < 0) st |= jpgd_host_split(file, seg.data(), n_int, span, nmcu, set, hs * vs, bpm, (uint32_t)-fr[JPGD_F_ROUTE], coef.data());
  if (fr[JPGD_F_ROUTE] > 0) st |= jpgd_host_sync(file + seg[0], file + seg[1], set, hs * vs, bpm, (uint32_t)fr[JPGD_F_ROUTE], k.nblocks, coef.data());
  for (int iv = 0; iv < n_int && !fr[JPGD_F_ROUTE]; ++iv) {
    if (seg[2 * iv] < 0) continue;  // no segment: the interval keeps its zeros
    JpgdBits b;
    jpgd_bits_open(b, file + seg[2 * iv], file + seg[2 * iv + 1]);
    int32_t pred[3] = {0, 0, 0};
    bool ok = true;
    for (int m = iv * span; ok && m < std::min((iv + 1) * span, nmcu); ++m)
      for (int j = 0; ok && j < bpm; ++j) {
        const int c = j < hs * vs ? 0 : j - hs * vs + 1;
        int16_t* blk = &coef[((size_t)m * bpm + j) * 64];
        ok = jpgd_block(b, jpgd_huff(set, c, 0), jpgd_huff(set, c, 1), pred[c], blk);
        if (!ok) memset(blk, 0, 128);
      }
    if (!ok) st |= JPGD_ST_BAD_CODE;
    if (jpgd_past_end(b)) st |= JPGD_ST_PAST_END;
  }
  // IDCT into the planes
  std::vector<uint8_t> planes(k.frame - k.plane[0]);
  uint8_t* pl[3] = {planes.data(), planes.data() + (k.plane[1] - k.plane[0]), planes.data() + (k.plane[2] - k.plane[0])};
  for (long long g = 0; g < k.nblocks; ++g) {
    const int m = (int)(g / bpm), j = (int)(g % bpm), my = m / mcux, mx = m % mcux;
    const int c = j < hs * vs ? 0 : j - hs * vs + 1;
    const int by = c ? my : my * vs + j / hs, bx = c ? mx : mx * hs + j % hs, stride = c ? k.cw : k.pw;
    const uint16_t* q = (const uint16_t*)(set + 32 * c);
    int32_t ws[64];
    for (int col = 0; col < 8; ++col) {
      int32_t v[8];
      for (int r = 0; r < 8; ++r) v[r] = jpgd_mul(coef[(size_t)g * 64 + r * 8 + col], q[r * 8 + col]);
      jpgd_idct8<11>(v);
      for (int r = 0; r < 8; ++r) ws[r * 8 + col] = v[r];
    }
    for (int r = 0; r < 8; ++r) {
      jpgd_idct8<18>(ws + r * 8);
      for (int col = 0; col < 8; ++col) pl[c][(size_t)(by * 8 + r) * stride + bx * 8 + col] = jpgd_sample(ws[r * 8 + col]);
    }
  }
  // upsample, convert, crop
  const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      uint8_t* o = rgb + ((size_t)y * W + x) * 3;
      const int32_t Y = pl[0][(size_t)y * k.pw + x];
      if (nc == 1) o[0] = o[1] = o[2] = (uint8_t)Y;
      else jpgd_rgb(Y, jpgd_chroma(pl[1], k.cw, cw, ch, hs, vs, x, y), jpgd_chroma(pl[2], k.cw, cw, ch, hs, vs, x, y), o);
    }
  *status = st;
}
