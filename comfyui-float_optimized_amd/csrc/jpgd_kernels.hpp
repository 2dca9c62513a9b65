// Kernels of float_jpg_decode: baseline JPEG files in HBM -> 8-bit RGB frames, bitwise host_models.jpeg_decode_rgb8.  Four
// launches per group of frames, all reading the DEVICE plan (jpgd_rule.hpp has its layout and the arithmetic):
//   jpgd_scan_kernel     one workgroup per frame walks the scan bytes, a byte pair per lane, and compacts the RSTn positions in
//                        order (wave ballot + prefix count) into the frame's interval table; writes the frame's status word.
//   jpgd_entropy_kernel  one restart interval per lane; the frame's table set sits in LDS once per workgroup, a lane gathers a
//                        block in an LDS row of its own (33 dwords apart: lanes fall into different banks) and hands it to the
//                        coefficient buffer as eight 16-byte stores.
//   (frames on the sync route - a scan without restart markers over up to 1024 lanes - are skipped by it and go through
//   jpgd_unstuff_kernel, jpgd_relax_kernel and jpgd_sync_write_kernel instead: three more launches, described where they are;
//   frames on the split route - the intervals of a scan WITH restart markers over up to 1024 lanes - through the jpgd_split_*
//   forms of the three)
//   jpgd_idct_kernel     32 blocks per workgroup: coefficients into LDS by 16-byte loads, pass 1 down the columns (dequantising),
//                        the block transposed through LDS, pass 2 along the rows, 8 samples per lane as one 8-byte store.
//   jpgd_rgb_kernel      4 pixels per lane: fancy upsampling from the chroma planes, colour conversion, one 12-byte store.
#pragma once
#include "common.hpp"
#include "jpgd_rule.hpp"

constexpr int kJpgdScanThreads = 256, kJpgdLanes = 64, kJpgdIdctBlocks = 32, kJpgdRgbThreads = 64;
constexpr int kJpgdRowDwords = 33;   // a lane's block in the entropy kernel: 32 dwords + 1, so that lane l starts in bank l
constexpr int kJpgdCoefDwords = 36;  // a block's coefficients in the IDCT kernel: 32 dwords + 4 (16-byte aligned, 8 blocks of a wave in 8 bank groups)
constexpr int kJpgdWsRow = 9, kJpgdWsBlock = 72;  // pass 1's result: rows 8 + 1 dwords apart, blocks 72

struct JpgdLaunch {  // what the host read from its copy of the plan
  int frame0, frames;  // the group
  unsigned long long seg, coef, plane[3], frame;  // byte offsets inside a frame's share of `work`, and its size
  int pw, cw;          // row strides of the luma and chroma planes
  long long nblocks;
  unsigned long long unst, table;  // the sync route's share: a scan without its stuffing, the lane table
};

// LDS words that are written as one type and read as another (a block's int16 coefficients, moved as dwords)
typedef int __attribute__((may_alias)) jpgd_word;
typedef short __attribute__((may_alias)) jpgd_half;
typedef unsigned short __attribute__((may_alias)) jpgd_uhalf;

__device__ __forceinline__ const int* jpgd_frame(const int* plan, int f) { return plan + plan[JPGD_P_FRAMES] + f * JPGD_F_INTS; }

__global__ __launch_bounds__(kJpgdScanThreads) void jpgd_scan_kernel(const uint8_t* __restrict__ files, const long long* __restrict__ offsets,
                                                                    const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work,
                                                                    int* __restrict__ status) {
  __shared__ int wave_cnt[kJpgdScanThreads / 64];
  const int f = L.frame0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* fr = jpgd_frame(plan, f);
  const uint8_t* file = files + offsets[f];
  const int s0 = fr[JPGD_F_SCAN0], s1 = fr[JPGD_F_SCAN1], n_int = fr[JPGD_F_NINT];
  int* seg = (int*)(work + (size_t)blockIdx.x * L.frame + L.seg);
  int total = 0;  // markers so far, the same in every lane
  for (int base = s0; base < s1; base += kJpgdScanThreads) {
    const int p = base + tid;
    const bool mark = p + 1 < s1 && file[p] == 0xFF && (file[p + 1] & 0xF8) == 0xD0;
    const unsigned long long vote = __ballot(mark);
    if (lane == 0) wave_cnt[wave] = __popcll(vote);
    __syncthreads();
    int before = total, all = 0;
#pragma unroll
    for (int w = 0; w < kJpgdScanThreads / 64; ++w) {
      const int c = wave_cnt[w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (mark) {
      const int k = before + __popcll(vote & ((1ull << lane) - 1ull));  // this marker's number: it ends interval k, interval k + 1 follows
      if (k < n_int) seg[2 * k + 1] = p;
      if (k + 1 < n_int) seg[2 * k + 2] = p + 2;
    }
    total += all;
    __syncthreads();
  }
  if (tid == 0) {
    seg[0] = s0;
    if (total < n_int) seg[2 * total + 1] = s1;
    status[f] = total == n_int - 1 ? 0 : JPGD_ST_RESTARTS;
  }
  for (int k = total + 1 + tid; k < n_int; k += kJpgdScanThreads) seg[2 * k] = -1, seg[2 * k + 1] = -1;  // no segment: an all-zero interval
}

__global__ __launch_bounds__(kJpgdLanes) void jpgd_entropy_kernel(const uint8_t* __restrict__ files, const long long* __restrict__ offsets,
                                                                 const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work,
                                                                 int* __restrict__ status) {
  __shared__ int set[kJpgdSetInts];
  __shared__ jpgd_word rows[kJpgdLanes * kJpgdRowDwords];
  const int f = L.frame0 + blockIdx.y, lane = threadIdx.x;
  const int* fr = jpgd_frame(plan, f);
  if (fr[JPGD_F_ROUTE]) return;  // the sync route's frame
  const int* gset = plan + plan[JPGD_P_SETS] + fr[JPGD_F_SET] * kJpgdSetInts;
  for (int i = lane; i < kJpgdSetInts; i += kJpgdLanes) set[i] = gset[i];
  __syncthreads();
  const int iv = blockIdx.x * kJpgdLanes + lane, n_int = fr[JPGD_F_NINT];
  if (iv >= n_int) return;
  uint8_t* mine = work + (size_t)blockIdx.y * L.frame;
  const int* seg = (const int*)(mine + L.seg);
  int16_t* coef = (int16_t*)(mine + L.coef);
  const int hv = plan[JPGD_P_HS] * plan[JPGD_P_VS], bpm = plan[JPGD_P_BPM], span = fr[JPGD_F_SPAN];
  const int nmcu = plan[JPGD_P_MCUX] * plan[JPGD_P_MCUY], m1 = min((iv + 1) * span, nmcu);
  const uint8_t* file = files + offsets[f];
  const int b0 = seg[2 * iv], b1 = seg[2 * iv + 1];
  jpgd_word* row = rows + lane * kJpgdRowDwords;
  JpgdBits b;
  jpgd_bits_open(b, file + max(b0, 0), file + max(b1, 0));
  bool ok = b0 >= 0;
  int st = 0;
  int32_t pred[3] = {0, 0, 0};
  for (int m = iv * span; m < m1; ++m)
    for (int j = 0; j < bpm; ++j) {
      const int c = j < hv ? 0 : j - hv + 1;
#pragma unroll
      for (int i = 0; i < 32; ++i) row[i] = 0;
      if (ok) {
        int32_t& pr = c == 0 ? pred[0] : c == 1 ? pred[1] : pred[2];
        ok = jpgd_block(b, jpgd_huff(set, c, 0), jpgd_huff(set, c, 1), pr, (jpgd_half*)row);
        if (!ok) {
          st |= JPGD_ST_BAD_CODE;
#pragma unroll
          for (int i = 0; i < 32; ++i) row[i] = 0;
        }
      }
      uint4* dst = (uint4*)(coef + ((size_t)m * bpm + j) * 64);
#pragma unroll
      for (int i = 0; i < 8; ++i) dst[i] = uint4{(unsigned)row[4 * i], (unsigned)row[4 * i + 1], (unsigned)row[4 * i + 2], (unsigned)row[4 * i + 3]};
    }
  if (b0 >= 0 && jpgd_past_end(b)) st |= JPGD_ST_PAST_END;
  if (st) atomicOr(status + f, st);
}

// ---------------------------------------------------------------- the sync route (jpgd_rule.hpp): frames whose ROUTE word is set
// The frame's one segment [seg[0], seg[1]) - jpgd_scan_kernel cut it - without the 0x00 behind a 0xFF: a byte per lane, wave
// ballot + prefix count as in the marker compaction.  Writes the table's header: the length, S and n_sub.
__global__ __launch_bounds__(kJpgdSyncLanes) void jpgd_unstuff_kernel(const uint8_t* __restrict__ files, const long long* __restrict__ offsets,
                                                                     const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work) {
  constexpr int kWaves = kJpgdSyncLanes / 64;
  __shared__ int wave_cnt[2][kWaves];  // iteration k + 2 writes a row only behind iteration k + 1's barrier: all have read k's
  const int f = L.frame0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* fr = jpgd_frame(plan, f);
  if (fr[JPGD_F_ROUTE] <= 0) return;  // the interval route's frame, or the split route's
  uint8_t* mine = work + (size_t)blockIdx.x * L.frame;
  const int* seg = (const int*)(mine + L.seg);
  const uint8_t* file = files + offsets[f];
  uint8_t* u = mine + L.unst;
  const int b0 = seg[0], b1 = seg[1];
  int total = 0;  // bytes kept so far, the same in every lane
  for (int base = b0, it = 0; base < b1; base += kJpgdSyncLanes, it ^= 1) {
    const int q = base + tid;
    const uint8_t v = q < b1 ? file[q] : 0;
    const bool keep = q < b1 && !(v == 0 && q > b0 && file[q - 1] == 0xFF);
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) wave_cnt[it][wave] = __popcll(vote);
    __syncthreads();
    int before = total, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = wave_cnt[it][w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (keep) u[before + __popcll(vote & ((1ull << lane) - 1ull))] = v;
    total += all;
  }
  if (tid == 0) {
    int* tab = (int*)(mine + L.table);
    const uint32_t S = jpgd_sync_sub((uint32_t)total, (uint32_t)fr[JPGD_F_ROUTE]);
    tab[JPGD_T_LEN] = total, tab[JPGD_T_S] = (int)S, tab[JPGD_T_NSUB] = (int)jpgd_sync_lanes((uint32_t)total, S);
  }
}

// One workgroup per frame, lane = subsequence, the exits in LDS.  Round 0 decodes from the guesses (8 i S, 0) - lane 0 from the
// true (0, 0) -, round r only where the predecessor's exit is not the entry last used; nothing is stored.  A dead exit is taken
// over in round i and not before, when lane i - 1 is final: a guess that ran into a bad code (one lane in six does, on 1080p
// frames) would otherwise kill every guess behind it, and the chain would be walked lane by lane.  The loop ends with the first
// round in which no exit changes and no lane waits, after n_sub rounds at the latest.  Then an exclusive prefix over the lanes of the block
// counts and DC sums gives every lane its first block and predictions: the lane table.
__global__ __launch_bounds__(kJpgdSyncLanes) void jpgd_relax_kernel(const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work) {
  __shared__ int set[kJpgdSetInts];
  __shared__ uint32_t xp[kJpgdSyncLanes], xn[kJpgdSyncLanes];
  __shared__ int xj[kJpgdSyncLanes], xd[3][kJpgdSyncLanes];
  const int f = L.frame0 + blockIdx.x, i = threadIdx.x;
  const int* fr = jpgd_frame(plan, f);
  if (fr[JPGD_F_ROUTE] <= 0) return;  // the interval route's frame, or the split route's
  const int* gset = plan + plan[JPGD_P_SETS] + fr[JPGD_F_SET] * kJpgdSetInts;
  for (int k = i; k < kJpgdSetInts; k += kJpgdSyncLanes) set[k] = gset[k];
  uint8_t* mine = work + (size_t)blockIdx.x * L.frame;
  const uint8_t* u = mine + L.unst;
  int* tab = (int*)(mine + L.table);
  const uint32_t len = (uint32_t)tab[JPGD_T_LEN], S = (uint32_t)tab[JPGD_T_S];
  const int nsub = tab[JPGD_T_NSUB], hv = plan[JPGD_P_HS] * plan[JPGD_P_VS], bpm = plan[JPGD_P_BPM];
  const bool active = i < nsub;
  const uint32_t end = jpgd_sync_end((uint32_t)i, S, len);
  uint32_t entry_p = 8u * (uint32_t)i * S;
  int entry_j = 0, rounds = 0;
  xp[i] = kJpgdDead, xj[i] = 0, xn[i] = 0, xd[0][i] = 0, xd[1][i] = 0, xd[2][i] = 0;
  __syncthreads();
  bool need = active, wait = false;
  for (int r = 0; r < nsub; ++r) {
    bool changed = wait;
    if (need) {
      JpgdRun x{entry_p, entry_j, 0u, {0, 0, 0}};
      JpgdRaw b;
      jpgd_sync_run(b, u, len, end, false, 0xFFFFFFFFu, hv, bpm, x, [&](JpgdRaw& bits, int c, int32_t& pred, uint32_t) {
        return jpgd_block(bits, jpgd_huff(set, c, 0), jpgd_huff(set, c, 1), pred, JpgdNoCoef());
      });
      changed = r == 0 || x.p != xp[i] || x.j != xj[i];
      xp[i] = x.p, xj[i] = x.j, xn[i] = x.n, xd[0][i] = x.dc[0], xd[1][i] = x.dc[1], xd[2][i] = x.dc[2];
    }
    ++rounds;
    if (!__syncthreads_or(changed)) break;
    need = wait = false;
    if (active && i > 0 && (xp[i - 1] != entry_p || xj[i - 1] != entry_j)) {
      if (xp[i - 1] == kJpgdDead && r + 1 < i) wait = true;  // a guess ran into a bad code: not final before round i
      else entry_p = xp[i - 1], entry_j = xj[i - 1], need = true;
    }
    __syncthreads();  // every exit is read before the round rewrites it
  }
  __syncthreads();
  const uint32_t own_n = xn[i];
  const int own_d[3] = {xd[0][i], xd[1][i], xd[2][i]};
  const bool dead = xp[nsub - 1] == kJpgdDead;
  for (int off = 1; off < kJpgdSyncLanes; off <<= 1) {  // inclusive prefix, in place
    const bool has = i >= off;
    const uint32_t an = has ? xn[i - off] : 0u;
    const int a0 = has ? xd[0][i - off] : 0, a1 = has ? xd[1][i - off] : 0, a2 = has ? xd[2][i - off] : 0;
    __syncthreads();
    xn[i] += an, xd[0][i] = jpgd_add(xd[0][i], a0), xd[1][i] = jpgd_add(xd[1][i], a1), xd[2][i] = jpgd_add(xd[2][i], a2);
    __syncthreads();
  }
  if (active) {
    int* e = tab + JPGD_T_HEADER + i * JPGD_T_LANE;
    e[0] = (int)entry_p, e[1] = entry_j, e[2] = (int)(xn[i] - own_n);
    e[3] = jpgd_sub(xd[0][i], own_d[0]), e[4] = jpgd_sub(xd[1][i], own_d[1]), e[5] = jpgd_sub(xd[2][i], own_d[2]);
  }
  if (i == 0) {  // a chain that died inside the data: every block from the bad one on is zero
    const long long good = xn[kJpgdSyncLanes - 1];
    tab[JPGD_T_ZERO] = (int)(dead && good < L.nblocks ? good : L.nblocks), tab[JPGD_T_ROUNDS] = rounds;
  }
}

// The write pass, jpgd_entropy_kernel's shape: a lane decodes its owned blocks once more, from its table entry, into an LDS row
// and the coefficient buffer, and stops at block nblocks.  The last lane goes on past the data on zero bits.  A bad code on
// the chain ends it; the blocks from there on are zeroed by all lanes of the launch when the relaxation saw the chain die, and
// by the lane itself when it died on the zero bits behind the data, which no lane owns.
__global__ __launch_bounds__(kJpgdLanes) void jpgd_sync_write_kernel(const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work,
                                                                    int* __restrict__ status) {
  __shared__ int set[kJpgdSetInts];
  __shared__ jpgd_word rows[kJpgdLanes * kJpgdRowDwords];
  const int f = L.frame0 + blockIdx.y, lane = threadIdx.x;
  const int* fr = jpgd_frame(plan, f);
  if (fr[JPGD_F_ROUTE] <= 0) return;  // the interval route's frame, or the split route's
  const int* gset = plan + plan[JPGD_P_SETS] + fr[JPGD_F_SET] * kJpgdSetInts;
  for (int k = lane; k < kJpgdSetInts; k += kJpgdLanes) set[k] = gset[k];
  __syncthreads();
  uint8_t* mine = work + (size_t)blockIdx.y * L.frame;
  const int* tab = (const int*)(mine + L.table);
  int16_t* coef = (int16_t*)(mine + L.coef);
  const uint32_t len = (uint32_t)tab[JPGD_T_LEN], S = (uint32_t)tab[JPGD_T_S];
  const int nsub = tab[JPGD_T_NSUB], i = blockIdx.x * kJpgdLanes + lane;
  const long long zero_from = tab[JPGD_T_ZERO];
  const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
  if (i < nsub) {
    const int* e = tab + JPGD_T_HEADER + i * JPGD_T_LANE;
    const long long first = (uint32_t)e[2];
    if ((uint32_t)e[0] != kJpgdDead && first < L.nblocks) {
      jpgd_word* row = rows + lane * kJpgdRowDwords;
      JpgdRun x{(uint32_t)e[0], e[1], 0u, {e[3], e[4], e[5]}};
      JpgdRaw b;
      bool bad = false;
      jpgd_sync_run(b, mine + L.unst, len, jpgd_sync_end((uint32_t)i, S, len), i == nsub - 1, (uint32_t)(L.nblocks - first), plan[JPGD_P_HS] * plan[JPGD_P_VS],
                    plan[JPGD_P_BPM], x, [&](JpgdRaw& bits, int c, int32_t& pred, uint32_t k) {
                      jpgd_word* r = row;  // the captured pointer, once
#pragma unroll
                      for (int w = 0; w < 32; ++w) r[w] = 0;
                      if (!jpgd_block(bits, jpgd_huff(set, c, 0), jpgd_huff(set, c, 1), pred, (jpgd_half*)r)) {
                        bad = true;
                        return false;
                      }
                      uint4* dst = (uint4*)(coef + (size_t)(first + k) * 64);
#pragma unroll
                      for (int w = 0; w < 8; ++w) dst[w] = uint4{(unsigned)r[4 * w], (unsigned)r[4 * w + 1], (unsigned)r[4 * w + 2], (unsigned)r[4 * w + 3]};
                      return true;
                    });
      int st = jpgd_past_end(b) ? JPGD_ST_PAST_END : 0;
      if (bad) {
        st |= JPGD_ST_BAD_CODE;
        if (zero_from == L.nblocks)  // died behind the data
          for (long long g = first + x.n; g < L.nblocks; ++g)
#pragma unroll
            for (int w = 0; w < 8; ++w) ((uint4*)(coef + (size_t)g * 64))[w] = zero4;
      }
      if (st) atomicOr(status + f, st);
    }
  }
  for (long long g = zero_from + i; g < L.nblocks; g += (long long)gridDim.x * kJpgdLanes)
#pragma unroll
    for (int w = 0; w < 8; ++w) ((uint4*)(coef + (size_t)g * 64))[w] = zero4;
}

// ---------------------------------------------------------------- the split route (jpgd_rule.hpp): frames whose ROUTE word is negative
// jpgd_unstuff_kernel over every segment of the interval table in turn, into one copy: interval k's bytes follow interval
// k - 1's, and its record gets (first byte, bytes).  The lengths are known only now, so the lanes are dealt out here: S from
// the copy's length and the number of segments, then a record's lane count from its length.  No segment: -1 bytes, no lane.
__global__ __launch_bounds__(kJpgdSyncLanes) void jpgd_split_unstuff_kernel(const uint8_t* __restrict__ files, const long long* __restrict__ offsets,
                                                                           const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work) {
  constexpr int kWaves = kJpgdSyncLanes / 64;
  __shared__ int wave_cnt[2][kWaves];  // as in jpgd_unstuff_kernel; `it` goes on from one segment to the next
  __shared__ int lens[kJpgdSplitIntervals];
  const int f = L.frame0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* fr = jpgd_frame(plan, f);
  if (fr[JPGD_F_ROUTE] >= 0) return;
  uint8_t* mine = work + (size_t)blockIdx.x * L.frame;
  const int* seg = (const int*)(mine + L.seg);
  const uint8_t* file = files + offsets[f];
  uint8_t* u = mine + L.unst;
  int* tab = (int*)(mine + L.table);
  int* iv = tab + kJpgdSplitIntAt;
  const int n_int = fr[JPGD_F_NINT];
  int total = 0, present = 0, it = 0;  // bytes kept and segments so far, the same in every lane
  for (int k = 0; k < n_int; ++k) {
    const int b0 = seg[2 * k], b1 = seg[2 * k + 1], start = total;
    present += b0 >= 0;
    for (int base = b0; b0 >= 0 && base < b1; base += kJpgdSyncLanes, it ^= 1) {
      const int q = base + tid;
      const uint8_t v = q < b1 ? file[q] : 0;
      const bool keep = q < b1 && !(v == 0 && q > b0 && file[q - 1] == 0xFF);
      const unsigned long long vote = __ballot(keep);
      if (lane == 0) wave_cnt[it][wave] = __popcll(vote);
      __syncthreads();
      int before = total, all = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const int c = wave_cnt[it][w];
        before += w < wave ? c : 0;
        all += c;
      }
      if (keep) u[before + __popcll(vote & ((1ull << lane) - 1ull))] = v;
      total += all;
    }
    if (tid == 0) iv[JPGD_X_INT * k] = start, iv[JPGD_X_INT * k + 1] = lens[k] = b0 >= 0 ? total - start : -1;
  }
  __syncthreads();
  const uint32_t S = jpgd_split_sub((uint32_t)total, (uint32_t)present, (uint32_t)-fr[JPGD_F_ROUTE]);
  if (tid < n_int) iv[JPGD_X_INT * tid + 2] = lens[tid] >= 0 ? (int)jpgd_split_lanes((uint32_t)lens[tid], S) : 0;
  if (tid == 0) tab[JPGD_T_LEN] = total, tab[JPGD_T_S] = (int)S;
}

// jpgd_relax_kernel with the chains cut at the markers.  An inclusive prefix of the records' lane counts sits in LDS; lane i
// looks its interval k up there (a binary search) and is lane q of it.  Lane q = 0 enters at the true (0, 0) and is final from
// round 0; a lane takes its predecessor's exit for q > 0 only, a dead one in round q and not before.  All intervals relax in
// the same rounds, so the loop ends after the longest interval's lane count at the latest.  The prefix over block counts and
// DC sums adds a neighbour's value only from inside the interval.  The last lane of an interval knows whether its chain died
// inside the data and from which of the interval's blocks on all are zero; a record without lanes is zero from block 0.
__global__ __launch_bounds__(kJpgdSyncLanes) void jpgd_split_relax_kernel(const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work) {
  __shared__ int set[kJpgdSetInts];
  __shared__ uint32_t xp[kJpgdSyncLanes], xn[kJpgdSyncLanes];
  __shared__ int xj[kJpgdSyncLanes], xd[3][kJpgdSyncLanes];
  __shared__ int lane0[kJpgdSplitIntervals + 1];  // interval k has lanes lane0[k] ... lane0[k + 1] - 1
  __shared__ int most;                            // the longest interval's lanes
  const int f = L.frame0 + blockIdx.x, i = threadIdx.x;
  const int* fr = jpgd_frame(plan, f);
  if (fr[JPGD_F_ROUTE] >= 0) return;
  const int* gset = plan + plan[JPGD_P_SETS] + fr[JPGD_F_SET] * kJpgdSetInts;
  for (int k = i; k < kJpgdSetInts; k += kJpgdSyncLanes) set[k] = gset[k];
  uint8_t* mine = work + (size_t)blockIdx.x * L.frame;
  int* tab = (int*)(mine + L.table);
  int* iv = tab + kJpgdSplitIntAt;
  const uint32_t S = (uint32_t)tab[JPGD_T_S];
  const int n_int = fr[JPGD_F_NINT], hv = plan[JPGD_P_HS] * plan[JPGD_P_VS], bpm = plan[JPGD_P_BPM];
  const int own_cnt = i < n_int ? iv[JPGD_X_INT * i + 2] : 0;
  xn[i] = (uint32_t)own_cnt;  // n_int <= kJpgdSplitIntervals: the upper half stays 0
  if (i == 0) most = 0, lane0[0] = 0;
  __syncthreads();
  atomicMax(&most, own_cnt);
  for (int off = 1; off < kJpgdSplitIntervals; off <<= 1) {
    const uint32_t a = i >= off ? xn[i - off] : 0u;
    __syncthreads();
    xn[i] += a;
    __syncthreads();
  }
  if (i < kJpgdSplitIntervals) lane0[i + 1] = (int)xn[i];
  __syncthreads();
  const int nsub = lane0[n_int], longest = most;
  const bool active = i < nsub;
  int k = 0;
  for (int hi = n_int; hi - k > 1;) {  // the last k with lane0[k] <= i: of equal ones the one that has lanes
    const int mid = (k + hi) >> 1;
    if (lane0[mid] <= i) k = mid;
    else hi = mid;
  }
  const int q = active ? i - lane0[k] : 0, cnt = lane0[k + 1] - lane0[k];
  const uint32_t len = active ? (uint32_t)iv[JPGD_X_INT * k + 1] : 0u;
  const uint8_t* u = mine + L.unst + (active ? iv[JPGD_X_INT * k] : 0);
  const uint32_t end = jpgd_sync_end((uint32_t)q, S, len);
  uint32_t entry_p = 8u * (uint32_t)q * S;
  int entry_j = 0, rounds = 0;
  xp[i] = kJpgdDead, xj[i] = 0, xn[i] = 0, xd[0][i] = 0, xd[1][i] = 0, xd[2][i] = 0;
  __syncthreads();
  bool need = active, wait = false;
  for (int r = 0; r < longest; ++r) {
    bool changed = wait;
    if (need) {
      JpgdRun x{entry_p, entry_j, 0u, {0, 0, 0}};
      JpgdRaw b;
      jpgd_sync_run(b, u, len, end, false, 0xFFFFFFFFu, hv, bpm, x, [&](JpgdRaw& bits, int c, int32_t& pred, uint32_t) {
        return jpgd_block(bits, jpgd_huff(set, c, 0), jpgd_huff(set, c, 1), pred, JpgdNoCoef());
      });
      changed = r == 0 || x.p != xp[i] || x.j != xj[i];
      xp[i] = x.p, xj[i] = x.j, xn[i] = x.n, xd[0][i] = x.dc[0], xd[1][i] = x.dc[1], xd[2][i] = x.dc[2];
    }
    ++rounds;
    if (!__syncthreads_or(changed)) break;
    need = wait = false;
    if (active && q > 0 && (xp[i - 1] != entry_p || xj[i - 1] != entry_j)) {
      if (xp[i - 1] == kJpgdDead && r + 1 < q) wait = true;  // not final before round q
      else entry_p = xp[i - 1], entry_j = xj[i - 1], need = true;
    }
    __syncthreads();  // every exit is read before the round rewrites it
  }
  __syncthreads();
  const uint32_t own_n = xn[i];
  const int own_d[3] = {xd[0][i], xd[1][i], xd[2][i]};
  for (int off = 1; off < longest; off <<= 1) {  // inclusive prefix inside the interval, in place
    const bool has = active && q >= off;
    const uint32_t an = has ? xn[i - off] : 0u;
    const int a0 = has ? xd[0][i - off] : 0, a1 = has ? xd[1][i - off] : 0, a2 = has ? xd[2][i - off] : 0;
    __syncthreads();
    xn[i] += an, xd[0][i] = jpgd_add(xd[0][i], a0), xd[1][i] = jpgd_add(xd[1][i], a1), xd[2][i] = jpgd_add(xd[2][i], a2);
    __syncthreads();
  }
  if (active) {
    int* e = tab + kJpgdSplitLaneAt + i * JPGD_X_LANE;
    e[0] = (int)entry_p, e[1] = entry_j, e[2] = (int)(xn[i] - own_n);
    e[3] = jpgd_sub(xd[0][i], own_d[0]), e[4] = jpgd_sub(xd[1][i], own_d[1]), e[5] = jpgd_sub(xd[2][i], own_d[2]);
    e[6] = k, e[7] = q;
    if (q == cnt - 1) {  // a chain that died inside the data: every block of the interval from the bad one on is zero
      const uint32_t blocks = jpgd_split_blocks(k, fr[JPGD_F_SPAN], plan[JPGD_P_MCUX] * plan[JPGD_P_MCUY], bpm);
      iv[JPGD_X_INT * k + 3] = (int)(xp[i] == kJpgdDead && xn[i] < blocks ? xn[i] : blocks);
    }
  }
  if (i < n_int && own_cnt == 0) iv[JPGD_X_INT * i + 3] = 0;
  if (i == 0) tab[JPGD_T_NSUB] = nsub, tab[JPGD_T_ROUNDS] = rounds;
}

// jpgd_sync_write_kernel with an interval's block budget in the place of the frame's: a lane decodes its owned blocks from
// its table entry into the interval's share of the coefficient buffer and stops at the interval's last block, so surplus bytes
// in front of a marker are nobody's.  An interval's last lane goes on past the interval's bytes on zero bits, never into the
// next interval's.  The blocks behind a dead chain's last good one are zeroed to the interval's end: by the lane that died
// behind the data, else - and for an interval without a segment - by lane k of the launch for interval k.
__global__ __launch_bounds__(kJpgdLanes) void jpgd_split_write_kernel(const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work,
                                                                     int* __restrict__ status) {
  __shared__ int set[kJpgdSetInts];
  __shared__ jpgd_word rows[kJpgdLanes * kJpgdRowDwords];
  const int f = L.frame0 + blockIdx.y, lane = threadIdx.x;
  const int* fr = jpgd_frame(plan, f);
  if (fr[JPGD_F_ROUTE] >= 0) return;
  const int* gset = plan + plan[JPGD_P_SETS] + fr[JPGD_F_SET] * kJpgdSetInts;
  for (int k = lane; k < kJpgdSetInts; k += kJpgdLanes) set[k] = gset[k];
  __syncthreads();
  uint8_t* mine = work + (size_t)blockIdx.y * L.frame;
  const int* tab = (const int*)(mine + L.table);
  const int* iv = tab + kJpgdSplitIntAt;
  int16_t* coef = (int16_t*)(mine + L.coef);
  const uint32_t S = (uint32_t)tab[JPGD_T_S];
  const int nsub = tab[JPGD_T_NSUB], i = blockIdx.x * kJpgdLanes + lane;
  const int n_int = fr[JPGD_F_NINT], span = fr[JPGD_F_SPAN], nmcu = plan[JPGD_P_MCUX] * plan[JPGD_P_MCUY], bpm = plan[JPGD_P_BPM];
  const uint4 zero4 = uint4{0u, 0u, 0u, 0u};
  if (i < nsub) {
    const int* e = tab + kJpgdSplitLaneAt + i * JPGD_X_LANE;
    const int k = e[6], q = e[7];
    const int* rec = iv + JPGD_X_INT * k;
    const uint32_t len = (uint32_t)rec[1], blocks = jpgd_split_blocks(k, span, nmcu, bpm), first = (uint32_t)e[2];
    int16_t* mine_coef = coef + (size_t)k * span * bpm * 64;  // the interval's block 0
    if ((uint32_t)e[0] != kJpgdDead && first < blocks) {
      jpgd_word* row = rows + lane * kJpgdRowDwords;
      JpgdRun x{(uint32_t)e[0], e[1], 0u, {e[3], e[4], e[5]}};
      JpgdRaw b;
      bool bad = false;
      jpgd_sync_run(b, mine + L.unst + rec[0], len, jpgd_sync_end((uint32_t)q, S, len), q == rec[2] - 1, blocks - first, plan[JPGD_P_HS] * plan[JPGD_P_VS], bpm, x,
                    [&](JpgdRaw& bits, int c, int32_t& pred, uint32_t n) {
                      jpgd_word* r = row;  // the captured pointer, once
#pragma unroll
                      for (int w = 0; w < 32; ++w) r[w] = 0;
                      if (!jpgd_block(bits, jpgd_huff(set, c, 0), jpgd_huff(set, c, 1), pred, (jpgd_half*)r)) {
                        bad = true;
                        return false;
                      }
                      uint4* dst = (uint4*)(mine_coef + (size_t)(first + n) * 64);
#pragma unroll
                      for (int w = 0; w < 8; ++w) dst[w] = uint4{(unsigned)r[4 * w], (unsigned)r[4 * w + 1], (unsigned)r[4 * w + 2], (unsigned)r[4 * w + 3]};
                      return true;
                    });
      int st = jpgd_past_end(b) ? JPGD_ST_PAST_END : 0;
      if (bad) {
        st |= JPGD_ST_BAD_CODE;
        if ((uint32_t)rec[3] == blocks)  // died behind the data
          for (uint32_t g = first + x.n; g < blocks; ++g)
#pragma unroll
            for (int w = 0; w < 8; ++w) ((uint4*)(mine_coef + (size_t)g * 64))[w] = zero4;
      }
      if (st) atomicOr(status + f, st);
    }
  }
  for (int k = i; k < n_int; k += (int)gridDim.x * kJpgdLanes) {
    int16_t* mine_coef = coef + (size_t)k * span * bpm * 64;
    for (uint32_t g = (uint32_t)iv[JPGD_X_INT * k + 3], blocks = jpgd_split_blocks(k, span, nmcu, bpm); g < blocks; ++g)
#pragma unroll
      for (int w = 0; w < 8; ++w) ((uint4*)(mine_coef + (size_t)g * 64))[w] = zero4;
  }
}

__global__ __launch_bounds__(kJpgdIdctBlocks * 8) void jpgd_idct_kernel(const int* __restrict__ plan, JpgdLaunch L, uint8_t* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) jpgd_word cf[kJpgdIdctBlocks * kJpgdCoefDwords];
  __shared__ int ws[kJpgdIdctBlocks * kJpgdWsBlock];
  __shared__ jpgd_word qt[3 * 32];  // three tables of 64 uint16
  const int f = L.frame0 + blockIdx.y, tid = threadIdx.x;
  const int* fr = jpgd_frame(plan, f);
  const int* gset = plan + plan[JPGD_P_SETS] + fr[JPGD_F_SET] * kJpgdSetInts;
  if (tid < 96) qt[tid] = gset[tid];
  uint8_t* mine = work + (size_t)blockIdx.y * L.frame;
  const long long g0 = (long long)blockIdx.x * kJpgdIdctBlocks;
  {  // 256 lanes x 16 bytes = the 32 blocks; a block past the end reads as zeros
    const int blk = tid >> 3, part = tid & 7;
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (g0 + blk < L.nblocks) v = *(const uint4*)(mine + L.coef + (size_t)(g0 + blk) * 128 + part * 16);
    jpgd_word* d = cf + blk * kJpgdCoefDwords + part * 4;
    d[0] = (int)v.x, d[1] = (int)v.y, d[2] = (int)v.z, d[3] = (int)v.w;
  }
  __syncthreads();
  const int blk = tid >> 3, k = tid & 7;
  const long long g = g0 + blk;
  const int hs = plan[JPGD_P_HS], hv = hs * plan[JPGD_P_VS], bpm = plan[JPGD_P_BPM], mcux = plan[JPGD_P_MCUX];
  const int m = (int)(g / bpm), j = (int)(g - (long long)m * bpm);
  const int c = j < hv ? 0 : j - hv + 1;
  {  // pass 1: column k
    const jpgd_half* src = (const jpgd_half*)(cf + blk * kJpgdCoefDwords);
    const jpgd_uhalf* q = (const jpgd_uhalf*)qt + c * 64;
    int32_t v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = jpgd_mul(src[r * 8 + k], q[r * 8 + k]);
    jpgd_idct8<11>(v);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[blk * kJpgdWsBlock + r * kJpgdWsRow + k] = v[r];
  }
  __syncthreads();
  if (g >= L.nblocks) return;
  int32_t v[8];  // pass 2: row k
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = ws[blk * kJpgdWsBlock + k * kJpgdWsRow + i];
  jpgd_idct8<18>(v);
  const int my = m / mcux, mx = m - my * mcux;
  const int by = c ? my : my * plan[JPGD_P_VS] + j / hs, bx = c ? mx : mx * hs + j % hs, stride = c ? L.cw : L.pw;
  uint2 o;
  o.x = jpgd_sample(v[0]) | (jpgd_sample(v[1]) << 8) | (jpgd_sample(v[2]) << 16) | ((unsigned)jpgd_sample(v[3]) << 24);
  o.y = jpgd_sample(v[4]) | (jpgd_sample(v[5]) << 8) | (jpgd_sample(v[6]) << 16) | ((unsigned)jpgd_sample(v[7]) << 24);
  *(uint2*)(mine + L.plane[c] + (size_t)(by * 8 + k) * stride + bx * 8) = o;
}

struct jpgd_u3 {  // 12 bytes at a 4-byte boundary
  unsigned x, y, z;
};
__global__ __launch_bounds__(kJpgdRgbThreads) void jpgd_rgb_kernel(const int* __restrict__ plan, JpgdLaunch L, const uint8_t* __restrict__ work,
                                                                  uint8_t* __restrict__ rgb) {
  const int H = plan[JPGD_P_H], W = plan[JPGD_P_W], nc = plan[JPGD_P_NCOMP], hs = plan[JPGD_P_HS], vs = plan[JPGD_P_VS];
  const int x0 = (blockIdx.x * kJpgdRgbThreads + threadIdx.x) * 4, y = blockIdx.y;
  if (x0 >= W) return;
  const uint8_t* mine = work + (size_t)blockIdx.z * L.frame;
  const uint8_t* yp = mine + L.plane[0];
  const uint8_t *cbp = mine + L.plane[1], *crp = mine + L.plane[2];
  const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
  const unsigned y4 = *(const unsigned*)(yp + (size_t)y * L.pw + x0);  // the plane's rows are whole blocks: x0 + 3 < pw
  uint8_t px[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int Y = (y4 >> (8 * i)) & 255, x = min(x0 + i, W - 1);
    if (nc == 1) px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = (uint8_t)Y;
    else jpgd_rgb(Y, jpgd_chroma(cbp, L.cw, cw, ch, hs, vs, x, y), jpgd_chroma(crp, L.cw, cw, ch, hs, vs, x, y), px + 3 * i);
  }
  uint8_t* o = rgb + (((size_t)(L.frame0 + blockIdx.z) * H + y) * W + x0) * 3;
  if (x0 + 4 <= W && ((uintptr_t)o & 3u) == 0) {
    jpgd_u3 v;
    v.x = px[0] | (px[1] << 8) | (px[2] << 16) | ((unsigned)px[3] << 24);
    v.y = px[4] | (px[5] << 8) | (px[6] << 16) | ((unsigned)px[7] << 24);
    v.z = px[8] | (px[9] << 8) | (px[10] << 16) | ((unsigned)px[11] << 24);
    *(jpgd_u3*)o = v;
  } else {
    const int n = min(4, W - x0) * 3;
    for (int i = 0; i < n; ++i) o[i] = px[i];
  }
}
