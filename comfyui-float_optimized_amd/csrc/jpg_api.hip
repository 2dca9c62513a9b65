// float_jpg_encode / float_jpg_work_bytes: baseline JPEG files from 8-bit RGB frames on the device (include/float_hip.h).
#include "jpg_kernels.hpp"

namespace {
constexpr int32_t kJpgMaxSide = 16384;

// ITU-T T.81 Annex K.1 / K.2, row-major
const uint8_t kQLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3: BITS[1 ... 16] and HUFFVAL of the four tables, in the order of the header: DC0, AC0, DC1, AC1
struct HuffSpec {
  uint8_t tc_th, bits[16];
  int n;
  const uint8_t* vals;
};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const HuffSpec kHuff[4] = {{0x00, {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, kDcVals},
                           {0x10, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, kAcLumaVals},
                           {0x01, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, kDcVals},
                           {0x11, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, kAcChromaVals}};

// frame geometry of a call; false for sizes the operator does not take.  padded: any sides from 1 on, the MCU grid rounded up.
bool jpg_plan(int32_t n_frames, int32_t h, int32_t w, int32_t restart, bool padded, JpgPlan* p) {
  if (n_frames < 1 || h < 1 || w < 1 || h > kJpgMaxSide || w > kJpgMaxSide || restart < 0 || restart > 65535) return false;
  if (!padded && (h % 16 || w % 16)) return false;
  p->h = h, p->w = w, p->mcw = (w + 15) / 16;
  p->nmcu = ((h + 15) / 16) * p->mcw;
  p->span = restart > 0 ? std::min(restart, p->nmcu) : p->nmcu;
  p->n_int = (p->nmcu + p->span - 1) / p->span;
  // the worst case of an interval: every block at its bound, every byte stuffed
  p->slot_bytes = ((unsigned long long)p->span * 6 * kJpgBlockBytes * 2 + 15) & ~15ull;
  return p->slot_bytes < (1ull << 31);
}

// work of one group: int64 dst[items], int32 lens[items] (rounded to 16 bytes), then the slots
size_t jpg_lens_off(size_t items) { return items * 8; }
size_t jpg_slots_off(size_t items) { return (items * 12 + 15) & ~(size_t)15; }

void jpg_tables(int quality, JpgTables* tb) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) tb->q[t][i] = (uint16_t)std::min(255, std::max(1, ((t ? kQChroma[i] : kQLuma[i]) * s + 50) / 100));
  memset(tb->dc, 0, sizeof(tb->dc));
  memset(tb->ac, 0, sizeof(tb->ac));
  for (int t = 0; t < 4; ++t) {  // T.81 Annex C: the codes of one length count up, and double to the next length
    const HuffSpec& h = kHuff[t];
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < h.bits[len - 1]; ++i, ++k, ++code) {
        uint32_t* dst = (h.tc_th & 0x10) ? tb->ac[h.tc_th & 1] : tb->dc[h.tc_th & 1];
        dst[h.vals[k]] = (code << 8) | (uint32_t)len;
      }
      code <<= 1;
    }
  }
}

void jpg_header(const JpgPlan& p, const JpgTables& tb, int restart, JpgHeader* hd) {
  uint8_t* o = hd->bytes;
  auto put = [&o](std::initializer_list<int> v) {
    for (int b : v) *o++ = (uint8_t)b;
  };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    put({0xFF, 0xDB, 0, 67, t});
    for (int i = 0; i < 64; ++i) *o++ = (uint8_t)tb.q[t][kZigzag[i]];
  }
  put({0xFF, 0xC0, 0, 17, 8, p.h >> 8, p.h & 255, p.w >> 8, p.w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (const HuffSpec& h : kHuff) {
    put({0xFF, 0xC4, (19 + h.n) >> 8, (19 + h.n) & 255, h.tc_th});
    for (int i = 0; i < 16; ++i) *o++ = h.bits[i];
    for (int i = 0; i < h.n; ++i) *o++ = h.vals[i];
  }
  if (restart > 0) put({0xFF, 0xDD, 0, 4, restart >> 8, restart & 255});
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  hd->len = (int)(o - hd->bytes);
}
size_t jpg_work_bytes(int32_t n_frames, int32_t h, int32_t w, int32_t restart, bool padded) {
  JpgPlan p{};
  if (!jpg_plan(n_frames, h, w, restart, padded, &p)) return 0;
  const size_t items = (size_t)std::min(n_frames, kJpgGroup) * p.n_int;
  return jpg_slots_off(items) + items * (size_t)p.slot_bytes;
}

// float_jpg_encode (padded = false) and float_jpg_encode_padded: one set of checks, one launch sequence.  The coding kernel is
// jpg_code_kernel<false> whenever the frames allow its 2-byte loads - whole MCUs and an even address - and <true> otherwise, so
// the padded entry runs float_jpg_encode's own kernel on the sizes float_jpg_encode takes.
int jpg_encode(const char* fn, bool padded, const uint8_t* rgb8, int32_t n_frames, int32_t h, int32_t w, int32_t quality, int32_t restart,
               uint8_t* out, size_t out_cap, int64_t* offsets, void* work, size_t work_bytes, void* stream) {
  FH_REQUIRE(rgb8 && out && offsets && work, "%s: null argument (rgb8, out, offsets or work)", fn);
  FH_REQUIRE(n_frames >= 1, "%s: n_frames (%d) must be positive", fn, n_frames);
  if (padded) {
    FH_REQUIRE(h >= 1 && w >= 1 && h <= kJpgMaxSide && w <= kJpgMaxSide, "%s: sides (%d x %d) must be in 1 ... %d", fn, h, w, kJpgMaxSide);
  } else {
    FH_REQUIRE(h >= 16 && w >= 16 && h <= kJpgMaxSide && w <= kJpgMaxSide && h % 16 == 0 && w % 16 == 0,
               "%s: sides (%d x %d) must be multiples of 16 in 16 ... %d (4:2:0 MCUs)", fn, h, w, kJpgMaxSide);
  }
  FH_REQUIRE(quality >= 1 && quality <= 100, "%s: quality (%d) must be 1 ... 100", fn, quality);
  FH_REQUIRE(restart >= 0 && restart <= 65535, "%s: restart (%d) must be 0 ... 65535 MCUs", fn, restart);
  FH_REQUIRE(padded || ((uintptr_t)rgb8 & 1u) == 0, "%s: rgb8 must be 2-byte aligned", fn);
  FH_REQUIRE(((uintptr_t)offsets & 7u) == 0, "%s: offsets must be 8-byte aligned", fn);
  FH_REQUIRE(((uintptr_t)work & 15u) == 0, "%s: work must be 16-byte aligned", fn);
  JpgPlan p{};
  FH_REQUIRE(jpg_plan(n_frames, h, w, restart, padded, &p), "%s: an interval of %d MCUs needs a slot beyond 2 GiB (use a restart interval)", fn,
             restart > 0 ? restart : ((h + 15) / 16) * ((w + 15) / 16));
  const size_t need = jpg_work_bytes(n_frames, h, w, restart, padded);
  FH_REQUIRE(work_bytes >= need, "%s: work_bytes %zu < float_jpg_work_bytes%s(%d, %d, %d, %d) = %zu", fn, work_bytes, padded ? "_padded" : "",
             n_frames, h, w, restart, need);

  JpgTables tb;
  JpgHeader hd{};
  jpg_tables(quality, &tb);
  jpg_header(p, tb, restart, &hd);
  p.hdr_len = hd.len;

  hipStream_t s = (hipStream_t)stream;
  const bool whole = h % 16 == 0 && w % 16 == 0 && ((uintptr_t)rgb8 & 1u) == 0;
  const size_t items = (size_t)std::min(n_frames, kJpgGroup) * p.n_int;
  long long* dst = (long long*)work;
  int* lens = (int*)((char*)work + jpg_lens_off(items));
  uint8_t* slots = (uint8_t*)work + jpg_slots_off(items);
  for (int f0 = 0; f0 < n_frames; f0 += kJpgGroup) {  // groups share `work` in stream order
    p.frame0 = f0, p.frames = std::min(kJpgGroup, n_frames - f0);
    const dim3 grid((unsigned)p.n_int, (unsigned)p.frames);
    if (whole) hipLaunchKernelGGL(jpg_code_kernel<false>, grid, dim3(kJpgThreads), 0, s, rgb8, p, tb, lens, slots);
    else hipLaunchKernelGGL(jpg_code_kernel<true>, grid, dim3(kJpgThreads), 0, s, rgb8, p, tb, lens, slots);
    hipLaunchKernelGGL(jpg_offsets_kernel, dim3(1), dim3(kJpgThreads), 0, s, p, (const int*)lens, dst, (long long*)offsets);
    hipLaunchKernelGGL(jpg_pack_kernel, grid, dim3(kJpgThreads), 0, s, p, hd, (const int*)lens, (const long long*)dst, (const uint8_t*)slots, out,
                       (unsigned long long)out_cap);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}
}  // namespace

extern "C" {

size_t float_jpg_work_bytes(int32_t n_frames, int32_t h, int32_t w, int32_t restart) { return jpg_work_bytes(n_frames, h, w, restart, false); }

size_t float_jpg_work_bytes_padded(int32_t n_frames, int32_t h, int32_t w, int32_t restart) {
  return jpg_work_bytes(n_frames, h, w, restart, true);
}

int float_jpg_encode(const uint8_t* rgb8, int32_t n_frames, int32_t h, int32_t w, int32_t quality, int32_t restart, uint8_t* out, size_t out_cap,
                     int64_t* offsets, void* work, size_t work_bytes, void* stream) {
  return jpg_encode("float_jpg_encode", false, rgb8, n_frames, h, w, quality, restart, out, out_cap, offsets, work, work_bytes, stream);
}

int float_jpg_encode_padded(const uint8_t* rgb8, int32_t n_frames, int32_t h, int32_t w, int32_t quality, int32_t restart, uint8_t* out,
                            size_t out_cap, int64_t* offsets, void* work, size_t work_bytes, void* stream) {
  return jpg_encode("float_jpg_encode_padded", true, rgb8, n_frames, h, w, quality, restart, out, out_cap, offsets, work, work_bytes, stream);
}

}  // extern "C"
