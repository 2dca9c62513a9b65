// float_png_encode / float_png_work_bytes / float_png_tables: lossless PNG files from 8-bit RGB frames on the device
// (include/float_hip.h).
#include "png_kernels.hpp"

namespace {
// frame geometry of a call; false for sizes the operator does not take.  band = 0: the default.
bool png_plan(int32_t n_frames, int32_t h, int32_t w, int32_t band, PngPlan* p) {
  if (n_frames < 1 || h < 1 || w < 1 || h > kPngMaxSide || w > kPngMaxSide || band < 0) return false;
  const int stride = 1 + 3 * w;
  if (band == 0) band = std::max(1, std::min({8, h, kPngBandBytes / stride}));
  if (band > h || (long long)band * stride > kPngBandBytes) return false;
  p->h = h, p->w = w, p->band = band, p->nb = (h + band - 1) / band, p->stride = stride;
  // the worst case of a band: the header, 9 bits per byte (the flat table bounds the chosen one), an end-of-block of at most 15
  // bits, the stored block's 3, up to 7 to the byte boundary, 00 00 FF FF
  const unsigned long long n = (unsigned long long)band * stride;
  p->slot_bytes = ((kPngHeaderBits + 9 * n + 15 + 3 + 7) / 8 + 4 + 15) & ~15ull;
  return true;
}

// work of one group: int64 dst[items]; int32 lens[items]; uint32 crc[items], ad1[items], ad2[items]; (rounded to 16 bytes) the 4
// words of meta per frame; then the slots
size_t png_meta_off(size_t items) { return (items * 24 + 15) & ~(size_t)15; }
size_t png_slots_off(size_t items) { return png_meta_off(items) + (size_t)kPngGroup * 16; }

void png_head(const PngPlan& p, uint8_t* o) {
  const uint8_t head[33] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R',
                            (uint8_t)(p.w >> 24), (uint8_t)(p.w >> 16), (uint8_t)(p.w >> 8), (uint8_t)p.w,
                            (uint8_t)(p.h >> 24), (uint8_t)(p.h >> 16), (uint8_t)(p.h >> 8), (uint8_t)p.h,
                            8, 2, 0, 0, 0, 0, 0, 0, 0};  // 8 bits, colour type 2, deflate, adaptive filters, no interlace
  memcpy(o, head, 33);
  const uint32_t crc = png_crc_bytes(kPngCrcHost, o + 12, 17);
  o[29] = (uint8_t)(crc >> 24), o[30] = (uint8_t)(crc >> 16), o[31] = (uint8_t)(crc >> 8), o[32] = (uint8_t)crc;
}
}  // namespace

extern "C" {

size_t float_png_work_bytes(int32_t n_frames, int32_t h, int32_t w, int32_t band) {
  PngPlan p{};
  if (!png_plan(n_frames, h, w, band, &p)) return 0;
  const size_t items = (size_t)std::min(n_frames, kPngGroup) * p.nb;
  return png_slots_off(items) + items * (size_t)p.slot_bytes;
}

int float_png_tables(int32_t lengths[8 * 257]) {
  FH_REQUIRE(lengths, "float_png_tables: null argument (lengths)");
  for (int k = 0; k < 8; ++k)
    for (int s = 0; s < 257; ++s) lengths[k * 257 + s] = kPngLengths.len[k][s];
  return FLOAT_OK;
}

int float_png_encode(const uint8_t* rgb8, int32_t n_frames, int32_t h, int32_t w, int32_t band, uint8_t* out, size_t out_cap, int64_t* offsets,
                     uint32_t* crcs, void* work, size_t work_bytes, void* stream) {
  const char* fn = "float_png_encode";
  FH_REQUIRE(rgb8 && out && offsets && work, "%s: null argument (rgb8, out, offsets or work)", fn);
  FH_REQUIRE(n_frames >= 1, "%s: n_frames (%d) must be positive", fn, n_frames);
  FH_REQUIRE(h >= 1 && w >= 1 && h <= kPngMaxSide && w <= kPngMaxSide, "%s: sides h x w (%d x %d) must be in 1 ... %d", fn, h, w, kPngMaxSide);
  FH_REQUIRE(band >= 0 && band <= h && (long long)band * (1 + 3 * w) <= kPngBandBytes,
             "%s: band (%d) must be 0 (the default) or 1 ... h (%d) rows of at most %d bytes in all (a row is %d)", fn, band, h, kPngBandBytes,
             1 + 3 * w);
  FH_REQUIRE(((uintptr_t)offsets & 7u) == 0, "%s: offsets must be 8-byte aligned", fn);
  FH_REQUIRE(((uintptr_t)crcs & 3u) == 0, "%s: crcs must be 4-byte aligned", fn);
  FH_REQUIRE(((uintptr_t)work & 15u) == 0, "%s: work must be 16-byte aligned", fn);
  PngPlan p{};
  FH_REQUIRE(png_plan(n_frames, h, w, band, &p), "%s: sides (%d x %d) and band (%d) are outside the operator's range", fn, h, w, band);
  const size_t need = float_png_work_bytes(n_frames, h, w, band);
  FH_REQUIRE(work_bytes >= need, "%s: work_bytes %zu < float_png_work_bytes(%d, %d, %d, %d) = %zu", fn, work_bytes, n_frames, h, w, band, need);
  png_head(p, p.head);

  hipStream_t s = (hipStream_t)stream;
  const size_t items = (size_t)std::min(n_frames, kPngGroup) * p.nb;
  long long* dst = (long long*)work;
  int* lens = (int*)((char*)work + items * 8);
  uint32_t* bcrc = (uint32_t*)((char*)work + items * 12);
  uint32_t* ad1 = (uint32_t*)((char*)work + items * 16);
  uint32_t* ad2 = (uint32_t*)((char*)work + items * 20);
  uint32_t* meta = (uint32_t*)((char*)work + png_meta_off(items));
  uint8_t* slots = (uint8_t*)work + png_slots_off(items);
  for (int f0 = 0; f0 < n_frames; f0 += kPngGroup) {  // groups share `work` in stream order
    p.frame0 = f0, p.frames = std::min(kPngGroup, n_frames - f0);
    const dim3 grid((unsigned)p.nb, (unsigned)p.frames);
    hipLaunchKernelGGL(png_code_kernel, grid, dim3(kPngThreads), 0, s, rgb8, p, lens, bcrc, ad1, ad2, slots);
    hipLaunchKernelGGL(png_offsets_kernel, dim3(1), dim3(kPngThreads), 0, s, p, (const int*)lens, (const uint32_t*)bcrc, (const uint32_t*)ad1,
                       (const uint32_t*)ad2, dst, meta, (long long*)offsets, crcs);
    hipLaunchKernelGGL(png_pack_kernel, grid, dim3(kPngThreads), 0, s, p, (const int*)lens, (const long long*)dst, (const uint32_t*)meta,
                       (const uint8_t*)slots, out, (unsigned long long)out_cap);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
