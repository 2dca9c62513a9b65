// float_aud_front / float_aud_front_len / float_aud_front_work_bytes: the audio front end on the device (include/float_hip.h).
#include "audf_kernels.hpp"

#include <math.h>

#include <numeric>

namespace {
constexpr int64_t kAudfMaxLen = (int64_t)1 << 34;  // n_in and n_out: m * down stays below 2^62, the grid below 2^26 tiles
constexpr int32_t kAudfMaxRate = 1 << 20;

// n_out = ceil(n_in * up / down) in exact integers; 0 when an argument is out of range
int64_t audf_len(int64_t n_in, int32_t rate_in, int32_t rate_out) {
  if (n_in <= 0 || n_in > kAudfMaxLen || rate_in <= 0 || rate_out <= 0 || rate_in > kAudfMaxRate || rate_out > kAudfMaxRate) return 0;
  const int64_t g = std::gcd((int64_t)rate_in, (int64_t)rate_out);
  const int64_t up = rate_out / g, down = rate_in / g;
  const int64_t n_out = (n_in * up + down - 1) / down;
  return n_out > kAudfMaxLen ? 0 : n_out;
}
}  // namespace

extern "C" {

int64_t float_aud_front_len(int64_t n_in, int32_t rate_in, int32_t rate_out) { return audf_len(n_in, rate_in, rate_out); }

size_t float_aud_front_work_bytes(int64_t n_in, int32_t rate_in, int32_t rate_out) {
  const int64_t n_out = audf_len(n_in, rate_in, rate_out);
  if (n_out == 0) return 0;
  return (size_t)(kAudfHead + 2 * ((n_out + kAudfTile - 1) / kAudfTile)) * sizeof(double);
}

int float_aud_front(const float* w, int32_t channels, int64_t ch_stride, int64_t n_in, int32_t rate_in, int32_t rate_out,
                    int32_t zeros, float rolloff, int32_t flags, float* a, int64_t n_out, void* work, size_t work_bytes,
                    void* stream) {
  FH_REQUIRE(w && a && work, "float_aud_front: null argument (w, a or work)");
  FH_REQUIRE(channels >= 1 && channels <= 8, "float_aud_front: channels (%d) must be 1 ... 8", channels);
  FH_REQUIRE(zeros >= 1 && zeros <= 32, "float_aud_front: zeros (%d) must be 1 ... 32", zeros);
  FH_REQUIRE(rolloff > 0.f && rolloff <= 1.f, "float_aud_front: rolloff (%g) must be in (0, 1]", (double)rolloff);
  FH_REQUIRE(rate_in >= 1 && rate_in <= kAudfMaxRate, "float_aud_front: rate_in (%d) must be 1 ... %d", rate_in, kAudfMaxRate);
  FH_REQUIRE(rate_out >= 1 && rate_out <= kAudfMaxRate, "float_aud_front: rate_out (%d) must be 1 ... %d", rate_out, kAudfMaxRate);
  FH_REQUIRE(n_in >= 1 && n_in <= kAudfMaxLen, "float_aud_front: n_in (%lld) must be 1 ... 2^34", (long long)n_in);
  FH_REQUIRE(flags == 0 || flags == FLOAT_AUD_FRONT_NORMALIZE, "float_aud_front: unknown flags (%d)", flags);
  const int64_t want = audf_len(n_in, rate_in, rate_out);
  FH_REQUIRE(want > 0, "float_aud_front: n_in (%lld) at %d -> %d Hz gives more than 2^34 samples", (long long)n_in, rate_in, rate_out);
  FH_REQUIRE(n_out == want, "float_aud_front: n_out (%lld) must be float_aud_front_len(%lld, %d, %d) = %lld", (long long)n_out,
             (long long)n_in, rate_in, rate_out, (long long)want);
  FH_REQUIRE(channels == 1 || ch_stride >= n_in, "float_aud_front: ch_stride (%lld) must be at least n_in (%lld)", (long long)ch_stride,
             (long long)n_in);
  FH_REQUIRE(((uintptr_t)w & 3u) == 0 && ((uintptr_t)a & 3u) == 0, "float_aud_front: w and a must be 4-byte aligned");
  FH_REQUIRE(((uintptr_t)work & 7u) == 0, "float_aud_front: work must be 8-byte aligned");
  const size_t need = float_aud_front_work_bytes(n_in, rate_in, rate_out);
  FH_REQUIRE(work_bytes >= need, "float_aud_front: work_bytes %zu < float_aud_front_work_bytes(%lld, %d, %d) = %zu", work_bytes,
             (long long)n_in, rate_in, rate_out, need);

  AudfPlan p{};
  const int g = std::gcd(rate_in, rate_out);
  p.n_in = n_in, p.n_out = n_out, p.ch_stride = ch_stride, p.channels = channels;
  p.up = rate_out / g, p.down = rate_in / g;
  p.zeros = zeros, p.stats = flags & FLOAT_AUD_FRONT_NORMALIZE;
  p.c = (double)rolloff * std::min(1.0, (double)p.up / (double)p.down);
  p.inv_up = 1.0 / (double)p.up, p.inv_zeros = 1.0 / (double)zeros;
  const bool resample = rate_in != rate_out;
  size_t lds = 0;
  if (resample) {
    // a tile reads floor((r0 + 255 down) / up) + 2 W + 2 <= floor(255 down / up) + 1 + 2 W + 2 samples (r0 < up)
    const double Wd = ceil((double)zeros / p.c);
    const double span = (double)((int64_t)(kAudfTile - 1) * p.down / p.up) + 2.0 * Wd + 3.0;
    FH_REQUIRE(span * sizeof(float) <= (double)kAudfMaxLds,
               "float_aud_front: rate_in %d -> rate_out %d with zeros %d, rolloff %g needs %.0f staged samples per tile of %d outputs, "
               "more than the %zu bytes of LDS hold",
               rate_in, rate_out, zeros, (double)rolloff, span, kAudfTile, kAudfMaxLds);
    p.W = (int)Wd;
    lds = (size_t)span * sizeof(float);
  }
  hipStream_t s = (hipStream_t)stream;
  const long long n_tiles = (n_out + kAudfTile - 1) / kAudfTile;
  double* wk = (double*)work;
  if (resample) {
    if (lds > 65536)  // beyond the default limit of dynamic LDS: ratios past ~50 : 1
      FH_CHECK_HIP(hipFuncSetAttribute((const void*)audf_resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAudfMaxLds));
    hipLaunchKernelGGL(audf_resample_kernel, dim3((unsigned)n_tiles), dim3(kAudfTile), lds, s, w, a, wk, p);
  } else {
    hipLaunchKernelGGL(audf_mix_kernel, dim3((unsigned)n_tiles), dim3(kAudfTile), 0, s, w, a, wk, p);
  }
  if (p.stats) {
    hipLaunchKernelGGL(audf_fold_kernel, dim3(1), dim3(kAudfTile), 0, s, wk, n_tiles, (long long)n_out);
    hipLaunchKernelGGL(audf_norm_kernel, dim3((unsigned)n_tiles), dim3(kAudfTile), 0, s, a, (const double*)wk, (long long)n_out);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
