// float_cmp_segments / float_cmp_work_bytes: the on-device comparison of the fp16 precision guard (include/float_hip.h).
#include "cmp_kernels.hpp"

namespace {
// Workgroups per segment.  ~2048 workgroups in all (256 CUs x 8 resident workgroups of 256 threads) when there are few
// segments - 8 frames get 256 slices each - and one launch round when there are many (250 frames: 8 slices, 2000
// workgroups); never less than 2048 elements per slice, so that short segments do not pay for empty workgroups.
// A function of (n_seg, seg_len) alone: float_cmp_work_bytes must agree with the launch without asking the device.
int cmp_slices(int32_t n_seg, int64_t seg_len) {
  int64_t s = 2048 / (int64_t)n_seg;
  s = std::min<int64_t>(s, seg_len / 2048);
  return (int)std::max<int64_t>(1, std::min<int64_t>(s, 512));
}
}  // namespace

extern "C" {

size_t float_cmp_work_bytes(int32_t n_seg, int64_t seg_len) {
  if (n_seg <= 0 || seg_len <= 0) return 0;
  return (size_t)n_seg * (size_t)cmp_slices(n_seg, seg_len) * kCmpStats * sizeof(double);
}

int float_cmp_segments(const float* a, const float* b, int32_t n_seg, int64_t seg_len, float thr, double* stats, void* work,
                       size_t work_bytes, void* stream) {
  FH_REQUIRE(a && b && stats && work, "float_cmp_segments: null argument");
  FH_REQUIRE(n_seg > 0 && seg_len > 0, "float_cmp_segments: n_seg (%d) and seg_len (%lld) must be positive", n_seg, (long long)seg_len);
  FH_REQUIRE(seg_len <= ((int64_t)1 << 60) / n_seg, "float_cmp_segments: %d segments of %lld elements overflow", n_seg, (long long)seg_len);
  FH_REQUIRE(!(thr != thr), "float_cmp_segments: thr is NaN");
  FH_REQUIRE(((uintptr_t)a & 3u) == 0 && ((uintptr_t)b & 3u) == 0, "float_cmp_segments: a and b must be 4-byte aligned");
  FH_REQUIRE(((uintptr_t)stats & 7u) == 0 && ((uintptr_t)work & 7u) == 0, "float_cmp_segments: stats and work must be 8-byte aligned");
  const size_t need = float_cmp_work_bytes(n_seg, seg_len);
  FH_REQUIRE(work_bytes >= need, "float_cmp_segments: work_bytes %zu < float_cmp_work_bytes(%d, %lld) = %zu", work_bytes, n_seg,
             (long long)seg_len, need);
  const int slices = cmp_slices(n_seg, seg_len);
  FH_REQUIRE((int64_t)n_seg * slices <= 0x7fffffff, "float_cmp_segments: too many segments (%d)", n_seg);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cmp_partial_kernel, dim3((unsigned)n_seg * (unsigned)slices), dim3(kCmpThreads), 0, s, a, b, (long long)seg_len,
                     slices, thr, (double*)work);
  hipLaunchKernelGGL(cmp_fold_kernel, dim3((unsigned)n_seg), dim3(64), 0, s, (const double*)work, slices, stats);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
