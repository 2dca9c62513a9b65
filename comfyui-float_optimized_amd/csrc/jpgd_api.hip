// float_jpg_decode_plan[_ints | _entropy] / float_jpg_decode_work_bytes / float_jpg_decode / float_jpg_decode_host: baseline JPEG files ->
// 8-bit RGB frames on the device (include/float_hip.h).
#include "jpgd_kernels.hpp"
#include "jpgd_plan.hpp"

namespace {
JpgdLaunch jpgd_launch(const int32_t* plan) {
  const JpgdWork k = jpgd_work(plan);
  JpgdLaunch L{};
  L.seg = k.seg, L.coef = k.coef, L.frame = k.frame, L.pw = k.pw, L.cw = k.cw, L.nblocks = k.nblocks, L.unst = k.unst, L.table = k.table;
  for (int c = 0; c < 3; ++c) L.plane[c] = k.plane[c];
  return L;
}
}  // namespace

extern "C" {

size_t float_jpg_decode_plan_ints(int32_t n_frames) { return jpgd_plan_ints(n_frames); }

int float_jpg_decode_plan(const uint8_t* files, const int64_t* offsets, int32_t n_frames, int32_t* plan, size_t plan_ints) {
  FH_REQUIRE(files && offsets && plan, "float_jpg_decode_plan: null argument (files, offsets or plan)");
  FH_REQUIRE(n_frames >= 1, "float_jpg_decode_plan: n_frames (%d) must be positive", n_frames);
  char why[400];
  FH_REQUIRE(jpgd_build_plan(files, offsets, n_frames, plan, plan_ints, why, sizeof(why)) == 0, "float_jpg_decode_plan: %s", why);
  return FLOAT_OK;
}

int float_jpg_decode_plan_entropy(const uint8_t* files, const int64_t* offsets, int32_t n_frames, int32_t* plan, size_t plan_ints, int32_t entropy,
                                  int32_t sync_bytes) {
  FH_REQUIRE(files && offsets && plan, "float_jpg_decode_plan_entropy: null argument (files, offsets or plan)");
  FH_REQUIRE(n_frames >= 1, "float_jpg_decode_plan_entropy: n_frames (%d) must be positive", n_frames);
  char why[400];
  FH_REQUIRE(jpgd_build_plan(files, offsets, n_frames, plan, plan_ints, why, sizeof(why), entropy, sync_bytes) == 0, "float_jpg_decode_plan_entropy: %s",
             why);
  return FLOAT_OK;
}

size_t float_jpg_decode_work_bytes(const int32_t* plan) {
  if (!jpgd_plan_ok(plan)) return 0;
  return (size_t)std::min(plan[JPGD_P_N], plan[JPGD_P_GROUP]) * jpgd_work(plan).frame;
}

int float_jpg_decode_host(const uint8_t* files, const int64_t* offsets, const int32_t* plan, int32_t n_frames, uint8_t* rgb8_out,
                          int32_t* status) {
  FH_REQUIRE(files && offsets && rgb8_out && status, "float_jpg_decode_host: null argument (files, offsets, rgb8_out or status)");
  FH_REQUIRE(jpgd_plan_ok(plan) && plan[JPGD_P_N] == n_frames, "float_jpg_decode_host: plan is not float_jpg_decode_plan's for %d frames", n_frames);
  const size_t frame = (size_t)plan[JPGD_P_H] * plan[JPGD_P_W] * 3;
  for (int i = 0; i < n_frames; ++i) jpgd_host_frame(files, offsets, plan, i, rgb8_out + i * frame, status + i);
  return FLOAT_OK;
}

int float_jpg_decode(const uint8_t* files, const int64_t* offsets, const int32_t* plan, const int32_t* plan_host, int32_t n_frames,
                     uint8_t* rgb8_out, int32_t* status, void* work, size_t work_bytes, void* stream) {
  FH_REQUIRE(files && offsets && plan && rgb8_out && status && work, "float_jpg_decode: null argument (files, offsets, plan, rgb8_out, status or work)");
  FH_REQUIRE(jpgd_plan_ok(plan_host) && plan_host[JPGD_P_N] == n_frames, "float_jpg_decode: plan_host is not float_jpg_decode_plan's for %d frames",
             n_frames);
  FH_REQUIRE(((uintptr_t)offsets & 7u) == 0 && ((uintptr_t)plan & 3u) == 0 && ((uintptr_t)status & 3u) == 0,
             "float_jpg_decode: offsets must be 8-byte, plan and status 4-byte aligned");
  FH_REQUIRE(((uintptr_t)work & 15u) == 0, "float_jpg_decode: work must be 16-byte aligned");
  const size_t need = float_jpg_decode_work_bytes(plan_host);
  FH_REQUIRE(work_bytes >= need, "float_jpg_decode: work_bytes %zu < float_jpg_decode_work_bytes(plan) = %zu", work_bytes, need);

  JpgdLaunch L = jpgd_launch(plan_host);
  const int H = plan_host[JPGD_P_H], W = plan_host[JPGD_P_W], group = plan_host[JPGD_P_GROUP];
  hipStream_t s = (hipStream_t)stream;
  const unsigned lanes = (unsigned)((plan_host[JPGD_P_MAXINT] + kJpgdLanes - 1) / kJpgdLanes);
  const unsigned idct = (unsigned)((L.nblocks + kJpgdIdctBlocks - 1) / kJpgdIdctBlocks);
  const unsigned cols = (unsigned)(((W + 3) / 4 + kJpgdRgbThreads - 1) / kJpgdRgbThreads);
  const unsigned sync = (unsigned)((jpgd_work(plan_host).sync_lanes + kJpgdLanes - 1) / kJpgdLanes);  // 0: no frame on the sync route
  const unsigned split = (unsigned)((jpgd_work(plan_host).split_lanes + kJpgdLanes - 1) / kJpgdLanes);  // the same for the split route
  for (int f0 = 0; f0 < n_frames; f0 += group) {  // groups share `work` in stream order
    L.frame0 = f0, L.frames = std::min(group, n_frames - f0);
    const unsigned nf = (unsigned)L.frames;
    hipLaunchKernelGGL(jpgd_scan_kernel, dim3(nf), dim3(kJpgdScanThreads), 0, s, files, (const long long*)offsets, (const int*)plan, L,
                       (uint8_t*)work, (int*)status);
    hipLaunchKernelGGL(jpgd_entropy_kernel, dim3(lanes, nf), dim3(kJpgdLanes), 0, s, files, (const long long*)offsets, (const int*)plan, L,
                       (uint8_t*)work, (int*)status);
    bool any = false, any_split = false;
    for (int f = f0; f < f0 + L.frames; ++f) {
      const int32_t route = plan_host[plan_host[JPGD_P_FRAMES] + f * JPGD_F_INTS + JPGD_F_ROUTE];
      any = any || route > 0, any_split = any_split || route < 0;
    }
    if (any_split) {  // the same three steps with the chains cut at the restart markers; each returns at once for any other frame
      hipLaunchKernelGGL(jpgd_split_unstuff_kernel, dim3(nf), dim3(kJpgdSyncLanes), 0, s, files, (const long long*)offsets, (const int*)plan, L,
                         (uint8_t*)work);
      hipLaunchKernelGGL(jpgd_split_relax_kernel, dim3(nf), dim3(kJpgdSyncLanes), 0, s, (const int*)plan, L, (uint8_t*)work);
      hipLaunchKernelGGL(jpgd_split_write_kernel, dim3(split, nf), dim3(kJpgdLanes), 0, s, (const int*)plan, L, (uint8_t*)work, (int*)status);
    }
    if (any) {  // each returns at once for a frame on another route, as jpgd_entropy_kernel does for the others
      hipLaunchKernelGGL(jpgd_unstuff_kernel, dim3(nf), dim3(kJpgdSyncLanes), 0, s, files, (const long long*)offsets, (const int*)plan, L,
                         (uint8_t*)work);
      hipLaunchKernelGGL(jpgd_relax_kernel, dim3(nf), dim3(kJpgdSyncLanes), 0, s, (const int*)plan, L, (uint8_t*)work);
      hipLaunchKernelGGL(jpgd_sync_write_kernel, dim3(sync, nf), dim3(kJpgdLanes), 0, s, (const int*)plan, L, (uint8_t*)work, (int*)status);
    }
    hipLaunchKernelGGL(jpgd_idct_kernel, dim3(idct, nf), dim3(kJpgdIdctBlocks * 8), 0, s, (const int*)plan, L, (uint8_t*)work);
    hipLaunchKernelGGL(jpgd_rgb_kernel, dim3(cols, (unsigned)H, nf), dim3(kJpgdRgbThreads), 0, s, (const int*)plan, L, (const uint8_t*)work,
                       rgb8_out);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
