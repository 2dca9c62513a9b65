// float_img_paste, float_img_paste_i420: the generated frames back in the source portrait on the device, as 8-bit RGB or as planar
// YUV 4:2:0 (include/float_hip.h).
#include "imgp_kernels.hpp"

namespace {
constexpr int32_t kImgpMaxSrc = 16384;    // source and box sides, feather
constexpr int32_t kImgpMaxFrame = 1024;   // sides of a generated frame: what keeps every sum in 32 bits (imgp_kernels.hpp).  A side that
                                          // equals the box's (frames already resampled: float_img_resample) reduces to P = Q = 1 on that
                                          // axis, so it may be as long as the box; a frame is then still below 3 * 2^28 bytes
constexpr int32_t kImgpMaxOff = 1 << 30;  // |rect_x|, |rect_y|: origin + side stays in 32 bits
constexpr unsigned kImgpMaxGrid = 1u << 30;
}  // namespace

extern "C" {

int float_img_paste(const uint8_t* src8, int32_t src_h, int32_t src_w, const uint8_t* frames8, int32_t n_frames, int32_t fr_h, int32_t fr_w,
                    int32_t rect_x, int32_t rect_y, int32_t rect_w, int32_t rect_h, int32_t feather, uint8_t* out, void* stream) {
  FH_REQUIRE(src8 && frames8 && out, "float_img_paste: null argument (src8, frames8 or out)");
  FH_REQUIRE(src_h >= 1 && src_h <= kImgpMaxSrc && src_w >= 1 && src_w <= kImgpMaxSrc,
             "float_img_paste: source sides src_h, src_w (%d x %d) must be 1 ... %d", src_h, src_w, kImgpMaxSrc);
  FH_REQUIRE(n_frames >= 1, "float_img_paste: n_frames (%d) must be at least 1", n_frames);
  FH_REQUIRE(fr_h >= 1 && (fr_h <= kImgpMaxFrame || fr_h == rect_h) && fr_w >= 1 && (fr_w <= kImgpMaxFrame || fr_w == rect_w),
             "float_img_paste: frame sides fr_h, fr_w (%d x %d) must be 1 ... %d, or the box's own", fr_h, fr_w, kImgpMaxFrame);
  FH_REQUIRE(rect_w >= 1 && rect_w <= kImgpMaxSrc && rect_h >= 1 && rect_h <= kImgpMaxSrc,
             "float_img_paste: box sides rect_h, rect_w (%d x %d) must be 1 ... %d", rect_h, rect_w, kImgpMaxSrc);
  FH_REQUIRE(rect_x >= -kImgpMaxOff && rect_x <= kImgpMaxOff && rect_y >= -kImgpMaxOff && rect_y <= kImgpMaxOff,
             "float_img_paste: box origin rect_x, rect_y (%d, %d) must be within +-%d", rect_x, rect_y, kImgpMaxOff);
  FH_REQUIRE(feather >= 0 && feather <= kImgpMaxSrc, "float_img_paste: feather (%d) must be 0 ... %d", feather, kImgpMaxSrc);

  ImgpPlan p = imgp_make_plan(src_h, src_w, fr_h, fr_w, rect_x, rect_y, rect_w, rect_h, feather);

  // one launch; a clip of more frames than a grid holds goes in groups of whole frames
  hipStream_t s = (hipStream_t)stream;
  const int32_t group = (int32_t)std::max(1u, kImgpMaxGrid / p.spans);
  for (int32_t f0 = 0; f0 < n_frames; f0 += group) {
    p.n_frames = std::min(group, n_frames - f0);
    hipLaunchKernelGGL(imgp_paste_kernel, dim3(p.spans * (unsigned)p.n_frames), dim3(kImgpThreads), 0, s, src8,
                       frames8 + (size_t)f0 * p.in_bytes, out + (size_t)f0 * p.frame_bytes, p);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

int float_img_paste_i420(const uint8_t* src8, int32_t src_h, int32_t src_w, const uint8_t* frames8, int32_t n_frames, int32_t fr_h, int32_t fr_w,
                         int32_t rect_x, int32_t rect_y, int32_t rect_w, int32_t rect_h, int32_t feather, int32_t matrix, uint8_t* out,
                         void* stream) {
  FH_REQUIRE(src8 && frames8 && out, "float_img_paste_i420: null argument (src8, frames8 or out)");
  FH_REQUIRE(src_h >= 2 && src_h <= kImgpMaxSrc && src_w >= 2 && src_w <= kImgpMaxSrc && src_h % 2 == 0 && src_w % 2 == 0,
             "float_img_paste_i420: source sides src_h, src_w (%d x %d) must be even and 2 ... %d (4:2:0 chroma)", src_h, src_w, kImgpMaxSrc);
  FH_REQUIRE(n_frames >= 1, "float_img_paste_i420: n_frames (%d) must be at least 1", n_frames);
  FH_REQUIRE(fr_h >= 1 && (fr_h <= kImgpMaxFrame || fr_h == rect_h) && fr_w >= 1 && (fr_w <= kImgpMaxFrame || fr_w == rect_w),
             "float_img_paste_i420: frame sides fr_h, fr_w (%d x %d) must be 1 ... %d, or the box's own", fr_h, fr_w, kImgpMaxFrame);
  FH_REQUIRE(rect_w >= 1 && rect_w <= kImgpMaxSrc && rect_h >= 1 && rect_h <= kImgpMaxSrc,
             "float_img_paste_i420: box sides rect_h, rect_w (%d x %d) must be 1 ... %d", rect_h, rect_w, kImgpMaxSrc);
  FH_REQUIRE(rect_x >= -kImgpMaxOff && rect_x <= kImgpMaxOff && rect_y >= -kImgpMaxOff && rect_y <= kImgpMaxOff,
             "float_img_paste_i420: box origin rect_x, rect_y (%d, %d) must be within +-%d", rect_x, rect_y, kImgpMaxOff);
  FH_REQUIRE(feather >= 0 && feather <= kImgpMaxSrc, "float_img_paste_i420: feather (%d) must be 0 ... %d", feather, kImgpMaxSrc);
  FhYuv t;
  FH_REQUIRE(fh_yuv_of(matrix, &t), "float_img_paste_i420: matrix (%d) must be one of " FH_YUV_IDS, matrix);

  ImgpPlan p = imgp_make_plan(src_h, src_w, fr_h, fr_w, rect_x, rect_y, rect_w, rect_h, feather);
  const ImgpYuv q = imgp_make_yuv(src_h, src_w);
  const size_t out_bytes = (size_t)q.y_bytes + 2u * (size_t)q.c_bytes;  // 3 H W / 2
  // dword and 16-bit stores where every frame, plane and row is aligned for them; else bytes (imgp_kernels.hpp)
  const bool fast = src_w % 4 == 0 && ((uintptr_t)out & 3u) == 0;

  void (*kern)(const unsigned char*, const unsigned char*, unsigned char*, ImgpPlan, ImgpYuv);
  switch (matrix) {
    case 2: kern = fast ? imgp_paste_i420_kernel<true, 2> : imgp_paste_i420_kernel<false, 2>; break;
    case 4: kern = fast ? imgp_paste_i420_kernel<true, 4> : imgp_paste_i420_kernel<false, 4>; break;
    case 6: kern = fast ? imgp_paste_i420_kernel<true, 6> : imgp_paste_i420_kernel<false, 6>; break;
    default: kern = fast ? imgp_paste_i420_kernel<true, 0> : imgp_paste_i420_kernel<false, 0>;
  }

  // one launch; a clip of more frames than a grid holds goes in groups of whole frames
  hipStream_t s = (hipStream_t)stream;
  const int32_t group = (int32_t)std::max(1u, kImgpMaxGrid / q.spans);
  for (int32_t f0 = 0; f0 < n_frames; f0 += group) {
    p.n_frames = std::min(group, n_frames - f0);
    const dim3 grid(q.spans * (unsigned)p.n_frames);
    const uint8_t* fr = frames8 + (size_t)f0 * p.in_bytes;
    uint8_t* o = out + (size_t)f0 * out_bytes;
    hipLaunchKernelGGL(kern, grid, dim3(kImgpThreads), 0, s, src8, fr, o, p, q);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
