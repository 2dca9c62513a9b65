// float_img_front / float_img_front_work_bytes: the image front end on the device (include/float_hip.h).
#include "imgf_kernels.hpp"

#include <numeric>

namespace {
constexpr int32_t kImgfMaxSrc = 16384;   // source sides
constexpr int32_t kImgfMaxDst = 4096;    // destination sides
constexpr int32_t kImgfMaxWin = 32768;   // window extents and both terms of a scale: 255 P < 2^23, n Q and (d + 1) P < 2^31
constexpr int32_t kImgfMaxOff = 65536;   // |rect_x|, |rect_y|

bool imgf_sizes_ok(int32_t src_h, int32_t src_w, int32_t dst_h, int32_t dst_w) {
  return src_h >= 1 && src_h <= kImgfMaxSrc && src_w >= 1 && src_w <= kImgfMaxSrc && dst_h >= 1 && dst_h <= kImgfMaxDst && dst_w >= 1 &&
         dst_w <= kImgfMaxDst;
}
}  // namespace

extern "C" {

size_t float_img_front_work_bytes(int32_t src_h, int32_t src_w, int32_t dst_h, int32_t dst_w) {
  if (!imgf_sizes_ok(src_h, src_w, dst_h, dst_w)) return 0;
  return (size_t)src_h * (size_t)dst_w * 3 * sizeof(int32_t);  // one row of sums per source row a window can hold
}

int float_img_front(const float* img, int32_t src_h, int32_t src_w, int32_t channels, int32_t rect_x, int32_t rect_y, int32_t rect_w,
                    int32_t rect_h, int32_t scale_num, int32_t scale_den, int32_t rgba_mode, int32_t bkg_r, int32_t bkg_g, int32_t bkg_b,
                    int32_t out_mode, void* out, int32_t dst_h, int32_t dst_w, void* work, size_t work_bytes, void* stream) {
  FH_REQUIRE(img && out && work, "float_img_front: null argument (img, out or work)");
  FH_REQUIRE(channels == 3 || channels == 4, "float_img_front: channels (%d) must be 3 or 4", channels);
  FH_REQUIRE(src_h >= 1 && src_h <= kImgfMaxSrc && src_w >= 1 && src_w <= kImgfMaxSrc,
             "float_img_front: source sides (%d x %d) must be 1 ... %d", src_h, src_w, kImgfMaxSrc);
  FH_REQUIRE(dst_h >= 1 && dst_h <= kImgfMaxDst && dst_w >= 1 && dst_w <= kImgfMaxDst,
             "float_img_front: destination sides (%d x %d) must be 1 ... %d", dst_h, dst_w, kImgfMaxDst);
  FH_REQUIRE(rect_w >= 1 && rect_w <= kImgfMaxWin && rect_h >= 1 && rect_h <= kImgfMaxWin,
             "float_img_front: window extents (%d x %d) must be 1 ... %d", rect_h, rect_w, kImgfMaxWin);
  FH_REQUIRE(rect_x >= -kImgfMaxOff && rect_x <= kImgfMaxOff && rect_y >= -kImgfMaxOff && rect_y <= kImgfMaxOff,
             "float_img_front: window origin (%d, %d) must be within +-%d", rect_x, rect_y, kImgfMaxOff);
  FH_REQUIRE((scale_num == 0 && scale_den == 0) || (scale_num >= 1 && scale_den >= 1),
             "float_img_front: scale_num (%d) and scale_den (%d) must be both 0 or both positive", scale_num, scale_den);
  FH_REQUIRE(rgba_mode == FLOAT_IMG_RGBA_DISCARD || rgba_mode == FLOAT_IMG_RGBA_BLEND || rgba_mode == FLOAT_IMG_RGBA_REPLACE,
             "float_img_front: unknown rgba_mode (%d)", rgba_mode);
  FH_REQUIRE(bkg_r >= 0 && bkg_r <= 255 && bkg_g >= 0 && bkg_g <= 255 && bkg_b >= 0 && bkg_b <= 255,
             "float_img_front: background colour (%d, %d, %d) must be 0 ... 255 per channel", bkg_r, bkg_g, bkg_b);
  FH_REQUIRE(out_mode == FLOAT_IMG_OUT_NCHW_PM1 || out_mode == FLOAT_IMG_OUT_HWC_U8, "float_img_front: unknown out_mode (%d)", out_mode);
  FH_REQUIRE(((uintptr_t)img & (channels == 4 ? 15u : 3u)) == 0, "float_img_front: img must be %d-byte aligned for %d channels",
             channels == 4 ? 16 : 4, channels);
  FH_REQUIRE(out_mode == FLOAT_IMG_OUT_HWC_U8 || ((uintptr_t)out & 3u) == 0, "float_img_front: out must be 4-byte aligned for fp32 output");
  FH_REQUIRE(((uintptr_t)work & 3u) == 0, "float_img_front: work must be 4-byte aligned");

  ImgfPlan p{};
  p.x.n = rect_w, p.x.off = rect_x, p.x.src = src_w, p.x.dst = dst_w;
  p.y.n = rect_h, p.y.off = rect_y, p.y.src = src_h, p.y.dst = dst_h;
  for (ImgfAxis* a : {&p.x, &p.y}) {
    const int num = scale_num ? scale_num : a->n, den = scale_num ? scale_den : a->dst;
    const int g = std::gcd(num, den);
    a->P = num / g, a->Q = den / g;
    FH_REQUIRE(a->P <= kImgfMaxWin && a->Q <= kImgfMaxWin, "float_img_front: scale %d / %d reduces to %d / %d, both terms must be at most %d",
               num, den, a->P, a->Q, kImgfMaxWin);
    FH_REQUIRE((long long)(a->dst - 1) * a->P < (long long)a->n * a->Q,
               "float_img_front: destination cell %d starts outside the window (extent %d at scale %d / %d)", a->dst - 1, a->n, a->P, a->Q);
  }
  const size_t need = float_img_front_work_bytes(src_h, src_w, dst_h, dst_w);
  FH_REQUIRE(work_bytes >= need, "float_img_front: work_bytes %zu < float_img_front_work_bytes(%d, %d, %d, %d) = %zu", work_bytes, src_h,
             src_w, dst_h, dst_w, need);

  p.channels = channels, p.rgba_mode = rgba_mode, p.out_mode = out_mode;
  p.bkg[0] = bkg_r, p.bkg[1] = bkg_g, p.bkg[2] = bkg_b;
  p.linear = (p.x.P < p.x.Q || p.y.P < p.y.Q) ? 1 : 0;
  p.row_lo = std::max(0, rect_y);
  p.rows = std::max(0, std::min(src_h, rect_y + rect_h) - p.row_lo);
  // a tile of kImgfTile columns reads at most ceil(kImgfTile P / Q) + 2 samples of a row, and never more than the row holds
  const long long span = ((long long)kImgfTile * p.x.P + p.x.Q - 1) / p.x.Q + 2;
  p.lds_px = (int)std::min<long long>(span, src_w);  // <= 16384 dwords = 64 KiB, the dynamic LDS a launch gets without asking

  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)((dst_w + kImgfTile - 1) / kImgfTile);
  if (p.rows > 0 && rect_x < src_w && rect_x + rect_w > 0)  // otherwise the window holds the zero border only
    hipLaunchKernelGGL(imgf_rows_kernel, dim3(tiles, (unsigned)p.rows), dim3(kImgfTile), (size_t)p.lds_px * sizeof(unsigned), s, img,
                       (int*)work, p);
  else
    p.rows = 0;
  hipLaunchKernelGGL(imgf_cols_kernel, dim3(tiles, (unsigned)dst_h), dim3(kImgfTile), 0, s, (const int*)work, out, p);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
