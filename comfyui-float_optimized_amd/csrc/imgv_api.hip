// float_img_front_frames: the image front end over a stack of frames, one window per frame (include/float_hip.h).
#include "imgv_kernels.hpp"

#include <algorithm>
#include <numeric>

namespace {
// float_img_front's limits (imgf_api.hip)
constexpr int32_t kImgvMaxSrc = 16384, kImgvMaxDst = 4096, kImgvMaxWin = 32768, kImgvMaxOff = 65536;
constexpr int32_t kImgvMaxFrames = 65535;
}  // namespace

extern "C" {

int float_img_front_frames(const void* frames, int32_t n_frames, int32_t src_h, int32_t src_w, int32_t channels, int32_t src_type,
                           const int32_t* rects, int32_t scale_num, int32_t scale_den, int32_t rgba_mode, int32_t bkg_r, int32_t bkg_g,
                           int32_t bkg_b, uint8_t* out, int32_t dst_h, int32_t dst_w, void* stream) {
  const char* fn = "float_img_front_frames";
  FH_REQUIRE(frames && rects && out, "%s: null argument (frames, rects or out)", fn);
  FH_REQUIRE(n_frames >= 1 && n_frames <= kImgvMaxFrames, "%s: n_frames (%d) must be 1 ... %d", fn, n_frames, kImgvMaxFrames);
  FH_REQUIRE(channels == 3 || channels == 4, "%s: channels (%d) must be 3 or 4", fn, channels);
  FH_REQUIRE(src_type == FLOAT_IMG_SRC_F32 || src_type == FLOAT_IMG_SRC_U8, "%s: unknown src_type (%d)", fn, src_type);
  FH_REQUIRE(src_h >= 1 && src_h <= kImgvMaxSrc && src_w >= 1 && src_w <= kImgvMaxSrc, "%s: source sides (%d x %d) must be 1 ... %d", fn,
             src_h, src_w, kImgvMaxSrc);
  FH_REQUIRE(dst_h >= 1 && dst_h <= kImgvMaxDst && dst_w >= 1 && dst_w <= kImgvMaxDst, "%s: destination sides (%d x %d) must be 1 ... %d",
             fn, dst_h, dst_w, kImgvMaxDst);
  FH_REQUIRE((scale_num == 0 && scale_den == 0) || (scale_num >= 1 && scale_den >= 1),
             "%s: scale_num (%d) and scale_den (%d) must be both 0 or both positive", fn, scale_num, scale_den);
  FH_REQUIRE(rgba_mode == FLOAT_IMG_RGBA_DISCARD || rgba_mode == FLOAT_IMG_RGBA_BLEND || rgba_mode == FLOAT_IMG_RGBA_REPLACE,
             "%s: unknown rgba_mode (%d)", fn, rgba_mode);
  FH_REQUIRE(bkg_r >= 0 && bkg_r <= 255 && bkg_g >= 0 && bkg_g <= 255 && bkg_b >= 0 && bkg_b <= 255,
             "%s: background colour (%d, %d, %d) must be 0 ... 255 per channel", fn, bkg_r, bkg_g, bkg_b);
  const bool u8 = src_type == FLOAT_IMG_SRC_U8;
  const unsigned align = u8 ? (channels == 4 ? 4u : 1u) : (channels == 4 ? 16u : 4u);
  FH_REQUIRE(((uintptr_t)frames & (align - 1)) == 0, "%s: frames must be %u-byte aligned for %d %s channels", fn, align, channels,
             u8 ? "8-bit" : "fp32");
  int P = 0, Q = 0;  // the shared scale, reduced
  if (scale_num) {
    const int g = std::gcd(scale_num, scale_den);
    P = scale_num / g, Q = scale_den / g;
    FH_REQUIRE(P <= kImgvMaxWin && Q <= kImgvMaxWin, "%s: scale %d / %d reduces to %d / %d, both terms must be at most %d", fn, scale_num,
               scale_den, P, Q, kImgvMaxWin);
  }
  // every rect before any HIP call; a frame's own scale is left unreduced (rect_w / dst_w: n Q and (d + 1) P stay below 2^27)
  for (int32_t f = 0; f < n_frames; ++f) {
    const int32_t *r = rects + 4 * (size_t)f, x = r[0], y = r[1], w = r[2], h = r[3];
    FH_REQUIRE(w >= 1 && w <= kImgvMaxWin && h >= 1 && h <= kImgvMaxWin, "%s: frame %d: window extents (%d x %d) must be 1 ... %d", fn, f,
               h, w, kImgvMaxWin);
    FH_REQUIRE(x >= -kImgvMaxOff && x <= kImgvMaxOff && y >= -kImgvMaxOff && y <= kImgvMaxOff,
               "%s: frame %d: window origin (%d, %d) must be within +-%d", fn, f, x, y, kImgvMaxOff);
    if (P)
      FH_REQUIRE((long long)(dst_w - 1) * P < (long long)w * Q && (long long)(dst_h - 1) * P < (long long)h * Q,
                 "%s: frame %d: the last destination cell starts outside the window (%d x %d at scale %d / %d)", fn, f, h, w, P, Q);
  }

  ImgvArgs a{};
  a.src_h = src_h, a.src_w = src_w, a.dst_h = dst_h, a.dst_w = dst_w;
  a.channels = channels, a.rgba_mode = rgba_mode;
  a.bkg[0] = bkg_r, a.bkg[1] = bkg_g, a.bkg[2] = bkg_b;
  a.scale_num = P, a.scale_den = Q;
  const size_t frame_bytes = (size_t)src_h * src_w * channels * (u8 ? 1 : 4);
  const dim3 tiles((unsigned)((dst_w + kImgvCols - 1) / kImgvCols), (unsigned)((dst_h + kImgvRows - 1) / kImgvRows));
  hipStream_t s = (hipStream_t)stream;
  for (int32_t at = 0; at < n_frames; at += kImgvBlock) {
    const int nb = std::min(kImgvBlock, n_frames - at);
    long long span = 1;  // the widest span of a tile's row among the block's frames: ceil(64 P / Q) + 2 samples
    for (int f = 0; f < nb; ++f) {
      for (int k = 0; k < 4; ++k) a.rect[f][k] = rects[4 * (size_t)(at + f) + k];
      const long long num = P ? P : a.rect[f][2], den = P ? Q : dst_w;
      span = std::max(span, (kImgvCols * num + den - 1) / den + 2);
    }
    a.stage_px = (int)std::min<long long>({span, (long long)src_w, (long long)kImgvStage});
    a.frames = (const unsigned char*)frames + (size_t)at * frame_bytes;
    a.out = out + (size_t)at * dst_h * dst_w * 3;
    a.bytes = (unsigned long long)nb * frame_bytes;
    const dim3 grid(tiles.x, tiles.y, (unsigned)nb);
    const size_t lds = (size_t)kImgvWaves * a.stage_px * sizeof(unsigned);  // <= 64 KiB
    if (u8)
      hipLaunchKernelGGL(imgv_frames_kernel<ImgvSrcU8>, grid, dim3(kImgvCols * kImgvWaves), lds, s, a);
    else
      hipLaunchKernelGGL(imgv_frames_kernel<ImgvSrcF32>, grid, dim3(kImgvCols * kImgvWaves), lds, s, a);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
