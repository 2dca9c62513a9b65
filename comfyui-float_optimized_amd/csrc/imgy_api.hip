// float_img_front_frames_yuv: the frame-stacked image front end reading 8-bit YUV 4:2:0, I420 or NV12 (include/float_hip.h).
#include "imgy_kernels.hpp"

#include <algorithm>
#include <numeric>

namespace {
// float_img_front_frames' limits (imgv_api.hip)
constexpr int32_t kImgyMaxSrc = 16384, kImgyMaxDst = 4096, kImgyMaxWin = 32768, kImgyMaxOff = 65536;
constexpr int32_t kImgyMaxFrames = 65535;

template <int LAYOUT, bool CENTRE>
void imgy_launch(const ImgyArgs& a, dim3 grid, hipStream_t s) {
  const size_t lds = (size_t)kImgvWaves * (a.v.stage_px + ImgySrc<LAYOUT, CENTRE>::kSlots * a.chroma_dw) * sizeof(unsigned);  // <= 48.2 KiB
  hipLaunchKernelGGL((imgv_frames_kernel<ImgySrc<LAYOUT, CENTRE>>), grid, dim3(kImgvCols * kImgvWaves), lds, s, a);
}
}  // namespace

extern "C" {

int float_img_front_frames_yuv(const uint8_t* frames, int32_t n_frames, int32_t src_h, int32_t src_w, int32_t layout, int32_t matrix,
                               int32_t chroma, const int32_t* rects, int32_t scale_num, int32_t scale_den, uint8_t* out, int32_t dst_h,
                               int32_t dst_w, void* stream) {
  const char* fn = "float_img_front_frames_yuv";
  FH_REQUIRE(frames && rects && out, "%s: null argument (frames, rects or out)", fn);
  FH_REQUIRE(n_frames >= 1 && n_frames <= kImgyMaxFrames, "%s: n_frames (%d) must be 1 ... %d", fn, n_frames, kImgyMaxFrames);
  FH_REQUIRE(layout == FLOAT_IMG_YUV_I420 || layout == FLOAT_IMG_YUV_NV12, "%s: unknown layout (%d)", fn, layout);
  FH_REQUIRE(chroma == FLOAT_IMG_CHROMA_NEAREST || chroma == FLOAT_IMG_CHROMA_CENTRE, "%s: unknown chroma rule (%d)", fn, chroma);
  ImgyArgs a{};
  FH_REQUIRE(fh_yuv_inverse_of(matrix, &a.k), "%s: unknown matrix (%d): " FH_YUV_IDS, fn, matrix);
  FH_REQUIRE(src_h >= 2 && src_h <= kImgyMaxSrc && src_w >= 2 && src_w <= kImgyMaxSrc, "%s: source sides (%d x %d) must be 2 ... %d", fn,
             src_h, src_w, kImgyMaxSrc);
  FH_REQUIRE(src_h % 2 == 0 && src_w % 2 == 0, "%s: source sides (%d x %d) must be even for 4:2:0 chroma", fn, src_h, src_w);
  FH_REQUIRE(dst_h >= 1 && dst_h <= kImgyMaxDst && dst_w >= 1 && dst_w <= kImgyMaxDst, "%s: destination sides (%d x %d) must be 1 ... %d",
             fn, dst_h, dst_w, kImgyMaxDst);
  FH_REQUIRE((scale_num == 0 && scale_den == 0) || (scale_num >= 1 && scale_den >= 1),
             "%s: scale_num (%d) and scale_den (%d) must be both 0 or both positive", fn, scale_num, scale_den);
  int P = 0, Q = 0;  // the shared scale, reduced
  if (scale_num) {
    const int g = std::gcd(scale_num, scale_den);
    P = scale_num / g, Q = scale_den / g;
    FH_REQUIRE(P <= kImgyMaxWin && Q <= kImgyMaxWin, "%s: scale %d / %d reduces to %d / %d, both terms must be at most %d", fn, scale_num,
               scale_den, P, Q, kImgyMaxWin);
  }
  for (int32_t f = 0; f < n_frames; ++f) {  // every rect before any HIP call
    const int32_t *r = rects + 4 * (size_t)f, x = r[0], y = r[1], w = r[2], h = r[3];
    FH_REQUIRE(w >= 1 && w <= kImgyMaxWin && h >= 1 && h <= kImgyMaxWin, "%s: frame %d: window extents (%d x %d) must be 1 ... %d", fn, f,
               h, w, kImgyMaxWin);
    FH_REQUIRE(x >= -kImgyMaxOff && x <= kImgyMaxOff && y >= -kImgyMaxOff && y <= kImgyMaxOff,
               "%s: frame %d: window origin (%d, %d) must be within +-%d", fn, f, x, y, kImgyMaxOff);
    if (P)
      FH_REQUIRE((long long)(dst_w - 1) * P < (long long)w * Q && (long long)(dst_h - 1) * P < (long long)h * Q,
                 "%s: frame %d: the last destination cell starts outside the window (%d x %d at scale %d / %d)", fn, f, h, w, P, Q);
  }

  a.v.src_h = src_h, a.v.src_w = src_w, a.v.dst_h = dst_h, a.v.dst_w = dst_w;
  a.v.channels = 3, a.v.rgba_mode = FLOAT_IMG_RGBA_DISCARD;
  a.v.scale_num = P, a.v.scale_den = Q;
  // libjpeg replicates instead where the chroma plane is at most 2 samples wide, and so does the definition
  const bool centre = chroma == FLOAT_IMG_CHROMA_CENTRE && src_w > 4;
  const size_t frame_bytes = (size_t)src_h * src_w * 3 / 2;
  const dim3 tiles((unsigned)((dst_w + kImgvCols - 1) / kImgvCols), (unsigned)((dst_h + kImgvRows - 1) / kImgvRows));
  hipStream_t s = (hipStream_t)stream;
  for (int32_t at = 0; at < n_frames; at += kImgvBlock) {
    const int nb = std::min(kImgvBlock, n_frames - at);
    long long span = 1;  // the widest span of a tile's row among the block's frames, + 1 for the even first column
    for (int f = 0; f < nb; ++f) {
      for (int k = 0; k < 4; ++k) a.v.rect[f][k] = rects[4 * (size_t)(at + f) + k];
      const long long num = P ? P : a.v.rect[f][2], den = P ? Q : dst_w;
      span = std::max(span, (kImgvCols * num + den - 1) / den + 3);
    }
    a.v.stage_px = (int)((std::min<long long>({span, (long long)src_w, (long long)kImgyStage}) + 3) & ~3LL);  // a multiple of 4
    a.chroma_dw = (a.v.stage_px / 4 + 4 + 3) & ~3;  // a multiple of 4: every wave's RGB slice then begins on 16 bytes
    a.v.frames = frames + (size_t)at * frame_bytes;
    a.v.out = out + (size_t)at * dst_h * dst_w * 3;
    a.v.bytes = (unsigned long long)nb * frame_bytes;
    const dim3 grid(tiles.x, tiles.y, (unsigned)nb);
    if (layout == FLOAT_IMG_YUV_NV12)
      centre ? imgy_launch<kImgyNv12, true>(a, grid, s) : imgy_launch<kImgyNv12, false>(a, grid, s);
    else
      centre ? imgy_launch<kImgyI420, true>(a, grid, s) : imgy_launch<kImgyI420, false>(a, grid, s);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
