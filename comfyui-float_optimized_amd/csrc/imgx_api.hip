// float_img_front_frames_planes: the frame-stacked image front end reading planar / semi-planar YUV of 8, 10 or 12 bits at
// 4:2:0, 4:2:2 or 4:4:4, pitched, as it lies in the caller's buffer (include/float_hip.h).
#include "imgx_kernels.hpp"

#include <algorithm>
#include <numeric>

namespace {
// float_img_front_frames' limits (imgv_api.hip)
constexpr int32_t kImgxMaxSrc = 16384, kImgxMaxDst = 4096, kImgxMaxWin = 32768, kImgxMaxOff = 65536;
constexpr int32_t kImgxMaxFrames = 65535;
constexpr int32_t kImgxMaxPitch = 1 << 20;  // bytes: far above 16384 samples of 4 bytes, and rows x pitch stays inside int64 by miles

template <int BITS, int HS, int VS, bool CENTRE>
void imgx_launch(const ImgxArgs& a, dim3 grid, hipStream_t s) {
  using Src = ImgxSrc<BITS, HS, VS, CENTRE>;
  const size_t lds = (size_t)kImgvWaves * (a.v.stage_px + Src::kSlots * a.chroma_dw) * sizeof(unsigned);  // <= 48.2 KiB (imgx_kernels.hpp)
  hipLaunchKernelGGL((imgv_frames_kernel<Src>), grid, dim3(kImgvCols * kImgvWaves), lds, s, a);
}

template <int BITS>
void imgx_launch_geometry(const ImgxArgs& a, int hs, int vs, bool centre, dim3 grid, hipStream_t s) {
  if (hs == 1)
    imgx_launch<BITS, 1, 1, false>(a, grid, s);  // 4:4:4 has nothing to interpolate
  else if (vs == 1)
    centre ? imgx_launch<BITS, 2, 1, true>(a, grid, s) : imgx_launch<BITS, 2, 1, false>(a, grid, s);
  else
    centre ? imgx_launch<BITS, 2, 2, true>(a, grid, s) : imgx_launch<BITS, 2, 2, false>(a, grid, s);
}

struct Extent {
  long long lo, hi;  // bytes [lo, hi) of a frame
};
}  // namespace

extern "C" {

int float_img_front_frames_planes(const uint8_t* data, uint64_t data_bytes, int32_t n_frames, int32_t src_h, int32_t src_w,
                                  const float_img_planes_t* fmt, int32_t matrix, int32_t chroma, const int32_t* rects, int32_t scale_num,
                                  int32_t scale_den, uint8_t* out, int32_t dst_h, int32_t dst_w, void* stream) {
  const char* fn = "float_img_front_frames_planes";
  FH_REQUIRE(data && fmt && rects && out, "%s: null argument (data, fmt, rects or out)", fn);
  FH_REQUIRE(n_frames >= 1 && n_frames <= kImgxMaxFrames, "%s: n_frames (%d) must be 1 ... %d", fn, n_frames, kImgxMaxFrames);
  const int hs = fmt->hs, vs = fmt->vs, depth = fmt->depth;
  FH_REQUIRE((hs == 2 && vs == 2) || (hs == 2 && vs == 1) || (hs == 1 && vs == 1),
             "%s: chroma geometry %d x %d is not read (2 x 2 = 4:2:0, 2 x 1 = 4:2:2, 1 x 1 = 4:4:4)", fn, hs, vs);
  FH_REQUIRE(depth == 8 || depth == 10 || depth == 12, "%s: depth (%d) must be 8, 10 or 12 (16-bit samples would overflow int32)", fn, depth);
  const int bytes = depth == 8 ? 1 : 2;
  FH_REQUIRE(fmt->shift >= 0 && fmt->shift <= 8 * bytes - depth, "%s: shift (%d) must be 0 ... %d at depth %d", fn, fmt->shift,
             8 * bytes - depth, depth);
  FH_REQUIRE(chroma == FLOAT_IMG_CHROMA_NEAREST || chroma == FLOAT_IMG_CHROMA_CENTRE, "%s: unknown chroma rule (%d)", fn, chroma);
  ImgxArgs a{};
  FH_REQUIRE(fh_yuv_inverse_of(matrix, &a.k), "%s: unknown matrix (%d): " FH_YUV_IDS, fn, matrix);
  FH_REQUIRE(src_h >= 1 && src_h <= kImgxMaxSrc && src_w >= 1 && src_w <= kImgxMaxSrc, "%s: source sides (%d x %d) must be 1 ... %d", fn,
             src_h, src_w, kImgxMaxSrc);
  // the planes: steps and pitches cover a row, 16-bit samples lie on even bytes, every plane inside the frame and the buffer
  const int cw = (src_w + hs - 1) / hs, ch = (src_h + vs - 1) / vs;
  const bool semi = fmt->c_step == 2 * bytes;
  FH_REQUIRE(fmt->c_step == bytes || semi, "%s: c_step (%d) must be %d (planar) or %d (semi-planar) at depth %d", fn, fmt->c_step, bytes,
             2 * bytes, depth);
  const long long y_row = (long long)src_w * bytes, c_row = (long long)(cw - 1) * fmt->c_step + bytes;
  FH_REQUIRE(fmt->y_pitch >= y_row && fmt->y_pitch <= kImgxMaxPitch && fmt->c_pitch >= c_row + (semi ? bytes : 0) && fmt->c_pitch <= kImgxMaxPitch,
             "%s: pitches (%d, %d) must cover a row (%lld, %lld bytes) and be at most %d", fn, fmt->y_pitch, fmt->c_pitch, y_row,
             c_row + (semi ? bytes : 0), kImgxMaxPitch);
  FH_REQUIRE(bytes == 1 || !((fmt->y_off | fmt->u_off | fmt->v_off | fmt->frame_stride | fmt->y_pitch | fmt->c_pitch) & 1),
             "%s: offsets, pitches and the frame stride of 16-bit planes must be even", fn);
  FH_REQUIRE(fmt->y_off >= 0 && fmt->u_off >= 0 && fmt->v_off >= 0 && fmt->frame_stride >= 0, "%s: negative offset or frame stride", fn);
  FH_REQUIRE(!semi || fmt->u_off - fmt->v_off == bytes || fmt->v_off - fmt->u_off == bytes,
             "%s: semi-planar U and V must be %d byte(s) apart (u_off %lld, v_off %lld)", fn, bytes, (long long)fmt->u_off, (long long)fmt->v_off);
  Extent e[3] = {{fmt->y_off, fmt->y_off + (long long)(src_h - 1) * fmt->y_pitch + y_row},
                 {fmt->u_off, fmt->u_off + (long long)(ch - 1) * fmt->c_pitch + c_row},
                 {fmt->v_off, fmt->v_off + (long long)(ch - 1) * fmt->c_pitch + c_row}};
  int n_ext = 3;
  if (semi) e[1] = Extent{std::min(e[1].lo, e[2].lo), std::max(e[1].hi, e[2].hi)}, n_ext = 2;  // one interleaved plane
  std::sort(e, e + n_ext, [](const Extent& p, const Extent& q) { return p.lo < q.lo; });
  for (int i = 0; i + 1 < n_ext; ++i)
    FH_REQUIRE(e[i].hi <= e[i + 1].lo, "%s: planes overlap (bytes %lld ... %lld and %lld ... %lld of a frame)", fn, e[i].lo, e[i].hi,
               e[i + 1].lo, e[i + 1].hi);
  const long long frame_end = e[n_ext - 1].hi;
  FH_REQUIRE(n_frames == 1 || fmt->frame_stride >= frame_end, "%s: frame_stride (%lld) is below the last plane's end (%lld)", fn,
             (long long)fmt->frame_stride, frame_end);
  FH_REQUIRE((unsigned long long)(n_frames - 1) * (unsigned long long)fmt->frame_stride + (unsigned long long)frame_end <= data_bytes,
             "%s: %d frames of stride %lld whose planes end at byte %lld need %llu bytes, data holds %llu", fn, n_frames,
             (long long)fmt->frame_stride, frame_end,
             (unsigned long long)(n_frames - 1) * (unsigned long long)fmt->frame_stride + (unsigned long long)frame_end,
             (unsigned long long)data_bytes);
  FH_REQUIRE(dst_h >= 1 && dst_h <= kImgxMaxDst && dst_w >= 1 && dst_w <= kImgxMaxDst, "%s: destination sides (%d x %d) must be 1 ... %d",
             fn, dst_h, dst_w, kImgxMaxDst);
  FH_REQUIRE((scale_num == 0 && scale_den == 0) || (scale_num >= 1 && scale_den >= 1),
             "%s: scale_num (%d) and scale_den (%d) must be both 0 or both positive", fn, scale_num, scale_den);
  int P = 0, Q = 0;  // the shared scale, reduced
  if (scale_num) {
    const int g = std::gcd(scale_num, scale_den);
    P = scale_num / g, Q = scale_den / g;
    FH_REQUIRE(P <= kImgxMaxWin && Q <= kImgxMaxWin, "%s: scale %d / %d reduces to %d / %d, both terms must be at most %d", fn, scale_num,
               scale_den, P, Q, kImgxMaxWin);
  }
  for (int32_t f = 0; f < n_frames; ++f) {  // every rect before any HIP call
    const int32_t *r = rects + 4 * (size_t)f, x = r[0], y = r[1], w = r[2], h = r[3];
    FH_REQUIRE(w >= 1 && w <= kImgxMaxWin && h >= 1 && h <= kImgxMaxWin, "%s: frame %d: window extents (%d x %d) must be 1 ... %d", fn, f,
               h, w, kImgxMaxWin);
    FH_REQUIRE(x >= -kImgxMaxOff && x <= kImgxMaxOff && y >= -kImgxMaxOff && y <= kImgxMaxOff,
               "%s: frame %d: window origin (%d, %d) must be within +-%d", fn, f, x, y, kImgxMaxOff);
    if (P)
      FH_REQUIRE((long long)(dst_w - 1) * P < (long long)w * Q && (long long)(dst_h - 1) * P < (long long)h * Q,
                 "%s: frame %d: the last destination cell starts outside the window (%d x %d at scale %d / %d)", fn, f, h, w, P, Q);
  }

  a.v.src_h = src_h, a.v.src_w = src_w, a.v.dst_h = dst_h, a.v.dst_w = dst_w;
  a.v.channels = 3, a.v.rgba_mode = FLOAT_IMG_RGBA_DISCARD;
  a.v.scale_num = P, a.v.scale_den = Q;
  a.data = data, a.data_bytes = data_bytes;
  a.frame_stride = fmt->frame_stride, a.y_off = fmt->y_off, a.u_off = fmt->u_off, a.v_off = fmt->v_off;
  a.y_pitch = fmt->y_pitch, a.c_pitch = fmt->c_pitch, a.c_step = fmt->c_step;
  a.shift = fmt->shift, a.mask = (1 << depth) - 1, a.s = depth - 8;
  a.cw = cw, a.ch = ch;
  // libjpeg replicates instead where the chroma plane is at most 2 samples wide, and so does the definition
  const bool centre = chroma == FLOAT_IMG_CHROMA_CENTRE && hs == 2 && cw > 2;
  const int cap = bytes == 1 ? kImgxStage8 : kImgxStage16;
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
    a.v.stage_px = (int)((std::min<long long>({span, (long long)src_w, (long long)cap}) + 3) & ~3LL);  // a multiple of 4
    // a slot: one dword per group of 4 pixels at 8 bits, two at 16, + 4; a multiple of 4, so every wave's RGB slice begins on 16 bytes
    a.chroma_dw = (a.v.stage_px / 4 * (bytes == 1 ? 1 : 2) + 4 + 3) & ~3;
    a.v.frames = data + (size_t)at * (size_t)fmt->frame_stride;
    a.v.out = out + (size_t)at * dst_h * dst_w * 3;
    a.v.bytes = 0;
    const dim3 grid(tiles.x, tiles.y, (unsigned)nb);
    if (bytes == 1)
      imgx_launch_geometry<8>(a, hs, vs, centre, grid, s);
    else
      imgx_launch_geometry<16>(a, hs, vs, centre, grid, s);
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
