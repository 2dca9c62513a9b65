// float_img_blend_plan / float_img_blend_plan_ints (host only), float_img_blend / float_img_blend_work_bytes: the generated face joined
// to the portrait by a multi-band (Laplacian pyramid) blend on the device (include/float_hip.h).
#include <vector>

#include "imgb_kernels.hpp"

namespace {
constexpr int32_t kImgbMaxSrc = 16384;    // source, box and window sides, inset: float_img_paste's
constexpr int32_t kImgbMaxOff = 1 << 30;  // |rect_x|, |rect_y|
constexpr unsigned kImgbMaxGridZ = 65535;

// the pyramid over a window: extents, where each level of the mask starts (in values) and where D_l and R_l of one frame start in
// `work` (in bytes, 16-byte aligned): D_1 ... D_L as int16 x 3, then R_1 ... R_{L-1} as int32 x 3
struct ImgbGeom {
  int levels;
  int h[kImgbMaxLevels + 1], w[kImgbMaxLevels + 1];
  size_t m_off[kImgbMaxLevels + 2];
  size_t d_off[kImgbMaxLevels + 1], r_off[kImgbMaxLevels + 1];
  size_t work_frame;
};

bool imgb_geom(int32_t win_h, int32_t win_w, int32_t levels, ImgbGeom* g) {
  if (win_h < 1 || win_w < 1 || win_h > kImgbMaxSrc || win_w > kImgbMaxSrc || levels < 1 || levels > kImgbMaxLevels) return false;
  g->levels = levels;
  g->h[0] = win_h, g->w[0] = win_w, g->m_off[0] = 0;
  for (int l = 0; l <= levels; ++l) {
    if (l) g->h[l] = (g->h[l - 1] + 1) / 2, g->w[l] = (g->w[l - 1] + 1) / 2;
    g->m_off[l + 1] = g->m_off[l] + (size_t)g->h[l] * (size_t)g->w[l];
  }
  size_t at = 0;
  g->d_off[0] = g->r_off[0] = g->r_off[levels] = 0;  // D_0 and R_L are never stored
  for (int l = 1; l <= levels; ++l) g->d_off[l] = at, at += ((size_t)g->h[l] * g->w[l] * 3 * sizeof(int16_t) + 15) & ~(size_t)15;
  for (int l = 1; l < levels; ++l) g->r_off[l] = at, at += ((size_t)g->h[l] * g->w[l] * 3 * sizeof(int32_t) + 15) & ~(size_t)15;
  g->work_frame = at;
  return true;
}

// host_models.blend_reduce on one channel
void imgb_reduce_host(const int32_t* a, int h, int w, int32_t* b, int oh, int ow, std::vector<int32_t>& tmp) {
  static const int k[5] = {1, 4, 6, 4, 1};
  tmp.assign((size_t)h * ow, 0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < ow; ++x) {
      int32_t s = 0;
      for (int j = 0; j < 5; ++j) s += k[j] * a[(size_t)y * w + std::min(std::max(2 * x + j - 2, 0), w - 1)];
      tmp[(size_t)y * ow + x] = s;
    }
  for (int y = 0; y < oh; ++y)
    for (int x = 0; x < ow; ++x) {
      int32_t s = 0;
      for (int i = 0; i < 5; ++i) s += k[i] * tmp[(size_t)std::min(std::max(2 * y + i - 2, 0), h - 1) * ow + x];
      b[(size_t)y * ow + x] = (s + 128) >> 8;
    }
}
}  // namespace

extern "C" {

size_t float_img_blend_plan_ints(int32_t win_h, int32_t win_w, int32_t levels) {
  ImgbGeom g;
  return imgb_geom(win_h, win_w, levels, &g) ? g.m_off[levels + 1] : 0;
}

int float_img_blend_plan(int32_t src_h, int32_t src_w, int32_t rect_x, int32_t rect_y, int32_t rect_w, int32_t rect_h, int32_t inset,
                         int32_t levels, int16_t* table, size_t table_ints) {
  const char* fn = "float_img_blend_plan";
  FH_REQUIRE(table, "%s: null argument (table)", fn);
  FH_REQUIRE(src_h >= 1 && src_h <= kImgbMaxSrc && src_w >= 1 && src_w <= kImgbMaxSrc, "%s: source sides src_h, src_w (%d x %d) must be 1 ... %d",
             fn, src_h, src_w, kImgbMaxSrc);
  FH_REQUIRE(rect_w >= 1 && rect_w <= kImgbMaxSrc && rect_h >= 1 && rect_h <= kImgbMaxSrc,
             "%s: box sides rect_h, rect_w (%d x %d) must be 1 ... %d", fn, rect_h, rect_w, kImgbMaxSrc);
  FH_REQUIRE(rect_x >= -kImgbMaxOff && rect_x <= kImgbMaxOff && rect_y >= -kImgbMaxOff && rect_y <= kImgbMaxOff,
             "%s: box origin rect_x, rect_y (%d, %d) must be within +-%d", fn, rect_x, rect_y, kImgbMaxOff);
  FH_REQUIRE(inset >= 0 && inset <= kImgbMaxSrc, "%s: inset (%d) must be 0 ... %d", fn, inset, kImgbMaxSrc);
  FH_REQUIRE(levels >= 1 && levels <= kImgbMaxLevels, "%s: levels (%d) must be 1 ... %d", fn, levels, kImgbMaxLevels);
  const int xa = std::max(0, rect_x), xb = std::min(src_w, rect_x + rect_w), ya = std::max(0, rect_y), yb = std::min(src_h, rect_y + rect_h);
  FH_REQUIRE(xb > xa && yb > ya, "%s: the box rect_x, rect_y, rect_w, rect_h (%d, %d, %d x %d) misses the %d x %d image: there is no window", fn,
             rect_x, rect_y, rect_w, rect_h, src_w, src_h);
  ImgbGeom g;
  imgb_geom(yb - ya, xb - xa, levels, &g);
  FH_REQUIRE(table_ints >= g.m_off[levels + 1], "%s: table_ints %zu < float_img_blend_plan_ints(%d, %d, %d) = %zu", fn, table_ints, yb - ya,
             xb - xa, levels, g.m_off[levels + 1]);
  // M_0: 256 where the distance to the nearest open side of the unclipped box is at least `inset` (open: float_img_paste's rule)
  const bool open_l = rect_x > 0, open_r = rect_x + rect_w < src_w, open_t = rect_y > 0, open_b = rect_y + rect_h < src_h;
  std::vector<int32_t> cur((size_t)g.h[0] * g.w[0]), nxt, tmp;
  for (int y = 0; y < g.h[0]; ++y)
    for (int x = 0; x < g.w[0]; ++x) {
      const int u = xa + x - rect_x, v = ya + y - rect_y;
      int d = 1 << 30;
      if (open_l) d = std::min(d, u);
      if (open_r) d = std::min(d, rect_w - 1 - u);
      if (open_t) d = std::min(d, v);
      if (open_b) d = std::min(d, rect_h - 1 - v);
      cur[(size_t)y * g.w[0] + x] = d >= inset ? 256 : 0;
    }
  for (int l = 0;; ++l) {
    int16_t* t = table + g.m_off[l];
    for (size_t i = 0; i < cur.size(); ++i) t[i] = (int16_t)cur[i];  // 0 ... 256: reduce is a weighted mean
    if (l == levels) break;
    nxt.resize((size_t)g.h[l + 1] * g.w[l + 1]);
    imgb_reduce_host(cur.data(), g.h[l], g.w[l], nxt.data(), g.h[l + 1], g.w[l + 1], tmp);
    cur.swap(nxt);
  }
  return FLOAT_OK;
}

size_t float_img_blend_work_bytes(int32_t n_frames, int32_t win_h, int32_t win_w, int32_t levels) {
  ImgbGeom g;
  if (n_frames < 1 || !imgb_geom(win_h, win_w, levels, &g)) return 0;
  return std::max((size_t)16, (size_t)n_frames * g.work_frame);
}

int float_img_blend(const uint8_t* src8, int32_t src_h, int32_t src_w, const uint8_t* face8, int32_t n_frames, int32_t win_x, int32_t win_y,
                    int32_t win_h, int32_t win_w, int32_t levels, const int16_t* mask, void* work, size_t work_bytes, uint8_t* out,
                    void* stream) {
  const char* fn = "float_img_blend";
  FH_REQUIRE(src8 && face8 && mask && work && out, "%s: null argument (src8, face8, mask, work or out)", fn);
  FH_REQUIRE(src_h >= 1 && src_h <= kImgbMaxSrc && src_w >= 1 && src_w <= kImgbMaxSrc, "%s: source sides src_h, src_w (%d x %d) must be 1 ... %d",
             fn, src_h, src_w, kImgbMaxSrc);
  FH_REQUIRE(n_frames >= 1, "%s: n_frames (%d) must be at least 1", fn, n_frames);
  FH_REQUIRE(levels >= 1 && levels <= kImgbMaxLevels, "%s: levels (%d) must be 1 ... %d", fn, levels, kImgbMaxLevels);
  FH_REQUIRE(win_w >= 1 && win_h >= 1 && win_x >= 0 && win_y >= 0 && win_x <= src_w - win_w && win_y <= src_h - win_h,
             "%s: the window win_x, win_y, win_h, win_w (%d, %d, %d x %d) must lie inside the %d x %d image", fn, win_x, win_y, win_h, win_w,
             src_h, src_w);
  ImgbGeom g;
  imgb_geom(win_h, win_w, levels, &g);  // the window lies inside the image: its sides are in range
  FH_REQUIRE(((uintptr_t)mask & 1u) == 0, "%s: mask must be 2-byte aligned", fn);
  FH_REQUIRE(((uintptr_t)work & 15u) == 0, "%s: work must be 16-byte aligned", fn);
  const size_t need = std::max((size_t)16, (size_t)n_frames * g.work_frame);
  FH_REQUIRE(work_bytes >= need, "%s: work_bytes %zu < float_img_blend_work_bytes(%d, %d, %d, %d) = %zu", fn, work_bytes, n_frames, win_h, win_w,
             levels, need);

  const size_t face_frame = (size_t)win_h * win_w * 3, out_frame = (size_t)src_h * src_w * 3;
  const bool fast = src_w % 4 == 0 && ((uintptr_t)out & 3u) == 0;
  const bool odd = (win_x & 1) != 0;
  hipStream_t s = (hipStream_t)stream;
  for (int32_t f0 = 0; f0 < n_frames; f0 += (int32_t)kImgbMaxGridZ) {  // frames are the grid's z; every frame has its own part of `work`
    const unsigned nf = (unsigned)std::min<int32_t>((int32_t)kImgbMaxGridZ, n_frames - f0);
    const uint8_t* fc = face8 + (size_t)f0 * face_frame;
    uint8_t* wk = (uint8_t*)work + (size_t)f0 * g.work_frame;
    uint8_t* o = out + (size_t)f0 * out_frame;
    for (int l = 0; l < levels; ++l) {  // down: D_{l+1} from D_l
      ImgbDown p{};
      p.in_h = g.h[l], p.in_w = g.w[l], p.out_h = g.h[l + 1], p.out_w = g.w[l + 1];
      p.src_w = src_w, p.win_x = win_x, p.win_y = win_y;
      p.face_frame = face_frame, p.work_frame = g.work_frame, p.in_off = g.d_off[l], p.out_off = g.d_off[l + 1];
      const dim3 grid((unsigned)(p.out_w + kImgbDownW - 1) / kImgbDownW, (unsigned)(p.out_h + kImgbDownH - 1) / kImgbDownH, nf);
      if (l == 0)
        hipLaunchKernelGGL(imgb_down_kernel<true>, grid, dim3(kImgbThreads), 0, s, src8, fc, wk, p);
      else
        hipLaunchKernelGGL(imgb_down_kernel<false>, grid, dim3(kImgbThreads), 0, s, src8, fc, wk, p);
    }
    for (int l = levels - 1; l >= 0; --l) {  // up: R_l from D_l, D_{l+1}, R_{l+1} (formed on the fly at the top) and M_l
      ImgbUp p{};
      p.dom_h = l ? g.h[l] : src_h, p.dom_w = l ? g.w[l] : src_w, p.win_x = l ? 0 : win_x, p.win_y = l ? 0 : win_y;
      p.h = g.h[l], p.w = g.w[l], p.ch = g.h[l + 1], p.cw = g.w[l + 1];
      p.face_frame = face_frame, p.work_frame = g.work_frame, p.out_frame = out_frame;
      p.d_off = g.d_off[l], p.dc_off = g.d_off[l + 1], p.rc_off = g.r_off[l + 1], p.r_off = g.r_off[l];
      const int16_t* ml = mask + g.m_off[l];
      const int16_t* mc = mask + g.m_off[l + 1];
      const bool top = l == levels - 1;
      const dim3 grid((unsigned)(p.dom_w + kImgbUpW - 1) / kImgbUpW, (unsigned)(p.dom_h + kImgbUpH - 1) / kImgbUpH, nf);
      void (*kern)(const unsigned char*, const unsigned char*, const short*, const short*, unsigned char*, unsigned char*, ImgbUp);
      if (l)  // a level's own coordinates: the window starts at 0
        kern = top ? imgb_up_kernel<false, true, false, false> : imgb_up_kernel<false, false, false, false>;
      else if (top)
        kern = fast ? (odd ? imgb_up_kernel<true, true, true, true> : imgb_up_kernel<true, true, true, false>)
                    : (odd ? imgb_up_kernel<true, true, false, true> : imgb_up_kernel<true, true, false, false>);
      else
        kern = fast ? (odd ? imgb_up_kernel<true, false, true, true> : imgb_up_kernel<true, false, true, false>)
                    : (odd ? imgb_up_kernel<true, false, false, true> : imgb_up_kernel<true, false, false, false>);
      hipLaunchKernelGGL(kern, grid, dim3(kImgbThreads), 0, s, src8, fc, ml, mc, wk, o, p);
    }
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
