// float_img_resample_plan / float_img_resample_plan_ints (host only), float_img_resample / float_img_resample_work_bytes: bicubic and
// Lanczos resampling of 8-bit RGB frames on the device by Pillow's fixed-point rule (include/float_hip.h).
#include <math.h>

#include "imgr_kernels.hpp"

// The tables are held to host_models.resample_coeffs integer for integer, and that to Pillow: every product and sum below is one
// IEEE double operation in the order written, never a fused multiply-add.
#pragma clang fp contract(off)

namespace {
constexpr int32_t kImgrMaxBox = 1 << 30;  // sides of the (virtual) result a window is cut from
constexpr unsigned kImgrMaxGridZ = 65535;

double imgr_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

double imgr_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

double imgr_lanczos(double x) {
  if (-3.0 <= x && x < 3.0) return imgr_sinc(x) * imgr_sinc(x / 3);
  return 0.0;
}

// one axis n_in -> n_out under a filter; false for what the operator does not take (an unknown filter, a size outside 1 ... 2^30,
// more than 255 taps)
struct ImgrAxis {
  int n_in, n_out, filter, ksize;
  double scale, support, ss;
};

bool imgr_axis(int32_t n_in, int32_t n_out, int32_t filter, ImgrAxis* a) {
  if (n_in < 1 || n_out < 1 || n_in > kImgrMaxBox || n_out > kImgrMaxBox) return false;
  if (filter != FLOAT_IMG_FILTER_BICUBIC && filter != FLOAT_IMG_FILTER_LANCZOS) return false;
  a->n_in = n_in, a->n_out = n_out, a->filter = filter;
  a->scale = (double)n_in / (double)n_out;
  const double fs = a->scale < 1.0 ? 1.0 : a->scale;
  a->support = (filter == FLOAT_IMG_FILTER_BICUBIC ? 2.0 : 3.0) * fs;
  const double c = ceil(a->support);
  if (c * 2 + 1 > (double)kImgrMaxKsize) return false;
  a->ksize = (int)c * 2 + 1;
  a->ss = 1.0 / fs;
  return true;
}

// the taps of output index xx: input samples [*xmin, *xmax); returns the centre
double imgr_bounds(const ImgrAxis& a, int xx, int* xmin, int* xmax) {
  const double center = (xx + 0.5) * a.scale;
  int lo = (int)(center - a.support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + a.support + 0.5);
  if (hi > a.n_in) hi = a.n_in;
  *xmin = lo, *xmax = hi;
  return center;
}

struct ImgrCall {
  ImgrAxis x, y;
  bool do_x, do_y;   // the axis changes size: its pass runs
  int row0, row1;    // the input rows the window's rows reference (do_y), else the window's own rows
  int cells_x;       // ceil(win_w / 4)
  size_t mid_pitch;  // bytes of a row of the intermediate: whole cells
  size_t need;       // bytes of `work`
};

// geometry of a call from its (unchecked) sizes; nullptr on success, else what is wrong
const char* imgr_call(int32_t n_frames, int32_t fr_h, int32_t fr_w, int32_t box_h, int32_t box_w, int32_t filter, int32_t win_x, int32_t win_y,
                      int32_t win_w, int32_t win_h, ImgrCall* c) {
  if (n_frames < 1) return "n_frames must be at least 1";
  if (fr_h < 1 || fr_w < 1 || fr_h > kImgrMaxSide || fr_w > kImgrMaxSide) return "frame sides fr_h, fr_w must be 1 ... 16384";
  if (filter != FLOAT_IMG_FILTER_BICUBIC && filter != FLOAT_IMG_FILTER_LANCZOS) return "filter must be FLOAT_IMG_FILTER_BICUBIC or FLOAT_IMG_FILTER_LANCZOS";
  if (box_h < 1 || box_w < 1 || box_h > kImgrMaxBox || box_w > kImgrMaxBox) return "box sides box_h, box_w must be 1 ... 2^30";
  if (win_w < 1 || win_h < 1 || win_w > kImgrMaxSide || win_h > kImgrMaxSide) return "window sides win_w, win_h must be 1 ... 16384";
  if (win_x < 0 || win_y < 0 || win_x > box_w - win_w || win_y > box_h - win_h) return "the window win_x, win_y, win_w, win_h must lie inside the box";
  if (!imgr_axis(fr_w, box_w, filter, &c->x) || !imgr_axis(fr_h, box_h, filter, &c->y))
    return "fr_w -> box_w or fr_h -> box_h needs more than 255 taps per sample (shrinking by more than about 42 x)";
  c->do_x = fr_w != box_w, c->do_y = fr_h != box_h;
  c->row0 = win_y, c->row1 = win_y + win_h;
  if (c->do_y) {  // xmin and xmax do not decrease with the output index
    int lo, hi;
    imgr_bounds(c->y, win_y, &c->row0, &hi);
    imgr_bounds(c->y, win_y + win_h - 1, &lo, &c->row1);
  }
  c->cells_x = (win_w + kImgrCellW - 1) / kImgrCellW;
  c->mid_pitch = (size_t)c->cells_x * kImgrCellW * 3;
  const size_t mid = (c->do_x && c->do_y) ? (size_t)n_frames * (size_t)(c->row1 - c->row0) * c->mid_pitch : 0;
  c->need = std::max((size_t)16, (mid + 15) & ~(size_t)15);
  return nullptr;
}

bool imgr_aligned(const void* p, size_t pitch, size_t frame) { return (((uintptr_t)p | pitch | frame) & 3u) == 0; }
}  // namespace

extern "C" {

size_t float_img_resample_plan_ints(int32_t n_in, int32_t n_out, int32_t filter, int32_t count) {
  ImgrAxis a;
  if (!imgr_axis(n_in, n_out, filter, &a) || count < 1 || count > n_out) return 0;
  return (size_t)count * (size_t)(2 + a.ksize);
}

int float_img_resample_plan(int32_t n_in, int32_t n_out, int32_t filter, int32_t first, int32_t count, int32_t* table, size_t table_ints) {
  const char* fn = "float_img_resample_plan";
  FH_REQUIRE(table, "%s: null argument (table)", fn);
  FH_REQUIRE(filter == FLOAT_IMG_FILTER_BICUBIC || filter == FLOAT_IMG_FILTER_LANCZOS,
             "%s: filter (%d) must be FLOAT_IMG_FILTER_BICUBIC (0) or FLOAT_IMG_FILTER_LANCZOS (1)", fn, filter);
  FH_REQUIRE(n_in >= 1 && n_in <= kImgrMaxBox && n_out >= 1 && n_out <= kImgrMaxBox, "%s: sizes n_in, n_out (%d -> %d) must be 1 ... 2^30", fn,
             n_in, n_out);
  ImgrAxis a;
  FH_REQUIRE(imgr_axis(n_in, n_out, filter, &a), "%s: n_in -> n_out (%d -> %d) needs more than %d taps per sample (ksize)", fn, n_in, n_out,
             kImgrMaxKsize);
  FH_REQUIRE(first >= 0 && count >= 1 && first <= n_out - count, "%s: indices first, count (%d, %d) must lie in 0 ... n_out (%d)", fn, first,
             count, n_out);
  const size_t stride = (size_t)(2 + a.ksize);
  FH_REQUIRE(table_ints >= (size_t)count * stride, "%s: table_ints %zu < float_img_resample_plan_ints(%d, %d, %d, %d) = %zu", fn, table_ints,
             n_in, n_out, filter, count, (size_t)count * stride);
  double w[kImgrMaxKsize];
  for (int i = 0; i < count; ++i) {
    int32_t* t = table + (size_t)i * stride;
    int xmin, xmax;
    const double center = imgr_bounds(a, first + i, &xmin, &xmax);
    const int n = xmax - xmin;  // <= ksize: the two roundings lie at most 2 support + 1 apart
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      const double v = (x + xmin - center + 0.5) * a.ss;
      w[x] = filter == FLOAT_IMG_FILTER_BICUBIC ? imgr_bicubic(v) : imgr_lanczos(v);
      ww += w[x];
    }
    long long l1 = 0;
    for (int x = 0; x < a.ksize; ++x) {
      int k = 0;
      if (x < n) {
        const double v = ww != 0.0 ? w[x] / ww : w[x];
        k = v < 0 ? (int)(-0.5 + v * (double)(1 << kImgrBits)) : (int)(0.5 + v * (double)(1 << kImgrBits));
      }
      t[2 + x] = k;
      l1 += k < 0 ? -(long long)k : k;
    }
    t[0] = xmin, t[1] = n;
    FH_REQUIRE(255 * l1 + (1 << (kImgrBits - 1)) < (1ll << 31), "%s: the coefficients of index %d do not fit 32-bit sums (n_in %d, n_out %d)", fn,
               first + i, n_in, n_out);
  }
  return FLOAT_OK;
}

size_t float_img_resample_work_bytes(int32_t n_frames, int32_t fr_h, int32_t fr_w, int32_t box_h, int32_t box_w, int32_t filter, int32_t win_x,
                                     int32_t win_y, int32_t win_w, int32_t win_h) {
  ImgrCall c;
  return imgr_call(n_frames, fr_h, fr_w, box_h, box_w, filter, win_x, win_y, win_w, win_h, &c) ? 0 : c.need;
}

int float_img_resample(const uint8_t* frames8, int32_t n_frames, int32_t fr_h, int32_t fr_w, int32_t box_h, int32_t box_w, int32_t filter,
                       int32_t win_x, int32_t win_y, int32_t win_w, int32_t win_h, const int32_t* tab_x, const int32_t* tab_y, void* work,
                       size_t work_bytes, uint8_t* out, void* stream) {
  const char* fn = "float_img_resample";
  FH_REQUIRE(frames8 && out && work, "%s: null argument (frames8, out or work)", fn);
  ImgrCall c;
  const char* bad = imgr_call(n_frames, fr_h, fr_w, box_h, box_w, filter, win_x, win_y, win_w, win_h, &c);
  FH_REQUIRE(!bad, "%s: %s (n_frames %d, frames %d x %d, box %d x %d, filter %d, window %d, %d, %d x %d)", fn, bad, n_frames, fr_h, fr_w, box_h,
             box_w, filter, win_x, win_y, win_h, win_w);
  FH_REQUIRE((!c.do_x || tab_x) && (!c.do_y || tab_y), "%s: null argument (tab_x or tab_y of an axis that changes its size)", fn);
  FH_REQUIRE((((uintptr_t)tab_x | (uintptr_t)tab_y) & 3u) == 0, "%s: tab_x and tab_y must be 4-byte aligned", fn);
  FH_REQUIRE(((uintptr_t)work & 15u) == 0, "%s: work must be 16-byte aligned", fn);
  FH_REQUIRE(work_bytes >= c.need, "%s: work_bytes %zu < float_img_resample_work_bytes(...) = %zu", fn, work_bytes, c.need);

  const size_t fr_pitch = (size_t)fr_w * 3, fr_frame = (size_t)fr_h * fr_pitch;
  const size_t out_pitch = (size_t)win_w * 3, out_frame = (size_t)win_h * out_pitch;
  const bool out_fast = win_w % kImgrCellW == 0 && imgr_aligned(out, out_pitch, out_frame);
  const int mid_rows = c.row1 - c.row0;
  const size_t mid_frame = (size_t)mid_rows * c.mid_pitch;
  uint8_t* mid = (uint8_t*)work;

  ImgrPass h{}, v{};
  h.width = v.width = win_w, h.cells_x = v.cells_x = c.cells_x;
  // horizontal: rows row0 ... row1 - 1 of the frames -> the intermediate, or (the vertical axis keeps its size) straight to out
  h.in_frame = (long long)fr_frame, h.in_off = (unsigned)((size_t)c.row0 * fr_pitch), h.in_pitch = (unsigned)fr_pitch, h.ksize = c.x.ksize;
  h.out_pitch = (unsigned)(c.do_y ? c.mid_pitch : out_pitch), h.out_frame = (long long)(c.do_y ? mid_frame : out_frame);
  // vertical: the intermediate, or (the horizontal axis keeps its size) the window's columns of the frames -> out
  v.ksize = c.y.ksize, v.out_pitch = (unsigned)out_pitch, v.out_frame = (long long)out_frame;
  if (c.do_x) {
    v.in_frame = (long long)mid_frame, v.in_off = 0, v.in_pitch = (unsigned)c.mid_pitch, v.in_first = c.row0, v.in_cols = c.cells_x * kImgrCellW;
  } else {  // rows are the frames' own; without a table (neither axis changes) row y of the window is row win_y + y
    v.in_frame = (long long)fr_frame, v.in_pitch = (unsigned)fr_pitch, v.in_first = 0, v.in_cols = win_w;
    v.in_off = (unsigned)((c.do_y ? 0 : (size_t)win_y * fr_pitch) + (size_t)win_x * 3);
  }

  hipStream_t s = (hipStream_t)stream;
  const unsigned gx = (unsigned)(c.cells_x + kImgrThreads - 1) / kImgrThreads;
  for (int32_t f0 = 0; f0 < n_frames; f0 += (int32_t)kImgrMaxGridZ) {  // frames are the grid's z: groups of 65535 share `work` in stream order
    const unsigned nf = (unsigned)std::min<int32_t>((int32_t)kImgrMaxGridZ, n_frames - f0);
    const uint8_t* fr = frames8 + (size_t)f0 * fr_frame;
    uint8_t* o = out + (size_t)f0 * out_frame;
    if (c.do_x) {
      const dim3 grid(gx, (unsigned)mid_rows, nf);
      if (c.do_y)
        hipLaunchKernelGGL(imgr_horizontal_kernel<true>, grid, dim3(kImgrThreads), 0, s, fr, tab_x, mid, h);
      else if (out_fast)
        hipLaunchKernelGGL(imgr_horizontal_kernel<true>, grid, dim3(kImgrThreads), 0, s, fr, tab_x, o, h);
      else
        hipLaunchKernelGGL(imgr_horizontal_kernel<false>, grid, dim3(kImgrThreads), 0, s, fr, tab_x, o, h);
    }
    if (c.do_y || !c.do_x) {
      const dim3 grid(gx, (unsigned)win_h, nf);
      const uint8_t* in = c.do_x ? (const uint8_t*)mid : fr;
      const int32_t* tab = c.do_y ? tab_y : nullptr;
      if (out_fast)
        hipLaunchKernelGGL(imgr_vertical_kernel<true>, grid, dim3(kImgrThreads), 0, s, in, tab, o, v);
      else
        hipLaunchKernelGGL(imgr_vertical_kernel<false>, grid, dim3(kImgrThreads), 0, s, in, tab, o, v);
    }
  }
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

}  // extern "C"
