// From a descriptor to a launch: the decoder's launchers (3x3 conv, up-conv + blur, flow / warp / ToRGB, style + demod) and the
// scheduler of the ride-along device-to-host copy.  Included by dec_api.hip only, after dec_kernels.hpp (the one translation
// unit that holds the kernels' instantiations).
#pragma once
#include "dec_pack.hpp"
#include "tuning.hpp"

namespace {

// FlowArgs::final_mode: what the last level's flow kernel writes beside (or instead of) the pyramids
enum DecOut : int { kOutNone = 0, kOutHWC = 1, kOutRawCHW = 2, kOutU8 = 3, kOutI420 = 4 };
// bytes of one size x size frame as the frames calls hand it over
inline size_t out_frame_bytes(DecOut mode, int size) {
  const size_t npix = (size_t)size * size;
  return mode == kOutI420 ? npix + npix / 2 : npix * 3 * (mode == kOutU8 ? sizeof(uint8_t) : sizeof(float));
}

// The launches of a high batch that may carry a share of the pending copy, per level
enum RideKind : int { kRideUpconv = 0, kRideConv2 = 1, kRideFlow = 2, kRideKinds = 3 };

// float_dec_frames_host, ride-along mode: the frames of the previous high batch still to be copied to the host by copy
// workgroups inside the next batch's launches (CopyTail, dec_kernels.hpp).  Per call: reset, then per high batch open_batch ->
// the launchers' take -> hand_over, and flush behind the last batch.
struct RideCopy {
  const char* src = nullptr;  // bytes: the frames are fp32, uint8 or I420 (float_dec_frames_host / _host_u8 / _host_i420)
  char* dst = nullptr;        // device-side address of the pinned destination (what the copy workgroups store through)
  char* dst_host = nullptr;   // the same position as the caller's host pointer (hipMemcpyAsync of what no launch took)
  size_t left16 = 0;   // 16-byte units not yet handed to a launch
  double wleft = 0.0;  // sum of the weights of the carrying launches still to come in this batch

  // Weight of a carrying launch at resolution R: the share of the pending copy it takes is proportional to it, so that every
  // share ends inside its launch (per 32-frame batch, ~us; other resolutions: equal shares).
  static double weight(const DecTune& tn, int R, int kind) {
    const int li = R == 64 ? 0 : R == 128 ? 1 : R == 256 ? 2 : R == 512 ? 3 : -1;
    return li < 0 ? 250.0 : tn.ride_w[li][kind];
  }
  void reset() { left16 = 0, wleft = 0.0; }
  // The batch about to run carries what is pending: every RideKind launch of levels[first..] from ride_min_res up takes a share.
  void open_batch(const DecTune& tn, const std::vector<Level>& levels, int first) {
    double wsum = 0.0;
    for (size_t li = first; li < levels.size(); ++li)
      if (levels[li].R >= tn.ride_min_res)
        for (int kind = 0; kind < kRideKinds; ++kind) wsum += weight(tn, levels[li].R, kind);
    wleft = left16 ? wsum : 0.0;
  }
  // The share of the pending copy that the next carrying launch takes.
  CopyTail take(const DecTune& tn, int R, RideKind kind) {
    CopyTail ct{};
    if (!left16 || wleft <= 0.0 || !tn.ride_wgs || R < tn.ride_min_res) return ct;
    const double w = weight(tn, R, kind);
    size_t n = (size_t)((double)left16 * std::min(1.0, w / wleft)) + 1;
    n = std::min(n, left16);
    wleft -= w;
    if (wleft < 1e-9) n = left16;  // the batch's last carrier takes what is left
    ct.src = reinterpret_cast<const u32x4*>(src);
    ct.dst = reinterpret_cast<u32x4*>(dst);
    ct.n16 = n;
    ct.nwg = tn.ride_wgs, ct.pace = tn.ride_pace;
    src += n * 16, dst += n * 16, dst_host += n * 16;
    left16 -= n;
    return ct;
  }
  // What no launch took (a decoder without carrying levels, the call's last batch): plain copy, in order.
  int flush(hipStream_t st) {
    if (left16) FH_CHECK_HIP(hipMemcpyAsync(dst_host, src, left16 * 16, hipMemcpyDeviceToHost, st));
    left16 = 0;
    return FLOAT_OK;
  }
  // A finished batch: its `bytes` at `from` cross PCIe under the next batch's kernels.
  int hand_over(const char* from, char* to_dev, char* to_host, size_t bytes, hipStream_t st) {
    int rc = flush(st);
    src = from, dst = to_dev, dst_host = to_host, left16 = bytes / 16;
    return rc;
  }
};

// What every launcher is given: the handle's switches, the pending copy its launches may carry a share of (nullptr: none, the
// unit operators) and the stream.
struct DecLaunch {
  const DecTune& tn;
  RideCopy* ride;
  hipStream_t st;
  CopyTail take(int R, RideKind kind) const { return ride ? ride->take(tn, R, kind) : CopyTail{}; }
  // dynamic LDS of a level-kernel launch: what it needs, or the occupancy cap (DecTune::lds_pad) where that is more
  size_t smem(size_t need) const { return std::max(need, (size_t)tn.lds_pad); }
};

struct Rows { const float* p = nullptr; int ld = 0; };  // a float table with one row per frame

// Every instantiation of the two level kernels with more than one choice to make: f(kernel, <what selects it>).
// raise_lds_limits and the launchers both walk these lists, so an instantiation is added by one line here.
template <class T, class F>
void for_each_conv16(F&& f) {  // f(kernel, output channels per workgroup, ToFlow in the epilogue)
  f(dec_conv16_kernel<T, 4, 3, 3>, 64, false);
  f(dec_conv16_kernel<T, 2, 3, 3>, 32, false);
  f(dec_conv16_kernel<T, 4, 3, 3, 1>, 64, true);
  f(dec_conv16_kernel<T, 2, 3, 3, 1>, 32, true);
}
template <class T, class F>
void for_each_flowlast(F&& f) {  // f(kernel, the final_mode it is for: kOutNone = every mode but the listed ones); raise_lds_limits walks it
  f(dec_flowlast_kernel<T>, kOutNone);
  f(dec_flowlast_kernel<T, true>, kOutU8);
  f(dec_flowlast_kernel<T, false, true>, kOutI420);
}
template <class T, class F>
void for_each_flow(F&& f) {  // f(kernel, pixels per lane group and iteration, last level)
  f(dec_flow_kernel<T, 4, false>, 4, false);
  f(dec_flow_kernel<T, 2, false>, 2, false);
  f(dec_flow_kernel<T, 1, false>, 1, false);
  f(dec_flow_kernel<T, 4, true>, 4, true);
  f(dec_flow_kernel<T, 2, true>, 2, true);
  f(dec_flow_kernel<T, 1, true>, 1, true);
}

// dynamic LDS above the 64 KiB default: 64 KiB per workgroup with 16-bit operands (2 workgroups per CU), twice that in the
// fp32 verification mode (the z tile of dec_zblur_kernel: 32 x 32 x 128 B)
template <class T>
int raise_lds_limits(const DecTune& tn) {
  const int lim = std::max(32 * 1024 * T::EB, tn.lds_pad);
  auto raise = [](auto kern, int bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  };
  for_each_conv16<T>([&](auto kern, int, bool) { raise(kern, lim); });
  for_each_flowlast<T>([&](auto kern, DecOut) { raise(kern, lim); });
  raise(dec_conv_kernel<T, 4>, lim);
  raise(dec_conv_kernel<T, 2>, lim);
  raise(dec_zconv4_kernel<T>, lim);
  raise(dec_zblur_kernel<T>, lim);
  for_each_flow<T>([&](auto kern, int, bool) { raise(kern, lim); });
  (void)hipGetLastError();
  return FLOAT_OK;
}

// Tile edge of the 3x3 conv kernels for an Ho x Wo output, and THE decision about the output channels per workgroup of layer
// `s` at that tile: 64 (NT = 4) in the 16x16-tile kernel where the layer has them, 32 in the generic low-resolution kernel
// (DecTune::conv_bn, conv_bn_lo: the measurements are there).
inline int conv_tile(int Ho, int Wo) {
  const int big = std::max(Ho, Wo);
  return big > 8 ? 16 : (big > 4 ? 8 : 4);
}
inline int conv_bn(const DecTune& tn, const Styled& s, int tdim) {
  return (s.cout >= 64 && (tdim == 16 ? tn.conv_bn : tn.conv_bn_lo) == 64) ? 64 : 32;
}
// ToFlow's conv can ride in the epilogue of layer `s` at R x R (dec_conv16_kernel FLOWM): 16x16 tiles, and the layer's whole
// channel range in one workgroup
inline bool conv_takes_flow_epi(const DecTune& tn, const Styled& s, int R) {
  return R >= 16 && R % 16 == 0 && s.cout == conv_bn(tn, s, conv_tile(R, R));
}

// Geometry of one launch of the 3x3 family: the input extent, the outputs it computes, where they land in the stored tensor
// (output (y, x) at (sy * y + py, sx * x + px) of OH x OW) and the taps - input offsets, and the index of the first one in
// the layer's packed weights.
struct ConvGeom {
  int Hi, Wi, Ho, Wo, OH, OW, sy, sx, py, px;
  int ntaps, tap0;
  int dy[9], dx[9];
  bool act;  // + FusedLeakyReLU bias, leaky_relu * sqrt2 (the parity classes' partial results take neither)

  // plain 3x3 conv, R x R -> R x R
  static ConvGeom same3x3(int R) {
    ConvGeom c = {};
    c.Hi = c.Wi = c.Ho = c.Wo = c.OH = c.OW = R;
    c.sy = c.sx = 1;
    c.ntaps = 9;
    for (int t = 0; t < 9; ++t) c.dy[t] = t / 3 - 1, c.dx[t] = t % 3 - 1;  // row by row, the order pack_styled packs them in
    c.act = true;
    return c;
  }
  // parity class (pu, pv) of the stride-2 transposed 3x3 conv, Ri x Ri -> its outputs inside (2 Ri + 1) x (2 Ri + 1)
  static ConvGeom up_class(int Ri, int pu, int pv) {
    const int first[4] = {0, 4, 6, 8};  // the classes are packed (0,0), (0,1), (1,0), (1,1) with 4 + 2 + 2 + 1 taps (pack_styled)
    const ClassTaps t = class_taps(pu, pv);
    ConvGeom c = {};
    c.Hi = c.Wi = Ri;
    c.Ho = Ri + 1 - pu, c.Wo = Ri + 1 - pv;
    c.OH = c.OW = 2 * Ri + 1;
    c.sy = c.sx = 2;
    c.py = pu, c.px = pv;
    c.ntaps = t.n, c.tap0 = first[2 * pu + pv];
    for (int i = 0; i < t.n; ++i) c.dy[i] = t.dy[i], c.dx[i] = t.dx[i];
    return c;
  }
};

// What the conv launchers share: the layer, its operands and the frame count
inline ConvArgs conv_args_of(const Styled& s, const void* X, void* Y, int F, int Hi, int Wi, int OH, int OW, Rows demod, unsigned long long* sat) {
  ConvArgs g;
  memset(&g, 0, sizeof(g));
  g.X = X, g.Y = Y;
  g.Wt = s.W;
  g.demod = demod.p, g.ldd = demod.ld;
  g.sat = sat, g.F = F;
  g.Hi = Hi, g.Wi = Wi;
  g.Cin = s.cin, g.Cout = s.cout;
  g.OH = OH, g.OW = OW;
  return g;
}

// One launch of the 3x3 family for F frames: Y = act(demod * conv(X, taps of s) + bias) * snext.  wfrag / oflow: ToFlow's conv
// in the epilogue instead of the store of Y (run_level).  Carries a share of the pending copy (16x16-tile kernel only).
template <class T>
int launch_conv(const DecLaunch& cx, const ConvGeom& c, const Styled& s, const void* X, void* Y, int F, Rows demod, Rows snext,
                unsigned long long* sat, const void* wfrag = nullptr, float* oflow = nullptr) {
  typedef typename T::elem E;
  constexpr size_t RB = 32 * T::EB;
  const DecTune& tn = cx.tn;
  ConvArgs g = conv_args_of(s, X, Y, F, c.Hi, c.Wi, c.OH, c.OW, demod, sat);
  g.Wt = reinterpret_cast<const E*>(s.W) + (size_t)c.tap0 * s.cout * s.cin;
  g.wfrag = wfrag, g.oflow = oflow;
  g.bias = c.act ? s.abias : nullptr, g.act = c.act ? 1 : 0;
  g.snext = snext.p, g.lds = snext.ld;
  g.Ho = c.Ho, g.Wo = c.Wo;
  g.sy = c.sy, g.sx = c.sx, g.py = c.py, g.px = c.px;
  g.ntaps = c.ntaps;
  for (int t = 0; t < c.ntaps; ++t) g.dy[t] = (signed char)c.dy[t], g.dx[t] = (signed char)c.dx[t];
  const int dymin = *std::min_element(c.dy, c.dy + c.ntaps), dymax = *std::max_element(c.dy, c.dy + c.ntaps);
  const int dxmin = *std::min_element(c.dx, c.dx + c.ntaps), dxmax = *std::max_element(c.dx, c.dx + c.ntaps);
  const int tdim = conv_tile(c.Ho, c.Wo);
  g.lth = g.ltw = ilog2(tdim);
  g.lnf = 8 - 2 * g.lth;  // th * tw * nf == 256
  g.dymin = dymin, g.dxmin = dxmin;
  g.hh = tdim + dymax - dymin, g.hw = tdim + dxmax - dxmin;
  g.tiles_x = (c.Wo + tdim - 1) / tdim, g.tiles_y = (c.Ho + tdim - 1) / tdim;
  const int nf = 1 << g.lnf;
  const int fblocks = (F + nf - 1) / nf;
  const int npix = nf * g.hh * g.hw;
  FH_REQUIRE(npix * 4 <= 9 * 256, "conv halo tile too large (%d pixels)", npix);
  const int bn = conv_bn(tn, s, tdim);
  FH_REQUIRE(s.cout % bn == 0 && s.cin % 32 == 0, "conv channels (%d -> %d) not tileable", s.cin, s.cout);
  const int ty_taps = dymax - dymin + 1, tx_taps = dxmax - dxmin + 1;
  void (*kern)(ConvArgs) = nullptr;  // the kernel, its grid and dynamic LDS: by tile size
  dim3 grid;
  size_t smem;
  if (tdim == 16 && ty_taps == 3 && tx_taps == 3 && c.ntaps == 9 && c.Ho % 16 == 0 && c.Wo % 16 == 0 && c.Ho == c.Hi && c.Wo == c.Wi) {
    // dense 3 x 3 window on 16x16 tiles: compile-time geometry, swizzled LDS, register prefetch
    const int total = g.tiles_x * g.tiles_y * F;
    g.tpw = tn.tpw ? tn.tpw : (total >= 16384 ? 4 : (total >= 4096 ? 2 : 1));
    smem = (size_t)(15 + ty_taps) * (15 + tx_taps) * RB + (size_t)c.ntaps * bn * RB + 3 * bn * sizeof(float);  // halo, weights, epilogue operands
    g.ct = cx.take(c.Ho, kRideConv2);
    grid = dim3((total + g.tpw - 1) / g.tpw + g.ct.nwg, s.cout / bn);
    if (tn.cb_order && s.cout / bn > 1) {  // channel blocks of a tile group side by side on one XCD (dec_group_cb)
      g.ngroups = (unsigned)((total + g.tpw - 1) / g.tpw);
      g.ncb = (unsigned)(s.cout / bn);
      grid = dim3(g.ngroups * g.ncb + g.ct.nwg, 1);
    }
    FH_REQUIRE(!oflow || s.cout == bn, "ToFlow epilogue needs the layer's %d output channels in one block of %d", s.cout, bn);
    for_each_conv16<T>([&](auto k, int kbn, bool kflow) {
      if (kbn == bn && kflow == (oflow != nullptr)) kern = k;
    });
    smem = cx.smem(smem);
  } else {
    FH_REQUIRE(!oflow, "ToFlow epilogue: only on the 16x16-tile 3x3 kernel (%d x %d)", c.Ho, c.Wo);
    smem = (size_t)npix * RB + (size_t)c.ntaps * bn * RB;
    grid = dim3(g.tiles_x * g.tiles_y * fblocks, s.cout / bn);
    kern = bn == 64 ? dec_conv_kernel<T, 4> : dec_conv_kernel<T, 2>;
  }
  FH_REQUIRE(kern, "no 3x3 conv kernel with %d channels per workgroup", bn);
  fh_launch_prof(1, kern, grid, dim3(256), smem, cx.st, g);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// The up-sampling StyledConv (styledecoder.py:302-325 with upsample=True: conv_transpose2d stride 2 -> Blur -> + bias ->
// leaky_relu * sqrt2) for `n` frames: x_in (Ri x Ri, already scaled by the layer's style) -> *U_out (2Ri x 2Ri, scaled by
// `snext`, the consumer's style).  Three forms by size: transposed conv + blur in one launch from `zblur_min` px up (the
// result lands in Zb: x_in may alias U), all four parity classes in one launch + blur kernel from 16 px up, class by class
// through the generic kernel below.  The fused launch may carry a share of the pending device-to-host copy.
template <class T>
int launch_upconv(const DecLaunch& cx, const Styled& up, int Ri, int n, const void* x_in, void* Zb, void* U, void** U_out, Rows demod,
                  Rows snext, unsigned long long* sat) {
  typedef typename T::elem E;
  constexpr size_t RB = 32 * T::EB;
  const DecTune& tn = cx.tn;
  const int R = 2 * Ri;
  int rc;
  if (R >= tn.zblur_min && up.cout % 32 == 0 && up.cin % 32 == 0) {
    ConvArgs z = conv_args_of(up, x_in, Zb, n, Ri, Ri, R, R, demod, sat);
    z.bias = up.abias;
    z.snext = snext.p, z.lds = snext.ld;
    for (int b = 0; b < 4; ++b) z.fir[b] = up.fir[b];
    z.fir_sym = (up.fir[0] == 0.25f && up.fir[1] == 0.75f && up.fir[2] == 0.75f && up.fir[3] == 0.25f) ? 1 : 0;
    z.tiles_x = z.tiles_y = (R + 27) / 28;
    z.ct = cx.take(R, kRideUpconv);
    dim3 grid(z.tiles_x * z.tiles_y * n + z.ct.nwg, up.cout / 32);
    if (tn.cb_order && up.cout / 32 > 1) {
      z.ngroups = (unsigned)(z.tiles_x * z.tiles_y * n);
      z.ncb = (unsigned)(up.cout / 32);
      grid = dim3(z.ngroups * z.ncb + z.ct.nwg, 1);
    }
    fh_launch_prof(1, dec_zblur_kernel<T>, grid, dim3(256), cx.smem(32 * 32 * RB), cx.st, z);
    *U_out = Zb;
    FH_CHECK_HIP(hipGetLastError());
    return FLOAT_OK;
  }
  if (Ri + 1 > 8 && up.cout % 32 == 0 && !tn.no_zfuse) {
    ConvArgs z = conv_args_of(up, x_in, Zb, n, Ri, Ri, R + 1, R + 1, demod, sat);
    z.tiles_x = z.tiles_y = (Ri + 1 + 15) / 16;
    dim3 grid(z.tiles_x * z.tiles_y * n, up.cout / 32);
    fh_launch_prof(1, dec_zconv4_kernel<T>, grid, dim3(256), 17 * 17 * RB + 9 * 32 * RB, cx.st, z);
  } else {
    const DecLaunch plain{tn, nullptr, cx.st};  // the generic kernel carries no copy
    for (int pu = 0; pu < 2; ++pu)
      for (int pv = 0; pv < 2; ++pv)
        if ((rc = launch_conv<T>(plain, ConvGeom::up_class(Ri, pu, pv), up, x_in, Zb, n, demod, Rows{}, sat))) return rc;
  }
  // FIR blur + bias + lrelu, scaled by the consumer's style
  const size_t tot = (size_t)n * (R / 2) * (R / 4) * (up.cout / 8);
  hipLaunchKernelGGL((dec_blur_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, cx.st, reinterpret_cast<const E*>(Zb),
                     reinterpret_cast<E*>(U), n, R, up.cout, up.abias, snext.p, snext.ld, sat, up.fir[0], up.fir[1], up.fir[2], up.fir[3]);
  *U_out = U;
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// What a level's flow launch takes from the Level itself; the caller adds x, the pyramids, snext / xnext, the final output
// and oflow.  styles: [F][ld_s], ToFlow's modulation at L.style_off.
inline FlowArgs flow_args_of(const Level& L, const float* styles, int ld_s, int F) {
  FlowArgs g;
  memset(&g, 0, sizeof(g));
  g.feat = L.feat;
  memcpy(g.upk_flow, L.upk_flow, sizeof(g.upk_flow));
  memcpy(g.upk_rgb, L.upk_rgb, sizeof(g.upk_rgb));
  g.wflow = L.wflow, g.bflow = L.bflow;
  g.sflow = styles + L.style_off, g.ld_s = ld_s;
  g.wrgb = L.wrgb, g.grgb = L.grgb;
  g.b1 = L.b1, g.b2 = L.b2, g.lin = L.lin;
  g.F = F, g.R = L.R, g.C = L.C;
  return g;
}

// dec_flowlast_kernel's I420 instantiation covers 2 rows x 128 columns per workgroup
inline bool flowlast_takes_i420(int R) { return R >= 128 && R % 128 == 0; }

// I420 frames from `n` finished 8-bit RGB frames of R x R (dec_rgb8_to_i420_kernel), behind the level that rendered them.
inline int launch_rgb8_to_i420(const DecLaunch& cx, const unsigned char* rgb, void* out, int n, int R, const FhYuv& yuv) {
  FH_REQUIRE(R % 8 == 0, "I420 frames: %d px is not a multiple of 8", R);
  const size_t lanes = (size_t)n * (R / 2) * (R / 8);
  hipLaunchKernelGGL(dec_rgb8_to_i420_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, cx.st, rgb,
                     static_cast<unsigned char*>(out), n, R, yuv);
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// ToFlow + warp + blend + ToRGB of one level (dec_flow_kernel); g holds everything but the grid.
// Grid: ~2048 workgroups in total (8 per CU) so that every lane group runs many pixel iterations and the per-workgroup
// prologue (56 per-lane weight values) is amortised; one row of workgroups per frame.
template <class T>
int launch_flow(const DecLaunch& cx, FlowArgs g) {
  const DecTune& tn = cx.tn;
  if (g.oflow) {  // one lane per pixel (dec_flowlast_kernel)
    const int runs = (g.R * g.R + 255) / 256;
    g.ct = cx.take(g.R, kRideFlow);
    FH_REQUIRE(g.final_mode != kOutU8 || (g.R * g.R) % 256 == 0, "8-bit frames: %d x %d pixels are not whole runs of 256", g.R, g.R);
    FH_REQUIRE(g.final_mode != kOutI420 || flowlast_takes_i420(g.R), "I420 frames: %d px is not whole blocks of 128 columns", g.R);
    void (*kern)(FlowArgs);
    switch (g.final_mode) {
      case kOutU8: kern = dec_flowlast_kernel<T, true>; break;
      case kOutI420: kern = dec_flowlast_kernel<T, false, true>; break;
      default: kern = dec_flowlast_kernel<T>;
    }
    hipLaunchKernelGGL(kern, dim3(runs * g.F + g.ct.nwg), dim3(256), (size_t)tn.lds_pad, cx.st, g);
    FH_CHECK_HIP(hipGetLastError());
    return FLOAT_OK;
  }
  const int R = g.R, n = g.F;
  const int lpp = g.C / 8, gpb = 256 / lpp;
  const int pix = (tn.flow_pix == 1 || tn.flow_pix == 2 || tn.flow_pix == 4) ? tn.flow_pix : (lpp <= 8 ? 4 : 2);
  const int step = gpb * pix;  // pixels one workgroup covers per iteration
  const int max_bx = (R * R + step - 1) / step;
  int bx = std::max(1, std::min(max_bx, (tn.flow_wgs + n - 1) / n));
  if (bx >= 8) bx &= ~7;  // bands in multiples of 8: band <-> XCD affinity (dec_flow_kernel)
  g.band_pix = ((R * R + bx - 1) / bx + step - 1) / step * step;
  g.nbands = bx = (R * R + g.band_pix - 1) / g.band_pix;
  g.ct = cx.take(R, kRideFlow);
  // dynamic LDS only as an occupancy cap (FLOAT_DEC_LDS_PAD); the kernel's own 14 KB are static
  const size_t pad = tn.lds_pad > 14 * 1024 ? (size_t)tn.lds_pad - 14 * 1024 : 0;
  const dim3 grid(bx * n + g.ct.nwg);
  for_each_flow<T>([&](auto kern, int kpix, bool klast) {
    if (kpix == pix && klast == !g.xnext) hipLaunchKernelGGL(kern, grid, dim3(256), pad, cx.st, g);
  });
  FH_CHECK_HIP(hipGetLastError());
  return FLOAT_OK;
}

// The modulation table and what the style launches write (the handle's, or a unit operator's own)
struct StyleTable {
  float *WmT, *bm;  // [style_dim][Stot] k-major, [Stot] (upload_mod_table)
  int Stot, Dtot;
  float *styles, *eps, *demod;  // [F][Stot], [F][16], [F][Dtot]
};

// styles = EqualLinear(r_d + s_r) of every modulation row for F frames (s_r may be nullptr): style @ (W / sqrt(sdim))^T + b
// (styledecoder.py:229,241)
inline void launch_style_gemm(const StyleTable& t, const float* r_d, const float* s_r, int sdim, int F, hipStream_t st) {
  constexpr int FB = 8;
  dim3 grid((t.Stot + 255) / 256, (F + FB - 1) / FB);
  hipLaunchKernelGGL((dec_small_gemm_kernel<SG_STYLE, FB>), grid, dim3(256), FB * sdim * sizeof(float), st, r_d, sdim, s_r, t.WmT, sdim,
                     t.Stot, t.bm, 1.0f / sqrtf((float)sdim), t.styles, t.Stot, F);
}

// Every style modulation and every demod factor of `convs` for F frames: style GEMM + 2 launches.
inline int launch_styles(const StyleTable& t, const Styled* convs, size_t nconv, const float* r_d, const float* s_r, int sdim, int F,
                         bool normalise, unsigned long long* sat, hipStream_t st) {
  constexpr int FB = 8;
  launch_style_gemm(t, r_d, s_r, sdim, F, st);
  DemodArgs d;
  memset(&d, 0, sizeof(d));
  int maxc = 0, maxcin = 0;
  FH_REQUIRE(nconv <= 16, "too many styled convs");
  for (size_t i = 0; i < nconv; ++i) {
    d.L[i] = {convs[i].WsqT, convs[i].cin, convs[i].cout, convs[i].style_off, convs[i].demod_off};
    maxc = std::max(maxc, convs[i].cout);
    maxcin = std::max(maxcin, convs[i].cin);
  }
  d.styles = t.styles, d.ld_s = t.Stot;
  d.demod = t.demod, d.ld_d = t.Dtot;
  d.eps = t.eps;
  d.F = F;
  d.normalise = normalise ? 1 : 0;
  d.sat = sat;
  // every StyledConv's style divided by its max |s| per frame, eps / max^2 left for the demodulation (dec_kernels.hpp)
  hipLaunchKernelGGL(dec_style_norm_kernel, dim3((unsigned)nconv, F), dim3(256), 0, st, d);
  dim3 g2((maxc + 255) / 256, (F + FB - 1) / FB, (unsigned)nconv);
  hipLaunchKernelGGL((dec_demod_all_kernel<FB>), g2, dim3(256), FB * maxcin * sizeof(float), st, d);
  return FLOAT_OK;
}

}  // namespace
